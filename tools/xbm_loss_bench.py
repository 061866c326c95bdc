#!/usr/bin/env python3
"""The cross-batch memory's cost: call for call beside the InfoNCE it extends, and on the whole captured default step.

    python tools/xbm_loss_bench.py [--rounds 6] [--step-blocks 5] [--parity-log FILE] [--out profiles/xbm_loss_bench.json]

calls   ``bsclip_infonce_xbm_fwd_bwd`` + ``bsclip_xbm_enqueue`` (one training step's share: the loss on a FULL bank, then the
        enqueue) against ``bsclip_infonce_fwd_bwd_ts`` at N = 256 in the same process, nmod 2 and 3, Q in 1024, 4096, 16384.  Each
        is timed as a captured graph of back-to-back calls, replayed, between two device events after untimed warm-up, in blocks
        that alternate between the two entries round by round.  ``product_tflops`` is the FLOPs of the call's products (the split
        logits and dz products, K = 3 x 768 and 3 x keys) over the WHOLE call's time: a lower bound on the rate of the product
        stages themselves, to be put against the step's GEMM rate.
step    ``bench.py``'s workload (its model, batch and labels, I+D+T at B = 256, one captured step) with ``ContrastiveLoss`` and with
        ``MemoryBankContrastiveLoss(memory_bank_size=4096)``, two models in one process, blocks of replayed steps alternating
        between them after the bank has filled; ms per step of every block and the difference of the medians.
parity  with ``--parity-log FILE`` (the GPU tests' parity log, one JSON record per line): the worst |hip - f64| / gate per quantity
        over the records tests/test_11_xbm_loss_gpu.py appended to it (those whose ``test`` begins with ``xbm_``).
Without a GPU the tool fails: there is nothing to time."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bioscan-clip_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

D = 768
CALLS = {1024: 50, 4096: 20, 16384: 8}


def launches(nmod):
    """Kernel launches per call at N = 256, from the sequence in csrc/loss_xbm.hip (the products batched over the pairs)."""
    runs = 2 if nmod == 2 else 4
    loss = {"prep": 1, "transpose_split": 1, "scrub": 1, "own_logits_gemm": 1, "bank_logits_gemm": 1, "row_stats": 1, "final": 1,
            "w": 1, "dz_own_gemm": nmod - 1, "dz_bank_splitk": 2 * runs, "l2norm_bwd": 1}
    loss["total"] = sum(loss.values())
    return {"infonce_xbm": loss, "xbm_enqueue": {"flags": 1, "decide": 1, "rows": 1, "columns": 1, "state": 1, "total": 5}}


def product_flops(N, Q, nmod):
    Np, P = (N + 255) // 256 * 256, nmod * (nmod - 1)
    logits = 2.0 * 3 * D * (P // 2 * N * Np + P * N * Q)
    dz = 2.0 * 3 * D * (P * N * Np + P * N * Q)
    return logits + dz


def timed(graph, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def bench_calls(rounds):
    from bioscanclip.hip import ops
    dev = torch.device("cuda", 0)
    F32 = torch.float32
    N = 256
    cases = []
    for nmod in (2, 3):
        for Q in (1024, 4096, 16384):
            g = torch.Generator().manual_seed(4000 + Q + nmod)
            base = torch.randn(N, D, generator=g)
            zs = [(base + 0.5 * torch.randn(N, D, generator=g)).to(dev) for _ in range(nmod)]
            labels = (torch.arange(N) // 3 * 3).to(dev)
            banks = [torch.zeros(ops.xbm_bank_floats(Q), dtype=F32, device=dev) for _ in range(nmod)]
            bank_labels = torch.zeros(Q, dtype=torch.int64, device=dev)
            state = torch.zeros(2, dtype=torch.int32, device=dev)
            ws = torch.empty(ops.xbm_workspace_floats(N, Q, nmod), dtype=F32, device=dev)
            for k in range(Q // N):          # a full bank of rows like the batch's, other labels
                ops.xbm_enqueue([z.roll(k + 1, 0) + 0.1 * k for z in zs], labels + 3 * N * (k % 2), banks, bank_labels, state, ws)
            torch.cuda.synchronize()
            assert state.tolist() == [0, Q]
            ws_n = torch.empty(ops.infonce_workspace_floats(N, nmod), dtype=F32, device=dev)
            dzs = [torch.empty(N, D, dtype=F32, device=dev) for _ in range(nmod)]
            loss_x, loss_n = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
            so_x, so_n = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
            t = torch.tensor([math.log(1 / 0.07)], device=dev)

            def xbm():
                ops.infonce_xbm(zs, labels, t, banks, bank_labels, state, loss_x, dzs, so_x, ws)
                ops.xbm_enqueue(zs, labels, banks, bank_labels, state, ws)

            fns = {"xbm": xbm, "infonce_ts": lambda: ops.infonce_fwd_bwd_ts(zs, labels, t, loss_n, dzs, so_n, workspace=ws_n)}
            calls = CALLS[Q]
            graphs = {}
            side = torch.cuda.Stream()
            for name, fn in fns.items():
                for _ in range(3):            # untimed: code objects loaded, every shape seen
                    fn()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=side):
                    for _ in range(calls):
                        fn()
                gr.replay()                   # untimed first replay
                graphs[name] = gr
            torch.cuda.synchronize()
            blocks = {n: [] for n in fns}
            for _ in range(rounds):
                for name in fns:
                    blocks[name].append(timed(graphs[name], calls))
            x, n = statistics.median(blocks["xbm"]), statistics.median(blocks["infonce_ts"])
            flops = product_flops(N, Q, nmod)
            case = {"N": N, "nmod": nmod, "Q": Q, "calls_per_block": calls, "launches": launches(nmod),
                    "workspace_MiB": round(ws.numel() * 4 / 2 ** 20, 1), "bank_MiB_per_modality": round(banks[0].numel() * 4 / 2 ** 20, 1),
                    "loss": {"xbm": loss_x.item(), "infonce_ts": loss_n.item()},
                    "xbm_loss_plus_enqueue_us": round(1e3 * x, 2), "infonce_ts_us": round(1e3 * n, 2),
                    "blocks_xbm_us": [round(1e3 * v, 2) for v in blocks["xbm"]],
                    "blocks_infonce_ts_us": [round(1e3 * v, 2) for v in blocks["infonce_ts"]],
                    "product_gflop": round(flops / 1e9, 2), "product_tflops_over_whole_call": round(flops / (x * 1e-3) / 1e12, 1)}
            cases.append(case)
            print(json.dumps(case), flush=True)
            del graphs, ws, banks, dzs
            torch.cuda.empty_cache()
    return cases


def bench_step(n_blocks, steps_per_block):
    """bench.py's default workload with and without the bank, alternating blocks of replayed steps."""
    import bench
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss, MemoryBankContrastiveLoss
    dev = torch.device("cuda", 0)
    B, Q = 256, 4096
    image, dna, text = bench.synthetic_batch(B, True, dev, seed=1234)
    label = torch.arange(B).to(dev)
    runs = {}
    for name in ("off", "on"):
        model = bench.build_model(True, dev)
        model.train()
        crit = (ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07) if name == "off" else
                MemoryBankContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07, memory_bank_size=Q))
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        step = GraphedStep(model, opt, crit, warmup=2)
        for _ in range(Q // B + 6):           # eager steps, the capture, replays: the bank is full before anything is timed
            loss = step(image, dna, text, label)
        torch.cuda.synchronize()
        assert step.graph is not None
        runs[name] = (step, crit, loss)
    assert int(runs["on"][1].filled()) == Q
    blocks = {"off": [], "on": []}
    for _ in range(n_blocks):
        for name in ("off", "on"):
            step = runs[name][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps_per_block):
                loss = step(image, dna, text, label)
            e1.record()
            e1.synchronize()
            blocks[name].append(e0.elapsed_time(e1) / steps_per_block)
            runs[name] = (step, runs[name][1], loss)
    off, on = statistics.median(blocks["off"]), statistics.median(blocks["on"])
    out = {"workload": "bench.py's I+D+T step at B = 256, one captured graph per criterion, blocks alternating off / on",
           "memory_bank_size": Q, "steps_per_block": steps_per_block,
           "ms_per_step_off_blocks": [round(v, 3) for v in blocks["off"]], "ms_per_step_on_blocks": [round(v, 3) for v in blocks["on"]],
           "ms_per_step_off": round(off, 3), "ms_per_step_on": round(on, 3), "added_ms": round(on - off, 3),
           "spread_off_ms": round(max(blocks["off"]) - min(blocks["off"]), 3),
           "final_loss": {k: v[2].item() for k, v in runs.items()}}
    print(json.dumps(out), flush=True)
    return out


def parity(path):
    if not path or not os.path.exists(path):
        return None
    recs = [r for r in (json.loads(ln) for ln in open(path) if ln.strip()) if str(r.get("test", "")).startswith("xbm_")]
    if not recs:
        return None
    out = {"cases": len(recs), "gates": {"loss_rel": 2e-5, "dz_rel": 2e-4, "dt": "(1 + 2 s) 2^-16 A"}}
    for k in ("loss_over_gate", "dz_over_gate", "dt_over_gate"):
        worst = max(recs, key=lambda r: r[k])
        out["worst_" + k] = {"ratio": worst[k], **{q: worst.get(q) for q in ("test", "N", "Q", "filled", "nmod", "t")}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--step-blocks", type=int, default=5, help="0 skips the whole-step measurement")
    ap.add_argument("--steps-per-block", type=int, default=20)
    ap.add_argument("--parity-log", default=None, help="the GPU tests' parity log (JSON lines); omitted: no parity section")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xbm_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/xbm_loss_bench.py needs a GPU: nothing is measured without one")
    result = {"tool": "tools/xbm_loss_bench.py", "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "calls": bench_calls(a.rounds)}
    if a.step_blocks > 0:
        result["step"] = bench_step(a.step_blocks, a.steps_per_block)
    result["parity"] = parity(a.parity_log)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)


if __name__ == "__main__":
    main()
