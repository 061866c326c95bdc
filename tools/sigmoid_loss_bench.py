#!/usr/bin/env python3
"""The sigmoid loss entry against the InfoNCE entry with a learnable scale, call for call.

    python tools/sigmoid_loss_bench.py [--rounds 6] [--out profiles/sigmoid_loss_bench.json]

Times ``bsclip_sigmoid_loss_fwd_bwd`` against ``bsclip_infonce_fwd_bwd_ts`` (forward + backward, all rows own rows) on the same inputs
in one process at N = 256, 1024 and 4096 with 2 and 3 modalities.  Inputs are in the trained regime (z_m = base + 0.5 noise_m, labels
arange(N) // 3 * 3).  Two timings per entry, both with device events after untimed warm-up calls, in blocks that alternate between the
two entries round by round:
  graph: a captured graph of ``calls`` back-to-back calls, replayed -- the kernels with the launch gaps of a captured training step;
  eager: the same calls enqueued from Python through ctypes -- the host's launch rate is part of it at small N.
Outputs of the two entries are not compared (they are different losses); each entry's loss is recorded so that a run can be told
from another.  The launch counts are those of the launch sequences in csrc/loss.hip for the form each entry takes at that size.
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

SLAB = 1024          # SLAB_ROWS of csrc/loss.hip
CALLS = {256: 100, 1024: 50, 4096: 10}


def launches(N, nmod):
    """Kernel launches per call (forward + backward), from the sequences in csrc/loss.hip."""
    Np = (N + 255) // 256 * 256
    ndir, nu, S = nmod * (nmod - 1), nmod * (nmod - 1) // 2, (N + SLAB - 1) // SLAB
    if Np <= SLAB:   # batched: every stage one launch over all modalities / pairs
        sig = {"form": "batched", "prep": 1, "transpose_split": 1, "logits_gemm": 1, "row_reduce": 1, "final": 1, "w": 1,
               "dz_gemm": nmod - 1, "l2norm_bwd": 1}
        nce = {"form": "batched", "scale": 1, "prep": 1, "transpose_split": 1, "count": 1, "logits_gemm": 1, "row_reduce": 1,
               "final": 1, "w": 1, "dz_gemm": nmod - 1, "l2norm_bwd": 1}
    else:
        sig = {"form": "slab", "prep": nmod, "transpose_split": nmod, "logits_gemm": nu * S + ndir * S, "row_reduce": nu * S,
               "final": 1, "w": ndir * S, "dz_gemm": ndir * S, "l2norm_bwd": nmod}
        if Np >= 2048:   # InfoNCE's default above 2 048 padded rows: the fused epilogues, no logits in memory
            nce = {"form": "fused", "scale": 1, "prep": nmod, "transpose_split": nmod, "count": 1, "lse_gemm": ndir, "combine": ndir,
                   "final": 1, "w_gemm": ndir * S, "dz_gemm": ndir * S, "l2norm_bwd": nmod}
        else:
            nce = {"form": "slab", "scale": 1, "prep": nmod, "transpose_split": nmod, "count": 1, "logits_gemm": 2 * ndir * S,
                   "row_reduce": ndir * S, "final": 1, "w": ndir * S, "dz_gemm": ndir * S, "l2norm_bwd": nmod}
    for d in (sig, nce):
        d["total"] = sum(v for v in d.values() if isinstance(v, int))
    return sig, nce


def timed(fn, calls, graph):
    """ms per call of one block of ``calls`` calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if graph is not None:
        graph.replay()
    else:
        for _ in range(calls):
            fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigmoid_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sigmoid_loss_bench.py needs a GPU: nothing is measured without one")
    from bioscanclip.hip import ops
    dev = torch.device("cuda", 0)
    F32 = torch.float32
    result = {"tool": "tools/sigmoid_loss_bench.py", "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
              "t_b_sigmoid": [math.log(10.0), -10.0], "t_infonce": math.log(1 / 0.07), "cases": []}
    for N in (256, 1024, 4096):
        for nmod in (2, 3):
            g = torch.Generator().manual_seed(3000 + N + nmod)
            base = torch.randn(N, 768, generator=g)
            zs = [(base + 0.5 * torch.randn(N, 768, generator=g)).to(dev) for _ in range(nmod)]
            labels = (torch.arange(N) // 3 * 3).to(dev)
            ws = torch.empty(ops.infonce_workspace_floats(N, nmod), dtype=F32, device=dev)
            dzs = [torch.empty(N, 768, dtype=F32, device=dev) for _ in range(nmod)]
            loss_s, loss_n = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
            aux, so = torch.zeros(4, device=dev), torch.zeros(2, device=dev)
            t_s = torch.tensor([math.log(10.0)], device=dev)
            b_s = torch.tensor([-10.0], device=dev)
            t_n = torch.tensor([math.log(1 / 0.07)], device=dev)
            fns = {"sigmoid": lambda: ops.sigmoid_loss_fwd_bwd(zs, labels, t_s, b_s, loss_s, dzs, aux, workspace=ws),
                   "infonce_ts": lambda: ops.infonce_fwd_bwd_ts(zs, labels, t_n, loss_n, dzs, so, workspace=ws)}
            calls = CALLS[N]
            graphs = {}
            side = torch.cuda.Stream()
            for name, fn in fns.items():
                for _ in range(5):          # untimed: code objects loaded, every shape seen
                    fn()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=side):
                    for _ in range(calls):
                        fn()
                gr.replay()                 # untimed first replay
                graphs[name] = gr
            torch.cuda.synchronize()
            blocks = {(n, k): [] for n in fns for k in ("graph", "eager")}
            for _ in range(a.rounds):
                for kind in ("graph", "eager"):
                    for name, fn in fns.items():
                        blocks[(name, kind)].append(timed(fn, calls, graphs[name] if kind == "graph" else None))
            sig_l, nce_l = launches(N, nmod)
            case = {"N": N, "nmod": nmod, "calls_per_block": calls, "launches": {"sigmoid": sig_l, "infonce_ts": nce_l},
                    "loss": {"sigmoid": loss_s.item(), "infonce_ts": loss_n.item()}}
            for kind in ("graph", "eager"):
                s, n = blocks[("sigmoid", kind)], blocks[("infonce_ts", kind)]
                case[kind] = {"sigmoid_us": round(1e3 * statistics.median(s), 2), "infonce_ts_us": round(1e3 * statistics.median(n), 2),
                              "ratio_sigmoid_over_infonce": round(statistics.median(s) / statistics.median(n), 4),
                              "blocks_sigmoid_us": [round(1e3 * x, 2) for x in s], "blocks_infonce_ts_us": [round(1e3 * x, 2) for x in n]}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del graphs, ws, dzs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)


if __name__ == "__main__":
    main()
