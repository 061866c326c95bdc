#!/usr/bin/env python3
"""Cost of gradient-norm clipping / non-finite-step skipping (FusedAdamW.set_grad_clip) on the captured training step.

    python tools/grad_clip_bench.py [--batch 256] [--rounds 6] [--steps 10] [--regimes lora,full_ft]

Times the graphed I+D+T step at local batch 256 with the option off and on (``max_grad_norm=1.0``), for the LoRA configuration and for
full fine-tuning (``disable_lora: true``), interleaved in one process (round by round: off, on, off, on ...), device events around each
block of ``--steps`` replays after warm-up, ``--rounds`` blocks per variant.  Also records what the option launches per step without a
GPU (tests/launch_trace.py's recorder on three small flat buffers) and, per regime, the size of the flat gradient buffers the extra
pass reads and the time of that pass alone (20 back-to-back repetitions outside the step, device events).  Writes profiles/grad_clip_bench.json (--out) and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bioscan-clip_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def launch_lists():
    """C-ABI calls of one eager optimizer step over three flat buffers, option off vs on, recorded on CPU tensors."""
    from launch_trace import recording
    from bioscanclip.hip import ops
    from bioscanclip.hip.engine import FlatParams
    from bioscanclip.hip.optim import FusedAdamW
    out = {}
    saved = ops.grad_norm_partials
    for on in (False, True):
        groups = [[torch.nn.Parameter(torch.zeros(40, 8))], [torch.nn.Parameter(torch.zeros(()))], [torch.nn.Parameter(torch.zeros(100))]]
        opt = FusedAdamW([p for g in groups for p in g], lr=1e-3, max_grad_norm=1.0 if on else None, skip_nonfinite=on)
        opt._flats = [FlatParams(g, torch.device("cpu")) for g in groups]
        with recording() as rec:
            try:
                ops.grad_norm_partials = lambda n: 1     # the recorder's stand-in library answers every query with 0
                opt.step()
            finally:
                ops.grad_norm_partials = saved
        out["on" if on else "off"] = [n for n, _ in rec.calls]
    out["added_per_step"] = len(out["on"]) - len(out["off"])
    return out


def norm_pass_ms(opt, reps=20):
    """The norm pass alone (one grad_sumsq_partial per flat buffer + grad_clip_finish) on the optimizer's own gradient buffers, into a
    scratch record: device events around ``reps`` back-to-back passes after three warm-up passes."""
    from bioscanclip.hip import ops
    flats = [f for f in opt._flats if f.valid()]
    counts = [ops.grad_norm_partials(f.grad.numel()) for f in flats]
    partials = torch.empty(sum(counts), dtype=torch.float64, device=flats[0].grad.device)
    state = torch.zeros(ops.GRAD_CLIP_STATE_WORDS, dtype=torch.int32, device=flats[0].grad.device)

    def once():
        off = 0
        for f, c in zip(flats, counts):
            ops.grad_sumsq_partial(f.grad, partials[off:off + c])
            off += c
        ops.grad_clip_finish(partials, 1.0, state)
    for _ in range(3):
        once()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regimes", default="lora,full_ft")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_bench.json"))
    a = ap.parse_args()
    result = {"tool": "tools/grad_clip_bench.py", "batch": a.batch, "rounds": a.rounds, "steps_per_block": a.steps, "max_grad_norm": 1.0}
    result["launches"] = launch_lists()
    if not torch.cuda.is_available():
        result["timing"] = "not measured (no GPU)"
        print(json.dumps(result))
        return
    import bench
    from bioscanclip.hip import ops
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    device = torch.device("cuda", 0)
    B = a.batch
    timing = {}
    for regime in [r for r in a.regimes.split(",") if r]:
        full_ft = regime == "full_ft"
        image, dna, text = bench.synthetic_batch(B, True, device, seed=4321)
        label = torch.arange(B, device=device)
        steps = {}
        for on in (False, True):
            model = bench.build_model(True, device, full_ft=full_ft)
            model.train()
            opt = FusedAdamW(model.parameters(), lr=1e-6 if full_ft else 1e-3, max_grad_norm=1.0 if on else None, skip_nonfinite=on)
            crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
            g = GraphedStep(model, opt, crit, warmup=2)
            for _ in range(6):      # two eager steps, the capture (+ its replay), three more replays
                g(image, dna, text, label)
            steps[on] = (g, opt)
        torch.cuda.synchronize()
        blocks = {False: [], True: []}
        for _ in range(a.rounds):
            for on in (False, True):
                g, _ = steps[on]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    g(image, dna, text, label)
                e1.record()
                e1.synchronize()
                blocks[on].append(e0.elapsed_time(e1) / a.steps)
        off_ms, on_ms = blocks[False], blocks[True]
        opt = steps[True][1]
        floats = [f.grad.numel() for f in opt._flats if f.valid()]
        pass_ms = norm_pass_ms(opt)
        timing[regime] = {"ms_per_step_off": round(statistics.median(off_ms), 4), "ms_per_step_on": round(statistics.median(on_ms), 4),
                          "blocks_off": [round(x, 4) for x in off_ms], "blocks_on": [round(x, 4) for x in on_ms],
                          "delta_ms": round(statistics.median(on_ms) - statistics.median(off_ms), 4),
                          "spread_off_ms": round(max(off_ms) - min(off_ms), 4), "spread_on_ms": round(max(on_ms) - min(on_ms), 4),
                          "timed_steps_each": a.rounds * a.steps,
                          "flat_gradient_floats": floats, "flat_gradient_mbytes": round(4 * sum(floats) / 1e6, 3),
                          "partials": [ops.grad_norm_partials(n) for n in floats],
                          "norm_pass_alone_ms": round(pass_ms, 4), "norm_pass_alone_gbytes_per_s": round(4 * sum(floats) / pass_ms / 1e6, 1),
                          "grad_stats_on": opt.grad_stats()}
        del steps
        torch.cuda.empty_cache()
    result["timing"] = timing
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
