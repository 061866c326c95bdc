#!/usr/bin/env python3
"""Cost of the weight average (EMA) fused into the AdamW update (FusedAdamW.set_ema).

    python tools/ema_bench.py [--sizes 1902848,174000000] [--batch 256] [--rounds 6] [--steps 10] [--regimes lora,full_ft]

In one process, variants alternated round by round, every shape warmed first:

(a) the optimizer update alone on flat f32 buffers of ``--sizes`` elements (the LoRA I+D+T configuration's trainable floats and about
    full fine-tuning's): ``off`` = ``adamw_step_dev``, ``fused`` = ``adamw_step_ema``, ``unfused`` = ``adamw_step_dev`` followed by
    ``torch.Tensor.lerp_`` of the average towards the flat parameters.  Device events around blocks of back-to-back launches sized to
    about 0.1 s each, ``--rounds`` blocks per variant.
(b) the graphed I+D+T training step at local batch ``--batch``, for the LoRA configuration and for full fine-tuning
    (``disable_lora: true``), the average off against on, as tools/grad_clip_bench.py times its option: interleaved blocks of
    ``--steps`` replays, ``--rounds`` blocks per variant.  ``--regimes ""`` runs part (a) only.

Writes profiles/ema_bench.json (--out) and prints it."""
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

HP = (0.9, 0.999, 1e-8, 0.01)
DECAY = 0.999
BYTES = {"off": 28, "fused": 36, "unfused": 40}     # per element: p, m, v read + written and g read; + ema read + written; + p re-read


def _block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _summary(blocks):
    return {"ms": round(statistics.median(blocks), 5), "blocks_ms": [round(x, 5) for x in blocks],
            "spread_ms": round(max(blocks) - min(blocks), 5)}


def update_alone(n, rounds, device):
    from bioscanclip.hip import ops
    gen = torch.Generator(device=device).manual_seed(n % 1000)
    p = torch.randn(n, device=device, generator=gen)
    g = torch.randn(n, device=device, generator=gen) * 1e-2
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    hyper = torch.zeros(2, dtype=torch.int32, device=device)
    hyper.view(torch.float32)[0:1].fill_(1e-6)
    hyper[1:2].fill_(100000)             # past the warm-up: w = 1 - decay
    w = 1.0 - DECAY

    def unfused():
        ops.adamw_step_dev(p, g, m, v, hyper, *HP)
        ema.lerp_(p, w)
    variants = {"off": lambda: ops.adamw_step_dev(p, g, m, v, hyper, *HP),
                "fused": lambda: ops.adamw_step_ema(p, g, m, v, ema, hyper, None, *HP, DECAY, True),
                "unfused": unfused}
    for fn in variants.values():
        _block(fn, 5)
    reps = max(5, min(10000, int(100.0 / max(_block(variants["unfused"], 5), 1e-3))))     # about 0.1 s per block
    blocks = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            blocks[k].append(_block(fn, reps))
    out = {"elements": n, "launches_per_block": reps, "timed_launches_each": reps * rounds}
    for k in variants:
        out[k] = _summary(blocks[k])
        out[k]["gbytes_per_s_at_%d_bytes_per_element" % BYTES[k]] = round(BYTES[k] * n / out[k]["ms"] / 1e6, 1)
    out["fused_over_off"] = round(out["fused"]["ms"] / out["off"]["ms"], 4)
    out["fused_over_unfused"] = round(out["fused"]["ms"] / out["unfused"]["ms"], 4)
    return out


def graphed_step(B, rounds, steps_per_block, device, full_ft):
    import bench
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    image, dna, text = bench.synthetic_batch(B, True, device, seed=4321)
    label = torch.arange(B, device=device)
    steps = {}
    for on in (False, True):
        model = bench.build_model(True, device, full_ft=full_ft)
        model.train()
        opt = FusedAdamW(model.parameters(), lr=1e-6 if full_ft else 1e-3, ema_decay=DECAY if on else None)
        g = GraphedStep(model, opt, ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07), warmup=2)
        for _ in range(6):      # two eager steps, the capture (+ its replay), three more replays
            g(image, dna, text, label)
        steps[on] = (g, opt)
    torch.cuda.synchronize()
    blocks = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            g = steps[on][0]
            blocks[on].append(_block(lambda: g(image, dna, text, label), steps_per_block))
    opt = steps[True][1]
    off, on = _summary(blocks[False]), _summary(blocks[True])
    return {"batch": B, "steps_per_block": steps_per_block, "timed_steps_each": rounds * steps_per_block, "off": off, "on": on,
            "delta_ms": round(on["ms"] - off["ms"], 5), "trainable_floats": [f.data.numel() for f in opt._flats if f.valid()],
            "effective_decay": opt.ema_effective_decay()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1902848,174000000")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regimes", default="lora,full_ft")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    result = {"tool": "tools/ema_bench.py", "ema_decay": DECAY, "rounds": a.rounds, "bytes_per_element": BYTES}
    if not torch.cuda.is_available():
        result["timing"] = "not measured (no GPU)"
        print(json.dumps(result))
        return
    device = torch.device("cuda", 0)
    result["update_alone"] = [update_alone(int(n), a.rounds, device) for n in a.sizes.split(",") if n]
    torch.cuda.empty_cache()
    result["graphed_step"] = {}
    for regime in [r for r in a.regimes.split(",") if r]:
        result["graphed_step"][regime] = graphed_step(a.batch, a.rounds, a.steps, device, regime == "full_ft")
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
