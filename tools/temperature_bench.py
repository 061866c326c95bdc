#!/usr/bin/env python3
"""Cost of the learnable temperature (model_config.trainable_temperature) on the captured training step.

    python tools/temperature_bench.py [--batch 256] [--rounds 6] [--steps 10]

Times the graphed I+D and I+D+T step at local batch 256 with the fixed scale and with ``model.logit_scale`` trained, interleaved
(round by round: off, on, off, on ...), device events around each block of ``--steps`` replays after warm-up, ``--rounds`` blocks per
variant (>= 50 timed steps each).  Also counts what the option adds per step without a GPU: the optimizer step of the 4-float buffer
through tests/launch_trace.py's recorder, the loss wrappers by name (the recorder takes no pointer arrays), and the kernel launches
behind them.  Writes profiles/temperature_bench.json (--out) and prints it."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bioscan-clip_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def added_calls():
    """C-ABI calls of the loss and of the temperature's optimizer step, fixed scale vs learnable, recorded on CPU tensors."""
    from launch_trace import recording
    from bioscanclip.hip import functional
    from bioscanclip.hip.dist import flat_buffers
    from bioscanclip.hip.engine import FlatParams
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.simple_clip import SimpleCLIP
    from bioscanclip.hip import ops
    out, loss_calls = {}, []
    saved = ops.infonce_fwd_bwd, ops.infonce_fwd_bwd_ts
    with recording() as rec:
        try:
            # the recorder takes no pointer arrays: the two loss wrappers are counted by name, one C-ABI call each
            ops.infonce_fwd_bwd = lambda *a, **k: loss_calls.append("bsclip_infonce_fwd_bwd")
            ops.infonce_fwd_bwd_ts = lambda *a, **k: loss_calls.append("bsclip_infonce_fwd_bwd_ts")
            functional._WS.clear()
            zs = [torch.zeros(8, 768, requires_grad=True) for _ in range(2)]
            labels = torch.arange(8)
            functional.infonce(zs, labels, 1 / 0.07).backward()
            out["loss_calls_fixed"], loss_calls = loss_calls, []
            model = SimpleCLIP(None, None, None)
            model.logit_scale = torch.nn.Parameter(torch.tensor(math.log(1 / 0.07)))
            model._temperature_flat = FlatParams([model.logit_scale], torch.device("cpu"))
            functional.infonce(zs, labels, model.logit_scale).backward()
            out["loss_calls_trainable"] = loss_calls
            rec.reset()
            opt = FusedAdamW(model.parameters(), lr=1e-3)
            opt.attach(model)
            assert len(flat_buffers(model)) == 1
            opt.step()
            out["optimizer_calls_added"] = [n for n, _ in rec.calls]
        finally:
            ops.infonce_fwd_bwd, ops.infonce_fwd_bwd_ts = saved
            functional._WS.clear()
    out["c_abi_calls_added_per_step"] = len(out["loss_calls_trainable"]) - len(out["loss_calls_fixed"]) + len(out["optimizer_calls_added"])
    # inside bsclip_infonce_fwd_bwd_ts: loss_scale_kernel ahead of the section; every other kernel replaces its by-value twin one for one
    out["kernel_launches_added_per_step"] = {"loss_section": 1, "adamw": len(out["optimizer_calls_added"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temperature_bench.json"))
    a = ap.parse_args()
    result = {"tool": "tools/temperature_bench.py", "batch": a.batch, "rounds": a.rounds, "steps_per_block": a.steps}
    result["launches"] = added_calls()
    if not torch.cuda.is_available():
        result["timing"] = "not measured (no GPU)"
        print(json.dumps(result))
        return
    import bench
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    device = torch.device("cuda", 0)
    B = a.batch
    timing = {}
    for with_text in (False, True):
        name = "I+D+T" if with_text else "I+D"
        image, dna, text = bench.synthetic_batch(B, with_text, device, seed=4321)
        label = torch.arange(B, device=device)
        steps = {}
        for trainable in (False, True):
            model = bench.build_model(with_text, device)
            if trainable:
                model.logit_scale = torch.nn.Parameter(torch.tensor(math.log(1 / 0.07), device=device))
            model.train()
            opt = FusedAdamW(model.parameters(), lr=1e-3)
            crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), model.logit_scale if trainable else 1 / 0.07)
            g = GraphedStep(model, opt, crit, warmup=2)
            for _ in range(6):      # two eager steps, the capture (+ its replay), three more replays
                g(image, dna, text, label)
            steps[trainable] = (g, crit)
        torch.cuda.synchronize()
        blocks = {False: [], True: []}
        for _ in range(a.rounds):
            for trainable in (False, True):
                g, _ = steps[trainable]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    g(image, dna, text, label)
                e1.record()
                e1.synchronize()
                blocks[trainable].append(e0.elapsed_time(e1) / a.steps)
        off, on = blocks[False], blocks[True]
        timing[name] = {"ms_per_step_fixed": round(statistics.median(off), 4), "ms_per_step_trainable": round(statistics.median(on), 4),
                        "blocks_fixed": [round(x, 4) for x in off], "blocks_trainable": [round(x, 4) for x in on],
                        "delta_ms": round(statistics.median(on) - statistics.median(off), 4),
                        "spread_fixed_ms": round(max(off) - min(off), 4), "spread_trainable_ms": round(max(on) - min(on), 4),
                        "timed_steps_each": a.rounds * a.steps,
                        "logit_scale_after": round(steps[True][1].current_scale().item(), 6)}
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
