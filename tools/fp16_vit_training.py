"""Measure the image tower's fp16-operand training (set_operand_format(model, "fp16", towers=("image",))); nothing is gated here.

  scale  per backward site of the ViT (tests/test_20's vit_L12 weights, inputs and unit-sized cotangents, and one B = 256 I+D+T InfoNCE
         step): the largest scaled |gradient| (units of 2^FP16_GRAD_SCALE_LOG2) and the share of non-zero values below 2^-14, fp16's
         smallest normal -- what the static scale is chosen from (>= 2^4 of headroom under 65 504)
  time   the graphed I+D and I+D+T step at B = 256, image tower fp16 against bf16, interleaved A/B rounds on one box
  kern   a few eager B = 256 I+D steps in one format (run under rocprofv3 --kernel-trace --stats to compare the kernels)
Records (one JSON object per line, with the tree hash and the date) are appended to --out (default r08_fp16_vit_training.jsonl in the
current directory).
    python tools/fp16_vit_training.py scale|time|kern [--fmt fp16|bf16] [--rounds N] [--steps K] [--out FILE]
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bioscan-clip_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from oracle import synth  # noqa: E402

OUT = "r08_fp16_vit_training.jsonl"   # set from --out


def _stamp(rec):
    try:
        tree = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        tree = ""
    if not tree and os.path.exists(os.path.join(ROOT, "tools", "scripts", ".tree")):
        tree = open(os.path.join(ROOT, "tools", "scripts", ".tree")).read().strip()
    rec.update(tree=tree or "unknown", date=datetime.date.today().isoformat())
    if os.path.dirname(OUT):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def _clip(with_text, seed=101):
    from test_20_encoders_gpu import _build_clip
    model, _ = _build_clip(with_text, seed)
    return model.to("cuda").train()


class _Sites:
    def __init__(self):
        self.amax = defaultdict(float)
        self.small = defaultdict(int)
        self.nz = defaultdict(int)

    def __call__(self, site, t):
        a = t.float().abs()
        self.amax[site] = max(self.amax[site], float(a.max()))
        nz = a[a > 0]
        self.small[site] += int((nz < 2.0 ** -14).sum())
        self.nz[site] += int(nz.numel())

    def record(self, what):
        from bioscanclip.hip.engine import ViTEngine
        s = ViTEngine.FP16_GRAD_SCALE_LOG2
        worst = max(self.amax.values())
        return {"what": what, "grad_scale_log2": s, "headroom_log2": round(float(torch.tensor(65504.0 / worst).log2()), 2),
                "sites": {k: {"scaled_amax": self.amax[k], "below_2^-14_share": self.small[k] / max(1, self.nz[k])} for k in self.amax}}


def scale():
    from bioscanclip.hip.engine import ViTEngine, set_operand_format
    from test_27_fp16_vit_training_gpu import _vit
    from bioscanclip.model.loss_func import ContrastiveLoss
    m, _, x, _ = _vit(12)
    w = synth.synth_tensor("vit.cot.12", (2, 768), seed=5).cuda()
    set_operand_format(m, "fp16")
    sites = _Sites()
    ViTEngine.grad_probe = staticmethod(sites)
    try:
        (m(x) * w).sum().backward()
        torch.cuda.synchronize()
        _stamp(sites.record("vit_L12 at test_20's cotangents (B = 2)"))
        model = _clip(True)
        set_operand_format(model, "fp16", towers=("image",))
        crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
        image, dna, text, label = synth.synth_batch(256, seed=77, with_text=True)
        sites = _Sites()
        ViTEngine.grad_probe = staticmethod(sites)
        crit(*model(image.cuda(), dna.cuda(), {k: v.cuda() for k, v in text.items()}), label.cuda()).backward()
        torch.cuda.synchronize()
        _stamp(sites.record("B = 256 I+D+T InfoNCE step"))
    finally:
        ViTEngine.grad_probe = None


def _graphed(with_text, fmt):
    from bioscanclip.hip.engine import set_operand_format
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    model = _clip(with_text)
    set_operand_format(model, fmt, towers=("image",))
    opt = FusedAdamW(model.parameters(), lr=1e-5)
    opt.enable_device_hyper(True)
    g = GraphedStep(model, opt, ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07), warmup=2)
    image, dna, text, label = synth.synth_batch(256, seed=5, with_text=with_text)
    batch = (image.cuda(), dna.cuda(), None if text is None else {k: v.cuda() for k, v in text.items()}, label.cuda())
    for _ in range(4):
        g(*batch)
    torch.cuda.synchronize()
    return g, batch


def _time(g, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g(*batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def timing(rounds, steps):
    for with_text in (False, True):
        runs = {fmt: _graphed(with_text, fmt) for fmt in ("bf16", "fp16")}
        ms = defaultdict(list)
        for _ in range(rounds):          # interleaved A / B
            for fmt in ("bf16", "fp16"):
                ms[fmt].append(_time(*runs[fmt], steps))
        med = {f: sorted(v)[len(v) // 2] for f, v in ms.items()}
        _stamp({"what": f"graphed {'I+D+T' if with_text else 'I+D'} step, B = 256, image tower fp16 vs bf16", "ms_per_step": ms,
                "median_ms": med, "fp16_over_bf16": med["fp16"] / med["bf16"]})
        del runs
        torch.cuda.empty_cache()


def kern(fmt, steps):
    from bioscanclip.hip.engine import set_operand_format
    from bioscanclip.model.loss_func import ContrastiveLoss
    model = _clip(False)
    set_operand_format(model, fmt, towers=("image",))
    crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
    image, dna, _, label = synth.synth_batch(256, seed=5)
    image, dna, label = image.cuda(), dna.cuda(), label.cuda()
    for _ in range(steps):
        model.zero_grad(set_to_none=True)
        crit(*model(image, dna, None), label).backward()
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["scale", "time", "kern"])
    ap.add_argument("--fmt", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=OUT, help="JSON-lines file the records are appended to")
    a = ap.parse_args()
    OUT = a.out
    if a.what == "scale":
        scale()
    elif a.what == "time":
        timing(a.rounds, a.steps)
    else:
        kern(a.fmt, a.steps)
