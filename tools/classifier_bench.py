"""Supervised fine-tuning head: forward + backward time of the fused HIP head (split-bf16 logits GEMM, bsclip_ce_fwd_bwd, the three
backward products) next to torch's f32 ``F.linear`` + ``F.cross_entropy`` forward + backward on the same GPU, at (B, C) = (256, 1213)
and (256, 8192); then one eager fine-tuning step (image + DNA classifiers, B = 256, C = 1213) next to the eager Image+DNA contrastive
step on the same model.

Warm-up first (code objects, algorithm selection), then ROUNDS rounds that alternate the two sides, each round timing ITERS
back-to-back calls with device events; the median over the rounds and their spread (min .. max) are printed, and one JSON line.

    python tools/classifier_bench.py [--rounds 7] [--iters 50] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bioscan-clip_amd")]
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(sides, rounds, iters, warmup=5):
    """{name: [ms per call, one per round]} with the sides alternating inside every round."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(timed(fn, iters))
    return out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def head_bench(B, C, rounds, iters):
    from bioscanclip.hip import functional as HF
    g = torch.Generator().manual_seed(C)
    z = torch.randn(B, 768, generator=g).cuda()
    t = torch.randint(0, C, (B,), generator=g).cuda()
    lin_h, lin_t = nn.Linear(768, C).cuda(), nn.Linear(768, C).cuda()
    lin_t.load_state_dict(lin_h.state_dict())
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def hip():
        zc = z.detach().requires_grad_(True)
        lin_h.weight.grad = lin_h.bias.grad = None
        HF.linear_cross_entropy(zc, lin_h.weight, lin_h.bias, t, flag=flag).backward()

    def torch_f32():
        zc = z.detach().requires_grad_(True)
        lin_t.weight.grad = lin_t.bias.grad = None
        F.cross_entropy(F.linear(zc, lin_t.weight, lin_t.bias), t).backward()

    r = alternate({"hip": hip, "torch_f32": torch_f32}, rounds, iters)
    return {k: stats(v) for k, v in r.items()}


def step_bench(B, C, rounds, iters):
    import bench
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    from bioscanclip.util.util import EncoderWithExtraLayer
    dev = torch.device("cuda", 0)
    model = bench.build_model(False, dev)
    image, dna, _ = bench.synthetic_batch(B, False, dev, 5)
    label = torch.arange(B, device=dev)
    target = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(3)).to(dev)
    img = EncoderWithExtraLayer(model.image_encoder, nn.Linear(768, C)).to(dev)
    dn = EncoderWithExtraLayer(model.dna_encoder, nn.Linear(768, C)).to(dev)
    holder = nn.ModuleList([img, dn])
    holder.train()
    opt_ft = FusedAdamW([p for p in holder.parameters() if p.requires_grad], lr=1e-3)
    opt_cl = FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    crit = ContrastiveLoss(criterion=nn.CrossEntropyLoss(), logit_scale=1 / 0.07)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def fine_tune():
        opt_ft.zero_grad()
        (img.loss(image, target, flag=flag) + dn.loss(dna, target, flag=flag)).backward()
        if opt_ft.needs_attach():
            opt_ft.attach(holder)
        opt_ft.step()

    def contrastive():
        opt_cl.zero_grad()
        crit(*model(image, dna, None), label).backward()
        if opt_cl.needs_attach():
            opt_cl.attach(model)
        opt_cl.step()

    r = alternate({"fine_tune_step": fine_tune, "contrastive_step_eager": contrastive}, rounds, iters, warmup=2)
    return {k: stats(v) for k, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "classifier_bench needs a GPU"
    out = {"gpu": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "head": {}}
    for B, C in ((256, 1213), (256, 8192)):
        r = head_bench(B, C, a.rounds, a.iters)
        out["head"][f"{B}x{C}"] = r
        print(f"head fwd+bwd B={B} C={C}: hip {r['hip']['median_ms']:.4f} ms ({r['hip']['min_ms']:.4f} .. {r['hip']['max_ms']:.4f})   "
              f"torch f32 {r['torch_f32']['median_ms']:.4f} ms ({r['torch_f32']['min_ms']:.4f} .. {r['torch_f32']['max_ms']:.4f})", flush=True)
    if not a.no_step:
        r = step_bench(256, 1213, max(3, a.rounds // 2), 5)
        out["step"] = r
        for k, v in r.items():
            print(f"{k} B=256: {v['median_ms']:.2f} ms ({v['min_ms']:.2f} .. {v['max_ms']:.2f})", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
