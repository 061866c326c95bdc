"""What would fp16 (instead of bf16) 16-bit operands buy, and which gradient scale keeps them in range?  (CPU only)

The rounding-aware oracle (oracle/refcpu.py, emulate_bf16=True) rounds every operand the HIP kernels round.  Here its rounding
function ``refcpu._q`` is replaced (monkeypatched, nothing under oracle/ is edited) by one that rounds through torch.float16: RNE,
subnormals kept, overflow to inf -- what v_cvt_f16_f32 does.  Unlike the emulation that quantified this first (forward roundings,
straight-through backward), the BACKWARD roundings are emulated too: at every activation rounding site (the "a" side of a GEMM, q / k
/ v / p, the LoRA t, the residual stream) the gradient flowing back through the operand is rounded as the kernels would store it,
scaled by the tower's static power of two, g -> fp16(g * 2^s) / 2^s.  Weight sites (".w") keep an f32 gradient: the kernels form
weight gradients in f32 (split-K GEMM, LoRA-gradient kernels), and frozen weights have none.

Per encoder (ViT depth 12, BarcodeBERT depth 12, text BERT depth 4; test_20's weights, inputs and cotangents) and per stream
setting (16-bit streams rounded to fp16 like the operands; f32 streams, refcpu.EMULATE_RESID_BF16 = False):
  * the embedding distance and the worst trainable-gradient distance to the plain f32 oracle (normwise relative L2), and the same
    for the bf16 emulation (today's default) for comparison;
  * per rounding site, the largest |value| of the forward operands and of the scaled gradients, and the share of non-zero values
    below 2^-14 (fp16's smallest normal);
  * the resolution of each emulation: the same rounding points evaluated with f64 instead of f32 accumulation.  Values near a
    rounding boundary flip with the accumulation order (and with the CPU's thread count), so an emulated distance is only defined to
    about this much -- for bf16 at depth 12 that is ~1e-2, which is why the bf16 rows move between machines.
The gradient scale s of a tower is chosen from an unscaled pass: the largest s that leaves the largest scaled gradient at least
2^4 below fp16's largest finite value (65504).
    python tools/fp16_sensitivity.py [vit|dna|txt|all]
"""
import math
import os
import sys
from collections import defaultdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bioscan-clip_amd"), os.path.join(ROOT, "tests")]
from bioscanclip.model import arch  # noqa: E402
from helpers import rel_err  # noqa: E402
from oracle import refcpu, synth  # noqa: E402

FP16_MAX = 65504.0
FP16_MIN_NORMAL = 2.0 ** -14
HEADROOM_LOG2 = 4
NODROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)

_orig_q = refcpu._q


class _Stats:
    def __init__(self):
        self.fwd_max = defaultdict(float)
        self.fwd_small = defaultdict(lambda: [0, 0])   # [below 2^-14, non-zero]
        self.bwd_max = defaultdict(float)
        self.bwd_small = defaultdict(lambda: [0, 0])

    @staticmethod
    def _acc(mx, small, site, t):
        a = t.detach().abs()
        mx[site] = max(mx[site], float(a.max())) if a.numel() else mx[site]
        nz = a[a > 0]
        small[site][0] += int((nz < FP16_MIN_NORMAL).sum())
        small[site][1] += int(nz.numel())


class _GradRound(torch.autograd.Function):
    """Identity forward; backward rounds the scaled gradient to fp16 and removes the scale (exact: a power of two)."""

    @staticmethod
    def forward(ctx, x, site, log2_scale, stats):
        ctx.site, ctx.scale, ctx.stats = site, 2.0 ** log2_scale, stats
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        gs = g * ctx.scale
        if ctx.stats is not None:
            _Stats._acc(ctx.stats.bwd_max, ctx.stats.bwd_small, ctx.site, gs)
        return gs.to(torch.float16).to(g.dtype) / ctx.scale, None, None, None


def make_q(fmt, log2_scale=0, stats=None, grads=True):
    """A replacement for refcpu._q: forward rounding to `fmt` (straight-through), backward rounding of the scaled gradient."""
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[fmt]

    def q(x, emulate_bf16, site=None):
        if not emulate_bf16 or (site is not None and site in refcpu.EXACT_SITES):
            return x
        name = site or "other"
        if stats is not None:
            stats._acc(stats.fwd_max, stats.fwd_small, name, x)
        y = x + (x.detach().to(dt).to(x.dtype) - x.detach())
        if grads and x.requires_grad and not name.endswith(".w"):
            y = _GradRound.apply(y, name, log2_scale, stats)
        return y
    return q


def _load(module, prefix, seed):
    return synth.synth_state_dict({prefix + k: v for k, v in synth.shapes_of(module).items()}, seed)


def encoder(which):
    """(state dict, oracle function (sd, emulate) -> embedding, cotangent) with test_20's seeds."""
    if which == "vit":
        from bioscanclip.model.image_encoder import LoRA_ViT_timm
        m = LoRA_ViT_timm(arch.VisionTransformerParams(depth=12), r=4, num_classes=768)
        sd = _load(m, "image_encoder.", 13)
        image, _, _, _ = synth.synth_batch(2, seed=23)
        return sd, (lambda s, e: refcpu.vit_encoder(s, image.to(s["image_encoder.lora_vit.cls_token"].dtype), emulate_bf16=e)), "vit.cot.12"
    if which == "dna":
        from bioscanclip.model.dna_encoder import LoRA_barcode_bert
        m = LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=12, **NODROP)), r=4,
                              num_classes=768)
        sd = _load(m, "dna_encoder.", 11)
        _, dna, _, _ = synth.synth_batch(2, seed=21)
        return sd, (lambda s, e: refcpu.barcode_bert_encoder(s, dna, emulate_bf16=e)), "dna.cot.12"
    from bioscanclip.model.language_encoder import LoRA_bert
    m = LoRA_bert(arch.BertModelParams(arch.bert_small_config(**NODROP)), r=4, num_classes=768)
    sd = _load(m, "language_encoder.", 12)
    _, _, text, _ = synth.synth_batch(4, seed=22, with_text=True)
    return sd, (lambda s, e: refcpu.bert_text_encoder(s, text, emulate_bf16=e)), "txt.cot"


def run(sd, fn, cot, emulate, f64=False):
    sd = {k: (v.double() if f64 and v.is_floating_point() else v).clone() for k, v in sd.items()}
    keys = [k for k in sd if refcpu.is_trainable_key(k) and sd[k].is_floating_point()]
    for k in keys:
        sd[k].requires_grad_(True)
    y = fn(sd, emulate)
    w = synth.synth_tensor(cot, y.shape, seed=5).to(y.dtype)
    (y * w).sum().backward()
    return y.detach(), {k: sd[k].grad for k in keys}


def distances(y, g, yo, go):
    worst_k = max(go, key=lambda k: rel_err(g[k], go[k]))
    return rel_err(y, yo), rel_err(g[worst_k], go[worst_k]), worst_k


def study(which):
    sd, fn, cot = encoder(which)
    refcpu._q = _orig_q
    yo, go = run(sd, fn, cot, False)
    print(f"== {which} (depth {12 if which != 'txt' else 4}) ==", flush=True)
    # unscaled pass: the range of the gradients at the rounding sites picks the tower's scale
    st0 = _Stats()
    refcpu._q = make_q("fp16", 0, st0)
    run(sd, fn, cot, True)
    gmax = max(st0.bwd_max.values())
    s = math.floor(math.log2(FP16_MAX / gmax)) - HEADROOM_LOG2
    print(f"  unscaled: largest |gradient| at a rounding site {gmax:.3e} -> log2 scale s = {s}")
    out = {"s": s}
    for streams in ("16-bit", "f32"):
        refcpu.EMULATE_RESID_BF16 = streams == "16-bit"
        for fmt in ("bf16", "fp16"):
            st = _Stats()
            refcpu._q = make_q(fmt, s if fmt == "fp16" else 0, st, grads=fmt == "fp16")
            y, g = run(sd, fn, cot, True)
            e, eg, k = distances(y, g, yo, go)
            nonfinite = sum(int((~torch.isfinite(t)).sum()) for t in [y, *g.values()])
            label = f"{fmt} operands, {streams} streams" + (f", grads x 2^{s}" if fmt == "fp16" else ", straight-through backward")
            print(f"  {label:58s} emb {e:.2e}  worst grad {eg:.2e} ({k.split('.', 1)[1]})  non-finite {nonfinite}", flush=True)
            out[(fmt, streams)] = (e, eg)
            if streams == "16-bit":
                refcpu._q = make_q(fmt, s if fmt == "fp16" else 0, None, grads=fmt == "fp16")
                y64, g64 = run(sd, fn, cot, True, f64=True)
                r, rg, _ = distances(y, g, y64, g64)
                print(f"    resolution (same roundings, f64 vs f32 accumulation): emb {r:.2e}  worst grad {rg:.2e}", flush=True)
                out[(fmt, "res")] = (r, rg)
            if fmt == "fp16" and streams == "16-bit":
                print("    site        fwd max|x|  fwd <2^-14   bwd max|g*2^s|  bwd <2^-14")
                for site in sorted(set(st.fwd_max) | set(st.bwd_max)):
                    fs, bs = st.fwd_small[site], st.bwd_small[site]
                    print(f"    {site:10s}  {st.fwd_max[site]:10.3e}  {fs[0] / max(fs[1], 1):10.2e}   "
                          f"{st.bwd_max[site]:13.3e}  {bs[0] / max(bs[1], 1):10.2e}")
    refcpu._q = _orig_q
    refcpu.EMULATE_RESID_BF16 = True
    return out


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "8")))
    sel = sys.argv[1] if len(sys.argv) > 1 else "all"
    res = {w: study(w) for w in (["vit", "dna", "txt"] if sel == "all" else [sel])}
    print("\nsummary (emb / worst grad vs f32):")
    for w, r in res.items():
        cells = "   ".join(f"{f} {st}: {r[(f, st)][0]:.2e} / {r[(f, st)][1]:.2e}" for st in ("16-bit", "res", "f32") for f in ("bf16", "fp16"))
        print(f"  {w}: s = {r['s']:3d}   {cells}")
