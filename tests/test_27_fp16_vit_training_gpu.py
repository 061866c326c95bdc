"""Training the LoRA ViT on fp16 operands (set_operand_format(model, "fp16", towers=("image",))): the fp16 backward kernels against
f32 / f64 torch arithmetic on fp16-decoded inputs, the ViT's gradients against the f32 oracle and against the oracle that also rounds
the backward as the kernels do (tests/fp16_grad_oracle.py, same static gradient scale), the gradient scale's bookkeeping (.grad holds
the true gradient), the mixed I+D(+T) step (B = 256, captured graph, golden trajectory, switch back to bf16) and train_cl end to end.

Gates of the encoder cases (test_20's weights, inputs and cotangents, train mode):
  * ViT-12 embedding <= 3e-3 and worst trainable gradient <= 1.2e-2 against the f32 oracle (the bf16 engine: 1.7e-2 / 6.8e-2);
  * HIP against the fp16-emulating oracle <= 1.5 x that oracle's own f32-vs-f64 drift (floors 5e-4 / 2e-3), test_20's criterion;
  * the bf16 engine's worst-gradient distance on the same inputs >= 3 x the fp16 engine's.
Measured values go to test_20's parity log.
"""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fp16_grad_oracle import fp16_grad_rounding  # noqa: E402
from helpers import load_golden, rel_err, skip_param_init  # noqa: E402
from oracle import refcpu, synth  # noqa: E402
import test_20_encoders_gpu as t20  # noqa: E402  (its parity log, trajectory runner and model builder)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = torch.float16
_log = t20._log


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _nrm(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _gs():
    from bioscanclip.hip.engine import ViTEngine
    return ViTEngine.FP16_GRAD_SCALE_LOG2


def _nan_buffer(rows, cols, pad_rows=4, pad_cols=64, dtype=F16):
    """A [rows, cols] view (row stride cols + pad_cols) of a NaN-filled buffer with pad_rows spare rows: nothing may be written there."""
    buf = torch.full((rows + pad_rows, cols + pad_cols), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[:rows, :cols]


def _pad_untouched(buf, rows, cols):
    return bool(torch.isnan(buf[rows:].float()).all() and torch.isnan(buf[:rows, cols:].float()).all())


# ------------------------------------------------------------------------------------------------------------- kernels
def _attn_bwd_ref(qkv, dctx, B, S, heads, scale):
    """f64 autograd of softmax attention on the fp16-decoded operands: dq | dk | dv [B S, 3 heads 64] and lse [B, heads, S]."""
    x = qkv.double().view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    s = (x[0] @ x[1].transpose(-1, -2)) * scale
    ctx = (torch.softmax(s, dim=-1) @ x[2]).permute(0, 2, 1, 3).reshape(B * S, heads * 64)
    (ctx * dctx.double()).sum().backward()
    d = x.grad.permute(1, 3, 0, 2, 4).reshape(B * S, 3 * heads * 64)
    return d, torch.logsumexp(s.detach(), dim=-1)


@pytest.mark.parametrize("q_rows,lora", [(0, False), (0, True), (1, True)])
def test_attention_backward_fp16(q_rows, lora):
    from bioscanclip.hip import ops
    B, S, heads, scale, H = 3, 197, 12, 0.125, 768
    g = torch.Generator().manual_seed(40 + q_rows)
    qkv = (torch.randn(B * S, 3 * H, generator=g) * 1.5).to(F16)
    # the scaled gradient stream's size (2^13 x ~1e-3): the fp16 kernels see values of order 1 - 10
    dctx = (torch.randn(B * S, H, generator=g) * 4).to(F16)
    if q_rows == 1:   # the last ViT block: only token 0 of each image carries a gradient
        keep = torch.zeros(B * S, 1, dtype=F16)
        keep[torch.arange(B) * S] = 1
        dctx = dctx * keep
    ref, lse = _attn_bwd_ref(qkv, dctx, B, S, heads, scale)
    dbuf, dqkv = _nan_buffer(B * S, 3 * H)
    args = dict(q_rows=q_rows)
    if lora:
        t = (torch.randn(B * S, 8, generator=g) * 0.5).to(F16)
        lb = torch.randn(2, H, 4, generator=g) * 3e-3
        tbuf = torch.zeros(B * S, 64, dtype=F16)
        tbuf[:, :8] = t
        n_dt, n_db = heads * 2 * B * S * 4, B * heads * 2 * 4 * 64
        dtp_buf = torch.full((n_dt + 64,), float("nan"), device="cuda")
        dbp_buf = torch.full((n_db + 64,), float("nan"), device="cuda")
        args["lora"] = (tbuf.cuda()[:, :8], lb.cuda().contiguous(), dtp_buf[:n_dt], dbp_buf[:n_db])
    ops.attn_bwd(qkv.cuda(), dctx.cuda(), lse.float().cuda().contiguous(), B, S, heads, scale, dqkv, **args)
    torch.cuda.synchronize()
    assert _pad_untouched(dbuf, B * S, 3 * H), "the attention backward wrote past dqkv"
    got = dqkv.cpu().double()
    rec = {"test": f"fp16_attn_bwd_q{q_rows}{'_lora' if lora else ''}"}
    for i, nm in enumerate("qkv"):
        rec[f"d{nm}_vs_f64"] = _nrm(got[:, i * H:(i + 1) * H], ref[:, i * H:(i + 1) * H])
    if q_rows == 1:   # query blocks past the first are written as zeros
        rows = torch.arange(B * S).view(B, S)[:, 32:].reshape(-1)
        assert torch.all(got[rows, :H] == 0)
    if lora:
        assert torch.isnan(dtp_buf[n_dt:]).all() and torch.isnan(dbp_buf[n_db:]).all(), "the LoRA partials were written past their end"
        dq, dv = ref[:, :H], ref[:, 2 * H:]
        hb = lambda x: x.view(B * S, heads, 64)
        lbd = lb.double()
        dt_ref = torch.stack([torch.einsum("mhd,hdj->hmj", hb(d), lbd[i].view(heads, 64, 4)) for i, d in enumerate((dq, dv))], 1)
        dtp = dtp_buf[:n_dt].view(heads, 2, B * S, 4).cpu().double()
        rec["dt_partial_vs_f64"] = _nrm(dtp, dt_ref)
        td = t.double().view(B, S, 8)
        db_ref = torch.stack([torch.einsum("bsj,bshd->bhjd", td[..., 4 * i:4 * i + 4], d.view(B, S, heads, 64))
                              for i, d in enumerate((dq, dv))], 2).reshape(B * heads, 2, 4, 64)
        dbp = dbp_buf[:n_db].view(B * heads, 2, 4, 64).cpu().double()
        rec["db_partial_vs_f64"] = _nrm(dbp, db_ref)
    _log(rec)
    # measured (f64 reference on the same fp16 operands): ~6e-4 for dq / dk / dv and the partials -- fp16's P and dS roundings
    worst = max(v for k, v in rec.items() if k != "test")
    assert worst < 2e-3, rec


def test_attention_backward_fp16_host_validation():
    from bioscanclip.hip import lib, ops
    h = lib.load()
    F = lib.OPERANDS_FP16
    z = lambda *s: torch.zeros(*s, dtype=F16, device="cuda")
    qkv, dctx, dq, lse = z(2 * 197, 2304), z(2 * 197, 768), z(2 * 197, 2304), torch.zeros(2, 12, 197, device="cuda")
    with pytest.raises(ValueError, match="dropout"):
        ops.attn_bwd(qkv, dctx, lse, 2, 197, 12, 0.125, dq, dropout=(0.1, 3))
    assert h.bsclip_attn_bwd(qkv.data_ptr(), 2304, dctx.data_ptr(), 768, lse.data_ptr(), 2, 133, 12, None,
                             __import__("ctypes").c_float(0.125), dq.data_ptr(), 2304, F, None, __import__("ctypes").c_float(0.0), 0,
                             None) == -1
    assert "S = 197" in lib.last_error()


def _ln_case(M, g, lora):
    H = 768
    x = (torch.randn(M, H, generator=g) * 2 + 0.3).to(F16)
    gamma = torch.rand(H, generator=g) + 0.5
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = (var + 1e-6).rsqrt()
    stats = torch.stack([mean[:, 0], rstd[:, 0]], 1).float()
    gr = (torch.randn(M, H, generator=g) * 8).to(F16)
    gg = (torch.randn(M, H, generator=g) * 8).to(F16)
    dt = torch.randn(M, 8, generator=g) * 20 if lora else None
    A = torch.randn(8, H, generator=g) * 0.05 if lora else None
    dy = gg.double() + (dt.double() @ A.double() if lora else 0)
    xh = (xd - stats[:, :1].double()) * stats[:, 1:].double()
    dxh = dy * gamma.double()
    dx = (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True)) * stats[:, 1:].double() + gr.double()
    return x, gamma, stats, gr, gg, dt, A, dx


@pytest.mark.parametrize("lora", [False, True])
def test_layernorm_backward_fp16_is_the_rounding_of_its_f32_value(lora):
    from bioscanclip.hip import ops
    M, H = 300, 768
    g = torch.Generator().manual_seed(7 + lora)
    x, gamma, stats, gr, gg, dt, A, ref = _ln_case(M, g, lora)
    obuf, out = _nan_buffer(M, H)
    # the ViT's call: the gradient stream is read as g_resid and rewritten in place -- here a separate output, to see the pad
    ops.layernorm_bwd(x.cuda(), stats.cuda(), gamma.cuda(), 0, g_resid=gr.cuda(), g_gemm=gg.cuda(),
                      dt=None if dt is None else dt.cuda().contiguous(), lora_a=None if A is None else A.cuda().contiguous(),
                      dx_bf16=out)
    torch.cuda.synchronize()
    assert _pad_untouched(obuf, M, H), "the LayerNorm backward wrote past its output"
    got = out.cpu()
    rne = ref.to(F16)        # the RNE rounding of the exact value; the kernel's f32 value may sit across a rounding boundary
    exact_share = (got == rne).double().mean().item()
    # RNE of a value within f32 arithmetic's reach of the exact one: |got - exact| <= half an fp16 ulp of got + an f32 band of the row
    # (2^-18 x its largest |dx|: the cancellations of dy - c1 - xhat c2 cost small elements more of their own ulps)
    r = got.double()
    ulp = torch.where(r.abs() >= 2.0 ** -14, 2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -14))) - 10),
                      torch.full_like(r, 2.0 ** -24))
    band = 2.0 ** -18 * ref.abs().amax(1, keepdim=True)
    excess = ((r - ref).abs() - 0.5 * ulp - band).max().item()
    rec = {"test": f"fp16_ln_bwd{'_lora' if lora else ''}", "rne_equal_share": exact_share, "max_excess_over_half_ulp_and_band": excess,
           "vs_f64": _nrm(got, ref)}
    _log(rec)
    assert torch.isfinite(got.float()).all()
    assert exact_share > 0.999 and excess <= 0, rec


def test_layernorm_backward_fp16_host_validation():
    from bioscanclip.hip import lib, ops
    x = torch.zeros(4, 768, dtype=F16, device="cuda")
    st, gm = torch.zeros(4, 2, device="cuda"), torch.ones(768, device="cuda")
    with pytest.raises(ValueError, match="fp16"):
        ops.layernorm_bwd(x, st, gm, 0, g_gemm=x, dx_bf16=x, dropout=(0.1, 1))
    with pytest.raises(ValueError, match="fp16"):
        ops.layernorm_bwd(x, st, gm, 0, g_gemm=x.to(torch.bfloat16), dx_bf16=x)
    import ctypes
    h = lib.load()
    F = lib.OPERANDS_FP16
    call = lambda flag, p=0.0, rf=0: h.bsclip_layernorm_bwd(x.data_ptr(), 768, flag, st.data_ptr(), gm.data_ptr(), 4, 768, None, 0,
                                                           x.data_ptr(), 768, None, None, 0, None, 0, x.data_ptr(), 768,
                                                           ctypes.c_float(p), 1, ctypes.c_float(0.0), 0, rf, None)
    assert call(1 | F) == 0
    assert call(1 | F, p=0.1) == -1 and "dropout" in lib.last_error()
    assert call(1 | F, rf=8) == -1 and "fp16" in lib.last_error()


def test_lora_gradients_fp16_take_the_scale_off():
    """bsclip_lora_grad_heads_f16: dA / dB receive 2^-s x the sums of 2^s-scaled partials, dt stays scaled."""
    from bioscanclip.hip import ops
    B, S, H, heads = 2, 197, 768, 12
    M, s = B * S, _gs()
    g = torch.Generator().manual_seed(3)
    h = torch.zeros(M, H + 64, dtype=F16)
    h[:, :H] = (torch.randn(M, H, generator=g)).to(F16)
    dtp = torch.randn(heads, 2, M, 4, generator=g) * 2.0 ** s * 1e-3
    dbp = torch.randn(B * heads, 2, 4, 64, generator=g) * 2.0 ** s * 1e-2
    dt = torch.zeros(M, 8, device="cuda")
    dA0 = torch.randn(8, H, generator=g)
    dB0 = torch.randn(2, H, 4, generator=g)
    dA, dB = dA0.clone().cuda(), dB0.clone().cuda()
    ops.lora_grad_heads(h.cuda(), M, H, B, dtp.cuda(), dbp.cuda(), dt, dA, dB[0], dB[1], grad_scale_log2=s)
    torch.cuda.synchronize()
    dt_ref = dtp.double().sum(0).permute(1, 0, 2).reshape(M, 8)
    db_ref = dbp.double().view(B, heads, 2, 4, 64).sum(0).permute(1, 0, 3, 2).reshape(2, H, 4) / 2.0 ** s
    da_ref = dt_ref.t() @ h[:, :H].double() / 2.0 ** s
    rec = {"test": "fp16_lora_grad_heads", "dt": _nrm(dt, dt_ref), "dA": _nrm(dA.cpu() - dA0, da_ref), "dB": _nrm(dB.cpu() - dB0, db_ref)}
    _log(rec)
    assert max(rec["dt"], rec["dA"], rec["dB"]) < 1e-4, rec   # f32 summation order; a scale left on would be off by 2^13
    with pytest.raises(ValueError, match="grad_scale_log2"):
        ops.lora_grad_heads(h.cuda(), M, H, B, dtp.cuda(), dbp.cuda(), dt, dA, dB[0], dB[1])


# ------------------------------------------------------------------------------------------------------------- encoders
# measured (gradients on the GPU box, profiles/r08_fp16_vit_training.jsonl): see DESIGN.md 4, part 3a
VIT_CAP = {"vit_L2": (3e-3, 1.2e-2), "vit_L12": (3e-3, 1.2e-2)}


def _vit(depth):
    from bioscanclip.model import arch
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    with skip_param_init():
        m = LoRA_ViT_timm(arch.VisionTransformerParams(depth=depth), r=4, num_classes=768)
    sd = t20._load(m, "image_encoder.", 13)
    image, _, _, _ = synth.synth_batch(2, seed=23)
    fn = lambda s, emulate=False, f64=False: refcpu.vit_encoder(s, image.double() if f64 else image, emulate_bf16=emulate)
    return m.to("cuda"), sd, image.cuda(), fn


def _hip_grads(m, x, w, fmt):
    from bioscanclip.hip.engine import set_operand_format
    set_operand_format(m, fmt, towers=("image",))
    m.train()
    m.zero_grad(set_to_none=True)
    y = m(x)
    (y * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("depth", [2, 12])
def test_vit_encoder_fp16_training(depth):
    name = f"vit_L{depth}"
    m, sd, x, fn = _vit(depth)
    w = synth.synth_tensor(f"vit.cot.{depth}", (2, 768), seed=5)
    y16, g16 = _hip_grads(m, x, w, "fp16")
    assert m._engine.fp16 and m._engine.ws["dxb"].dtype == F16
    ybf, gbf = _hip_grads(m, x, w, "bf16")
    yo, go = t20._oracle_f32(name, sd, fn, w)
    keys = list(go)
    prefix = "image_encoder."
    with fp16_grad_rounding(_gs()):
        sde, _, ye = t20._oracle_grads(sd, lambda s: fn(s, emulate=True))
        (ye * w).sum().backward()
        sde64, _, ye64 = t20._oracle_grads(t20._f64(sd), lambda s: fn(s, emulate=True, f64=True))
        (ye64 * w.double()).sum().backward()
    rec = {"test": f"fp16_train_{name}", "grad_scale_log2": _gs(), "emb_vs_f32_oracle": rel_err(y16, yo),
           "emb_vs_fp16_emulating_oracle": rel_err(y16, ye), "emulating_oracle_f32acc_vs_f64acc": rel_err(ye, ye64.detach()),
           "bf16_emb_vs_f32_oracle": rel_err(ybf, yo), "grads": {}}
    worst = worst_emu = self_g = worst_bf = 0.0
    for k in keys:
        kk = k[len(prefix):]
        assert kk in g16, k
        e = rel_err(g16[kk], go[k])
        rec["grads"][k] = e
        worst = max(worst, e)
        worst_emu = max(worst_emu, rel_err(g16[kk], sde[k].grad))
        self_g = max(self_g, rel_err(sde[k].grad, sde64[k].grad))
        worst_bf = max(worst_bf, rel_err(gbf[kk], go[k]))
    rec.update(worst_grad=worst, worst_grad_vs_emulating_oracle=worst_emu, worst_grad_emulating_oracle_f32acc_vs_f64acc=self_g,
               bf16_worst_grad=worst_bf)
    _log(rec)
    cap_emb, cap_grad = VIT_CAP[name]
    assert torch.isfinite(y16).all()
    assert rec["emb_vs_f32_oracle"] <= cap_emb and worst <= cap_grad, rec
    assert rec["emb_vs_fp16_emulating_oracle"] < max(1.5 * rec["emulating_oracle_f32acc_vs_f64acc"], 5e-4), rec
    assert worst_emu < max(1.5 * self_g, 2e-3), rec
    assert worst_bf >= 3 * worst, rec


def test_grad_is_unscaled_and_accumulates_over_chunks():
    """.grad holds the true gradient: a batch's gradients equal the sum of its chunks' (accumulated over two backward calls), and the
    fp16 gradient's norm sits within the bf16 engine's distance of the bf16 one's."""
    from bioscanclip.hip.engine import set_operand_format
    m, _, _, _ = _vit(2)
    image, _, _, _ = synth.synth_batch(4, seed=29)
    image = image.cuda()
    w = synth.synth_tensor("vit.cot.chunks", (4, 768), seed=6).cuda()
    set_operand_format(m, "fp16", towers=("image",))
    m.train()
    m.zero_grad(set_to_none=True)
    (m(image) * w).sum().backward()
    whole = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    for sl in (slice(0, 2), slice(2, 4)):
        (m(image[sl]) * w[sl]).sum().backward()
    parts = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    worst = max(rel_err(parts[k], v) for k, v in whole.items())
    set_operand_format(m, "bf16")
    m.zero_grad(set_to_none=True)
    (m(image) * w).sum().backward()
    bf = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    n16 = torch.cat([v.reshape(-1) for v in whole.values()]).norm().item()
    nbf = torch.cat([v.reshape(-1) for v in bf.values()]).norm().item()
    rec = {"test": "fp16_grad_chunks", "worst_chunk_sum_vs_batch": worst, "norm_fp16": n16, "norm_bf16": nbf,
           "worst_fp16_vs_bf16": max(rel_err(whole[k], v) for k, v in bf.items())}
    _log(rec)
    # the same fp16 kernels on the same images: only the f32 summation order of the batch reductions differs (a missing 2^-s would
    # be off by 2^13)
    assert worst < 1e-3, rec
    assert abs(n16 - nbf) / nbf <= rec["worst_fp16_vs_bf16"], rec


# ------------------------------------------------------------------------------------------------------------- the mixed step
def _clip(seed, with_text):
    model, _ = t20._build_clip(with_text, seed)
    return model.to("cuda").train()


def test_b256_mixed_step_gradient_stream_within_headroom():
    """A B = 256 I+D+T step with the image tower on fp16: no non-finite value in the fp16 gradient stream, the largest scaled |gradient|
    at least 2^4 under 65 504, the share of non-zero values below 2^-14 small."""
    from bioscanclip.hip.engine import ViTEngine, count_nonfinite, set_operand_format
    from bioscanclip.model.loss_func import ContrastiveLoss
    model = _clip(101, True)
    set_operand_format(model, "fp16", towers=("image",))
    crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
    image, dna, text, label = synth.synth_batch(256, seed=77, with_text=True)
    stats = {"amax": 0.0, "small": 0, "nz": 0, "nonfinite": 0}

    def probe(site, t):
        a = t.float().abs()
        stats["nonfinite"] += count_nonfinite(t)
        stats["amax"] = max(stats["amax"], float(a[torch.isfinite(a)].max()))
        nz = a[a > 0]
        stats["small"] += int((nz < 2.0 ** -14).sum())
        stats["nz"] += int(nz.numel())

    ViTEngine.grad_probe = staticmethod(probe)
    try:
        loss = crit(*model(image.cuda(), dna.cuda(), {k: v.cuda() for k, v in text.items()}), label.cuda())
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ViTEngine.grad_probe = None
    eng = model.image_encoder._engine
    assert eng.fp16 and not model.dna_encoder._engine.fp16
    rec = {"test": "fp16_b256_idt_step", "grad_scale_log2": _gs(), "loss": loss.item(), "scaled_amax": stats["amax"],
           "below_min_normal_share": stats["small"] / max(1, stats["nz"]), "nonfinite": stats["nonfinite"]}
    _log(rec)
    assert stats["nonfinite"] == 0 and math.isfinite(loss.item()), rec
    assert stats["amax"] <= 65504.0 / 16, rec
    # recorded at this step (profiles/r08_fp16_vit_training.jsonl): 0.14 over all sites at s = 14 (dfc1_out and dqkv worst)
    assert rec["below_min_normal_share"] < 0.25, rec
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


def test_graph_replay_of_the_mixed_step_equals_eager():
    from bioscanclip.hip.engine import set_operand_format
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    from test_30_graph_gpu import _build
    steps = 6
    batches = [synth.synth_batch(16, seed=500 + s % 3, with_text=True) for s in range(steps)]
    cuda = lambda t: {k: v.cuda() for k, v in t.items()} if isinstance(t, dict) else t.cuda()
    runs = {}
    for mode in ("eager", "graph"):
        model = _build(93, True)
        set_operand_format(model, "fp16", towers=("image",))
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        opt.enable_device_hyper(True)
        crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
        g = GraphedStep(model, opt, crit, warmup=2) if mode == "graph" else None
        losses = []
        for s in range(steps):
            image, dna, text, label = (cuda(t) for t in batches[s])
            if g is not None:
                loss = g(image, dna, text, label)
            else:
                opt.zero_grad()
                loss = crit(*model(image, dna, text), label)
                loss.backward()
                if opt.needs_attach():
                    opt.attach(model)
                opt.step()
            losses.append(loss.item())
        if g is not None:
            assert g.graph is not None
        assert model.image_encoder._engine.fp16 and not model.dna_encoder._engine.fp16
        runs[mode] = (losses, {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad})
    assert runs["eager"][0] == runs["graph"][0], runs
    for k, v in runs["eager"][1].items():
        assert torch.equal(v, runs["graph"][1][k]), k


def test_golden_trajectory_with_the_image_tower_on_fp16(monkeypatch):
    """configs[0] (I+D, B = 8, 10 steps) with the image tower on fp16 passes the default mode's trajectory gates."""
    from bioscanclip.hip.engine import set_operand_format
    orig = t20._build_clip

    def build(*a, **k):
        model, sd = orig(*a, **k)
        set_operand_format(model, "fp16", towers=("image",))
        return model, sd

    monkeypatch.setattr(t20, "_build_clip", build)
    t20._run_trajectory(False, t20.TRAJ_TOL[False], "trajectory_fp16_image text=False")


def test_switch_back_to_bf16_keeps_parameters_and_optimizer_state():
    from bioscanclip.hip.engine import set_operand_format
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    model = _clip(55, False)
    set_operand_format(model, "fp16", towers=("image",))
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
    image, dna, _, label = (t.cuda() if t is not None else None for t in synth.synth_batch(8, seed=61))

    def step():
        opt.zero_grad()
        loss = crit(*model(image, dna, None), label)
        loss.backward()
        if opt.needs_attach():
            opt.attach(model)
        opt.step()
        return loss.item()

    l16 = [step() for _ in range(3)]
    eng16 = model.image_encoder._engine
    flat = eng16.flat
    params = {k: p.detach().clone() for k, p in model.image_encoder.named_parameters() if p.requires_grad}
    st = opt._state_for(flat)
    m_before, step_before = st["m"].clone(), st["step"]
    set_operand_format(model, "bf16")
    lbf = step()
    engbf = model.image_encoder._engine
    assert engbf is not eng16 and not engbf.fp16 and engbf.flat is flat      # rebuilt engine, same flat buffer
    st2 = opt._state_for(flat)
    assert st2["step"] == step_before + 1 and not torch.equal(st2["m"], m_before) and st2["m"].norm() > 0
    moved = max(rel_err(p.detach(), params[k]) for k, p in model.image_encoder.named_parameters() if p.requires_grad)
    _log({"test": "fp16_switch_back", "losses_fp16": l16, "loss_bf16": lbf, "param_move": moved})
    assert all(math.isfinite(x) for x in l16 + [lbf]) and lbf < l16[0]   # the bf16 step continues from the fp16-trained values
    assert moved > 0


def test_train_cl_with_the_image_tower_on_fp16(tmp_path, capsys):
    scripts = os.path.join(ROOT, "bioscan-clip_amd", "scripts")
    sys.path.insert(0, scripts)
    import train_cl
    losses = train_cl.main(["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.batch_size=8", "model_config.epochs=1",
                            "synthetic_steps_per_epoch=2", "save_ckpt=true", "debug_flag=false", "hip_fp16_towers=image",
                            f"project_root_path={tmp_path}"])
    assert len(losses) == 1 and all(math.isfinite(float(x)) for x in losses)
    ck = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith("last.pth")]
    assert ck
    keys = set(torch.load(ck[0], map_location="cpu").keys())
    assert keys == {k for k in load_golden("state_dict_keys")["keys"] if not k.startswith("language_encoder.")}
