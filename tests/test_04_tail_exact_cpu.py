"""The claims tests/test_16_tail_kernels_gpu.py rests on, proven without a GPU (tests/tail_exact.py holds the inputs, cases, references,
comparisons and bars).  Kernels: bsclip_cast_f32_bf16 / _f16 / _f16_scaled, bsclip_add_scaled_f32, bsclip_adamw_step / _dev / _clip,
bsclip_count_nonfinite, bsclip_counter_add, bsclip_im2col_patch16, bsclip_dgelu_mul, bsclip_softmax_meanpool_fwd / _bwd,
bsclip_meanpool_tokens_fwd / _bwd, bsclip_bert_embed, bsclip_l2norm_fwd / _bwd, bsclip_vit_cls_rows, bsclip_waug_set_lora_layers,
bsclip_mask_to_bias, bsclip_gather_cast_rows, bsclip_transpose_bf16 (element kernel).

Path-change sizes (tail_exact.py names the source line of each): the casts' grid-stride loop starts past 2^21 elements, add_scaled_f32's
past 2^20, the AdamW kernels' and count_nonfinite's past 524 288, im2col's past 1 048 576 items (B >= 56), dgelu_mul's past 1 048 576
groups of four; softmax_meanpool_fwd leaves waves without a token at S < 4; l2norm clamps below ||x|| = 1e-12.

* every reference equals the framework's own operation in f64 on the CPU: torch.optim.AdamW over the trajectory, F.normalize and its
  autograd, softmax -> mean and its autograd, nn.functional.embedding sums, F.unfold, mean's autograd;
* the exact inputs are exact at every case size: each reference's own assertion runs, and the f32 restatement equals f64;
* each comparison can fail: for every kernel, outputs corrupted the way that kernel could go wrong -- the n & 3 tail unwritten, the
  second grid-stride pass skipped or applied twice, a row skipped, two rows swapped, a lane's 4-column piece one lane off, a truncating
  conversion, the id clamp removed, 1 / S applied twice -- are rejected, and a SINGLE-element corruption that the whole-tensor
  ``rel_err`` of tests/test_10_kernels_gpu.py accepts at that test's bar is rejected too;
* the bars: each kernel's arithmetic restated in f32 (same formula and association as the source, no fused multiply-adds, exp correctly
  rounded to f32), its worst distance from f64 over every GPU case in the unit the GPU test asserts in, printed as ``FIGURES {json}``
  lines; tail_exact.BAR must equal 4 x those figures."""
import json
import math

import pytest
import torch
import torch.nn.functional as Fn

import tail_exact as tx
from helpers import rel_err

F32, F64, BF16, F16 = tx.F32, tx.F64, tx.BF16, tx.F16
TOL_F32, TOL_BF16, TOL_ADAMW = 2e-5, 4e-3, 1e-6          # tests/test_10_kernels_gpu.py's whole-tensor bars


def _log(test, **figures):
    print("FIGURES " + json.dumps({"test": test, **figures}))


def f(x):
    return torch.tensor(x, dtype=F32)


# ------------------------------------------------------------------------------------------ f32 restatements of the kernels
def butterfly(s):
    """csrc/common.h wave_sum on the lanes' partial sums s [rows, 64]: five xor stages; every lane ends with the same value."""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, :1]


def lane_pieces(t):
    """[rows, D] -> [rows, K, 64, 4] with column = 256 k + 4 lane + i (zero columns appended up to a multiple of 256: a lane without
    data adds nothing)."""
    rows, D = t.shape
    K = -(-D // 256)
    pad = torch.zeros(rows, K * 256, dtype=t.dtype)
    pad[:, :D] = t
    return pad.view(rows, K, 64, 4)


def exp32(x):
    """f32 exp, correctly rounded (through f64): the same on every CPU."""
    return torch.exp(x.double()).float()


def adamw_step_f32(p, m, v, g, hp, t):
    """csrc/optim.hip adamw_update statement by statement in f32, the bias corrections formed in f64 from the f32 betas and rounded, as
    bsclip_adamw_step and adamw_hyper do."""
    lr, b1, b2, eps, wd, gs = (f(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "grad_scale"))
    one = f(1.0)
    inv_bc1 = f(1.0 / (1.0 - b1.double().item() ** t))
    inv_sqrt_bc2 = f(1.0 / math.sqrt(1.0 - b2.double().item() ** t))
    gi = g * gs
    pi = p * (one - lr * wd)
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + ((one - b2) * gi) * gi
    denom = torch.sqrt(vi) * inv_sqrt_bc2 + eps
    return pi - (lr * inv_bc1) * (mi / denom), mi, vi


def l2norm_fwd_f32(x):
    q = lane_pieces(x)
    s = torch.zeros(x.shape[0], 64, dtype=F32)
    for k in range(q.shape[1]):
        a = q[:, k]
        s = s + ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + (a[..., 2] * a[..., 2] + a[..., 3] * a[..., 3]))
    inv = f(1.0) / torch.maximum(torch.sqrt(butterfly(s)), f(1e-12))
    return x * inv, inv[:, 0]


def l2norm_bwd_f32(y, inv, dy):
    a, g = lane_pieces(y), lane_pieces(dy)
    s = torch.zeros(y.shape[0], 64, dtype=F32)
    for k in range(a.shape[1]):
        p = a[:, k] * g[:, k]
        s = s + ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3]))
    return (dy - y * butterfly(s)) * inv[:, None]


def lane_seq_sum(t):
    """The softmax kernels' per-lane sum: s += t[j][i] over j, then i, in order; then the butterfly."""
    q = lane_pieces(t)
    s = torch.zeros(t.shape[0], 64, dtype=F32)
    for j in range(q.shape[1]):
        for i in range(4):
            s = s + q[:, j, :, i]
    return butterfly(s)


def softmax_fwd_f32(logits, B, S):
    """csrc/heads.hip softmax_meanpool_fwd_kernel: wave w sums tokens w, w + 4, ...; (r0 + r1) + (r2 + r3); times 1.0f / S."""
    C = logits.shape[1]
    m = logits.amax(1, keepdim=True)
    v = exp32(logits - m)
    s = lane_seq_sum(v)
    contrib = (v * (f(1.0) / s)).view(B, S, C)
    acc = [torch.zeros(B, C, dtype=F32) for _ in range(4)]
    for t in range(S):
        acc[t % 4] = acc[t % 4] + contrib[:, t]
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) * (f(1.0) / f(float(S))), torch.cat([m, s], 1)


def softmax_bwd_f32(logits, stats, dp, B, S):
    """softmax_meanpool_bwd_kernel up to the bf16 rounding of its result."""
    g = (dp * (f(1.0) / f(float(S)))).repeat_interleave(S, 0)
    p = exp32(logits - stats[:, :1]) * (f(1.0) / stats[:, 1:])
    return p * (g - lane_seq_sum(p * g))


def meanpool_fwd_f32(x, B, S):
    xv = x.view(B, S, -1)
    acc = torch.zeros(B, xv.shape[2], dtype=F32)
    for t in range(S):
        acc = acc + xv[:, t]
    return acc * (f(1.0) / f(float(S)))


# ------------------------------------------------------------------------------------------------ references = the framework's ops
@pytest.mark.parametrize("name", list(tx.ADAMW_SETS))
def test_adamw_reference_is_torch_adamw(name):
    hp, step0 = tx.ADAMW_SETS[name]
    p, m, v, g = tx.adamw_inputs(1000)
    grads = [tx.adamw_grad(g, s) for s in range(tx.ADAMW_STEPS)]
    ref = tx.adamw64(p, m, v, grads, hp, step0)
    h = {k: tx.f32r(x) for k, x in hp.items()}
    q = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.AdamW([q], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"])
    opt.state[q] = {"step": torch.tensor(float(step0 - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    for s, gr in enumerate(grads):
        q.grad = gr.double() * h["grad_scale"]
        opt.step()
        for got, want in zip(ref[s + 1], (q.data, opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"])):
            assert ((got - want).abs() <= 1e-13 * want.abs() + 1e-300).all()
    if name == "lr0":
        assert torch.equal(ref[-1][0], p.double())


def test_l2norm_reference_is_normalize_and_its_autograd():
    for D in tx.L2_D:
        x, dy, kinds = tx.l2norm_rows(37, D)
        xd = x.double().requires_grad_(True)
        yt = Fn.normalize(xd, p=2, dim=-1, eps=tx.L2_EPS)
        y, inv = tx.l2norm_fwd64(x)
        assert torch.allclose(y, yt.detach(), rtol=1e-14, atol=0) and set(kinds) == {"ord", "zero", "tiny", "big"}
        (gx,) = torch.autograd.grad(yt, xd, dy.double())
        dx = tx.l2norm_bwd64(y, inv, dy)
        for r, k in enumerate(kinds):
            scale = gx[r].abs().max()
            dev = ((dx[r] - gx[r]).abs().max() / scale).item()
            if k == "tiny":      # clamped and non-zero: the documented formula keeps the y (y . dy) term, |y|^2 ~ 1e-6 of the answer
                assert dev < 4 * (y[r].norm() ** 2).item() and y[r].norm() < 2e-3
            else:
                assert dev < 1e-12, (D, r, k, dev)
        # the rows do what they are there for in f32 too
        ss = (x * x).sum(1)
        assert ss[kinds.index("tiny")] > 0 and ss[kinds.index("tiny")].sqrt() < 1e-12 and 1e29 < ss[kinds.index("big")] < 1e31


@pytest.mark.parametrize("B,S", [(1, 1), (3, 5), (2, 4)])
def test_softmax_reference_is_softmax_mean_and_its_autograd(B, S):
    x = tx.softmax_logits(B, S, 3.0)
    dp = tx.hash_real(B * 768, 82).view(B, 768)
    xd = x.double().requires_grad_(True)
    want = torch.softmax(xd.view(B, S, -1), -1).mean(1)
    pooled, stats, _ = tx.softmax_pool64(x, B, S)
    assert torch.allclose(pooled, want.detach(), rtol=1e-13, atol=1e-300)
    assert torch.equal(stats[:, 0], x.double().amax(1)) and torch.allclose(stats[:, 1], torch.exp(x.double() - stats[:, :1]).sum(1))
    (gx,) = torch.autograd.grad(want, xd, dp)
    d, denom = tx.softmax_pool_bwd64(x, dp, B, S)
    assert ((d - gx).abs() <= 1e-12 * denom).all()
    assert x[0].argmax() == 767 and (B * S == 1 or (x[1, 5] == x[1].max() and x[1, 700] == x[1].max()))


def test_embed_reference_is_embedding_sums():
    for kind in ("exact", "real"):
        for types in (False, True):
            c = tx.embed_case(3, 43, 512, kind, types)
            V = tx.EMBED_VOCAB
            ids = c["ids"].clamp(0, V - 1)
            tt = (c["type_ids"] != 0).long() if types else torch.zeros_like(ids)
            want = Fn.embedding(ids, c["word"].double()) + c["pos"][:43].double()[None] + Fn.embedding(tt, c["typ"][:2].double())
            ref64, ref32 = tx.embed_ref(c)
            assert torch.equal(ref64, want.view(-1, 512)) and not torch.isnan(ref64).any()
            flat = c["ids"].view(-1).tolist()
            assert {V + 5, -1, 0, V - 1} <= set(flat) and (not types or set(c["type_ids"].view(-1).tolist()) == {0, 1, 2, -1})
            if kind == "exact":
                assert torch.equal(ref32.double(), ref64)
            else:
                assert (ref32.double() - ref64).abs().max() < 1e-6 and not torch.equal(ref32.double(), ref64)


def test_im2col_reference_is_unfold():
    img = tx.im2col_image(2)
    want = Fn.unfold(img, kernel_size=16, stride=16).transpose(1, 2).reshape(2 * 196, 768)
    for dtype in (BF16, F16):
        ref = tx.im2col_ref(img, True, dtype)
        assert torch.equal(ref[:, :768], want.to(dtype)) and torch.equal(ref[:, 1536:], ref[:, :768])
        assert torch.equal(ref[:, :768].double() + ref[:, 768:1536].double(), want.double())
        assert (ref[:, 768:1536] != 0).double().mean() > 0.75         # the lo third carries something on most elements
        assert torch.equal(tx.im2col_ref(img, False, dtype), want.to(dtype))


def test_small_references():
    # meanpool_tokens_bwd: the autograd of mean(tokens)
    d, want = tx.meanpool_bwd_case(3, 7, 512)
    x = torch.zeros(3, 7, 512, dtype=F64, requires_grad=True)
    (gx,) = torch.autograd.grad(x.mean(1), x, d.double())
    assert (want.double().view(3, 7, 512) - gx).abs().max() <= 2.0 ** -24 * 1000
    # mask_to_bias: HF's (1 - m) * finfo.min on {0, 1}; any non-zero value keeps the key
    mask, want = tx.mask_case(1000)
    assert set(mask.tolist()) == {0, 1, 2, -1}
    hf = (1.0 - mask.clamp(0, 1).float()) * torch.finfo(F32).min
    sel = (mask == 0) | (mask == 1)
    assert torch.equal(want[sel], hf[sel]) and (want[~sel] == 0).all() and tx.F32_MIN == torch.finfo(F32).min
    # gather_cast_rows: the engine's use (drop the class row of every sequence) and what the wrapper wants of src
    src = tx.hash_real(3 * 197 * 8, 1).float().view(3 * 197, 8)
    assert torch.equal(tx.gather_ref(src, 3 * 196, 197, 196, 1), src.view(3, 197, 8)[:, 1:].reshape(-1, 8).to(BF16))
    for p_in, p_out, off, rows in tx.GATHER_CASES:
        need, last = tx.gather_src_rows(rows, p_in, p_out, off)
        assert last <= need and rows % 4 != 0
    # dgelu_mul: the decode is test_12's, the product one rounding of the f64 product of the decoded f32
    g, codes, want = tx.dgelu_case(5, 3072)
    exact = g.double() * (codes.double() * tx.DG8_STEP - tx.DG8_OFF)
    assert ((want.double() - exact).abs() <= 2.0 ** -8 * exact.abs() + 1e-30).all() and set(codes[0].tolist()) == set(range(256))


def test_cast_table_holds_what_it_claims():
    sp = tx._f32_from_bits(list(tx.CAST_SPECIAL_BITS))
    b, h = sp.to(BF16), sp.to(F16)
    val = lambda w: tx._f32_from_bits([w])  # noqa: E731
    assert val(0x3F808000).to(BF16).item() == 1.0 and val(0x3F818000).to(BF16).item() == 1.015625          # ties to even, both ways
    assert val(0x3F801000).to(F16).item() == 1.0 and val(0x3F803000).to(F16).item() == 1.0 + 2.0 ** -9
    assert val(0x3FFFFFFF).to(BF16).item() == 2.0 and val(0x3FFFF000).to(F16).item() == 2.0                  # into the next binade
    assert val(0x477FEFFF).to(F16).item() == 65504.0 and math.isinf(val(0x477FF000).to(F16).item())         # around 65 520
    assert val(0x33000000).to(F16).item() == 0.0 and val(0x33000001).to(F16).item() == 2.0 ** -24           # fp16 subnormal ties
    assert val(0x33C00000).to(F16).item() == 2.0 ** -23 and math.isinf(val(0x7F7FFFFF).to(BF16).item())
    assert torch.isnan(b).sum() == 1 and torch.isnan(h).sum() == 1 and (sp == 0).sum() == 2
    assert val(0x007FFFFF).to(BF16).view(torch.int16).item() == 0x0080                                       # an f32 subnormal rounds up to a normal
    sub = val(0x00000001) * f(2.0 ** 64)
    assert sub.item() == 2.0 ** -85                                                                        # 2^64 makes the f32 subnormal normal
    assert (val(0x58000000) * f(2.0 ** -64)).to(F16).item() == 2.0 ** -15 and (val(0x587FE000) * f(2.0 ** -64)).to(F16).item() == 2.0 ** -14                                  # 2^-64 carries a normal into fp16's subnormals
    assert (val(0x1CFFF000) * f(2.0 ** 64)).to(F16).item() == 2.0 ** -5                                       # a tie that rounds up a binade after scaling
    for n in tx.CAST_N:
        x = tx.cast_input(n)
        assert x.shape == (n,)
        if n >= 4 * sp.numel():
            bits = set(x.view(torch.int32).tolist()[-sp.numel():]) | {0x7FC00000 - (1 << 32)}
            assert len(bits) >= sp.numel()                  # the whole table sits in the tail
            mags = x.double().abs()
            assert ((mags > 0) & (mags < 2.0 ** -14)).any() and (mags > 65520).any()


# ----------------------------------------------------------------------------------------------------- exact inputs are exact
def test_exact_inputs_at_every_size():
    for n in tx.ADD_SCALED_N:
        for k in tx.ADD_SCALED_K:
            src, out0, want = tx.add_scaled_case(n, k)
            got = out0 + src * f(2.0 ** k)                       # the kernel's f32 statement
            assert torch.equal(got.double(), want) and (n < 100 or (src != 0).double().mean() > 0.99)
    for form, Bs in tx.IM2COL_B.items():
        for B in Bs:
            if B == 112 or (B >= 55 and form != "bf16-split"):
                continue                                         # the split assertion depends on the values, not on B: run it once per size class
            tx.im2col_ref(tx.im2col_image(B), "split" in form, F16 if "fp16" in form else BF16)
    tx.im2col_ref(tx.im2col_image(56), True, F16)
    for H in tx.MEANPOOL_H:
        for S in tx.MEANPOOL_S:
            for B in tx.MEANPOOL_B:
                d, want = tx.meanpool_bwd_case(B, S, H)
                assert want.shape == (B * S, H) and (want[0] != 0).any()
    for H in tx.EMBED_H:
        for B, S in tx.EMBED_BS:
            for types in (False, True):
                ref64, ref32 = tx.embed_ref(tx.embed_case(B, S, H, "exact", types))
                tx._exact(ref64.abs(), 1.0, "bert_embed")
                assert torch.equal(ref32.double(), ref64)
    for n in tx.ADAMW_N:
        for dtype in (F32, BF16, F16):
            t, want = tx.nonfinite_case(n, dtype)
            assert (want == 0) == (n == 63)


def test_clip_record_can_be_made_exact():
    """For every AdamW size there is an f32 max_norm for which grad_clip_finish's coef, restated, is exactly 0.25."""
    for n in tx.ADAMW_N:
        g0 = tx.adamw_inputs(n)[3]
        g, mn = tx.clip_gradient(g0)
        assert (g != g0).sum() <= 1 and (n == 1 or (g - g0).abs().max() <= 0.1 * g0.abs().max())
        for s in range(tx.ADAMW_STEPS):
            root = tx.adamw_grad(g, s).double().pow(2).sum().sqrt().item()
            assert f(min(1.0, mn / (root + 1e-6))).item() == 0.25


# ---------------------------------------------------------------------------------------------------------------- the bars
def _measure():
    top = {k: 0.0 for k in tx.MEASURED}

    def put(key, got, want, scale):
        top[key] = max(top[key], tx.worst(got, want, scale))

    for n in tx.ADAMW_N:
        p, m, v, g = tx.adamw_inputs(n)
        grads = [tx.adamw_grad(g, s) for s in range(tx.ADAMW_STEPS)]
        for hp, step0 in tx.ADAMW_SETS.values():
            state = (p, m, v)                              # the f32 state runs on, each step is held to f64 on the state it started from
            for s, gr in enumerate(grads):
                (p1, m1, v1), (ps, ms, vs) = tx.adamw_step64(*state, gr, hp, step0 + s)
                state = adamw_step_f32(*state, gr, hp, step0 + s)
                put("adamw_p_ulps", state[0], p1, tx.ulp32(ps))
                put("adamw_m_rel", state[1], m1, ms)
                put("adamw_v_rel", state[2], v1, vs)
    for D in tx.L2_D:
        for M in tx.L2_M:
            x, dy, _ = tx.l2norm_rows(M, D)
            y64, inv64 = tx.l2norm_fwd64(x)
            y32, inv32 = l2norm_fwd_f32(x)
            put("l2norm_fwd_row", y32, y64, tx.rowmax(y64))
            put("l2norm_inv_rel", inv32, inv64, inv64)
            yin, iin = y64.float(), inv64.float()
            dx64 = tx.l2norm_bwd64(yin, iin, dy)
            put("l2norm_bwd_row", l2norm_bwd_f32(yin, iin, dy), dx64, tx.rowmax(dx64))
    for B, S in tx.SOFTMAX_BS:
        dp = tx.softmax_d_pooled(B)
        for scale in tx.SOFTMAX_SCALES:
            x = tx.softmax_logits(B, S, scale)
            pooled64, stats64, _ = tx.softmax_pool64(x, B, S)
            pooled32, stats32 = softmax_fwd_f32(x, B, S)
            assert torch.equal(stats32[:, 0].double(), stats64[:, 0])
            put("softmax_pooled_row", pooled32, pooled64, tx.rowmax(pooled64))
            put("softmax_sum_rel", stats32[:, 1], stats64[:, 1], stats64[:, 1])
            d64, denom = tx.softmax_pool_bwd64(x, dp, B, S)
            put("softmax_bwd_row", softmax_bwd_f32(x, tx.softmax_stats32(x, B, S), dp, B, S), d64, denom)
    for H in tx.MEANPOOL_H:
        for S in tx.MEANPOOL_S:
            for B in tx.MEANPOOL_B:
                x = tx.meanpool_fwd_input(B, S, H)
                want = x.double().view(B, S, H).mean(1)
                put("meanpool_fwd_row", meanpool_fwd_f32(x, B, S), want, tx.rowmax(want))
    return top


def test_bars_are_four_times_the_measured_restatement():
    top = _measure()
    _log("tail_bars", **{k + "_measured": v for k, v in top.items()}, **{k + "_bar": tx.BAR[k] for k in top})
    for k, v in top.items():
        assert 0 < v < float("inf"), (k, v)
        assert math.isclose(tx.MEASURED[k], v, rel_tol=1e-6), f"{k}: tail_exact.MEASURED holds {tx.MEASURED[k]!r}, measured {v!r}"
        assert tx.BAR[k] == 4.0 * tx.MEASURED[k]
    assert top["adamw_p_ulps"] < 16 and max(v for k, v in top.items() if k != "adamw_p_ulps") < 4e-6     # f32 arithmetic, nothing else (the softmax backward's 0.1 |p g| floor allows ten roundings of p g)


# ------------------------------------------------------------------------------------------------ each comparison can fail
def trunc16(x, dtype):
    """A truncating f32 -> 16-bit conversion (toward zero)."""
    h = x.to(dtype)
    over = (h.float().abs() > x.abs()) & torch.isfinite(h.float())
    return torch.where(over, (h.view(torch.int16) - 1).view(dtype), h)


def one_elem(want, rel=2.0 ** -14, median=False):
    """``want`` with its largest finite element (``median``: the one of median magnitude) changed: by ``rel`` relative for f32 / f64, by
    one unit in the last place for 16 bits."""
    got = want.clone()
    flat = got.view(-1)
    mag = torch.where(torch.isfinite(flat.double()), flat.double().abs(), torch.zeros(flat.shape, dtype=F64))
    i = int(mag.argsort()[flat.numel() // 2]) if median else int(mag.argmax())
    if want.element_size() == 2:
        flat.view(torch.int16)[i] -= 1
    else:
        flat[i] = flat[i] * (1 - rel)
    return got


def lane_swap(t, row, lane=7):
    """Row ``row`` with the 4-column pieces of lanes ``lane`` and ``lane + 1`` exchanged (a piece stored one lane off)."""
    got = t.clone()
    a, b = slice(4 * lane, 4 * lane + 4), slice(4 * lane + 4, 4 * lane + 8)
    got[row, a], got[row, b] = t[row, b], t[row, a]
    return got


def row_swap(t, r0, r1):
    got = t.clone()
    got[r0], got[r1] = t[r1], t[r0]
    return got


def test_casts_reject():
    n = tx.CAST_CAP + 1027
    x = tx.cast_input(n)
    for dtype, k in ((BF16, 0), (F16, 0), (F16, 13)):
        want = tx.cast_ref(x, dtype, k)
        assert tx.bits_equal(want.clone(), want)
        tail = want.clone()
        tail[n - (n & 3):] = tx.NAN                                           # the n & 3 tail never written
        second = want.clone()
        second[tx.CAST_CAP:] = tx.NAN                                         # the second pass never written
        again = want.clone()
        again[tx.CAST_CAP:] = tx.cast_ref(x[tx.CAST_CAP:] * f(2.0 ** k), dtype, k)   # ... scaled twice
        tr = trunc16(x * f(2.0 ** k), dtype)
        for got in [tail, second, tr] + ([again] if k else []):
            assert not tx.bits_equal(got, want)
    zero = torch.zeros(4, dtype=BF16)
    assert not tx.bits_equal(-zero, zero) and tx.bits_equal(torch.full((2,), tx.NAN, dtype=F16), (-torch.full((2,), tx.NAN)).to(F16))
    # what test_10 asks of this kernel accepts one truncated element
    y = tx.hash_real(1003, 4).float()
    want = y.to(BF16)
    got = one_elem(want)
    assert rel_err(got, want) < TOL_BF16 and not tx.bits_equal(got, want)


def test_add_scaled_rejects():
    n, k = tx.ADD_SCALED_CAP + 1027, 13
    src, out0, want = tx.add_scaled_case(n, k)
    want = want.float()
    tail, second, twice = want.clone(), want.clone(), want.clone()
    tail[n - (n & 3):] = out0[n - (n & 3):]
    second[tx.ADD_SCALED_CAP:] = out0[tx.ADD_SCALED_CAP:]
    twice[tx.ADD_SCALED_CAP:] += (src * f(2.0 ** k))[tx.ADD_SCALED_CAP:]
    for got in (tail, second, twice, one_elem(want)):
        assert not tx.bits_equal(got, want)
    assert rel_err(one_elem(want), want) < TOL_ADAMW


def test_adamw_rejects():
    n = tx.ADAMW_CAP + 259
    hp, step0 = tx.ADAMW_SETS["defaults"]
    p, m, v, g = tx.adamw_inputs(n)
    before = (p.double(), m.double(), v.double())
    after, scales = tx.adamw_step64(p, m, v, g, hp, step0)
    again, _ = tx.adamw_step64(*after, g, hp, step0)
    allow = tx.adamw_allowances(scales)
    right = [t.float() for t in after]
    for j in range(3):
        assert tx.worst(right[j], after[j], allow[j]) <= 0.5                  # one f32 rounding of the reference passes
        stale, twice = right[j].clone(), right[j].clone()
        stale[tx.ADAMW_CAP:] = before[j][tx.ADAMW_CAP:].float()               # the second pass never ran
        twice[tx.ADAMW_CAP:] = again[j][tx.ADAMW_CAP:].float()                # ... ran twice
        last = right[j].clone()
        last[-1] = before[j][-1].float()                                      # one element missed
        single = one_elem(right[j], 2.0 ** -12, median=True)
        for got in (stale, twice, last, single):
            assert tx.worst(got, after[j], allow[j]) > 1
        assert rel_err(single, after[j]) < TOL_ADAMW
    assert rel_err(torch.cat([right[0][:-1], before[0][-1:].float()]), after[0]) < TOL_ADAMW  # ... which the whole-tensor norm lets through
    # the f32 hyperparameters matter: the reference on a beta2 one f32 ulp away is itself outside the bar
    off = tx.adamw_step64(p, m, v, g, {**hp, "beta2": 0.999 + 6e-8}, step0)[0][2]
    assert tx.worst(off.float(), after[2], allow[2]) > 1


def test_count_and_movers_reject():
    t, want = tx.nonfinite_case(tx.NONFINITE_CAP + 259, BF16)
    first_pass = int((~torch.isfinite(t[:tx.NONFINITE_CAP].float())).sum())
    assert first_pass != want and rel_err(torch.tensor([1000.0 + want - 1]), torch.tensor([1000.0 + want])) < TOL_BF16
    mask, bias = tx.mask_case(257)
    skipped = bias.clone()
    skipped[256] = tx.NAN
    assert not tx.bits_equal(skipped, bias) and not tx.bits_equal(one_elem(bias), bias) and rel_err(one_elem(bias), bias) < TOL_F32
    assert not tx.bits_equal(torch.where(mask == 1, 0.0, tx.F32_MIN).float(), bias)          # "mask == 1" instead of "mask != 0"
    # gather_cast_rows
    p_in, p_out, off, rows = tx.GATHER_CASES[0]
    src = tx.hash_real(tx.gather_src_rows(rows, p_in, p_out, off)[0] * 768, 141).float().view(-1, 768)
    want = tx.gather_ref(src, rows, p_in, p_out, off)
    skip = want.clone()
    skip[rows - 1] = tx.NAN
    r = torch.arange(rows)
    for got in (skip, row_swap(want, 3, 4), lane_swap(want, 5), trunc16(src[(r // p_out) * p_in + off + r % p_out], BF16),
                tx.gather_ref(src, rows, p_in, p_out, 0), one_elem(want)):
        assert not tx.bits_equal(got, want)
    assert rel_err(one_elem(want), want) < TOL_BF16
    # transpose
    w = tx.words16(65, 200, 151)
    want = w.t().contiguous()
    for got in (row_swap(want, 0, 1), lane_swap(want, 2), w.reshape(200, 65)):
        assert not tx.bits_equal(got, want)
    assert rel_err(one_elem(want), want) < TOL_BF16 and not tx.bits_equal(one_elem(want), want)
    assert len(set(w.view(torch.int16)[0].tolist())) > 190 and torch.isfinite(w.float()).all()
    # dgelu_mul, im2col: a skipped second pass, swapped rows, truncation
    g, codes, want = tx.dgelu_case(7, 3072)
    d32 = (codes.double() * (f(1.26) / 255).double() - f(0.13).double()).float()
    for got in (row_swap(want, 1, 2), lane_swap(want, 3), trunc16(g.float() * d32, BF16), one_elem(want)):
        assert not tx.bits_equal(got, want)
    assert rel_err(one_elem(want), want) < TOL_BF16
    img = tx.im2col_image(1)
    for dtype in (BF16, F16):
        want = tx.im2col_ref(img, True, dtype)
        cols = want[:, :768].float() + want[:, 768:1536].float()
        lo_trunc = want.clone()
        lo_trunc[:, :768] = trunc16(cols, dtype)
        lo_trunc[:, 1536:] = lo_trunc[:, :768]
        for got in (row_swap(want, 13, 14), lane_swap(want, 100), lo_trunc, one_elem(want)):
            assert not tx.bits_equal(got, want)
        assert rel_err(one_elem(want), want) < TOL_BF16
    # vit_cls_rows / waug_set_lora_layers: one RNE of an f32; a truncation or a row left alone shows
    t32 = tx.real16_table(768, 4, 161)
    for dtype in (BF16, F16):
        want = t32.to(dtype)
        skip = want.clone()
        skip[767] = tx.NAN
        for got in (trunc16(t32, dtype), skip, row_swap(want, 1, 2), one_elem(want)):
            assert not tx.bits_equal(got, want)
        assert rel_err(one_elem(torch.nan_to_num(want.float(), 0, 0, 0).to(dtype)), torch.nan_to_num(want.float(), 0, 0, 0)) < TOL_BF16


def test_embed_and_meanpool_bwd_reject():
    for kind in ("exact", "real"):
        c = tx.embed_case(3, 43, 768, kind, True)
        _, want = tx.embed_ref(c)
        _, wrapped = tx.embed_ref(c, clamp=False)
        skip = want.clone()
        skip[128] = tx.NAN
        no_types = tx.embed_ref({**c, "type_ids": None})[1]
        raw_types = want - c["typ"][(c["type_ids"].view(-1) != 0).long()] + c["typ"][c["type_ids"].view(-1).clamp(0, 1)]   # tt clamped, not tt ? 1 : 0
        for got in (wrapped, skip, row_swap(want, 5, 6), lane_swap(want, 7), no_types, raw_types, one_elem(want, median=True)):
            assert not tx.bits_equal(got, want)
        assert rel_err(one_elem(want, median=True), want) < TOL_ADAMW
    w, p, y = c["word"][5], c["pos"][7], c["typ"][1]
    assert not torch.equal((w + p) + y, w + (p + y))                     # the order is part of the answer on real inputs
    d, want = tx.meanpool_bwd_case(3, 7, 512)
    twice = want * (f(1.0) / f(7.0))
    divided = (d / 7.0).repeat_interleave(7, 0)                          # a division instead of the multiplication by 1.0f / S
    for got in (twice, divided, row_swap(want, 6, 7), lane_swap(want, 8), one_elem(want, median=True)):
        assert not tx.bits_equal(got, want)
    assert rel_err(one_elem(want, median=True), want) < TOL_ADAMW and rel_err(divided, want) < TOL_ADAMW


def test_toleranced_rows_reject():
    # l2norm
    x, dy, kinds = tx.l2norm_rows(37, 768)
    y64, inv64 = tx.l2norm_fwd64(x)
    dx64 = tx.l2norm_bwd64(y64.float(), inv64.float(), dy)
    for want, key in ((y64, "l2norm_fwd_row"), (dx64, "l2norm_bwd_row")):
        allow = tx.row_allowance(want, tx.BAR[key])
        right = want.float()
        assert tx.worst(right, want, allow) <= 0.25
        skip = right.clone()
        skip[36] = tx.NAN
        single = one_elem(right[:5])                                   # among the ordinary rows test_10 uses
        for got in (skip, row_swap(right, 0, 1), lane_swap(right, 2)):
            assert tx.worst(got, want, allow) > 1
        assert tx.worst(single, want[:5], allow[:5]) > 1 and rel_err(single, want[:5]) < TOL_F32
    no_clamp = (x.double() / x.double().norm(dim=1, keepdim=True)).float()
    assert tx.worst(no_clamp, y64, tx.row_allowance(y64, tx.BAR["l2norm_fwd_row"])) > 1           # 0 / 0 and the tiny row at unit norm
    assert tx.worst(one_elem(inv64.float(), 2.0 ** -18), inv64, tx.BAR["l2norm_inv_rel"] * inv64) > 1
    # softmax pooling
    B, S = 5, 133
    dp = tx.softmax_d_pooled(B)
    for scale in (3.0, 50.0):
        lg = tx.softmax_logits(B, S, scale)
        pooled, stats, _ = tx.softmax_pool64(lg, B, S)
        allow = tx.row_allowance(pooled, tx.BAR["softmax_pooled_row"])
        right = pooled.float()
        assert tx.worst(right, pooled, allow) <= 0.25
        dropped = ((pooled * S - tx.softmax_pool64(lg, B, S)[2].view(B, S, -1)[:, S - 1]) / S).float()     # a token row skipped
        single = one_elem(right)
        for got in (right / S, dropped, row_swap(right, 0, 1), lane_swap(right, 2), single):
            assert tx.worst(got, pooled, allow) > 1
        assert rel_err(single, pooled) < TOL_F32
        d64, denom = tx.softmax_pool_bwd64(lg, dp, B, S)
        allow = tx.BAR["softmax_bwd_row"] * denom + tx.half_ulp_bf16(d64)
        right = d64.float().to(BF16)
        assert tx.worst(right, d64, allow) <= 1
        skip = right.clone()
        skip[B * S - 1] = tx.NAN
        hot = int(d64.abs().amax(1).argmax())
        single = right.clone()
        col = int(d64[hot].abs().argmax())
        single.view(torch.int16)[hot, col] += 2                          # two bf16 ulps on one element
        for got in ((d64 / S).to(BF16), skip, row_swap(right, hot, (hot + 1) % (B * S)), trunc16(d64.float(), BF16), single):
            assert tx.worst(got, d64, allow) > 1
        assert rel_err(single, d64) < TOL_BF16
    # meanpool_tokens_fwd
    B, S, H = 3, 20, 768
    x = tx.meanpool_fwd_input(B, S, H)
    want = x.double().view(B, S, H).mean(1)
    allow = tx.row_allowance(want, tx.BAR["meanpool_fwd_row"], bf16_out=True)
    right = want.float().to(BF16)
    assert tx.worst(right, want, allow) <= 1
    single = right.clone()
    single.view(torch.int16)[1, int(want[1].abs().argmax())] += 2
    dropped = ((want * S - x.double().view(B, S, H)[:, S - 1]) / S).float().to(BF16)
    for got in ((want / S).to(BF16), dropped, row_swap(right, 0, 1), lane_swap(right, 2), trunc16(want.float(), BF16), single):
        assert tx.worst(got, want, allow) > 1
    assert rel_err(single, want) < TOL_BF16
