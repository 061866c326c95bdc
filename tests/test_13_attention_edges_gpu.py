"""Attention kernels at the edges the other attention tests leave out (csrc/attn.hip, csrc/attn_x3.hip, the attention part of
csrc/exact.hip), against ``_attn_ref`` of tests/test_10_kernels_gpu.py in float64 with autograd:

* every key-block count NB = ceil(S / 32) = 1..7 of the generic (TAIL = 32) instantiations, at a ragged and at a full last block
  (S = 31 32 | 33 64 | 65 96 | 100 128 | 129 160 | 161 192 | 223), a one-row last block (33, 65, 129, 161), and the two tail-5 forms
  (133, 197);
* a FINITE additive key bias (2 N(0, 1) on the visible keys, finfo.min on the masked ones): with 0 / finfo.min alone a wrong factor
  on the bias, or a wrong lane -> key mapping of the bias reads, changes nothing;
* scale = 0.1, which is no power of two (1 / scale * scale is not exact, and a constant 0.125 would show);
* a peaked softmax (q and k scaled by sqrt(8): the median row maximum of P is 0.7 .. 0.99, printed per case), where the
  softmax-backward cancellation dS = P (dP - delta) matters and P rounds to exactly 1 or 0, and a forward-only case whose exp2 underflows;
* errors per (sequence, head, 32-row block) slab next to the global normwise ones: one wrong head, one wrong query block or a wrong
  ragged last block is not diluted by the rest;
* strided, sentinel-filled outputs with two spare rows: nothing beyond [B S, heads 64] is written.

Bars.  bf16 kernels: the project's (ctx 6e-3, gradients 1e-2, lse 1e-5 normwise; tests/test_10_kernels_gpu.py), on the global figure
AND on the worst slab.  A CPU emulation of the kernel's rounding points (P -> bf16 for P.V and P^T.dO, delta from the unrounded P,
dS -> bf16, outputs -> bf16) against float64 over S = 7, 65, 161, 224, all kinds and both scales has a worst slab of 3.8e-3 (ctx) and
4.1e-3 (gradients), global figures of 2.1 .. 2.5e-3.  The kernels on an MI355X: global ctx <= 2.2e-3, gradients <= 3.2e-3; worst slab
ctx 3.0e-3, dq 6.0e-3 (S = 129 peaked + biased, the one-row block), dk 3.6e-3, dv 3.6e-3 in the kinds with more than one visible key.
One slab bar is case-dependent: test_attention_bf16_one_visible_key says why, and how it is set from ``_emulate_bwd``, which adds the
kernels' f32 rounding points to that emulation.
The per-row lse bar LSE_ROW_BAR is 4 x the worst row of a float32 torch restatement (f32 scores, f32 ``torch.logsumexp``) of the same
cases on the CPU against float64, |d| / max(1, |lse|): measured 3.28e-7 over every bf16 case of this file (flat 0.9e-7, biased 1.3e-7,
peaked 2.5e-7, one visible key 3.3e-7, underflow 1.9e-7), so the bar is 1.32e-6; the margin covers the kernel's other summation order
and its exp2 / log2 path (the kernels' worst row: 3.0e-7).  The case's own f32 figure is printed with the kernel's.
Exact mode: the bars of test_exact_attention_fwd_bwd_f32 per implementation; for the peaked kind max(that bar, 4 x the error of a
float32 torch restatement of the same case against float64), both printed (the restatement has ctx 9e-7, lse 1e-7, gradients 1.6e-6,
so the existing bars stand).  Slab figures are printed, not asserted, there: the split-bf16 implementation's worst is the one-row
last block of S = 129 / 161 in the peaked kind (dq 2.0e-4 / 2.6e-4, dk 2.5e-4, against 3e-5 globally; the f32-operand implementation
has 1.3e-5 / 2.4e-5 in the same slabs): one query row, no averaging over rows, and dS = P (dP - delta) cancels most of dP there.

Every figure is printed, one ``FIGURES`` JSON line per case, before it is asserted (``pytest -s`` shows them)."""
import functools
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_err  # noqa: E402
from test_10_kernels_gpu import _attn_ref  # noqa: E402

B, HEADS = 2, 3          # an odd head count: a head-stride error cannot land on another head's start
H = HEADS * 64
FMIN = torch.finfo(torch.float32).min
SENT = -123.0            # exact in bf16
TOL_CTX, TOL_G, TOL_LSE = 6e-3, 1e-2, 1e-5      # tests/test_10_kernels_gpu.py::test_attention_fwd_bwd
LSE_ROW_F32 = 3.3e-7     # worst row of the f32 restatement over this file's bf16 cases (CPU, against f64): 3.28e-7, one visible key
LSE_ROW_BAR = 4 * LSE_ROW_F32
EXACT_BARS = {0: (5e-5, 1e-5, 2e-4), 2: (2e-5, 1e-6, 3e-5)}   # (ctx, lse, gradients): test_exact_attention_fwd_bwd_f32

# kind -> (gain on q.k, finite key bias)
KINDS = {"flat": (1.0, False), "peaked": (8.0, False), "biased": (1.0, True), "peaked_biased": (8.0, True), "underflow": (40.0, False)}
S_GENERIC = (31, 32, 33, 64, 65, 96, 100, 128, 129, 160, 161, 192, 223)
S_TAIL5 = (133, 197)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    return o


def _log(test, **figures):
    print("FIGURES " + json.dumps({"test": test, **figures}))


@functools.lru_cache(maxsize=None)
def _inputs(S, kind, onehot=False, rounded=True):
    """(qkv [B S, 3H], dctx [B S, H], key_bias [B, S] or None) on the CPU in f32; ``rounded``: to bf16 values (what the bf16 kernels
    are given).  biased kinds: sequence 0 fully visible, sequence 1 a random prefix in [1, S) (``onehot``: 1 key)."""
    gain, biased = KINDS[kind]
    g = torch.Generator().manual_seed(1000 * S + 10 * sorted(KINDS).index(kind) + int(onehot))
    qkv = torch.randn(B * S, 3 * H, generator=g)
    qkv[:, :2 * H] *= math.sqrt(gain)
    dctx = torch.randn(B * S, H, generator=g)
    if rounded:
        qkv, dctx = qkv.bfloat16().float(), dctx.bfloat16().float()
    bias = None
    if biased:
        lens = torch.tensor([S, 1 if onehot else int(torch.randint(1, S, (1,), generator=g))])
        visible = torch.arange(S)[None] < lens[:, None]
        bias = torch.where(visible, 2 * torch.randn(B, S, generator=g), torch.full((B, S), FMIN))
    return qkv, dctx, bias


def _restate(S, kind, scale, onehot, rounded, dtype, grads):
    qkv, dctx, bias = _inputs(S, kind, onehot, rounded)
    x = qkv.to(dtype).reshape(B, S, 3 * H).requires_grad_(grads)
    ctx, lse = _attn_ref(x, B, S, HEADS, scale, None if bias is None else bias.to(dtype))
    g = torch.autograd.grad(ctx, x, dctx.to(dtype))[0].reshape(B * S, 3 * H) if grads else None
    return ctx.detach(), lse.detach(), g


@functools.lru_cache(maxsize=None)
def _reference(S, kind, scale, onehot=False, rounded=True, grads=True):
    """float64 ctx / lse / d[q | k | v] of a case, computed once (read only), the median row maximum of P, and the float32
    restatement's worst lse row."""
    ctx, lse, g = _restate(S, kind, scale, onehot, rounded, torch.float64, grads)
    qkv, _, bias = _inputs(S, kind, onehot, rounded)
    q, k, _ = [t.reshape(B, S, HEADS, 64).transpose(1, 2) for t in qkv.double().split(H, dim=-1)]
    s = (q @ k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    p_max = (s.max(-1).values - lse).exp().median().item()
    _, lse32, _ = _restate(S, kind, scale, onehot, rounded, torch.float32, False)
    return dict(ctx=ctx, lse=lse, g=g, p_max=p_max, lse_row_f32=_lse_row(lse32, lse))


def _lse_row(got, ref):
    return ((got.double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()


def _slabs(got, ref, S, floor):
    """Worst normwise error over the (sequence, head, 32-row block) slabs [<= 32, 64] of a [B S, heads 64] tensor, and where."""
    d = (got.double().cpu() - ref).reshape(B, S, -1, 64)
    r = ref.reshape(B, S, -1, 64)
    worst, where = 0.0, None
    for blk in range((S + 31) // 32):
        rows = slice(32 * blk, 32 * blk + 32)
        e = d[:, rows].pow(2).sum((1, 3)).sqrt() / (r[:, rows].pow(2).sum((1, 3)).sqrt() + floor)   # [B, heads]
        if e.max().item() >= worst:
            worst = e.max().item()
            where = [int(e.argmax()) // e.shape[1], int(e.argmax()) % e.shape[1], blk]
    return worst, where


def _parts(t):
    return (("dq", t[:, :H]), ("dk", t[:, H:2 * H]), ("dv", t[:, 2 * H:3 * H]))


def _mfma_chain(a, b, start):
    """start + a b^T as the kernels' MFMA chains form it: four steps of 16 k, the running f32 sum rounded after each."""
    acc = start
    for ks in range(4):
        cols = slice(16 * ks, 16 * ks + 16)
        acc = (acc.double() + a[..., cols].double() @ b[..., cols].double().transpose(-1, -2)).float()
    return acc


def _emulate_bwd(S, kind, scale, onehot):
    """d[q | k | v] of a case with the f32 AND the bf16 rounding points of attn_fwd_kernel / attn_bwd_kernel (csrc/attn.hip), on the CPU:
    the score accumulator starts from bias / scale; lse is stored as a natural-log f32 and taken back to the log2 domain; P from one fma
    and an exp2; delta from the unrounded P; the query-owner phase forms dS = bf16(P) (dP - delta), the key-owner phase starts the dP
    accumulator from -delta (dS = P dP'); dS -> bf16, P -> bf16 for P^T dO, outputs -> bf16.  Nothing here comes from the kernel."""
    qkv, dctx, bias = _inputs(S, kind, onehot)
    q, k, v = [t.reshape(B, S, HEADS, 64).transpose(1, 2) for t in qkv.split(H, dim=-1)]
    do = dctx.reshape(B, S, HEADS, 64).transpose(1, 2)
    f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    sc, log2e, ln2 = f(scale), f(math.log2(math.e)), f(math.log(2.0))
    scale2 = sc * log2e
    zero = torch.zeros(B, HEADS, S, S)
    acc = _mfma_chain(q, k, zero if bias is None else (bias * (1.0 / sc))[:, None, None, :].expand(B, HEADS, S, S))
    fma = lambda x, y, z: (x.double() * y.double() + z.double()).float()   # noqa: E731
    nm2 = -(acc.max(-1, keepdim=True).values * scale2)
    lse = (torch.log2(torch.exp2(fma(acc, scale2, nm2)).sum(-1, keepdim=True)) - nm2) * ln2
    p = torch.exp2(fma(acc, scale2, -(lse * log2e)))
    dp = _mfma_chain(do, v, zero)
    delta = torch.zeros(B, HEADS, S, 1)
    for key in range(S):
        delta = fma(p[..., key:key + 1], dp[..., key:key + 1], delta)
    pb = p.bfloat16().float()
    ds_q = (pb * (dp - delta)).bfloat16().float()
    ds_k = (p * _mfma_chain(do, v, (-delta).expand(B, HEADS, S, S))).bfloat16().float()
    parts = ((ds_q @ k) * sc, (ds_k.transpose(-1, -2) @ q) * sc, pb.transpose(-1, -2) @ do)
    return torch.cat([t.transpose(1, 2).reshape(B * S, H) for t in parts], -1).bfloat16().float()


# ------------------------------------------------------------------------------------- 2. bf16 kernels: attn_fwd / attn_bwd
def _bf16_case(ops, S, kind, scale, onehot=False, backward=True):
    qkv, dctx, bias = _inputs(S, kind, onehot)
    ref = _reference(S, kind, scale, onehot, True, backward)
    R = B * S
    name = f"attn_bf16 S={S} {kind}{' onehot' if onehot else ''} scale={scale}"
    slab_bar, emul = dict(dq=TOL_G, dk=TOL_G, dv=TOL_G), {}
    if onehot:      # see test_attention_bf16_one_visible_key
        floor = 1e-5 * ref["g"].norm()
        for (n, got), (_, want) in zip(_parts(_emulate_bwd(S, kind, scale, onehot)), _parts(ref["g"])):
            emul[n + "_slab"], emul[n + "_slab_at"] = _slabs(got, want, S, floor)
        for n in ("dq", "dk"):
            slab_bar[n] = max(TOL_G, 2 * emul[n + "_slab"])

    def padded(t, ld):
        buf = torch.zeros(R, ld, device="cuda", dtype=torch.bfloat16)
        buf[:, :t.shape[1]] = t.cuda()
        return buf[:, :t.shape[1]]
    qkv_d, dctx_d = padded(qkv, 3 * H + 64), padded(dctx, H + 64)
    bias_d = None if bias is None else bias.cuda()
    ctx = torch.full((R + 2, H + 64), SENT, device="cuda", dtype=torch.bfloat16)
    lse = torch.full((B * HEADS * S + 64,), SENT, device="cuda")
    ops.attn_fwd(qkv_d, B, S, HEADS, scale, ctx[:, :H], lse, key_bias=bias_d)
    lse_v = lse[:B * HEADS * S].view(B, HEADS, S)
    c = ctx[:R, :H].float().cpu()
    fig = dict(NB=(S + 31) // 32, p_max_median=ref["p_max"],
               ctx=rel_err(c, ref["ctx"]), lse=rel_err(lse_v, ref["lse"]), lse_row=_lse_row(lse_v, ref["lse"]),
               lse_row_f32=ref["lse_row_f32"])
    fig["ctx_slab"], fig["ctx_slab_at"] = _slabs(c, ref["ctx"], S, 1e-5 * ref["ctx"].norm())
    clean = bool((ctx[:, H:] == SENT).all() and (ctx[R:] == SENT).all() and (lse[B * HEADS * S:] == SENT).all())
    finite = bool(torch.isfinite(c).all() and torch.isfinite(lse_v).all())
    if backward:
        dqkv = torch.full((R + 2, 3 * H + 64), SENT, device="cuda", dtype=torch.bfloat16)
        ops.attn_bwd(qkv_d, dctx_d, lse_v, B, S, HEADS, scale, dqkv[:, :3 * H], key_bias=bias_d)
        clean = clean and bool((dqkv[:, 3 * H:] == SENT).all() and (dqkv[R:] == SENT).all())
        d = dqkv[:R, :3 * H].float().cpu()
        finite = finite and bool(torch.isfinite(d).all())
        floor = 1e-5 * ref["g"].norm()       # zero gradient parts (one visible key: dq = dk = 0) are measured against the whole gradient
        for (n, got), (_, want) in zip(_parts(d), _parts(ref["g"])):
            fig[n] = ((got.double() - want).norm() / (want.norm() + floor)).item()
            fig[n + "_slab"], fig[n + "_slab_at"] = _slabs(got, want, S, floor)
    _log(name, **fig, bars=dict(ctx=TOL_CTX, grad=TOL_G, lse=TOL_LSE, lse_row=LSE_ROW_BAR, grad_slab=slab_bar), emulation=emul,
         slab_at="[sequence, head, block]")
    assert clean, "padding columns or spare rows of ctx / lse / dqkv written"
    assert finite, "non-finite output"
    assert fig["ctx"] < TOL_CTX and fig["ctx_slab"] < TOL_CTX, (fig["ctx"], fig["ctx_slab"], fig["ctx_slab_at"])
    assert fig["lse"] < TOL_LSE and fig["lse_row"] < LSE_ROW_BAR, (fig["lse"], fig["lse_row"])
    if backward:
        for n in ("dq", "dk", "dv"):
            assert fig[n] < TOL_G and fig[n + "_slab"] < slab_bar[n], (n, fig[n], fig[n + "_slab"], fig[n + "_slab_at"], slab_bar[n])


@pytest.mark.parametrize("kind,scale", [("flat", 0.125), ("peaked", 0.125), ("biased", 0.125), ("peaked_biased", 0.125), ("biased", 0.1)])
@pytest.mark.parametrize("S", S_GENERIC + S_TAIL5)
def test_attention_bf16_every_block_count(ops, S, kind, scale):
    _bf16_case(ops, S, kind, scale)


@pytest.mark.parametrize("S", S_GENERIC + S_TAIL5)
def test_attention_bf16_one_visible_key(ops, S):
    """Sequence 1 sees one key: P is one-hot there and dq = dk = 0, so its slabs are measured against the floor 1e-5 |g| alone, and
    the bar of 1e-2 asks for 1e-7 of the gradient's norm: f32 rounding.  What the kernel leaves there is dS = -eps dP for P = 1 + eps:
    the score accumulator holds q.k + bias / scale, lse comes back from a natural-log f32, and the key-owner phase rounds its dP chain
    at the magnitude of delta.  Measured on the GPU: every size stays below 5.1e-3 but S = 33, where the only visible key's bias is a
    3 sigma draw (-5.98): |q.k + bias / scale| ~ 48 and |lse| log2 e ~ 8.6, so eps ~ 5e-7, and the slab (sequence 1, head 2, block 0)
    has dq 8.8e-3, dk 1.14e-2 with global figures of 3.0e-3 and 2.4e-3.  ``_emulate_bwd`` has those rounding points and puts the same
    slab at 7.2e-3 / 7.5e-3 (and the other sizes' worst slabs within 30 % of the kernel's), so the slab bar of dq and dk is
    max(1e-2, 2 x the emulation's worst slab of the same case) here: 1.44e-2 / 1.5e-2 at S = 33, 1e-2 at every other size.  Global
    bars, the dv and ctx slabs and every other test keep 1e-2 / 6e-3."""
    _bf16_case(ops, S, "biased", 0.125, onehot=True)


@pytest.mark.parametrize("S", [65, 224])
def test_attention_bf16_forward_underflow(ops, S):
    """Scores ~ N(0, 40^2): exp2 underflows for all but a few keys of a row.  Forward only."""
    _bf16_case(ops, S, "underflow", 0.125, backward=False)


# ----------------------------------------------------------------- 4. exact mode: attn_fwd_f32 / attn_bwd_f32, impl 0 and impl 2
def _grad_errs(got, want):
    """The gradient measure of test_exact_attention_fwd_bwd_f32: each part against max(its norm, 1e-2 of the whole gradient's)."""
    return {n: ((g.double() - w).norm() / torch.maximum(w.norm(), 1e-2 * want.norm())).item()
            for (n, g), (_, w) in zip(_parts(got), _parts(want))}


@pytest.mark.parametrize("kind,scale", [("flat", 0.125), ("peaked", 0.125), ("biased", 0.125), ("biased", 0.1)])
@pytest.mark.parametrize("S", [65, 100, 129, 161, 192])
def test_exact_attention_every_block_count(ops, S, kind, scale):
    """f32 operands (not rounded to bf16); both implementations against float64 and against each other."""
    qkv, dctx, bias = _inputs(S, kind, False, False)
    ref = _reference(S, kind, scale, False, False, True)
    R = B * S
    qkv_d = torch.zeros(R, 3 * H + 64, device="cuda")
    qkv_d[:, :3 * H] = qkv.cuda()
    qkv_d = qkv_d[:, :3 * H]
    dctx_d = dctx.cuda()
    bias_d = None if bias is None else bias.cuda()
    f32 = dict(ctx=0.0, lse=0.0, grad=0.0)
    if kind == "peaked":     # the bars of the flat kind are not established here: what f32 arithmetic itself loses, restated in torch
        c32, l32, g32 = _restate(S, kind, scale, False, False, torch.float32, True)
        f32 = dict(ctx=rel_err(c32, ref["ctx"]), lse=rel_err(l32, ref["lse"]), grad=max(_grad_errs(g32, ref["g"]).values()))
    out, figs, bars = {}, {}, {}
    for impl in (0, 2):
        ops.exact_attn_set_impl(impl)        # (tests/conftest.py resets the switch after every GPU test)
        ctx = torch.empty(R, H, device="cuda")
        lse = torch.empty(B, HEADS, S, device="cuda")
        c3 = torch.full((R, 3 * H + 8), float("nan"), device="cuda", dtype=torch.bfloat16)[:, :3 * H]
        ops.attn_fwd_f32(qkv_d, B, S, HEADS, scale, ctx, lse, key_bias=bias_d, ctx_split3=c3)
        assert torch.equal(c3, ops.split3_rows(ctx, torch.empty(R, 3 * H, device="cuda", dtype=torch.bfloat16)))
        dqkv = torch.full((R, 3 * H), float("nan"), device="cuda")
        d3 = torch.full((R, 9 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
        ops.attn_bwd_f32(qkv_d, dctx_d, ctx, lse, B, S, HEADS, scale, dqkv, key_bias=bias_d, dqkv_split3=d3)
        assert torch.equal(d3, ops.split3_rows(dqkv, torch.empty(R, 9 * H, device="cuda", dtype=torch.bfloat16)))
        out[impl] = (ctx.cpu(), lse.cpu(), dqkv.cpu())
        fig = dict(ctx=rel_err(ctx, ref["ctx"]), lse=rel_err(lse, ref["lse"]), lse_row=_lse_row(lse, ref["lse"]),
                   **_grad_errs(out[impl][2], ref["g"]))
        fig["ctx_slab"], fig["ctx_slab_at"] = _slabs(out[impl][0], ref["ctx"], S, 1e-5 * ref["ctx"].norm())
        for (n, got), (_, want) in zip(_parts(out[impl][2]), _parts(ref["g"])):
            fig[n + "_slab"], fig[n + "_slab_at"] = _slabs(got, want, S, 1e-5 * ref["g"].norm())
        figs[impl] = fig
        bars[impl] = dict(zip(("ctx", "lse", "grad"), (max(b, 4 * f32[n]) for b, n in zip(EXACT_BARS[impl], ("ctx", "lse", "grad")))))
    cross = dict(ctx=rel_err(out[0][0], out[2][0]), lse=rel_err(out[0][1], out[2][1]),
                 **{n: rel_err(a, b) for (n, a), (_, b) in zip(_parts(out[0][2]), _parts(out[2][2]))})
    _log(f"attn_exact S={S} {kind} scale={scale}", NB=(S + 31) // 32, p_max_median=ref["p_max"], impl0=figs[0], impl2=figs[2],
         impl0_vs_impl2=cross, f32_restatement=f32, existing_bars={i: EXACT_BARS[i] for i in (0, 2)}, bars=bars)
    for impl in (0, 2):
        f, b = figs[impl], bars[impl]
        assert f["ctx"] < b["ctx"] and f["lse"] < b["lse"], (impl, f["ctx"], f["lse"], b)
        for n in ("dq", "dk", "dv"):
            assert f[n] < b["grad"], (impl, n, f[n], b)
    assert cross["ctx"] < bars[0]["ctx"] + bars[2]["ctx"] and cross["lse"] < bars[0]["lse"] + bars[2]["lse"], cross
    for n in ("dq", "dk", "dv"):
        assert cross[n] < bars[0]["grad"] + bars[2]["grad"], (n, cross)
