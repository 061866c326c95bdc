"""Kernel-level tests of the fp8 (e4m3) entry points (BASELINE.json configs[4]): the LayerNorm that writes e4m3 operands, the LoRA
gradient kernels that decode them, the LoRA-B augmentation tile, and the fp8 GEMM / row quantiser at the shapes the engines really
call them with (a handful of rows, strided operands, dropout).  The encoder-level gates of tests/test_45_fp8_gpu.py allow tens of
per cent because e4m3 is noisy; here nothing is noisy: an e4m3 code is a rounding of an f32 value the kernel also writes out (so
codes are compared bit for bit with tests/fp8_oracle.py), and products of e4m3 values are exact in f32 (so a kernel fed e4m3
operands is held to the bars of its bf16 twin in tests/test_10_kernels_gpu.py against f64 arithmetic on the dequantised operands).
Every toleranced figure is printed, one JSON line per case, before it is asserted (``pytest -s`` shows them)."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp8_oracle  # noqa: E402
from helpers import rel_err  # noqa: E402

TOL_F32 = 2e-5      # f32 outputs (tests/test_10_kernels_gpu.py)
TOL_BF16 = 4e-3     # bf16 outputs
TOL_DT, TOL_DAB = 1e-5, 1e-4   # test_lora_grad
TOL_KEEP = 5e-3     # dropout keep rate (tests/test_40_dropout_gpu.py)
SENT8 = 0x55        # sentinel byte of fp8 / aux buffers (a finite e4m3 code, neither zero nor a bound)
P = 0.1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    o.init_tables()
    return o


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def grnd(*shape, seed=0):
    """Large operands: drawn on the GPU (deterministic for a seed)."""
    return torch.randn(*shape, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))


def _log(test, **figures):
    print("FIGURES " + json.dumps({"test": test, **figures}))


def u8(t):
    return t.view(torch.uint8)


def fp8_buf(ops, rows, ld):
    """An e4m3 buffer [rows, ld] holding the sentinel byte everywhere."""
    return torch.full((rows, ld), SENT8, dtype=torch.uint8, device="cuda").view(ops.FP8)


def is_nan_code(c):
    return (c & 0x7F) == 0x7F


# ------------------------------------------------------------------------------------------------------- 1. LayerNorm -> e4m3
SENT_F = -123.0


def _ln_case(ops, H, eps, M, xbf16, ld_t, seed=1, gamma=None, beta=None, dropout=None, x=None):
    """One layernorm_fwd_fp8 call on strided, sentinel-filled buffers (two spare rows each).  Returns everything a caller checks."""
    ldx, ldy = H + 8, H + 16
    xb = (grnd(M + 2, ldx, seed=seed) * 2 + 0.3)
    if x is not None:
        xb[:M, :H] = x
    if xbf16:
        xb = xb.bfloat16()
    xv = xb[:, :H]
    g = gamma if gamma is not None else 1 + 0.1 * rnd(H, seed=2)
    b = beta if beta is not None else 0.1 * rnd(H, seed=3)
    A = rnd(8, H, seed=4, scale=0.05) if ld_t else None
    y8 = fp8_buf(ops, M + 2, ldy)
    t = torch.full((M + 2, ld_t), 7.0, dtype=torch.bfloat16, device="cuda") if ld_t else None
    y32 = torch.full((M + 2, H), SENT_F, device="cuda")
    stats = torch.full((M + 2, 2), SENT_F, device="cuda")
    ops.layernorm_fwd_fp8(xv, g, b, eps, y8, t_aug=t, y_f32=y32, lora_a=A, stats=stats, M=M, dropout=dropout)
    # the ViT engine's form of the call: no f32 copy, no statistics
    y8b = fp8_buf(ops, M + 2, ldy)
    tb = torch.full_like(t, 7.0) if ld_t else None
    ops.layernorm_fwd_fp8(xv, g, b, eps, y8b, t_aug=tb, lora_a=A, M=M, dropout=dropout)
    torch.cuda.synchronize()
    return dict(x=xv[:M], g=g, b=b, A=A, y8=u8(y8), y8b=u8(y8b), t=t, tb=tb, y32=y32, stats=stats)


def _ln_untouched(r, M, H, ld_t):
    assert (r["y8"][:, H:] == SENT8).all() and (r["y8b"][:, H:] == SENT8).all(), "padding columns of y_fp8 written"
    assert (r["y8"][M:] == SENT8).all() and (r["y8b"][M:] == SENT8).all(), "rows >= M of y_fp8 written"
    assert (r["y32"][M:] == SENT_F).all() and (r["stats"][M:] == SENT_F).all(), "rows >= M of y_f32 / stats written"
    if ld_t:
        assert (r["t"][M:] == 7.0).all() and (r["tb"][M:] == 7.0).all(), "rows >= M of t_aug written"
        assert (r["t"][:M, 8:64] == 0).all()
        assert (r["t"][:, 64:] == 7.0).all(), "t_aug columns >= 64 written"


@pytest.mark.parametrize("ld_t", [0, 64, 128])
@pytest.mark.parametrize("xbf16", [False, True])
@pytest.mark.parametrize("H,eps", [(768, 1e-6), (512, 1e-12)])
def test_layernorm_fwd_fp8(ops, H, eps, xbf16, ld_t):
    """M = 1; 3 (fewer rows than a workgroup has waves); 1031; and one row count just past the grid cap (256 * 5 workgroups of 4 rows
    with LoRA, 256 * 8 without), where the first waves take a second row and the rest do not (the ``row + nwaves < M`` prefetch)."""
    worst = dict(y32=0.0, mean=0.0, rstd=0.0, t=0.0)
    for M in (1, 3, 1031, 5125 if ld_t else 8195):
        r = _ln_case(ops, H, eps, M, xbf16, ld_t, seed=M)
        xd = r["x"].double()
        ref = torch.nn.functional.layer_norm(xd, (H,), r["g"].double(), r["b"].double(), eps)
        y32 = r["y32"][:M]
        worst["y32"] = max(worst["y32"], rel_err(y32, ref))
        worst["mean"] = max(worst["mean"], rel_err(r["stats"][:M, 0], xd.mean(-1)))
        worst["rstd"] = max(worst["rstd"], rel_err(r["stats"][:M, 1], (xd.var(-1, unbiased=False) + eps).rsqrt()))
        # the e4m3 operand is a rounding of exactly the f32 value the same call wrote: no tolerance
        want = fp8_oracle.e4m3_codes(y32)
        got = r["y8"][:M, :H]
        assert torch.equal(got, want), (M, (got != want).sum().item(), y32[got != want][:4], got[got != want][:4], want[got != want][:4])
        assert torch.equal(r["y8b"][:M, :H], got), "the call without y_f32 / stats gives other codes"
        _ln_untouched(r, M, H, ld_t)
        if ld_t:
            worst["t"] = max(worst["t"], rel_err(r["t"][:M, :8].float(), y32.double() @ r["A"].double().t()))
            assert torch.equal(r["tb"][:M, :64], r["t"][:M, :64])
    _log(f"layernorm_fwd_fp8 H={H} xbf16={xbf16} ld_t={ld_t}", **worst, bars=dict(y32=TOL_F32, mean=1e-4, rstd=1e-4, t=TOL_BF16))
    assert worst["y32"] < TOL_F32 and worst["mean"] < 1e-4 and worst["rstd"] < 1e-4 and worst["t"] < TOL_BF16, worst


def test_layernorm_fwd_fp8_saturates_at_448(ops):
    """gamma ~ 300: the normalised row is ~ N(0, 1), so ~ 13 % of the outputs lie beyond +-448 (|z| > 1.49).  They must come out as
    the largest finite code with their sign, never as the NaN code the bare conversion instruction gives an overflow."""
    H, M, eps = 768, 67, 1e-6
    g = 300 * (1 + 0.1 * rnd(H, seed=12))
    b = torch.zeros(H, device="cuda")
    r = _ln_case(ops, H, eps, M, False, 64, seed=11, gamma=g, beta=b)
    ref = torch.nn.functional.layer_norm(r["x"].float().cpu(), (H,), g.cpu(), b.cpu(), eps)      # f32, on the CPU
    share = (ref.abs() > 448).float().mean().item()
    assert share > 0.01, share
    y32, got = r["y32"][:M], r["y8"][:M, :H]
    assert rel_err(y32, ref) < TOL_F32
    over = (ref.abs() > 449).cuda()      # one unit clear of the bound: the kernel's own f32 value is beyond it as well
    assert (y32[over].abs() > 448).all()
    assert torch.equal(got[over], torch.where(ref.cuda()[over] > 0, 0x7E, 0xFE).to(torch.uint8))
    assert not is_nan_code(got).any()
    assert torch.equal(got, fp8_oracle.e4m3_codes(y32))
    _ln_untouched(r, M, H, 64)
    _log("layernorm_fwd_fp8 saturation", share_beyond_448=share, y32=rel_err(y32, ref), bars=dict(y32=TOL_F32))


@pytest.mark.parametrize("H,xbf16", [(768, False), (512, True)])
def test_layernorm_fwd_fp8_dropout(ops, H, xbf16):
    """HF BertEmbeddings' dropout(LayerNorm(.)): the e4m3 operand, the f32 copy and the bf16 kernel draw one mask for one (p, seed).
    beta = 8 keeps every output at least one unit away from zero (checked), so a zero -- in f32 or as an e4m3 code, which also
    rounds |y| < 2^-10 to zero -- is a dropped element and nothing else."""
    M, eps, seed = 517, 1e-12, 7
    g, b = 1 + 0.1 * rnd(H, seed=2), 8 + 0.1 * rnd(H, seed=3)
    r = _ln_case(ops, H, eps, M, xbf16, 64, seed=5, gamma=g, beta=b, dropout=(P, seed))
    ref = torch.nn.functional.layer_norm(r["x"].double(), (H,), g.double(), b.double(), eps)
    assert ref.abs().min().item() > 1.0
    y32, got = r["y32"][:M], r["y8"][:M, :H]
    kept = y32 != 0
    assert torch.equal(got, fp8_oracle.e4m3_codes(y32))
    assert torch.equal(fp8_oracle.e4m3_values(got) != 0, kept), "zero pattern of the e4m3 operand != zero pattern of y_f32"
    assert torch.equal(r["y8b"][:M, :H], got)
    # the bf16 kernel, same (p, seed), same [M, H]
    y32b = torch.empty(M, H, device="cuda")
    ops.layernorm_fwd(r["x"], g, b, eps, y_f32=y32b, dropout=(P, seed))
    assert torch.equal(y32b != 0, kept), "mask differs from bsclip_layernorm_fwd's"
    rate = kept.float().mean().item()
    surv = rel_err(y32[kept], (ref / (1 - P))[kept])
    t_err = rel_err(r["t"][:M, :8].float(), y32.double() @ r["A"].double().t())     # t from the DROPPED activations
    t_undropped = rel_err(r["t"][:M, :8].float(), ref @ r["A"].double().t())
    _log(f"layernorm_fwd_fp8 dropout H={H}", keep_rate=rate, survivors=surv, t=t_err, t_vs_undropped=t_undropped,
         bars=dict(keep_rate=TOL_KEEP, survivors=TOL_F32, t=TOL_BF16))
    assert abs(rate - (1 - P)) < TOL_KEEP and surv < TOL_F32 and t_err < TOL_BF16
    assert t_undropped > 10 * TOL_BF16, "the check above cannot tell dropped from undropped activations"
    ops.layernorm_fwd_fp8(r["x"], g, b, eps, fp8_buf(ops, M, H), y_f32=y32b, M=M, dropout=(P, seed + 1))
    assert ((y32b != 0) != kept).float().mean().item() > 0.1, "another seed must give another mask"
    _ln_untouched(r, M, H, 64)


def test_layernorm_fwd_fp8_nan_and_inf(ops):
    """A NaN must stay visible in the e4m3 operand (code 0x7f / 0xff): BSCLIP_DETECT_ANOMALY looks downstream of it.  One NaN and one
    +inf in x: LayerNorm's mean and variance of such a row are NaN, so the whole row is (y_f32 says so too).  +inf / -inf in beta make
    one column +inf / -inf in every other row: those saturate to +-448.  Nothing else may change."""
    H, M, eps = 768, 9, 1e-6
    clean = _ln_case(ops, H, eps, M, False, 64, seed=21)
    x = clean["x"].clone()
    x[2, 100], x[5, 700] = float("nan"), float("inf")
    b = clean["b"].clone()
    b[33], b[600] = float("inf"), float("-inf")
    r = _ln_case(ops, H, eps, M, False, 64, seed=21, beta=b, x=x)
    y32, got = r["y32"][:M], r["y8"][:M, :H]
    bad = torch.zeros(M, dtype=torch.bool, device="cuda")
    bad[2] = bad[5] = True
    cols = torch.ones(H, dtype=torch.bool, device="cuda")
    cols[33] = cols[600] = False
    assert torch.isnan(y32[bad]).all() and torch.isfinite(y32[~bad][:, cols]).all()
    assert (y32[~bad][:, 33] == float("inf")).all() and (y32[~bad][:, 600] == float("-inf")).all()
    assert (got[~bad][:, 33] == 0x7E).all() and (got[~bad][:, 600] == 0xFE).all(), "+-inf must saturate to +-448"
    assert torch.equal(got[~bad][:, cols], clean["y8"][:M, :H][~bad][:, cols]), "a NaN / inf leaked into another row or column"
    assert is_nan_code(got[bad]).all(), ("NaN rows must carry the NaN code", got[bad][:, :8])
    assert torch.equal(r["y8b"][:M, :H], got)
    _ln_untouched(r, M, H, 64)
    # ... and the NaN code is a NaN to the GEMM that reads the operand: its rows come out NaN, the others (448s included) finite
    from bioscanclip.hip.lib import EPI_F32
    w8, ws = ops.quantize_rows_fp8(rnd(256, H, seed=22, scale=0.05))
    for form in (1, 2):
        out = torch.zeros(M, 256, device="cuda")
        ops.gemm_fp8(r["y8"].view(ops.FP8), w8, out, ws, torch.zeros(256, device="cuda"), EPI_F32, M=M, K=H, form=form)
        assert torch.isnan(out[bad]).all() and torch.isfinite(out[~bad]).all(), form


# ------------------------------------------------------------------------------------------------------- 2. LoRA gradients
def _asym_codes(ops, M, H, ld, seed):
    """Random e4m3 rows [M, ld bytes] whose four columns of every group of four differ in offset and scale, so that a decode that
    takes a byte from the wrong position cannot cancel in a sum."""
    col = torch.arange(H, device="cuda") % 4
    y = grnd(M, H, seed=seed) * (0.5 + 0.25 * col) + torch.tensor([0.5, -1.0, 2.0, -3.0], device="cuda")[col]
    buf = fp8_buf(ops, M + 1, ld)
    u8(buf)[:M, :H] = u8(y.to(ops.FP8))
    return buf


@pytest.mark.parametrize("M", [1, 31, 100, 2077, 24583])
@pytest.mark.parametrize("H", [768, 512])
def test_lora_grad_fp8(ops, H, M):
    """M: one row; fewer rows than a workgroup's 32; a partial three-row prefetch group; the interior; more than LG_MAX_BLOCKS * 32 =
    24576, so waves loop.  M = 100 takes y_fp8 / t_aug from layernorm_fwd_fp8, the others random codes.  ld_t alternates 64 / 128."""
    ld_t = 128 if M in (31, 2077) else 64
    ld_g, ld_y = 3 * H + 8, H + 16
    dqkv = (grnd(M + 1, ld_g, seed=1)).bfloat16()[:, :3 * H]
    lb = rnd(2, H, 4, seed=3, scale=0.1)
    if M == 100:
        r = _ln_case(ops, H, 1e-6, M, False, ld_t, seed=9)
        y8, t = r["y8"].view(ops.FP8), r["t"]
    else:
        y8 = _asym_codes(ops, M, H, ld_y, seed=2)
        t = torch.full((M + 1, ld_t), 7.0, dtype=torch.bfloat16, device="cuda")
        t[:M, :8] = grnd(M, 8, seed=4).bfloat16()
        t[:M, 8:64] = 0

    def run(n_calls=1):
        dt = torch.full((M + 1, 8), float("nan"), device="cuda")
        acc = [torch.zeros(8, H, device="cuda"), torch.zeros(H, 4, device="cuda"), torch.zeros(H, 4, device="cuda")]
        for _ in range(n_calls):
            ops.lora_grad_fp8(dqkv, y8, t, M, H, lb, dt, *acc)
        return [dt] + acc

    dt, dA, dBq, dBv = run()
    dq, dv = dqkv[:M, :H].double(), dqkv[:M, 2 * H:].double()
    y = fp8_oracle.e4m3_values(u8(y8)[:M, :H])
    tq, tv = t[:M, :4].double(), t[:M, 4:8].double()
    ref_dt = torch.cat([dq @ lb[0].double(), dv @ lb[1].double()], 1)
    ref = dict(dt=ref_dt, dA=ref_dt.t() @ y, dBq=dq.t() @ tq, dBv=dv.t() @ tv)
    err = {k: rel_err(v, ref[k]) for k, v in zip(("dt", "dA", "dBq", "dBv"), (dt[:M], dA, dBq, dBv))}
    # two calls from equal initial buffers give equal bits (fixed summation order); dt is overwritten, dA / dB accumulate
    again = run()
    twice = run(2)
    err2 = {k: rel_err(v, 2 * ref[k]) for k, v in zip(("dA", "dBq", "dBv"), twice[1:])}
    # the bf16 kernel on the same numbers: every e4m3 value is exact in bf16
    h = torch.zeros(M, H + 64, dtype=torch.bfloat16, device="cuda")
    h[:, :H] = y8[:M, :H].to(torch.bfloat16)
    h[:, H:H + 8] = t[:M, :8]
    dt16 = torch.full((M, 8), float("nan"), device="cuda")
    acc16 = [torch.zeros(8, H, device="cuda"), torch.zeros(H, 4, device="cuda"), torch.zeros(H, 4, device="cuda")]
    ops.lora_grad(dqkv, h, M, H, lb, dt16, *acc16)
    cross = {k: rel_err(a, b) for k, a, b in zip(("dt", "dA", "dBq", "dBv"), (dt[:M], dA, dBq, dBv), [dt16] + acc16)}
    _log(f"lora_grad_fp8 H={H} M={M} ld_t={ld_t}", **err, twice=err2, vs_bf16_kernel=cross,
         bars=dict(dt=TOL_DT, dA=TOL_DAB, dB=TOL_DAB, vs_bf16_kernel=1e-6))
    assert err["dt"] < TOL_DT and err["dA"] < TOL_DAB and err["dBq"] < TOL_DAB and err["dBv"] < TOL_DAB, err
    assert torch.equal(again[0][:M], dt[:M]) and all(torch.equal(a, b) for a, b in zip(again[1:], (dA, dBq, dBv))), \
        "two calls from equal buffers differ"
    assert all(v < TOL_DAB for v in err2.values()), err2
    assert torch.equal(twice[0][:M], dt[:M]), "dt must be overwritten, not accumulated"
    assert torch.isnan(dt[M:]).all(), "dt row M written"
    assert all(v < 1e-6 for v in cross.values()), cross


# ------------------------------------------------------------------------------------------------------- 3. the LoRA-B tile
def _beff(H, bq, bv, alpha):
    """What lora_baug_set must write, by torch: bf16 of one f32 division.  [3H, 8], zero outside the two blocks."""
    want = torch.zeros(3 * H, 8, dtype=torch.bfloat16, device="cuda")
    want[:H, :4] = (bq / alpha[:H, None]).bfloat16()
    want[2 * H:, 4:] = (bv / alpha[2 * H:, None]).bfloat16()
    return want


@pytest.mark.parametrize("ld", [64, 128])
@pytest.mark.parametrize("H", [768, 512])
def test_lora_baug_set(ops, H, ld):
    bq, bv = rnd(H, 4, seed=1, scale=0.05), rnd(H, 4, seed=2, scale=0.05)
    alpha = torch.exp(rnd(3 * H, seed=3, scale=2.0))      # a factor e^2 from row to row: a wrong row index shows
    b_aug = torch.full((3 * H + 1, ld), 7.0, dtype=torch.bfloat16, device="cuda")
    ops.lora_baug_set(b_aug, H, bq, bv, alpha)
    torch.cuda.synchronize()
    want = torch.full_like(b_aug, 7.0)
    blocks = _beff(H, bq, bv, alpha)
    want[:H, :4] = blocks[:H, :4]
    want[2 * H:3 * H, 4:8] = blocks[2 * H:, 4:]
    assert torch.equal(b_aug.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("M", [8, 394])
def test_fp8_qkv_projection_composed(ops, M, form):
    """The QKV projection as the fp8 engines run it: LayerNorm -> e4m3 + t, row-quantised W_qkv, LoRA-B tile, GEMM with the
    K-augmentation block -- against f64 arithmetic on the dequantised operands."""
    from bioscanclip.hip.lib import EPI_BF16, EPI_F32
    H = 768
    r = _ln_case(ops, H, 1e-6, M, False, 64, seed=31)
    y8, t = r["y8"].view(ops.FP8), r["t"]
    w8, ws = ops.quantize_rows_fp8(rnd(3 * H, H, seed=32, scale=0.05))
    bq, bv = rnd(H, 4, seed=33, scale=0.05), rnd(H, 4, seed=34, scale=0.05)
    bias = rnd(3 * H, seed=35)
    b_aug = torch.zeros(3 * H, 64, dtype=torch.bfloat16, device="cuda")
    ops.lora_baug_set(b_aug, H, bq, bv, ws)
    out16 = torch.empty(M, 3 * H, dtype=torch.bfloat16, device="cuda")
    ops.gemm_fp8(y8, w8, out16, ws, bias, EPI_BF16, a_aug=t, b_aug=b_aug, M=M, K=H, form=form)
    yd, wd = fp8_oracle.e4m3_values(u8(y8)[:M, :H]), fp8_oracle.e4m3_values(u8(w8))
    td, al = t[:M, :8].double(), ws.double()
    b_eff = al[:, None] * _beff(H, bq, bv, ws).double()           # alpha * bf16(B / alpha), from torch, not from the kernel
    ref = al * (yd @ wd.t()) + td @ b_eff.t() + bias.double()
    e16 = rel_err(out16.float(), ref)
    # the LoRA share alone
    o_with, o_without = torch.empty(M, 3 * H, device="cuda"), torch.empty(M, 3 * H, device="cuda")
    ops.gemm_fp8(y8, w8, o_with, ws, bias, EPI_F32, a_aug=t, b_aug=b_aug, M=M, K=H, form=form)
    ops.gemm_fp8(y8, w8, o_without, ws, bias, EPI_F32, M=M, K=H, form=form)
    share = o_with.double() - o_without.double()
    q, k, v = slice(0, H), slice(H, 2 * H), slice(2 * H, 3 * H)
    true_q, true_v = td[:, :4] @ bq.double().t(), td[:, 4:] @ bv.double().t()
    sq, sv = rel_err(share[:, q], true_q), rel_err(share[:, v], true_v)
    sq_eff, sv_eff = rel_err(share[:, q], td @ b_eff[q].t()), rel_err(share[:, v], td @ b_eff[v].t())
    bar = TOL_F32 + 2.0 ** -9         # B_eff is one bf16 rounding (relative 2^-9 at most) of B
    _log(f"fp8 qkv composed M={M} form={form}", out_bf16=e16, e32=rel_err(o_with, ref), lora_q=sq, lora_v=sv,
         lora_q_vs_rounded_B=sq_eff, lora_v_vs_rounded_B=sv_eff, bars=dict(out_bf16=TOL_BF16, lora=bar))
    assert e16 < TOL_BF16
    assert rel_err(o_with, ref) < TOL_F32
    assert sq < bar and sv < bar
    assert (share[:, k] == 0).all(), "the k columns have no LoRA branch"


# ------------------------------------------------------------------------------------------------------- 4. GEMM edges
def gelu(x):
    return torch.nn.functional.gelu(x)


def _dgelu(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def _gemm_operands(ops, M, N, K, aug, seed=0):
    """Strided e4m3 operands (lda, ldb > K) with two spare rows of A, plus the dequantised f64 reference alpha * A B^T + bias."""
    abuf = fp8_buf(ops, M + 2, K + 16)
    u8(abuf)[:, :K] = u8(grnd(M + 2, K, seed=seed + 1).to(ops.FP8))
    a8 = abuf[:, :K]
    w = rnd(N, K, seed=seed + 2, scale=0.05)
    wq, ws = ops.quantize_rows_fp8(w)
    bbuf = fp8_buf(ops, N, K + 32)
    u8(bbuf)[:, :K] = u8(wq)
    b8 = bbuf[:, :K]
    bias = rnd(N, seed=seed + 3)
    ref = (fp8_oracle.e4m3_values(u8(a8)[:M]) @ fp8_oracle.e4m3_values(u8(wq)).t()) * ws.double() + bias.double()
    kw = {}
    if aug:     # the whole 64-column tile carries values here (the engines fill 8)
        t = rnd(M + 2, 128, seed=seed + 4, scale=0.3).bfloat16()[:, :64]
        b = (rnd(N, 64, seed=seed + 5, scale=0.05) / ws[:, None]).bfloat16()
        ref = ref + (t[:M].double() @ b.double().t()) * ws.double()
        kw = dict(a_aug=t, b_aug=b)
    return a8, b8, ws, bias, ref, kw


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("K,aug", [(128, False), (128, True), (768, False)])
@pytest.mark.parametrize("M", [1, 8, 255, 257])
def test_gemm_fp8_few_rows_and_strides(ops, form, M, K, aug):
    """The ViT's last block runs its MLP on the token-0 rows only: M = B, far below the 256-row tile.  Strided A, B, C, residual and
    aux; rows >= M and columns >= N of every output keep what they held."""
    from bioscanclip.hip.lib import EPI_BF16, EPI_F32, EPI_GELU_FP8, EPI_RESID_F32
    N, ldc = 256, 256 + 16
    a8, b8, alpha, bias, ref, kw = _gemm_operands(ops, M, N, K, aug, seed=10 * M)
    nan = float("nan")
    out32 = torch.full((M + 3, ldc), nan, device="cuda")
    ops.gemm_fp8(a8, b8, out32[:, :N], alpha, bias, EPI_F32, M=M, K=K, form=form, **kw)
    e32 = rel_err(out32[:M, :N], ref)
    assert torch.isnan(out32[M:]).all() and torch.isnan(out32[:, N:]).all()
    out16 = torch.full((M + 3, ldc), nan, dtype=torch.bfloat16, device="cuda")
    ops.gemm_fp8(a8, b8, out16[:, :N], alpha, bias, EPI_BF16, M=M, K=K, form=form, **kw)
    e16 = rel_err(out16[:M, :N].float(), ref)
    assert torch.isnan(out16[M:]).all() and torch.isnan(out16[:, N:]).all()
    resid = rnd(M, N + 8, seed=6)[:, :N]
    out32.fill_(nan)
    ops.gemm_fp8(a8, b8, out32[:, :N], alpha, bias, EPI_RESID_F32, resid=resid, M=M, K=K, form=form, **kw)
    er = rel_err(out32[:M, :N], ref + resid.double())
    assert torch.isnan(out32[M:]).all() and torch.isnan(out32[:, N:]).all()
    out8, z = fp8_buf(ops, M + 3, ldc), torch.full((M + 3, ldc), SENT8, dtype=torch.uint8, device="cuda")
    ops.gemm_fp8(a8, b8, out8[:, :N], alpha, bias, EPI_GELU_FP8, aux=z[:, :N], M=M, K=K, form=form, **kw)
    assert (u8(out8)[M:] == SENT8).all() and (u8(out8)[:, N:] == SENT8).all() and (z[M:] == SENT8).all() and (z[:, N:] == SENT8).all()
    _log(f"gemm_fp8 M={M} K={K} aug={aug} form={form}", f32=e32, bf16=e16, resid_f32=er, bars=dict(f32=TOL_F32, bf16=TOL_BF16))
    assert e32 < TOL_F32 and e16 < TOL_BF16 and er < TOL_F32
    # GELU output and gelu' side band: the comparison of tests/test_45_fp8_gpu.py
    reff = ref.float()
    got, exp = out8[:M, :N].float(), gelu(reff).to(ops.FP8).float()
    assert ((got - exp).abs() <= 0.126 * exp.abs() + 2e-3).all()
    assert (got != exp).sum().item() <= max(1, int(2e-3 * M * N))       # test_45's 2e-3 of the elements; at M = 1 that is one element
    assert ((z[:M, :N].float() * (1.26 / 255) - 0.13) - _dgelu(reff).float()).abs().max().item() < 0.5 * 1.26 / 255 + 6e-4


def test_gemm_fp8_resid_dropout(ops):
    """The BERT towers' out-projection / fc2 epilogue: C = dropout(alpha acc + bias) + resid.  The mask is a function of (seed, element)
    alone: both MFMA forms and the bf16 GEMM draw the same one.  With a zero residual a zero is a dropped element and nothing else."""
    from bioscanclip.hip.lib import EPI_RESID_F32
    M, N, K, seed = 600, 256, 256, 1234
    a8, b8, alpha, bias, ref, _ = _gemm_operands(ops, M, N, K, False, seed=50)
    assert (ref != 0).all()
    zero = torch.zeros(M, N, device="cuda")
    # the bf16 kernel's mask for [M, N]: acc = 0, bias = 1
    ob = torch.empty(M, N, device="cuda")
    ops.gemm(torch.zeros(M, 64, dtype=torch.bfloat16, device="cuda"), torch.zeros(N, 64, dtype=torch.bfloat16, device="cuda"), ob,
             EPI_RESID_F32, bias=torch.ones(N, device="cuda"), resid=zero, dropout=(P, seed))
    kept = ob != 0
    resid = rnd(M, N, seed=7)
    for form in (1, 2):
        d = torch.empty(M, N, device="cuda")
        ops.gemm_fp8(a8, b8, d, alpha, bias, EPI_RESID_F32, resid=zero, M=M, K=K, dropout=(P, seed), form=form)
        assert torch.equal(d != 0, kept), f"form {form}: mask differs from the bf16 GEMM's"
        rate, surv = kept.float().mean().item(), rel_err(d[kept], (ref / (1 - P))[kept])
        d2, d3, d4 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
        ops.gemm_fp8(a8, b8, d2, alpha, bias, EPI_RESID_F32, resid=zero, M=M, K=K, dropout=(P, seed), form=form)
        ops.gemm_fp8(a8, b8, d3, alpha, bias, EPI_RESID_F32, resid=zero, M=M, K=K, dropout=(P, seed + 1), form=form)
        ops.gemm_fp8(a8, b8, d4, alpha, bias, EPI_RESID_F32, resid=resid, M=M, K=K, dropout=(P, seed), form=form)
        with_resid = rel_err(d4, d.double() + resid.double())
        _log(f"gemm_fp8 resid dropout form={form}", keep_rate=rate, survivors=surv, with_resid=with_resid,
             bars=dict(keep_rate=TOL_KEEP, survivors=TOL_F32, with_resid=TOL_F32))
        assert abs(rate - (1 - P)) < TOL_KEEP and surv < TOL_F32 and with_resid < TOL_F32
        assert torch.equal(d2, d), "same seed -> same bits"
        assert ((d3 != 0) != kept).float().mean().item() > 0.1, "another seed -> another mask"


@pytest.mark.parametrize("form", [1, 2])
def test_gemm_fp8_gelu_at_the_ends_of_the_range(ops, form):
    """Pre-activations above +448 (gelu(x) = x there: the largest finite code, gelu' = 1) and below -10 (gelu and gelu' vanish)."""
    from bioscanclip.hip.lib import EPI_GELU_FP8
    M, N, K = 70, 256, 128
    a8, b8, alpha, bias, ref, _ = _gemm_operands(ops, M, N, K, False, seed=70)
    acc = ref - bias.double()
    bias = bias.clone()
    bias[:64], bias[64:128] = 600.0, -20.0
    pre = acc + bias.double()
    hi, lo = slice(0, 64), slice(64, 128)
    assert (pre[:, hi] > 448).all() and (pre[:, lo] < -10).all()
    out8, z = fp8_buf(ops, M, N), torch.full((M, N), SENT8, dtype=torch.uint8, device="cuda")
    ops.gemm_fp8(a8, b8, out8, alpha, bias, EPI_GELU_FP8, aux=z, M=M, K=K, form=form)
    c = u8(out8)
    code = lambda v: round((v + 0.13) * 255 / 1.26)   # noqa: E731  the 8-bit gelu' code (csrc/common.h)
    assert (c[:, hi] == 0x7E).all() and (z[:, hi] == code(1.0)).all()
    assert ((c[:, lo] == 0x00) | (c[:, lo] == 0x80)).all() and (z[:, lo] == code(0.0)).all()
    assert not is_nan_code(c).any()
    mid = pre[:, 128:].float()
    got, exp = out8[:, 128:].float(), gelu(mid).to(ops.FP8).float()
    assert ((got - exp).abs() <= 0.126 * exp.abs() + 2e-3).all()
    assert (got != exp).float().mean().item() < 2e-3
    assert ((z[:, 128:].float() * (1.26 / 255) - 0.13) - _dgelu(mid).float()).abs().max().item() < 0.5 * 1.26 / 255 + 6e-4


@pytest.mark.parametrize("form", [1, 2])
def test_gemm_fp8_gelu_nan_and_inf(ops, form):
    """A NaN pre-activation must leave the NaN code in the next GEMM's operand; +inf saturates to 448; no other column changes."""
    from bioscanclip.hip.lib import EPI_GELU_FP8
    M, N, K = 40, 256, 128
    a8, b8, alpha, bias, _, _ = _gemm_operands(ops, M, N, K, False, seed=80)
    bad = bias.clone()
    bad[17], bad[200] = float("nan"), float("inf")

    def run(b):
        out8, z = fp8_buf(ops, M, N), torch.full((M, N), SENT8, dtype=torch.uint8, device="cuda")
        ops.gemm_fp8(a8, b8, out8, alpha, b, EPI_GELU_FP8, aux=z, M=M, K=K, form=form)
        return u8(out8), z
    c0, z0 = run(bias)
    c1, z1 = run(bad)
    cols = torch.ones(N, dtype=torch.bool, device="cuda")
    cols[17] = cols[200] = False
    assert torch.equal(c1[:, cols], c0[:, cols]) and torch.equal(z1[:, cols], z0[:, cols]), "a NaN / inf leaked into another column"
    assert not is_nan_code(c0).any()
    assert (c1[:, 200] == 0x7E).all(), ("+inf must saturate to 448", c1[:4, 200])
    assert is_nan_code(c1[:, 17]).all(), ("a NaN pre-activation must give the NaN code", c1[:4, 17])


@pytest.mark.parametrize("C", [4, 132, 768])
def test_quantize_rows_fp8_edge_rows(ops, C):
    """R = 5 is no multiple of the 4 rows per workgroup.  Row 0 is zero, row 1's largest magnitude is negative, row 2 has one non-zero
    element.  Codes against the table rounding of exactly what the kernel rounds: the f32 product w * (1 / scale)."""
    R = 5
    w = rnd(R, C, seed=C)
    w[0] = 0
    w[1, C // 2] = -3.0 * w[1].abs().max()
    w[2] = 0
    w[2, C - 1] = 0.37
    q, sc = ops.quantize_rows_fp8(w)
    c = u8(q)
    amax = w.abs().amax(dim=1)
    assert sc[0].item() == 1.0 and (c[0] == 0).all()
    assert torch.allclose(sc[1:], amax[1:] / 448, rtol=1e-6, atol=0)
    assert c[1, C // 2].item() == 0xFE
    assert c[2, C - 1].item() == 0x7E and (c[2, :C - 1] == 0).all()
    assert torch.equal(c, fp8_oracle.e4m3_codes(w * (1.0 / sc)[:, None]))
    # against the f64 quotient the two may differ where w / scale sits within an f32 ulp of a rounding boundary: nowhere here
    differ = (c != fp8_oracle.e4m3_codes(w.double() / sc.double()[:, None])).sum().item()
    _log(f"quantize_rows_fp8 C={C}", codes_differing_from_f64_quotient=differ)
    assert differ == 0
