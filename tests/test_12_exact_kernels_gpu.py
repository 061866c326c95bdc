"""Kernel-level parity of the exact mode's (BSCLIP_PARITY=2) split-operand producers and f32 heads, each against f64 torch on the
same f32 inputs.

The exact mode forms every product on split-bf16 operands: x = hi + lo with hi = bf16(x), lo = bf16(x - hi), exact to about 2^-16.  A
kernel that loses or garbles the lo term leaves a plain bf16 product behind (2^-9), which the encoder tests only see through a whole
network.  Every test here therefore also checks that a bf16-only result would miss its tolerance by at least 10x, and puts NaN
sentinels (or a fill byte) beyond the logical extent of every output: nothing may be written there.

Entry points covered: bsclip_split3_weight (QKV with the LoRA update folded, plain weights, the head), the y_split3 output of
bsclip_layernorm_fwd, bsclip_gelu_split3 (dst / g32 / codes, the M < rows CLS call, the g32-only DNA transform call),
bsclip_meanpool_tokens_f32, bsclip_softmax_meanpool_bwd_f32 and the default path's bsclip_dgelu_mul.

bsclip_dgelu_mul issues 8-byte loads and stores on g and out and 4-byte loads on the codes, but its host code checks only that the
row strides are multiples of 4 elements, not that the base pointers are aligned: a view that starts at an odd element would fault
instead of returning an error code.  The views below are all 8-byte aligned; the missing check is a separate issue."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_err  # noqa: E402

NAN = float("nan")
DG8_STEP = 1.26 / 255          # include/bsclip.h / csrc/common.h: gelu' codes, decode = code * step - 0.13 (test_10's rule)
DG8_OFF = 0.13


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to("cuda")


def split(x):
    """The split the kernels are specified to produce, restated in torch: hi = bf16(x) (round to nearest even), lo = bf16(x - hi).
    x - hi is exact in f32, so lo is a single rounding."""
    hi = x.float().bfloat16()
    return hi, (x.float() - hi.float()).bfloat16()


def nan_full(rows, cols, dtype=torch.float32):
    return torch.full((rows, cols), NAN, device="cuda", dtype=dtype)


def gelu64(z):
    z = z.double()
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))


def dgelu64(z):
    z = z.double()
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def half_ulp_bf16(hi):
    """Half a unit in the last place of each bf16 value, read off its exponent field E: 1.m x 2^(E - 127) with 7 stored fraction bits
    -> 2^(E - 135) (E = 0, subnormals: 2^-134); 0 for zeros."""
    E = (hi.bfloat16().view(torch.int16).to(torch.int32) >> 7) & 0xFF
    return torch.where(hi == 0, 0.0, torch.exp2((torch.clamp(E, min=1) - 135).double()))


# ------------------------------------------------------------------------------------------------------ split3_weight
@pytest.mark.parametrize("N,K,lora", [(2304, 768, True), (2304, 768, False), (3072, 768, False), (768, 3072, False), (768, 768, False)])
def test_split3_weight(ops, N, K, lora):
    """bsclip_split3_weight: rows [hi | hi | lo] of a frozen f32 weight, the QKV weight with W + B A folded in f32 on the q and v
    rows.  Without LoRA the layout is checked bit for bit; with LoRA the k rows must be the plain split and the q / v rows must
    represent W_eff to 2^-16.  One split-operand GEMM against the f64 product closes the loop (3e-5; hi alone sits near 3e-3)."""
    from bioscanclip.hip.ops import EPI_F32
    w = rnd(N, K, seed=1, scale=K ** -0.5)
    w[0, :8] = 0.0                                   # exact zeros: hi = lo = 0
    w[1, :4] = torch.tensor([3.0, -1e-20, 1.0 + 2 ** -8, -(1.0 + 3 * 2 ** -9)], device="cuda")   # wide range, bf16 ties
    n = N * 3 * K
    buf = torch.full((n + 64,), NAN, device="cuda", dtype=torch.bfloat16)
    dst = buf[:n].view(N, 3 * K)
    A = Bm = None
    if lora:
        H = K
        A, Bm = rnd(8, H, seed=2, scale=0.05), rnd(2, H, 4, seed=3, scale=0.05)
    ops.split3_weight(w, dst, lora_a=A, lora_b=Bm)
    torch.cuda.synchronize()
    assert torch.isnan(buf[n:].float()).all(), "split3_weight wrote past [N, 3K]"
    assert torch.equal(dst[:, :K], dst[:, K:2 * K]), "the first two thirds must both be hi"
    hi, lo = dst[:, :K], dst[:, 2 * K:]
    weff = w.double().clone()
    fold_mag = torch.zeros_like(weff)               # sum_j |b_j a_j|: the size of the f32 fold's intermediates beyond |W|
    if lora:
        weff[:H] += Bm[0].double() @ A[:4].double()
        weff[2 * H:] += Bm[1].double() @ A[4:].double()
        fold_mag[:H] = Bm[0].double().abs() @ A[:4].double().abs()
        fold_mag[2 * H:] = Bm[1].double().abs() @ A[4:].double().abs()
        plain = torch.empty(N, 3 * K, device="cuda", dtype=torch.bfloat16)
        ops.split3_weight(w, plain)
        assert torch.equal(dst[H:2 * H], plain[H:2 * H]), "the k rows [H, 2H) carry no LoRA update"
        qv = torch.cat([torch.arange(0, H), torch.arange(2 * H, 3 * H)]).cuda()
        hq, lq, we = hi[qv].double(), lo[qv].double(), weff[qv]
        # the split represents x to 2^-18 |x|; x = the f32 fold, four fmas each rounded to 2^-24 of an intermediate <= |W| + sum |b a|
        bound = 2 ** -16 * we.abs() + 2 ** -21 * (w.double()[qv].abs() + fold_mag[qv]) + 1e-12
        err = (hq + lq - we).abs()
        assert (err <= bound).all(), (err / bound).max().item()
        assert ((hq - we).abs() / bound).max().item() > 10, "a bf16-only weight must fail the bound by 10x"
        assert rel_err(hq + lq, we) < 2 ** -16 < rel_err(hq, we) / 10
    else:
        rh, rl = split(w)
        assert torch.equal(hi, rh) and torch.equal(lo, rl)
    assert (lo.double().abs() <= half_ulp_bf16(hi)).all(), "|lo| <= 1/2 ulp(hi)"
    # the B operand of a split-bf16 GEMM: [hi | lo | hi] rows of x against [hi | hi | lo] rows of W = hi.hi + lo.hi + hi.lo
    M = 333
    x = rnd(M, K, seed=4)
    a3 = ops.split3_rows(x, torch.empty(M, 3 * K, device="cuda", dtype=torch.bfloat16))
    out = nan_full(M + 2, N)
    ops.gemm(a3, dst, out, EPI_F32, M=M)
    ref = x.double() @ weff.t()
    e3 = rel_err(out[:M], ref)
    out_hi = torch.empty(M, N, device="cuda")
    ops.gemm(a3[:, :K], dst[:, :K], out_hi, EPI_F32, M=M, K=K)     # the same product on hi only: plain bf16 operands
    e1 = rel_err(out_hi, ref)
    assert torch.isnan(out[M:]).all()
    assert e3 < 3e-5 and 10 * 3e-5 < e1 < 1e-2, (e3, e1)


# ------------------------------------------------------------------------------------------------------ layernorm_fwd y_split3
@pytest.mark.parametrize("variant", ["f32", "offset", "cls"])
@pytest.mark.parametrize("M", [1, 7, 300])
@pytest.mark.parametrize("H", [768, 512])
def test_layernorm_fwd_split3(ops, H, M, variant):
    """bsclip_layernorm_fwd with y_f32, stats and the split operand y_split3 [hi | lo | hi] (bf16, row stride > 3H): y_f32 against
    f64 LayerNorm, y_split3 bit for bit the split of y_f32.  Variants: plain f32 rows; rows whose mean is 32-64x their standard
    deviation (a one-pass variance would cancel); the strided CLS-rows view the ViT's last layer passes (t.view(B, S H)[:, :H])."""
    S = 3
    if variant == "cls":
        t = rnd(M * S, H, seed=1)
        t0 = t.clone()
        x = t.view(M, S * H)[:, :H]
    else:
        x = rnd(M, H, seed=1)
        if variant == "offset":
            g = torch.Generator().manual_seed(5)
            x = x + 32.0 * (1 + torch.rand(M, 1, generator=g)).to("cuda")
    gamma, beta = 1 + rnd(H, seed=2, scale=0.2), rnd(H, seed=3, scale=0.1)
    y32 = nan_full(M + 2, H)
    y3buf = nan_full(M + 2, 3 * H + 8, torch.bfloat16)
    y3 = y3buf[:, :3 * H]
    stats = torch.full((2 * M + 4,), NAN, device="cuda")
    ops.layernorm_fwd(x, gamma, beta, 1e-6, y_f32=y32, y_split3=y3, stats=stats, M=M)
    torch.cuda.synchronize()
    xd = x.double()
    ref = torch.nn.functional.layer_norm(xd, (H,), gamma.double(), beta.double(), 1e-6)
    # the f32 mean carries a few ulps of the row's offset into every output: 1e-6 plus 8 ulps of |mean| / std (an f32 emulation of
    # the kernel's summation order reaches a third of that on single rows; a one-pass variance would be ~|mean| / std times worse)
    ratio = (xd.mean(1).abs() / xd.std(1, unbiased=False)).max().item()
    tol = 1e-6 + 2 ** -21 * ratio
    e = rel_err(y32[:M], ref)
    assert e < tol, (e, tol)
    st = stats[:2 * M].view(M, 2).double()
    assert ((st[:, 0] - xd.mean(1)).abs() <= 2 ** -20 * xd.abs().amax(1)).all()
    assert rel_err(st[:, 1], (xd.var(1, unbiased=False) + 1e-6).rsqrt()) < 1e-6
    hi, lo = split(y32[:M])
    assert torch.equal(y3[:M, :H], hi) and torch.equal(y3[:M, H:2 * H], lo) and torch.equal(y3[:M, 2 * H:], hi)
    assert rel_err(hi.double() + lo.double(), ref) < tol + 2 ** -17 and rel_err(hi.double(), ref) > 10 * tol
    # nothing beyond the M rows, the 3H columns, the 2M statistics
    assert torch.isnan(y32[M:]).all() and torch.isnan(y3buf[M:].float()).all() and torch.isnan(y3buf[:, 3 * H:].float()).all()
    assert torch.isnan(stats[2 * M:]).all()
    if variant == "cls":
        assert torch.equal(t, t0), "the input's non-CLS rows were written"


# ------------------------------------------------------------------------------------------------------ gelu_split3
def _gelu_input(rows, N, ldz):
    z = rnd(rows, ldz, seed=1, scale=3.0)[:, :N]
    z[0] = torch.linspace(-10, 10, N, device="cuda")               # both tails
    z[1] = rnd(N, seed=2, scale=1e-3)                             # near 0
    z[2, ::3] = 0.0                                               # exact zeros
    z[3] = -rnd(N, seed=3, scale=2.0).abs()                       # negatives
    return z


@pytest.mark.parametrize("N,M,rows", [(3072, 300, 304), (3072, 2, 394), (768, 7, 9)])
def test_gelu_split3(ops, N, M, rows):
    """bsclip_gelu_split3: g32 = exact erf GELU in f32, dst = its split [hi | lo | hi], codes = gelu' on test_10's 8-bit grid; z with a
    row stride > N; M < rows is the ViT's CLS-rows call (rows >= M untouched)."""
    z = _gelu_input(rows, N, N + 4)
    dbuf = nan_full(rows, 3 * N + 8, torch.bfloat16)
    gbuf = nan_full(rows, N + 4)
    cbuf = torch.full((rows, N + 4), 0xAB, device="cuda", dtype=torch.uint8)
    ops.gelu_split3(z, dbuf[:, :3 * N], codes=cbuf[:, :N], g32=gbuf[:, :N], M=M)
    torch.cuda.synchronize()
    zm = z[:M].double()
    ref = gelu64(zm)
    g32 = gbuf[:M, :N]
    e = rel_err(g32, ref)
    assert e < 1e-6, e
    # elementwise: a few f32 ulps at the scale of |z| (for z << 0 the f32 formula's 1 + erf cancels: so does the reference module's)
    err = (g32.double() - ref).abs()
    assert (err <= 2 ** -22 * torch.maximum(ref.abs(), zm.abs()) + 1e-30).all(), (err / torch.maximum(ref.abs(), zm.abs())).max().item()
    assert (g32[0, :8] == 0).all() or (g32[0, :8].abs() < 1e-20).all()    # GELU(-10) ~ -7.6e-23
    hi, lo = split(g32)
    d3 = dbuf[:M, :3 * N]
    assert torch.equal(d3[:, :N], hi) and torch.equal(d3[:, N:2 * N], lo) and torch.equal(d3[:, 2 * N:], hi)
    assert rel_err(hi.double() + lo.double(), ref) < 1e-6 + 2 ** -17 < rel_err(hi.double(), ref) / 10
    dec = cbuf[:M, :N].double() * DG8_STEP - DG8_OFF
    assert ((dec - dgelu64(zm)).abs() <= DG8_STEP + 1e-6).all(), "gelu' codes more than one code away"
    assert torch.isnan(dbuf[M:].float()).all() and torch.isnan(dbuf[:, 3 * N:].float()).all()
    assert torch.isnan(gbuf[M:]).all() and torch.isnan(gbuf[:, N:]).all()
    assert (cbuf[M:] == 0xAB).all() and (cbuf[:, N:] == 0xAB).all()
    # the DNA head's transform: g32 only (no split, no codes)
    g2 = nan_full(rows, N)
    ops.gelu_split3(z, None, g32=g2, M=M)
    assert torch.equal(g2[:M], g32) and torch.isnan(g2[M:]).all()


# ------------------------------------------------------------------------------------------------------ meanpool_tokens_f32
@pytest.mark.parametrize("H", [512, 768])
@pytest.mark.parametrize("S", [1, 7, 133])
def test_meanpool_tokens_f32(ops, S, H):
    """bsclip_meanpool_tokens_f32 (the text tower's pooled output, padding included) against the f64 mean; NaN rows after B S must
    not be read, rows after B not written."""
    B = 3
    x = rnd(B * S + 2, H, seed=1) + 0.5
    x[B * S:] = NAN
    out = nan_full(B + 2, H)
    ops.meanpool_tokens_f32(x, B, S, out)
    torch.cuda.synchronize()
    ref = x[:B * S].double().view(B, S, H).mean(1)
    assert rel_err(out[:B], ref) < 1e-6 < rel_err(ref.bfloat16().double(), ref) / 10
    assert torch.isnan(out[B:]).all()


# ------------------------------------------------------------------------------------------------------ softmax_meanpool_bwd_f32
@pytest.mark.parametrize("B,S,scale,ld_pad", [(3, 7, 0.01, 0), (3, 7, 30.0, 4), (5, 133, 3.0, 8), (2, 1, 50.0, 4), (4, 5, 1.0, 0)])
def test_softmax_meanpool_bwd_f32(ops, B, S, scale, ld_pad):
    """bsclip_softmax_meanpool_bwd_f32 (the DNA MLM head's backward, f32 out) with the statistics of softmax_meanpool_fwd, against
    f64 autograd of softmax(logits).mean(tokens) . d_pooled.  M = B S not a multiple of 4 (four rows per workgroup), flat and peaked
    logits (scale 30 / 50 would overflow exp without the row maximum), dlogits with a row stride > C; rows >= M untouched."""
    C = 768
    M = B * S
    logits = rnd(M, C, seed=1, scale=scale)
    pooled, stats = torch.empty(B, C, device="cuda"), torch.empty(M, 2, device="cuda")
    ops.softmax_meanpool_fwd(logits, B, S, pooled, stats)
    dp = rnd(B, C, seed=2)
    lf = logits.double().requires_grad_(True)
    ref = torch.softmax(lf.view(B, S, C), -1).mean(1)
    (gl,) = torch.autograd.grad(ref, lf, dp.double())
    buf = nan_full(M + 3, C + ld_pad)
    ops.softmax_meanpool_bwd_f32(logits, stats, dp, B, S, buf[:, :C])
    torch.cuda.synchronize()
    # a peaked row's gradient p (g - p.g) cancels to far below its terms p g (f32 forms those terms to 2^-24 and cannot do better):
    # the error is measured against max(|gradient|, 0.1 |p g|), which is |gradient| itself on all but near one-hot rows
    pg = (torch.softmax(lf.detach(), -1) * dp.double().repeat_interleave(S, 0) / S).norm().item()
    denom = max(gl.norm().item(), 0.1 * pg)
    e = (buf[:M, :C].double() - gl).norm().item() / denom
    assert e < 1e-5, (e, gl.norm().item(), pg)
    if gl.norm().item() >= 0.1 * pg:
        assert rel_err(gl.bfloat16().double(), gl) > 10 * 1e-5
    assert torch.isnan(buf[M:]).all() and torch.isnan(buf[:, C:]).all()


# ------------------------------------------------------------------------------------------------------ dgelu_mul
@pytest.mark.parametrize("M,N", [(300, 768), (37, 3072)])
def test_dgelu_mul(ops, M, N):
    """bsclip_dgelu_mul (the default path's BERT MLM-head backward): out = bf16(g * decode(codes)), g and out bf16 with row strides
    > N, every code value, in place as the engine calls it (out = g); rows >= M untouched."""
    g_buf = rnd(M + 2, N + 4, seed=1).bfloat16()
    g = g_buf[:, :N]
    gen = torch.Generator().manual_seed(2)
    c_buf = torch.randint(0, 256, (M + 2, N + 8), generator=gen, dtype=torch.uint8).to("cuda")
    c_buf[0, :256] = torch.arange(256, dtype=torch.uint8, device="cuda")
    codes = c_buf[:, :N]
    o_buf = nan_full(M + 2, N + 12, torch.bfloat16)
    out = o_buf[:, :N]
    ops.dgelu_mul(g, codes, M, N, out)
    torch.cuda.synchronize()
    gm, cm = g[:M].float(), codes[:M]
    ref = (gm * (cm.float() * DG8_STEP - DG8_OFF)).bfloat16()
    exact = gm.double() * (cm.double() * DG8_STEP - DG8_OFF)
    o = out[:M].double()
    # one bf16 rounding of the product: within half an ulp (plus the f32 decode's rounding) of the exact value, one ulp of ref
    assert ((o - exact).abs() <= 2 ** -8 * exact.abs() + 1e-30).all()
    assert ((o - ref.double()).abs() <= 2 * half_ulp_bf16(ref) + 1e-30).all()
    # the kernel decodes with one fma in f32: restated exactly (code * step is exact in f64, the sum too), the result is bit-exact
    step32 = torch.tensor(1.26, dtype=torch.float32) / 255
    off32 = torch.tensor(0.13, dtype=torch.float32)
    d32 = (cm.double() * step32.double() - off32.double()).float()
    assert torch.equal(out[:M], (gm * d32).bfloat16())
    assert torch.isnan(o_buf[M:].float()).all() and torch.isnan(o_buf[:, N:].float()).all()
    # in place, as BertEngine.backward calls it
    g2 = g_buf.clone()
    ops.dgelu_mul(g2[:, :N], codes, M, N, g2[:, :N])
    assert torch.equal(g2[:M, :N], out[:M]) and torch.equal(g2[M:], g_buf[M:]) and torch.equal(g2[:, N:], g_buf[:, N:])
