"""fp16-operand GEMMs (bsclip_gemm_bf16 with BSCLIP_OPERANDS_FP16; ops.gemm on float16 tensors) against torch f32 arithmetic on the
fp16-decoded inputs, on every kernel the tile selection can pick (generic 128x128 / 256x128 / 256x256, ping-pong, persistent) and
every epilogue the engines use.  The duo kernel has no fp16 form: tile 5 checks that a forced duo tile takes the fallback route
(ping-pong for N % 256 == 0, the 256x128 generic tile otherwise) and still computes the right product.  f32 outputs: accumulation
order only (1e-5 normwise).  fp16 outputs: one fp16 rounding (2^-11 relative per element), gated at 5e-4 normwise -- a bf16
rounding anywhere (2^-8 .. 2^-9) lands near 2e-3 and fails."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_err  # noqa: E402

TOL_F32 = 1e-5
TOL_F16 = 5e-4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def dgelu(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("M,N,K", [(300, 256, 64), (1000, 768, 832), (197 * 8, 2304, 832), (5120, 768, 3072), (700, 384, 128)])
def test_gemm_fp16_epilogues(ops, tile, M, N, K):
    from bioscanclip.hip.lib import (EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_BF16, EPI_RESID_F32)
    h = torch.float16
    ops.set_gemm_tile(tile)
    try:
        a = rnd(M, K + 16, seed=1).to(h).cuda()[:, :K]      # row stride > K on purpose
        b = rnd(N, K, seed=2, scale=0.1).to(h).cuda()
        bias = rnd(N, seed=3).cuda()
        ref = a.float() @ b.float().t() + bias
        out32 = torch.full((M + 3, N), float("nan"), device="cuda")
        ops.gemm(a, b, out32, EPI_F32, bias=bias, M=M)
        assert rel_err(out32[:M], ref) < TOL_F32
        assert torch.isnan(out32[M:]).all(), "rows beyond M were written"
        out16 = torch.empty(M, N, device="cuda", dtype=h)
        ops.gemm(a, b, out16, EPI_BF16, bias=bias)
        assert rel_err(out16.float(), ref) < TOL_F16
        ops.gemm(a, b, out16, EPI_BF16)
        assert rel_err(out16.float(), ref - bias) < TOL_F16
        # GELU (table-driven, as in the bf16 form) with the 8-bit gelu' side band
        z = torch.empty(M, N, device="cuda", dtype=torch.uint8)
        ops.gemm(a, b, out16, EPI_GELU_BF16, bias=bias, aux=z)
        dg = z.float() * (1.26 / 255) - 0.13
        assert (dg - dgelu(ref)).abs().max().item() < 0.5 * 1.26 / 255 + 6e-4
        assert rel_err(out16.float(), gelu(ref)) < 1e-3     # the table's own error (~2e-4 |x|) plus one fp16 rounding
        r = rnd(M, N, seed=4).cuda()
        ops.gemm(a, b, out32, EPI_RESID_F32, bias=bias, resid=r, M=M)
        assert rel_err(out32[:M], ref + r) < TOL_F32
        # the 16-bit residual stream in fp16: sum formed in f32, rounded once
        rh = torch.zeros(M, N + 64, device="cuda", dtype=h)
        rh[:, :N] = r.to(h)
        out16r = torch.full((M + 3, N), float("nan"), device="cuda", dtype=h)
        ops.gemm(a, b, out16r, EPI_RESID_BF16, bias=bias, resid=rh, M=M)
        assert rel_err(out16r[:M].float(), ref + rh[:, :N].float()) < TOL_F16
        assert torch.isnan(out16r[M:]).all(), "rows beyond M were written"
        zz = torch.randint(0, 256, (M, N), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
        ops.gemm(a, b, out16, EPI_DGELU_BF16, aux=zz)
        assert rel_err(out16.float(), (ref - bias) * (zz.float() * (1.26 / 255) - 0.13)) < TOL_F16
    finally:
        ops.set_gemm_tile(0)


@pytest.mark.parametrize("tile", [1, 4, 8])
def test_gemm_fp16_patch_epilogues(ops, tile):
    from bioscanclip.hip.lib import EPI_PATCH_BF16, EPI_PATCH_F32
    B, N, K = 4, 768, 768
    M = 196 * B
    a = rnd(M, K, seed=6).half().cuda()
    b = rnd(N, K, seed=7, scale=0.05).half().cuda()
    bias = rnd(N, seed=8).cuda()
    pos = rnd(197, N, seed=9).cuda()
    ref = (a.float() @ b.float().t() + bias).view(B, 196, N) + pos[1:]
    ops.set_gemm_tile(tile)
    try:
        o32 = torch.full((B * 197, N), float("nan"), device="cuda")
        ops.gemm(a, b, o32, EPI_PATCH_F32, bias=bias, resid=pos)
        assert rel_err(o32.view(B, 197, N)[:, 1:], ref) < TOL_F32
        assert torch.isnan(o32.view(B, 197, N)[:, 0]).all(), "class-token rows were written"
        o16 = torch.zeros(B * 197, N, device="cuda", dtype=torch.float16)
        ops.gemm(a, b, o16, EPI_PATCH_BF16, bias=bias, resid=pos)
        assert rel_err(o16.view(B, 197, N)[:, 1:].float(), ref) < TOL_F16
    finally:
        ops.set_gemm_tile(0)


@pytest.mark.parametrize("tile", [1, 4, 8])
def test_gemm_fp16_keeps_subnormals_and_overflows_to_inf(ops, tile):
    """Operands below fp16's smallest normal (2^-14) enter the matrix cores unflushed, subnormal results are stored as such, and a
    result beyond 65504 is stored as inf (never clamped, never wrapped)."""
    from bioscanclip.hip.lib import EPI_BF16, EPI_F32
    M, N, K = 2048, 1024, 256
    a = (rnd(M, K, seed=10) * 2.0 ** -18).half()          # |a| ~ 2^-18: subnormal in fp16
    assert (a.abs() < 2.0 ** -14).float().mean() > 0.99 and (a != 0).float().mean() > 0.9
    b = rnd(N, K, seed=11).half()
    a, b = a.cuda(), b.cuda()
    ref = a.float() @ b.float().t()
    ops.set_gemm_tile(tile)
    try:
        o32 = torch.empty(M, N, device="cuda")
        ops.gemm(a, b, o32, EPI_F32)
        assert rel_err(o32, ref) < TOL_F32                 # flushed inputs would give 0
        tiny = torch.empty(M, N, device="cuda", dtype=torch.float16)
        b_small = (b.float() * 2.0 ** -6).half()           # results ~ 2^-20: subnormal outputs
        ops.gemm(a, b_small, tiny, EPI_BF16)
        ref_small = a.float() @ b_small.float().t()
        assert (tiny != 0).float().mean() > 0.9
        assert (tiny.float() - ref_small).abs().max().item() <= 2.0 ** -24 * 0.5 + 1e-3 * ref_small.abs().max().item()
        big = torch.full((M, N), 200.0, device="cuda", dtype=torch.float16)
        ops.gemm(big[:, :K], torch.full((N, K), 200.0, device="cuda", dtype=torch.float16), tiny, EPI_BF16)
        assert torch.isinf(tiny).all() and (tiny > 0).all()   # 256 * 40 000 = 1.0e7 > 65504
    finally:
        ops.set_gemm_tile(0)


@pytest.mark.parametrize("M,N,K", [(2500, 512, 576), (197 * 8, 2304, 768)])
def test_gemm_fp16_persistent_equals_ping_pong(ops, M, N, K):
    """The persistent kernel's fp16 form walks tiles with the ping-pong kernel's MFMA order and epilogue arithmetic: bit-identical."""
    from bioscanclip.hip.lib import EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_BF16
    h = torch.float16
    a = rnd(M, K, seed=1).to(h).cuda()
    b = rnd(N, K, seed=2, scale=0.1).to(h).cuda()
    bias = rnd(N, seed=3).cuda()
    rh = rnd(M, N, seed=4).to(h).cuda()
    zz = torch.randint(0, 256, (M, N), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()

    def run():
        outs = []
        for epi, dt, kw in ((EPI_F32, torch.float32, dict(bias=bias)), (EPI_BF16, h, dict(bias=bias)),
                            (EPI_GELU_BF16, h, dict(bias=bias)), (EPI_RESID_BF16, h, dict(bias=bias, resid=rh, dropout=(0.1, 77))),
                            (EPI_DGELU_BF16, h, dict(aux=zz))):
            out = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
            ops.gemm(a, b, out, epi, **kw)
            outs.append(out)
        return outs

    try:
        ops.set_gemm_tile(4)
        ref = run()
        ops.set_gemm_tile(8)
        ops.set_gemm_persistent_grid(5)
        got = run()
    finally:
        ops.set_gemm_tile(0)
        ops.set_gemm_persistent_grid(0)
    for i, (x, y) in enumerate(zip(ref, got)):
        assert torch.equal(x, y), i


def test_gemm_fp16_host_checks(ops):
    from bioscanclip.hip.lib import EPI_BF16, EPI_RESID_BF16
    a = torch.zeros(256, 64, device="cuda", dtype=torch.float16)
    with pytest.raises(ValueError, match="both bf16 or both fp16"):
        ops.gemm(a, a.bfloat16(), torch.empty(256, 256, device="cuda", dtype=torch.float16), EPI_BF16)
    with pytest.raises(ValueError, match="out dtype"):
        ops.gemm(a, a, torch.empty(256, 256, device="cuda", dtype=torch.bfloat16), EPI_BF16)
    with pytest.raises(ValueError, match="resid"):
        ops.gemm(a, a, torch.empty(256, 256, device="cuda", dtype=torch.float16), EPI_RESID_BF16,
                 resid=torch.zeros(256, 256, device="cuda", dtype=torch.bfloat16))
