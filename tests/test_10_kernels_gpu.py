"""Kernel-level parity: every C-ABI entry point vs an fp32 torch restatement of the same op on identical
(bf16-rounded where the kernel consumes bf16) inputs.  Tolerances: f32 outputs 2e-5 normwise (accumulation
order only); bf16 outputs 4e-3 normwise (one bf16 rounding = 2^-9 relative per element)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_err  # noqa: E402

TOL_F32 = 2e-5
TOL_BF16 = 4e-3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    return o


def dev(t):
    return t.to("cuda")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def dgelu(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


# ------------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("M,N,K", [(300, 256, 64), (300, 256, 128), (1000, 768, 832), (2500, 512, 576), (197 * 8, 2304, 832),
                                   (5120, 768, 3072)])
def test_gemm_epilogues(ops, tile, M, N, K):
    from bioscanclip.hip.lib import (EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_BF16, EPI_RESID_F32)
    ops.set_gemm_tile(tile)
    try:
        a = dev(rnd(M, K + 16, seed=1).bfloat16())[:, :K]      # row stride > K on purpose
        b = dev(rnd(N, K, seed=2, scale=0.1).bfloat16())
        bias = dev(rnd(N, seed=3))
        ref = a.float() @ b.float().t() + bias
        out32 = torch.full((M + 3, N), float("nan"), device="cuda")
        ops.gemm(a, b, out32, EPI_F32, bias=bias, M=M)
        assert rel_err(out32[:M], ref) < TOL_F32
        assert torch.isnan(out32[M:]).all(), "rows beyond M were written"
        out16 = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        ops.gemm(a, b, out16, EPI_BF16, bias=bias)
        assert rel_err(out16.float(), ref) < TOL_BF16
        ops.gemm(a, b, out16, EPI_BF16)  # no bias
        assert rel_err(out16.float(), ref - bias) < TOL_BF16
        # GELU with saved pre-activation
        z = torch.empty(M, N, device="cuda", dtype=torch.uint8)
        ops.gemm(a, b, out16, EPI_GELU_BF16, bias=bias, aux=z)
        dg = z.float() * (1.26 / 255) - 0.13                     # side band = gelu'(pre-activation), 8-bit codes
        # half a code step + the table's error in phi (1/16 grid, first order: 2e-4 |x|, csrc/gemm_epilogue.h)
        assert (dg - dgelu(ref)).abs().max().item() < 0.5 * 1.26 / 255 + 6e-4
        assert rel_err(dg, dgelu(ref)) < TOL_BF16
        assert rel_err(out16.float(), gelu(ref)) < TOL_BF16
        # residual
        r = dev(rnd(M, N, seed=4))
        ops.gemm(a, b, out32, EPI_RESID_F32, bias=bias, resid=r, M=M)
        assert rel_err(out32[:M], ref + r) < TOL_F32
        # bf16 residual stream: the sum is formed in f32 and rounded once (resid bf16 with a row stride > N, as the BERT engine
        # passes the LayerNorm's K-augmented operand)
        rb = torch.zeros(M, N + 64, device="cuda", dtype=torch.bfloat16)
        rb[:, :N] = r.bfloat16()
        out16r = torch.full((M + 3, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        ops.gemm(a, b, out16r, EPI_RESID_BF16, bias=bias, resid=rb, M=M)
        assert torch.equal(out16r[:M], (out32[:M] - r + rb[:, :N].float()).bfloat16()) or \
            rel_err(out16r[:M].float(), ref + rb[:, :N].float()) < 2.5e-3     # = one bf16 rounding of the f32 sum
        assert torch.isnan(out16r[M:]).all(), "rows beyond M were written"
        # in-place residual (C aliases resid): used by the loss gradient accumulation
        acc = r.clone()
        ops.gemm(a, b, acc, EPI_RESID_F32, resid=acc)
        assert rel_err(acc, ref - bias + r) < TOL_F32
        # backward GELU scaling
        zz = torch.randint(0, 256, (M, N), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
        ops.gemm(a, b, out16, EPI_DGELU_BF16, aux=zz)
        assert rel_err(out16.float(), (ref - bias) * (zz.float() * (1.26 / 255) - 0.13)) < TOL_BF16
    finally:
        ops.set_gemm_tile(0)


@pytest.mark.parametrize("wgs", [1, 3, 7])
@pytest.mark.parametrize("M,N,K", [(2500, 512, 576), (1300, 768, 832), (900, 1024, 128), (197 * 8, 2304, 768)])
def test_gemm_persistent_walks_tiles(ops, wgs, M, N, K):
    """The persistent kernel (tile 8) with a grid far below the tile count: every workgroup walks several tiles, the next tile's
    first K-tile staged under the current one's last (odd and even K-tile counts flip the LDS set parity differently).  Same
    MFMA order and epilogue arithmetic as the ping-pong kernel: bit-identical outputs, rows beyond M untouched."""
    from bioscanclip.hip.lib import (EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_BF16, EPI_RESID_F32)
    a = dev(rnd(M, K + 16, seed=1).bfloat16())[:, :K]
    b = dev(rnd(N, K, seed=2, scale=0.1).bfloat16())
    bias = dev(rnd(N, seed=3))
    r = dev(rnd(M, N, seed=4))
    rb = r.bfloat16()
    zz = torch.randint(0, 256, (M, N), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    drop = (0.1, 1234)

    def run():
        outs = {}
        for name, epi, dt, kw in (("f32", EPI_F32, torch.float32, dict(bias=bias)), ("bf16", EPI_BF16, torch.bfloat16, dict(bias=bias)),
                                  ("bf16_nobias", EPI_BF16, torch.bfloat16, {}),
                                  ("gelu", EPI_GELU_BF16, torch.bfloat16, dict(bias=bias, aux="z")),
                                  ("resid32", EPI_RESID_F32, torch.float32, dict(bias=bias, resid=r)),
                                  ("resid16", EPI_RESID_BF16, torch.bfloat16, dict(bias=bias, resid=rb)),
                                  ("resid16_drop", EPI_RESID_BF16, torch.bfloat16, dict(bias=bias, resid=rb, dropout=drop)),
                                  ("dgelu", EPI_DGELU_BF16, torch.bfloat16, dict(aux=zz))):
            out = torch.full((M + 3, N), float("nan"), device="cuda", dtype=dt)
            if kw.get("aux") == "z":
                kw = dict(kw, aux=torch.zeros(M, N, device="cuda", dtype=torch.uint8))
                outs[name + "_aux"] = kw["aux"]
            ops.gemm(a, b, out, epi, M=M, **kw)
            outs[name] = out
        return outs

    try:
        ops.set_gemm_tile(4)
        ref = run()
        ops.set_gemm_tile(8)
        ops.set_gemm_persistent_grid(wgs)
        got = run()
    finally:
        ops.set_gemm_tile(0)
        ops.set_gemm_persistent_grid(0)
    for k in ref:
        assert torch.equal(ref[k][:M], got[k][:M]), k
        if ref[k].is_floating_point() and ref[k].shape[0] > M:
            assert torch.isnan(got[k][M:].float()).all(), f"{k}: rows beyond M were written"


def test_gemm_layout_identity(ops):
    """A = I with an asymmetric B catches row/col swaps in the C write (cdna guide 3)."""
    from bioscanclip.hip.lib import EPI_F32
    K = N = 256
    a = torch.eye(K, device="cuda", dtype=torch.bfloat16)
    b = (torch.arange(N, device="cuda")[:, None] * 2 + torch.arange(K, device="cuda")[None, :] % 7).float()
    b = b.bfloat16()
    for tile in (1, 2, 3, 4, 5, 8):
        ops.set_gemm_tile(tile)
        out = torch.empty(K, N, device="cuda")
        ops.gemm(a, b, out, EPI_F32)
        assert torch.equal(out, b.float().t().contiguous()), f"tile {tile}"
    ops.set_gemm_tile(0)


@pytest.mark.parametrize("M,N,K,splits", [(512, 256, 64 * 21, 7), (768, 768, 64 * 40, 8), (300, 512, 64 * 6, 1), (256, 256, 64 * 6, 3)])
def test_gemm_splitk_accumulates_in_fixed_order(ops, M, N, K, splits):
    """bsclip_gemm_splitk_f32 (weight gradients of full fine-tuning): C += A B^T with the reduction cut into K ranges; same
    values as the f32 product of the bf16 operands, added to what C held, and bitwise reproducible (ordered sum, no atomics)."""
    a, b = dev(rnd(M, K + 64, seed=1)).bfloat16(), dev(rnd(N, K + 64, seed=2)).bfloat16()   # leading dimensions > K
    c0 = dev(rnd(M, N, seed=3))
    ref = c0.double() + a[:, :K].double() @ b[:, :K].double().t()
    partial = torch.empty(splits * M * N, device="cuda")
    outs = []
    for _ in range(2):
        c = c0.clone()
        ops.gemm_splitk_f32(a, b, c, splits, partial, K=K)
        outs.append(c)
    assert rel_err(outs[0], ref) < TOL_F32
    assert torch.equal(outs[0], outs[1])
    with pytest.raises(Exception):
        ops.gemm_splitk_f32(a, b, c0.clone(), 2, partial, K=64 * 3)     # three K-tiles do not split in two


@pytest.mark.parametrize("R,C,ld_in", [(394, 768, 768), (1000, 832, 840), (64, 64, 64), (50432 // 8, 3072, 3072), (130, 200, 200)])
def test_transpose_and_fused_column_sums(ops, R, C, ld_in):
    """bsclip_transpose_bf16 (16-byte path and the element path for unaligned leading dimensions) and the fused
    bsclip_transpose_colsum_bf16: exact transpose, column sums equal to the f64 sums to f32 accumulation, added to what the
    output held, bitwise reproducible."""
    src = dev(rnd(R, ld_in, seed=4)).bfloat16()[:, :C]
    Rp = (R + 63) // 64 * 64
    dst = torch.zeros(C, Rp, device="cuda", dtype=torch.bfloat16)
    ops.transpose_bf16(src, R, C, dst)
    assert torch.equal(dst[:, :R], src.t()) and (dst[:, R:] == 0).all()
    odd = torch.zeros(C, R + 1, device="cuda", dtype=torch.bfloat16)      # ld_out % 8 != 0: element path
    ops.transpose_bf16(src, R, C, odd)
    assert torch.equal(odd[:, :R], src.t())
    if ld_in % 8 == 0:
        base = dev(rnd(C, seed=5))
        outs = []
        for _ in range(2):
            dst2 = torch.zeros(C, Rp, device="cuda", dtype=torch.bfloat16)
            cs = base.clone()
            ops.transpose_colsum_bf16(src, R, C, dst2, cs)
            assert torch.equal(dst2, dst)
            outs.append(cs)
        ref = base.double() + src.double().sum(0)
        assert (outs[0].double() - ref).abs().max().item() < 2e-5 * max(1.0, src.float().abs().sum(0).max().item())
        assert torch.equal(outs[0], outs[1])


def test_gemm_patch_epilogue(ops):
    from bioscanclip.hip.lib import EPI_PATCH_F32
    B = 3
    a = dev(rnd(B * 196, 768, seed=1).bfloat16())
    w = dev(rnd(768, 768, seed=2, scale=0.05).bfloat16())
    bias, pos = dev(rnd(768, seed=3)), dev(rnd(197, 768, seed=4))
    out = torch.full((B * 197, 768), float("nan"), device="cuda")      # NaN, not zeros: a class row the kernel wrote zeros to shows
    ops.gemm(a, w, out, EPI_PATCH_F32, bias=bias, resid=pos)
    ref = (a.float() @ w.float().t() + bias).reshape(B, 196, 768) + pos[1:]
    got = out.reshape(B, 197, 768)
    assert rel_err(got[:, 1:], ref) < TOL_F32
    assert torch.isnan(got[:, 0]).all(), "a class-token row was written"
    from bioscanclip.hip.lib import EPI_PATCH_BF16
    for tile in (1, 4, 5):
        ops.set_gemm_tile(tile)
        out16 = torch.full((B * 197, 768), float("nan"), device="cuda", dtype=torch.bfloat16)
        ops.gemm(a, w, out16, EPI_PATCH_BF16, bias=bias, resid=pos)
        ops.set_gemm_tile(0)
        got16 = out16.reshape(B, 197, 768)
        assert torch.equal(got16[:, 1:], got[:, 1:].bfloat16()), f"tile {tile}"      # the f32 result rounded once
        assert torch.isnan(got16[:, 0]).all(), f"tile {tile}: a class-token row was written"


def test_gemm_rejects_bad_shapes(ops):
    from bioscanclip.hip.lib import EPI_F32
    a = torch.zeros(64, 100, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(128, 100, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.gemm(a, b, torch.zeros(64, 128, device="cuda"), EPI_F32)


# ------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("H,eps", [(768, 1e-6), (512, 1e-12)])
@pytest.mark.parametrize("xbf16", [False, True])
def test_layernorm_fwd_bwd(ops, H, eps, xbf16):
    M = 1031
    x = dev(rnd(M, H, seed=1) * 2 + 0.3)
    if xbf16:
        x = x.bfloat16()
    g, b = dev(1 + 0.1 * rnd(H, seed=2)), dev(0.1 * rnd(H, seed=3))
    A = dev(rnd(8, H, seed=4, scale=0.05))
    ld = H + 64
    y16 = torch.full((M, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    y32 = torch.full((M, H), float("nan"), device="cuda")
    stats = torch.full((M, 2), float("nan"), device="cuda")
    ops.layernorm_fwd(x, g, b, eps, y_bf16=y16, y_f32=y32, lora_a=A, stats=stats)
    xf = x.float().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xf, (H,), g, b, eps)
    assert rel_err(y32, ref) < TOL_F32
    assert rel_err(y16[:, :H].float(), ref) < TOL_BF16
    assert rel_err(y16[:, H:H + 8].float(), ref @ A.t()) < TOL_BF16
    assert (y16[:, H + 8:] == 0).all()
    assert rel_err(stats[:, 0], xf.mean(-1)) < 1e-4
    # plain variant (no lora, no f32 copy)
    y16b = torch.full((M, H), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.layernorm_fwd(x, g, b, eps, y_bf16=y16b, stats=stats)
    assert rel_err(y16b.float(), ref) < TOL_BF16

    # backward, both modes, with and without the LoRA term
    g_resid = dev(rnd(M, H, seed=5))
    g_gemm = dev(rnd(M, H + 64, seed=6).bfloat16())[:, :H]
    dt = dev(rnd(M, 8, seed=7))
    for mode in (0, 1):
        for use_lora in (False, True):
            dy_ln = g_gemm.float() + (dt @ A if use_lora else 0)
            if mode == 1:
                dy_ln = dy_ln + g_resid
            (gx,) = torch.autograd.grad(ref, xf, dy_ln, retain_graph=True)
            want = gx + (g_resid if mode == 0 else 0)
            dx32 = torch.full((M, H), float("nan"), device="cuda")
            dx16 = torch.full((M, H), float("nan"), device="cuda", dtype=torch.bfloat16)
            ops.layernorm_bwd(x, stats, g, mode, g_resid=g_resid, g_gemm=g_gemm, dt=dt if use_lora else None,
                              lora_a=A if use_lora else None, dx_f32=dx32, dx_bf16=dx16)
            assert rel_err(dx32, want) < 5e-5, (mode, use_lora)
            assert rel_err(dx16.float(), want) < TOL_BF16
    # only a GEMM gradient (top of the ViT / MLM head)
    (gx,) = torch.autograd.grad(ref, xf, g_gemm.float())
    dx32 = torch.full((M, H), float("nan"), device="cuda")
    ops.layernorm_bwd(x, stats, g, 0, g_gemm=g_gemm, dx_f32=dx32)
    assert rel_err(dx32, gx) < 5e-5


# ------------------------------------------------------------------------------------------------- attention
def _attn_ref(qkv, B, S, heads, scale, bias):
    H = heads * 64
    q, k, v = [t.reshape(B, S, heads, 64).transpose(1, 2) for t in qkv.split(H, dim=-1)]
    s = (q @ k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias[:, None, None, :]
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(B * S, H), torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,S,heads,masked", [(3, 197, 12, False), (2, 133, 12, False), (5, 20, 8, True),
                                              (2, 64, 2, False), (1, 33, 1, False), (2, 7, 3, True),
                                              (2, 224, 2, True), (3, 1, 2, False), (1, 193, 1, True)])  # max S, S = 1
def test_attention_fwd_bwd(ops, B, S, heads, masked):
    H = heads * 64
    qkv = dev(rnd(B * S, 3 * H + 64, seed=1).bfloat16())[:, :3 * H]
    bias = None
    if masked:
        lens = torch.randint(1, S + 1, (B,), generator=torch.Generator().manual_seed(3))
        m = (torch.arange(S)[None] < lens[:, None]).float()
        bias = dev((1.0 - m) * torch.finfo(torch.float32).min)
    scale = 0.125
    ctx = torch.empty(B * S, H, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, heads, S, device="cuda")
    ops.attn_fwd(qkv, B, S, heads, scale, ctx, lse, key_bias=bias)
    qf = qkv.float().reshape(B, S, 3 * H).requires_grad_(True)
    ref, ref_lse = _attn_ref(qf, B, S, heads, scale, bias)
    assert rel_err(ctx.float(), ref) < 6e-3          # P is rounded to bf16 before P.V
    assert rel_err(lse, ref_lse) < 1e-5

    dctx = dev(rnd(B * S, H, seed=2).bfloat16())
    (gq,) = torch.autograd.grad(ref, qf, dctx.float())
    dqkv = torch.full((B * S, 3 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd(qkv, dctx, lse, B, S, heads, scale, dqkv, key_bias=bias)
    gq = gq.reshape(B * S, 3 * H)
    # S = 1: dQ = dK = 0 exactly in the reference (one key: dS = P (dP - delta) = 0).  Since round 5 the key-owner phase starts the dP
    # accumulator from -delta (the row constant as the MFMA chain's initial value), so dS is f32 rounding noise (~1e-7 of dP) instead
    # of an exact zero there: errors are measured against the whole gradient's norm
    floor = 1e-5 * gq.norm()
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        err = ((dqkv[:, sl].float() - gq[:, sl]).norm() / (gq[:, sl].norm() + floor)).item()
        assert err < 1e-2, (name, err)


@pytest.mark.parametrize("B,S,heads,q_rows", [(3, 197, 12, 1), (2, 133, 4, 40), (2, 20, 2, 1),
                                               (2, 100, 3, 33), (2, 161, 2, 1)])   # two of four blocks, one of six
def test_attention_leading_query_rows_only(ops, B, S, heads, q_rows):
    """q_rows: only the first rows of each sequence are wanted (last ViT block: token 0).  Forward must give the same ctx / lse
    on those rows; backward with dctx zero elsewhere must equal the full backward and write zeros into the other dq rows."""
    H = heads * 64
    qkv = dev(rnd(B * S, 3 * H, seed=4).bfloat16())
    ctx_full = torch.empty(B * S, H, device="cuda", dtype=torch.bfloat16)
    lse_full = torch.empty(B, heads, S, device="cuda")
    ops.attn_fwd(qkv, B, S, heads, 0.125, ctx_full, lse_full)
    ctx = torch.full((B * S, H), 7.0, device="cuda", dtype=torch.bfloat16)
    lse = torch.full((B, heads, S), 7.0, device="cuda")
    ops.attn_fwd(qkv, B, S, heads, 0.125, ctx, lse, q_rows=q_rows)
    rows = torch.arange(B)[:, None] * S + torch.arange(q_rows)[None]
    assert torch.equal(ctx[rows.reshape(-1)], ctx_full[rows.reshape(-1)])
    assert torch.equal(lse[:, :, :q_rows], lse_full[:, :, :q_rows])
    nq = min(S, (q_rows + 31) // 32 * 32)  # whole 32-row blocks are computed, nothing beyond them is touched
    assert (ctx.view(B, S, H)[:, nq:] == 7.0).all()
    dctx = torch.zeros(B * S, H, device="cuda", dtype=torch.bfloat16)
    dctx[rows.reshape(-1)] = dev(rnd(B * q_rows, H, seed=5).bfloat16())
    full = torch.empty(B * S, 3 * H, device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd(qkv, dctx, lse_full, B, S, heads, 0.125, full)
    part = torch.full((B * S, 3 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd(qkv, dctx, lse, B, S, heads, 0.125, part, q_rows=q_rows)  # lse holds 7.0 outside the wanted blocks
    assert torch.equal(part, full)
    assert (part.view(B, S, 3 * H)[:, nq:, :H] == 0).all()
    with pytest.raises(RuntimeError):
        ops.attn_fwd(qkv, B, S, heads, 0.125, ctx, lse, q_rows=S + 1)


def test_attention_rejects_unsupported_shapes(ops):
    qkv = dev(rnd(2 * 225, 3 * 64, seed=1).bfloat16())
    ctx = torch.empty(2 * 225, 64, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(2, 1, 225, device="cuda")
    with pytest.raises(RuntimeError):
        ops.attn_fwd(qkv, 2, 225, 1, 0.125, ctx, lse)  # S > 224
    with pytest.raises(ValueError):
        ops.attn_fwd(qkv.float(), 2, 225, 1, 0.125, ctx, lse)  # dtype


# ------------------------------------------------------------------------------------------ embeddings / misc
def test_im2col_and_cls(ops):
    B = 3
    img = dev(torch.rand(B, 3, 224, 224, generator=torch.Generator().manual_seed(1)))
    cols = torch.empty(B * 196, 768, device="cuda", dtype=torch.bfloat16)
    ops.im2col_patch16(img, cols)
    ref = img.reshape(B, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(B * 196, 768)
    assert torch.equal(cols, ref.bfloat16())
    # split-bf16 rows [hi | lo | hi] and the K = 2304 product against [hi | hi | lo] weights: ~2^-16 instead of 2^-8 relative
    from bioscanclip.hip.lib import EPI_F32
    cols3 = torch.empty(B * 196, 2304, device="cuda", dtype=torch.bfloat16)
    ops.im2col_patch16(img, cols3)
    hi = ref.bfloat16()
    assert torch.equal(cols3[:, :768], hi) and torch.equal(cols3[:, 1536:], hi)
    assert torch.equal(cols3[:, 768:1536], (ref - hi.float()).bfloat16())
    w = dev(rnd(768, 768, seed=7, scale=0.05))
    w = w - w.mean(dim=1, keepdim=True)                       # zero-sum filters: the regime where operand rounding costs most
    w_hi = w.bfloat16()
    w3 = torch.cat([w_hi, w_hi, (w - w_hi.float()).bfloat16()], dim=1).contiguous()
    exact = (ref.double() @ w.double().t()).float()
    out3, out1 = torch.empty(B * 196, 768, device="cuda"), torch.empty(B * 196, 768, device="cuda")
    ops.gemm(cols3, w3, out3, EPI_F32)
    ops.gemm(cols, w_hi, out1, EPI_F32)
    assert rel_err(out3, exact) < 3e-5 and rel_err(out1, exact) > 1e-3, (rel_err(out3, exact), rel_err(out1, exact))
    x = torch.zeros(B * 197, 768, device="cuda")
    cls, pos = dev(rnd(768, seed=2)), dev(rnd(197, 768, seed=3))
    ops.vit_cls_rows(x, cls, pos, B, 197, 768)
    got = x.reshape(B, 197, 768)
    assert torch.equal(got[:, 0], (cls + pos[0]).expand(B, -1)) and (got[:, 1:] == 0).all()
    xb = torch.zeros(B * 197, 768, device="cuda", dtype=torch.bfloat16)
    ops.vit_cls_rows(xb, cls, pos, B, 197, 768)
    assert torch.equal(xb.reshape(B, 197, 768)[:, 0], (cls + pos[0]).bfloat16().expand(B, -1))


@pytest.mark.parametrize("H,vocab", [(768, 1027), (512, 30522)])
def test_bert_embed(ops, H, vocab):
    B, S = 4, 20
    g = torch.Generator().manual_seed(1)
    ids = dev(torch.randint(0, vocab, (B, S), generator=g))
    tt = dev(torch.randint(0, 2, (B, S), generator=g))
    word, pos, typ = dev(rnd(vocab, H, seed=2)), dev(rnd(512, H, seed=3)), dev(rnd(2, H, seed=4))
    out = torch.empty(B * S, H, device="cuda")
    ops.bert_embed(ids, tt, word, pos, typ, out)
    ref = word[ids] + pos[:S][None] + typ[tt]
    assert rel_err(out, ref.reshape(B * S, H)) < 1e-6
    ops.bert_embed(ids, None, word, pos, typ, out)
    assert rel_err(out, (word[ids] + pos[:S][None] + typ[0]).reshape(B * S, H)) < 1e-6


def test_softmax_meanpool(ops):
    B, S, C = 5, 133, 768
    logits = dev(rnd(B * S, C, seed=1, scale=3.0)).requires_grad_(True)
    pooled = torch.empty(B, C, device="cuda")
    stats = torch.empty(B * S, 2, device="cuda")
    ops.softmax_meanpool_fwd(logits.detach(), B, S, pooled, stats)
    ref = torch.softmax(logits.reshape(B, S, C), -1).mean(1)
    assert rel_err(pooled, ref) < TOL_F32
    assert abs(pooled.sum(-1) - 1).max() < 1e-5
    dp = dev(rnd(B, C, seed=2))
    (gl,) = torch.autograd.grad(ref, logits, dp)
    dl = torch.empty(B * S, C, device="cuda", dtype=torch.bfloat16)
    ops.softmax_meanpool_bwd(logits.detach(), stats, dp, B, S, dl)
    assert rel_err(dl.float(), gl) < TOL_BF16


def test_meanpool_and_l2norm(ops):
    B, S, H = 6, 20, 512
    x = dev(rnd(B * S, H, seed=1))
    out = torch.empty(B, H, device="cuda", dtype=torch.bfloat16)
    ops.meanpool_tokens_fwd(x, B, S, out)
    assert rel_err(out.float(), x.reshape(B, S, H).mean(1)) < TOL_BF16
    dp = dev(rnd(B, 768, seed=2))[:, :H]  # strided
    dx = torch.empty(B * S, H, device="cuda")
    ops.meanpool_tokens_bwd(dp, B, S, dx)
    assert rel_err(dx.reshape(B, S, H), (dp / S)[:, None].expand(B, S, H)) < 1e-6

    z = dev(rnd(37, 768, seed=3)).requires_grad_(True)
    y, inv = torch.empty(37, 768, device="cuda"), torch.empty(37, device="cuda")
    ops.l2norm_fwd(z.detach(), y, inv)
    ref = torch.nn.functional.normalize(z, p=2, dim=-1)
    assert rel_err(y, ref) < 1e-6
    dy = dev(rnd(37, 768, seed=4))
    (gz,) = torch.autograd.grad(ref, z, dy)
    dz = torch.empty(37, 768, device="cuda")
    ops.l2norm_bwd(y, inv, dy, dz)
    assert rel_err(dz, gz) < 1e-5


# ------------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("N,nmod,dup", [(8, 2, False), (8, 3, True), (64, 3, True), (200, 2, True), (256, 2, False),
                                        (256, 3, True), (1300, 2, True)])
def test_infonce_vs_oracle(ops, N, nmod, dup):
    from oracle import refcpu
    zs = [rnd(N, 768, seed=10 + i) for i in range(nmod)]
    label = torch.arange(N)
    if dup:
        label = label // 3 * 3 if N > 8 else torch.tensor([0, 0, 1, 2, 3, 3, 3, 4])
    zc = [z.clone().requires_grad_(True) for z in zs]
    ref = refcpu.contrastive_loss(zc[0], zc[1], zc[2] if nmod == 3 else None, label)
    ref.backward()
    zd = [dev(z) for z in zs]
    dz = [torch.empty(N, 768, device="cuda") for _ in range(nmod)]
    loss = torch.zeros(1, device="cuda")
    ws = torch.empty(ops.infonce_workspace_floats(N, nmod), device="cuda")
    ops.infonce_fwd_bwd(zd, dev(label), 1 / 0.07, loss, dz, workspace=ws)
    assert abs(loss.item() - ref.item()) < 2e-5 * abs(ref.item()), (loss.item(), ref.item())
    for i in range(nmod):
        assert rel_err(dz[i], zc[i].grad) < 2e-4, i
    # local slice of an all-gathered batch: rows [row0, row0+n_local) only
    if N >= 64:
        row0, nl = N // 4, N // 2
        dzl = [torch.empty(nl, 768, device="cuda") for _ in range(nmod)]
        ops.infonce_fwd_bwd(zd, dev(label), 1 / 0.07, loss, dzl, row0=row0, n_local=nl, workspace=ws)
        for i in range(nmod):
            assert rel_err(dzl[i], zc[i].grad[row0:row0 + nl]) < 2e-4


def test_infonce_too_few_modalities(ops):
    with pytest.raises(ValueError, match="Too less element"):
        ops.infonce_fwd_bwd([torch.zeros(8, 768, device="cuda")], torch.arange(8, device="cuda"), 1.0,
                            torch.zeros(1, device="cuda"))


# --------------------------------------------------------------------------------------- LoRA grads / optimiser
@pytest.mark.parametrize("H", [768, 512])
def test_lora_grad(ops, H):
    M = 2077
    dqkv = dev(rnd(M, 3 * H, seed=1).bfloat16())
    h = dev(rnd(M, H + 64, seed=2).bfloat16())
    lb = dev(rnd(2, H, 4, seed=3, scale=0.1))
    dt = torch.full((M, 8), float("nan"), device="cuda")
    dA, dBq, dBv = torch.zeros(8, H, device="cuda"), torch.zeros(H, 4, device="cuda"), torch.zeros(H, 4, device="cuda")
    ops.lora_grad(dqkv, h, M, H, lb, dt, dA, dBq, dBv)
    dq, dv = dqkv[:, :H].float(), dqkv[:, 2 * H:].float()
    y, tq, tv = h[:, :H].float(), h[:, H:H + 4].float(), h[:, H + 4:H + 8].float()
    ref_dt = torch.cat([dq @ lb[0], dv @ lb[1]], 1)
    assert rel_err(dt, ref_dt) < 1e-5
    assert rel_err(dA, ref_dt.t() @ y) < 1e-4
    assert rel_err(dBq, dq.t() @ tq) < 1e-4
    assert rel_err(dBv, dv.t() @ tv) < 1e-4
    ops.lora_grad(dqkv, h, M, H, lb, dt, dA, dBq, dBv)  # accumulates
    assert rel_err(dA, 2 * ref_dt.t() @ y) < 1e-4


@pytest.mark.parametrize("B,S,heads,p,q_rows", [(3, 197, 12, 0.0, 0), (3, 133, 12, 0.1, 0), (2, 197, 12, 0.0, 1), (5, 20, 8, 0.1, 0),
                                                (2, 64, 8, 0.0, 0), (9, 1, 12, 0.0, 0), (2, 224, 12, 0.1, 0), (2, 100, 8, 0.0, 40),
                                                # the LoRA forms at the remaining block counts: keep words at NB = 2 .. 6 (5 = the
                                                # generic form, not S = 133's), preloaded delta at NB = 3, 5, 6
                                                (2, 40, 8, 0.1, 0), (1, 70, 8, 0.1, 0), (2, 70, 8, 0.0, 0), (1, 100, 8, 0.1, 0),
                                                (1, 150, 8, 0.1, 0), (2, 150, 8, 0.0, 0), (1, 170, 8, 0.1, 0), (1, 170, 8, 0.0, 0)])
def test_lora_grad_from_attention_partials(ops, B, S, heads, p, q_rows):
    """bsclip_attn_bwd_lora + bsclip_lora_grad_heads (round 5: dt and dB as MFMA products of dq / dv while they sit in the attention
    backward's accumulators, per head and per sequence, reduced in a fixed order) against bsclip_attn_bwd + bsclip_lora_grad, which read
    dq and dv back from HBM: the same dqkv bit for bit, dt / dA / dB to f32 accumulation order (B enters as hi + lo bf16 parts)."""
    H, M = heads * 64, B * S
    qkv = dev(rnd(M, 3 * H, seed=1).bfloat16())
    h = dev(rnd(M, H + 64, seed=2).bfloat16())
    lb = dev(rnd(2, H, 4, seed=3, scale=0.1))
    dctx = dev(rnd(M, H, seed=4).bfloat16())
    if q_rows:
        keep = torch.zeros(B, S, 1, dtype=torch.bool)
        keep[:, :q_rows] = True
        dctx = torch.where(dev(keep.reshape(M, 1)), dctx, torch.zeros_like(dctx))
    drop = (p, 777) if p else None
    ctx = torch.empty(M, H, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, heads, S, device="cuda")
    bits = torch.zeros(B * heads * S * ops.KEEP_WORDS, device="cuda", dtype=torch.int32) if p else None
    ops.attn_fwd(qkv, B, S, heads, 0.125, ctx, lse, dropout=drop, keep_bits=bits)

    def grads():
        return (torch.full((M, 8), float("nan"), device="cuda"), torch.zeros(8, H, device="cuda"), torch.zeros(H, 4, device="cuda"),
                torch.zeros(H, 4, device="cuda"))
    ref_d = torch.empty(M, 3 * H, device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd(qkv, dctx, lse, B, S, heads, 0.125, ref_d, dropout=drop, q_rows=q_rows, keep_bits=bits)
    rdt, rdA, rdBq, rdBv = grads()
    ops.lora_grad(ref_d, h, M, H, lb, rdt, rdA, rdBq, rdBv)

    dqkv = torch.full((M, 3 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
    dtp = torch.full((heads, 2, M, 4), float("nan"), device="cuda")
    dbp = torch.full((B * heads, 2, 4, 64), float("nan"), device="cuda")
    ops.attn_bwd(qkv, dctx, lse, B, S, heads, 0.125, dqkv, dropout=drop, q_rows=q_rows, keep_bits=bits, lora=(h[:, H:], lb, dtp, dbp))
    assert torch.equal(dqkv, ref_d)
    assert torch.isfinite(dtp).all() and torch.isfinite(dbp).all()
    dt, dA, dBq, dBv = grads()
    ops.lora_grad_heads(h, M, H, B, dtp, dbp, dt, dA, dBq, dBv)
    # direct f64 products from the same bf16 dq / dv
    dq, dv = ref_d[:, :H].double(), ref_d[:, 2 * H:].double()
    t = h[:, H:H + 8].double()
    want_dt = torch.cat([dq @ lb[0].double(), dv @ lb[1].double()], 1)
    for name, got, old, want in (("dt", dt, rdt, want_dt), ("dA", dA, rdA, want_dt.t() @ h[:, :H].double()),
                                 ("dBq", dBq, rdBq, dq.t() @ t[:, :4]), ("dBv", dBv, rdBv, dv.t() @ t[:, 4:])):
        floor = 1e-6 * want.norm() + 1e-30
        err = ((got.double() - want).norm() / (want.norm() + floor)).item()
        err_old = ((old.double() - want).norm() / (want.norm() + floor)).item()
        assert err < 2e-5, (name, err, err_old)
    ops.lora_grad_heads(h, M, H, B, dtp, dbp, dt, dA, dBq, dBv)   # accumulates into dA / dB like lora_grad, dt is overwritten
    assert rel_err(dA, 2 * want_dt.t().float() @ h[:, :H].float()) < 1e-4 and rel_err(dBv, 2 * (dv.t() @ t[:, 4:]).float()) < 1e-4
    again = grads()
    ops.lora_grad_heads(h, M, H, B, dtp, dbp, *again)            # fixed summation order: bit-reproducible
    first = grads()
    ops.lora_grad_heads(h, M, H, B, dtp, dbp, *first)
    assert all(torch.equal(a, b) for a, b in zip(again, first))


def test_small_ops(ops):
    g16 = dev(rnd(1000, 768, seed=1).bfloat16())
    out = torch.zeros(768, device="cuda")
    ops.colsum(g16, 1000, 768, out)
    assert rel_err(out, g16.float().sum(0)) < 1e-5
    g32 = dev(rnd(77, 512, seed=2))
    out = torch.ones(512, device="cuda")
    ops.colsum(g32, 77, 512, out)
    assert rel_err(out, 1 + g32.sum(0)) < 1e-5
    # narrow fallback (N not a multiple of 8, strided view) and a large bf16 case twice: bitwise reproducible
    g3 = dev(rnd(333, 40, seed=5))[:, :36]
    out = torch.zeros(36, device="cuda")
    ops.colsum(g3, 333, 36, out)
    assert rel_err(out, g3.sum(0)) < 1e-5
    g3b = dev(rnd(333, 40, seed=5).bfloat16())[:, :36]   # the fallback on bf16
    out = torch.zeros(36, device="cuda")
    ops.colsum(g3b, 333, 36, out)
    assert rel_err(out, g3b.float().sum(0)) < 1e-5
    big = dev(rnd(34048, 768, seed=6).bfloat16())
    o1, o2 = torch.zeros(768, device="cuda"), torch.zeros(768, device="cuda")
    ops.colsum(big, 34048, 768, o1)
    ops.colsum(big, 34048, 768, o2)
    assert torch.equal(o1, o2) and rel_err(o1, big.double().sum(0)) < 1e-5
    src = dev(rnd(300, 200, seed=3).bfloat16())
    dst = torch.zeros(200, 304, device="cuda", dtype=torch.bfloat16)
    ops.transpose_bf16(src, 300, 200, dst)
    assert torch.equal(dst[:, :300], src.t()) and (dst[:, 300:] == 0).all()
    x = dev(rnd(1003, seed=4))
    y = torch.full((1003,), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.cast_f32_bf16(x, y)
    assert torch.equal(y, x.bfloat16())
    w = torch.zeros(3 * 768, 832, device="cuda", dtype=torch.bfloat16)
    bq, bv = dev(rnd(768, 4, seed=5)), dev(rnd(768, 4, seed=6))
    table = torch.tensor([[w.data_ptr(), bq.data_ptr(), bv.data_ptr()]], dtype=torch.int64, device="cuda")
    ops.waug_set_lora_layers(table, 1, w.stride(0), 768)
    assert torch.equal(w[:768, 768:772], bq.bfloat16()) and torch.equal(w[1536:, 772:776], bv.bfloat16())
    w[:768, 768:772] = 0
    w[1536:, 772:776] = 0
    assert (w == 0).all(), "waug_set_lora wrote outside the two LoRA-B blocks"


def test_adamw_matches_oracle_and_torch(ops):
    from oracle import refcpu
    n = 100003
    p0, g = rnd(n, seed=1), rnd(n, seed=2, scale=1e-3)
    p, m, v = dev(p0.clone()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pr, mr, vr = p0.clone(), torch.zeros(n), torch.zeros(n)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-3)
    for step in range(1, 4):
        gs = g * step
        ops.adamw_step(p, dev(gs), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step)
        refcpu.adamw_update(pr, gs, mr, vr, step, 1e-3)
        pt.grad = gs.clone()
        opt.step()
    assert rel_err(p, pr) < 1e-6
    assert rel_err(p, pt) < 1e-6


@pytest.mark.parametrize("N,nmod", [(256, 2), (700, 3), (2048, 3)])
def test_infonce_fused_epilogues_vs_logits_slabs(ops, N, nmod):
    """The fused form (logits tile reduced in the GEMM's accumulators, dL/dG emitted from them) against round 1's form that
    writes f32 logits slabs and reduces them with separate kernels: two implementations of the same arithmetic.  Timings of
    both go to gpurun_out/infonce_timing.jsonl."""
    import json
    import os
    zs = [dev(torch.nn.functional.normalize(rnd(N, 768, seed=40 + i) + 0.3 * rnd(1, 768, seed=50), dim=-1)) for i in range(nmod)]
    label = dev(torch.arange(N) // 2 * 2)
    ws = torch.empty(ops.infonce_workspace_floats(N, nmod), device="cuda")
    res, ms = {}, {}
    try:
        for impl in (2, 1):   # 2 = fused epilogues (forced), 1 = logits slabs; 0 = by size is the default
            ops.infonce_set_impl(impl)
            loss = torch.zeros(1, device="cuda")
            dz = [torch.empty(N, 768, device="cuda") for _ in range(nmod)]
            ops.infonce_fwd_bwd(zs, label, 1 / 0.07, loss, dz, workspace=ws)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                ops.infonce_fwd_bwd(zs, label, 1 / 0.07, loss, dz, workspace=ws)
            e1.record()
            torch.cuda.synchronize()
            ms[impl] = e0.elapsed_time(e1) / 5
            res[impl] = (loss.item(), [d.clone() for d in dz])
    finally:
        ops.infonce_set_impl(0)
    assert abs(res[2][0] - res[1][0]) < 2e-6 * abs(res[1][0]), (res[2][0], res[1][0])
    for a, b in zip(res[2][1], res[1][1]):
        assert rel_err(a, b) < 2e-5
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/infonce_timing.jsonl", "a") as f:
        f.write(json.dumps({"N": N, "nmod": nmod, "fused_ms": ms[2], "slab_ms": ms[1]}) + "\n")


# ------------------------------------------------------------------------------- full fine-tuning kernels
@pytest.mark.parametrize("H,vocab,B,S,types", [(768, 1027, 6, 133, False), (512, 30522, 5, 20, True)])
def test_embed_grad_matches_autograd_and_is_ordered(ops, H, vocab, B, S, types):
    """bsclip_embed_grad vs autograd of the three HF BertEmbeddings lookups (word with padding_idx = 0, position, token type);
    added to what the tables held; bitwise reproducible (no atomics)."""
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, vocab, (B, S), generator=g)
    ids[:, 0] = 0                                     # the padding row: no gradient
    ids[1, 5:9] = ids[0, 5]                           # repeated ids across and within samples
    tt = torch.randint(0, 2, (B, S), generator=g) if types else None
    d = rnd(B * S, H, seed=4)
    word = torch.zeros(vocab, H, requires_grad=True)
    pos = torch.zeros(S + 3, H, requires_grad=True)
    typ = torch.zeros(2, H, requires_grad=True)
    e = torch.nn.functional.embedding(ids, word, padding_idx=0) + pos[:S][None] + \
        torch.nn.functional.embedding(tt if types else torch.zeros_like(ids), typ)
    (e.reshape(B * S, H) * d).sum().backward()
    outs = []
    for _ in range(2):
        dw, dp, dty = (torch.full((vocab, H), 0.5, device="cuda"), torch.full((S + 3, H), 0.25, device="cuda"),
                       torch.full((2, H), -1.0, device="cuda"))
        ops.embed_grad(dev(ids), dev(tt) if types else None, dev(d), dw, dp, dty, pad_id=0)
        outs.append((dw, dp, dty))
    dw, dp, dty = outs[0]
    assert rel_err(dw - 0.5, word.grad) < TOL_F32 and (dw[0] == 0.5).all()
    assert rel_err(dp - 0.25, pos.grad) < TOL_F32 and rel_err(dty + 1.0, typ.grad) < TOL_F32
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


@pytest.mark.parametrize("H,xbf16", [pytest.param(768, False, id="768"), pytest.param(512, False, id="512"),
                                     pytest.param(512, True, id="512-x16")])
def test_ln_param_grad(ops, H, xbf16):
    """d_gamma / d_beta of a LayerNorm whose upstream gradient is assembled like layernorm_bwd assembles it (bf16 GEMM output +
    f32 residual gradient + the LoRA term dt . A)."""
    M = 777
    x = dev(rnd(M, H, seed=1) * 2 + 0.3)
    if xbf16:   # the 16-bit stream: the kernel and the reference below see the same rounded x
        x = x.bfloat16()
    gamma, beta = dev(rnd(H, seed=2) * 0.2 + 1), dev(rnd(H, seed=3) * 0.1)
    y, stats = torch.full((M, H + 64), float("nan"), device="cuda", dtype=torch.bfloat16), torch.full((M, 2), float("nan"), device="cuda")
    ops.layernorm_fwd(x, gamma, beta, 1e-6, y_bf16=y, stats=stats)
    g_gemm = dev(rnd(M, H, seed=4)).bfloat16()
    g_resid = dev(rnd(M, H, seed=5))
    dt, la = dev(rnd(M, 8, seed=6)), dev(rnd(8, H, seed=7) * 0.1)
    dy = g_gemm.float() + g_resid + dt @ la
    xf = x.float()
    xhat = (xf - xf.mean(1, keepdim=True)) / torch.sqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-6)
    dg, db = dev(rnd(H, seed=8)), dev(rnd(H, seed=9))
    dg0, db0 = dg.clone(), db.clone()
    ops.ln_param_grad(x, stats, 1, dg, db, g_resid=g_resid, g_gemm=g_gemm, dt=dt, lora_a=la)
    assert rel_err(dg - dg0, (dy * xhat).sum(0)) < 5e-5 and rel_err(db - db0, dy.sum(0)) < 5e-5


def test_gather_cast_rows(ops):
    src = dev(rnd(3 * 197, 768, seed=1))
    dst = torch.empty(3 * 196, 768, device="cuda", dtype=torch.bfloat16)
    ops.gather_cast_rows(src, 3 * 196, 197, 196, 1, dst)
    assert torch.equal(dst, src.view(3, 197, 768)[:, 1:].reshape(-1, 768).bfloat16())


def test_clock_probe_reads_a_plausible_engine_clock(ops):
    """bsclip_clock_probe: per-XCD shader-clock and 100 MHz counters; two probes around some work give a clock between the
    idle and the peak engine clock, and the real-time delta matches the host's clock."""
    import time
    p0, p1 = torch.zeros(32, dtype=torch.int64, device="cuda"), torch.zeros(32, dtype=torch.int64, device="cuda")
    a = torch.randn(4096, 4096, device="cuda")
    for _ in range(40):            # library initialisation and the clock's ramp from idle stay outside the measured window
        a = a @ a * 1e-3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.clock_probe(p0)
    for _ in range(40):
        a = a @ a * 1e-3
    ops.clock_probe(p1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ghz = ops.engine_clock_ghz(p0, p1)
    assert ghz is not None and 0.5 < ghz < 3.0, ghz
    q0, q1 = p0.cpu().view(16, 2), p1.cpu().view(16, 2)
    seen = [x for x in range(16) if q0[x, 1] and q1[x, 1]]
    assert len(seen) >= 1
    ticks = max(int(q1[x, 1] - q0[x, 1]) for x in seen)          # 100 MHz
    assert 0.3 * dt < ticks / 1e8 < 1.05 * dt + 1e-3, (ticks, dt)   # the probes run inside [t0, t0 + dt]; enqueue leads execution


# ------------------------------------------------------------------------------ exact mode (BSCLIP_PARITY=2) kernels
@pytest.mark.parametrize("impl", [0, 2])
@pytest.mark.parametrize("B,S,heads,masked", [(3, 197, 12, False), (2, 133, 12, False), (5, 20, 8, True), (2, 224, 2, True),
                                              (3, 1, 2, False), (2, 7, 3, True), (1, 64, 1, False), (1, 193, 2, True)])
def test_exact_attention_fwd_bwd_f32(ops, B, S, heads, masked, impl):
    """impl 0 (the default since round 5): every product of the attention on split-bf16 operands (hi.hi + lo.hi + hi.lo, ~2^-16 per
    product: csrc/attn_x3.hip) -- bars 5e-5 (output), 1e-5 (lse), 2e-4 (gradients), an order of magnitude inside north_star's 1e-3;
    impl 2: the f32-operand MFMA kernels (exact f32 chains), held to f32 rounding:
    bsclip_attn_fwd_f32 / bsclip_attn_bwd_f32 against autograd in f64: f32 arithmetic end to end, so the bar is 2e-5, not the
    6e-3 / 1e-2 of the bf16 kernels (reference: timm Attention / HF BertSelfAttention)."""
    H = heads * 64
    qkv = dev(rnd(B * S, 3 * H + 64, seed=1))[:, :3 * H]
    bias = None
    if masked:
        lens = torch.randint(1, S + 1, (B,), generator=torch.Generator().manual_seed(3))
        m = (torch.arange(S)[None] < lens[:, None]).float()
        bias = dev((1.0 - m) * torch.finfo(torch.float32).min)
    scale = 0.125
    ctx = torch.empty(B * S, H, device="cuda")
    lse = torch.empty(B, heads, S, device="cuda")
    ops.exact_attn_set_impl(impl)        # (tests/conftest.py resets the switch after every GPU test)
    tol_out, tol_lse, tol_g = {0: (5e-5, 1e-5, 2e-4), 2: (TOL_F32, 1e-6, 3e-5)}[impl]
    c3 = torch.full((B * S, 3 * H + 8), float("nan"), device="cuda", dtype=torch.bfloat16)[:, :3 * H]
    ops.attn_fwd_f32(qkv, B, S, heads, scale, ctx, lse, key_bias=bias, ctx_split3=c3)
    # the split output IS the split of the f32 output: [hi | lo | hi] as bsclip_split3_rows builds it (the out-projection GEMM's operand)
    assert torch.equal(c3, ops.split3_rows(ctx, torch.empty(B * S, 3 * H, device="cuda", dtype=torch.bfloat16)))
    qf = qkv.double().reshape(B, S, 3 * H).requires_grad_(True)
    ref, ref_lse = _attn_ref(qf, B, S, heads, scale, None if bias is None else bias.double())
    assert rel_err(ctx, ref.float()) < tol_out and rel_err(lse, ref_lse.float()) < tol_lse, (rel_err(ctx, ref.float()), rel_err(lse, ref_lse.float()))
    dctx = dev(rnd(B * S, H, seed=2))
    (gq,) = torch.autograd.grad(ref, qf, dctx.double())
    gq = gq.reshape(B * S, 3 * H).float()
    dqkv = torch.full((B * S, 3 * H), float("nan"), device="cuda")
    d3 = torch.full((B * S, 9 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd_f32(qkv, dctx, ctx, lse, B, S, heads, scale, dqkv, key_bias=bias, dqkv_split3=d3)
    assert torch.equal(d3, ops.split3_rows(dqkv, torch.empty(B * S, 9 * H, device="cuda", dtype=torch.bfloat16)))
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        # S = 1: dq = dk = 0 in the reference (one key: dS = P (dP - delta) = 0); here dP and delta are two f32 summation orders of
        # the same dot product, so dS is rounding noise (1e-7 of the gradient's scale): measured against the whole gradient then
        # (impl 0 at S = 1: dP carries the split products' 2^-16, delta = dO . O is f32: the noise is 3e-6 of the gradient's norm)
        e = ((dqkv[:, sl] - gq[:, sl]).norm() / torch.maximum(gq[:, sl].norm(), 1e-2 * gq.norm())).item()
        assert e < (1e-3 if impl == 0 and S == 1 else tol_g), (name, e)


def test_exact_attention_dropout_masks_are_the_bf16_kernels(ops):
    """The f32 attention draws the (seed, element) masks of the bf16 kernels: with the same seed its output and gradients stay at
    bf16 distance from theirs (a different mask on 10 % of the probabilities would be an O(0.3) difference), and its backward is
    the exact derivative of its forward under that mask (central finite difference in the direction of a random perturbation)."""
    B, S, heads = 2, 133, 4
    H = heads * 64
    qkv = dev(rnd(B * S, 3 * H, seed=4))
    drop = (0.1, 0x1234567)
    ctx, lse = torch.empty(B * S, H, device="cuda"), torch.empty(B, heads, S, device="cuda")
    ops.attn_fwd_f32(qkv, B, S, heads, 0.125, ctx, lse, dropout=drop)
    q16 = qkv.bfloat16()
    ctx16, lse16 = torch.empty(B * S, H, device="cuda", dtype=torch.bfloat16), torch.empty(B, heads, S, device="cuda")
    ops.attn_fwd(q16, B, S, heads, 0.125, ctx16, lse16, dropout=drop)
    assert rel_err(ctx16.float(), ctx) < 1.5e-2
    dctx = dev(rnd(B * S, H, seed=5))
    dqkv = torch.empty(B * S, 3 * H, device="cuda")
    ops.attn_bwd_f32(qkv, dctx, ctx, lse, B, S, heads, 0.125, dqkv, dropout=drop)
    dq16 = torch.empty(B * S, 3 * H, device="cuda", dtype=torch.bfloat16)
    ops.attn_bwd(q16, dctx.bfloat16(), lse16, B, S, heads, 0.125, dq16, dropout=drop)
    assert rel_err(dq16.float(), dqkv) < 3e-2
    u = dev(rnd(B * S, 3 * H, seed=6))
    cp, cm = torch.empty_like(ctx), torch.empty_like(ctx)

    def central(h):
        ops.attn_fwd_f32(qkv + h * u, B, S, heads, 0.125, cp, lse, dropout=drop)
        ops.attn_fwd_f32(qkv - h * u, B, S, heads, 0.125, cm, lse, dropout=drop)
        return (((cp - cm).double() * dctx.double()).sum() / (2 * h)).item()
    # the difference quotient divides the forward's rounding by 2 h: it is taken on the f32-operand forward (impl 2, same masks) --
    # the split-bf16 forward's 2^-16 per product (1e-5 of ctx) would show as 7e-3 of the quotient at h = 1e-2
    ops.exact_attn_set_impl(2)
    fd = (4 * central(1e-2) - central(2e-2)) / 3          # Richardson: the h^2 term of the central difference cancels
    ops.exact_attn_set_impl(0)
    an = (dqkv.double() * u.double()).sum().item()
    assert abs(fd - an) < 2e-3 * abs(an), (fd, an)


@pytest.mark.parametrize("H", [768, 512])
def test_exact_lora_grad_f32(ops, H):
    """bsclip_lora_grad_f32 against the f64 products (reference lora_layer.py:16-39: q += B_q (A_q y), v += B_v (A_v y)); adds to
    what the gradient buffers hold."""
    M = 1237
    dqkv, y = dev(rnd(M, 3 * H + 8, seed=1))[:, :3 * H], dev(rnd(M, H, seed=2))
    A, Bm = dev(rnd(8, H, seed=3, scale=0.05)), dev(rnd(2, H, 4, seed=4, scale=0.05))
    dA, dB = dev(rnd(8, H, seed=5)), dev(rnd(2, H, 4, seed=6))
    dA0, dB0 = dA.clone().double(), dB.clone().double()
    ops.lora_grad_f32(dqkv, y, M, H, A, Bm, dA, dB)
    yd, Ad, Bd = y.double(), A.double(), Bm.double()
    dq, dv = dqkv[:, :H].double(), dqkv[:, 2 * H:].double()
    t = yd @ Ad.t()                                              # [M, 8]
    ref_dA = torch.cat([(dq @ Bd[0]).t() @ yd, (dv @ Bd[1]).t() @ yd], 0)
    ref_dB = torch.stack([dq.t() @ t[:, :4], dv.t() @ t[:, 4:]], 0)
    assert rel_err(dA.double() - dA0, ref_dA) < 1e-5 and rel_err(dB.double() - dB0, ref_dB) < 1e-5
    again_A, again_B = dA0.float().clone(), dB0.float().clone()
    ops.lora_grad_f32(dqkv, y, M, H, A, Bm, again_A, again_B)
    assert torch.equal(again_A, dA) and torch.equal(again_B, dB)     # fixed summation order


def test_exact_split_operand_gemms(ops):
    """The split-operand GEMM family of the exact backward: dX = dY W through split3_transpose(W) (with the LoRA update folded),
    dW = dY^T X through split3_transpose of both operands (reduction over a ragged number of rows, zero-padded), and
    dgelu_split3, each against the f64 product at 3e-5 where the plain bf16 GEMM sits at 3e-3."""
    H, M = 256, 333
    w = dev(rnd(3 * H, H, seed=1, scale=H ** -0.5))
    A, Bm = dev(rnd(8, H, seed=2, scale=0.1)), dev(rnd(2, H, 4, seed=3, scale=0.1))
    weff = w.double().clone()
    weff[:H] += Bm[0].double() @ A[:4].double()
    weff[2 * H:] += Bm[1].double() @ A[4:].double()
    dy = dev(rnd(M, 3 * H, seed=4))
    wt = ops.split3_transpose(w, torch.empty(H * 9 * H, device="cuda", dtype=torch.bfloat16), 1, lora_a=A, lora_b=Bm)
    a3 = ops.split3_rows(dy, torch.empty(M, 9 * H, device="cuda", dtype=torch.bfloat16))
    dx = torch.empty(M, H, device="cuda")
    from bioscanclip.hip.ops import EPI_F32, EPI_RESID_F32
    ops.gemm(a3, wt, dx, EPI_F32)
    assert rel_err(dx.double(), dy.double() @ weff) < 3e-5
    x = dev(rnd(M, H, seed=5))
    Mp = (M + 63) // 64 * 64
    ta = ops.split3_transpose(dy, torch.empty(3 * H * 3 * Mp, device="cuda", dtype=torch.bfloat16), 0)
    tb = ops.split3_transpose(x, torch.empty(H * 3 * Mp, device="cuda", dtype=torch.bfloat16), 1)
    gw = dev(rnd(3 * H, H, seed=6))
    gw0 = gw.double().clone()
    ops.gemm(ta, tb, gw, EPI_RESID_F32, resid=gw)
    assert rel_err(gw.double() - gw0, dy.double().t() @ x.double()) < 3e-5
    z, g = dev(rnd(M, H, seed=7, scale=1.5)), dev(rnd(M, H, seed=8))
    o32 = torch.empty(M, H, device="cuda")
    d3 = ops.dgelu_split3(g, z, dst=torch.empty(M, 3 * H, device="cuda", dtype=torch.bfloat16), out32=o32)
    ref = g.double() * dgelu(z.double())
    assert rel_err(o32.double(), ref) < 1e-6
    assert rel_err(d3[:, :H].float().double() + d3[:, H:2 * H].float().double(), ref) < 2e-5 and torch.equal(d3[:, :H], d3[:, 2 * H:])


def test_exact_layernorm_bwd_f32_operands(ops):
    """bsclip_layernorm_bwd with the f32 GEMM gradient in and the f32 operand out (resid_flags bits 2 / 3): the same numbers as the
    bf16-operand call when the inputs are bf16-representable, and the operand carries the dropout mask of the bf16 one."""
    M, H = 300, 768
    x, gr = dev(rnd(M, H, seed=1)), dev(rnd(M, H, seed=2))
    gg16 = dev(rnd(M, H, seed=3)).bfloat16()
    gamma = dev(rnd(H, seed=4).abs() + 0.5)
    stats = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-6).rsqrt()], 1).contiguous()
    drop = (0.1, 77)
    for mode in (0, 1):
        d_ref, op_ref = torch.empty(M, H, device="cuda"), torch.empty(M, H, device="cuda", dtype=torch.bfloat16)
        ops.layernorm_bwd(x, stats, gamma, mode, g_resid=gr, g_gemm=gg16, dx_f32=d_ref, dx_bf16=op_ref, dropout=drop)
        d_new, op_new = torch.empty(M, H, device="cuda"), torch.empty(M, H, device="cuda")
        ops.layernorm_bwd(x, stats, gamma, mode, g_resid=gr, g_gemm=gg16.float(), dx_f32=d_new, dx_bf16=op_new, dropout=drop)
        assert torch.equal(d_new, d_ref) and torch.equal(op_new.bfloat16(), op_ref)
        kept = op_new != 0
        assert torch.allclose(op_new[kept], d_new[kept] / 0.9, rtol=1e-6) and 0.85 < kept.float().mean().item() < 0.95


@pytest.mark.parametrize("B,S,heads,masked,drop", [(3, 197, 12, False, None), (2, 133, 12, False, (0.1, 99)), (5, 20, 8, True, (0.1, 7)),
                                                   (2, 224, 2, True, None), (3, 1, 2, False, None),
                                                   # dropout at the block counts 2, 3, 4, 6, 7 (1 and 5 are above)
                                                   (2, 40, 2, False, (0.1, 5)), (1, 70, 2, True, (0.1, 6)), (2, 100, 2, False, (0.1, 8)),
                                                   (1, 170, 2, True, (0.1, 9)), (1, 200, 2, False, (0.1, 10))])
def test_exact_attention_two_implementations_agree(ops, B, S, heads, masked, drop):
    """The exact-mode attention exists three times -- split-bf16 operands on the bf16 matrix cores (impl 0, the default since round 5),
    f32 operands on the matrix pipe (impl 2: v_mfma_f32_32x32x2_f32, transposed tiles) and one-row-per-thread vector-ALU kernels
    (impl 1) -- with the same dropout masks: the two f32 forms agree to f32 rounding (different summation orders), the split form
    sits within 2^-16-per-product of them (5e-5 / 2e-4), dropout included (a mask mismatch would be an O(0.3) difference)."""
    H = heads * 64
    qkv, dctx = dev(rnd(B * S, 3 * H, seed=1)), dev(rnd(B * S, H, seed=2))
    bias = None
    if masked:
        lens = torch.randint(1, S + 1, (B,), generator=torch.Generator().manual_seed(3))
        bias = dev((1.0 - (torch.arange(S)[None] < lens[:, None]).float()) * torch.finfo(torch.float32).min)
    out = {}
    try:
        for impl in (0, 1, 2):
            ops.exact_attn_set_impl(impl)
            ctx, lse = torch.empty(B * S, H, device="cuda"), torch.empty(B, heads, S, device="cuda")
            dqkv = torch.full((B * S, 3 * H), float("nan"), device="cuda")
            ops.attn_fwd_f32(qkv, B, S, heads, 0.125, ctx, lse, key_bias=bias, dropout=drop)
            ops.attn_bwd_f32(qkv, dctx, ctx, lse, B, S, heads, 0.125, dqkv, key_bias=bias, dropout=drop)
            out[impl] = (ctx, lse, dqkv)
    finally:
        ops.exact_attn_set_impl(0)
    assert rel_err(out[2][0], out[1][0]) < 2e-6 and rel_err(out[2][1], out[1][1]) < 1e-6
    assert rel_err(out[0][0], out[2][0]) < 5e-5 and rel_err(out[0][1], out[2][1]) < 1e-5, (rel_err(out[0][0], out[2][0]), rel_err(out[0][1], out[2][1]))
    g0, g1, gx = out[2][2], out[1][2], out[0][2]
    for sl in (slice(0, H), slice(H, 2 * H), slice(2 * H, 3 * H)):
        assert ((gx[:, sl] - g0[:, sl]).norm() / torch.maximum(g0[:, sl].norm(), 1e-2 * g0.norm())).item() < (1e-3 if S == 1 else 2e-4)
    for sl in (slice(0, H), slice(H, 2 * H), slice(2 * H, 3 * H)):
        # S = 1: dq = dk = 0 analytically, what is left is dS = P (dP - delta) rounding noise against 1e-2 of the gradient's norm
        assert ((g0[:, sl] - g1[:, sl]).norm() / torch.maximum(g1[:, sl].norm(), 1e-2 * g1.norm())).item() < (3e-5 if S == 1 else 3e-6)
