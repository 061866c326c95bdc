"""Tensor-level wrappers over the C ABI (one function per ``bsclip_*`` entry point).

torch is plumbing here (device memory + the current HIP stream); every function validates shapes, dtypes and
contiguity on the host before handing raw pointers to the library, because an out-of-bounds access in a
hand-written kernel can take the whole GPU down.  Nothing in this module computes with torch ops.
"""
import ctypes

import numpy as np
import torch

from . import lib as _l
from .lib import (EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_GELU_FP8, EPI_PATCH_BF16, EPI_PATCH_F32,  # noqa: F401
                  EPI_RESID_BF16, EPI_RESID_F32, KPAD, OPERANDS_FP16,
                  EpiArgs, Fp8Args, check)

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def _rowmajor(t, name):
    # messages are only formatted on failure: these checks run ~1 500 times per training step
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a GPU tensor")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a 2-D tensor with unit inner stride")
    return t.stride(0)


def _f32_shaped(t, shape, name):
    # as above: nothing is formatted unless the check fails
    if t is None or t.dtype != F32 or not t.is_contiguous() or t.shape != shape:
        raise ValueError(f"{name} must be contiguous f32 {list(shape)}")


def _i32(t, dev, msg, shape=None, dims=None):
    # a contiguous int32 tensor on the GPU ``dev``, of ``shape`` or of one of ``dims`` dimensions; ``msg`` names the wrapper
    if (t is None or t.dtype != torch.int32 or not t.is_contiguous() or not t.is_cuda or t.device != dev
            or (shape is not None and tuple(t.shape) != tuple(shape)) or (dims is not None and t.dim() not in dims)):
        raise ValueError(msg)


def _lora_grads_ok(M, H, dt, dA, dBq, dBv):
    _req(dt.dtype == F32 and dt.is_contiguous() and dt.numel() >= 8 * M, "dt f32 [M,8]")
    _f32_shaped(dA, (8, H), "dA")
    _f32_shaped(dBq, (H, 4), "dBq")
    _f32_shaped(dBv, (H, 4), "dBv")


def _key_bias_ok(key_bias, B, S):
    if key_bias is not None and not (key_bias.dtype == F32 and key_bias.is_contiguous() and key_bias.numel() >= B * S):
        raise ValueError("key_bias f32 [B,S]")


def _drop(dropout):   # a dropout site's (p, seed), or None for none, as the kernels take it
    return (0.0, 0) if dropout is None else (float(dropout[0]), int(dropout[1]) & 0xFFFFFFFF)


_STREAM_WS = {}


def _stream_ws(tag, device, floats):
    """f32 scratch of >= ``floats`` elements for kernel family ``tag``: one per device and launching stream (the towers run concurrently)."""
    key = (tag, str(device), torch.cuda.current_stream().cuda_stream)
    ws = _STREAM_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = _STREAM_WS[key] = torch.empty(floats, dtype=F32, device=device)
    return ws


def gemm(a, b, out, epilogue=EPI_BF16, bias=None, resid=None, aux=None, M=None, K=None, dropout=None):
    """out = epilogue(a[:M, :K] @ b[:, :K].T).  a [M, >=K], b [N, >=K] (row strides may exceed K), both bf16 or both fp16; with
    fp16 operands every 16-bit output / residual of the epilogue is fp16 too (BSCLIP_OPERANDS_FP16)."""
    lda, ldb, ldc = _rowmajor(a, "a"), _rowmajor(b, "b"), _rowmajor(out, "out")
    _req(a.dtype == b.dtype and a.dtype in (BF16, F16), "gemm operands must be both bf16 or both fp16")
    h16 = a.dtype
    M = a.shape[0] if M is None else M
    K = min(a.shape[1], b.shape[1]) if K is None else K
    N = b.shape[0]
    _req(M <= a.shape[0] and K <= a.shape[1] and K <= b.shape[1], "gemm: M/K exceed operand shapes")
    want = F32 if epilogue in (EPI_F32, EPI_RESID_F32, EPI_PATCH_F32) else h16
    if out.dtype != want:
        raise ValueError(f"gemm: out dtype {out.dtype} != {want}")
    if epilogue in (EPI_PATCH_F32, EPI_PATCH_BF16):
        _req(M % 196 == 0 and out.shape[0] >= M // 196 * 197 and out.shape[1] >= N, "gemm(PATCH): out too small")
    else:
        _req(out.shape[0] >= M and out.shape[1] >= N, "gemm: out too small")
    args = EpiArgs()
    if bias is not None:
        _req(bias.dtype == F32 and bias.numel() >= N and bias.is_contiguous(), "gemm: bias must be f32 [N]")
        args.bias = bias.data_ptr()
    if resid is not None:
        _req(resid.dtype == (h16 if epilogue == EPI_RESID_BF16 else F32),
             "gemm: resid must be f32 (for EPI_RESID_BF16 the operands' 16-bit type)")
        need = 197 if epilogue in (EPI_PATCH_F32, EPI_PATCH_BF16) else M
        _req(resid.shape[0] >= need and resid.shape[1] >= N, "gemm: resid too small")
        args.resid = resid.data_ptr()
        args.ld_resid = _rowmajor(resid, "resid")
    if aux is not None:  # gelu' side band: 8-bit codes (include/bsclip.h)
        _req(aux.dtype == torch.uint8 and aux.shape[0] >= M and aux.shape[1] >= N, "gemm: aux must be uint8 [M, N]")
        args.aux = aux.data_ptr()
        args.ld_aux = _rowmajor(aux, "aux")
    if dropout is not None:  # (p, seed): C = dropout(acc + bias) + resid
        _req(epilogue in (EPI_RESID_F32, EPI_RESID_BF16), "gemm: dropout is only defined for EPI_RESID_F32 / _BF16")
        args.dropout_p, args.dropout_seed = _drop(dropout)
    fmt = OPERANDS_FP16 if h16 == F16 else 0
    check(_l.load().bsclip_gemm_bf16(_p(a), lda, _p(b), ldb, _p(out), ldc, M, N, K, epilogue | fmt, ctypes.byref(args),
                                     _stream()))
    return out


FP8 = torch.float8_e4m3fn   # OCP e4m3 (gfx950); one byte per element
FP8_FORM = int(__import__("os").environ.get("BSCLIP_FP8_FORM", "1"))   # 1: 16x16x32 fp8 MFMA (faster here), 2: block-scaled 16x16x128


def gemm_fp8(a8, b8, out, alpha, bias, epilogue=EPI_BF16, resid=None, aux=None, a_aug=None, b_aug=None, M=None, K=None,
             dropout=None, form=None):
    """out = epilogue(alpha[n] * (a8[:M, :K] @ b8[:, :K].T + a_aug @ b_aug.T) + bias).  a8 [M, >=K], b8 [N, >=K] fp8 e4m3;
    a_aug [M, >=64] / b_aug [N, >=64] bf16 (the LoRA K-augmentation block) or both None."""
    lda, ldb, ldc = _rowmajor(a8, "a8"), _rowmajor(b8, "b8"), _rowmajor(out, "out")
    _req(a8.dtype == FP8 and b8.dtype == FP8, "gemm_fp8 operands must be float8_e4m3fn")
    M = a8.shape[0] if M is None else M
    K = min(a8.shape[1], b8.shape[1]) if K is None else K
    N = b8.shape[0]
    _req(M <= a8.shape[0] and K <= a8.shape[1] and K <= b8.shape[1], "gemm_fp8: M/K exceed operand shapes")
    want = {EPI_BF16: BF16, EPI_F32: F32, EPI_RESID_F32: F32, EPI_GELU_FP8: FP8}.get(epilogue)
    _req(want is not None and out.dtype == want, f"gemm_fp8: epilogue {epilogue} needs out dtype {want}")
    _req(out.shape[0] >= M and out.shape[1] >= N, "gemm_fp8: out too small")
    _req(alpha.dtype == F32 and alpha.numel() >= N and alpha.is_contiguous(), "gemm_fp8: alpha must be f32 [N]")
    _req(bias.dtype == F32 and bias.numel() >= N and bias.is_contiguous(), "gemm_fp8: bias must be f32 [N]")
    args = EpiArgs()
    args.bias = bias.data_ptr()
    if resid is not None:
        _req(resid.dtype == F32 and resid.shape[0] >= M and resid.shape[1] >= N, "gemm_fp8: resid must be f32 [M, N]")
        args.resid, args.ld_resid = resid.data_ptr(), _rowmajor(resid, "resid")
    if aux is not None:
        _req(aux.dtype == torch.uint8 and aux.shape[0] >= M and aux.shape[1] >= N, "gemm_fp8: aux must be uint8 [M, N]")
        args.aux, args.ld_aux = aux.data_ptr(), _rowmajor(aux, "aux")
    if dropout is not None:
        _req(epilogue == EPI_RESID_F32, "gemm_fp8: dropout is only defined for EPI_RESID_F32")
        args.dropout_p, args.dropout_seed = _drop(dropout)
    f8 = Fp8Args()
    f8.form = FP8_FORM if form is None else form
    f8.alpha = alpha.data_ptr()
    _req((a_aug is None) == (b_aug is None), "gemm_fp8: a_aug and b_aug go together")
    if a_aug is not None:
        _req(a_aug.dtype == BF16 and b_aug.dtype == BF16 and a_aug.shape[0] >= M and b_aug.shape[0] >= N
             and a_aug.shape[1] >= 64 and b_aug.shape[1] >= 64, "gemm_fp8: aug blocks must be bf16 [M,>=64] / [N,>=64]")
        f8.a_aug, f8.ld_a_aug = a_aug.data_ptr(), _rowmajor(a_aug, "a_aug")
        f8.b_aug, f8.ld_b_aug = b_aug.data_ptr(), _rowmajor(b_aug, "b_aug")
    check(_l.load().bsclip_gemm_fp8(_p(a8), lda, _p(b8), ldb, _p(out), ldc, M, N, K, epilogue, ctypes.byref(args),
                                    ctypes.byref(f8), _stream()))
    return out


def quantize_rows_fp8(w):
    """f32 [R, C] -> (fp8 e4m3 [R, C], f32 scale [R]) with w ~= q * scale[:, None] (row amax mapped to 448)."""
    _req(w.dtype == F32 and w.is_contiguous() and w.dim() == 2 and w.is_cuda and w.shape[1] % 4 == 0, "quantize_rows_fp8: f32 [R, C]")
    q = torch.empty(w.shape, dtype=FP8, device=w.device)
    sc = torch.empty(w.shape[0], dtype=F32, device=w.device)
    check(_l.load().bsclip_quantize_rows_fp8(_p(w), w.shape[0], w.shape[1], _p(q), w.shape[1], _p(sc), _stream()))
    return q, sc


def lora_baug_set(b_aug, H, bq, bv, alpha):
    _req(b_aug.dtype == BF16 and b_aug.shape[0] >= 3 * H and b_aug.shape[1] >= 64, "b_aug bf16 [3H, >=64]")
    _f32_shaped(bq, (H, 4), "bq")
    _f32_shaped(bv, (H, 4), "bv")
    _req(alpha.dtype == F32 and alpha.is_contiguous() and alpha.numel() >= 3 * H, "alpha f32 [3H]")
    check(_l.load().bsclip_lora_baug_set(_p(b_aug), _rowmajor(b_aug, "b_aug"), H, _p(bq), _p(bv), _p(alpha), _stream()))


_tables_ready = False


def init_tables():
    """One-time device tables, synchronised, so GEMMs launched from several streams all see them."""
    global _tables_ready
    if not _tables_ready:
        check(_l.load().bsclip_init_tables(_stream()))
        torch.cuda.synchronize()
        _tables_ready = True


def set_gemm_tile(tile):
    check(_l.load().bsclip_gemm_set_tile(tile))


def set_gemm_persistent_grid(workgroups):
    """Workgroups of the persistent GEMM kernel's launch (tile 8); 0 = one per CU."""
    check(_l.load().bsclip_gemm_set_persistent_grid(workgroups))


def _h16(*ts, who):
    """The 16-bit operand format shared by the 16-bit tensors among ``ts`` (None entries skipped): bf16 or fp16, never mixed."""
    kinds = {t.dtype for t in ts if t is not None and t.dtype in (BF16, F16)}
    _req(len(kinds) <= 1, f"{who}: 16-bit tensors must all be bf16 or all fp16, got {sorted(str(k) for k in kinds)}")
    return kinds.pop() if kinds else BF16


def layernorm_fwd(x, gamma, beta, eps, y_bf16=None, y_f32=None, lora_a=None, stats=None, M=None, dropout=None, y_split3=None):
    """``y_split3`` (exact mode): bf16 [M, >= 3H] that receives the output as a split-bf16 GEMM operand [hi | lo | hi].
    fp16 operands (BSCLIP_OPERANDS_FP16): a 16-bit x and y_bf16 are fp16; no y_split3, no dropout."""
    ld_x = _rowmajor(x, "x")
    H = gamma.numel()
    M = x.shape[0] if M is None else M
    _req(x.dtype in (F32, BF16, F16) and x.shape[1] >= H and M <= x.shape[0], "layernorm_fwd: bad x")
    h16 = _h16(x, y_bf16, who="layernorm_fwd")
    _req(gamma.dtype == F32 and beta.dtype == F32 and beta.numel() == H, "layernorm_fwd: gamma/beta f32 [H]")
    ld_y = 0
    if y_bf16 is not None:
        ld_y = _rowmajor(y_bf16, "y_bf16")
        _req(y_bf16.dtype == h16 and y_bf16.shape[0] >= M and y_bf16.shape[1] >= H + (KPAD if lora_a is not None else 0),
             "layernorm_fwd: y_bf16 too small")
    if y_f32 is not None:
        _req(y_f32.dtype == F32 and y_f32.is_contiguous() and y_f32.shape[0] >= M and y_f32.shape[1] == H,
             "layernorm_fwd: y_f32 must be contiguous f32 [M, H]")
    if lora_a is not None:
        _f32_shaped(lora_a, (8, H), "lora_a")
    if stats is not None:
        _req(stats.dtype == F32 and stats.is_contiguous() and stats.numel() >= 2 * M, "stats must be f32 [M,2]")
    ld_y3 = 0
    if y_split3 is not None:
        ld_y3 = _rowmajor(y_split3, "y_split3")
        _req(y_split3.dtype == BF16 and y_split3.shape[0] >= M and y_split3.shape[1] >= 3 * H, "layernorm_fwd: y_split3 bf16 [M, >= 3H]")
    dp, ds = _drop(dropout)
    fmt = OPERANDS_FP16 if h16 == F16 else 0
    check(_l.load().bsclip_layernorm_fwd(_p(x), ld_x, int(x.dtype != F32) | fmt, M, H, _p(gamma), _p(beta), float(eps),
                                         _p(y_bf16), ld_y, _p(y_f32), _p(y_split3), ld_y3, _p(lora_a), _p(stats), dp, ds, _stream()))


def layernorm_fwd_fp8(x, gamma, beta, eps, y_fp8, t_aug=None, y_f32=None, lora_a=None, stats=None, M=None, dropout=None):
    """LayerNorm whose GEMM operand comes out as fp8 e4m3 (y_fp8 [M, >=H]) with the LoRA t block in its own bf16 buffer."""
    ld_x = _rowmajor(x, "x")
    H = gamma.numel()
    M = x.shape[0] if M is None else M
    _req(x.dtype in (F32, BF16) and x.shape[1] >= H and M <= x.shape[0], "layernorm_fwd_fp8: bad x")
    _req(gamma.dtype == F32 and beta.dtype == F32 and beta.numel() == H, "layernorm_fwd_fp8: gamma/beta f32 [H]")
    _req(y_fp8.dtype == FP8 and y_fp8.shape[0] >= M and y_fp8.shape[1] >= H, "layernorm_fwd_fp8: y_fp8 [M, >=H]")
    _req((lora_a is None) == (t_aug is None), "layernorm_fwd_fp8: lora_a and t_aug go together")
    ld_t = 0
    if t_aug is not None:
        ld_t = _rowmajor(t_aug, "t_aug")
        _req(t_aug.dtype == BF16 and t_aug.shape[0] >= M and t_aug.shape[1] >= KPAD, "t_aug bf16 [M, >=64]")
        _f32_shaped(lora_a, (8, H), "lora_a")
    if y_f32 is not None:
        _req(y_f32.dtype == F32 and y_f32.is_contiguous() and y_f32.shape[0] >= M and y_f32.shape[1] == H, "y_f32 f32 [M,H]")
    if stats is not None:
        _req(stats.dtype == F32 and stats.is_contiguous() and stats.numel() >= 2 * M, "stats must be f32 [M,2]")
    dp, ds = _drop(dropout)
    check(_l.load().bsclip_layernorm_fwd_fp8(_p(x), ld_x, int(x.dtype == BF16), M, H, _p(gamma), _p(beta), float(eps),
                                             _p(y_fp8), _rowmajor(y_fp8, "y_fp8"), _p(t_aug), ld_t, _p(y_f32), _p(lora_a),
                                             _p(stats), dp, ds, _stream()))


def layernorm_bwd(x, stats, gamma, mode, g_resid=None, g_gemm=None, dt=None, lora_a=None, dx_f32=None, dx_bf16=None,
                  M=None, dropout=None, in_dropout=None, dx_split3=None):
    """``g_resid`` / ``dx_f32`` are the residual-gradient stream in / out: f32, or bf16 (half the bytes; the dtype of each
    tensor is passed on as ``resid_flags``).  ``dx_bf16`` is the next dX GEMM's operand (carries ``dropout``'s mask); the exact
    backward passes ``g_gemm`` and ``dx_bf16`` as f32 tensors, or takes the operand as ``dx_split3``: bf16 [M, >= 3H] = [hi | lo | hi],
    the A operand of the next split-bf16 dX GEMM (instead of ``dx_bf16``).
    fp16 operands (BSCLIP_OPERANDS_FP16, the LoRA ViT's backward): x fp16, and every 16-bit tensor passed (g_resid, g_gemm, dx_f32,
    dx_bf16) fp16 as well; no dropout, no f32 / split operand forms."""
    ld_x = _rowmajor(x, "x")
    H = gamma.numel()
    M = x.shape[0] if M is None else M
    _req(x.dtype in (F32, BF16, F16) and x.shape[1] >= H and M <= x.shape[0], "layernorm_bwd: bad x")
    f16 = x.dtype == F16
    if f16:
        _req(dropout is None and in_dropout is None and dx_split3 is None
             and all(t is None or t.dtype == F16 for t in (g_resid, g_gemm, dx_f32, dx_bf16)),
             "layernorm_bwd: fp16 operands take fp16 g_resid / g_gemm / dx_f32 / dx_bf16, no dropout, no split output")
    else:
        _req(all(t is None or t.dtype != F16 for t in (g_resid, g_gemm, dx_f32, dx_bf16)), "layernorm_bwd: fp16 tensors need an fp16 x")
    b16 = (BF16, F16)
    _req(stats.dtype == F32 and stats.numel() >= 2 * M, "layernorm_bwd: stats")
    ld_g = ld_dxb = ld_gr = ld_dx = 0
    if g_resid is not None:
        ld_gr = _rowmajor(g_resid, "g_resid")
        _req(g_resid.dtype in (F32, BF16, F16) and g_resid.shape[0] >= M and g_resid.shape[1] >= H, "g_resid must be f32 / bf16 [M,>=H]")
    if g_gemm is not None:
        ld_g = _rowmajor(g_gemm, "g_gemm")
        _req(g_gemm.dtype in (BF16, F32, F16) and g_gemm.shape[0] >= M and g_gemm.shape[1] >= H, "g_gemm must be bf16 / f32 [M,>=H]")
    if dt is not None:
        _req(dt.dtype == F32 and dt.is_contiguous() and dt.numel() >= 8 * M, "dt must be f32 [M,8]")
        _f32_shaped(lora_a, (8, H), "lora_a")
    if dx_f32 is not None:
        ld_dx = _rowmajor(dx_f32, "dx_f32")
        _req(dx_f32.dtype in (F32, BF16, F16) and dx_f32.shape[0] >= M and dx_f32.shape[1] >= H, "dx_f32 must be f32 / bf16 [M,>=H]")
    if dx_split3 is not None:
        _req(dx_bf16 is None and dx_split3.dtype == BF16 and dx_split3.shape[0] >= M and dx_split3.shape[1] >= 3 * H,
             "dx_split3: bf16 [M, >= 3H], instead of dx_bf16")
        dx_bf16 = dx_split3
    if dx_bf16 is not None:
        ld_dxb = _rowmajor(dx_bf16, "dx_bf16")
        _req(dx_bf16.dtype in (BF16, F32, F16) and dx_bf16.shape[0] >= M and dx_bf16.shape[1] >= H, "dx_bf16 (bf16 / f32 operand) too small")
    check(_l.load().bsclip_layernorm_bwd(_p(x), ld_x, (1 | OPERANDS_FP16) if f16 else int(x.dtype == BF16), _p(stats), _p(gamma), M, H, _p(g_resid),
                                         ld_gr, _p(g_gemm), ld_g, _p(dt), _p(lora_a) if dt is not None else None,
                                         int(mode), _p(dx_f32), ld_dx, _p(dx_bf16), ld_dxb,
                                         *_drop(dropout), *_drop(in_dropout),
                                         (1 if g_resid is not None and g_resid.dtype in b16 else 0)
                                         | (2 if dx_f32 is not None and dx_f32.dtype in b16 else 0)
                                         | (4 if g_gemm is not None and g_gemm.dtype == F32 else 0)
                                         | (8 if dx_bf16 is not None and dx_bf16.dtype == F32 else 0)
                                         | (16 if dx_split3 is not None else 0), _stream()))


KEEP_WORDS = 16   # csrc/attn_common.h: 32-bit dropout keep words per (batch, head, query) row (2 lane halves x 8)


def _keep_bits_ok(keep_bits, B, S, heads, who):
    if keep_bits is not None:
        _req(keep_bits.dtype == torch.int32 and keep_bits.is_contiguous() and keep_bits.is_cuda
             and keep_bits.numel() >= B * heads * S * KEEP_WORDS, f"{who}: keep_bits int32 [B * heads, S, 2, {KEEP_WORDS // 2}]")


def attn_fwd(qkv, B, S, heads, scale, ctx, lse, key_bias=None, dropout=None, q_rows=0, keep_bits=None):
    """``keep_bits`` (int32 [B * heads, S, 2, 8], with dropout only): the forward leaves its keep decisions there for ``attn_bwd``.
    qkv and ctx both bf16, or both fp16 (BSCLIP_OPERANDS_FP16: inference only, no dropout / keep_bits)."""
    ld_qkv, ld_ctx = _rowmajor(qkv, "qkv"), _rowmajor(ctx, "ctx")
    _keep_bits_ok(keep_bits, B, S, heads, "attn_fwd")
    h16 = _h16(qkv, ctx, who="attn_fwd")
    _req(qkv.dtype == h16 and ctx.dtype == h16 and lse.dtype == F32, "attn_fwd dtypes")
    _req(qkv.shape[0] >= B * S and qkv.shape[1] >= 3 * heads * 64, "attn_fwd: qkv too small")
    _req(ctx.shape[0] >= B * S and ctx.shape[1] >= heads * 64 and lse.numel() >= B * heads * S, "attn_fwd: outputs too small")
    _key_bias_ok(key_bias, B, S)
    dp, ds = _drop(dropout)
    fmt = OPERANDS_FP16 if h16 == F16 else 0
    check(_l.load().bsclip_attn_fwd(_p(qkv), ld_qkv, B, S, heads, _p(key_bias), float(scale), _p(ctx), ld_ctx, _p(lse),
                                    int(q_rows) | fmt, _p(keep_bits), dp, ds, _stream()))


def attn_bwd(qkv, dctx, lse, B, S, heads, scale, dqkv, key_bias=None, dropout=None, q_rows=0, keep_bits=None, lora=None):
    """``keep_bits``: the words the forward of the SAME (seed, step) left; None = re-hash the decisions (same masks, slower).
    ``lora`` = (t_aug, lora_b, dt_partial, db_partial): also leave the LoRA gradients' partial sums (``lora_grad_heads`` reduces them):
    t_aug bf16 [>= B S, >= 8] with t in columns 0..7 (a view of the LayerNorm output's t block), lora_b f32 [2, H, 4], dt_partial f32
    [heads, 2, B S, 4], db_partial f32 [B heads, 2, 4, 64].
    fp16 operands (BSCLIP_OPERANDS_FP16, the LoRA ViT's backward): qkv, dctx, dqkv (and t_aug) fp16; S = 197, no dropout / keep_bits."""
    ld_qkv, ld_ctx, ld_d = _rowmajor(qkv, "qkv"), _rowmajor(dctx, "dctx"), _rowmajor(dqkv, "dqkv")
    _keep_bits_ok(keep_bits, B, S, heads, "attn_bwd")
    h16 = qkv.dtype
    _req(h16 in (BF16, F16) and all(t.dtype == h16 for t in (qkv, dctx, dqkv)) and lse.dtype == F32, "attn_bwd dtypes")
    fmt = OPERANDS_FP16 if h16 == F16 else 0
    _req(not fmt or (dropout is None and keep_bits is None), "attn_bwd: fp16 operands take no dropout / keep_bits")
    _req(min(qkv.shape[0], dctx.shape[0], dqkv.shape[0]) >= B * S, "attn_bwd: rows")
    _req(qkv.shape[1] >= 3 * heads * 64 and dqkv.shape[1] >= 3 * heads * 64 and dctx.shape[1] >= heads * 64
         and lse.numel() >= B * heads * S, "attn_bwd: cols")
    _key_bias_ok(key_bias, B, S)
    dp, ds = _drop(dropout)
    if lora is not None:
        t_aug, lora_b, dtp, dbp = lora
        ld_t = _rowmajor(t_aug, "t_aug")
        _req(t_aug.dtype == h16 and t_aug.shape[0] >= B * S and t_aug.shape[1] >= 8, "attn_bwd: t_aug 16-bit [>= B S, >= 8] (qkv's format)")
        _f32_shaped(lora_b, (2, heads * 64, 4), "attn_bwd: lora_b")
        _req(dtp.dtype == F32 and dtp.is_contiguous() and dtp.numel() >= heads * B * S * 8
             and dbp.dtype == F32 and dbp.is_contiguous() and dbp.numel() >= B * heads * 512, "attn_bwd: dt_partial / db_partial sizes")
        _req(dp == 0.0 or keep_bits is not None, "attn_bwd: the LoRA partials under dropout need the forward's keep_bits")
        check(_l.load().bsclip_attn_bwd_lora(_p(qkv), ld_qkv, _p(dctx), ld_ctx, _p(lse), B, S, heads, _p(key_bias), float(scale), _p(dqkv),
                                             ld_d, int(q_rows) | fmt, _p(keep_bits), _p(t_aug), ld_t, _p(lora_b), _p(dtp), _p(dbp), dp, ds,
                                             _stream()))
        return
    check(_l.load().bsclip_attn_bwd(_p(qkv), ld_qkv, _p(dctx), ld_ctx, _p(lse), B, S, heads, _p(key_bias),
                                    float(scale), _p(dqkv), ld_d, int(q_rows) | fmt, _p(keep_bits), dp, ds, _stream()))


def split3_rows(src, dst, M=None, K=None):
    """f32 [M, K] -> bf16 [M, 3K] = [hi | lo | hi]: the A operand of a split-bf16 GEMM."""
    M = src.shape[0] if M is None else M
    K = src.shape[1] if K is None else K
    _req(src.dtype == F32 and dst.dtype == BF16 and src.shape[0] >= M and src.shape[1] >= K and K % 4 == 0, "split3_rows: f32 [M, K]")
    _req(dst.shape[0] >= M and dst.shape[1] >= 3 * K, "split3_rows: dst bf16 [M, 3K]")
    check(_l.load().bsclip_split3_rows(_p(src), _rowmajor(src, "src"), M, K, _p(dst), _rowmajor(dst, "dst"), _stream()))
    return dst[:M, :3 * K]


def split3_weight(w, dst, lora_a=None, lora_b=None):
    """f32 [N, K] (+ LoRA: W + B A on the q / v rows) -> bf16 [N, 3K] = [hi | hi | lo]: the B operand of a split-bf16 GEMM."""
    N, K = w.shape
    _req(w.dtype == F32 and w.is_contiguous() and dst.dtype == BF16 and dst.is_contiguous() and tuple(dst.shape) == (N, 3 * K),
         "split3_weight: w f32 [N, K] -> dst bf16 [N, 3K]")
    H = 0
    if lora_a is not None:
        H = K
        _req(N == 3 * K, "split3_weight: the LoRA fold needs w [3H, H]")
        _f32_shaped(lora_a, (8, K), "lora_a")
        _f32_shaped(lora_b, (2, K, 4), "lora_b")
    check(_l.load().bsclip_split3_weight(_p(w), K, N, K, _p(lora_a), _p(lora_b if lora_a is not None else None), H, _p(dst), 3 * K,
                                         _stream()))
    return dst


def gelu_split3(z, dst=None, codes=None, g32=None, M=None):
    """f32 pre-activation [M, N] -> exact GELU as bf16 [M, 3N] = [hi | lo | hi] (dst) and / or f32 [M, N] (g32), + the 8-bit gelu'
    codes the backward reads."""
    M = z.shape[0] if M is None else M
    N = z.shape[1]
    _req(z.dtype == F32 and N % 4 == 0 and (dst is not None or g32 is not None), "gelu_split3: z f32 [M, N], an output")
    if dst is not None:
        _req(dst.dtype == BF16 and dst.shape[0] >= M and dst.shape[1] >= 3 * N, "gelu_split3: dst bf16 [M, 3N]")
    if g32 is not None:
        _req(g32.dtype == F32 and g32.shape[0] >= M and g32.shape[1] >= N, "gelu_split3: g32 f32 [M, N]")
    if codes is not None:
        _req(codes.dtype == torch.uint8 and codes.shape[0] >= M and codes.shape[1] >= N, "gelu_split3: codes u8 [M, N]")
    check(_l.load().bsclip_gelu_split3(_p(z), _rowmajor(z, "z"), M, N, _p(dst), 0 if dst is None else _rowmajor(dst, "dst"), _p(codes),
                                       0 if codes is None else _rowmajor(codes, "codes"), _p(g32),
                                       0 if g32 is None else _rowmajor(g32, "g32"), _stream()))
    return None if dst is None else dst[:M, :3 * N]


def meanpool_tokens_f32(x, B, S, out):
    H = x.shape[1]
    _req(x.dtype == F32 and x.is_contiguous() and x.shape[0] >= B * S and out.dtype == F32 and out.is_contiguous()
         and out.shape[0] >= B and out.shape[1] == H, "meanpool_tokens_f32: x f32 [B*S,H], out f32 [B,H]")
    check(_l.load().bsclip_meanpool_tokens_f32(_p(x), B, S, H, _p(out), _stream()))


def attn_fwd_f32(qkv, B, S, heads, scale, ctx, lse, key_bias=None, dropout=None, ctx_split3=None):
    """``ctx_split3``: bf16 [>= B S, >= 3 heads 64] that receives ctx as the out-projection GEMM's split operand [hi | lo | hi]."""
    ld_qkv, ld_ctx = _rowmajor(qkv, "qkv"), _rowmajor(ctx, "ctx")
    ld_c3 = 0
    if ctx_split3 is not None:
        ld_c3 = _rowmajor(ctx_split3, "ctx_split3")
        _req(ctx_split3.dtype == BF16 and ctx_split3.shape[0] >= B * S and ctx_split3.shape[1] >= 3 * heads * 64, "attn_fwd_f32: ctx_split3")
    _req(qkv.dtype == F32 and ctx.dtype == F32 and lse.dtype == F32, "attn_fwd_f32 dtypes")
    _req(qkv.shape[0] >= B * S and qkv.shape[1] >= 3 * heads * 64 and ctx.shape[0] >= B * S and ctx.shape[1] >= heads * 64
         and lse.numel() >= B * heads * S, "attn_fwd_f32 shapes")
    _key_bias_ok(key_bias, B, S)
    dp, ds = _drop(dropout)
    check(_l.load().bsclip_attn_fwd_f32(_p(qkv), ld_qkv, B, S, heads, _p(key_bias), float(scale), _p(ctx), ld_ctx, _p(lse),
                                        _p(ctx_split3), ld_c3, dp, ds, _stream()))


# ---- exact backward (BSCLIP_PARITY=2): f32 gradients, split operands on the dX / dW GEMMs (csrc/exact.hip) ----
def dgelu_split3(dact, z, dst=None, out32=None, M=None):
    """dact * gelu'(z), both f32 [M, N] -> bf16 [M, 3N] = [hi | lo | hi] (dst) and / or f32 (out32; may alias dact)."""
    M = z.shape[0] if M is None else M
    N = z.shape[1]
    _req(z.dtype == F32 and dact.dtype == F32 and dact.shape[0] >= M and dact.shape[1] >= N and N % 4 == 0
         and (dst is not None or out32 is not None), "dgelu_split3: dact, z f32 [M, N], an output")
    if dst is not None:
        _req(dst.dtype == BF16 and dst.shape[0] >= M and dst.shape[1] >= 3 * N, "dgelu_split3: dst bf16 [M, 3N]")
    if out32 is not None:
        _req(out32.dtype == F32 and out32.shape[0] >= M and out32.shape[1] >= N, "dgelu_split3: out32 f32 [M, N]")
    check(_l.load().bsclip_dgelu_split3(_p(dact), _rowmajor(dact, "dact"), _p(z), _rowmajor(z, "z"), M, N, _p(dst),
                                        0 if dst is None else _rowmajor(dst, "dst"), _p(out32),
                                        0 if out32 is None else _rowmajor(out32, "out32"), _stream()))
    return None if dst is None else dst[:M, :3 * N]


def split3_transpose(src, dst_flat, order, R=None, lora_a=None, lora_b=None):
    """src f32 [R, C] -> bf16 [C, 3 Rp] (Rp = R rounded up to 64; carved out of the flat bf16 buffer ``dst_flat``): row c is the
    split of column c, order 0 = [hi | lo | hi], 1 = [hi | hi | lo]; lora_a / lora_b fold W + B A first (src = the [3H, H] QKV weight)."""
    R = src.shape[0] if R is None else R
    C = src.shape[1]
    Rp = (R + 63) // 64 * 64
    _req(src.dtype == F32 and src.shape[0] >= R and dst_flat.dtype == BF16 and dst_flat.is_contiguous()
         and dst_flat.numel() >= C * 3 * Rp, "split3_transpose: src f32 [R, C], dst bf16 >= C * 3 * Rp")
    H = 0
    if lora_a is not None:
        H = C
        _req(src.is_contiguous() and R == 3 * C, "split3_transpose: the LoRA fold needs src [3H, H]")
        _f32_shaped(lora_a, (8, C), "lora_a")
        _f32_shaped(lora_b, (2, C, 4), "lora_b")
    dst = dst_flat.view(-1)[:C * 3 * Rp].view(C, 3 * Rp)
    check(_l.load().bsclip_split3_transpose(_p(src), _rowmajor(src, "src"), R, C, Rp, int(order), _p(lora_a),
                                            _p(lora_b if lora_a is not None else None), H, _p(dst), 3 * Rp, _stream()))
    return dst


def softmax_meanpool_bwd_f32(logits, stats, d_pooled, B, S, dlogits):
    C = logits.shape[1]
    _req(logits.dtype == F32 and logits.is_contiguous() and stats.dtype == F32 and d_pooled.dtype == F32 and d_pooled.is_contiguous()
         and dlogits.dtype == F32 and dlogits.shape[0] >= B * S and dlogits.shape[1] >= C, "softmax_meanpool_bwd_f32: f32 tensors")
    check(_l.load().bsclip_softmax_meanpool_bwd_f32(_p(logits), _p(stats), _p(d_pooled), B, S, C, _p(dlogits),
                                                    _rowmajor(dlogits, "dlogits"), _stream()))


def lora_grad_f32(dqkv, y, M, H, lora_a, lora_b, dA, dB):
    """dA [8, H] += ..., dB [2, H, 4] += ... from f32 dqkv [M, >= 3H] and the f32 LayerNorm output y [M, >= H]."""
    _req(dqkv.dtype == F32 and y.dtype == F32 and dqkv.shape[0] >= M and dqkv.shape[1] >= 3 * H and y.shape[0] >= M and y.shape[1] >= H,
         "lora_grad_f32 shapes")
    _f32_shaped(lora_a, (8, H), "lora_a")
    _f32_shaped(lora_b, (2, H, 4), "lora_b")
    _f32_shaped(dA, (8, H), "dA")
    _f32_shaped(dB, (2, H, 4), "dB")
    ws = _stream_ws(("lora_grad_f32", M, H), dqkv.device, _l.load().bsclip_lora_grad_f32_workspace_floats(M, H))
    check(_l.load().bsclip_lora_grad_f32(_p(dqkv), _rowmajor(dqkv, "dqkv"), _p(y), _rowmajor(y, "y"), M, H, _p(lora_a), _p(lora_b),
                                         _p(dA), _p(dB), _p(ws), _stream()))


def exact_attn_set_impl(impl):
    """0 = split-bf16 operands on the bf16 matrix cores (default, csrc/attn_x3.hip); 2 = f32-operand MFMA, 1 = vector-ALU kernels (exact-f32
    second implementations, for tests)."""
    check(_l.load().bsclip_exact_attn_set_impl(int(impl)))


def attn_bwd_f32(qkv, dctx, ctx, lse, B, S, heads, scale, dqkv, key_bias=None, dropout=None, dqkv_split3=None):
    """``dqkv_split3``: bf16 [>= B S, >= 9 heads 64] that receives [dq | dk | dv] as the QKV dX GEMM's split operand [hi | lo | hi]."""
    _req(all(t.dtype == F32 for t in (qkv, dctx, ctx, lse, dqkv)), "attn_bwd_f32 dtypes")
    ld_d3 = 0
    if dqkv_split3 is not None:
        ld_d3 = _rowmajor(dqkv_split3, "dqkv_split3")
        _req(dqkv_split3.dtype == BF16 and dqkv_split3.shape[0] >= B * S and dqkv_split3.shape[1] >= 9 * heads * 64, "attn_bwd_f32: dqkv_split3")
    _req(qkv.shape[0] >= B * S and qkv.shape[1] >= 3 * heads * 64 and dqkv.shape[0] >= B * S and dqkv.shape[1] >= 3 * heads * 64
         and ctx.shape[0] >= B * S and ctx.shape[1] >= heads * 64 and dctx.shape[0] >= B * S and dctx.shape[1] >= heads * 64
         and lse.numel() >= B * heads * S, "attn_bwd_f32 shapes")
    _key_bias_ok(key_bias, B, S)
    dp, ds = _drop(dropout)
    check(_l.load().bsclip_attn_bwd_f32(_p(qkv), _rowmajor(qkv, "qkv"), _p(dctx), _rowmajor(dctx, "dctx"), _p(ctx), _rowmajor(ctx, "ctx"),
                                        _p(lse), B, S, heads, _p(key_bias), float(scale), _p(dqkv), _rowmajor(dqkv, "dqkv"),
                                        _p(dqkv_split3), ld_d3, dp, ds, _stream()))


def im2col_patch16(image, cols):
    B = image.shape[0]
    _req(image.dtype == F32 and image.is_contiguous() and tuple(image.shape[1:]) == (3, 224, 224), "image f32 [B,3,224,224]")
    _req(cols.dtype in (BF16, F16) and cols.is_contiguous() and cols.shape[0] >= B * 196 and cols.shape[1] in (768, 2304),
         "cols bf16 / fp16 [B*196, 768] (or [B*196, 2304]: split rows [hi | lo | hi])")
    fmt = OPERANDS_FP16 if cols.dtype == F16 else 0
    check(_l.load().bsclip_im2col_patch16(_p(image), B, _p(cols), cols.shape[1], int(cols.shape[1] == 2304) | fmt, _stream()))


def mask_to_bias(mask, bias):
    _req(mask.dtype == torch.int64 and mask.is_contiguous() and bias.dtype == F32 and bias.is_contiguous()
         and bias.numel() >= mask.numel(), "mask_to_bias: int64 mask, f32 bias")
    check(_l.load().bsclip_mask_to_bias(_p(mask), mask.numel(), _p(bias), _stream()))


def vit_cls_rows(x, cls_token, pos_embed, B, S, H):
    _req(x.dtype in (F32, BF16, F16) and x.is_contiguous() and x.numel() >= B * S * H, "x f32 / bf16 / fp16 [B*S,H]")
    _req(cls_token.numel() == H and pos_embed.numel() >= H and cls_token.dtype == F32 and pos_embed.dtype == F32, "cls/pos")
    flag = {F32: 0, BF16: 1, F16: 1 | OPERANDS_FP16}[x.dtype]
    check(_l.load().bsclip_vit_cls_rows(_p(x), flag, _p(cls_token), _p(pos_embed), B, S, H, _stream()))


def bert_embed(ids, type_ids, word, pos, typ, out):
    B, S = ids.shape
    H = word.shape[1]
    _req(ids.dtype == torch.int64 and ids.is_contiguous(), "ids int64 [B,S]")
    if type_ids is not None:
        _req(type_ids.dtype == torch.int64 and type_ids.is_contiguous() and type_ids.shape == ids.shape, "type_ids")
    _req(all(t.dtype == F32 and t.is_contiguous() for t in (word, pos, typ, out)), "bert_embed tables f32")
    _req(pos.shape[0] >= S and pos.shape[1] == H and typ.shape[0] >= 2 and typ.shape[1] == H, "bert_embed: pos/type shapes")
    _req(out.shape[0] >= B * S and out.shape[1] == H, "bert_embed: out f32 [B*S,H]")
    check(_l.load().bsclip_bert_embed(_p(ids), _p(type_ids), B, S, H, _p(word), word.shape[0], _p(pos), _p(typ), _p(out),
                                      _stream()))


def softmax_meanpool_fwd(logits, B, S, pooled, stats):
    C = logits.shape[1]
    _req(logits.dtype == F32 and logits.is_contiguous() and logits.shape[0] >= B * S, "logits f32 [B*S,C]")
    _req(pooled.dtype == F32 and pooled.is_contiguous() and pooled.shape[0] >= B and pooled.shape[1] == C, "pooled")
    _req(stats.dtype == F32 and stats.numel() >= 2 * B * S, "stats")
    check(_l.load().bsclip_softmax_meanpool_fwd(_p(logits), B, S, C, _p(pooled), _p(stats), _stream()))


def softmax_meanpool_bwd(logits, stats, d_pooled, B, S, dlogits):
    C = logits.shape[1]
    _req(logits.dtype == F32 and logits.is_contiguous() and d_pooled.dtype == F32 and d_pooled.is_contiguous(), "dtypes")
    _req(d_pooled.shape[0] >= B and d_pooled.shape[1] == C, "d_pooled f32 [B,C]")
    _req(dlogits.dtype == BF16 and dlogits.shape[0] >= B * S and dlogits.shape[1] >= C, "dlogits bf16 [B*S,C]")
    check(_l.load().bsclip_softmax_meanpool_bwd(_p(logits), _p(stats), _p(d_pooled), B, S, C, _p(dlogits),
                                                _rowmajor(dlogits, "dlogits"), _stream()))


def meanpool_tokens_fwd(x, B, S, out):
    H = x.shape[1]
    _req(x.dtype == F32 and x.is_contiguous() and x.shape[0] >= B * S, "x f32 [B*S,H]")
    _req(out.dtype == BF16 and out.shape[0] >= B and out.shape[1] >= H, "out bf16 [B,H]")
    check(_l.load().bsclip_meanpool_tokens_fwd(_p(x), B, S, H, _p(out), _rowmajor(out, "out"), _stream()))


def meanpool_tokens_bwd(d_pooled, B, S, dx):
    H = dx.shape[1]
    _req(d_pooled.dtype == F32 and d_pooled.shape[0] >= B and d_pooled.shape[1] >= H, "d_pooled f32 [B,>=H]")
    _req(dx.dtype == F32 and dx.is_contiguous() and dx.shape[0] >= B * S, "dx f32 [B*S,H]")
    check(_l.load().bsclip_meanpool_tokens_bwd(_p(d_pooled), _rowmajor(d_pooled, "d_pooled"), B, S, H, _p(dx), _stream()))


def dgelu_mul(g, z, M, N, out):
    _req(all(t.dtype == BF16 and t.shape[0] >= M and t.shape[1] >= N for t in (g, out)), "dgelu_mul: g/out bf16 [M,>=N]")
    _req(z.dtype == torch.uint8 and z.shape[0] >= M and z.shape[1] >= N, "dgelu_mul: z uint8 codes [M,>=N]")
    check(_l.load().bsclip_dgelu_mul(_p(g), _rowmajor(g, "g"), _p(z), _rowmajor(z, "z"), M, N, _p(out),
                                     _rowmajor(out, "out"), _stream()))


def l2norm_fwd(x, y, inv_norm):
    M, D = x.shape
    _req(all(t.dtype == F32 and t.is_contiguous() for t in (x, y, inv_norm)), "l2norm_fwd f32 contiguous")
    _req(y.shape == x.shape and inv_norm.numel() >= M, "l2norm_fwd shapes")
    check(_l.load().bsclip_l2norm_fwd(_p(x), M, D, _p(y), _p(inv_norm), _stream()))


def l2norm_bwd(y, inv_norm, dy, dx):
    M, D = y.shape
    _req(all(t.dtype == F32 and t.is_contiguous() for t in (y, inv_norm, dy, dx)), "l2norm_bwd f32 contiguous")
    _req(dy.shape == y.shape and dx.shape == y.shape and inv_norm.numel() >= M, "l2norm_bwd shapes")
    check(_l.load().bsclip_l2norm_bwd(_p(y), _p(inv_norm), _p(dy), M, D, _p(dx), _stream()))


def infonce_set_impl(impl):
    """0 = fused InfoNCE epilogues (default), 1 = f32 logits slabs (kept for timing / cross-checks)."""
    check(_l.load().bsclip_infonce_set_impl(int(impl)))


def infonce_workspace_floats(N, nmod):
    n = _l.load().bsclip_infonce_workspace_floats(N, nmod)
    if n < 0:
        raise ValueError("Too less element for calculating the contrastive loss." if nmod < 2 else "bad N/nmod")
    return n


def _infonce_args(zs, labels, loss_out, dzs, row0, n_local, workspace):
    """The checks ``infonce_fwd_bwd`` and ``infonce_fwd_bwd_ts`` share; returns (nmod, N, D, n_local, zp, dzp)."""
    nmod = len(zs)
    if nmod < 2:
        raise ValueError("Too less element for calculating the contrastive loss.")
    N, D = zs[0].shape
    n_local = N if n_local is None else n_local
    _req(all(z.dtype == F32 and z.is_contiguous() and tuple(z.shape) == (N, D) for z in zs), "zs f32 [N,D]")
    _req(labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == N, "labels int64 [N]")
    _req(loss_out.dtype == F32 and loss_out.numel() >= 1, "loss_out f32 [1]")
    need = infonce_workspace_floats(N, nmod)
    _req(workspace is not None and workspace.dtype == F32 and workspace.numel() >= need and workspace.is_contiguous(),
         f"workspace must be f32 with >= {need} elements")
    zp = (ctypes.c_void_p * nmod)(*[z.data_ptr() for z in zs])
    dzp = None
    if dzs is not None:
        _req(len(dzs) == nmod and all(d.dtype == F32 and d.is_contiguous() and tuple(d.shape) == (n_local, D) for d in dzs),
             "dzs f32 [n_local, D]")
        dzp = (ctypes.c_void_p * nmod)(*[d.data_ptr() for d in dzs])
    return nmod, N, D, n_local, zp, dzp


def infonce_fwd_bwd(zs, labels, scale, loss_out, dzs=None, row0=0, n_local=None, workspace=None):
    """zs: list of 2-3 f32 [N, 768]; dzs: list of f32 [n_local, 768] (or None for loss only)."""
    nmod, N, D, n_local, zp, dzp = _infonce_args(zs, labels, loss_out, dzs, row0, n_local, workspace)
    check(_l.load().bsclip_infonce_fwd_bwd(zp, nmod, _p(labels), N, D, float(scale), row0, n_local, _p(loss_out), dzp,
                                           _p(workspace), _stream()))


def infonce_fwd_bwd_ts(zs, labels, log_scale, loss_out, dzs, scale_out, row0=0, n_local=None, workspace=None):
    """``infonce_fwd_bwd`` at the scale exp(clamp(t, 0, ln 100)), t = ``log_scale`` (one f32 on the GPU), read by the kernels when
    they run.  ``scale_out`` f32 [2] receives (the own rows' share of dLoss/dt, the scale used)."""
    _req(torch.is_tensor(log_scale) and log_scale.is_cuda and log_scale.dtype == F32 and log_scale.numel() == 1,
         "log_scale must be a 1-element f32 CUDA tensor")
    _req(torch.is_tensor(scale_out) and scale_out.is_cuda and scale_out.dtype == F32 and scale_out.is_contiguous()
         and scale_out.numel() >= 2, "scale_out must be a contiguous f32 CUDA tensor with >= 2 elements")
    nmod, N, D, n_local, zp, dzp = _infonce_args(zs, labels, loss_out, dzs, row0, n_local, workspace)
    check(_l.load().bsclip_infonce_fwd_bwd_ts(zp, nmod, _p(labels), N, D, _p(log_scale), row0, n_local, _p(loss_out), dzp,
                                              _p(scale_out), _p(workspace), _stream()))


def sigmoid_loss_fwd_bwd(zs, labels, log_scale, bias, loss_out, dzs, aux_out, row0=0, n_local=None, workspace=None):
    """The sigmoid (SigLIP) loss over every modality pair: x = s G + b with s = exp(clamp(t, 0, ln 100)), t = ``log_scale`` and
    b = ``bias`` (one f32 each on the GPU), read by the kernels when they run.  zs / dzs / row0 / n_local / workspace as for
    ``infonce_fwd_bwd``.  ``aux_out`` f32 [4] receives (the own rows' share of dLoss/dt, s, the own rows' share of dLoss/db, b)."""
    for name, v in (("log_scale", log_scale), ("bias", bias)):
        _req(torch.is_tensor(v) and v.is_cuda and v.dtype == F32 and v.numel() == 1, f"{name} must be a 1-element f32 CUDA tensor")
    _req(torch.is_tensor(aux_out) and aux_out.is_cuda and aux_out.dtype == F32 and aux_out.is_contiguous()
         and aux_out.numel() >= 4, "aux_out must be a contiguous f32 CUDA tensor with >= 4 elements")
    nmod, N, D, n_local, zp, dzp = _infonce_args(zs, labels, loss_out, dzs, row0, n_local, workspace)
    check(_l.load().bsclip_sigmoid_loss_fwd_bwd(zp, nmod, _p(labels), N, D, _p(log_scale), _p(bias), row0, n_local, _p(loss_out), dzp,
                                                _p(aux_out), _p(workspace), _stream()))



def xbm_bank_floats(Q):
    n = _l.load().bsclip_xbm_bank_floats(int(Q))
    if n < 0:
        raise ValueError(f"xbm: Q={Q} must be a multiple of 256 in 256 .. 16384")
    return n


def xbm_workspace_floats(N, Q, nmod):
    n = _l.load().bsclip_xbm_workspace_floats(int(N), int(Q), int(nmod))
    if n < 0:
        raise ValueError(f"xbm: bad N={N} (1 .. 1024, <= Q) / Q={Q} (a multiple of 256 in 256 .. 16384) / nmod={nmod} (2 or 3)")
    return n


def _xbm_args(zs, labels, banks, bank_labels, state, workspace, name):
    """The checks ``xbm_enqueue`` and ``infonce_xbm`` share; returns (nmod, N, D, Q, zp, bp)."""
    nmod = len(zs)
    if nmod < 2:
        raise ValueError("Too less element for calculating the contrastive loss.")
    N, D = zs[0].shape
    dev = zs[0].device
    _req(all(z.is_cuda and z.dtype == F32 and z.is_contiguous() and tuple(z.shape) == (N, D) for z in zs), f"{name}: zs f32 [N,D] on the GPU")
    _req(labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == N and labels.device == dev, f"{name}: labels int64 [N]")
    _req(bank_labels.dtype == torch.int64 and bank_labels.is_contiguous() and bank_labels.dim() == 1 and bank_labels.device == dev,
         f"{name}: bank_labels int64 [Q]")
    Q = bank_labels.numel()
    need = xbm_bank_floats(Q)
    _req(len(banks) == nmod and all(b.dtype == F32 and b.is_contiguous() and b.numel() >= need and b.device == dev for b in banks),
         f"{name}: one contiguous f32 bank of >= {need} elements per modality")
    _i32(state, dev, f"{name}: state must be a contiguous int32 [2] tensor on the inputs' GPU", shape=(2,))
    need = xbm_workspace_floats(N, Q, nmod)
    _req(workspace is not None and workspace.dtype == F32 and workspace.numel() >= need and workspace.is_contiguous()
         and workspace.device == dev, f"{name}: workspace must be f32 with >= {need} elements")
    zp = (ctypes.c_void_p * nmod)(*[z.data_ptr() for z in zs])
    bp = (ctypes.c_void_p * nmod)(*[b.data_ptr() for b in banks])
    return nmod, N, D, Q, zp, bp


def xbm_enqueue(zs, labels, banks, bank_labels, state, workspace):
    """Write the normalised rows of ``zs`` (2-3 f32 [N, 768]) and ``labels`` into the ring at ``state`` = (head, filled), int32 [2] on
    the GPU, and advance it there; nothing is written when a row holds a non-finite value (``bsclip_xbm_enqueue``)."""
    nmod, N, D, Q, zp, bp = _xbm_args(zs, labels, banks, bank_labels, state, workspace, "xbm_enqueue")
    check(_l.load().bsclip_xbm_enqueue(zp, nmod, _p(labels), N, D, bp, _p(bank_labels), Q, _p(state), _p(workspace), _stream()))


def infonce_xbm(zs, labels, log_scale, banks, bank_labels, state, loss_out, dzs, scale_out, workspace):
    """InfoNCE with the valid bank slots as extra keys (``bsclip_infonce_xbm_fwd_bwd``): ``log_scale`` is t = log(scale), one f32 on
    the GPU; ``scale_out`` f32 [2] receives (dLoss/dt, the scale used); ``dzs`` f32 [N, 768] per modality, or None for the loss only."""
    _req(torch.is_tensor(log_scale) and log_scale.is_cuda and log_scale.dtype == F32 and log_scale.numel() == 1,
         "log_scale must be a 1-element f32 CUDA tensor")
    _req(torch.is_tensor(scale_out) and scale_out.is_cuda and scale_out.dtype == F32 and scale_out.is_contiguous()
         and scale_out.numel() >= 2, "scale_out must be a contiguous f32 CUDA tensor with >= 2 elements")
    nmod, N, D, Q, zp, bp = _xbm_args(zs, labels, banks, bank_labels, state, workspace, "infonce_xbm")
    _req(loss_out.dtype == F32 and loss_out.is_cuda and loss_out.numel() >= 1, "loss_out f32 [1]")
    dzp = None
    if dzs is not None:
        _req(len(dzs) == nmod and all(d.dtype == F32 and d.is_contiguous() and d.is_cuda and tuple(d.shape) == (N, D) for d in dzs),
             "dzs f32 [N, D]")
        dzp = (ctypes.c_void_p * nmod)(*[d.data_ptr() for d in dzs])
    check(_l.load().bsclip_infonce_xbm_fwd_bwd(zp, nmod, _p(labels), N, D, _p(log_scale), bp, _p(bank_labels), Q, _p(state),
                                               _p(loss_out), dzp, _p(scale_out), _p(workspace), _stream()))


def _topk_outputs(queries, K, k, msg_q, msg_k):
    """What ``topk_ip`` and ``topk_ip_indexed`` share: the query check and the outputs.  Returns (Q, D, scores, idx)."""
    _req(queries.dim() == 2 and queries.dtype == F32 and queries.is_contiguous() and queries.is_cuda, msg_q)
    Q, D = queries.shape
    _req(Q >= 1 and 1 <= k <= min(16, K) and D % 64 == 0, msg_k)
    return Q, D, torch.empty(Q, k, dtype=F32, device=queries.device), torch.empty(Q, k, dtype=torch.int64, device=queries.device)


def topk_ip(queries, keys, k):
    """Top-k inner products of L2-normalised rows: returns (scores f32 [Q,k], indices int64 [Q,k]) on the GPU."""
    K = keys.shape[0]
    msg = "topk_ip: contiguous f32 GPU [Q,D], [K,D]"
    Q, D, scores, idx = _topk_outputs(queries, K, k, msg, "topk_ip: 1 <= k <= 16, D % 64 == 0")
    _req(keys.dtype == F32 and keys.is_contiguous() and tuple(keys.shape) == (K, D) and keys.is_cuda, msg)
    ws = torch.empty(_l.load().bsclip_topk_ip_workspace_floats(Q, K, D), dtype=F32, device=queries.device)
    check(_l.load().bsclip_topk_ip(_p(queries), Q, _p(keys), K, D, k, _p(scores), _p(idx), _p(ws), _stream()))
    return scores, idx


I32 = torch.int32


def retrieval_index_build(keys):
    """The key operand of ``topk_ip`` built once (faiss ``index.add``): returns the f32-typed buffer ``topk_ip_indexed`` searches."""
    _req(keys.dim() == 2 and keys.dtype == F32 and keys.is_contiguous() and keys.is_cuda, "retrieval_index_build: contiguous f32 GPU [K,D]")
    K, D = keys.shape
    _req(K >= 1 and D % 64 == 0, "retrieval_index_build: K >= 1, D % 64 == 0")
    index = torch.empty(_l.load().bsclip_retrieval_index_floats(K, D), dtype=F32, device=keys.device)
    check(_l.load().bsclip_retrieval_index_build(_p(keys), K, D, _p(index), _stream()))
    return index


def topk_ip_indexed(queries, index, K, k):
    """``topk_ip`` against a prebuilt index of K keys (``retrieval_index_build``): same kernels, bit-identical outputs."""
    Q, D, scores, idx = _topk_outputs(queries, K, k, "topk_ip_indexed: contiguous f32 GPU [Q,D]",
                                      "topk_ip_indexed: Q >= 1, 1 <= k <= 16, k <= K, D % 64 == 0")
    _req(index.dtype == F32 and index.is_contiguous() and index.device == queries.device
         and index.numel() == _l.load().bsclip_retrieval_index_floats(K, D), "topk_ip_indexed: index is not that of [K,D] keys")
    ws = torch.empty(_l.load().bsclip_topk_ip_indexed_workspace_floats(Q, K, D), dtype=F32, device=queries.device)
    check(_l.load().bsclip_topk_ip_indexed(_p(queries), Q, _p(index), K, D, k, _p(scores), _p(idx), _p(ws), _stream()))
    return scores, idx


def retrieval_index_empty(K, D, device):
    """A zero-filled index buffer for K keys of width D: what ``retrieval_index_append`` fills and ``topk_ip_indexed`` searches."""
    _req(K >= 1 and D >= 64 and D % 64 == 0, "retrieval_index_empty: K >= 1, D % 64 == 0")
    return torch.zeros(_l.load().bsclip_retrieval_index_floats(K, D), dtype=F32, device=device)


def retrieval_index_append(index, K, keys, row0):
    """Rows ``[row0, row0 + n)`` of an index for K keys (``retrieval_index_empty``) from ``keys`` f32 ``[n, D]``: the rows
    ``retrieval_index_build`` of the whole table would have written, bit for bit."""
    _req(keys.dim() == 2 and keys.dtype == F32 and keys.is_contiguous() and keys.is_cuda, "retrieval_index_append: contiguous f32 GPU [n,D]")
    n, D = keys.shape
    _req(n >= 1 and D % 64 == 0 and 0 <= row0 and row0 + n <= K, "retrieval_index_append: n >= 1, D % 64 == 0, 0 <= row0, row0 + n <= K")
    _req(index.dtype == F32 and index.is_contiguous() and index.device == keys.device
         and index.numel() == _l.load().bsclip_retrieval_index_floats(K, D), "retrieval_index_append: index is not that of [K,D] keys")
    check(_l.load().bsclip_retrieval_index_append(_p(keys), n, D, _p(index), K, int(row0), _stream()))


def feature_rows(image, dna, text, row0, t_image=None, t_dna=None, t_text=None, t_avg=None, t_cat=None):
    """One batch of encoder outputs (each f32 ``[B, D]`` or None) into rows ``[row0, row0 + B)`` of its ``[N, D]`` table (None exactly
    where the input is), ``(image + dna) * 0.5`` into ``t_avg [N, D]`` and ``[image | dna]`` into ``t_cat [N, 2 D]`` (both optional)."""
    ins, tabs = (image, dna, text), (t_image, t_dna, t_text)
    first = next((x for x in ins if x is not None), None)
    _req(first is not None and first.dim() == 2 and first.is_cuda, "feature_rows: at least one f32 GPU [B,D] input")
    (B, D), dev = first.shape, first.device
    given = [t for t in (*tabs, t_avg) if t is not None]
    _req(len(given) > 0 and given[0].dim() == 2, "feature_rows: a table per input")
    N = given[0].shape[0]
    _req(B >= 1 and D % 4 == 0 and 0 <= row0 and row0 + B <= N, "feature_rows: B >= 1, D % 4 == 0, 0 <= row0, row0 + B <= N")
    for x, t in zip(ins, tabs):
        _req((x is None) == (t is None), "feature_rows: an input and its table are given together")
        if x is not None:
            _req(x.dtype == F32 and x.is_contiguous() and x.device == dev and tuple(x.shape) == (B, D), "feature_rows: inputs contiguous f32 [B,D]")
    for t, width in (*[(t, D) for t in tabs], (t_avg, D), (t_cat, 2 * D)):
        if t is not None:
            _req(t.dtype == F32 and t.is_contiguous() and t.device == dev and tuple(t.shape) == (N, width),
                 "feature_rows: tables contiguous f32 [N,D] (t_cat [N,2D]) on the inputs' GPU")
    _req((t_avg is None and t_cat is None) or (image is not None and dna is not None), "feature_rows: t_avg / t_cat need image and dna")
    check(_l.load().bsclip_feature_rows(_p(image), _p(dna), _p(text), B, D, int(row0), N, _p(t_image), _p(t_dna), _p(t_text), _p(t_avg),
                                        _p(t_cat), _stream()))


def _eval_flag(flag, device):
    if flag is None:
        return torch.zeros(1, dtype=I32, device=device), True
    _req(flag.dtype == I32 and flag.numel() == 1 and flag.device == device, "flag: int32 [1] on the same GPU")
    return flag, False


def check_retrieval_flag(word):
    """Raise for the error bits the scoring kernels OR into their flag word (``word``: its value on the host)."""
    if word & 1:
        raise ValueError("retrieval_hit_ranks: an idx entry lies outside [0, K)")
    if word & 2:
        raise ValueError("retrieval_class_counts / retrieval_match_bits: a label lies outside its level's class range or the member table")


def retrieval_hit_ranks(idx, key_labels, query_labels, flag=None):
    """hit_rank int32 [Q,L]: the first rank r < k with key_labels[idx[q,r], l] == query_labels[q,l], or k.  Without ``flag`` the
    error word is read back here and a bad idx raises; with a caller's ``flag`` (int32 [1], cleared by the caller) nothing
    synchronises and the caller runs ``check_retrieval_flag`` on it."""
    _req(idx.dim() == 2 and idx.dtype == torch.int64 and idx.is_contiguous() and idx.is_cuda, "retrieval_hit_ranks: idx int64 GPU [Q,k]")
    Q, k = idx.shape
    dev = idx.device
    for labels in (key_labels, query_labels):
        _i32(labels, dev, "retrieval_hit_ranks: labels int32 contiguous [K,L], [Q,L] on idx's GPU", dims=(2,))
    K, L = key_labels.shape
    _req(Q >= 1 and K >= 1 and 1 <= k <= 16 and 1 <= L <= 8 and tuple(query_labels.shape) == (Q, L),
         "retrieval_hit_ranks: 1 <= k <= 16, 1 <= L <= 8, query_labels [Q,L]")
    flag, own = _eval_flag(flag, dev)
    hit_rank = torch.empty(Q, L, dtype=I32, device=dev)
    check(_l.load().bsclip_retrieval_hit_ranks(_p(idx), Q, k, _p(key_labels), K, _p(query_labels), L, _p(hit_rank), _p(flag), _stream()))
    if own:
        check_retrieval_flag(int(flag.item()))
    return hit_rank


def retrieval_class_counts(hit_rank, query_labels, level_offsets, k_list, flag=None, out=None):
    """(seen int32 [C], right int32 [nk,C]) with C = level_offsets[-1]: queries per class and those hit within k_list[j].
    ``level_offsets`` / ``k_list`` are host sequences.  ``out``: an int32 buffer of (1 + nk) * C elements to hold both."""
    dev = hit_rank.device
    msg = "retrieval_class_counts: hit_rank, query_labels int32 GPU [Q,L]"
    _i32(hit_rank, dev, msg, dims=(2,))
    _i32(query_labels, dev, msg, shape=hit_rank.shape)
    Q, L = hit_rank.shape
    offs, ks = [int(o) for o in level_offsets], [int(k) for k in k_list]
    nk = len(ks)
    _req(Q >= 1 and 1 <= L <= 8 and len(offs) == L + 1 and 1 <= nk <= 8, "retrieval_class_counts: L <= 8 levels, L + 1 offsets, nk <= 8")
    _req(offs[0] == 0 and all(a <= b for a, b in zip(offs, offs[1:])) and offs[-1] >= 1 and min(ks) >= 1,
         "retrieval_class_counts: offsets start at 0 and do not decrease, k >= 1")
    C = offs[-1]
    flag, own = _eval_flag(flag, dev)
    if out is None:
        out = torch.empty((1 + nk) * C, dtype=I32, device=dev)
    _i32(out, dev, "retrieval_class_counts: out int32 [(1+nk)*C]")
    _req(out.numel() == (1 + nk) * C, "retrieval_class_counts: out int32 [(1+nk)*C]")
    seen, right = out[:C], out[C:].view(nk, C)
    c_offs, c_ks = (ctypes.c_int32 * (L + 1))(*offs), (ctypes.c_int32 * nk)(*ks)
    check(_l.load().bsclip_retrieval_class_counts(_p(hit_rank), _p(query_labels), Q, L, ctypes.cast(c_offs, ctypes.c_void_p),
                                                  ctypes.cast(c_ks, ctypes.c_void_p), nk, _p(seen), _p(right), _p(flag), _stream()))
    if own:
        check_retrieval_flag(int(flag.item()))
    return seen, right


def _masks(name, sim, A, B):
    _req(sim.dim() == 2 and sim.dtype == F32 and sim.is_contiguous() and sim.is_cuda, f"{name}: sim f32 contiguous GPU [Q,k]")
    Q, k = sim.shape
    msg = f"{name}: A, B int32 contiguous [Q,L] (or [Q]) on sim's GPU"
    _i32(A, sim.device, msg, dims=(1, 2))
    _i32(B, sim.device, msg, shape=A.shape)
    _req(A.shape[0] == Q, msg)
    L = A.shape[1] if A.dim() == 2 else 1
    _req(Q >= 1 and 1 <= k <= 16 and 1 <= L <= 8, f"{name}: Q >= 1, 1 <= k <= 16, 1 <= L <= 8")
    return Q, k, L


def retrieval_match_bits(idx, key_labels, query_labels=None, member=None, level=0, flag=None):
    """bits int32 [Q,L]: bit r set exactly when key_labels[idx[q,r], l] == query_labels[q,l].  With ``member`` (int32 0/1 [C]) the
    member mask int32 [Q] of column ``level`` instead: bit r set exactly when member[key_labels[idx[q,r], level]] != 0.  ``flag`` as
    for ``retrieval_hit_ranks``: an idx outside [0, K) or a label outside the member table sets its bit and is not read."""
    _req(idx.dim() == 2 and idx.dtype == torch.int64 and idx.is_contiguous() and idx.is_cuda, "retrieval_match_bits: idx int64 GPU [Q,k]")
    Q, k = idx.shape
    dev = idx.device
    _i32(key_labels, dev, "retrieval_match_bits: key_labels int32 contiguous [K,L] on idx's GPU", dims=(2,))
    K, L = key_labels.shape
    _req(Q >= 1 and K >= 1 and 1 <= k <= 16 and 1 <= L <= 8, "retrieval_match_bits: Q, K >= 1, 1 <= k <= 16, 1 <= L <= 8")
    C = 0
    if member is None:
        _i32(query_labels, dev, "retrieval_match_bits: query_labels int32 contiguous [Q,L] on idx's GPU", shape=(Q, L))
        bits = torch.empty(Q, L, dtype=I32, device=dev)
    else:
        _i32(member, dev, "retrieval_match_bits: member int32 contiguous [C] on idx's GPU", dims=(1,))
        _req(member.numel() >= 1, "retrieval_match_bits: member int32 contiguous [C] on idx's GPU")
        _req(0 <= int(level) < L, "retrieval_match_bits: 0 <= level < L")
        C, query_labels = member.numel(), None
        bits = torch.empty(Q, dtype=I32, device=dev)
    flag, own = _eval_flag(flag, dev)
    check(_l.load().bsclip_retrieval_match_bits(_p(idx), Q, k, _p(key_labels), K, _p(query_labels), L, _p(member), C, int(level),
                                                _p(bits), _p(flag), _stream()))
    if own:
        check_retrieval_flag(int(flag.item()))
    return bits


def retrieval_merge_hit_ranks(sim, A, B, threshold):
    """hit_rank int32 (the shape of A): the lowest r < k with bit r of (A & s) | (B & ~s) set, or k, where bit r of s is
    ``float64(sim[q,r]) > threshold`` (strict; a NaN similarity selects B)."""
    Q, k, L = _masks("retrieval_merge_hit_ranks", sim, A, B)
    hit_rank = torch.empty_like(A)
    check(_l.load().bsclip_retrieval_merge_hit_ranks(_p(sim), Q, k, _p(A), _p(B), L, float(threshold), _p(hit_rank), _stream()))
    return hit_rank


def retrieval_threshold_sweep(sim, A, B, level, k_prime, thresholds, out=None):
    """counts int32 [T]: per threshold (``thresholds`` float64 GPU [T]) the number of queries whose merged hit rank at ``level`` is
    below ``k_prime``.  ``out``: a zeroed int32 [T] buffer the counts are added to (default: a fresh one)."""
    Q, k, L = _masks("retrieval_threshold_sweep", sim, A, B)
    _req(thresholds.dim() == 1 and thresholds.dtype == torch.float64 and thresholds.is_contiguous() and thresholds.device == sim.device
         and thresholds.numel() >= 1, "retrieval_threshold_sweep: thresholds float64 contiguous [T] on sim's GPU")
    T = thresholds.numel()
    _req(0 <= int(level) < L and int(k_prime) >= 1, "retrieval_threshold_sweep: 0 <= level < L, k_prime >= 1")
    if out is None:
        out = torch.zeros(T, dtype=I32, device=sim.device)
    _i32(out, sim.device, "retrieval_threshold_sweep: out int32 [T]")
    _req(out.numel() == T, "retrieval_threshold_sweep: out int32 [T]")
    check(_l.load().bsclip_retrieval_threshold_sweep(_p(sim), Q, k, _p(A), _p(B), L, int(level), int(k_prime), _p(thresholds), T,
                                                     _p(out), _stream()))
    return out


def check_ce_flag(word, what="target"):
    """Raise for the error bit ``ce_fwd_bwd`` ORs into its flag word (``word``: its value on the host)."""
    if word & 1:
        raise ValueError(f"ce_fwd_bwd: a {what} index lies outside [0, C)")


def ce_fwd_bwd(logits, targets, C, loss_out, row_loss, dlogits=None, dlogits_split3=None, flag=None):
    """Mean cross-entropy of the class logits ``logits[:B, :C]`` (f32 [B, ldc >= C], a padded buffer) against ``targets`` (int32 [B]) into
    ``loss_out`` (f32 [1]), and dlogits = (softmax - onehot) / B as f32 [B, >= C] (``dlogits``) and / or as the split-bf16 operand
    [hi | lo | hi] over C rounded up to 64 columns (``dlogits_split3`` bf16 [B, >= 3 Cp]).  Without ``flag`` the error word is read
    back here and a target outside [0, C) raises; with a caller's ``flag`` (int32 [1], cleared by the caller) nothing synchronises
    and the caller runs ``check_ce_flag`` on it."""
    ldc = _rowmajor(logits, "logits")
    B = logits.shape[0]
    dev = logits.device
    _req(logits.dtype == F32 and B >= 1 and 1 <= C <= logits.shape[1] and ldc % 4 == 0, "ce_fwd_bwd: logits f32 [B, >= C], row stride % 4 == 0")
    _req(targets.dtype == I32 and targets.is_contiguous() and targets.numel() == B and targets.device == dev, "ce_fwd_bwd: targets int32 [B]")
    _req(loss_out.dtype == F32 and loss_out.numel() >= 1 and loss_out.device == dev, "ce_fwd_bwd: loss_out f32 [1]")
    _req(row_loss.dtype == F32 and row_loss.is_contiguous() and row_loss.numel() >= B and row_loss.device == dev, "ce_fwd_bwd: row_loss f32 [B]")
    Cp = (C + 63) // 64 * 64
    ld_d = ld_d3 = 0
    if dlogits is not None:
        ld_d = _rowmajor(dlogits, "dlogits")
        _req(dlogits.dtype == F32 and dlogits.shape[0] >= B and dlogits.shape[1] >= C and ld_d % 4 == 0, "ce_fwd_bwd: dlogits f32 [B, >= C]")
    if dlogits_split3 is not None:
        ld_d3 = _rowmajor(dlogits_split3, "dlogits_split3")
        _req(dlogits_split3.dtype == BF16 and dlogits_split3.shape[0] >= B and dlogits_split3.shape[1] >= 3 * Cp and ld_d3 % 4 == 0,
             "ce_fwd_bwd: dlogits_split3 bf16 [B, >= 3 x (C rounded up to 64)]")
    flag, own = _eval_flag(flag, dev)
    check(_l.load().bsclip_ce_fwd_bwd(_p(logits), ldc, _p(targets), B, C, _p(loss_out), _p(row_loss), _p(dlogits), ld_d,
                                      _p(dlogits_split3), ld_d3, _p(flag), _stream()))
    if own:
        check_ce_flag(int(flag.item()))


def _class_topk(name, logits, C, k, out=None):
    ldc = _rowmajor(logits, "logits")
    B = logits.shape[0]
    _req(logits.dtype == F32 and B >= 1 and 1 <= C <= logits.shape[1] and ldc % 4 == 0, f"{name}: logits f32 [B, >= C], row stride % 4 == 0")
    _req(1 <= k <= min(16, C), f"{name}: 1 <= k <= 16, k <= C")
    if out is None:
        out = torch.empty(B, k, dtype=F32, device=logits.device)
        idx = torch.empty(B, k, dtype=torch.int64, device=logits.device)
    else:
        out, idx = out
        for t, dt in ((out, F32), (idx, torch.int64)):
            _req(t.dtype == dt and t.is_contiguous() and t.device == logits.device and tuple(t.shape) == (B, k),
                 f"{name}: out = (f32 [B, k], int64 [B, k]), contiguous, on the logits' GPU")
    check(getattr(_l.load(), "bsclip_" + name)(_p(logits), ldc, B, C, k, _p(out), _p(idx), _stream()))
    return out, idx


def class_topk(logits, C, k):
    """The k (<= 16, <= C) largest of ``logits[:, :C]`` per row, descending, ties to the lower class index: (scores f32 [B, k],
    indices int64 [B, k]) on the GPU.  ``logits`` f32 [B, >= C] may be a view into a padded buffer (row stride % 4 == 0)."""
    return _class_topk("class_topk", logits, C, k)


def class_softmax_topk(logits, C, k, out=None):
    """``F.softmax(logits[:, :C], -1)`` then ``torch.topk(..., k, sorted=True)`` in one kernel: (confidences f32 [B, k], class indices
    int64 [B, k]) on the GPU, ordered by logit descending, ties to the lower class index.  ``logits`` as for ``class_topk``.
    ``out``: the pair of tensors to write to, e.g. rows ``[row0, row0 + B)`` of a split's ``[Q, k]`` tables."""
    return _class_topk("class_softmax_topk", logits, C, k, out=out)


def check_silhouette_flag(word):
    """Raise for the error bits ``silhouette_samples`` ORs into its flag word (``word``: its value on the host)."""
    if word & 2:
        raise ValueError("silhouette_samples: seg_start is not a non-decreasing sequence from 0 to N")
    if word & 1:
        raise ValueError("silhouette_samples: the features hold a NaN or an infinity (or a squared distance overflows float32)")


def silhouette_samples(x_sorted, seg_start, D=None, out=None, flag=None):
    """Silhouette coefficients f32 [N] of the class-sorted rows ``x_sorted[:, :D]`` (f32 GPU [N, >= D], row stride % 4 == 0; D
    defaults to the width), class c being the rows ``[seg_start[c], seg_start[c+1])`` (``seg_start`` int32 GPU [C + 1]), in the
    sorted order.  ``out``: an f32 buffer of >= N elements to write them to (the rest is left alone).  ``flag`` as for
    ``retrieval_hit_ranks``: without it the error word is read back here and bad input raises; with a caller's word nothing
    synchronises and the caller runs ``check_silhouette_flag`` on it."""
    ld = _rowmajor(x_sorted, "x_sorted")
    N = x_sorted.shape[0]
    D = x_sorted.shape[1] if D is None else int(D)
    dev = x_sorted.device
    _req(x_sorted.dtype == F32 and 1 <= D <= x_sorted.shape[1] and ld % 4 == 0 and x_sorted.data_ptr() % 16 == 0,
         "silhouette_samples: x_sorted f32 [N, >= D], row stride % 4 == 0, 16-byte aligned")
    _i32(seg_start, dev, "silhouette_samples: seg_start int32 contiguous [C + 1] on x_sorted's GPU", dims=(1,))
    C = seg_start.numel() - 1
    _req(N >= 3 and 2 <= C <= N - 1, "silhouette_samples: N >= 3 samples in 2 .. N - 1 classes")
    if out is None:
        out = torch.empty(N, dtype=F32, device=dev)
    _req(out.dtype == F32 and out.dim() == 1 and out.is_contiguous() and out.numel() >= N and out.device == dev,
         "silhouette_samples: out f32 contiguous [>= N] on x_sorted's GPU")
    flag, own = _eval_flag(flag, dev)
    check(_l.load().bsclip_silhouette_samples(_p(x_sorted), ld, N, D, _p(seg_start), C, _p(out), _p(flag), _stream()))
    if own:
        check_silhouette_flag(int(flag.item()))
    return out[:N]


def _lora_grad_workspace(H, device):
    return _stream_ws(("lora_grad", H), device, _l.load().bsclip_lora_grad_workspace_floats(H))


def lora_grad(dqkv, h_aug, M, H, lora_b, dt, dA, dBq, dBv):
    _req(dqkv.dtype == BF16 and h_aug.dtype == BF16, "lora_grad: bf16 inputs")
    _req(dqkv.shape[0] >= M and dqkv.shape[1] >= 3 * H and h_aug.shape[0] >= M and h_aug.shape[1] >= H + 8, "lora_grad shapes")
    _f32_shaped(lora_b, (2, H, 4), "lora_b")
    _lora_grads_ok(M, H, dt, dA, dBq, dBv)
    check(_l.load().bsclip_lora_grad(_p(dqkv), _rowmajor(dqkv, "dqkv"), _p(h_aug), _rowmajor(h_aug, "h_aug"), M, H,
                                     _p(lora_b), _p(dt), _p(dA), _p(dBq), _p(dBv),
                                     _p(_lora_grad_workspace(H, dqkv.device)), _stream()))


def lora_grad_heads(h_aug, M, H, B, dt_partial, db_partial, dt, dA, dBq, dBv, grad_scale_log2=None):
    """``lora_grad`` from the partial sums ``attn_bwd(..., lora=...)`` left: dt [M, 8], dBq / dBv and dA accumulate as ``lora_grad`` (dt_partial f32 [heads, 2, M, 4], db_partial f32 [B heads, 2, 4, 64]).
    fp16 ``h_aug`` (bsclip_lora_grad_heads_f16): the partials and dt hold 2^grad_scale_log2 times the gradient; dA / dB get the true one."""
    heads = H // 64
    if h_aug.dtype == F16:
        _req(grad_scale_log2 is not None and 0 <= int(grad_scale_log2) <= 64, "lora_grad_heads: fp16 h_aug needs grad_scale_log2 in [0, 64]")
    else:
        _req(grad_scale_log2 is None, "lora_grad_heads: grad_scale_log2 is for the fp16 form")
    _req(h_aug.dtype in (BF16, F16) and h_aug.shape[0] >= M and h_aug.shape[1] >= H and M % B == 0, "lora_grad_heads: h_aug bf16 [M, >= H]")
    _req(dt_partial.dtype == F32 and dt_partial.is_contiguous() and dt_partial.numel() >= heads * M * 8
         and db_partial.dtype == F32 and db_partial.is_contiguous() and db_partial.numel() >= B * heads * 512, "lora_grad_heads: partials")
    _lora_grads_ok(M, H, dt, dA, dBq, dBv)
    if h_aug.dtype == F16:
        check(_l.load().bsclip_lora_grad_heads_f16(_p(h_aug), _rowmajor(h_aug, "h_aug"), M, H, B, _p(dt_partial), _p(db_partial), _p(dt),
                                                   _p(dA), _p(dBq), _p(dBv), _p(_lora_grad_workspace(H, h_aug.device)),
                                                   OPERANDS_FP16 | int(grad_scale_log2), _stream()))
        return
    check(_l.load().bsclip_lora_grad_heads(_p(h_aug), _rowmajor(h_aug, "h_aug"), M, H, B, _p(dt_partial), _p(db_partial), _p(dt), _p(dA),
                                           _p(dBq), _p(dBv), _p(_lora_grad_workspace(H, h_aug.device)), _stream()))


def lora_grad_fp8(dqkv, y_fp8, t_aug, M, H, lora_b, dt, dA, dBq, dBv):
    _req(dqkv.dtype == BF16 and y_fp8.dtype == FP8 and t_aug.dtype == BF16, "lora_grad_fp8: dtypes")
    _req(dqkv.shape[0] >= M and dqkv.shape[1] >= 3 * H and y_fp8.shape[0] >= M and y_fp8.shape[1] >= H
         and t_aug.shape[0] >= M and t_aug.shape[1] >= 8, "lora_grad_fp8 shapes")
    _f32_shaped(lora_b, (2, H, 4), "lora_b")
    _lora_grads_ok(M, H, dt, dA, dBq, dBv)
    check(_l.load().bsclip_lora_grad_fp8(_p(dqkv), _rowmajor(dqkv, "dqkv"), _p(y_fp8), _rowmajor(y_fp8, "y_fp8"), _p(t_aug),
                                         _rowmajor(t_aug, "t_aug"), M, H, _p(lora_b), _p(dt), _p(dA), _p(dBq), _p(dBv),
                                         _p(_lora_grad_workspace(H, dqkv.device)), _stream()))


def colsum(g, M, N, out):
    _req(g.dtype in (BF16, F32) and g.shape[0] >= M and g.shape[1] >= N, "colsum: g")
    _req(out.dtype == F32 and out.is_contiguous() and out.numel() >= N, "colsum: out f32 [N]")
    check(_l.load().bsclip_colsum(_p(g), _rowmajor(g, "g"), int(g.dtype == BF16), M, N, _p(out), _stream()))


def transpose_bf16(src, R, C, dst):
    """dst[C, R] = src[R, C]^T for 16-bit words: bf16, or fp16 (the kernel only moves the words)."""
    _req(src.dtype in (BF16, F16) and dst.dtype == src.dtype, "transpose_bf16 dtypes (bf16 or fp16, both the same)")
    _req(src.shape[0] >= R and src.shape[1] >= C and dst.shape[0] >= C and dst.shape[1] >= R, "transpose_bf16 shapes")
    check(_l.load().bsclip_transpose_bf16(_p(src), _rowmajor(src, "src"), R, C, _p(dst), _rowmajor(dst, "dst"), _stream()))


def transpose_colsum_bf16(src, R, C, dst, colsum_out):
    """dst[C, R] = src[R, C]^T and colsum_out[c] += sum_r src[r, c] in one pass over src (weight-gradient operand + bias gradient)."""
    _req(src.dtype == BF16 and dst.dtype == BF16, "transpose_colsum_bf16 dtypes")
    _req(src.shape[0] >= R and src.shape[1] >= C and dst.shape[0] >= C and dst.shape[1] >= R, "transpose_colsum_bf16 shapes")
    _req(colsum_out.dtype == F32 and colsum_out.is_contiguous() and colsum_out.numel() >= C, "transpose_colsum_bf16: colsum f32 [C]")
    lib = _l.load()
    ws = _stream_ws("transpose_colsum", src.device, lib.bsclip_transpose_colsum_workspace_floats(R, C))
    check(lib.bsclip_transpose_colsum_bf16(_p(src), _rowmajor(src, "src"), R, C, _p(dst), _rowmajor(dst, "dst"), _p(colsum_out),
                                           _p(ws), _stream()))


def cast_f32_bf16(src, dst):
    """dst = src rounded to dst's 16-bit format: bf16, or fp16 (bsclip_cast_f32_f16)."""
    _req(src.dtype == F32 and dst.dtype in (BF16, F16) and src.is_contiguous() and dst.is_contiguous()
         and dst.numel() >= src.numel(), "cast_f32_bf16")
    fn = _l.load().bsclip_cast_f32_f16 if dst.dtype == F16 else _l.load().bsclip_cast_f32_bf16
    check(fn(_p(src), src.numel(), _p(dst), _stream()))


def cast_f32_f16_scaled(src, dst, scale_log2):
    """dst fp16 = RNE(src * 2^scale_log2): the scaled dout of the fp16-operand backward (one static power of two per tower)."""
    _req(src.dtype == F32 and dst.dtype == F16 and src.is_contiguous() and dst.is_contiguous() and dst.numel() >= src.numel(),
         "cast_f32_f16_scaled")
    check(_l.load().bsclip_cast_f32_f16_scaled(_p(src), src.numel(), int(scale_log2), _p(dst), _stream()))


def add_scaled_f32(src, dst, scale_log2):
    """dst += src * 2^scale_log2 (f32, same size, contiguous): exact removal of a static gradient scale."""
    _req(src.dtype == F32 and dst.dtype == F32 and src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel(),
         "add_scaled_f32")
    check(_l.load().bsclip_add_scaled_f32(_p(src), src.numel(), int(scale_log2), _p(dst), _stream()))


def waug_set_lora_layers(table, layers, ld_w, H, dtype=BF16):
    """One launch for all LoRA layers of an encoder: ``table`` int64 [layers, 3] of device addresses (W_aug, B_q, B_v); ``dtype`` is
    the W_aug buffers' 16-bit format (fp16: BSCLIP_OPERANDS_FP16, fewer than 256 layers)."""
    _req(table.dtype == torch.int64 and table.is_contiguous() and table.is_cuda and table.numel() >= 3 * layers, "waug_set_lora_layers: table")
    _req(dtype in (BF16, F16), "waug_set_lora_layers: dtype bf16 or fp16")
    fmt = OPERANDS_FP16 if dtype == F16 else 0
    check(_l.load().bsclip_waug_set_lora_layers(_p(table), int(layers) | fmt, int(ld_w), int(H), _stream()))


def _adamw_flat_ok(p, g, m, v):
    _req(all(t.dtype == F32 and t.is_contiguous() and t.numel() == p.numel() for t in (p, g, m, v)), "adamw: flat f32 buffers")


def _adamw_hyper_ok(hyper):
    _req(hyper.element_size() == 4 and hyper.is_cuda and hyper.is_contiguous() and hyper.numel() >= 2,
         "adamw: hyper must be a device pair of 4-byte words (lr f32, step uint32)")


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _adamw_flat_ok(p, g, m, v)
    check(_l.load().bsclip_adamw_step(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2),
                                      float(eps), float(weight_decay), int(step), float(grad_scale), _stream()))


def adamw_step_dev(p, g, m, v, hyper, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    """AdamW with (lr, step) read from the device pair ``hyper`` = [lr as f32, step as uint32] when the kernel runs:
    graph-capturable (advance the step word with ``counter_add(hyper[1:2])``)."""
    _adamw_flat_ok(p, g, m, v)
    _adamw_hyper_ok(hyper)
    check(_l.load().bsclip_adamw_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), float(beta1), float(beta2),
                                          float(eps), float(weight_decay), float(grad_scale), _stream()))


GRAD_CLIP_STATE_WORDS = 12   # the device record of grad_clip_finish (include/bsclip.h): int32 [12], 16-byte aligned


def grad_norm_partials(n):
    """How many f64 partial sums ``grad_sumsq_partial`` writes for a buffer of ``n`` floats (a pure function of ``n``)."""
    count = int(_l.load().bsclip_grad_norm_partials(int(n)))
    if count < 1:
        raise ValueError(f"grad_norm_partials: n={n} must be positive")
    return count


def _grad_clip_state_ok(state, name):
    _req(state.is_cuda and state.element_size() == 4 and state.is_contiguous() and state.numel() >= GRAD_CLIP_STATE_WORDS,
         f"{name}: state must be a contiguous device record of {GRAD_CLIP_STATE_WORDS} 4-byte words")


def grad_sumsq_partial(g, partial):
    """partial[b] = sum of g[i]^2 over workgroup b's elements, in f64; ``partial`` is exactly ``grad_norm_partials(g.numel())`` long."""
    _req(g.dtype == F32 and g.is_cuda and g.is_contiguous() and g.numel() > 0, "grad_sumsq_partial: contiguous f32 GPU buffer")
    _req(partial.dtype == torch.float64 and partial.is_cuda and partial.is_contiguous() and partial.device == g.device
         and partial.numel() == grad_norm_partials(g.numel()), "grad_sumsq_partial: partial must be f64 [grad_norm_partials(n)]")
    check(_l.load().bsclip_grad_sumsq_partial(_p(g), g.numel(), _p(partial), _stream()))


def grad_clip_finish(partial, max_norm, state):
    """All partials summed in index order -> (apply, coef, norm, counters) in the device record ``state``; ``max_norm`` > 0, +inf for
    monitoring and skipping without clipping."""
    _req(partial.dtype == torch.float64 and partial.is_cuda and partial.is_contiguous() and partial.numel() > 0,
         "grad_clip_finish: partial must be a contiguous f64 GPU buffer")
    _grad_clip_state_ok(state, "grad_clip_finish")
    _req(float(max_norm) > 0.0, f"grad_clip_finish: max_norm={max_norm} must be positive")
    check(_l.load().bsclip_grad_clip_finish(_p(partial), partial.numel(), float(max_norm), _p(state), _stream()))


def counter_add_if(counter, inc, cond):
    """counter += inc when the device word ``cond`` is not zero."""
    _req(counter.is_cuda and counter.numel() >= 1 and counter.element_size() == 4, "counter: 4-byte device word")
    _req(cond.is_cuda and cond.numel() >= 1 and cond.element_size() == 4, "cond: 4-byte device word")
    check(_l.load().bsclip_counter_add_if(_p(counter), int(inc) & 0xFFFFFFFF, _p(cond), _stream()))


def adamw_step_clip(p, g, m, v, hyper, state, beta1, beta2, eps, weight_decay):
    """``adamw_step_dev`` on ``g * coef`` with ``coef`` read from ``state`` (``grad_clip_finish``); nothing is written when the record
    says skip."""
    _adamw_flat_ok(p, g, m, v)
    _adamw_hyper_ok(hyper)
    _grad_clip_state_ok(state, "adamw_step_clip")
    check(_l.load().bsclip_adamw_step_clip(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(state), float(beta1), float(beta2),
                                           float(eps), float(weight_decay), _stream()))


def _overlap(a, b):
    """True when the two contiguous tensors share a byte."""
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


def adamw_step_ema(p, g, m, v, ema, hyper, state, beta1, beta2, eps, weight_decay, ema_decay, ema_warmup):
    """``adamw_step_dev`` (``state`` None) or ``adamw_step_clip`` (``state`` the record of ``grad_clip_finish``) that also moves the
    weight average: ``ema += w * (p_new - ema)`` with ``w = 1 - d_t`` formed on the device from the step word of ``hyper`` (DESIGN.md
    4h).  Nothing is written, ``ema`` included, when the record says skip."""
    _adamw_flat_ok(p, g, m, v)
    _req(ema.dtype == F32 and ema.is_contiguous() and ema.numel() == p.numel(), "adamw_step_ema: ema must be a flat f32 buffer of p's size")
    _req(not any(_overlap(ema, t) for t in (p, g, m, v)), "adamw_step_ema: ema must not alias p, g, m or v")
    _adamw_hyper_ok(hyper)
    if state is not None:
        _grad_clip_state_ok(state, "adamw_step_ema")
    _req(0.0 < float(ema_decay) < 1.0, f"adamw_step_ema: ema_decay={ema_decay} must lie strictly inside (0, 1)")
    check(_l.load().bsclip_adamw_step_ema(_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), _p(hyper), _p(state), float(beta1),
                                          float(beta2), float(eps), float(weight_decay), float(ema_decay), int(bool(ema_warmup)),
                                          _stream()))


def swap_f32(a, b):
    """a[i] <-> b[i]: two contiguous f32 buffers of one size that share no byte."""
    _req(a.dtype == F32 and b.dtype == F32, "swap_f32: f32 buffers")
    _req(a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel() and a.numel() > 0,
         "swap_f32: contiguous buffers of the same non-zero size")
    _req(not _overlap(a, b), "swap_f32: a and b must not be the same or overlapping buffers")
    check(_l.load().bsclip_swap_f32(_p(a), _p(b), a.numel(), _stream()))


def set_dropout_step(counter):
    """Every dropout-carrying launch this thread makes from now on mixes the device word ``counter`` (uint32/int32 [1]) into
    its seed at run time (None: seeds are used as passed)."""
    if counter is not None:
        _req(counter.is_cuda and counter.numel() >= 1 and counter.element_size() == 4, "dropout step: 4-byte device word")
    check(_l.load().bsclip_set_dropout_step(_p(counter)))


def count_nonfinite(t, counter):
    """counter (int32 / uint32 device word) += the number of Inf / NaN elements of the contiguous f32 / bf16 / fp16 tensor ``t``."""
    _req(t.dtype in (F32, BF16, F16) and t.is_contiguous() and t.numel() > 0, "count_nonfinite: contiguous f32 / bf16 / fp16 tensor")
    _req(counter.dtype == torch.int32 and counter.numel() >= 1 and counter.device == t.device, "count_nonfinite: int32 device counter")
    kind = {F32: 0, BF16: 1, F16: 1 | OPERANDS_FP16}[t.dtype]
    check(_l.load().bsclip_count_nonfinite(_p(t), t.numel(), kind, _p(counter), _stream()))


def counter_add(counter, inc=1):
    _req(counter.is_cuda and counter.numel() >= 1 and counter.element_size() == 4, "counter: 4-byte device word")
    check(_l.load().bsclip_counter_add(_p(counter), int(inc) & 0xFFFFFFFF, _stream()))


def clock_probe(out32):
    """out32: zeroed int64 [32] on the GPU <- per XCD {shader-clock counter, 100 MHz real-time counter} when the current stream
    gets here (include/bsclip.h)."""
    _req(out32.is_cuda and out32.dtype == torch.int64 and out32.numel() >= 32 and out32.is_contiguous(), "clock_probe: int64 [32] on the GPU")
    check(_l.load().bsclip_clock_probe(_p(out32), _stream()))


def engine_clock_ghz(probe0, probe1):
    """Median over the XCDs of the shader clock between two clock_probe() samples, in GHz (None if no XCD gives a sane reading)."""
    a, b = probe0.cpu().view(16, 2), probe1.cpu().view(16, 2)
    ghz = []
    for x in range(16):
        dc, dt = int(b[x, 0] - a[x, 0]), int(b[x, 1] - a[x, 1])
        if a[x, 1] and b[x, 1] and dt > 0 and 0.5 < dc / (dt * 10.0) < 3.0:
            ghz.append(dc / (dt * 10.0))
    ghz.sort()
    return ghz[len(ghz) // 2] if ghz else None


def kmer_tokenize(blob, offsets, B, max_len, k, ids):
    _req(blob.dtype == torch.uint8 and blob.is_cuda and blob.is_contiguous(), "kmer_tokenize: uint8 GPU byte buffer")
    _req(offsets.dtype == torch.int64 and offsets.is_cuda and offsets.numel() == B + 1, "kmer_tokenize: offsets int64 [B+1]")
    _req(ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous() and tuple(ids.shape) == (B, max_len // k + 1),
         "kmer_tokenize: ids int64 [B, max_len/k + 1]")
    check(_l.load().bsclip_kmer_tokenize(_p(blob), _p(offsets), B, max_len, k, _p(ids), _stream()))


def augment_images(src, records, B, mid_capacity, mid, out_size, out):
    _req(src.dtype == torch.uint8 and src.is_cuda and src.is_contiguous(), "augment_images: uint8 GPU source buffer")
    _req(records.dtype == torch.int32 and records.is_cuda and records.numel() == 16 * B, "augment_images: records int32 [B,16]")
    _req(mid.dtype == F32 and mid.is_cuda and mid.numel() >= 3 * B * mid_capacity, "augment_images: mid f32 [B,3,cap]")
    _req(out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (B, 3, out_size, out_size), "augment_images: out")
    check(_l.load().bsclip_augment_images(_p(src), _p(records), B, mid_capacity, _p(mid), out_size, _p(out), _stream()))


# ------------------------------------------------------------------------------------------- JPEG shards
class JpegRefused(ValueError):
    """A stream the decoder does not take; ``code`` is the library's return code (include/bsclip.h BSCLIP_JPEG_ERR_*)."""

    def __init__(self, msg, code):
        super().__init__(msg)
        self.code = code


def _host_bytes(data):
    """(address, length, keep-alive) of ``bytes`` / a C-contiguous uint8 NumPy array (a memory-mapped slice included)."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = np.frombuffer(data, dtype=np.uint8)
    _req(data.dtype.itemsize == 1 and data.flags["C_CONTIGUOUS"], "JPEG bytes: bytes or a contiguous uint8 array")
    return ctypes.c_void_p(data.ctypes.data), data.size, data


def jpeg_probe(data):
    """Header of one JPEG stream (host only): a ``lib.JpegInfo``.  Raises ``JpegRefused`` naming the reason otherwise."""
    ptr, n, _keep = _host_bytes(data)
    info = _l.JpegInfo()
    rc = _l.load().bsclip_jpeg_probe(ptr, n, ctypes.byref(info))
    if rc != 0:
        raise JpegRefused(_l.last_error(), rc)
    return info


def jpeg_entropy_decode(src_addr, n, coef_addr, coef_capacity, qtab_addr, record_addr):
    """Huffman-decode one stream (host only, the GIL is released: loader threads call this side by side).  Plain addresses:
    coefficients int16 [coef_capacity], tables uint16 [3, 64], record int32 [16].  Raises ``JpegRefused`` on a refused, truncated or
    corrupt stream."""
    rc = _l.load().bsclip_jpeg_entropy_decode(src_addr, n, coef_addr, coef_capacity, qtab_addr, record_addr)
    if rc != 0:
        raise JpegRefused(_l.last_error(), rc)


def jpeg_pixels_workspace_bytes(coef_count):
    return int(_l.load().bsclip_jpeg_pixels_workspace_bytes(int(coef_count)))


def jpeg_pixels(coef, coef_count, qtab, records_host, records_dev, B, scratch, out):
    """B entropy-decoded images -> uint8 HWC pixels at their records' offsets in ``out``.  ``records_host`` (CPU int32 [B, 16], pinned
    for a copy that does not stall, unchanged until the stream has passed the call) is validated by the library, which then copies it
    into ``records_dev`` (GPU int32 [B, 16], scratch) in stream order: the kernels read what was checked."""
    _req(coef.dtype == torch.int16 and coef.is_cuda and coef.is_contiguous() and coef.numel() >= coef_count, "jpeg_pixels: coef int16")
    _req(qtab.dtype == torch.int16 and qtab.is_cuda and qtab.is_contiguous() and qtab.numel() % 64 == 0,
         "jpeg_pixels: qtab uint16 bits [slots, 64] held as int16")
    _req(records_host.dtype == torch.int32 and not records_host.is_cuda and records_host.is_contiguous()
         and records_host.numel() == _l.JPEG_REC * B, "jpeg_pixels: records_host CPU int32 [B,16]")
    _req(records_dev.dtype == torch.int32 and records_dev.is_cuda and records_dev.is_contiguous()
         and records_dev.numel() == _l.JPEG_REC * B, "jpeg_pixels: records_dev int32 [B,16]")
    _req(scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous(), "jpeg_pixels: scratch uint8")
    _req(out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous(), "jpeg_pixels: out uint8")
    check(_l.load().bsclip_jpeg_pixels(_p(coef), coef_count, _p(qtab), qtab.numel() // 64, _p(records_host), _p(records_dev), B,
                                       _p(scratch), scratch.numel(), _p(out), out.numel(), _stream()))


def jpeg_sync_index(data, sync_mcus):
    """The sync index of one stream (host only): int32 [entries, 4] = bit position, first MCU, Y predictor, Cb | Cr << 16 (see
    include/bsclip.h).  Raises ``JpegRefused`` on whatever the entropy decoder refuses, and on ``sync_mcus < 1``."""
    ptr, n, _keep = _host_bytes(data)
    h = _l.load()
    count = h.bsclip_jpeg_sync_index(ptr, n, int(sync_mcus), None, 0)
    if count < 0:
        raise JpegRefused(_l.last_error(), int(count))
    out = np.empty((int(count), _l.JPEG_SYNC_ENTRY), dtype=np.int32)
    rc = h.bsclip_jpeg_sync_index(ptr, n, int(sync_mcus), out.ctypes.data, int(count))
    if rc != count:
        raise JpegRefused(_l.last_error(), int(rc))
    return out


def jpeg_device_tables(src_addr, n, huff_addr, qtab_addr, record_addr):
    """Parse one stream's headers (host only; plain addresses, like ``jpeg_entropy_decode``): four device-ready Huffman tables
    (``lib.JPEG_HUFF_BYTES`` each), quantisation tables uint16 [3, 64], record int32 [16].  Raises ``JpegRefused``."""
    rc = _l.load().bsclip_jpeg_device_tables(src_addr, n, huff_addr, qtab_addr, record_addr)
    if rc != 0:
        raise JpegRefused(_l.last_error(), rc)


def jpeg_entropy_device(stream_bytes, sync, huff, records_host, segments_host, records_dev, segments_dev, B, coef, coef_count, status):
    """Huffman-decode B stored streams on the device, one lane per index segment, into the coefficient raster ``jpeg_pixels`` reads.
    ``records_host`` / ``segments_host`` (CPU int32 [B, 16] / [B, 8], unchanged until the stream has passed the call) are validated by
    the library, which then copies them into ``records_dev`` / ``segments_dev`` and zeroes ``status`` (int32 [B]) in stream order;
    afterwards ``status[b] != 0`` means image b's bytes or index are damaged."""
    _req(stream_bytes.dtype == torch.uint8 and stream_bytes.is_cuda and stream_bytes.is_contiguous(), "jpeg_entropy_device: bytes uint8")
    _req(sync.dtype == torch.int32 and sync.is_cuda and sync.is_contiguous() and sync.numel() % _l.JPEG_SYNC_ENTRY == 0,
         "jpeg_entropy_device: sync int32 [entries, 4]")
    _req(huff.dtype == torch.uint8 and huff.is_cuda and huff.is_contiguous() and huff.numel() % (4 * _l.JPEG_HUFF_BYTES) == 0,
         "jpeg_entropy_device: huff uint8 [slots, 4 * JPEG_HUFF_BYTES]")
    for t, w, nm in ((records_host, _l.JPEG_REC, "records"), (segments_host, _l.JPEG_SEG_REC, "segments")):
        _req(t.dtype == torch.int32 and not t.is_cuda and t.is_contiguous() and t.numel() == w * B, f"jpeg_entropy_device: {nm}_host CPU int32 [B,{w}]")
    for t, w, nm in ((records_dev, _l.JPEG_REC, "records"), (segments_dev, _l.JPEG_SEG_REC, "segments"), (status, 1, "status")):
        _req(t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == w * B, f"jpeg_entropy_device: {nm} GPU int32 [B,{w}]")
    _req(coef.dtype == torch.int16 and coef.is_cuda and coef.is_contiguous() and coef.numel() >= coef_count, "jpeg_entropy_device: coef int16")
    check(_l.load().bsclip_jpeg_entropy_device(_p(stream_bytes), stream_bytes.numel(), _p(sync), sync.numel() // _l.JPEG_SYNC_ENTRY, _p(huff),
                                               huff.numel() // (4 * _l.JPEG_HUFF_BYTES), _p(records_host), _p(segments_host), _p(records_dev),
                                               _p(segments_dev), B, _p(coef), coef_count, _p(status), _stream()))


# ------------------------------------------------------------------------------------------- full fine-tuning (8f-4)
def ln_param_grad(x, stats, mode, d_gamma, d_beta, g_resid=None, g_gemm=None, dt=None, lora_a=None, M=None, in_dropout=None):
    """d_gamma / d_beta += LayerNorm parameter gradients, dy assembled as layernorm_bwd does."""
    ld_x = _rowmajor(x, "x")
    H = d_gamma.numel()
    M = x.shape[0] if M is None else M
    _req(x.dtype in (F32, BF16) and x.shape[1] >= H and M <= x.shape[0], "ln_param_grad: bad x")
    _req(stats.dtype == F32 and stats.numel() >= 2 * M, "ln_param_grad: stats")
    _req(all(t.dtype == F32 and t.is_contiguous() and t.numel() == H for t in (d_gamma, d_beta)), "ln_param_grad: d_gamma/d_beta")
    ld_g = ld_gr = 0
    if g_resid is not None:
        ld_gr = _rowmajor(g_resid, "g_resid")
        _req(g_resid.dtype == F32 and g_resid.shape[0] >= M and g_resid.shape[1] >= H, "g_resid f32 [M,>=H]")
    if g_gemm is not None:
        ld_g = _rowmajor(g_gemm, "g_gemm")
        _req(g_gemm.dtype == BF16 and g_gemm.shape[0] >= M and g_gemm.shape[1] >= H, "g_gemm bf16 [M,>=H]")
    if dt is not None:
        _req(dt.dtype == F32 and dt.is_contiguous() and dt.numel() >= 8 * M, "dt f32 [M,8]")
        _f32_shaped(lora_a, (8, H), "lora_a")
    ws = _stream_ws(("ln_param_grad", H), x.device, _l.load().bsclip_ln_param_grad_workspace_floats(H))
    dp, ds = _drop(in_dropout)
    check(_l.load().bsclip_ln_param_grad(_p(x), ld_x, int(x.dtype == BF16), _p(stats), M, H, _p(g_resid), ld_gr, _p(g_gemm), ld_g,
                                         _p(dt), _p(lora_a) if dt is not None else None, int(mode), dp, ds, _p(d_gamma),
                                         _p(d_beta), _p(ws), _stream()))


def embed_grad(ids, type_ids, d_emb, d_word, d_pos, d_type, pad_id=0):
    B, S = ids.shape
    H = d_word.shape[1]
    _req(ids.dtype == torch.int64 and ids.is_contiguous(), "embed_grad: ids int64 [B,S]")
    _req(type_ids is None or (type_ids.dtype == torch.int64 and type_ids.is_contiguous() and type_ids.shape == ids.shape), "type_ids")
    _req(d_emb.dtype == F32 and d_emb.is_contiguous() and d_emb.shape[0] >= B * S and d_emb.shape[1] == H, "d_emb f32 [B*S,H]")
    _req(all(t.dtype == F32 and t.is_contiguous() and t.shape[1] == H for t in (d_word, d_pos, d_type)) and d_pos.shape[0] >= S
         and d_type.shape[0] >= 2, "embed_grad: gradient tables f32 [*,H]")
    ws = _stream_ws(("embed_grad", H), d_emb.device, _l.load().bsclip_embed_grad_workspace_floats(H))
    check(_l.load().bsclip_embed_grad(_p(ids), _p(type_ids), B, S, H, d_word.shape[0], int(pad_id), _p(d_emb), _p(d_word),
                                      _p(d_pos), _p(d_type), _p(ws), _stream()))


def gemm_splitk_f32(a, b, c, splits, partial, K=None):
    """c[M, N] (f32) += a[M, K] . b[N, K]^T, reduction cut into ``splits`` K ranges (weight gradients of full fine-tuning)."""
    M, N = c.shape
    K = a.shape[1] if K is None else K
    lda, ldb, ldc = _rowmajor(a, "a"), _rowmajor(b, "b"), _rowmajor(c, "c")
    _req(a.dtype == BF16 and b.dtype == BF16 and c.dtype == F32 and partial.dtype == F32 and partial.is_contiguous(), "gemm_splitk_f32 dtypes")
    _req(a.shape[0] >= M and b.shape[0] >= N and a.shape[1] >= K and b.shape[1] >= K, "gemm_splitk_f32: operand shapes")
    _req(N % 256 == 0 and splits >= 1 and K % (64 * splits) == 0, "gemm_splitk_f32: N % 256 == 0, K % (64 * splits) == 0")
    _req(partial.numel() >= splits * M * N, "gemm_splitk_f32: partial needs splits * M * N floats")
    check(_l.load().bsclip_gemm_splitk_f32(_p(a), lda, _p(b), ldb, _p(c), ldc, M, N, K, int(splits), _p(partial), _stream()))


def gather_cast_rows(src, rows_out, period_in, period_out, offset, dst):
    H = src.shape[1]
    _req(src.dtype == F32 and dst.dtype == BF16 and dst.shape[0] >= rows_out and dst.shape[1] >= H, "gather_cast_rows dtypes/shapes")
    n_in = (rows_out + period_out - 1) // period_out * period_in
    _req(src.shape[0] >= n_in - (period_in - offset - period_out), "gather_cast_rows: src too small")
    check(_l.load().bsclip_gather_cast_rows(_p(src), _rowmajor(src, "src"), rows_out, period_in, period_out, offset, H, _p(dst),
                                            _rowmajor(dst, "dst"), _stream()))
