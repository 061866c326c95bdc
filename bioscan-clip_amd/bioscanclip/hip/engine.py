"""Host-side orchestration of the HIP kernels for the three encoders (forward + hand-written backward).

Everything numerical happens in ``libbsclip_hip.so``; this file decides *which* kernel runs on *which* buffer:
  * frozen backbone weights are packed once into bf16 [N,K] operands (plus the transposed copy the dX GEMMs
    need -- HBM is 288 GB, the extra 0.35 GB buys a single NT GEMM kernel for forward and backward);
  * trainable tensors (LoRA A/B, heads) are re-homed into one flat f32 buffer per encoder (``FlatParams``) whose
    layout is exactly what the kernels consume (``lora_a[8,H]``, ``lora_b[2,H,4]`` per layer), with a twin flat
    gradient buffer that ``p.grad`` aliases -- kernels accumulate straight into it and the fused AdamW kernel
    updates the whole buffer in one launch;
  * activations needed by backward live in a per-batch-size workspace sized for HBM (f32 residual stream saved per
    sub-layer, bf16 GEMM operands, attention LSE, LN statistics).
Reference call shapes: SURVEY.md 2.3 (K1-K15), 3.2; semantics App. A.1-A.3.
"""
import itertools
import os
import zlib
from collections import namedtuple

import torch

from . import ops
from .lib import (EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_GELU_FP8, EPI_PATCH_BF16, EPI_PATCH_F32, EPI_RESID_BF16,
                  EPI_RESID_F32, KPAD)

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
# The six switches below (set_parity_mode assigns three of them) are the REQUEST: how the next engine should run.  No engine reads
# them: it is built for one EngineMode -- wanted_mode(module): these switches and the module's hip_* attributes -- and keeps it as
# ``engine.mode``.  _engine_for compares request and engine at every forward and rebuilds the engine when they differ; the flat
# parameter / gradient buffer (FlatParams) of the old engine goes to the new one.
# Residual-GRADIENT stream dtype of the LoRA-regime backward (the gradient that flows down the skip connections, read and
# written by every LayerNorm backward): "bf16" halves its bytes (LN backward is HBM-bound: 16 -> 10-12 bytes per element);
# the forward and the parameter gradients' f32 accumulation are unchanged.  "f32" restores round 2's behaviour.  Full
# fine-tuning keeps f32 (its LayerNorm parameter gradients read the same stream).
GRAD_STREAM_BF16 = os.environ.get("BSCLIP_GRAD_STREAM", "bf16").lower() != "f32"
# Residual stream dtype of the FORWARD (the tensor every sub-layer adds its output to; saved per sub-layer as the LayerNorm
# backward's input).  "bf16": each sum is formed in f32 in the GEMM epilogue and rounded once on the way to HBM; the
# out-projection / fc2 epilogues move 4 instead of 8 bytes per element, LayerNorm forward reads 2 instead of 4 (BERT: writes no
# f32 copy either), LayerNorm backward reads 2 instead of 4, and the saved stream halves (3.9 -> 2.0 GB for the ViT at B = 256).
# Cost, measured on the CPU oracle at depth 12: the distance to the f32 reference grows by ~10 % (2.5e-2 -> 2.8e-2),
# the gradients' not at all.  "f32" restores round 2's stream.  Full fine-tuning and fp8 trunks keep f32.
RESID_STREAM_BF16 = os.environ.get("BSCLIP_RESID_STREAM", "bf16").lower() != "f32"
# Patch embedding on split-bf16 operands (hi.hi + lo.hi + hi.lo in one K = 2304 GEMM): the first GEMM's operand rounding is the
# one every block amplifies -- exact to ~2^-16 it takes the ViT's distance to the f32 reference at depth 12 from 2.5e-2 to
# 1.7e-2 on the CPU emulation, for +0.8 % of the ViT's forward FLOPs.  "0" restores the plain bf16 GEMM.
PATCH_SPLIT = os.environ.get("BSCLIP_PATCH_SPLIT", "1") != "0"
# Attention-probs dropout (BERT towers, train mode): the forward kernel leaves its keep decisions as bit words, the backward reads them
# instead of re-hashing (csrc/attn_common.h KEEP_WORDS).  "0" = re-hash in the backward (round 4's form; identical masks and gradients).
ATTN_KEEP_BITS = os.environ.get("BSCLIP_ATTN_KEEP_BITS", "1") != "0"
# LoRA gradients: the attention backward leaves dt = dq B_q | dv B_v and dB = (dq | dv)^T t as per-head / per-sequence partial sums taken
# from its accumulators (csrc/attn.hip LoraPart), bsclip_lora_grad_heads reduces them -- instead of bsclip_lora_grad's pass that reads dq
# and dv back from HBM.  "0" = that pass (round 4's form; the same sums up to f32 accumulation order).
ATTN_LORA = os.environ.get("BSCLIP_ATTN_LORA", "1") != "0"


# BSCLIP_PARITY=1 / set_parity_mode(1): f32 residual stream, f32 residual-gradient stream, split-bf16 patch embedding -- at the
# price bench.py reports as `parity_mode_ms_per_step`.  NOT north_star's 1e-3: every trunk GEMM and the attention products still
# take bf16 operands.
# BSCLIP_PARITY=2 / set_parity_mode(2): the EXACT mode (round 4, csrc/exact.hip) -- every GEMM of the forward and of the backward
# on split-bf16 operands (hi + lo, K tripled: exact to ~2^-16 on the bf16 matrix cores), LoRA folded into the weight in f32,
# exact-erf GELU, every attention product on split operands too (round 5, csrc/attn_x3.hip: f32 in / out, f32 softmax arithmetic), f32
# LoRA gradients, f32 streams; the LayerNorm and attention kernels write the next GEMM's split operand themselves.  Embeddings, loss
# and every gradient within 1e-3 of the f32 reference at depth 12 (measured <= 1.6e-4, tests/test_20_encoders_gpu.py).
# LoRA-regime ViT / BERT engines only (fp8 and full fine-tuning keep their own paths, on the f32 streams).
EXACT_FORWARD = False
if os.environ.get("BSCLIP_PARITY", "0") in ("1", "2"):
    GRAD_STREAM_BF16 = RESID_STREAM_BF16 = False
    PATCH_SPLIT = True
    EXACT_FORWARD = os.environ.get("BSCLIP_PARITY") == "2"


# Everything that shapes an engine: the six switches above, then the module's own requests (set_precision, set_operand_format, hip_full_ft)
EngineMode = namedtuple("EngineMode", "grad_stream_bf16 resid_stream_bf16 patch_split exact attn_keep_bits attn_lora fp8 fp16 full_ft")


def wanted_mode(module):
    """The mode an engine of encoder ``module`` should have now."""
    return EngineMode(GRAD_STREAM_BF16, RESID_STREAM_BF16, PATCH_SPLIT, EXACT_FORWARD, ATTN_KEEP_BITS, ATTN_LORA,
                      wants_fp8(module), wants_fp16(module), wants_full_ft(module))


def set_parity_mode(on, model=None):
    """Change the request at run time: 0 / False = default, 1 / True = f32 streams, 2 = the exact mode (f32 streams + the exact
    forward and backward, csrc/exact.hip).  An encoder whose engine was built for another mode gets a new engine at its next forward,
    with or without ``model``; the flat parameter / gradient buffer carries over.  ``model``: drop its engines now.  Returns the previous
    (grad_stream_bf16, resid_stream_bf16) pair (restore with the module attributes; EXACT_FORWARD is reset by passing 0 / 1)."""
    global GRAD_STREAM_BF16, RESID_STREAM_BF16, EXACT_FORWARD
    prev = (GRAD_STREAM_BF16, RESID_STREAM_BF16)
    level = int(on)
    GRAD_STREAM_BF16 = RESID_STREAM_BF16 = level == 0
    EXACT_FORWARD = level == 2
    for m in model.modules() if model is not None else ():
        if getattr(m, "_engine", None) is not None:
            _park_engine(m)
    return prev


# BSCLIP_DETECT_ANOMALY=1 / set_detect_anomaly(True): this build's counterpart of ``torch.autograd.set_detect_anomaly(True)``, which
# the reference loop switches on in every epoch (train_epoch.py:12).  Every encoder forward / backward is followed by a device-side
# count of Inf / NaN values (bsclip_count_nonfinite) in its output / its flat gradient buffer, read back at once; on a hit the
# per-layer activations are probed in execution order and a RuntimeError names the first tensor that holds non-finite values (the
# reference's anomaly mode names the autograd node).  A debugging aid: it synchronises the host after every tower, so the step
# stays eager (train_epoch skips the captured-graph path) -- off by default, as SURVEY App. B-6 decides for timed runs.
DETECT_ANOMALY = os.environ.get("BSCLIP_DETECT_ANOMALY", "0") == "1"


def set_detect_anomaly(on):
    global DETECT_ANOMALY
    prev, DETECT_ANOMALY = DETECT_ANOMALY, bool(on)
    return prev


def count_nonfinite(t):
    """Number of Inf / NaN elements of an f32 / bf16 device tensor (host-synchronising: a debugging aid)."""
    c = torch.zeros(1, dtype=torch.int32, device=t.device)
    ops.count_nonfinite(t.contiguous(), c)
    return int(c.item())


def _anomaly_check(engine, phase, out=None):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("BSCLIP_DETECT_ANOMALY reads every tower's result back to the host: it cannot run inside a hipGraph "
                           "capture (train_epoch takes the eager path when it is on)")
    who = type(engine).__name__
    if phase == "forward":
        if count_nonfinite(out) == 0:
            return
        for name, t in engine.anomaly_probes():
            if count_nonfinite(t):
                raise RuntimeError(f"{who} forward: non-finite values first appear in {name} (BSCLIP_DETECT_ANOMALY)")
        raise RuntimeError(f"{who} forward: non-finite values in the encoder output (BSCLIP_DETECT_ANOMALY)")
    # the fp16 backward's scaled gradient stream: an overflow there is the finding, whether or not it reached .grad
    for name, t in engine.backward_probes():
        if count_nonfinite(t):
            raise RuntimeError(f"{who} backward: non-finite values in {name} (fp16 gradient scale 2^{engine.FP16_GRAD_SCALE_LOG2}; "
                                   "BSCLIP_DETECT_ANOMALY)")
    if count_nonfinite(engine.flat.grad) == 0:
        return
    names = {id(p): n for n, p in engine._owner.named_parameters()} if engine._owner is not None else {}
    bad = [names.get(id(p), f"trainable tensor #{i}") for i, p in enumerate(engine.flat.params)
           if p.grad is not None and count_nonfinite(p.grad)]
    raise RuntimeError(f"{who} backward: non-finite gradient values in {', '.join(bad[:6])}"
                       f"{' ...' if len(bad) > 6 else ''} (BSCLIP_DETECT_ANOMALY)")


_WS_GEN = itertools.count(1)   # every workspace gets a unique, never reused number (hip/graph.py keys captured graphs on it)


def _bf16(w, dev):
    return w.detach().to(dev, F32).to(BF16).contiguous()


def _f32(w, dev):
    return w.detach().to(dev, F32).contiguous()


def split_plan(M, N, K):
    """(splits, padded reduction length) for a weight gradient dW[N, K] = dY^T X reduced over M rows (bsclip_gemm_splitk_f32): as
    many K ranges as bring the launch to about two rounds of the 256 CUs, each at least four 64-wide K-tiles long.  The output
    is 9 .. 36 tiles of 256 x 256; one workgroup per tile would leave most of the chip idle for the whole reduction."""
    tiles = -(-N // 256) * (K // 256)
    if K % 256 or tiles >= 192 or M < 512:
        return 1, _pad64(M)
    S = max(1, min(512 // tiles, M // 256))
    unit = 64 * S
    return S, -(-M // unit) * unit


def _pad64(n):
    return (n + 63) // 64 * 64


def tok0(t, B):
    """Token 0 of every image: rows 0, S, 2S, ... of a [B * S, w] tensor as a [B, w] view (row stride S * w)."""
    return t.view(B, -1)[:, :t.shape[1]]


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class FlatParams:
    """Contiguous f32 home for a list of trainable parameters and their gradients."""

    def __init__(self, params, device):
        self.params = list(params)
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.offsets = offs
        self.data = torch.zeros(total, dtype=F32, device=device)
        self.grad = torch.zeros(total, dtype=F32, device=device)
        for p, o in zip(self.params, offs):
            view = self.data[o:o + p.numel()].view(p.shape)
            view.copy_(p.data.to(device, F32))
            p.data = view
        self.bind_grads(force=True)

    def view(self, p_index, shape=None, n=None, grad=False):
        o = self.offsets[p_index]
        buf = self.grad if grad else self.data
        n = self.params[p_index].numel() if n is None else n
        t = buf[o:o + n]
        return t.view(shape) if shape is not None else t

    def valid(self):
        return all(p.data.data_ptr() == self.data.data_ptr() + 4 * o and p.data.device == self.data.device
                   for p, o in zip(self.params, self.offsets))

    def bind_grads(self, force=False):
        """Make every ``p.grad`` alias the flat gradient buffer.  If autograd/optimizer dropped the grads
        (``zero_grad(set_to_none=True)``) the buffer is cleared first, so accumulate-into-grad stays correct."""
        ok = [p.grad is not None and p.grad.data_ptr() == self.grad.data_ptr() + 4 * o
              for p, o in zip(self.params, self.offsets)]
        if all(ok) and not force:
            return
        if not any(ok):
            self.grad.zero_()
        for p, o, good in zip(self.params, self.offsets, ok):
            if not good:
                p.grad = self.grad[o:o + p.numel()].view(p.shape)


def _pack_qkv(w_qkv, b_qkv, H, dev, h16=BF16, transposed=True):
    """W_aug [3H, H+KPAD] (LoRA-B columns refreshed every step) and W^T [H, 3H] for dX, both in the 16-bit format h16.  An engine
    that runs no backward (the fp16 BERT engines) gets no transposed copy (transposed=False: None)."""
    w = w_qkv.detach().to(dev, F32)
    waug = torch.zeros(3 * H, H + KPAD, dtype=h16, device=dev)
    waug[:, :H] = w.to(h16)
    return waug, w.t().contiguous().to(h16) if transposed else None, _f32(b_qkv, dev)


def _pack_linear(lin, dev, h16=BF16, transposed=True):
    w = lin.weight.detach().to(dev, F32)
    return w.to(h16).contiguous(), w.t().contiguous().to(h16) if transposed else None, _f32(lin.bias, dev)


class _Layer:
    def __init__(self):   # one block's packed weights; the exact mode's split copies are made by its first forward / backward
        self.qkv32 = self.wqkv3 = self.w3 = self.w3t = self.wqkvT3 = None


# What the sequences of one ViT block work on below the attention (ViTEngine._workspace makes one per block).  Blocks 0 .. L-2: all
# B * 197 rows.  The last block: the B token-0 rows, as views of row stride S * w (tok0) of the same stream buffers -- the head reads
# token 0 only (timm global_pool='token') and within a block a token depends on the others through K and V alone, so attention runs
# for query 0 and the out-projection, LayerNorm 2 and the MLP, forward and backward, do 1/197 of the work for the same values.
#   M, q_rows        row count, and the attention kernels' query-rows flag (1 = query 0 only)
#   x                the residual stream before the block, after attention, after the MLP
#   ctx, h2, act     operands of the out-projection, fc1 and fc2 (exact mode: ctx in f32; full fine-tuning: h2 / act kept per block)
#   z, st2           gelu' codes (exact mode: the f32 fc1 pre-activation), LayerNorm-2 statistics
#   mlp8             the MLP runs on fp8 operands
#   split            exact mode: the attention and LayerNorm kernels write the next GEMM's split operand themselves (else a
#                    split3_rows pass over the f32 rows does)
#   g, dxb           the residual-gradient stream and the dX GEMMs' 16-bit operand
#   dz, dh, dctx     outputs of the fc2, fc1 and out-projection dX GEMMs; zero: the whole dctx buffer where dctx covers only some of
#                    the rows the attention backward reads, so that it must be cleared first (else None)
_Rows = namedtuple("_Rows", "M q_rows x ctx h2 act z st2 mlp8 split g dxb dz dh dctx zero")


class EncoderEngineBase:
    """Shared pieces of the ViT and BERT engines: the mode, LoRA bookkeeping and the flat trainable buffer."""

    def __init__(self, mode, device):
        self.mode, self.device = mode, device
        self.full_ft = mode.full_ft
        self.fp8 = mode.fp8 and not mode.full_ft     # full fine-tuning has no fp8 path
        # what the request comes to in this engine: full fine-tuning and fp8 trunks keep the f32 residual stream, full fine-tuning the
        # f32 gradient stream too; the exact mode is the LoRA-regime engines' alone
        self.resid_bf16 = mode.resid_stream_bf16 and not mode.full_ft and not self.fp8
        self.grad_bf16 = mode.grad_stream_bf16 and not mode.full_ft
        self._exact = mode.exact and not self.fp8 and not mode.full_ft
        # fp16 operands: every frozen weight, the head weight's per-forward cast and the workspace's 16-bit buffers are IEEE fp16, the
        # kernels get BSCLIP_OPERANDS_FP16.  The ViT trains on them; the BERT engines are inference-only.
        self.fp16, self.h16 = mode.fp16, F16 if mode.fp16 else BF16
        self.ws = None
        # run_encoder: the owning module, its train / eval state, a count of forwards (_EncoderFn.backward checks that the saved
        # activations are still its own); _engine_for: what the packed frozen weights were made from
        self._owner, self.training, self._fwd_generation, self._frozen_sig = None, False, 0, None
        self._waug_table = None        # refresh_lora_weights: device addresses of the K-augmentation columns, made at the first call
        self._step_word = None         # BERT dropout: the device step counter, made by the first training-mode forward
        self.w_tr3 = self.w_tr3t = None   # exact mode, MLM head: the transform weight's split and transposed split

    def _setup_lora(self, qv_modules, H, dev, extra_params, reuse_flat):
        """qv_modules: per layer either None (no LoRA) or (A_q, A_v, B_q, B_v) nn.Linear modules.  reuse_flat: the replaced engine's flat buffer, or None."""
        params = []
        self._lora_index = []
        for mods in qv_modules:
            if mods is None:
                self._lora_index.append(None)
                continue
            self._lora_index.append(len(params))
            params += [mods[0].weight, mods[1].weight, mods[2].weight, mods[3].weight]
        self._extra_index = len(params)
        params += list(extra_params)
        self._trunk_index = len(params)
        params += list(self._trunk_trainables())   # full fine-tuning (hip/engine_ft.py): every trunk tensor, in its order
        ops.init_tables()
        if (reuse_flat is not None and len(reuse_flat.params) == len(params) and all(p is q for p, q in zip(reuse_flat.params, params))
                and reuse_flat.data.device.type == torch.device(dev).type and torch.device(dev).index in (None, reuse_flat.data.device.index)):
            self.flat = reuse_flat   # an engine rebuilt for another mode / frozen weights keeps the trained values and .grad
        else:
            self.flat = FlatParams(params, dev)
        self._zero_a = torch.zeros(8, H, dtype=F32, device=dev)

    def _trunk_trainables(self):
        return []

    def lora_a(self, l, grad=False):
        i = self._lora_index[l]
        if i is None:
            return None if grad else self._zero_a
        return self.flat.view(i, (8, self.H), n=8 * self.H, grad=grad)

    def lora_b(self, l, grad=False):
        i = self._lora_index[l]
        if i is None:
            return None
        return self.flat.view(i + 2, (2, self.H, 4), n=8 * self.H, grad=grad)

    def extra(self, k, grad=False):
        return self.flat.view(self._extra_index + k, self.flat.params[self._extra_index + k].shape, grad=grad)

    def refresh_lora_weights(self):
        """LoRA-B into the K-augmentation columns of every layer's QKV weight: one launch over a table of device addresses (the
        weights and the flat parameter buffer live as long as the engine)."""
        if self._waug_table is None:
            rows = [(lay.waug.data_ptr(), self.lora_b(l)[0].data_ptr(), self.lora_b(l)[1].data_ptr())
                    for l, lay in enumerate(self.layers) if self.lora_b(l) is not None]
            lds = {_lay.waug.stride(0) for _lay in self.layers}
            assert len(lds) == 1
            self._waug_table = (torch.tensor(rows, dtype=torch.int64, device=self.device).reshape(-1, 3).contiguous(), len(rows), lds.pop())
        table, n, ld_w = self._waug_table
        if n:
            ops.waug_set_lora_layers(table, n, ld_w, self.H, dtype=self.h16)
        if self.fp8:  # LoRA-B columns of the bf16 K-augmentation tile, in the fp8 accumulator's units
            for l, lay in enumerate(self.layers):
                b = self.lora_b(l)
                if b is not None:
                    ops.lora_baug_set(lay.baug, self.H, b[0], b[1], lay.s_qkv)

    def _lora_grads(self, l, ws, h_aug, h_fp8, part, grad_scale_log2=None):
        """dA / dB of layer l's LoRA pair, and dt for the LayerNorm backward below it, from ws["dqkv"].  ``h_aug``: the QKV GEMM's
        operand (LayerNorm output | t); ``h_fp8``: its fp8 form (fp8 engines); ``part``: attn_bwd left the partial sums."""
        lb = self.lora_b(l)
        if lb is None:
            return
        M, H = ws["M"], self.H
        dA, dB = self.lora_a(l, grad=True), self.lora_b(l, grad=True)
        if self.fp8:
            ops.lora_grad_fp8(ws["dqkv"], h_fp8, ws["t"][l], M, H, lb, ws["dt"], dA, dB[0], dB[1])
        elif part:
            ops.lora_grad_heads(h_aug, M, H, ws["B"], ws["dtp"], ws["dbp"], ws["dt"], dA, dB[0], dB[1],
                                grad_scale_log2=grad_scale_log2)
        else:
            ops.lora_grad(ws["dqkv"], h_aug, M, H, lb, ws["dt"], dA, dB[0], dB[1])

    # What full fine-tuning adds to the backward sequences (hip/engine_ft.py implements them): nothing here, where only the LoRA
    # pairs and the heads are trained.  Their arguments are evaluated in both regimes: no FT-only workspace entry among them.
    def _dw(self, dY, X, M, N, K, wname, bname, w_n=None):
        """Weight and bias gradient of a Linear; called in front of the dX GEMM that reads the same dY."""

    def _ln_dw(self, x, stats, mode, wname, bname, **grads):
        """Gain and bias gradient of a LayerNorm; called in front of its layernorm_bwd."""

    def _below_layer0(self, ws, *grads):
        """The embeddings' gradients, once the chain has passed layer 0."""

    def _extend_workspace(self, ws):
        """What a subclass adds to a workspace that ``_workspace`` has just built (hip/engine_ft.py); nothing here."""

    def _keep_workspace(self, ws):
        self._extend_workspace(ws)
        self.ws = ws
        return ws

    def backward_probes(self):
        """(name, tensor) of the fp16 backward's gradient buffers (BSCLIP_DETECT_ANOMALY); none unless the engine has that backward."""
        return ()

    # Static gradient scale of the fp16 backward (part 3a; profiles/r08_fp16_vit_training.jsonl): dL/dz of the head is
    # multiplied by 2^s where it becomes the fp16 dout, so the whole gradient stream lives 2^s up, clear of fp16's subnormals; each
    # trainable gradient is brought back by 2^-s (exact) before it is added into .grad.  s is the largest that leaves the largest
    # scaled |gradient| of any site >= 2^4 under 65 504 at unit-sized cotangents (tests/test_20's: 1627 at s = 13, so 3254 at s = 14);
    # a B = 256 InfoNCE step's cotangents are ~2^8 smaller (largest 6.9 at s = 13), and a share of its smallest values is subnormal.
    FP16_GRAD_SCALE_LOG2 = 14

    def _head_backward(self, ws, dout, pooled, pooled_t, dx, dx_epi):
        """Backward of the trainable linear head out = pooled W^T + b over the B pooled rows: dW += dout^T pooled, db += colsum(dout),
        dx = dout W through ``dx_epi``.  fp16: dout enters 2^s up, dW leaves the scale in ``gw_head``; db is summed from the f32 dout."""
        B, N, K = ws["B"], self.out_dim, self.head_in
        gw = self.extra(0, grad=True)
        if self.fp16:
            ops.cast_f32_f16_scaled(dout, ws["dout_bf"], self.FP16_GRAD_SCALE_LOG2)
        else:
            ops.cast_f32_bf16(dout, ws["dout_bf"])
        ops.transpose_bf16(ws["dout_bf"], B, N, ws["dout_t"])
        ops.transpose_bf16(pooled, B, K, pooled_t)
        if self.fp16:
            ops.gemm(ws["dout_t"], pooled_t, ws["gw_head"], EPI_F32)
            ops.add_scaled_f32(ws["gw_head"], gw, -self.FP16_GRAD_SCALE_LOG2)
        else:
            ops.gemm(ws["dout_t"], pooled_t, gw, EPI_RESID_F32, resid=gw)
        ops.colsum(dout, B, N, self.extra(1, grad=True))
        ops.transpose_bf16(self.w_head_bf, N, K, self.w_head_t)
        ops.gemm(ws["dout_bf"], self.w_head_t, dx, dx_epi)

    def _no_fp16_backward(self):
        if self.fp16:
            raise RuntimeError(f"{type(self).__name__}: the fp16-operand engines are inference-only (the fp16 backward is not built "
                               "yet): run the encoder under eval() and torch.no_grad(), or set_operand_format(model, 'bf16')")

    # ------------------------------------------------------------------------------ exact mode (BSCLIP_PARITY=2)
    def exact(self):
        return self._exact

    def _ex_weight(self, w_f32, lora=None):
        """[hi | hi | lo] rows of a frozen f32 weight (LoRA folded in f32 when given: refreshed by the caller every step)."""
        w = w_f32.detach().to(self.device, F32).contiguous()
        dst = torch.empty(w.shape[0], 3 * w.shape[1], dtype=BF16, device=self.device)
        if lora is None:
            ops.split3_weight(w, dst)
        return w, dst

    def _ex_gemm(self, a_f32, w3, out, epi, scratch, M=None, presplit=False, **kw):
        """out = epilogue(a_f32 @ W^T) with both operands split: a_f32 f32 [M, K] (row stride free) -> [hi | lo | hi] in ``scratch``.
        ``presplit``: the kernel that produced a_f32 wrote that split into ``scratch`` itself (see _ex_gemm3): no split3_rows pass."""
        M = a_f32.shape[0] if M is None else M
        K = w3.shape[1] // 3
        if presplit:
            return self._ex_gemm3(scratch, w3, out, epi, M, **kw)
        a3 = ops.split3_rows(a_f32, scratch, M=M, K=K)
        return ops.gemm(a3, w3, out, epi, M=M, K=3 * K, **kw)

    def _ex_gemm3(self, a3, w3, out, epi, M, **kw):
        """The same with the A operand already split: ``a3`` bf16 [>= M, >= 3K] = [hi | lo | hi], written by the producer itself (the
        LayerNorm kernels' y_split3 / dx_split3 outputs, round 5) instead of a stand-alone split3_rows pass over an f32 tensor."""
        K = w3.shape[1] // 3
        return ops.gemm(a3[:M, :3 * K], w3, out, epi, M=M, K=3 * K, **kw)

    def _ex_weight_t(self, w_f32):
        """[hi | hi | lo] rows of the TRANSPOSE of a frozen f32 weight [N, K] -> bf16 [K, 3N]: the B operand of its dX GEMM."""
        w = w_f32.detach().to(self.device, F32).contiguous()
        N, K = w.shape
        assert N % 64 == 0
        return ops.split3_transpose(w, torch.empty(K * 3 * N, dtype=BF16, device=self.device), 1)

    def _ex_dw(self, dy, x, gw, ws, M=None):
        """gw[N, K] += dy[M, N]^T x[M, K], f32 operands split along the reduction (the M rows, zero-padded to a multiple of 64)."""
        M = dy.shape[0] if M is None else M
        a = ops.split3_transpose(dy, ws["t3a"], 0, R=M)
        b = ops.split3_transpose(x, ws["t3b"], 1, R=M)
        ops.gemm(a, b, gw, EPI_RESID_F32, resid=gw)

    def _ex_forward_weights(self):
        """Split weights of the frozen Linears (once) and the f32 QKV master whose LoRA-folded split is refilled every step."""
        for lay in self.layers:
            if lay.w3 is None:
                lay.qkv32, lay.wqkv3 = self._ex_weight(lay.src[0], lora=True)
                lay.w3 = [self._ex_weight(w)[1] for w in lay.src[1:]]   # ViT: proj, fc1, fc2; BERT: attention output, intermediate, output

    def _ex_backward_weights(self):
        """Transposed split weights of the frozen Linears (once) and the buffer of the LoRA-folded QKV transpose (refilled every step)."""
        for lay in self.layers:
            if lay.w3t is None:
                lay.w3t = [self._ex_weight_t(w) for w in lay.src[1:]]
                lay.wqkvT3 = torch.empty(self.H * 9 * self.H, dtype=BF16, device=self.device)

    def _pack_fp8(self, lay, w_qkv, w_fc1, w_fc2, dev):
        """BASELINE configs[4]: the frozen QKV / fc1 / fc2 weights as OCP fp8 e4m3 with one scale per output row (row amax
        -> 448); activations are quantised with scale 1 by their producers (LayerNorm, GELU epilogue), so a GEMM's
        dequantisation vector alpha is the weight-row scale itself.  LoRA, attention, out-projection, heads, loss and the
        whole backward stay in bf16 / f32."""
        lay.w_qkv8, lay.s_qkv = ops.quantize_rows_fp8(_f32(w_qkv, dev))
        lay.w_fc1_8, lay.s_fc1 = ops.quantize_rows_fp8(_f32(w_fc1, dev))
        lay.w_fc2_8, lay.s_fc2 = ops.quantize_rows_fp8(_f32(w_fc2, dev))
        lay.baug = torch.zeros(3 * self.H, KPAD, dtype=BF16, device=dev)


# ======================================================================================================== ViT
class ViTEngine(EncoderEngineBase):
    """LoRA ViT-B/16 forward/backward (reference image_encoder.py:15-109 over timm vit_base_patch16_224)."""

    def __init__(self, module, device, mode, reuse_flat=None):
        super().__init__(mode, device)
        vit = module.lora_vit
        h16, dev = self.h16, device
        self.H = H = vit.blocks[0].norm1.weight.numel()
        self.heads = vit.blocks[0].attn.num_heads
        self.S = vit.pos_embed.shape[1]
        assert H == 768 and self.S == 197 and vit.patch_embed.proj.weight.shape[-1] == 16, \
            "HIP ViT engine is built for vit_base_patch16_224"
        self.w_patch = vit.patch_embed.proj.weight.detach().reshape(H, -1).to(dev, F32).to(h16).contiguous()
        # split-bf16 patch embedding (mode.patch_split): the weight as [hi | hi | lo] against im2col rows [hi | lo | hi] (fp16 parts in fp16 mode)
        w32 = vit.patch_embed.proj.weight.detach().reshape(H, -1).to(dev, F32)
        w_hi = w32.to(h16)
        self.w_patch3 = torch.cat([w_hi, w_hi, (w32 - w_hi.to(F32)).to(h16)], dim=1).contiguous()
        self.b_patch = _f32(vit.patch_embed.proj.bias, dev)
        self.cls = _f32(vit.cls_token.reshape(-1), dev)
        self.pos = _f32(vit.pos_embed.reshape(self.S, H), dev)
        self.layers, qv = [], []
        for blk in vit.blocks:
            lay = _Layer()
            q = blk.attn.qkv
            if hasattr(q, "linear_a_q"):
                base = q.qkv
                qv.append((q.linear_a_q, q.linear_a_v, q.linear_b_q, q.linear_b_v))
            else:
                base = q
                qv.append(None)
            # the transposed weights of the dX GEMMs in the operand format (the fp16 ViT trains too)
            lay.waug, lay.wqkv_t, lay.b_qkv = _pack_qkv(base.weight, base.bias, H, dev, h16)
            lay.src = (base.weight, blk.attn.proj.weight, blk.mlp.fc1.weight, blk.mlp.fc2.weight)   # f32 masters (exact forward)
            lay.ln1 = (_f32(blk.norm1.weight, dev), _f32(blk.norm1.bias, dev))
            lay.ln2 = (_f32(blk.norm2.weight, dev), _f32(blk.norm2.bias, dev))
            lay.w_proj, lay.w_proj_t, lay.b_proj = _pack_linear(blk.attn.proj, dev, h16)
            lay.w_fc1, lay.w_fc1_t, lay.b_fc1 = _pack_linear(blk.mlp.fc1, dev, h16)
            lay.w_fc2, lay.w_fc2_t, lay.b_fc2 = _pack_linear(blk.mlp.fc2, dev, h16)
            if self.fp8:
                self._pack_fp8(lay, base.weight, blk.mlp.fc1.weight, blk.mlp.fc2.weight, dev)
            self.layers.append(lay)
        self.ln_f = (_f32(vit.norm.weight, dev), _f32(vit.norm.bias, dev))
        self.FF = self.layers[0].w_fc1.shape[0]
        self.out_dim, self.head_in = vit.head.weight.shape
        assert self.out_dim % 128 == 0, "head width must be a multiple of 128 for the HIP GEMM"
        self._setup_lora(qv, H, dev, [vit.head.weight, vit.head.bias], reuse_flat)
        self.w_head_bf = torch.empty(self.out_dim, H, dtype=h16, device=dev)     # the head weight in the operand format, cast every forward
        self.w_head_t = torch.empty(H, self.out_dim, dtype=h16, device=dev)

    # ------------------------------------------------------------------------------------------ workspace
    def _workspace(self, B):
        if self.ws is not None and self.ws["B"] == B:
            return self.ws
        dev, H, S, L, FF = self.device, self.H, self.S, len(self.layers), self.FF
        M = B * S
        h16 = self.h16     # the 16-bit operand buffers (and the 16-bit residual stream) are fp16 in an fp16 engine
        z = lambda *s, dt=h16: torch.empty(*s, dtype=dt, device=dev)
        ws = {"B": B, "M": M, "gen": next(_WS_GEN)}
        rows = lambda l: B if l == L - 1 else M     # the last block's MLP runs on the token-0 rows alone (_Rows)
        ws["cols"] = z(B * 196, 3 * H if (self.mode.patch_split and not self.full_ft) else H)
        rb, ex = self.resid_bf16, self.exact()
        ws["resid_bf16"], ws["grad_bf16"] = rb, self.grad_bf16
        if ex:
            assert not rb and not self.grad_bf16, "the exact forward runs on the f32 streams"
            # per layer, all f32: LN1 output, q | k | v, attention output, fc1 pre-activation -- what the exact backward reads
            ws["y32s"], ws["ctx32s"] = [z(M, H, dt=F32) for _ in range(L)], [z(M, H, dt=F32) for _ in range(L)]
            ws["qkv32s"] = [z(M, 3 * H, dt=F32) for _ in range(L)]
            ws["z32s"] = [z(rows(l), FF, dt=F32) for l in range(L)]
            ws["y32"], ws["cls32"] = z(M, H, dt=F32), z(B, H, dt=F32)
            ws["a3"] = z(M, 3 * FF)                                   # [hi | lo | hi] rows of the current GEMM's A operand
            ws["whead3"] = z(self.out_dim, 3 * H)
            Bq = _pad64(B)
            ws["g32"], ws["dh32"], ws["dctx32"], ws["dqkv32"] = z(M, FF, dt=F32), z(M, H, dt=F32), z(M, H, dt=F32), z(M, 3 * H, dt=F32)
            ws["dcls32"] = z(B, H, dt=F32)
            ws["t3a"], ws["t3b"] = z(self.out_dim * 3 * Bq), z(H * 3 * Bq)         # dW operands of the head
            ws["wheadT3"] = z(H * 3 * self.out_dim)
        ws["x"] = [z(M, H, dt=h16 if rb else F32) for _ in range(2 * L + 1)]   # residual stream after every sub-layer
        ws["h1"] = [z(M, H + KPAD) for _ in range(L)]                 # LN1 output + LoRA t (QKV operand)
        ws["st1"] = [z(M, 2, dt=F32) for _ in range(L)]
        ws["st2"] = [z(rows(l), 2, dt=F32) for l in range(L)]
        ws["qkv"] = [z(M, 3 * H) for _ in range(L)]
        ws["ctx"] = [z(M, H) for _ in range(L)]
        ws["lse"] = [z(B, self.heads, S, dt=F32) for _ in range(L)]
        ws["z"] = [z(rows(l), FF, dt=torch.uint8) for l in range(L)]   # gelu'(fc1 pre-activation), 8-bit codes
        ws["h2"] = z(M, H)
        ws["act"] = z(M, FF)
        if self.full_ft:  # inputs of fc1 / fc2 per block: operands of their weight-gradient GEMMs
            ws["h2s"] = [z(rows(l), H) for l in range(L)]
            ws["acts"] = [z(rows(l), FF) for l in range(L)]
        if self.fp8:  # fp8 GEMM operands: LN1 output per block (lora_grad reads it again) + its bf16 t block, LN2 / GELU shared
            ws["h1_8"] = [z(M, H, dt=ops.FP8) for _ in range(L)]
            ws["t"] = [z(M, KPAD) for _ in range(L)]
            ws["h2_8"], ws["act8"] = z(M, H, dt=ops.FP8), z(M, FF, dt=ops.FP8)
        ws["clsn"] = z(B, H)
        ws["st_f"] = z(B, 2, dt=F32)
        # backward temporaries (16-bit ones in the operand format: an fp16 engine's gradient stream and dX operands are fp16, in
        # units of the tower's static gradient scale 2^FP16_GRAD_SCALE_LOG2)
        assert ws["grad_bf16"] or not self.fp16, "the fp16 backward runs on the 16-bit gradient stream"
        ws["dx"] = None if ws["grad_bf16"] else torch.zeros(M, H, dtype=F32, device=dev)
        ws["dxb"] = torch.zeros(M, H, dtype=h16, device=dev)
        ws["dz"] = z(M, FF)
        ws["dh"] = z(M, H)
        ws["dctx"] = z(M, H)
        ws["dqkv"] = z(M, 3 * H)
        ws["dt"] = z(M, 8, dt=F32)
        ws["dtp"], ws["dbp"] = z(self.heads, 2, M, 4, dt=F32), z(B * self.heads, 2, 4, 64, dt=F32)   # LoRA partial sums (mode.attn_lora)
        Bp = _pad64(B)
        ws["dout_bf"] = torch.zeros(B, self.out_dim, dtype=h16, device=dev)
        ws["dout_t"] = torch.zeros(self.out_dim, Bp, dtype=h16, device=dev)
        ws["clsn_t"] = torch.zeros(H, Bp, dtype=h16, device=dev)
        if self.fp16:   # the head's dW in 2^s units, before bsclip_add_scaled_f32 takes the scale off into .grad
            ws["gw_head"] = torch.empty(self.out_dim, H, dtype=F32, device=dev)
        ws["dclsn"] = z(B, H)
        g, ctx, dctx = ws["dxb" if ws["grad_bf16"] else "dx"], ws["ctx32s" if ex else "ctx"], ws["dctx32" if ex else "dctx"]
        ws["rows"] = []
        for l in range(L):
            last = l == L - 1
            v = (lambda t: tok0(t, B)) if last else (lambda t: t)
            if self.full_ft:
                h2, act = ws["h2s"][l], ws["acts"][l]
            else:
                h2, act = (z(B, H), z(B, FF)) if last else (ws["h2"], ws["act"])
            ws["rows"].append(_Rows(
                M=rows(l), q_rows=int(last), x=[v(t) for t in ws["x"][2 * l:2 * l + 3]], ctx=v(ctx[l]), h2=h2, act=act,
                z=ws["z32s" if ex else "z"][l], st2=ws["st2"][l], mlp8=self.fp8 and not last, split=not last, g=v(g), dxb=v(ws["dxb"]),
                dz=z(B, FF) if last else ws["dz"], dh=z(B, H) if last else ws["dh"], dctx=v(dctx), zero=dctx if last else None))
        return self._keep_workspace(ws)

    def backward_probes(self):
        """(name, tensor) of the backward's 16-bit gradient buffers (BSCLIP_DETECT_ANOMALY on an fp16 engine: the scaled gradient
        stream is where an fp16 overflow would show first).  What the last backward left in them: the shared temporaries hold
        block 0's values (the head's for dout)."""
        ws = self.ws
        for name in ("dout_bf", "dxb", "dz", "dh", "dctx", "dqkv") if self.fp16 else ():
            yield f"the fp16 backward's {name}", ws[name]

    def anomaly_probes(self):
        """(name, tensor) of the forward's saved activations in execution order (BSCLIP_DETECT_ANOMALY).  The last block's
        sub-layers exist on the token-0 rows only."""
        ws = self.ws
        qkv, ctx = ("qkv32s", "ctx32s") if self.exact() else ("qkv", "ctx")
        yield "the patch embedding + position table", ws["x"][0]
        for l, r in enumerate(ws["rows"]):
            yield f"blocks.{l}.attn.qkv output", ws[qkv][l]
            if not r.q_rows:
                yield f"blocks.{l}.attn output", ws[ctx][l]
            yield f"blocks.{l} residual stream after attention", r.x[1]
            yield f"blocks.{l} residual stream after the MLP", r.x[2]

    # -------------------------------------------------------------------------------------------- forward
    def _forward_exact(self, image, ws):
        """BSCLIP_PARITY=2: the same block sequence with every Linear and every attention product on split-bf16 operands (f32 in / out), exact-erf GELU; what
        ``_backward_exact`` reads -- per layer the f32 LN1 output, q | k | v, attention output and fc1 pre-activation, the
        LayerNorm statistics, lse, the f32 residual stream -- stays resident."""
        B, H, S, M = image.shape[0], self.H, self.S, ws["M"]
        scale = 64 ** -0.5
        x, a3 = ws["x"], ws["a3"]
        self._ex_forward_weights()
        ops.im2col_patch16(image, ws["cols"])
        ops.gemm(ws["cols"], self.w_patch3, x[0], EPI_PATCH_F32, bias=self.b_patch, resid=self.pos)
        ops.vit_cls_rows(x[0], self.cls, self.pos, B, S, H)
        for l, (lay, r) in enumerate(zip(self.layers, ws["rows"])):
            has = self._lora_index[l] is not None
            y32, qkv32 = ws["y32s"][l], ws["qkv32s"][l]
            # the LayerNorm writes the QKV GEMM's split operand itself (and the f32 copy the LoRA gradients read in the backward)
            ops.layernorm_fwd(x[2 * l], lay.ln1[0], lay.ln1[1], 1e-6, y_f32=y32, y_split3=a3, stats=ws["st1"][l])
            ops.split3_weight(lay.qkv32, lay.wqkv3, lora_a=self.lora_a(l) if has else None, lora_b=self.lora_b(l) if has else None)
            self._ex_gemm3(a3, lay.wqkv3, qkv32, EPI_F32, M, bias=lay.b_qkv)
            ops.attn_fwd_f32(qkv32, B, S, self.heads, scale, ws["ctx32s"][l], ws["lse"][l], ctx_split3=a3 if r.split else None)
            self._ex_gemm(r.ctx, lay.w3[0], r.x[1], EPI_RESID_F32, a3, M=r.M, presplit=r.split, bias=lay.b_proj, resid=r.x[0])
            if r.split:     # a3: written by the LayerNorm
                ops.layernorm_fwd(r.x[1], lay.ln2[0], lay.ln2[1], 1e-6, y_split3=a3, stats=r.st2)
                self._ex_gemm3(a3, lay.w3[1], r.z, EPI_F32, r.M, bias=lay.b_fc1)
            else:
                ops.layernorm_fwd(r.x[1], lay.ln2[0], lay.ln2[1], 1e-6, y_bf16=r.h2, y_f32=ws["cls32"], stats=r.st2)
                self._ex_gemm(ws["cls32"], lay.w3[1], r.z, EPI_F32, a3, bias=lay.b_fc1)
            g3 = ops.gelu_split3(r.z, a3, M=r.M)
            ops.gemm(g3, lay.w3[2], r.x[2], EPI_RESID_F32, bias=lay.b_fc2, resid=r.x[1], M=r.M)
        ops.layernorm_fwd(ws["rows"][-1].x[2], self.ln_f[0], self.ln_f[1], 1e-6, y_bf16=ws["clsn"], y_f32=ws["cls32"], stats=ws["st_f"])
        ops.split3_weight(self.extra(0), ws["whead3"])
        out = torch.empty(B, self.out_dim, dtype=F32, device=self.device)
        self._ex_gemm(ws["cls32"], ws["whead3"], out, EPI_F32, a3, bias=self.extra(1))
        return out

    def forward(self, image):
        B = image.shape[0]
        ws = self._workspace(B)
        H, S, M = self.H, self.S, ws["M"]
        scale = 64 ** -0.5
        self.refresh_lora_weights()
        ops.cast_f32_bf16(self.extra(0), self.w_head_bf)
        if self.exact():
            return self._forward_exact(image, ws)
        x = ws["x"]
        EPI_R, EPI_P = (EPI_RESID_BF16, EPI_PATCH_BF16) if ws["resid_bf16"] else (EPI_RESID_F32, EPI_PATCH_F32)
        ops.im2col_patch16(image, ws["cols"])
        ops.gemm(ws["cols"], self.w_patch3 if ws["cols"].shape[1] == 3 * H else self.w_patch, x[0], EPI_P, bias=self.b_patch,
                 resid=self.pos)
        ops.vit_cls_rows(x[0], self.cls, self.pos, B, S, H)
        for l, (lay, r) in enumerate(zip(self.layers, ws["rows"])):
            if self.fp8:
                ops.layernorm_fwd_fp8(x[2 * l], lay.ln1[0], lay.ln1[1], 1e-6, ws["h1_8"][l], t_aug=ws["t"][l],
                                      lora_a=self.lora_a(l), stats=ws["st1"][l])
                ops.gemm_fp8(ws["h1_8"][l], lay.w_qkv8, ws["qkv"][l], lay.s_qkv, lay.b_qkv, EPI_BF16, a_aug=ws["t"][l],
                             b_aug=lay.baug)
            else:
                ops.layernorm_fwd(x[2 * l], lay.ln1[0], lay.ln1[1], 1e-6, y_bf16=ws["h1"][l], lora_a=self.lora_a(l),
                                  stats=ws["st1"][l])
                ops.gemm(ws["h1"][l], lay.waug, ws["qkv"][l], EPI_BF16, bias=lay.b_qkv)
            ops.attn_fwd(ws["qkv"][l], B, S, self.heads, scale, ws["ctx"][l], ws["lse"][l], q_rows=r.q_rows)
            ops.gemm(r.ctx, lay.w_proj, r.x[1], EPI_R, bias=lay.b_proj, resid=r.x[0])
            if r.mlp8:
                ops.layernorm_fwd_fp8(r.x[1], lay.ln2[0], lay.ln2[1], 1e-6, ws["h2_8"], stats=r.st2)
                ops.gemm_fp8(ws["h2_8"], lay.w_fc1_8, ws["act8"], lay.s_fc1, lay.b_fc1, EPI_GELU_FP8, aux=r.z)
                ops.gemm_fp8(ws["act8"], lay.w_fc2_8, r.x[2], lay.s_fc2, lay.b_fc2, EPI_RESID_F32, resid=r.x[1])
                continue
            ops.layernorm_fwd(r.x[1], lay.ln2[0], lay.ln2[1], 1e-6, y_bf16=r.h2, stats=r.st2)
            ops.gemm(r.h2, lay.w_fc1, r.act, EPI_GELU_BF16, bias=lay.b_fc1, aux=r.z)
            ops.gemm(r.act, lay.w_fc2, r.x[2], EPI_R, bias=lay.b_fc2, resid=r.x[1])
        ops.layernorm_fwd(ws["rows"][-1].x[2], self.ln_f[0], self.ln_f[1], 1e-6, y_bf16=ws["clsn"], stats=ws["st_f"])
        out = torch.empty(B, self.out_dim, dtype=F32, device=self.device)
        ops.gemm(ws["clsn"], self.w_head_bf, out, EPI_F32, bias=self.extra(1))
        return out

    # ------------------------------------------------------------------------------------------- backward
    # measurement hook (tools/fp16_grad_scale.py, tests): a callable (site, tensor) called after each backward site writes its 16-bit
    # gradient -- it may read the tensor back (host sync), so only eager runs set it.  None: no calls.
    grad_probe = None

    def backward(self, dout):
        """The LoRA, fp8, fp16 and full fine-tuning backward.  Full fine-tuning (hip/engine_ft.py) differs by what the hooks
        ``_dw`` / ``_ln_dw`` / ``_below_layer0`` add -- no-ops here -- and by the chain continuing through block 0.  One block body
        for every block: ``ws["rows"][l]`` (_Rows) says which rows of which buffers the MLP, LayerNorm-2 and out-projection backward
        of block l work on -- the last block's are the token-0 rows, as only those carry a gradient from the head."""
        if self.exact():
            return self._backward_exact(dout)
        ws = self.ws
        B, M, H, S, FF = ws["B"], ws["M"], self.H, self.S, self.FF
        scale = 64 ** -0.5
        self.flat.bind_grads()
        x = ws["x"]
        dx, dxb = ws["dx"], ws["dxb"]
        f16, ft = self.fp16, self.full_ft
        gs = self.FP16_GRAD_SCALE_LOG2 if f16 else None
        self._head_backward(ws, dout, ws["clsn"], ws["clsn_t"], ws["dclsn"], EPI_BF16)
        probe = self.grad_probe or (lambda site, t: None)
        probe("dout", ws["dout_bf"])     # the head's scaled dout: still in its buffer
        # final norm on token-0 rows only: every other row of the residual gradient is zero
        # bf16 gradient stream (no dropout in the ViT): the bf16 operand buffer IS the residual gradient, read and rewritten
        # in place by each LayerNorm backward (same lane, same elements); the f32 copy does not exist
        g16 = ws["grad_bf16"]
        R = dxb if g16 else dx          # the residual-gradient stream
        if not g16:
            dx.zero_()
        dxb.zero_()
        r = ws["rows"][-1]
        self._ln_dw(r.x[2], ws["st_f"], 0, "norm.w", "norm.b", g_gemm=ws["dclsn"])
        ops.layernorm_bwd(r.x[2], ws["st_f"], self.ln_f[0], 0, g_gemm=ws["dclsn"], dx_f32=None if g16 else r.g, dx_bf16=r.dxb)
        for l in range(len(self.layers) - 1, -1, -1):
            lay, r = self.layers[l], ws["rows"][l]
            probe("grad_stream", r.dxb)
            self._dw(r.dxb, r.act, r.M, H, FF, f"{l}.fc2.w", f"{l}.fc2.b")
            ops.gemm(r.dxb, lay.w_fc2_t, r.dz, EPI_DGELU_BF16, aux=r.z)
            probe("dfc1_out", r.dz)
            self._dw(r.dz, r.h2, r.M, FF, H, f"{l}.fc1.w", f"{l}.fc1.b")
            ops.gemm(r.dz, lay.w_fc1_t, r.dh, EPI_BF16)
            probe("dln2_out", r.dh)
            self._ln_dw(r.x[1], r.st2, 0, f"{l}.n2.w", f"{l}.n2.b", g_gemm=r.dh)
            ops.layernorm_bwd(r.x[1], r.st2, lay.ln2[0], 0, g_resid=r.g, g_gemm=r.dh, dx_f32=None if g16 else r.g, dx_bf16=r.dxb)
            probe("grad_stream", r.dxb)
            self._dw(r.dxb, r.ctx, r.M, H, H, f"{l}.proj.w", f"{l}.proj.b")
            if r.zero is not None:
                r.zero.zero_()
            ops.gemm(r.dxb, lay.w_proj_t, r.dctx, EPI_BF16)
            probe("dattn_out", ws["dctx"])
            lb = self.lora_b(l)
            # dt / dB partial sums out of the attention backward (the fp16 backward has this form only)
            part = lb is not None and (self.mode.attn_lora or f16) and not self.fp8
            ops.attn_bwd(ws["qkv"][l], ws["dctx"], ws["lse"][l], B, S, self.heads, scale, ws["dqkv"],
                         q_rows=r.q_rows, lora=(ws["h1"][l][:, H:], lb, ws["dtp"], ws["dbp"]) if part else None)
            probe("dqkv", ws["dqkv"])
            self._dw(ws["dqkv"], ws["h1"][l], M, 3 * H, H, f"{l}.qkv.w", f"{l}.qkv.b")
            self._lora_grads(l, ws, ws["h1"][l], ws["h1_8"][l] if self.fp8 else None, part, gs)
            if l > 0 or ft:  # LoRA regime: nothing trainable sits below block 0 (patch-embed, cls, pos are frozen)
                ops.gemm(ws["dqkv"], lay.wqkv_t, ws["dh"], EPI_BF16)
                probe("dln1_out", ws["dh"])
                dt, la = (ws["dt"], self.lora_a(l)) if lb is not None else (None, None)
                self._ln_dw(x[2 * l], ws["st1"][l], 0, f"{l}.n1.w", f"{l}.n1.b", g_gemm=ws["dh"], dt=dt, lora_a=la)
                ops.layernorm_bwd(x[2 * l], ws["st1"][l], lay.ln1[0], 0, g_resid=R, g_gemm=ws["dh"], dt=dt, lora_a=la,
                                  dx_f32=None if g16 else dx, dx_bf16=dxb)
        self._below_layer0(ws)

    def _backward_exact(self, dout):
        """BSCLIP_PARITY=2: the backward of ``_forward_exact`` with every gradient in f32 -- dX GEMMs on split operands against the
        transposed split weights (LoRA folded: W + B A), exact gelu' from the f32 pre-activation, the attention backward on split operands (f32 in / out), f32 LoRA
        gradients, the head's dW on operands split along the batch."""
        ws = self.ws
        B, M, H, S, L = ws["B"], ws["M"], self.H, self.S, len(self.layers)
        scale = 64 ** -0.5
        self.flat.bind_grads()
        self._ex_backward_weights()
        x, dx, a3 = ws["x"], ws["dx"], ws["a3"]
        dout = dout.contiguous()
        self._ex_dw(dout, ws["cls32"], self.extra(0, grad=True), ws)            # cls32 = the final LayerNorm's f32 output
        ops.colsum(dout, B, self.out_dim, self.extra(1, grad=True))
        self._ex_gemm(dout, ops.split3_transpose(self.extra(0), ws["wheadT3"], 1), ws["dcls32"], EPI_F32, a3)
        dx.zero_()
        r = ws["rows"][-1]
        ops.layernorm_bwd(r.x[2], ws["st_f"], self.ln_f[0], 0, g_gemm=ws["dcls32"], dx_f32=r.g)
        for l in range(L - 1, -1, -1):
            lay, r = self.layers[l], ws["rows"][l]
            # r.split: a3 holds the split of r.g, left there by the LayerNorm backward that produced r.g
            self._ex_gemm(r.g, lay.w3t[2], ws["g32"], EPI_F32, a3, M=r.M, presplit=r.split)
            g3 = ops.dgelu_split3(ws["g32"], r.z, dst=a3, M=r.M)
            ops.gemm(g3, lay.w3t[1], ws["dh32"], EPI_F32, M=r.M)
            ops.layernorm_bwd(r.x[1], r.st2, lay.ln2[0], 0, g_resid=r.g, g_gemm=ws["dh32"], dx_f32=r.g,
                              dx_split3=a3 if r.split else None, M=r.M)
            if r.zero is not None:
                r.zero.zero_()
            self._ex_gemm(r.g, lay.w3t[0], r.dctx, EPI_F32, a3, M=r.M, presplit=r.split)
            ops.attn_bwd_f32(ws["qkv32s"][l], ws["dctx32"], ws["ctx32s"][l], ws["lse"][l], B, S, self.heads, scale, ws["dqkv32"],
                             dqkv_split3=a3 if l > 0 else None)      # the QKV dX GEMM's operand, written split by the attention kernel
            has = self._lora_index[l] is not None
            if has:
                ops.lora_grad_f32(ws["dqkv32"], ws["y32s"][l], M, H, self.lora_a(l), self.lora_b(l), self.lora_a(l, grad=True),
                                  self.lora_b(l, grad=True))
            if l > 0:  # nothing trainable sits below block 0
                wt = ops.split3_transpose(lay.qkv32, lay.wqkvT3, 1, lora_a=self.lora_a(l) if has else None,
                                          lora_b=self.lora_b(l) if has else None)
                self._ex_gemm3(a3, wt, ws["dh32"], EPI_F32, M)
                ops.layernorm_bwd(x[2 * l], ws["st1"][l], lay.ln1[0], 0, g_resid=dx, g_gemm=ws["dh32"], dx_f32=dx, dx_split3=a3)

# ======================================================================================================= BERT
class BertEngine(EncoderEngineBase):
    """HF-BERT trunk with LoRA on query/value (reference dna_encoder.py:40-105, language_encoder.py:24-89).

    ``head`` selects what follows the trunk:
      'mlm_softmax_mean' : cls.predictions.transform -> decoder Linear -> softmax(-1) -> mean over tokens (DNA)
      'mean_proj'        : mean over tokens -> proj Linear (text)
    """

    def __init__(self, bert, head, head_modules, device, mode, reuse_flat=None):
        super().__init__(mode, device)
        h16, dev = self.h16, device
        cfg = getattr(bert, "config", None)
        emb = bert.embeddings
        self.H = H = emb.word_embeddings.weight.shape[1]
        assert H in (768, 512), "HIP BERT engine supports hidden sizes 768 and 512"
        self.heads = H // 64
        nh = getattr(cfg, "num_attention_heads", self.heads)
        assert nh == self.heads, "HIP attention kernel is built for head_dim 64"
        self.eps = float(getattr(cfg, "layer_norm_eps", 1e-12))
        self.p_hidden = float(getattr(cfg, "hidden_dropout_prob", 0.0))
        self.p_attn = float(getattr(cfg, "attention_probs_dropout_prob", 0.0))
        self.word, self.posw, self.typew = (_f32(emb.word_embeddings.weight, dev),
                                            _f32(emb.position_embeddings.weight, dev),
                                            _f32(emb.token_type_embeddings.weight, dev))
        self.ln_e = (_f32(emb.LayerNorm.weight, dev), _f32(emb.LayerNorm.bias, dev))
        self.layers, qv = [], []
        for layer in bert.encoder.layer:
            lay = _Layer()
            sa = layer.attention.self
            q, k, v = sa.query, sa.key, sa.value
            if hasattr(q, "w_a"):
                qv.append((q.w_a, v.w_a, q.w_b, v.w_b))
                qb, vb = q.w, v.w
            else:
                qv.append(None)
                qb, vb = q, v
            w = torch.cat([qb.weight.detach(), k.weight.detach(), vb.weight.detach()], 0)
            b = torch.cat([qb.bias.detach(), k.bias.detach(), vb.bias.detach()], 0)
            lay.waug, lay.wqkv_t, lay.b_qkv = _pack_qkv(w, b, H, dev, h16, transposed=not self.fp16)
            lay.src = (w, layer.attention.output.dense.weight, layer.intermediate.dense.weight, layer.output.dense.weight)   # f32 masters
            lay.w_o, lay.w_o_t, lay.b_o = _pack_linear(layer.attention.output.dense, dev, h16, transposed=not self.fp16)
            lay.ln_a = (_f32(layer.attention.output.LayerNorm.weight, dev), _f32(layer.attention.output.LayerNorm.bias, dev))
            lay.w_fc1, lay.w_fc1_t, lay.b_fc1 = _pack_linear(layer.intermediate.dense, dev, h16, transposed=not self.fp16)
            lay.w_fc2, lay.w_fc2_t, lay.b_fc2 = _pack_linear(layer.output.dense, dev, h16, transposed=not self.fp16)
            lay.ln_b = (_f32(layer.output.LayerNorm.weight, dev), _f32(layer.output.LayerNorm.bias, dev))
            if self.fp8:
                self._pack_fp8(lay, w, layer.intermediate.dense.weight, layer.output.dense.weight, dev)
            self.layers.append(lay)
        self.FF = self.layers[0].w_fc1.shape[0]
        self.head = head
        if head == "mlm_softmax_mean":
            tr, dec = head_modules
            self.w_tr, self.w_tr_t, self.b_tr = _pack_linear(tr.dense, dev, h16, transposed=not self.fp16)
            self.src_tr = tr.dense.weight
            self.ln_t = (_f32(tr.LayerNorm.weight, dev), _f32(tr.LayerNorm.bias, dev))
            self.eps_t = float(tr.LayerNorm.eps)
            trainable = [dec.weight, dec.bias]
            self.out_dim, self.head_in = dec.weight.shape
            assert self.out_dim == 768, "softmax-mean head kernel is built for 768 classes"
        else:
            (proj,) = head_modules
            trainable = [proj.weight, proj.bias]
            self.out_dim, self.head_in = proj.weight.shape
        assert self.out_dim % 128 == 0 and self.head_in % 128 == 0
        self._setup_lora(qv, H, dev, trainable, reuse_flat)
        self.w_head_bf = torch.empty(self.out_dim, self.head_in, dtype=h16, device=dev)   # the head weight in the operand format
        self.w_head_t = None if self.fp16 else torch.empty(self.head_in, self.out_dim, dtype=BF16, device=dev)

    def _workspace(self, B, S):
        if self.ws is not None and self.ws["B"] == B and self.ws["S"] == S:
            return self.ws
        dev, H, L, FF = self.device, self.H, len(self.layers), self.FF
        M = B * S
        h16 = self.h16     # the 16-bit operand buffers (and the 16-bit residual stream) are fp16 in an fp16 engine
        z = lambda *s, dt=h16: torch.empty(*s, dtype=dt, device=dev)
        ws = {"B": B, "S": S, "M": M, "gen": next(_WS_GEN)}
        ws["emb"] = z(M, H, dt=F32)
        ws["yb"] = [z(M, H + KPAD) for _ in range(L + 1)]   # LN outputs feeding each layer's QKV GEMM (+ LoRA t)
        mode = self.mode
        rb = ws["resid_bf16"] = self.resid_bf16
        sdt = h16 if rb else F32
        ws["y"] = z(M, H, dt=F32)                           # f32 copy of the current layer input (residual; bf16 stream: head input only)
        ws["ym"] = None if rb else z(M, H, dt=F32)
        ws["ymb"] = z(M, H)
        ws["qkv"] = [z(M, 3 * H) for _ in range(L)]
        ws["ctx"] = [z(M, H) for _ in range(L)]
        ws["lse"] = [z(B, self.heads, S, dt=F32) for _ in range(L)]
        # attention-probs dropout: the forward leaves its keep decisions (1 bit per probability, 32 B per query row) for the backward,
        # which otherwise re-hashes every element (mode.attn_keep_bits off: the re-hashing form, same masks); 64 B per query row
        ws["kbits"] = ([torch.zeros(B * self.heads * S * ops.KEEP_WORDS, dtype=torch.int32, device=dev) for _ in range(L)]
                       if self.p_attn > 0.0 and mode.attn_keep_bits and not self.exact() and not self.fp16 else None)
        ws["s1"] = [z(M, H, dt=sdt) for _ in range(L)]      # pre-LN sums (LN backward inputs)
        ws["s2"] = [z(M, H, dt=sdt) for _ in range(L)]
        ws["sta"] = [z(M, 2, dt=F32) for _ in range(L)]
        ws["stb"] = [z(M, 2, dt=F32) for _ in range(L)]
        ws["z"] = [z(M, FF, dt=torch.uint8) for _ in range(L)]       # gelu'(intermediate pre-activation), 8-bit codes
        ws["act"] = z(M, FF)
        if self.full_ft:
            ws["ymbs"] = [z(M, H) for _ in range(L)]
            ws["acts"] = [z(M, FF) for _ in range(L)]
            ws["st_e"] = z(M, 2, dt=F32)
        if self.fp8:  # fp8 GEMM operands (the last LN output stays bf16: it feeds the head)
            ws["yb8"] = [z(M, H, dt=ops.FP8) for _ in range(L)]
            ws["t"] = [z(M, KPAD) for _ in range(L)]
            ws["ymb8"], ws["act8"] = z(M, H, dt=ops.FP8), z(M, FF, dt=ops.FP8)
        if self.exact():
            assert not rb and not self.grad_bf16, "the exact forward runs on the f32 streams"
            # per layer, all f32: the layer input (ys[l]; ys[L] = the last hidden state), q | k | v, attention output, intermediate
            # pre-activation -- what the exact backward reads
            ws["ys"] = [ws["y"]] + [z(M, H, dt=F32) for _ in range(L)]
            ws["ctx32s"], ws["qkv32s"] = [z(M, H, dt=F32) for _ in range(L)], [z(M, 3 * H, dt=F32) for _ in range(L)]
            ws["z32s"] = [z(M, FF, dt=F32) for _ in range(L)]
            ws["a3"] = z(M, 3 * FF)
            ws["whead3"] = z(self.out_dim, 3 * self.head_in)
            ws["t32"], ws["mp32"] = z(M, H, dt=F32), z(B, H, dt=F32)
            ws["g32"], ws["dh32"], ws["dctx32"], ws["dqkv32"] = z(M, FF, dt=F32), z(M, H, dt=F32), z(M, H, dt=F32), z(M, 3 * H, dt=F32)
            ws["dop32"] = z(M, H, dt=F32)                       # a dX GEMM's operand when it carries a dropout mask
            ws["wheadT3"] = z(self.head_in * 3 * self.out_dim)
            rows = _pad64(M if self.head == "mlm_softmax_mean" else B)   # the head's dW reduces over tokens (MLM decoder) or sequences
            ws["t3a"], ws["t3b"] = z(self.out_dim * 3 * rows), z(self.head_in * 3 * rows)
            if self.head == "mlm_softmax_mean":
                ws["tz32"], ws["tn32"], ws["dlog32"] = z(M, H, dt=F32), z(M, H, dt=F32), z(M, self.out_dim, dt=F32)
        ws["key_bias"] = None
        ws["kb_buf"] = z(B, S, dt=F32)
        if self.fp16:    # inference only: the forward's head buffers, no backward temporaries
            if self.head == "mlm_softmax_mean":
                ws["tz"], ws["tg"], ws["tn"] = z(M, H, dt=torch.uint8), z(M, H), z(M, H)
                ws["st_t"], ws["logits"], ws["sm"] = z(M, 2, dt=F32), z(M, self.out_dim, dt=F32), z(M, 2, dt=F32)
            else:
                ws["mp"], ws["mp32"] = z(B, H), z(B, H, dt=F32)
            return self._keep_workspace(ws)
        # backward temporaries
        ws["grad_bf16"] = self.grad_bf16
        gdt = BF16 if ws["grad_bf16"] else F32       # residual-gradient stream (mode.grad_stream_bf16)
        ws["ds"] = z(M, H, dt=gdt)
        ws["dsb"] = z(M, H)
        ws["ds1"] = z(M, H, dt=gdt)
        ws["dz"] = z(M, FF)
        ws["dh"] = z(M, H)
        ws["dctx"] = z(M, H)
        ws["dqkv"] = z(M, 3 * H)
        ws["dt"] = z(M, 8, dt=F32)
        ws["dtp"], ws["dbp"] = z(self.heads, 2, M, 4, dt=F32), z(B * self.heads, 2, 4, 64, dt=F32)   # LoRA partial sums (mode.attn_lora)
        if self.head == "mlm_softmax_mean":
            ws["head_splits"], Mp = split_plan(M, self.out_dim, H)
            if ws["head_splits"] > 1:
                ws["head_partial"] = z(ws["head_splits"] * self.out_dim * H, dt=F32)
            ws["tz"] = z(M, H, dt=torch.uint8)   # gelu'(transform pre-activation), 8-bit codes
            ws["tg"] = z(M, H)            # gelu(transform)
            ws["tn"] = z(M, H)            # LN(gelu(.)) = decoder input
            ws["st_t"] = z(M, 2, dt=F32)
            ws["logits"] = z(M, self.out_dim, dt=F32)
            ws["sm"] = z(M, 2, dt=F32)
            ws["dlog"] = z(M, self.out_dim)
            ws["dlog_t"] = torch.zeros(self.out_dim, Mp, dtype=BF16, device=dev)
            ws["tn_t"] = torch.zeros(H, Mp, dtype=BF16, device=dev)
            ws["dtn"] = z(M, H)
            ws["dtg"] = z(M, H)
        else:
            Bp = _pad64(B)
            ws["mp"] = z(B, H)
            ws["dout_bf"] = torch.zeros(B, self.out_dim, dtype=BF16, device=dev)
            ws["dout_t"] = torch.zeros(self.out_dim, Bp, dtype=BF16, device=dev)
            ws["mp_t"] = torch.zeros(H, Bp, dtype=BF16, device=dev)
            ws["dmp"] = z(B, H, dt=F32)
            ws["dyl"] = z(M, H, dt=F32)
        return self._keep_workspace(ws)

    def _decoder_grads(self, ws, gw, gb):
        """dW_dec += dlogits^T tn (reduced over all B*S tokens: split-K, the [768, 768] output alone is 9 tiles) and db_dec += column
        sums of dlogits, which fall out of the transpose that builds the GEMM operand."""
        M, H = ws["M"], self.H
        ops.transpose_colsum_bf16(ws["dlog"], M, self.out_dim, ws["dlog_t"], gb)
        ops.transpose_bf16(ws["tn"], M, H, ws["tn_t"])
        if ws["head_splits"] > 1:
            ops.gemm_splitk_f32(ws["dlog_t"], ws["tn_t"], gw, ws["head_splits"], ws["head_partial"], K=ws["dlog_t"].shape[1])
        else:
            ops.gemm(ws["dlog_t"], ws["tn_t"], gw, EPI_RESID_F32, resid=gw)

    def _drop(self, ws, p, layer, site):
        """(p, seed) of one dropout site, or None when dropout is off (eval mode / p = 0).  The seed names the site; what
        makes the masks differ from step to step is the engine's device step word, mixed in when the kernel runs."""
        if not ws["train"] or p <= 0.0:
            return None
        return (p, (ws["drop_base"] + 0x9E3779B1 * (layer + 2) + 0x85EBCA6B * site) & 0xFFFFFFFF)

    def _begin_dropout(self, ws, advance):
        """Point this thread's dropout launches at the engine's step word (``bsclip_set_dropout_step``) and, in forward,
        advance it by one (a captured launch: a replayed hipGraph draws fresh masks, its backward re-reads the same value)."""
        if not (ws["train"] and (self.p_hidden > 0.0 or self.p_attn > 0.0)):
            ops.set_dropout_step(None)
            return
        if self._step_word is None:
            self._step_word = torch.zeros(1, dtype=torch.int32, device=self.device)
        if advance:
            ops.counter_add(self._step_word, 1)
        ops.set_dropout_step(self._step_word)

    def anomaly_probes(self):
        """(name, tensor) of the forward's saved activations in execution order (BSCLIP_DETECT_ANOMALY)."""
        ws = self.ws
        qkv = "qkv32s" if self.exact() else "qkv"
        yield "the embedding sum (word + position + token type)", ws["emb"]
        for l in range(len(self.layers)):
            yield f"encoder.layer.{l}.attention.self q / k / v", ws[qkv][l]
            yield f"encoder.layer.{l}.attention.output (pre-LayerNorm sum)", ws["s1"][l]
            yield f"encoder.layer.{l}.output (pre-LayerNorm sum)", ws["s2"][l]
        if self.head == "mlm_softmax_mean":
            yield "cls.predictions.decoder logits", ws["logits"]

    def _forward_exact(self, ws, key_bias):
        """BSCLIP_PARITY=2 (see ViTEngine._forward_exact): the layers after the embedding LayerNorm (which has just written the f32
        layer input ys[0]) with every Linear and every attention product on split-bf16 operands (f32 in / out), exact-erf GELU; dropout sites and seeds as in
        the default path; what ``_backward_exact`` reads stays resident in f32."""
        B, S, M, H, L, FF = ws["B"], ws["S"], ws["M"], self.H, len(self.layers), self.FF
        a3, ys = ws["a3"], ws["ys"]
        self._ex_forward_weights()
        for l, lay in enumerate(self.layers):
            has = self._lora_index[l] is not None
            qkv32, ctx32, z32 = ws["qkv32s"][l], ws["ctx32s"][l], ws["z32s"][l]
            ops.split3_weight(lay.qkv32, lay.wqkv3, lora_a=self.lora_a(l) if has else None, lora_b=self.lora_b(l) if has else None)
            self._ex_gemm3(a3, lay.wqkv3, qkv32, EPI_F32, M, bias=lay.b_qkv)     # a3 = split of ys[l], written by the LayerNorm before
            ops.attn_fwd_f32(qkv32, B, S, self.heads, 0.125, ctx32, ws["lse"][l], key_bias=key_bias,
                             dropout=self._drop(ws, self.p_attn, l, 1), ctx_split3=a3)
            self._ex_gemm3(a3, lay.w3[0], ws["s1"][l], EPI_RESID_F32, M, bias=lay.b_o, resid=ys[l],
                           dropout=self._drop(ws, self.p_hidden, l, 2))
            ops.layernorm_fwd(ws["s1"][l], lay.ln_a[0], lay.ln_a[1], self.eps, y_f32=ws["ym"], y_split3=a3, stats=ws["sta"][l])
            self._ex_gemm3(a3, lay.w3[1], z32, EPI_F32, M, bias=lay.b_fc1)
            g3 = ops.gelu_split3(z32, a3)
            ops.gemm(g3, lay.w3[2], ws["s2"][l], EPI_RESID_F32, bias=lay.b_fc2, resid=ws["ym"],
                     dropout=self._drop(ws, self.p_hidden, l, 3))
            ops.layernorm_fwd(ws["s2"][l], lay.ln_b[0], lay.ln_b[1], self.eps, y_f32=ys[l + 1], y_split3=a3, stats=ws["stb"][l])
        out = torch.empty(B, self.out_dim, dtype=F32, device=self.device)
        ops.split3_weight(self.extra(0), ws["whead3"])
        if self.head == "mlm_softmax_mean":
            if self.w_tr3 is None:
                self.w_tr3 = self._ex_weight(self.src_tr)[1]
            self._ex_gemm(ys[L], self.w_tr3, ws["tz32"], EPI_F32, a3, bias=self.b_tr)
            ops.gelu_split3(ws["tz32"], None, g32=ws["t32"])                                # the GELU feeds a LayerNorm: f32 out
            ops.layernorm_fwd(ws["t32"], self.ln_t[0], self.ln_t[1], self.eps_t, y_bf16=ws["tn"], y_f32=ws["tn32"], stats=ws["st_t"])
            self._ex_gemm(ws["tn32"], ws["whead3"], ws["logits"], EPI_F32, a3, bias=self.extra(1))
            ops.softmax_meanpool_fwd(ws["logits"], B, S, out, ws["sm"])
        else:
            ops.meanpool_tokens_f32(ys[L], B, S, ws["mp32"])
            self._ex_gemm(ws["mp32"], ws["whead3"], out, EPI_F32, a3, bias=self.extra(1))
        ops.set_dropout_step(None)
        return out

    def _backward_exact(self, dout):
        """BSCLIP_PARITY=2: the backward of ``_forward_exact`` in f32 (see ViTEngine._backward_exact); post-LN residuals and the
        dropout sites as in ``backward``."""
        ws = self.ws
        B, S, M, H, L = ws["B"], ws["S"], ws["M"], self.H, len(self.layers)
        self.flat.bind_grads()
        self._begin_dropout(ws, advance=False)
        self._ex_backward_weights()
        a3, ys = ws["a3"], ws["ys"]
        gw, gb = self.extra(0, grad=True), self.extra(1, grad=True)
        dout = dout.contiguous()
        wt_head = ops.split3_transpose(self.extra(0), ws["wheadT3"], 1)
        if self.head == "mlm_softmax_mean":
            if self.w_tr3t is None:
                self.w_tr3t = self._ex_weight_t(self.src_tr)
            ops.softmax_meanpool_bwd_f32(ws["logits"], ws["sm"], dout, B, S, ws["dlog32"])
            self._ex_dw(ws["dlog32"], ws["tn32"], gw, ws)
            ops.colsum(ws["dlog32"], M, self.out_dim, gb)
            self._ex_gemm(ws["dlog32"], wt_head, ws["dh32"], EPI_F32, a3)                   # d tn
            ops.layernorm_bwd(ws["t32"], ws["st_t"], self.ln_t[0], 0, g_gemm=ws["dh32"], dx_f32=ws["dop32"])
            g3 = ops.dgelu_split3(ws["dop32"], ws["tz32"], dst=a3)
            ops.gemm(g3, self.w_tr3t, ws["dh32"], EPI_F32)                                   # d (last hidden state)
            g_resid, g_gemm = None, ws["dh32"]
        else:
            self._ex_dw(dout, ws["mp32"], gw, ws)
            ops.colsum(dout, B, self.out_dim, gb)
            self._ex_gemm(dout, wt_head, ws["dmp"], EPI_F32, a3)
            ops.meanpool_tokens_bwd(ws["dmp"], B, S, ws["dyl"])
            g_resid, g_gemm = ws["dyl"], None
        for l in range(L - 1, -1, -1):
            lay = self.layers[l]
            drop_b, drop_a = self._drop(ws, self.p_hidden, l, 3), self._drop(ws, self.p_hidden, l, 2)
            # a dX GEMM's operand carries the mask its Linear's forward output was dropped with; without dropout it IS the stream
            # (round 5: the LayerNorm backward writes that operand split, [hi | lo | hi], straight into the GEMM's A buffer)
            ops.layernorm_bwd(ws["s2"][l], ws["stb"][l], lay.ln_b[0], 1, g_resid=g_resid, g_gemm=g_gemm, dx_f32=ws["ds"],
                              dx_split3=a3, dropout=drop_b)
            self._ex_gemm3(a3, lay.w3t[2], ws["g32"], EPI_F32, M)
            g3 = ops.dgelu_split3(ws["g32"], ws["z32s"][l], dst=a3)
            ops.gemm(g3, lay.w3t[1], ws["dh32"], EPI_F32)
            ops.layernorm_bwd(ws["s1"][l], ws["sta"][l], lay.ln_a[0], 1, g_resid=ws["ds"], g_gemm=ws["dh32"], dx_f32=ws["ds1"],
                              dx_split3=a3, dropout=drop_a)
            self._ex_gemm3(a3, lay.w3t[0], ws["dctx32"], EPI_F32, M)
            ops.attn_bwd_f32(ws["qkv32s"][l], ws["dctx32"], ws["ctx32s"][l], ws["lse"][l], B, S, self.heads, 0.125, ws["dqkv32"],
                             key_bias=ws["key_bias"], dropout=self._drop(ws, self.p_attn, l, 1), dqkv_split3=a3 if l > 0 else None)
            has = self._lora_index[l] is not None
            if has:
                ops.lora_grad_f32(ws["dqkv32"], ys[l], M, H, self.lora_a(l), self.lora_b(l), self.lora_a(l, grad=True),
                                  self.lora_b(l, grad=True))
            if l > 0:  # embeddings are frozen: nothing to do below layer 0
                wt = ops.split3_transpose(lay.qkv32, lay.wqkvT3, 1, lora_a=self.lora_a(l) if has else None,
                                          lora_b=self.lora_b(l) if has else None)
                self._ex_gemm3(a3, wt, ws["dh32"], EPI_F32, M)
                g_resid, g_gemm = ws["ds1"], ws["dh32"]
        ops.set_dropout_step(None)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None):
        B, S = input_ids.shape
        ws = self._workspace(B, S)
        H, M, L = self.H, ws["M"], len(self.layers)
        scale = 0.125
        # HF BERT dropout (hidden 0.1 / attention-probs 0.1) is active in train mode (reference train_epoch.py:20);
        # masks are functions of (seed, element index), regenerated in backward from the seeds kept here
        ws["train"] = bool(self.training)
        # the rank is mixed in: ranks seeded alike (bench.py, train_cl.py) must not draw the same masks for their shards
        # ... and the engine (its head kind): the DNA and text towers share layer / site numbers and step values
        ws["drop_base"] = (torch.initial_seed() * 0x2545F491 + _rank() * 0x632BE5AB + zlib.crc32(self.head.encode())) & 0xFFFFFFFF
        self._begin_dropout(ws, advance=True)
        self.refresh_lora_weights()
        ops.cast_f32_bf16(self.extra(0), self.w_head_bf)
        key_bias = None
        if attention_mask is not None:
            # HF extended mask (App. A.3): (1 - m) * finfo.min added to the scores of padded keys.
            key_bias = ws["kb_buf"]
            ops.mask_to_bias(attention_mask.to(torch.int64).contiguous(), key_bias)
        ws["key_bias"] = key_bias
        ops.bert_embed(input_ids.contiguous(), None if token_type_ids is None else token_type_ids.contiguous(),
                       self.word, self.posw, self.typew, ws["emb"])
        f8 = self.fp8
        rb = ws["resid_bf16"]   # bf16 residual stream: the LN's bf16 operand IS the residual, no f32 copy is written
        EPI_R = EPI_RESID_BF16 if rb else EPI_RESID_F32
        if f8:
            ops.layernorm_fwd_fp8(ws["emb"], self.ln_e[0], self.ln_e[1], self.eps, ws["yb8"][0], t_aug=ws["t"][0], y_f32=ws["y"],
                                  lora_a=self.lora_a(0), dropout=self._drop(ws, self.p_hidden, -1, 0))
        else:
            ops.layernorm_fwd(ws["emb"], self.ln_e[0], self.ln_e[1], self.eps, y_bf16=ws["yb"][0], y_f32=None if rb else ws["y"],
                              lora_a=self.lora_a(0), dropout=self._drop(ws, self.p_hidden, -1, 0),
                              stats=ws["st_e"] if self.full_ft else None,
                              y_split3=ws["a3"] if self.exact() else None)     # exact mode: layer 0's QKV operand, already split
        ws["ids"], ws["type_ids"] = input_ids, token_type_ids
        if self.exact():
            return self._forward_exact(ws, key_bias)
        for l, lay in enumerate(self.layers):
            if f8:
                ops.gemm_fp8(ws["yb8"][l], lay.w_qkv8, ws["qkv"][l], lay.s_qkv, lay.b_qkv, EPI_BF16, a_aug=ws["t"][l],
                             b_aug=lay.baug)
            else:
                ops.gemm(ws["yb"][l], lay.waug, ws["qkv"][l], EPI_BF16, bias=lay.b_qkv)
            drop_p = self._drop(ws, self.p_attn, l, 1)
            ops.attn_fwd(ws["qkv"][l], B, S, self.heads, scale, ws["ctx"][l], ws["lse"][l], key_bias=key_bias, dropout=drop_p,
                         keep_bits=ws["kbits"][l] if drop_p is not None and ws["kbits"] is not None else None)
            ops.gemm(ws["ctx"][l], lay.w_o, ws["s1"][l], EPI_R, bias=lay.b_o, resid=ws["yb"][l] if rb else ws["y"],
                     dropout=self._drop(ws, self.p_hidden, l, 2))
            if f8:
                ops.layernorm_fwd_fp8(ws["s1"][l], lay.ln_a[0], lay.ln_a[1], self.eps, ws["ymb8"], y_f32=ws["ym"],
                                      stats=ws["sta"][l])
                ops.gemm_fp8(ws["ymb8"], lay.w_fc1_8, ws["act8"], lay.s_fc1, lay.b_fc1, EPI_GELU_FP8, aux=ws["z"][l])
                ops.gemm_fp8(ws["act8"], lay.w_fc2_8, ws["s2"][l], lay.s_fc2, lay.b_fc2, EPI_RESID_F32, resid=ws["ym"],
                             dropout=self._drop(ws, self.p_hidden, l, 3))
            else:
                ymb, act = (ws["ymbs"][l], ws["acts"][l]) if self.full_ft else (ws["ymb"], ws["act"])
                ops.layernorm_fwd(ws["s1"][l], lay.ln_a[0], lay.ln_a[1], self.eps, y_bf16=ymb, y_f32=ws["ym"],
                                  stats=ws["sta"][l])
                ops.gemm(ymb, lay.w_fc1, act, EPI_GELU_BF16, bias=lay.b_fc1, aux=ws["z"][l])
                ops.gemm(act, lay.w_fc2, ws["s2"][l], EPI_R, bias=lay.b_fc2, resid=ymb if rb else ws["ym"],
                         dropout=self._drop(ws, self.p_hidden, l, 3))
            nxt = self.lora_a(l + 1) if l + 1 < L else self._zero_a
            if f8 and l + 1 < L:
                ops.layernorm_fwd_fp8(ws["s2"][l], lay.ln_b[0], lay.ln_b[1], self.eps, ws["yb8"][l + 1], t_aug=ws["t"][l + 1],
                                      y_f32=ws["y"], lora_a=nxt, stats=ws["stb"][l])
            else:
                # (bf16 stream: the f32 copy is written for the last layer only, where the mean-pool head reads it)
                ops.layernorm_fwd(ws["s2"][l], lay.ln_b[0], lay.ln_b[1], self.eps, y_bf16=ws["yb"][l + 1],
                                  y_f32=None if rb and not (l + 1 == L and self.head != "mlm_softmax_mean") else ws["y"],
                                  lora_a=nxt, stats=ws["stb"][l])
        out = torch.empty(B, self.out_dim, dtype=F32, device=self.device)
        if self.head == "mlm_softmax_mean":
            ops.gemm(ws["yb"][L], self.w_tr, ws["tg"], EPI_GELU_BF16, bias=self.b_tr, aux=ws["tz"], K=H)
            ops.layernorm_fwd(ws["tg"], self.ln_t[0], self.ln_t[1], self.eps_t, y_bf16=ws["tn"], stats=ws["st_t"])
            ops.gemm(ws["tn"], self.w_head_bf, ws["logits"], EPI_F32, bias=self.extra(1))
            ops.softmax_meanpool_fwd(ws["logits"], B, S, out, ws["sm"])
        else:
            if self.fp16:   # the mean-pool kernel writes bf16: pool in f32, round once to fp16
                ops.meanpool_tokens_f32(ws["y"], B, S, ws["mp32"])
                ops.cast_f32_bf16(ws["mp32"], ws["mp"])
            else:
                ops.meanpool_tokens_fwd(ws["y"], B, S, ws["mp"])
            ops.gemm(ws["mp"], self.w_head_bf, out, EPI_F32, bias=self.extra(1))
        ops.set_dropout_step(None)   # the pointer is per thread: do not leak it into the caller's own launches
        return out

    def backward(self, dout):
        """The LoRA, fp8 and full fine-tuning backward (see ViTEngine.backward for the hooks)."""
        self._no_fp16_backward()
        if self.exact():
            return self._backward_exact(dout)
        ws = self.ws
        B, S, M, H, L, FF = ws["B"], ws["S"], ws["M"], self.H, len(self.layers), self.FF
        scale = 0.125
        ft = self.full_ft
        self.flat.bind_grads()
        self._begin_dropout(ws, advance=False)   # backward runs on autograd's thread: the pointer is per thread
        if self.head == "mlm_softmax_mean":
            ops.transpose_bf16(self.w_head_bf, self.out_dim, self.head_in, self.w_head_t)
            ops.softmax_meanpool_bwd(ws["logits"], ws["sm"], dout, B, S, ws["dlog"])
            self._decoder_grads(ws, self.extra(0, grad=True), self.extra(1, grad=True))
            ops.gemm(ws["dlog"], self.w_head_t, ws["dtn"], EPI_BF16)                   # d tn
            self._ln_dw(ws["tg"], ws["st_t"], 0, "lnt.w", "lnt.b", g_gemm=ws["dtn"])
            ops.layernorm_bwd(ws["tg"], ws["st_t"], self.ln_t[0], 0, g_gemm=ws["dtn"], dx_bf16=ws["dtg"])
            ops.dgelu_mul(ws["dtg"], ws["tz"], M, H, ws["dtg"])
            self._dw(ws["dtg"], ws["yb"][L], M, H, H, "tr.w", "tr.b")
            ops.gemm(ws["dtg"], self.w_tr_t, ws["dh"], EPI_BF16)                       # d (last hidden state)
            g_resid, g_gemm = None, ws["dh"]
        else:
            self._head_backward(ws, dout, ws["mp"], ws["mp_t"], ws["dmp"], EPI_F32)   # dW_proj += dout^T mean, ...
            ops.meanpool_tokens_bwd(ws["dmp"], B, S, ws["dyl"])
            g_resid, g_gemm = ws["dyl"], None
        dt_in, a_in = None, None
        g16 = ws["grad_bf16"]
        for l in range(L - 1, -1, -1):
            lay = self.layers[l]
            ymb, act = (ws["ymbs"][l], ws["acts"][l]) if ft else (ws["ymb"], ws["act"])   # the dW hooks' operands, as the forward chose them
            # dsb is the operand of fc2's dX GEMM: it carries the mask fc2's forward output was dropped with.  With the bf16
            # gradient stream and no dropout the operand IS the residual gradient: one output, rewritten in place next time
            drop_b, drop_a = self._drop(ws, self.p_hidden, l, 3), self._drop(ws, self.p_hidden, l, 2)
            one_b, one_a = g16 and drop_b is None, g16 and drop_a is None
            self._ln_dw(ws["s2"][l], ws["stb"][l], 1, f"{l}.lnb.w", f"{l}.lnb.b", g_resid=g_resid, g_gemm=g_gemm, dt=dt_in, lora_a=a_in)
            ops.layernorm_bwd(ws["s2"][l], ws["stb"][l], lay.ln_b[0], 1, g_resid=g_resid, g_gemm=g_gemm, dt=dt_in,
                              lora_a=a_in, dx_f32=None if one_b else ws["ds"], dx_bf16=ws["dsb"], dropout=drop_b)
            self._dw(ws["dsb"], act, M, H, FF, f"{l}.fc2.w", f"{l}.fc2.b")
            ops.gemm(ws["dsb"], lay.w_fc2_t, ws["dz"], EPI_DGELU_BF16, aux=ws["z"][l])
            self._dw(ws["dz"], ymb, M, FF, H, f"{l}.fc1.w", f"{l}.fc1.b")
            ops.gemm(ws["dz"], lay.w_fc1_t, ws["dh"], EPI_BF16)
            r_a = ws["dsb"] if one_b else ws["ds"]
            self._ln_dw(ws["s1"][l], ws["sta"][l], 1, f"{l}.lna.w", f"{l}.lna.b", g_resid=r_a, g_gemm=ws["dh"])
            ops.layernorm_bwd(ws["s1"][l], ws["sta"][l], lay.ln_a[0], 1, g_resid=r_a, g_gemm=ws["dh"],
                              dx_f32=None if one_a else ws["ds1"], dx_bf16=ws["dsb"], dropout=drop_a)
            self._dw(ws["dsb"], ws["ctx"][l], M, H, H, f"{l}.o.w", f"{l}.o.b")
            ops.gemm(ws["dsb"], lay.w_o_t, ws["dctx"], EPI_BF16)
            drop_p = self._drop(ws, self.p_attn, l, 1)   # the forward left its keep decisions in ws["kbits"]
            lb = self.lora_b(l)
            kb = ws["kbits"][l] if drop_p is not None and ws["kbits"] is not None else None
            part = lb is not None and self.mode.attn_lora and not self.fp8 and (drop_p is None or kb is not None)
            ops.attn_bwd(ws["qkv"][l], ws["dctx"], ws["lse"][l], B, S, self.heads, scale, ws["dqkv"],
                         key_bias=ws["key_bias"], dropout=drop_p, keep_bits=kb,
                         lora=(ws["yb"][l][:, H:], lb, ws["dtp"], ws["dbp"]) if part else None)
            self._dw(ws["dqkv"], ws["yb"][l], M, 3 * H, H, f"{l}.q.w", f"{l}.q.b", w_n=3 * H * H)   # q / k / v are adjacent
            self._lora_grads(l, ws, ws["yb"][l], ws["yb8"][l] if self.fp8 else None, part)
            if l > 0 or ft:  # LoRA regime: embeddings are frozen, nothing to do below layer 0
                ops.gemm(ws["dqkv"], lay.wqkv_t, ws["dh"], EPI_BF16)
                g_resid, g_gemm = (ws["dsb"] if one_a else ws["ds1"]), ws["dh"]
                dt_in, a_in = (ws["dt"], self.lora_a(l)) if lb is not None else (None, None)
        self._below_layer0(ws, g_resid, g_gemm, dt_in, a_in)
        ops.set_dropout_step(None)


# ====================================================================================== autograd integration
_PARENT_STREAM = []  # stack: the stream a tower's side stream was forked from (set by SimpleCLIP.forward)


class forked_from:
    """``with forked_from(stream):`` -- encoders run inside (on a side stream) make ``stream`` wait for their BACKWARD.

    Autograd replays a node on the stream of its forward and, when backward() returns, only joins the streams on which it
    accumulated leaf gradients itself.  The encoder nodes write their parameter gradients from inside the kernels (they
    return ``None`` for the parameters), so autograd would not join the tower streams: the optimizer on the main stream
    could read the flat gradient buffer while the last blocks' backward kernels are still running."""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        _PARENT_STREAM.append(self.stream)

    def __exit__(self, *exc):
        _PARENT_STREAM.pop()


class _EncoderFn(torch.autograd.Function):
    """One autograd node per encoder: forward and backward are whole kernel sequences.  Trainable parameters are
    passed only so autograd records the node; their gradients are accumulated in place by the kernels (into the
    flat buffer ``p.grad`` aliases), hence ``None`` is returned for them."""

    @staticmethod
    def forward(ctx, engine, fwd_args, *params):
        ctx.engine = engine
        ctx.parent = _PARENT_STREAM[-1] if _PARENT_STREAM else None
        ctx.generation = engine._fwd_generation
        out = engine.forward(*fwd_args)
        if DETECT_ANOMALY:
            _anomaly_check(engine, "forward", out)
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.generation != ctx.engine._fwd_generation:
            raise RuntimeError("backward through an encoder forward whose saved activations were overwritten by a later forward "
                               "of the same encoder: the HIP engines hold one workspace per encoder -- run backward before the "
                               "next training-mode forward (the reference loop does: train_epoch.py:28-42)")
        ctx.engine.backward(dout.contiguous())
        if DETECT_ANOMALY:
            _anomaly_check(ctx.engine, "backward")
        from .dist import start_allreduce
        start_allreduce(ctx.engine.flat, type(ctx.engine).__name__)  # global-batch step: this tower's gradients are complete on this stream
        here = torch.cuda.current_stream()
        # gradients are complete before anything queued afterwards on the stream the tower was forked from -- and, outside a
        # stream capture, on the default stream (inside a capture that wait would pull the default stream into the graph and
        # leave it unjoined)
        parents = {ctx.parent} if torch.cuda.is_current_stream_capturing() else {ctx.parent, torch.cuda.default_stream(here.device)}
        for parent in parents:
            if parent is not None and parent != here:
                parent.wait_stream(here)
        return (None, None) + (None,) * len(ctx.engine.flat.params)


def _frozen_signature(module, eng):
    """(storage address, in-place version) of every tensor the engine packed into its own bf16 layouts.  An in-place
    ``load_state_dict`` / ``copy_`` after the engine was built bumps the version, ``.to()`` moves the storage."""
    mine = {id(p) for p in eng.flat.params}
    return tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers())
                 if id(t) not in mine)


def wants_fp8(module):
    """``module.hip_precision = "fp8"`` (set_precision) selects the fp8 frozen-trunk GEMMs (BASELINE configs[4])."""
    return getattr(module, "hip_precision", "bf16") == "fp8"


def set_precision(model, precision):
    """Select "bf16" (default) or "fp8" frozen-trunk GEMMs for the ViT and BarcodeBERT encoders under ``model``; engines
    are rebuilt on the next forward (the text tower stays bf16: its GEMMs are latency-sized)."""
    if precision not in ("bf16", "fp8"):
        raise ValueError(f"precision must be 'bf16' or 'fp8', not {precision!r}")
    for m in model.modules():
        if hasattr(m, "lora_vit") or hasattr(m, "lora_barcode_bert"):
            m.hip_precision = precision
            _park_engine(m)


OPERAND_FORMATS = ("bf16", "fp16")


def wants_fp16(module):
    """``module.hip_operands = "fp16"`` (set_operand_format): the encoder runs on fp16 operands -- the LoRA ViT forward and backward
    (training included), the BarcodeBERT and text encoders' forward only (inference)."""
    return getattr(module, "hip_operands", "bf16") == "fp16"


# set_operand_format's tower names -> the attribute that marks the encoder module of that tower
OPERAND_TOWERS = {"image": "lora_vit", "dna": "lora_barcode_bert", "language": "lora_bert"}


def set_operand_format(model, fmt, towers=None):
    """Select the 16-bit operand format of the ViT, BarcodeBERT and text encoders under ``model``: "bf16" (default) or "fp16".
    fp16 runs every GEMM, attention product and LayerNorm output on IEEE fp16 (same MFMA rate, 3 more mantissa bits: DESIGN.md 4).
    The image tower (LoRA ViT) also trains on fp16: its backward runs on fp16 operands with a static gradient scale, and .grad holds
    the true gradient.  The DNA and text towers' fp16 engines are inference-only -- eval() and torch.no_grad() -- until their fp16
    backward (dropout forms) exists.  ``towers``: a subset of ("image", "dna", "language"), default None = every tower; the others
    keep their format (a mixed step: image on fp16, DNA and text on bf16).  Engines are rebuilt on the next forward; their flat
    trainable buffers (LoRA, heads, the optimizer's moments keyed on them) carry over, as after every change of mode."""
    if fmt not in OPERAND_FORMATS:
        raise ValueError(f"operand format must be 'bf16' or 'fp16', not {fmt!r}")
    if towers is None:
        towers = tuple(OPERAND_TOWERS)
    elif isinstance(towers, str):
        towers = (towers,)
    bad = [t for t in towers if t not in OPERAND_TOWERS]
    if bad or not towers:
        raise ValueError(f"towers must be a non-empty subset of {tuple(OPERAND_TOWERS)}, not {towers!r}")
    marks = [OPERAND_TOWERS[t] for t in towers]
    for m in model.modules():
        if any(hasattr(m, a) for a in marks):
            m.hip_operands = fmt
            _park_engine(m)


def _check_fp16(module):
    """fp16 operands: the LoRA-regime engines on the 16-bit streams -- the ViT in train or eval mode, the BERT engines for inference
    only; everything else is refused before an engine is built."""
    who = type(module).__name__
    if wants_fp8(module):
        raise ValueError(f"{who}: fp16 operands cannot be combined with set_precision(..., 'fp8')")
    if wants_full_ft(module):
        raise ValueError(f"{who}: fp16 operands are not available for full fine-tuning (disable_lora: true)")
    if EXACT_FORWARD or not RESID_STREAM_BF16:
        raise ValueError(f"{who}: fp16 operands run on the 16-bit residual stream: not with BSCLIP_PARITY=1 / 2 "
                         "(set_parity_mode) or BSCLIP_RESID_STREAM=f32")
    trains = module.training or (torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()))
    if hasattr(module, "lora_vit"):
        if trains and not GRAD_STREAM_BF16:
            raise ValueError(f"{who}: the fp16 backward runs on the 16-bit gradient stream: not with BSCLIP_GRAD_STREAM=f32")
        return
    if trains:
        raise RuntimeError(f"{who}: the fp16-operand forward is inference-only (the fp16 backward is not built yet): call "
                           "model.eval() and run it under torch.no_grad(), or set_operand_format(model, 'bf16')")


def wants_full_ft(module):
    """``module.hip_full_ft`` (set by load_clip_model for ``disable_lora: true``): every parameter is trained."""
    return bool(getattr(module, "hip_full_ft", False))


def _park_engine(m):
    """Drop module ``m``'s engine now; its flat buffer goes to the engine that the next forward builds (_engine_for)."""
    if getattr(m, "_engine", None) is not None:
        m._engine_prev = m._engine
    m._engine = None


def _engine_for(module, build):
    """The module's engine, rebuilt (``build(mode, reuse_flat)``) when it was made for another mode than the one wanted now, when its
    parameters left the flat buffer (``.to()``) or when the frozen weights it packed were overwritten (a checkpoint loaded later)."""
    eng, mode = getattr(module, "_engine", None), wanted_mode(module)
    if eng is None or eng.mode != mode or not eng.flat.valid() or _frozen_signature(module, eng) != eng._frozen_sig:
        if not torch.cuda.is_available():
            raise RuntimeError("bioscanclip needs a ROCm GPU: all arithmetic runs in libbsclip_hip.so "
                               "(there is no CPU/torch fallback)")
        old = eng or getattr(module, "_engine_prev", None)
        eng = build(mode, old.flat if old is not None and old.flat.valid() else None)
        eng._frozen_sig = _frozen_signature(module, eng)
        module._engine, module._engine_prev = eng, None
    return eng


def run_encoder(module, build, fwd_args):
    if wants_fp16(module):
        _check_fp16(module)
    eng = _engine_for(module, build)
    eng.training, eng._owner = module.training, module
    # the engine keeps ONE set of saved activations (its workspace): any later forward of the same encoder, with or without
    # autograd, overwrites them -- _EncoderFn.backward checks that it still owns them
    eng._fwd_generation += 1
    if torch.is_grad_enabled() and any(p.requires_grad for p in eng.flat.params):
        return _EncoderFn.apply(eng, fwd_args, *eng.flat.params)
    out = eng.forward(*fwd_args)
    if DETECT_ANOMALY:
        _anomaly_check(eng, "forward", out)
    return out
