"""Autograd nodes for the small ops outside the encoders: F.normalize, the contrastive loss and the supervised fine-tuning
head (Linear + cross-entropy)."""
import torch

from . import ops

F32 = torch.float32


class _L2Normalize(torch.autograd.Function):
    """``F.normalize(x, p=2, dim=-1)`` (reference simple_clip.py:34,47,49) on the HIP kernel."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        inv = torch.empty(x.shape[0], dtype=F32, device=x.device)
        ops.l2norm_fwd(x, y, inv)
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        dx = torch.empty_like(y)
        ops.l2norm_bwd(y, inv, dy.contiguous(), dx)
        return dx


def l2_normalize(x):
    if not x.is_cuda:
        raise RuntimeError("bioscanclip: tensors must live on the GPU (no CPU compute path)")
    return _L2Normalize.apply(x.to(F32))


class _InfoNCE(torch.autograd.Function):
    """ContrastiveLoss.forward (reference loss_func.py:29-54): loss and dLoss/dz come out of one fused call; the
    backward of this node only scales the stored gradients by the incoming scalar."""

    @staticmethod
    def forward(ctx, labels, scale, row0, n_local, workspace, *zs):
        zs = [z.contiguous() for z in zs]
        N = zs[0].shape[0]
        n_local = N if n_local is None else n_local
        loss = torch.zeros(1, dtype=F32, device=zs[0].device)
        need_grad = any(ctx.needs_input_grad[5:])
        dzs = [torch.empty(n_local, z.shape[1], dtype=F32, device=z.device) for z in zs] if need_grad else None
        ops.infonce_fwd_bwd(zs, labels, scale, loss, dzs, row0=row0, n_local=n_local, workspace=workspace)
        ctx.dzs, ctx.row0, ctx.N = dzs, row0, N
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        outs = []
        for d in ctx.dzs:
            if d.shape[0] == ctx.N:
                outs.append(d * g)
            else:  # gathered batch: only the local rows carry gradient
                full = torch.zeros(ctx.N, d.shape[1], dtype=F32, device=d.device)
                full[ctx.row0:ctx.row0 + d.shape[0]] = d * g
                outs.append(full)
        return (None, None, None, None, None) + tuple(outs)


class _InfoNCETrainableScale(torch.autograd.Function):
    """``_InfoNCE`` with a learnable temperature: ``log_scale`` is t = log(scale), one f32 on the GPU that the kernels read when they
    run (``bsclip_infonce_fwd_bwd_ts``).  The same call leaves dLoss/dt next to dLoss/dz; the returned loss carries ``scale_out``
    = (dLoss/dt of the own rows, the scale used) for logging."""

    @staticmethod
    def forward(ctx, labels, log_scale, row0, n_local, workspace, scale_out, *zs):
        zs = [z.contiguous() for z in zs]
        N = zs[0].shape[0]
        n_local = N if n_local is None else n_local
        loss = torch.zeros(1, dtype=F32, device=zs[0].device)
        need_grad = ctx.needs_input_grad[1] or any(ctx.needs_input_grad[6:])
        dzs = [torch.empty(n_local, z.shape[1], dtype=F32, device=z.device) for z in zs] if need_grad else None
        ops.infonce_fwd_bwd_ts(zs, labels, log_scale, loss, dzs, scale_out, row0=row0, n_local=n_local, workspace=workspace)
        ctx.dzs, ctx.row0, ctx.N, ctx.scale_out, ctx.t_shape = dzs, row0, N, scale_out, log_scale.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        outs = []
        for i, d in enumerate(ctx.dzs):
            if not ctx.needs_input_grad[6 + i]:
                outs.append(None)
            elif d.shape[0] == ctx.N:
                outs.append(d * g)
            else:  # gathered batch: only the local rows carry gradient
                full = torch.zeros(ctx.N, d.shape[1], dtype=F32, device=d.device)
                full[ctx.row0:ctx.row0 + d.shape[0]] = d * g
                outs.append(full)
        dt = (ctx.scale_out[0] * g).reshape(ctx.t_shape) if ctx.needs_input_grad[1] else None
        return (None, dt, None, None, None, None) + tuple(outs)


_WS = {}


def _workspace(N, nmod, device):
    key = (N, nmod, str(device))
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(ops.infonce_workspace_floats(N, nmod), dtype=F32, device=device)
        _WS.clear()
        _WS[key] = ws
    return ws


def infonce(zs, labels, scale, row0=0, n_local=None):
    if len(zs) < 2:
        raise ValueError("Too less element for calculating the contrastive loss.")
    if not zs[0].is_cuda:
        raise RuntimeError("bioscanclip: tensors must live on the GPU (no CPU compute path)")
    ws = _workspace(zs[0].shape[0], len(zs), zs[0].device)
    if torch.is_tensor(scale):   # a learnable temperature: ``scale`` is its logarithm, read on the device
        if not (scale.is_cuda and scale.dtype == F32 and scale.numel() == 1):
            raise ValueError("infonce: a tensor scale is the log scale, a 1-element f32 CUDA tensor")
        scale_out = torch.empty(2, dtype=F32, device=zs[0].device)
        loss = _InfoNCETrainableScale.apply(labels.to(torch.int64).contiguous(), scale, row0, n_local, ws, scale_out,
                                            *[z.to(F32) for z in zs])
        loss.scale_out = scale_out   # (dLoss/dt of the own rows, the scale used)
        return loss
    return _InfoNCE.apply(labels.to(torch.int64).contiguous(), float(scale), row0, n_local, ws, *[z.to(F32) for z in zs])


class MemoryBank:
    """The device state of a cross-batch memory: one f32 bank per modality (``ops.xbm_bank_floats(Q)`` elements; the first
    Q * 768 are the normalised rows by slot), the slots' labels (int64 [Q]) and ``state`` = (head, filled) as int32 [2].  Plain
    references: the owner (``MemoryBankContrastiveLoss``) allocates them and keeps them alive."""

    def __init__(self, banks, labels, state):
        self.banks, self.labels, self.state = list(banks), labels, state
        self.Q = labels.numel()
        self._ws = {}

    def workspace(self, N, nmod):
        """The workspace of the loss and enqueue calls at batch size N, kept per shape for the bank's lifetime: a captured step holds
        a pointer into it."""
        ws = self._ws.get((N, nmod))
        if ws is None:
            ws = self._ws[(N, nmod)] = torch.empty(ops.xbm_workspace_floats(N, self.Q, nmod), dtype=F32, device=self.labels.device)
        return ws

    def rows(self, m):
        """The documented f32 rows of modality ``m`` as a [Q, 768] view."""
        return self.banks[m][:self.Q * 768].view(self.Q, 768)


class _InfoNCEXbm(torch.autograd.Function):
    """InfoNCE with the valid slots of a cross-batch memory as extra key columns (``bsclip_infonce_xbm_fwd_bwd``).  ``log_scale``
    is t = log(scale), one f32 on the GPU; the bank takes no gradient; dLoss/dt comes out of the same call in ``scale_out``."""

    @staticmethod
    def forward(ctx, labels, log_scale, bank, workspace, scale_out, *zs):
        zs = [z.contiguous() for z in zs]
        loss = torch.zeros(1, dtype=F32, device=zs[0].device)
        need_grad = ctx.needs_input_grad[1] or any(ctx.needs_input_grad[5:])
        dzs = [torch.empty_like(z) for z in zs] if need_grad else None
        ops.infonce_xbm(zs, labels, log_scale, bank.banks, bank.labels, bank.state, loss, dzs, scale_out, workspace)
        ctx.dzs, ctx.scale_out, ctx.t_shape = dzs, scale_out, log_scale.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        outs = [d * g if ctx.needs_input_grad[5 + i] else None for i, d in enumerate(ctx.dzs)]
        dt = (ctx.scale_out[0] * g).reshape(ctx.t_shape) if ctx.needs_input_grad[1] else None
        return (None, dt, None, None, None) + tuple(outs)


def infonce_xbm(zs, labels, log_scale, bank):
    """The InfoNCE of ``infonce`` over the current batch AND the valid slots of ``bank`` (a ``MemoryBank``), read as it stands:
    nothing is enqueued here.  ``log_scale`` is a 1-element f32 CUDA tensor holding t = log(scale) -- the model's parameter when the
    temperature is learnable (it then receives dLoss/dt), a plain device word otherwise.  The returned loss carries ``scale_out`` =
    (dLoss/dt, the scale used)."""
    if len(zs) < 2:
        raise ValueError("Too less element for calculating the contrastive loss.")
    if not zs[0].is_cuda:
        raise RuntimeError("bioscanclip: tensors must live on the GPU (no CPU compute path)")
    if not (torch.is_tensor(log_scale) and log_scale.is_cuda and log_scale.dtype == F32 and log_scale.numel() == 1):
        raise ValueError("infonce_xbm: log_scale is the log scale, a 1-element f32 CUDA tensor")
    ws = bank.workspace(zs[0].shape[0], len(zs))
    scale_out = torch.empty(2, dtype=F32, device=zs[0].device)
    loss = _InfoNCEXbm.apply(labels.to(torch.int64).contiguous(), log_scale, bank, ws, scale_out, *[z.to(F32) for z in zs])
    loss.scale_out = scale_out
    return loss


def xbm_enqueue(zs, labels, bank):
    """Write the (detached) rows of ``zs`` and their labels into ``bank`` and advance its ring, all on the device."""
    zs = [z.detach().to(F32).contiguous() for z in zs]
    ws = bank.workspace(zs[0].shape[0], len(zs))
    ops.xbm_enqueue(zs, labels.to(torch.int64).contiguous(), bank.banks, bank.labels, bank.state, ws)


class _SigmoidLoss(torch.autograd.Function):
    """The sigmoid (SigLIP) loss with a learnable scale and bias (``bsclip_sigmoid_loss_fwd_bwd``): ``log_scale`` (t) and ``bias``
    (b) are one f32 each on the GPU, read by the kernels when they run.  One call leaves the loss, dLoss/dz and, in ``aux_out``,
    (dLoss/dt of the own rows, the scale used, dLoss/db of the own rows, b); the backward only scales them."""

    @staticmethod
    def forward(ctx, labels, log_scale, bias, row0, n_local, workspace, aux_out, *zs):
        zs = [z.contiguous() for z in zs]
        N = zs[0].shape[0]
        n_local = N if n_local is None else n_local
        loss = torch.zeros(1, dtype=F32, device=zs[0].device)
        need_grad = ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or any(ctx.needs_input_grad[7:])
        dzs = [torch.empty(n_local, z.shape[1], dtype=F32, device=z.device) for z in zs] if need_grad else None
        ops.sigmoid_loss_fwd_bwd(zs, labels, log_scale, bias, loss, dzs, aux_out, row0=row0, n_local=n_local, workspace=workspace)
        ctx.dzs, ctx.row0, ctx.N, ctx.aux_out, ctx.t_shape, ctx.b_shape = dzs, row0, N, aux_out, log_scale.shape, bias.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        outs = []
        for i, d in enumerate(ctx.dzs):
            if not ctx.needs_input_grad[7 + i]:
                outs.append(None)
            elif d.shape[0] == ctx.N:
                outs.append(d * g)
            else:  # gathered batch: only the local rows carry gradient
                full = torch.zeros(ctx.N, d.shape[1], dtype=F32, device=d.device)
                full[ctx.row0:ctx.row0 + d.shape[0]] = d * g
                outs.append(full)
        dt = (ctx.aux_out[0] * g).reshape(ctx.t_shape) if ctx.needs_input_grad[1] else None
        db = (ctx.aux_out[2] * g).reshape(ctx.b_shape) if ctx.needs_input_grad[2] else None
        return (None, dt, db, None, None, None, None) + tuple(outs)


def sigmoid_loss(zs, labels, log_scale, bias, row0=0, n_local=None):
    """loss = 1/(P N) sum over the directed modality pairs and the cells (i, j) of softplus(-y_ij (s zn^a_i . zn^b_j + b)), with
    s = exp(clamp(log_scale, 0, ln 100)) and y = +1 where the labels agree, -1 elsewhere.  The returned loss carries ``aux_out`` =
    (dLoss/dt of the own rows, s, dLoss/db of the own rows, b)."""
    if len(zs) < 2:
        raise ValueError("Too less element for calculating the contrastive loss.")
    if not zs[0].is_cuda:
        raise RuntimeError("bioscanclip: tensors must live on the GPU (no CPU compute path)")
    for name, v in (("log_scale", log_scale), ("bias", bias)):
        if not (torch.is_tensor(v) and v.is_cuda and v.dtype == F32 and v.numel() == 1):
            raise ValueError(f"sigmoid_loss: {name} must be a 1-element f32 CUDA tensor")
    ws = _workspace(zs[0].shape[0], len(zs), zs[0].device)
    aux_out = torch.empty(4, dtype=F32, device=zs[0].device)
    loss = _SigmoidLoss.apply(labels.to(torch.int64).contiguous(), log_scale, bias, row0, n_local, ws, aux_out,
                              *[z.to(F32) for z in zs])
    loss.aux_out = aux_out
    return loss


# ---- supervised fine-tuning head: Linear(768, C) + CrossEntropyLoss (reference util.py:13-25, fine_tuning_epoch.py:27) ----------
HEAD_D = 768


def _pad(n, m):
    return (n + m - 1) // m * m


class _HeadWorkspace:
    """Scratch of one (B, C) head call: the split-bf16 operands of the three products and the padded logits.  Everything in here is
    dead once the call that filled it returns (forward) or finishes (backward); what a backward needs from its forward -- dlogits
    in both forms -- is allocated per call, because two classifiers of one (B, C) have their forwards queued before either backward."""

    def __init__(self, B, C, device):
        D = HEAD_D
        self.Cn, self.Ck, self.Bp = _pad(C, 128), _pad(C, 64), _pad(B, 64)   # GEMM N, the dz product's K, the dW product's K
        bf, f32 = torch.bfloat16, F32
        self.z3 = torch.empty(B, 3 * D, dtype=bf, device=device)
        # rows / elements [C, Cn) are never written: the GEMM forms logits for them that every reader masks out
        self.w3 = torch.zeros(self.Cn, 3 * D, dtype=bf, device=device)
        self.bias = torch.zeros(self.Cn, dtype=f32, device=device)
        self.logits = torch.empty(B, self.Cn, dtype=f32, device=device)
        self.row_loss = torch.empty(B, dtype=f32, device=device)
        self.wT3 = torch.empty(D * 3 * self.Ck, dtype=bf, device=device)
        self.zT3 = torch.empty(D * 3 * self.Bp, dtype=bf, device=device)
        self.dT3 = torch.empty(C * 3 * self.Bp, dtype=bf, device=device)
        # dW[C, 768] reduces over K = 3 Bp columns -- the hi.hi, lo.hi and hi.lo terms, Bp each: from four 64-wide K-tiles per term up
        # each term is a K range (workgroup) of its own, unless that would be more than two rounds of workgroups over the chip
        tiles = -(-C // 256) * (D // 256)
        self.splits = 3 if self.Bp >= 256 and 3 * tiles <= 512 else 1
        self.partial = torch.empty(self.splits * C * D, dtype=f32, device=device)
        self.db = torch.empty(C, dtype=f32, device=device)


_HEAD_WS = {}
_CE_FLAG = {}


def _head_workspace(B, C, device):
    # one workspace per launching stream, as ops._lora_grad_workspace: classifiers may be driven from streams of their own
    key = (B, C, str(device), torch.cuda.current_stream().cuda_stream)
    ws = _HEAD_WS.get(key)
    if ws is None:
        ws = _HEAD_WS[key] = _HeadWorkspace(B, C, device)
    return ws


def ce_flag(device):
    """The int32 device word ``linear_cross_entropy`` ORs its out-of-range-target bit into when the caller passes none."""
    key = str(torch.device(device))
    if key not in _CE_FLAG:
        _CE_FLAG[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _CE_FLAG[key]


def _head_inputs(z, weight, bias):
    if not (z.is_cuda and weight.is_cuda and bias.is_cuda):
        raise RuntimeError("bioscanclip: tensors must live on the GPU (no CPU compute path)")
    if z.dim() != 2 or z.shape[1] != HEAD_D or weight.dim() != 2 or weight.shape[1] != HEAD_D or tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"classifier head: z [B, {HEAD_D}], weight [C, {HEAD_D}], bias [C] expected, got {tuple(z.shape)}, "
                         f"{tuple(weight.shape)}, {tuple(bias.shape)}")
    if weight.dtype != F32 or bias.dtype != F32 or not weight.is_contiguous() or not bias.is_contiguous():
        raise ValueError("classifier head: weight and bias must be contiguous f32 (fp16 / fp8 operand modes are not built for the head)")
    if z.shape[0] < 1 or weight.shape[0] < 1:
        raise ValueError("classifier head: B >= 1 and C >= 1")


def _head_logits(z, weight, bias, ws, out):
    """out[:B, :Cn] = z W^T + b on the split-bf16 GEMM (hi.hi + lo.hi + hi.lo: ~2^-16 per product)."""
    C = weight.shape[0]
    ops.split3_rows(z, ws.z3)
    ops.split3_weight(weight, ws.w3[:C])
    ws.bias[:C].copy_(bias)
    ops.gemm(ws.z3, ws.w3, out, epilogue=ops.EPI_F32, bias=ws.bias)


def linear_logits(z, weight, bias):
    """``F.linear(z, weight, bias)`` for the classifier head without autograd (evaluation): f32 [B, C], a view into a freshly
    allocated padded buffer [B, C rounded up to 128] -- the layout ``ops.class_topk`` and ``ops.ce_fwd_bwd`` read."""
    _head_inputs(z, weight, bias)
    z = z.detach().to(F32).contiguous()
    B, C = z.shape[0], weight.shape[0]
    ws = _head_workspace(B, C, z.device)
    out = torch.empty(B, ws.Cn, dtype=F32, device=z.device)
    _head_logits(z, weight.detach(), bias.detach(), ws, out)
    return out[:, :C]


class _LinearCrossEntropy(torch.autograd.Function):
    """``F.cross_entropy(F.linear(z, W, b), target)``: the forward forms the logits and, in one pass over them, the loss and
    dlogits; the backward is the three products.  dW and db are accumulated in place into ``.grad`` (``None`` is returned for
    them), as the encoders' nodes do; dz goes back through autograd."""

    @staticmethod
    def forward(ctx, z, weight, bias, target, flag, ws):
        B, C = z.shape[0], weight.shape[0]
        _head_logits(z, weight, bias, ws, ws.logits)
        loss = torch.empty(1, dtype=F32, device=z.device)
        dl = dl3 = None
        if any(ctx.needs_input_grad[:3]):
            dl = torch.empty(B, ws.Cn, dtype=F32, device=z.device)
            dl3 = torch.empty(B, 3 * ws.Ck, dtype=torch.bfloat16, device=z.device)
        ops.ce_fwd_bwd(ws.logits, target, C, loss, ws.row_loss, dl, dl3, flag)
        ctx.save_for_backward(z, weight)
        ctx.dl, ctx.dl3, ctx.ws, ctx.bias = dl, dl3, ws, bias
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        z, weight = ctx.saved_tensors
        dl, dl3, ws, bias = ctx.dl, ctx.dl3, ctx.ws, ctx.bias
        B, C = z.shape[0], weight.shape[0]
        dz = None
        # the incoming scalar scales the small side of every product (as _InfoNCE.backward scales its stored gradients)
        if ctx.needs_input_grad[0]:
            wT3 = ops.split3_transpose(weight, ws.wT3, 1)                    # W^T as the B operand: [768, 3 Ck], [hi | hi | lo]
            dz = torch.empty(B, HEAD_D, dtype=F32, device=z.device)
            ops.gemm(dl3, wT3, dz, epilogue=ops.EPI_F32)
            dz = dz * g
        if ctx.needs_input_grad[1]:
            if weight.grad is None:
                weight.grad = torch.zeros_like(weight)
            zT3 = ops.split3_transpose(z * g, ws.zT3, 1)                     # [768, 3 Bp], zeros in the padded rows' columns
            dT3 = ops.split3_transpose(dl[:, :C], ws.dT3, 0)                 # dlogits^T: [C, 3 Bp], [hi | lo | hi]
            ops.gemm_splitk_f32(dT3, zT3, weight.grad, ws.splits, ws.partial, K=3 * ws.Bp)
        if ctx.needs_input_grad[2]:
            if bias.grad is None:
                bias.grad = torch.zeros_like(bias)
            ws.db.zero_()
            ops.colsum(dl, B, C, ws.db)
            bias.grad.addcmul_(ws.db, g)
        return dz, None, None, None, None, None


def linear_cross_entropy(z, weight, bias, target, flag=None):
    """Mean cross-entropy of ``z @ weight.T + bias`` against integer ``target`` [B] as one autograd node (the fused path of
    ``EncoderWithExtraLayer.loss``).  No host synchronisation: a target outside [0, C) contributes zero loss and zero gradient and
    sets bit 0 of ``flag`` (int32 [1] on the GPU; default: the per-device word ``ce_flag(device)``), which the caller reads when it
    chooses to -- the epoch drivers do once per epoch."""
    _head_inputs(z, weight, bias)
    if target.dim() != 1 or target.shape[0] != z.shape[0] or target.dtype not in (torch.int32, torch.int64):
        raise ValueError("linear_cross_entropy: target must be an integer tensor [B]")
    z = z.to(F32).contiguous()
    ws = _head_workspace(z.shape[0], weight.shape[0], z.device)
    flag = ce_flag(z.device) if flag is None else flag
    return _LinearCrossEntropy.apply(z, weight, bias, target.to(z.device, torch.int32).contiguous(), flag, ws)
