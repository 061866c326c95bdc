"""Contrastive loss -- drop-in for reference ``bioscanclip/model/loss_func.py`` (``construct_label_metrix``,
``ContrastiveLoss``) plus the global-batch form north_star asks for (semantics of ``gather_features`` /
``ClipLoss`` with gather_with_grad=False, local_loss=False: loss_func.py:58-91,117-165).

The arithmetic is the fused HIP InfoNCE (``bsclip_infonce_fwd_bwd``): soft-target CE over every ordered modality
pair, second ``F.normalize`` applied inside (loss_func.py:43-44).  The temperature is fixed at construction (a float) or
learnable: an ``nn.Parameter`` holding t = log(scale), which the kernels read on the device (``bsclip_infonce_fwd_bwd_ts``).

``SigmoidContrastiveLoss`` is a second criterion with the same call signature: the pairwise sigmoid loss of SigLIP on a learnable
scale and bias (``bsclip_sigmoid_loss_fwd_bwd``, ``model_config.contrastive_loss: sigmoid``).

``MemoryBankContrastiveLoss`` is ``ContrastiveLoss`` with a cross-batch memory (``model_config.memory_bank_size``): the embeddings of
the last steps stay on the GPU and enter the InfoNCE as extra key columns without gradient (``bsclip_infonce_xbm_fwd_bwd``).
"""
import math

import torch
import torch.nn as nn

from bioscanclip.hip.functional import MemoryBank, infonce, infonce_xbm, sigmoid_loss, xbm_enqueue


def construct_label_metrix(labels):
    """Reference loss_func.py:18-21.  Kept for API compatibility (index compare only, no float math); the HIP
    loss builds the same 0/1 targets on the fly from the label vector."""
    matrix = (labels.unsqueeze(0) == labels.unsqueeze(1)).float()
    return matrix


class ContrastiveLoss(nn.Module):
    def __init__(self, criterion=None, logit_scale=1 / 0.07):
        super(ContrastiveLoss, self).__init__()
        # ``criterion`` is nn.CrossEntropyLoss() in the reference (train_cl.py:190); its soft-target form is what the
        # kernel implements.  Anything else cannot be honoured by the fused kernel.
        if criterion is not None and not isinstance(criterion, nn.CrossEntropyLoss):
            raise TypeError("ContrastiveLoss: the HIP path implements nn.CrossEntropyLoss() with soft targets only")
        self.criterion = criterion
        # a float, or an nn.Parameter holding t = log(scale) (model.logit_scale: the model owns it, its optimizer updates it).  Kept
        # out of this module's own parameters, so that the criterion adds nothing to a state dict or an optimizer.
        object.__setattr__(self, "logit_scale", logit_scale)
        self._scale_out = None

    def current_scale(self):
        """The logit scale as a device scalar tensor: for a learnable temperature the scale the last forward used (before any
        forward, exp(clamp(t, 0, ln 100)) of the parameter's present value), the fixed float otherwise."""
        t = self.logit_scale
        if not torch.is_tensor(t):
            dev = "cuda" if torch.cuda.is_available() else "cpu"
            return torch.tensor(float(t), dtype=torch.float32, device=dev)
        if self._scale_out is not None:
            return self._scale_out[1]
        return t.detach().float().clamp(0.0, 4.605170185988092).exp().reshape(())

    def _infonce(self, feats, labels, **kw):
        loss = infonce(feats, labels, self.logit_scale, **kw)
        self._scale_out = getattr(loss, "scale_out", None)
        return loss

    def forward(self, image_features, dna_features, text_features, label, logit_scale=1 / 0.07):
        # the per-call ``logit_scale`` argument is ignored, as in the reference (loss_func.py:46-47 use self.logit_scale)
        feature_list = [image_features, dna_features, text_features]
        feature_list = [item for item in feature_list if item is not None]
        if len(feature_list) < 2:
            raise ValueError("Too less element for calculating the contrastive loss.")
        return self._infonce(feature_list, label)


class SigmoidContrastiveLoss(nn.Module):
    """The pairwise sigmoid loss of SigLIP (Zhai et al., ICCV 2023) over every modality pair, with ``ContrastiveLoss``'s call
    signature: every cell (i, j) is a binary decision "same label or not" on x = s cos(i, j) + b, so several positives per row
    need no soft targets and nothing is normalised over the batch.  ``logit_scale`` (t = log s, clamped to [0, ln 100]) and
    ``logit_bias`` (b) are the model's ``nn.Parameter``s (``model_config.contrastive_loss: sigmoid``); the kernels read them on the
    device (``bsclip_sigmoid_loss_fwd_bwd``).  One rank only: ``world_size`` is the process group's size when not given."""

    def __init__(self, logit_scale, logit_bias, world_size=None):
        super().__init__()
        if world_size is None:
            import torch.distributed as dist
            world_size = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world_size > 1:
            raise ValueError(f"SigmoidContrastiveLoss: the sigmoid loss is not built for more than one rank (world_size={world_size})")
        for name, v in (("logit_scale", logit_scale), ("logit_bias", logit_bias)):
            if not (torch.is_tensor(v) and v.numel() == 1):
                raise TypeError(f"SigmoidContrastiveLoss: {name} is a 1-element tensor (the model's parameter)")
        # the model owns both: kept out of this module's own parameters, as ContrastiveLoss keeps its learnable temperature
        object.__setattr__(self, "logit_scale", logit_scale)
        object.__setattr__(self, "logit_bias", logit_bias)
        self._aux_out = None

    def current_scale(self):
        """The scale the last forward used, as a device scalar (before any forward, exp(clamp(t, 0, ln 100)) of the parameter)."""
        if self._aux_out is not None:
            return self._aux_out[1]
        return self.logit_scale.detach().float().clamp(0.0, 4.605170185988092).exp().reshape(())

    def current_bias(self):
        """The bias the last forward used, as a device scalar (before any forward, the parameter's present value)."""
        if self._aux_out is not None:
            return self._aux_out[3]
        return self.logit_bias.detach().float().reshape(())

    def forward(self, image_features, dna_features, text_features, label):
        feature_list = [item for item in (image_features, dna_features, text_features) if item is not None]
        if len(feature_list) < 2:
            raise ValueError("Too less element for calculating the contrastive loss.")
        loss = sigmoid_loss(feature_list, label, self.logit_scale, self.logit_bias)
        self._aux_out = loss.aux_out
        return loss


def check_memory_bank_size(Q, batch_size=None):
    """``model_config.memory_bank_size`` as an int, or ValueError: a multiple of 256 in [256, 16384], at least the batch size."""
    if isinstance(Q, bool) or not isinstance(Q, int):
        raise ValueError(f"memory_bank_size={Q!r}: an integer number of slots")
    if Q % 256 != 0 or not 256 <= Q <= 16384:
        raise ValueError(f"memory_bank_size={Q}: a multiple of 256 in 256 .. 16384")
    if batch_size is not None and Q < batch_size:
        raise ValueError(f"memory_bank_size={Q} is smaller than the batch size {batch_size}: a step's rows must fit the ring")
    return Q


class MemoryBankContrastiveLoss(ContrastiveLoss):
    """``ContrastiveLoss`` over the current batch and a cross-batch memory (XBM, Wang et al., CVPR 2020): the normalised embeddings
    of the last steps, ``memory_bank_size`` slots per modality in a ring on the GPU, are extra key columns of every ordered pair's
    logits and take no gradient.  In train mode a forward computes the loss on the bank as it stands and THEN enqueues the detached
    current embeddings, so a sample never meets its own copy in the step that wrote it; in eval mode it reads the bank and enqueues
    nothing.  Ring position and fill count live on the device and every launch reads them there, so the step can be captured.

    The banks, their labels and the state are non-persistent buffers, allocated on first use for the modalities present: they are
    in no state dict and no checkpoint, and a restarted run refills the bank in memory_bank_size / batch steps.  ``logit_scale``
    is a float or the model's learnable ``nn.Parameter`` (t = log scale).  One rank only: ``world_size`` is the process group's
    size when not given."""

    def __init__(self, criterion=None, logit_scale=1 / 0.07, memory_bank_size=4096, world_size=None):
        if world_size is None:
            import torch.distributed as dist
            world_size = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world_size > 1:
            raise ValueError(f"MemoryBankContrastiveLoss: the cross-batch memory is not built for more than one rank (world_size={world_size})")
        super().__init__(criterion, logit_scale)
        self.memory_bank_size = check_memory_bank_size(memory_bank_size)
        self._bank = None
        self._present = None

    def _allocate(self, present, device):
        from bioscanclip.hip import ops
        Q = self.memory_bank_size
        n = ops.xbm_bank_floats(Q)
        for name in present:
            self.register_buffer(f"bank_{name}", torch.zeros(n, dtype=torch.float32, device=device), persistent=False)
        self.register_buffer("bank_labels", torch.zeros(Q, dtype=torch.int64, device=device), persistent=False)
        self.register_buffer("bank_state", torch.zeros(2, dtype=torch.int32, device=device), persistent=False)   # (head, filled)
        if not torch.is_tensor(self.logit_scale):   # the fixed temperature as the device word the kernels read
            self.register_buffer("log_scale_word", torch.tensor([math.log(float(self.logit_scale))], dtype=torch.float32, device=device),
                                 persistent=False)
        self._bank = MemoryBank([getattr(self, f"bank_{name}") for name in present], self.bank_labels, self.bank_state)
        self._present = present

    def bank(self):
        """The ``MemoryBank`` (None before the first forward)."""
        return self._bank

    def reset(self):
        """Empty the bank: head = filled = 0 (the slots' contents stop mattering)."""
        if self._bank is not None:
            self.bank_state.zero_()

    def filled(self):
        """The number of valid slots as a device scalar (no host synchronisation)."""
        if self._bank is None:
            return torch.zeros((), dtype=torch.int32)
        return self.bank_state[1]

    def forward(self, image_features, dna_features, text_features, label, logit_scale=1 / 0.07):
        named = [(n, f) for n, f in (("image", image_features), ("dna", dna_features), ("text", text_features)) if f is not None]
        if len(named) < 2:
            raise ValueError("Too less element for calculating the contrastive loss.")
        present, feats = tuple(n for n, _ in named), [f for _, f in named]
        if not feats[0].is_cuda:
            raise RuntimeError("bioscanclip: tensors must live on the GPU (no CPU compute path)")
        if self._bank is None:
            self._allocate(present, feats[0].device)
        elif present != self._present:
            raise ValueError(f"MemoryBankContrastiveLoss: the bank holds {self._present}, this batch has {present}")
        t = self.logit_scale if torch.is_tensor(self.logit_scale) else self.log_scale_word
        loss = infonce_xbm(feats, label, t, self._bank)
        self._scale_out = loss.scale_out
        if self.training:
            xbm_enqueue(feats, label, self._bank)
        return loss


class GlobalBatchContrastiveLoss(ContrastiveLoss):
    """Global-batch loss over an all-gathered batch: every rank gathers all ranks' embeddings and
    labels (RCCL all_gather over xGMI, issued per modality from its tower's stream in SimpleCLIP.forward and only
    waited for here), evaluates the full N x N loss
    redundantly and keeps dLoss/dz for its own rows only; the caller all-reduces (SUM) the flat trainable
    gradients.  Equivalent to the single-process loss on the concatenated batch."""

    def __init__(self, criterion=None, logit_scale=1 / 0.07, group=None, overlap=True):
        if torch.is_tensor(logit_scale):
            raise ValueError("GlobalBatchContrastiveLoss: a trainable temperature is not built for more than one rank")
        super().__init__(criterion, logit_scale)
        self.group = group
        if overlap:  # all-gathers from the tower streams, gradient all-reduces from the encoder nodes (hip/dist.py)
            from bioscanclip.hip.dist import enable_overlap
            enable_overlap(group)

    def prefetch_labels(self, label):
        """Start the label all-gather at the top of the step (train_epoch calls this before the encoders run)."""
        from bioscanclip.hip.dist import start_label_gather
        start_label_gather(label)

    def forward(self, image_features, dna_features, text_features, label, logit_scale=1 / 0.07):
        from bioscanclip.hip.dist import gather_features_and_labels
        feats = [f for f in (image_features, dna_features, text_features) if f is not None]
        if len(feats) < 2:
            raise ValueError("Too less element for calculating the contrastive loss.")
        gathered, labels, row0 = gather_features_and_labels(feats, label, self.group)
        return infonce(gathered, labels, self.logit_scale, row0=row0, n_local=feats[0].shape[0])
