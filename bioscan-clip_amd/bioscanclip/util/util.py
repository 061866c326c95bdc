"""Checkpoint helpers with the reference's names (bioscanclip/util/util.py:72-84) and ``EncoderWithExtraLayer`` (:13-25), the
species classifier of supervised fine-tuning.  The rest of the reference's util.py (result tables, plotting colours, faiss
helper) is control plane and not rebuilt."""
import torch
import torch.nn as nn


class EncoderWithExtraLayer(nn.Module):
    """An encoder of a trained model with a new ``nn.Linear(768, C)`` on its output (reference util.py:13-25): same constructor,
    same ``get_feature`` / ``forward`` signatures, same ``state_dict`` keys (``encoder.*``, ``new_linear_layer.weight`` / ``.bias``).

    ``forward(x)`` returns the logits [B, C] from the HIP head (``hip.functional.linear_logits``); it carries no autograd graph,
    so it serves evaluation.  Training goes through ``loss(x, target)``, the fast path: logits, cross-entropy and dlogits in one
    fused call and the three backward products on the HIP GEMMs (``hip.functional.linear_cross_entropy``).  There is no torch
    compute path: calling ``forward`` where a gradient would be recorded raises instead of silently training through ``nn.Linear``."""

    def __init__(self, encoder, new_linear_layer):
        super().__init__()
        if not isinstance(new_linear_layer, nn.Linear) or new_linear_layer.bias is None:
            raise NotImplementedError("EncoderWithExtraLayer: new_linear_layer must be an nn.Linear with a bias (the MLP + Softmax head of "
                                      "SimpleCLIPWithClassificationHead is not built)")
        self.encoder = encoder
        self.new_linear_layer = new_linear_layer

    def get_feature(self, x):
        return self.encoder(x)

    def forward(self, x):
        from bioscanclip.hip import functional as HF
        lin = self.new_linear_layer
        if torch.is_grad_enabled() and (lin.weight.requires_grad or any(p.requires_grad for p in self.encoder.parameters())):
            raise RuntimeError("EncoderWithExtraLayer.forward returns logits without an autograd graph: call it under torch.no_grad() "
                               "(evaluation) and train through .loss(x, target), the fused HIP path")
        return HF.linear_logits(self.encoder(x), lin.weight, lin.bias)

    def loss(self, x, target, flag=None):
        """Mean cross-entropy of the classifier on batch ``x`` against integer ``target`` [B]: the fused fast path (one autograd
        node for the head).  ``flag``: see ``hip.functional.linear_cross_entropy``."""
        from bioscanclip.hip import functional as HF
        lin = self.new_linear_layer
        return HF.linear_cross_entropy(self.encoder(x), lin.weight, lin.bias, target, flag=flag)


def remove_extra_pre_fix(state_dict):
    """Strip the ``module.`` prefix DataParallel/DDP checkpoints carry (util.py:72-78)."""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def load_bert_model(bert_model, path_to_ckpt):
    """util.py:81-84: load a (possibly ``module.``-prefixed) checkpoint into a BERT parameter tree, strictly."""
    state_dict = torch.load(path_to_ckpt, map_location=torch.device("cpu"))
    bert_model.load_state_dict(remove_extra_pre_fix(state_dict))


def load_checked(module, state_dict, what, allow_missing=(), allow_unexpected=()):
    """``load_state_dict`` that refuses a checkpoint which does not cover the module: the reference loads strictly
    (util.py:81-84); a silently half-loaded trunk would train on random weights.  ``allow_*``: key prefixes that may be
    absent / extra (e.g. a classifier head that is replaced right after, HF's ``position_ids`` buffer)."""
    res = module.load_state_dict(state_dict, strict=False)
    missing = [k for k in res.missing_keys if not any(k.startswith(a) for a in allow_missing)]
    unexpected = [k for k in res.unexpected_keys if not any(k.startswith(a) for a in allow_unexpected)]
    if missing or unexpected:
        raise RuntimeError(f"{what}: checkpoint does not match the parameter tree -- missing {missing[:8]} "
                           f"({len(missing)} keys), unexpected {unexpected[:8]} ({len(unexpected)} keys)")
    return res


def load_model_and_checkpoint(args, device, ckpt_optional=False):
    """How every script's ``main`` starts its model: ``load_clip_model`` on ``device``, then ``model_config.ckpt_path`` loaded
    strictly (``load_checked``) unless ``model_config.load_ckpt`` is false.  ``ckpt_optional`` (supervised fine-tuning, which may
    start from the encoders as initialised): a configuration without ``ckpt_path`` is no error either and ``allow_random_init``
    defaults to true.  Returns ``(model, loaded)``."""
    from ..model import simple_clip   # looked up per call: the tests replace load_clip_model
    mc = args.model_config
    if ckpt_optional and not hasattr(args, "allow_random_init"):
        args.allow_random_init = True
    model = simple_clip.load_clip_model(args, device)
    if hasattr(mc, "load_ckpt") and mc.load_ckpt is False or ckpt_optional and not hasattr(mc, "ckpt_path"):
        return model, False
    state_dict = remove_extra_pre_fix(torch.load(str(mc.ckpt_path), map_location="cpu"))
    # the loss's learnable scalars (model_config.trainable_temperature: logit_scale; model_config.contrastive_loss=sigmoid: logit_scale
    # and logit_bias) are the keys a checkpoint and a model may disagree on: a checkpoint trained without one starts it at its
    # initial value, a model built without one ignores the checkpoint's
    missing, unexpected = [], []
    for key, what in (("logit_scale", "temperature"), ("logit_bias", "bias")):
        if key in model._parameters:
            missing.append(key)
            if key not in state_dict:
                print(f"checkpoint {mc.ckpt_path} has no {key}: the {what} keeps its initial value "
                      f"({key} = {float(model._parameters[key].detach()):.6f})")
        else:
            unexpected.append(key)
    load_checked(model, state_dict, f"checkpoint {mc.ckpt_path}", allow_missing=tuple(missing), allow_unexpected=tuple(unexpected))
    return model, True
