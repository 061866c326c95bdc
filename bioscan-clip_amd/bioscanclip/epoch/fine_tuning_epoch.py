"""Supervised fine-tuning drivers with the reference's names and signatures (``bioscanclip/epoch/fine_tuning_epoch.py``):
``label_batch_to_species_idx``, ``fine_tuning_epoch``, ``evaluate_epoch``, ``fine_tuning_epoch_image_and_dna``.  The models are
``bioscanclip.util.util.EncoderWithExtraLayer`` classifiers; the return values are the reference's (the epoch-mean loss,
``{"top{k}_accuracy": ...}``).

What differs, deliberately:
  * ``criterion`` must be an ``nn.CrossEntropyLoss`` with default arguments: the loss then runs as the fused HIP path
    (``model.loss(x, target)``: logits, cross-entropy and dlogits in one call, hip/functional.py).  Anything else raises -- there is
    no torch compute fallback.  One consequence of the defaults: a target of -100 (``ignore_index``) is not skipped here, it is an
    out-of-range target like any other (below); ``label_batch_to_species_idx`` never produces one.
  * which parameters train is decided by the regime of the loaded model, not switched on wholesale (the reference sets
    ``requires_grad = True`` on every parameter under the LoRA wrappers): in the LoRA regime the LoRA pairs, the projection heads
    and the new Linear train; with ``disable_lora: true`` every parameter does.
  * a target outside [0, C) is never used as an index: its row contributes zero loss and zero gradient and sets a bit in a device
    flag word, which is read once per epoch and raises with the label level named.
  * the training loss is read back once per epoch unless a progress bar or wandb wants it per step; ``evaluate_epoch`` keeps
    targets and predictions on the GPU (``bsclip_class_topk`` in place of the argsort, ``bsclip_retrieval_hit_ranks`` /
    ``bsclip_retrieval_class_counts`` for the hits) and downloads one integer count per k at the end; the accuracy is
    ``count * 1.0 / n`` on the host in float64.
  * tqdm / wandb are optional, as in ``train_epoch.py`` here.
"""
import torch
import torch.nn as nn

try:  # neither ships in this image
    from tqdm import tqdm
except Exception:  # pragma: no cover
    tqdm = None
try:
    import wandb
except Exception:  # pragma: no cover
    wandb = None

LABEL_LEVEL = "species"   # the taxonomy level the classifiers are trained on (reference fine_tuning_epoch.py:7)


def label_batch_to_species_idx(label_batch, unique_species_for_seen):
    """Reference fine_tuning_epoch.py:6-9: the position of every sample's species in the class list (``list.index``: the first
    occurrence; a species that is not in the list raises ValueError on the host)."""
    species_list = label_batch[LABEL_LEVEL]
    return torch.tensor([unique_species_for_seen.index(species) for species in species_list])


class ResidentTargets:
    """``targets_of`` hook of the drivers below for a ``ShardLoader(labels="ids")``: the split's class-index column (int32 ``[n]``,
    ``shards.class_indices``) is uploaded once and a batch's targets are that column at the batch's sample indices (slot 6 of the
    batch) -- torch indexing on the device, no label dictionaries and no ``list.index``.  A species outside the class list is
    ``shards.NOT_A_CLASS`` in the column and ends in the drivers' existing out-of-range errors."""

    def __init__(self, class_index, device):
        import numpy as np
        self.column = torch.from_numpy(np.ascontiguousarray(class_index, dtype=np.int32)).to(device)

    def __call__(self, batch):
        return self.column[batch[6].to(self.column.device)]


def _require_fused(criterion):
    ok = (type(criterion) is nn.CrossEntropyLoss and criterion.weight is None and criterion.ignore_index == -100
          and criterion.reduction == "mean" and criterion.label_smoothing == 0.0)
    if not ok:
        raise NotImplementedError("supervised fine-tuning runs nn.CrossEntropyLoss() with default arguments on the fused HIP path; "
                                  f"{criterion!r} has no HIP implementation and there is no torch compute fallback")


def _require_classifier(model):
    if not hasattr(model, "loss") or not hasattr(model, "new_linear_layer"):
        raise TypeError("expected a bioscanclip.util.util.EncoderWithExtraLayer classifier")


def _modality_input(batch, modality, device):
    _, image_input_batch, dna_input_batch, _, _, _, label_batch = batch
    if modality == "image":
        return image_input_batch.to(device), label_batch
    if modality == "dna":
        return dna_input_batch.to(device), label_batch
    raise NotImplementedError(f"modality {modality!r}: only the image and DNA encoders have classifiers (no text-tower classifier)")


def _check_flag(flag, n_classes):
    if int(flag.item()) & 1:
        raise ValueError(f"supervised fine-tuning: a {LABEL_LEVEL} target lies outside [0, {n_classes}); those rows contributed "
                         "nothing to the loss or the gradients of this epoch")


def _run_epoch(args, classifiers, inputs_of, dataloader, optimizer, criterion, unique_species_for_seen, epoch, device, targets_of=None):
    """The loop shared by the one- and the two-classifier driver.  ``inputs_of(batch)`` -> one input per classifier;
    ``targets_of(batch)`` -> the integer targets ``[B]`` (default: ``label_batch_to_species_idx`` of the batch's label dictionaries)."""
    _require_fused(criterion)
    for m in classifiers:
        _require_classifier(m)
    holder = classifiers[0] if len(classifiers) == 1 else nn.ModuleList(classifiers)
    n_steps = len(dataloader)
    show = tqdm is not None
    log = bool(getattr(args, "activate_wandb", False)) and wandb is not None
    steps = tqdm(enumerate(dataloader), total=n_steps) if show else enumerate(dataloader)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    losses = []
    for step, batch in steps:
        if targets_of is None:
            target = label_batch_to_species_idx(batch[6], unique_species_for_seen).to(device)
        else:
            target = targets_of(batch).to(device)
        optimizer.zero_grad()
        loss = None
        for m, x in zip(classifiers, inputs_of(batch)):
            term = m.loss(x, target, flag=flag)
            loss = term if loss is None else loss + term
        loss.backward()
        if hasattr(optimizer, "needs_attach") and optimizer.needs_attach():
            optimizer.attach(holder)  # FusedAdamW: adopt the engines' flat buffers once they exist
        optimizer.step()
        if show or log:
            value = loss.item()
            losses.append(value)
            if show:
                steps.set_description(f"loss: {value}")
            if log:
                wandb.log({"loss": value, "step": step + epoch * n_steps})
        else:
            losses.append(loss.detach())
    _check_flag(flag, len(unique_species_for_seen))
    if losses and torch.is_tensor(losses[0]):
        losses = torch.stack(losses).tolist()   # the epoch's only download of the loss
    return sum(losses) * 1.0 / len(losses)


def fine_tuning_epoch(args, model, insect_train_dataloader, optimizer, criterion, unique_species_for_seen, epoch, device,
                      modality="image", targets_of=None):
    """Reference fine_tuning_epoch.py:11-37: one epoch of one classifier (``modality``: "image" or "dna"); returns the mean loss."""
    if modality not in ("image", "dna"):
        raise NotImplementedError(f"modality {modality!r}: only the image and DNA encoders have classifiers (no text-tower classifier)")
    return _run_epoch(args, [model], lambda batch: [_modality_input(batch, modality, device)[0]], insect_train_dataloader,
                      optimizer, criterion, unique_species_for_seen, epoch, device, targets_of=targets_of)


def fine_tuning_epoch_image_and_dna(args, image_classifier, dna_classifier, insect_train_dataloader, optimizer, criterion,
                                    unique_species_for_seen, epoch, device, targets_of=None):
    """Reference fine_tuning_epoch.py:78-104: both classifiers per batch, loss = CE(image) + CE(dna); returns the mean loss."""
    image_classifier.train()
    dna_classifier.train()
    return _run_epoch(args, [image_classifier, dna_classifier],
                      lambda batch: [batch[1].to(device), batch[2].to(device)], insect_train_dataloader, optimizer, criterion,
                      unique_species_for_seen, epoch, device, targets_of=targets_of)


def evaluate_epoch(model, dataloader, device, unique_species_for_seen, k_values=None, modality="image", targets_of=None):
    """Reference fine_tuning_epoch.py:39-76: ``{"top{k}_accuracy": share of samples whose target is among the k highest logits}``.
    Ties between equal logits resolve to the lower class index (the reference's argsort leaves them unspecified).
    ``targets_of(batch)`` replaces ``label_batch_to_species_idx`` (which raises on the host for a species outside the class list):
    a target outside [0, C) then is handed to the counting kernel as a label outside its class range, so the flag word raises."""
    from bioscanclip.hip import ops
    _require_classifier(model)
    if k_values is None:
        k_values = [1, 3, 5]
    k_values = [int(k) for k in k_values]
    C = len(unique_species_for_seen)
    if not k_values or min(k_values) < 1 or len(k_values) > 8 or min(max(k_values), C) > 16:
        raise ValueError("evaluate_epoch: 1 to 8 values of k, each >= 1 and at most 16 (or the class count, if smaller)")
    model.eval()
    kmax = min(max(k_values), C)    # argsort(...)[:, :max(k)] has no more than C columns
    class_ids = torch.arange(C, dtype=torch.int32, device=device).view(C, 1)   # "key labels" of the hit search: class c is c
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    ranks, outside = [], []
    steps = enumerate(dataloader)
    if tqdm is not None:
        steps = tqdm(steps, total=len(dataloader))
    with torch.no_grad():
        for _, batch in steps:
            x, label_batch = _modality_input(batch, modality, device)
            if targets_of is None:
                target = label_batch_to_species_idx(label_batch, unique_species_for_seen).to(device, torch.int32).view(-1, 1)
            else:
                target = targets_of(batch).to(device, torch.int32).view(-1, 1)
                outside.append(((target < 0) | (target >= C)).to(torch.int32))   # 0 = the one class of the count below, 1 = outside it
            output = model(x)
            _, predictions = ops.class_topk(output, C, kmax)
            ranks.append(ops.retrieval_hit_ranks(predictions, class_ids, target.contiguous(), flag=flag))   # first rank of the target, or kmax
    if not ranks:
        raise ValueError("evaluate_epoch: the dataloader is empty")
    hit_rank = torch.cat(ranks)
    n = hit_rank.shape[0]
    # one "class" for every sample: right[j, 0] = the samples whose target sits within the first k_values[j] predictions
    one_class = torch.cat(outside).contiguous() if outside else torch.zeros_like(hit_rank)
    _, right = ops.retrieval_class_counts(hit_rank, one_class, [0, 1], k_values, flag=flag)
    counts = torch.cat([right.view(-1), flag]).tolist()   # the evaluation's only download: one integer per k (+ the flag word)
    ops.check_retrieval_flag(counts[-1])
    return {f"top{k}_accuracy": counts[j] * 1.0 / n for j, k in enumerate(k_values)}
