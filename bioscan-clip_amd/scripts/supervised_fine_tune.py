"""Supervised fine-tuning of a trained model's image and DNA encoders as species classifiers -- the HIP path of reference
``scripts/supervised_fine_tune_bioscan_clip_model_on_insect.py``.

    python scripts/supervised_fine_tune.py 'model_config=lora_vit_lora_barcode_bert_ssl' [key=value ...]

Keeps the reference's structure: config -> ``load_clip_model`` -> checkpoint (``model_config.ckpt_path`` unless
``model_config.load_ckpt`` is false) -> ``EncoderWithExtraLayer`` around the image and the DNA encoder with a new
``nn.Linear(768, C)`` each, C = the species of the training labels -> AdamW(lr=1e-3) -> per epoch
``fine_tuning_epoch_image_and_dna`` and ``evaluate_epoch`` on both classifiers, printed as a table of loss and top-1/3/5.
Differences, all deliberate:
  * which parameters train follows the regime of the loaded model (the reference switches ``requires_grad`` on for every parameter
    under the LoRA wrappers): in the LoRA regime the LoRA pairs, the projection heads and the new Linear train; with
    ``disable_lora: true`` every parameter does;
  * the INSECT dataset loaders are not rebuilt: ``dataset=synthetic`` (the default) feeds synthetic batches of the reference's
    layout whose labels are taxonomy-name dicts (``SyntheticEvalLoader``), as ``train_cl.py`` does for its ``synthetic_eval=true``;
    ``dataset=<root>`` names a protocol root of shards (``shards.protocol_splits``): training on ``train_seen`` (shuffled, a new
    order per epoch, the evaluation transform unless ``fine_tune_augment=true``), evaluation on ``val_seen``, the class list
    ``train_seen``'s species in order of first appearance, the targets a class-index column resident on the GPU
    (``fine_tuning_epoch.ResidentTargets``; ``hip_jpeg_entropy=host|gpu`` for JPEG shards);
  * head, loss, top-k and the accuracy counts run on the HIP kernels (bsclip_ce_fwd_bwd, bsclip_class_topk); one GPU, no graph capture.
Keys: ``fine_tune_epochs`` (default 1), ``synthetic_steps_per_epoch`` (20), ``synthetic_eval_batches`` (2), ``model_config.batch_size``.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from bioscanclip.epoch.fine_tuning_epoch import evaluate_epoch, fine_tuning_epoch_image_and_dna  # noqa: E402
from bioscanclip.hip.optim import FusedAdamW  # noqa: E402
from bioscanclip.util.config import load_config  # noqa: E402
from bioscanclip.util.synthetic import SyntheticEvalLoader  # noqa: E402
from bioscanclip.util.util import EncoderWithExtraLayer, load_model_and_checkpoint  # noqa: E402

K_VALUES = [1, 3, 5]
SHARD_SPLITS = ("train_seen", "val_seen")


def unique_species(dataloader):
    """The class list: the species of the training labels, in order of first appearance."""
    seen = {}
    for batch in dataloader:
        for s in batch[6]["species"]:
            seen.setdefault(s, None)
    return list(seen)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = load_config(os.path.join(PKG, "bioscanclip", "config"), argv)
    if "model_config" not in args:
        raise SystemExit("usage: supervised_fine_tune.py 'model_config=<name>' [key=value ...]")
    mc = args.model_config
    dataset = str(getattr(args, "dataset", "synthetic"))
    if dataset != "synthetic":
        from bioscanclip.util import shards
        if not os.path.isdir(dataset):
            raise NotImplementedError("the INSECT dataset loaders are not part of the HIP path: dataset=synthetic, or a protocol root "
                                      "of shards (a directory holding train_seen and val_seen)")
        shards.protocol_splits(dataset, SHARD_SPLITS)
        entropy = str(getattr(args, "hip_jpeg_entropy", None) or "host")
        if entropy not in shards.ENTROPY_MODES:
            raise ValueError(f"hip_jpeg_entropy must be one of {shards.ENTROPY_MODES}, got {entropy!r}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("supervised fine-tuning runs on one GPU")
    if not hasattr(mc, "dna"):
        raise NotImplementedError("supervised fine-tuning wraps the image and the DNA encoder: the model config has no DNA tower")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)

    print("Initialize model...")
    model, loaded = load_model_and_checkpoint(args, device, ckpt_optional=True)
    if not loaded:
        print("no checkpoint (model_config.load_ckpt=false or no model_config.ckpt_path): fine-tuning the encoders as initialised")

    print("Construct dataloader...")
    batch_size = int(mc.batch_size)
    steps = int(getattr(args, "synthetic_steps_per_epoch", 20))
    n_eval = int(getattr(args, "synthetic_eval_batches", 2))
    train_targets = val_targets = None
    if dataset != "synthetic":
        from bioscanclip.hip.protocols import ProtocolRoot
        proto = ProtocolRoot(dataset, SHARD_SPLITS, batch_size=batch_size, entropy=entropy, device=device)
        train_loader = proto.loader("train_seen", shuffle=True, for_training=bool(getattr(args, "fine_tune_augment", False)))
        val_loader = proto.loader("val_seen")
        classes = proto.first_appearance_classes("train_seen")
        train_targets, val_targets = proto.targets(classes, "train_seen"), proto.targets(classes, "val_seen")
    else:
        train_loader = SyntheticEvalLoader(batch_size, steps, seed=8001)
        val_loader = SyntheticEvalLoader(batch_size, n_eval, seed=8002)
        classes = unique_species(train_loader)
    print(f"{len(classes)} species in the training labels")

    out_dim = int(getattr(mc, "output_dim", 768))
    image_classifier = EncoderWithExtraLayer(model.image_encoder, nn.Linear(out_dim, len(classes))).to(device)
    dna_classifier = EncoderWithExtraLayer(model.dna_encoder, nn.Linear(out_dim, len(classes))).to(device)
    params = [p for m in (image_classifier, dna_classifier) for p in m.parameters() if p.requires_grad]
    print(f"{sum(p.numel() for p in params)} trainable parameters "
          f"({'every parameter' if getattr(mc, 'disable_lora', False) else 'LoRA pairs, projection heads, new Linear layers'})")
    optimizer = FusedAdamW(params, lr=1e-3)
    criterion = nn.CrossEntropyLoss()

    epochs = int(getattr(args, "fine_tune_epochs", 1))
    rows = []
    for epoch in range(epochs):
        if dataset != "synthetic":
            train_loader.set_epoch(epoch)
        loss = fine_tuning_epoch_image_and_dna(args, image_classifier, dna_classifier, train_loader, optimizer, criterion, classes,
                                               epoch, device, targets_of=train_targets)
        acc_i = evaluate_epoch(image_classifier, val_loader, device, classes, k_values=K_VALUES, modality="image", targets_of=val_targets)
        acc_d = evaluate_epoch(dna_classifier, val_loader, device, classes, k_values=K_VALUES, modality="dna", targets_of=val_targets)
        rows.append((epoch, loss, acc_i, acc_d))
        cells = "  ".join(f"{name} top{k} {acc[f'top{k}_accuracy']:.4f}" for name, acc in (("image", acc_i), ("dna", acc_d)) for k in K_VALUES)
        print(f"epoch {epoch}: loss {loss:.6f}  {cells}")
    return rows


if __name__ == "__main__":
    main()
