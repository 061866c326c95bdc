"""Method-two evaluation (reference scripts/method_two_fine_tuning_and_eval.py): classifier confidences merged with a DNA search.

    python scripts/method_two_fine_tuning_and_eval.py 'model_config=lora_vit_lora_barcode_bert_ssl' model_config.load_ckpt=false [hip_eval=gpu]

A copy of the trained image encoder is fine-tuned as a species classifier on the seen species.  For every image query the
classifier's five highest softmax confidences are taken; the same query, encoded by the ORIGINAL model, is searched against the DNA
keys of the unseen species.  For each rank slot the classifier's prediction is kept when its confidence is above a threshold,
otherwise the slot takes the search's prediction.  The threshold is the one of ``np.linspace(0, 1, 1001)`` with the best harmonic
mean of the seen and unseen top-1 species micro accuracy.

Mirrored entry points (same names, argument meaning and return shapes as the reference; its function bodies are the specification):
    ViTWIthExtraLayer                                        :24-36
    inference_with_fine_tuned_image_encoder                  :39-83
    decide_prediction_with_threshold                         :88-114
    make_final_pred                                          :117-131
    inference_with_original_image_encoder_and_dna_encoder    :134-165
    harmonic_mean                                            :167-175
    search_threshold_with_harmonic_mean                      :177-204
    get_final_pred_and_acc                                   :208-223
    method_2_inference_and_eval_for_seen_and_unseen          :226-277
    get_all_unique_species_from_dataloader                   :280-288
    load_all_seen_species_name_and_create_label_map          :290-315
    label_to_index, label_batch_to_species_idx               :318-325
    fine_tuning_epoch, evaluate_epoch                        :328-385
    print_acc_for_google_doc                                 :388-408
    check_for_acc_about_correct_predict_seen_or_unseen       :411-424
    main                                                     :428-565
Those whose bodies are the same as in the method-one script are that script's functions.

Confidences are ``ops.class_softmax_topk`` (``F.softmax`` then ``torch.topk(k=5, sorted=True)``, :57-62).  Tie rule: a query's five
slots are ordered by logit descending, ties to the lower class index.

``hip_eval=host`` (default) is the reference's string-list arithmetic; the classifier and the searches still run on HIP (logits,
``class_softmax_topk``, ``make_prediction``) and the confidences go through ``.tolist()``.  ``hip_eval=gpu`` keeps everything after
logits and features on the GPU (``bioscanclip/hip/method_two.py``): the classifier side is a key table of C classes, the rest is the
method-one machinery.  Its output dictionaries equal the host path's with ``==``; ``final_pred_labels`` is ``None`` unless
``with_predictions=True`` and ``merged`` carries the GPU handle (``method_one_eval.MergedOnGpu``).

Differences from the reference, all deliberate: the classifier's encoder is a second model loaded from the first one's
``state_dict`` (engine-backed encoders are not deep-copied), so fine-tuning leaves the original model's features untouched; the head
has C = the seen species outputs, not a literal 916; which parameters train follows the regime of the loaded model
(``bioscanclip/epoch/fine_tuning_epoch.py``); the HDF5 splits come from ``SyntheticEvalLoader``; and the last membership check, which
in the reference passes the test-unseen species list twice (:563-564), checks against val + test unseen species in both places, as
the method-one script does.
``eval_shards=<root>`` reads the eight splits from a protocol root of shards (``shards.protocol_splits``).  The classifier is
fine-tuned on ``train_seen`` -- shuffled, a new order per epoch, batch ``model_config.batch_size``, the evaluation transform unless
``fine_tune_augment=true`` selects the training augmentation chain -- with its targets taken from a class-index column resident on the
GPU (``fine_tuning_epoch.ResidentTargets``), so no label dictionary is built for a training batch.  With ``hip_eval=gpu`` each query
split is walked once: the classifier's softmax top-5 goes straight into the split's ``[Q, 5]`` tables while the original model's image
features are filed (``bioscanclip/hip/protocols.py``); with ``hip_eval=host`` the functions below walk shard loaders.
``eval_batch_size`` (default 40), ``hip_jpeg_entropy=host|gpu``; a ``synthetic_*`` option next to ``eval_shards`` is refused.
Keys: ``fine_tune_epochs`` (default 1), ``synthetic_steps_per_epoch`` (20), ``synthetic_eval_batches`` (2), ``model_config.batch_size``
(the training batch; evaluation runs at 40), ``model_config.fine_tuning_set.fine_tune_model_output_dir`` (``last.pth``), ``save_ckpt``.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioscanclip.epoch import fine_tuning_epoch as _epoch  # noqa: E402
from bioscanclip.epoch.inference_epoch import get_feature_and_label  # noqa: E402
from bioscanclip.util.util import EncoderWithExtraLayer  # noqa: E402
from inference_and_eval import LEVELS, make_prediction  # noqa: E402
from method_one_eval import (MAX_K, MergedOnGpu, _k_list, _key_features, _predictions_of,  # noqa: E402,F401
                             check_for_acc_about_correct_predict_seen_or_unseen, decide_prediction_with_threshold, eval_mode,
                             get_all_unique_species_from_dataloader, get_final_pred_and_acc, harmonic_mean, merge_checked,
                             PARTS, print_acc_for_google_doc, report, score_splits_on_gpu, search_threshold, shard_source)

K_LIST = None


class ViTWIthExtraLayer(EncoderWithExtraLayer):
    """Reference :24-36 with ``EncoderWithExtraLayer``'s behaviour: ``forward`` gives the logits without an autograd graph (the HIP
    head), ``.loss`` is the fused training path.  The ``state_dict`` keys are the reference's -- ``vit.*``,
    ``new_linear_layer.weight`` / ``.bias`` -- so a reference ``last.pth`` loads."""

    def __init__(self, vit_model, new_linear_layer):
        super().__init__(vit_model, new_linear_layer)      # the head checks
        del self.encoder, self.new_linear_layer            # registered again under the reference's names, in its order
        self.vit = vit_model
        self.new_linear_layer = new_linear_layer

    @property
    def encoder(self):
        return self.vit


def inference_with_fine_tuned_image_encoder(image_encoder, dataloader, species_level_label_to_index_dict, idx_to_all_labels, device):
    """``(all_confidence_score [[float] * 5], pred_labels [{level: [name] * 5}], gt_labels)``: logits and the softmax top-5 on the
    GPU, then the reference's lists."""
    from bioscanclip.hip.method_two import classifier_confidences
    conf, idx, gt_labels = classifier_confidences(image_encoder, dataloader, device, len(idx_to_all_labels), k=MAX_K)
    pred_labels = []
    for top_5_indices_for_curr_pred in idx.tolist():
        curr_pred_in_multi_levels = {}
        for i in top_5_indices_for_curr_pred:
            for level, name in idx_to_all_labels[i].items():
                curr_pred_in_multi_levels.setdefault(level, []).append(name)
        pred_labels.append(curr_pred_in_multi_levels)
    return conf.tolist(), pred_labels, gt_labels


SPLIT_KEYS = ('pred_labels_from_a', 'pred_confidence_from_a', 'pred_labels_from_b', 'gt_labels')   # :117-131, :190-199


def make_final_pred(args, pred_labels_from_a, pred_confidence_from_a, pred_labels_from_b, gt_labels, threshold):
    # the length report prints the three arguments' names, which here are also the first three dictionary keys
    return merge_checked(args, SPLIT_KEYS[:3], (pred_labels_from_a, pred_confidence_from_a, pred_labels_from_b), gt_labels, threshold)


def inference_with_original_image_encoder_and_dna_encoder(original_model, seen_dataloader, unseen_dataloader,
                                                          val_unseen_keys_dataloader, test_unseen_keys_dataloader, device):
    """``(seen_pred_labels, unseen_pred_labels)``: both query splits' image features searched in val + test unseen DNA keys."""
    _, seen_q, _ = get_feature_and_label(seen_dataloader, original_model, device, type_of_feature="image", multi_gpu=False)
    _, unseen_q, _ = get_feature_and_label(unseen_dataloader, original_model, device, type_of_feature="image", multi_gpu=False)
    keys, key_labels = _key_features(original_model, [val_unseen_keys_dataloader, test_unseen_keys_dataloader], device, "dna")
    return make_prediction(seen_q, keys, key_labels, max_k=MAX_K), make_prediction(unseen_q, keys, key_labels, max_k=MAX_K)


def search_threshold_with_harmonic_mean(args, all_split_data, num_intervals=1000):
    """Host path: every merged list is rebuilt for each of the ``num_intervals + 1`` thresholds (:179), as the reference does."""
    return search_threshold(args, all_split_data, np.linspace(0, 1, num_intervals + 1), SPLIT_KEYS, make_final_pred)


def score_predictions_on_host(args, seen, unseen, searched_threshold=None, num_intervals=1000):
    """The host path from predictions on: each of ``seen`` / ``unseen`` is (classifier predictions, confidences as lists, search
    predictions, ground truth)."""
    if searched_threshold is None:
        print("Searching best threshold.")
        searched_threshold = search_threshold_with_harmonic_mean(args, [dict(zip(SPLIT_KEYS, s)) for s in (seen, unseen)],
                                                                 num_intervals=num_intervals)
    return tuple(get_final_pred_and_acc(args, *s, best_threshold=searched_threshold) for s in (seen, unseen))


def score_confidences_on_gpu(args, confidences, idx_to_all_labels, unseen_keys, unseen_key_labels, query_features,
                             searched_threshold=None, with_predictions=False, num_intervals=1000):
    """The GPU path from confidences and features on.  ``confidences``: per split ``(conf f32 GPU [Q, k], class indices int64 GPU
    [Q, k], gt_labels)``; ``query_features``: per split the original model's image features; the keys are the unseen species' DNA
    features with their label list.  The classifier side becomes a key table: row c holds the labels of class c."""
    from bioscanclip.hip.method_two import MethodTwoSplit, linspace_thresholds
    from bioscanclip.hip.retrieval import Labels, RetrievalIndex, encode_labels
    class_rows = [idx_to_all_labels[c] for c in range(len(idx_to_all_labels))]
    gts = [gt for _, _, gt in confidences]
    arrays, vocab = encode_labels(class_rows, unseen_key_labels, *gts, levels=LEVELS)
    unseen_index = RetrievalIndex(unseen_keys)                      # built once, shared by the splits
    class_table, unseen_ids = Labels(arrays[0]), Labels(arrays[1])
    splits = [MethodTwoSplit.from_classifier(conf, idx, class_table, unseen_index, unseen_ids, feats, ids, levels=LEVELS)
              for (conf, idx, _), feats, ids in zip(confidences, query_features, arrays[2:])]
    return score_splits_on_gpu(args, splits, gts, vocab, class_rows, unseen_key_labels, searched_threshold, with_predictions,
                               num_intervals, grid=linspace_thresholds)


def method_2_inference_and_eval_for_seen_and_unseen(args, image_classifier, original_model, seen_dataloader, unseen_dataloader,
                                                    val_unseen_keys_dataloader, test_unseen_keys_dataloader,
                                                    species_level_label_to_index_dict, idx_to_all_labels, device,
                                                    searched_threshold=None, with_predictions=False, num_intervals=1000):
    """``(seen_output_dict, unseen_output_dict)``.  ``with_predictions`` and ``num_intervals`` are additions: the first matters on
    the GPU path only (the host path always holds its string lists), the second is the number of intervals of the threshold grid."""
    if eval_mode(args) == "gpu":
        from bioscanclip.hip.method_two import classifier_confidences
        confidences = [classifier_confidences(image_classifier, loader, device, len(idx_to_all_labels), k=MAX_K)
                       for loader in (seen_dataloader, unseen_dataloader)]
        unseen_keys, unseen_key_labels = _key_features(original_model, [val_unseen_keys_dataloader, test_unseen_keys_dataloader],
                                                       device, "dna")
        feats = [get_feature_and_label(loader, original_model, device, type_of_feature="image", multi_gpu=False)[1]
                 for loader in (seen_dataloader, unseen_dataloader)]
        return score_confidences_on_gpu(args, confidences, idx_to_all_labels, unseen_keys, unseen_key_labels, feats, searched_threshold,
                                        with_predictions, num_intervals)
    seen_conf, seen_pred_a, seen_gt = inference_with_fine_tuned_image_encoder(image_classifier, seen_dataloader,
                                                                              species_level_label_to_index_dict, idx_to_all_labels, device)
    unseen_conf, unseen_pred_a, unseen_gt = inference_with_fine_tuned_image_encoder(image_classifier, unseen_dataloader,
                                                                                    species_level_label_to_index_dict, idx_to_all_labels,
                                                                                    device)
    seen_pred_b, unseen_pred_b = inference_with_original_image_encoder_and_dna_encoder(original_model, seen_dataloader, unseen_dataloader,
                                                                                       val_unseen_keys_dataloader,
                                                                                       test_unseen_keys_dataloader, device)
    return score_predictions_on_host(args, (seen_pred_a, seen_conf, seen_pred_b, seen_gt),
                                     (unseen_pred_a, unseen_conf, unseen_pred_b, unseen_gt), searched_threshold, num_intervals)


def load_all_seen_species_name_and_create_label_map(train_seen_dataloader):
    """``(label_to_index_dict, idx_to_all_labels)``: the sorted species of the training labels numbered from 0, and per index the
    species with the order / family / genus of its first appearance (:290-315)."""
    species_to_other_labels = {}
    for batch in train_seen_dataloader:
        label_batch = batch[6]
        for i, species in enumerate(label_batch['species']):
            if species not in species_to_other_labels:
                species_to_other_labels[species] = {'order': label_batch['order'][i], 'family': label_batch['family'][i],
                                                    'genus': label_batch['genus'][i]}
    label_to_index_dict, idx_to_all_labels = {}, {}
    for idx, species_label in enumerate(sorted(species_to_other_labels)):
        other = species_to_other_labels[species_label]
        label_to_index_dict[species_label] = idx
        idx_to_all_labels[idx] = {'species': species_label, 'order': other['order'], 'family': other['family'], 'genus': other['genus']}
    return label_to_index_dict, idx_to_all_labels


def label_to_index(label, label_map):
    return label_map[label]


def label_batch_to_species_idx(label_batch, species_level_label_to_index_dict):
    return torch.tensor([label_to_index(species, species_level_label_to_index_dict) for species in label_batch['species']])


def _class_list(species_level_label_to_index_dict):
    """The class list of the epoch drivers: position in it == the dictionary's value (the sorted species)."""
    classes = sorted(species_level_label_to_index_dict, key=species_level_label_to_index_dict.get)
    if [species_level_label_to_index_dict[s] for s in classes] != list(range(len(classes))):
        raise ValueError("the label map must number its species 0 .. C-1")
    return classes


def fine_tuning_epoch(args, model, train_dataloader, val_seen_dataloader, val_unseen_dataloader, optimizer, criterion, device,
                      species_level_label_to_index_dict, epoch=0, targets_of=None, val_targets_of=None):
    """``(epoch_loss, seen_evaluation_result)`` (:328-351) through ``bioscanclip.epoch.fine_tuning_epoch`` -- the fused HIP loss.
    ``targets_of`` / ``val_targets_of``: the drivers' hooks for loaders that yield sample indices instead of label dictionaries."""
    classes = _class_list(species_level_label_to_index_dict)
    epoch_loss = _epoch.fine_tuning_epoch(args, model, train_dataloader, optimizer, criterion, classes, epoch, device, targets_of=targets_of)
    print("Eval on seen val.")
    seen_evaluation_result = evaluate_epoch(model, val_seen_dataloader, device, species_level_label_to_index_dict,
                                            targets_of=val_targets_of)
    print("Evaluation Result:", seen_evaluation_result)
    return epoch_loss, seen_evaluation_result


def evaluate_epoch(model, dataloader, device, species_level_label_to_index_dict, k_values=None, targets_of=None):
    """``{"top{k}_accuracy": ...}`` for k in 1, 3, 5 (:354-385), counted on the GPU."""
    return _epoch.evaluate_epoch(model, dataloader, device, _class_list(species_level_label_to_index_dict), k_values=k_values,
                                 targets_of=targets_of)


def method_2_from_shards(args, image_classifier, original_model, proto, label_map, idx_to_all_labels, class_table, device):
    """The evaluation half of ``main`` for a protocol root: ``{"val": ..., "test": ...}``.  ``hip_eval=gpu``: the unseen-key index
    built once during one walk per key split, one walk per query split with the classifier riding along, member tables from the
    joint ids; ``hip_eval=host``: ``method_2_inference_and_eval_for_seen_and_unseen`` on shard loaders."""
    from bioscanclip.hip import protocols
    from bioscanclip.hip.method_two import linspace_thresholds
    from bioscanclip.hip.retrieval import Labels
    k_list = _k_list(args)
    gpu = eval_mode(args) == "gpu"
    val_keys, test_keys = protocols.UNSEEN_KEY_SPLITS
    C = len(idx_to_all_labels)
    if gpu:
        unseen_index, unseen_labels = protocols.unseen_key_index(proto, original_model, device,
                                                                 width=int(getattr(args.model_config, "output_dim", 768)))
        classes = Labels(class_table, device)
        class_rows = [idx_to_all_labels[c] for c in range(C)]
        unseen_rows = protocols.LabelRows(unseen_labels.ids, proto.vocab)
        seen_species, unseen_species = proto.member_table("seen_keys"), proto.member_table(val_keys, test_keys)
    else:
        seen_species, unseen_species = proto.species_names("seen_keys"), proto.species_names(val_keys, test_keys)
    results, threshold = {}, None
    for part, seen, unseen in PARTS:
        if gpu:
            splits = [protocols.method_two_split(proto, name, image_classifier, C, classes, original_model, device, unseen_index,
                                                 unseen_labels, top_k=MAX_K) for name in (seen, unseen)]
            results[part] = score_splits_on_gpu(args, splits, [protocols.ground_truth(proto, name) for name in (seen, unseen)], proto.vocab,
                                                class_rows, unseen_rows, searched_threshold=threshold, grid=linspace_thresholds)
        else:
            ld = lambda name: proto.loader(name, labels=None)
            results[part] = method_2_inference_and_eval_for_seen_and_unseen(
                args, image_classifier, original_model, ld(seen), ld(unseen), ld(val_keys), ld(test_keys), label_map, idx_to_all_labels,
                device, searched_threshold=threshold)
        threshold = results[part][0]['best_threshold']              # the val threshold is the test splits' searched_threshold
        report(results, part, seen_species, unseen_species, k_list)
    return results


def main(argv=None):
    """Reference entry (:428-565): config -> model -> optional checkpoint -> seen-species label map from the train-seen loader ->
    classifier (a second model's image encoder + ``nn.Linear(output_dim, C)``) -> resume from ``last.pth`` or train
    ``fine_tune_epochs`` epochs -> threshold search and tables on the val splits -> the same threshold on the test splits.
    Returns ``{"val": (seen, unseen), "test": (seen, unseen), "history": [(epoch_loss, seen_evaluation_result)]}``."""
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.simple_clip import load_clip_model
    from bioscanclip.util.config import load_config
    from bioscanclip.util.synthetic import SyntheticEvalLoader
    from bioscanclip.util.util import load_model_and_checkpoint
    here = os.path.dirname(os.path.abspath(__file__))
    argv = list(sys.argv[1:] if argv is None else argv)
    args = load_config(os.path.join(here, "..", "bioscanclip", "config"), argv)
    eval_mode(args)
    root, entropy, eval_batch = shard_source(args, argv)
    if "model_config" not in args:
        raise SystemExit("usage: method_two_fine_tuning_and_eval.py 'model_config=<name>' [key=value ...]")
    mc = args.model_config
    if root is not None:
        from bioscanclip.util import shards
        shards.protocol_splits(root)
    if getattr(mc, "for_open_clip", False):
        raise NotImplementedError("the open_clip branch is not part of the HIP-accelerated path")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("method-two fine-tuning and evaluation run on one GPU")
    if not torch.cuda.is_available():
        raise RuntimeError("method_two_fine_tuning_and_eval needs a ROCm GPU: the encoders, the classifier head and the top-k run in "
                           "libbsclip_hip.so")
    global K_LIST
    K_LIST = _k_list(args)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)

    print("Construct dataloader...")
    proto, targets_of, val_targets_of = None, None, None
    if root is not None:
        from bioscanclip.hip.protocols import ProtocolRoot
        proto = ProtocolRoot(root, shards.PROTOCOL_SPLITS, batch_size=eval_batch, entropy=entropy, device=device)
        species_level_label_to_index_dict, idx_to_all_labels, class_table = proto.sorted_class_list("train_seen")
        classes = _class_list(species_level_label_to_index_dict)
        train_seen = proto.loader("train_seen", batch_size=int(mc.batch_size), shuffle=True,
                                  for_training=bool(getattr(args, "fine_tune_augment", False)))
        seen_val, unseen_val = proto.loader("val_seen"), proto.loader("val_unseen")
        targets_of, val_targets_of = proto.targets(classes, "train_seen"), proto.targets(classes, "val_seen")
    else:
        n_eval = int(getattr(args, "synthetic_eval_batches", 2))
        mk = lambda seed: SyntheticEvalLoader(40, n_eval, with_text=False, seed=seed)
        train_seen = SyntheticEvalLoader(int(mc.batch_size), int(getattr(args, "synthetic_steps_per_epoch", 20)), seed=6300)
        seen_keys, val_unseen_keys, test_unseen_keys = mk(6301), mk(6302), mk(6303)
        seen_val, unseen_val, seen_test, unseen_test = mk(6304), mk(6305), mk(6306), mk(6307)
        species_level_label_to_index_dict, idx_to_all_labels = load_all_seen_species_name_and_create_label_map(train_seen)
    print(f"{len(idx_to_all_labels)} seen species")

    original_model, _ = load_model_and_checkpoint(args, device)
    original_model.eval()
    # the reference deep-copies original_model.image_encoder (:459); here the copy is a second model with the first one's parameters
    copy_of_model = load_clip_model(args, device)
    copy_of_model.load_state_dict(original_model.state_dict())
    image_classifier = ViTWIthExtraLayer(copy_of_model.image_encoder,
                                         nn.Linear(int(getattr(mc, "output_dim", 768)), len(idx_to_all_labels))).to(device)
    criterion = nn.CrossEntropyLoss()
    optimizer = FusedAdamW([p for p in image_classifier.parameters() if p.requires_grad], lr=0.001)

    out_dir = getattr(getattr(mc, "fine_tuning_set", None), "fine_tune_model_output_dir", None)
    last_ckpt_path = os.path.join(str(out_dir), "last.pth") if out_dir is not None else None
    save_ckpt = bool(getattr(args, "save_ckpt", False)) and last_ckpt_path is not None
    history = []
    if last_ckpt_path is not None and os.path.exists(last_ckpt_path):
        print(f"Found pre-trained model in {last_ckpt_path}")
        image_classifier.load_state_dict(torch.load(last_ckpt_path, map_location="cpu"))
        save_ckpt = False
    else:
        for epoch in range(int(getattr(args, "fine_tune_epochs", 1))):
            if proto is not None:
                train_seen.set_epoch(epoch)                            # a new order of train_seen per epoch
            history.append(fine_tuning_epoch(args, image_classifier, train_seen, seen_val, unseen_val, optimizer, criterion, device,
                                             species_level_label_to_index_dict, epoch=epoch, targets_of=targets_of,
                                             val_targets_of=val_targets_of))
            print(f"epoch {epoch}: loss {history[-1][0]:.6f}")
    if save_ckpt:
        os.makedirs(str(out_dir), exist_ok=True)
        torch.save(image_classifier.state_dict(), last_ckpt_path)
        print(f'Last ckpt: {last_ckpt_path}')
    image_classifier.eval()
    if proto is not None:
        return {"history": history, **method_2_from_shards(args, image_classifier, original_model, proto, species_level_label_to_index_dict,
                                                           idx_to_all_labels, class_table, device)}

    run = lambda seen, unseen, threshold: method_2_inference_and_eval_for_seen_and_unseen(
        args, image_classifier, original_model, seen, unseen, val_unseen_keys, test_unseen_keys, species_level_label_to_index_dict,
        idx_to_all_labels, device, searched_threshold=threshold)
    seen_species = get_all_unique_species_from_dataloader(seen_keys)
    unseen_species = (get_all_unique_species_from_dataloader(val_unseen_keys)
                      + get_all_unique_species_from_dataloader(test_unseen_keys))
    results = {"history": history}
    threshold = None
    for part, seen, unseen in (("val", seen_val, unseen_val), ("test", seen_test, unseen_test)):
        results[part] = run(seen, unseen, threshold)
        threshold = results[part][0]['best_threshold']              # the val threshold is the test splits' searched_threshold
        print_acc_for_google_doc(*results[part], K_LIST=K_LIST)
        print("For seen")
        check_for_acc_about_correct_predict_seen_or_unseen(_predictions_of(results[part][0]), seen_species)
        print("For unseen")
        check_for_acc_about_correct_predict_seen_or_unseen(_predictions_of(results[part][1]), unseen_species)
    return results


if __name__ == '__main__':
    main()
