"""Method-one evaluation (reference scripts/method_one_eval.py): the seen / unseen protocol that ends in a harmonic mean.

An image query is searched against the seen keys, image to image.  For each rank slot that prediction is kept only when its
similarity is above a threshold; otherwise the slot takes the prediction of a search against the unseen keys, image to DNA.  The
threshold is the one of ``np.linspace(0, 1, 1000)`` that maximises the harmonic mean of the seen and unseen top-1 species micro
accuracy; the accuracy tables are then formed from the merged lists.

Mirrored entry points (same names, argument meaning and return shapes as the reference; its function bodies are the specification
-- the reference script itself does not import, it asks ``bioscanclip.util.dataset`` for a loader that does not exist):
    inference_with_original_image_encoder_and_dna_encoder   :19-56
    decide_prediction_with_threshold                        :59-84
    get_final_pred_and_acc                                  :87-102
    make_final_pred                                         :105-118
    harmonic_mean                                           :121-128
    search_threshold_with_harmonic_mean                     :131-157
    get_all_unique_species_from_dataloader                  :160-167
    method_1_inference_and_eval_for_seen_and_unseen         :170-239
    print_acc_for_google_doc                                :242-262
    check_for_acc_about_correct_predict_seen_or_unseen      :264-278
    main                                                    :282-359

``hip_eval=host`` (default) is the string-list arithmetic of the reference with the searches on the HIP top-k (``make_prediction``).
``hip_eval=gpu`` keeps everything after the features on the GPU (``bioscanclip/hip/method_one.py``): both key indices are built once,
label matches are bit masks, the 1 000 thresholds are one sweep launch per split, the tables come from integer class counts.  Its
output dictionaries equal the host path's with ``==``; ``final_pred_labels`` holds strings only with ``with_predictions=True``
(otherwise ``None``, and ``merged`` carries the GPU handle the membership check reads).

``eval_shards=<root>`` reads the seven splits from a protocol root of shards (``shards.protocol_splits``: ``seen_keys``,
``val_unseen_keys``, ``test_unseen_keys``, ``val_seen``, ``val_unseen``, ``test_seen``, ``test_unseen``) instead of the synthetic loaders.
With ``hip_eval=gpu`` every split is walked once with the one tower it needs and features, key indices and label ids stay on the GPU
(``bioscanclip/hip/protocols.py``); with ``hip_eval=host`` the functions below walk ``ShardLoader(for_training=False)`` loaders.
``eval_batch_size`` (default 40, the reference's) and ``hip_jpeg_entropy=host|gpu`` as in ``inference_and_eval.py``; a ``synthetic_*``
option next to ``eval_shards`` is refused.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioscanclip.epoch.inference_epoch import get_feature_and_label  # noqa: E402
from bioscanclip.hip.method_one import harmonic_mean as _harmonic_mean  # noqa: E402
from inference_and_eval import (LEVELS, _k_list, eval_mode, make_prediction, top_k_macro_accuracy,  # noqa: E402
                                top_k_micro_accuracy)

K_LIST = None
MAX_K = 5   # the search depth of both searches (:50, :54)
# the keys of one split's dictionary in search_threshold_with_harmonic_mean: the two lists of the first search, the second's, the truth
SPLIT_KEYS = ('pred_labels_from_search_with_seen_keys', 'pred_similarity_from_search_with_seen_keys',
              'pred_labels_from_search_with_unseen_keys', 'gt_label')


def _key_features(original_model, key_dataloaders, device, key_type):
    feats, labels = [], []
    for loader in key_dataloaders:
        _, f, lab = get_feature_and_label(loader, original_model, device, type_of_feature=key_type, multi_gpu=False)
        feats.append(f)
        labels = labels + lab
    return np.concatenate(feats, axis=0), labels


def inference_with_original_image_encoder_and_dna_encoder(original_model, seen_query_dataloader, unseen_query_dataloader,
                                                          key_dataloaders, device, key_type='dna'):
    _, seen_q, seen_gt = get_feature_and_label(seen_query_dataloader, original_model, device, type_of_feature="image", multi_gpu=False)
    _, unseen_q, unseen_gt = get_feature_and_label(unseen_query_dataloader, original_model, device, type_of_feature="image",
                                                   multi_gpu=False)
    keys, key_labels = _key_features(original_model, key_dataloaders, device, key_type)
    seen_pred, seen_sim = make_prediction(seen_q, keys, key_labels, with_similarity=True, max_k=MAX_K)
    unseen_pred, unseen_sim = make_prediction(unseen_q, keys, key_labels, with_similarity=True, max_k=MAX_K)
    return seen_pred, seen_sim, seen_gt, unseen_pred, unseen_sim, unseen_gt


def decide_prediction_with_threshold(args, pred_labels_from_image_classifier, confidence_score_or_similarity,
                                     pred_labels_from_search, threshold):
    final_pred_labels = []
    for first, scores, second in zip(pred_labels_from_image_classifier, confidence_score_or_similarity, pred_labels_from_search):
        merged = {}
        for kth, score in enumerate(scores):
            source = first if score > threshold else second          # strict; a NaN takes the second list
            for level in source:
                merged.setdefault(level, []).append(source[level][kth])
        final_pred_labels.append(merged)
    return final_pred_labels


def get_final_pred_and_acc(args, pred_labels_from_search_with_seen_keys, similarity_from_search_with_seen_keys,
                           pred_labels_from_search_with_unseen_keys, gt_labels, best_threshold=None):
    final_pred_labels = decide_prediction_with_threshold(args, pred_labels_from_search_with_seen_keys,
                                                         similarity_from_search_with_seen_keys,
                                                         pred_labels_from_search_with_unseen_keys, best_threshold)
    k_list = _k_list(args)
    macro_acc, per_class_acc = top_k_macro_accuracy(final_pred_labels, gt_labels, k_list=k_list)
    return {"final_pred_labels": final_pred_labels, "gt_labels": gt_labels, "best_threshold": best_threshold,
            "micro_acc": top_k_micro_accuracy(final_pred_labels, gt_labels, k_list=k_list), "macro_acc": macro_acc,
            "per_class_acc": per_class_acc}


def merge_checked(args, names, lists, gt_labels, threshold):
    """``make_final_pred`` of both methods: ``lists`` = (first predictions, their scores, second predictions), ``names`` what the
    length report calls them."""
    n = [len(x) for x in lists]
    if n[0] != n[1] != n[2]:   # the reference's chained comparison (:107-108), kept as it is
        for name, count in zip(names, n):
            print(f"{name}: {count}")
        sys.exit()
    return decide_prediction_with_threshold(args, *lists, threshold), gt_labels


def make_final_pred(args, pred_labels_from_search_with_seen_keys, similarity_from_search_with_seen_keys,
                    pred_labels_from_search_with_unseen_keys, gt_labels, threshold):
    names = ('pred_labels_from_search_with_seen_keys', 'similarity_from_search_with_seen_keys', 'pred_labels_from_search_with_unseen_keys')
    return merge_checked(args, names, (pred_labels_from_search_with_seen_keys, similarity_from_search_with_seen_keys,
                                       pred_labels_from_search_with_unseen_keys), gt_labels, threshold)


def harmonic_mean(l):
    return _harmonic_mean(l)


def search_threshold(args, all_split_data, grid, keys, make_final_pred):
    """``search_threshold_with_harmonic_mean`` of both methods over the thresholds ``grid``; ``keys`` name a split's four entries in
    ``make_final_pred``'s order."""
    best_threshold, max_score = None, float('-inf')
    k_list = _k_list(args)
    for threshold in grid:
        acc_list = []
        for split in all_split_data:
            final_pred_labels, gt_labels = make_final_pred(args, *(split[key] for key in keys), threshold=threshold)
            acc_list.append(top_k_micro_accuracy(final_pred_labels, gt_labels, k_list=k_list)[1]['species'])
        score = harmonic_mean(acc_list)
        if score > max_score:
            max_score, best_threshold = score, threshold
    return best_threshold


def search_threshold_with_harmonic_mean(args, all_split_data, num_intervals=1000):
    """Host path: every merged list is rebuilt for every threshold, as the reference does (no progress bar)."""
    return search_threshold(args, all_split_data, np.linspace(0, 1, num_intervals), SPLIT_KEYS, make_final_pred)


def get_all_unique_species_from_dataloader(dataloader):
    names = set()
    for batch in dataloader:
        names.update(batch[6]['species'])
    return list(names)


class MergedOnGpu:
    """What the GPU path returns in place of the merged string lists: the split's GPU state, the threshold, and what is needed to
    name things (``vocab``) or to build the strings after all (``strings()``)."""

    def __init__(self, split, threshold, vocab, seen_key_labels, unseen_key_labels):
        self.split, self.threshold, self.vocab = split, threshold, vocab
        self.seen_key_labels, self.unseen_key_labels = seen_key_labels, unseen_key_labels

    def strings(self):
        from bioscanclip.hip.method_one import merged_predictions
        return merged_predictions(self.split, self.threshold, self.seen_key_labels, self.unseen_key_labels)

    def member_share(self, species_list, ks=(1, 3, 5)):
        """``species_list``: names, or the int32 0/1 member table over the species ids itself (``ProtocolRoot.member_table``)."""
        from bioscanclip.hip.method_one import member_share
        if isinstance(species_list, np.ndarray):
            table = np.ascontiguousarray(species_list, dtype=np.int32)
        else:
            listed = set(species_list)
            table = np.asarray([int(name in listed) for name in self.vocab["species"]], dtype=np.int32)
        return member_share(self.split, self.threshold, table, ks=ks, level="species")


def _method_1_gpu(args, original_model, seen_query_dataloader, unseen_query_dataloader, seen_keys_dataloader,
                  val_unseen_keys_dataloader, test_unseen_keys_dataloader, device, searched_threshold, with_predictions, num_intervals):
    """The GPU path: features as on the host path, then both key indices built once, every split's two searches and its masks."""
    seen_keys, seen_key_labels = _key_features(original_model, [seen_keys_dataloader], device, "image")
    print()
    unseen_keys, unseen_key_labels = _key_features(original_model, [val_unseen_keys_dataloader, test_unseen_keys_dataloader], device,
                                                   "dna")
    queries = [get_feature_and_label(loader, original_model, device, type_of_feature="image", multi_gpu=False)[1:]
               for loader in (seen_query_dataloader, unseen_query_dataloader)]
    return score_features_on_gpu(args, seen_keys, seen_key_labels, unseen_keys, unseen_key_labels, queries, searched_threshold,
                                 with_predictions, num_intervals)


def score_features_on_gpu(args, seen_keys, seen_key_labels, unseen_keys, unseen_key_labels, queries, searched_threshold=None,
                          with_predictions=False, num_intervals=1000):
    """The GPU path from features on: ``queries`` is ``[(image features, gt_labels)]``, one pair per split (seen queries, unseen
    queries); the keys are the seen keys' image features and the unseen keys' DNA features with their label lists."""
    from bioscanclip.hip.method_one import MethodOneSplit
    from bioscanclip.hip.retrieval import Labels, RetrievalIndex, encode_labels
    arrays, vocab = encode_labels(seen_key_labels, unseen_key_labels, *[gt for _, gt in queries], levels=LEVELS)
    seen_index, unseen_index = RetrievalIndex(seen_keys), RetrievalIndex(unseen_keys)    # built once, shared by the splits
    seen_ids, unseen_ids = Labels(arrays[0]), Labels(arrays[1])
    splits = [MethodOneSplit.from_queries(seen_index, seen_ids, unseen_index, unseen_ids, feats, ids, max_k=MAX_K, levels=LEVELS)
              for (feats, _), ids in zip(queries, arrays[2:])]
    return score_splits_on_gpu(args, splits, [gt for _, gt in queries], vocab, seen_key_labels, unseen_key_labels, searched_threshold,
                               with_predictions, num_intervals)


def score_splits_on_gpu(args, splits, gt_labels, vocab, seen_key_labels, unseen_key_labels, searched_threshold=None,
                        with_predictions=False, num_intervals=1000, grid=None):
    """Threshold search (unless given) and one output dictionary per ``MethodOneSplit``.  ``grid``: the function that makes the
    thresholds of ``num_intervals`` (default: method one's ``linspace_thresholds``; method two passes its own)."""
    from bioscanclip.hip.method_one import linspace_thresholds, merged_accuracy, pick_threshold, sweep
    k_list = _k_list(args)
    print("Searching best threshold.")
    if searched_threshold is None:
        if 1 not in k_list:
            raise KeyError(1)     # the host path reads micro_acc[1] in its threshold search
        thresholds = (grid or linspace_thresholds)(num_intervals)
        counts, totals = sweep(splits, thresholds, level="species", k=1)
        best_threshold = pick_threshold(counts, totals, thresholds)
    else:
        best_threshold = searched_threshold
    outputs = []
    for split, gt in zip(splits, gt_labels):
        acc, per_class = merged_accuracy(split, best_threshold, k_list, vocab)
        merged = MergedOnGpu(split, best_threshold, vocab, seen_key_labels, unseen_key_labels)
        outputs.append({"final_pred_labels": merged.strings() if with_predictions else None, "gt_labels": gt,
                        "best_threshold": best_threshold, "micro_acc": acc["micro_acc"], "macro_acc": acc["macro_acc"],
                        "per_class_acc": per_class, "merged": merged})
    return tuple(outputs)


def method_1_inference_and_eval_for_seen_and_unseen(args, original_model, seen_query_dataloader, unseen_query_dataloader,
                                                    seen_keys_dataloader, val_unseen_keys_dataloader, test_unseen_keys_dataloader,
                                                    device, searched_threshold=None, with_predictions=False, num_intervals=1000):
    """``(seen_output_dict, unseen_output_dict)``.  ``with_predictions`` and ``num_intervals`` are additions: the first matters on
    the GPU path only (the host path always holds its string lists), the second is the grid size of the threshold search."""
    if eval_mode(args) == "gpu":
        return _method_1_gpu(args, original_model, seen_query_dataloader, unseen_query_dataloader, seen_keys_dataloader,
                             val_unseen_keys_dataloader, test_unseen_keys_dataloader, device, searched_threshold, with_predictions,
                             num_intervals)
    (seen_pred_seen_keys, seen_sim, seen_gt, unseen_pred_seen_keys, unseen_sim,
     unseen_gt) = inference_with_original_image_encoder_and_dna_encoder(original_model, seen_query_dataloader, unseen_query_dataloader,
                                                                        [seen_keys_dataloader], device=device, key_type='image')
    print()
    seen_pred_unseen_keys, _, _, unseen_pred_unseen_keys, _, _ = inference_with_original_image_encoder_and_dna_encoder(
        original_model, seen_query_dataloader, unseen_query_dataloader, [val_unseen_keys_dataloader, test_unseen_keys_dataloader],
        device=device, key_type='dna')
    return score_predictions_on_host(args, (seen_pred_seen_keys, seen_sim.tolist(), seen_pred_unseen_keys, seen_gt),
                          (unseen_pred_seen_keys, unseen_sim.tolist(), unseen_pred_unseen_keys, unseen_gt), searched_threshold,
                          num_intervals)


def score_predictions_on_host(args, seen, unseen, searched_threshold=None, num_intervals=1000):
    """The host path from predictions on: each of ``seen`` / ``unseen`` is (seen-key predictions, similarities as lists,
    unseen-key predictions, ground truth)."""
    print("Searching best threshold.")
    if searched_threshold is None:
        searched_threshold = search_threshold_with_harmonic_mean(args, [dict(zip(SPLIT_KEYS, s)) for s in (seen, unseen)],
                                                                 num_intervals=num_intervals)
    return tuple(get_final_pred_and_acc(args, *s, best_threshold=searched_threshold) for s in (seen, unseen))


def print_acc_for_google_doc(seen_output_dict, unseen_output_dict, K_LIST=None):
    if K_LIST is None:
        K_LIST = [1, 3, 5]
    outputs = (seen_output_dict, unseen_output_dict)
    for type_of_acc in ['micro_acc', 'macro_acc']:
        for k in K_LIST:
            values = [out[type_of_acc][k][level] for out in outputs for level in LEVELS]
            means = [harmonic_mean([out[type_of_acc][k][level] for out in outputs]) for level in LEVELS]
            print("".join(" " + str(round(v, 4)) for v in values + means))


def check_for_acc_about_correct_predict_seen_or_unseen(final_pred_list, species_list):
    """Prints, for k in 1, 3, 5, the share of records whose top-k species hold a name of ``species_list``.  ``final_pred_list`` is
    the list of merged predictions, or the GPU path's ``merged`` handle (the same numbers from member masks)."""
    if isinstance(final_pred_list, MergedOnGpu):
        shares = final_pred_list.member_share(species_list)
    else:
        shares = {}
        for k in [1, 3, 5]:
            correct = sum(any(name in species_list for name in record['species'][:k]) for record in final_pred_list)
            shares[k] = correct * 1.0 / len(final_pred_list)
    for k in [1, 3, 5]:
        print(f"for k = {k}: {shares[k]}")
    return shares


def shard_source(args, overrides=()):
    """``(root, entropy, batch_size)`` of ``eval_shards=<root>`` (``root`` None without it).  Refused before any GPU work: a
    ``synthetic_*`` option among the command line's ``overrides`` next to ``eval_shards`` (both name the splits; the configuration
    file's own defaults do not count), an unknown ``hip_jpeg_entropy``, a batch size below 1."""
    from bioscanclip.util import shards
    root = getattr(args, "eval_shards", None)
    root = None if root in (None, "") else str(root)
    synthetic = sorted({ov.strip().strip("'").strip('"').lstrip("+").split("=", 1)[0] for ov in overrides} & {k for k in args if str(k).startswith("synthetic_")})
    if root is not None and synthetic:
        raise ValueError(f"{', '.join(synthetic)} and eval_shards=<root> both name the splits: give one of them")
    entropy = getattr(args, "hip_jpeg_entropy", None)
    entropy = "host" if entropy is None or entropy == "" else str(entropy)
    if entropy not in shards.ENTROPY_MODES:
        raise ValueError(f"hip_jpeg_entropy must be one of {shards.ENTROPY_MODES}, got {entropy!r}")
    batch_size = int(getattr(args, "eval_batch_size", 40))           # the reference evaluates at batch 40 (:295)
    if batch_size < 1:
        raise ValueError(f"eval_batch_size must be >= 1, got {batch_size}")
    return root, entropy, batch_size


METHOD_ONE_SPLITS = ("seen_keys", "val_unseen_keys", "test_unseen_keys", "val_seen", "val_unseen", "test_seen", "test_unseen")
PARTS = (("val", "val_seen", "val_unseen"), ("test", "test_seen", "test_unseen"))


def report(results, part, seen_species, unseen_species, k_list):
    """What ``main`` prints per part: the table rows and the two membership checks."""
    print_acc_for_google_doc(*results[part], K_LIST=k_list)
    print("For seen")
    check_for_acc_about_correct_predict_seen_or_unseen(_predictions_of(results[part][0]), seen_species)
    print("For unseen")
    check_for_acc_about_correct_predict_seen_or_unseen(_predictions_of(results[part][1]), unseen_species)


def method_1_from_shards(args, original_model, proto, device):
    """``main`` from ``load_model`` on for a protocol root.  ``hip_eval=gpu``: both key indices built once during one walk per key
    split, one walk per query split, member tables from the joint ids; ``hip_eval=host``: the functions above on shard loaders."""
    from bioscanclip.hip import protocols
    k_list = _k_list(args)
    results, threshold = {}, None
    unseen_key_splits = protocols.UNSEEN_KEY_SPLITS
    if eval_mode(args) == "gpu":
        keys = protocols.method_one_keys(proto, original_model, device, width=int(getattr(args.model_config, "output_dim", 768)))
        key_rows = (protocols.LabelRows(keys[1].ids, proto.vocab), protocols.LabelRows(keys[3].ids, proto.vocab))
        seen_species, unseen_species = proto.member_table("seen_keys"), proto.member_table(*unseen_key_splits)
    else:
        seen_species, unseen_species = proto.species_names("seen_keys"), proto.species_names(*unseen_key_splits)
    for part, seen, unseen in PARTS:
        if eval_mode(args) == "gpu":
            splits = [protocols.method_one_split(proto, name, original_model, device, keys) for name in (seen, unseen)]
            results[part] = score_splits_on_gpu(args, splits, [protocols.ground_truth(proto, name) for name in (seen, unseen)], proto.vocab,
                                                *key_rows, searched_threshold=threshold)
        else:
            ld = lambda name: proto.loader(name, labels=None)
            results[part] = method_1_inference_and_eval_for_seen_and_unseen(
                args, original_model, ld(seen), ld(unseen), ld("seen_keys"), ld(unseen_key_splits[0]), ld(unseen_key_splits[1]), device,
                searched_threshold=threshold)
        threshold = results[part][0]['best_threshold']              # the val threshold is the test splits' searched_threshold
        report(results, part, seen_species, unseen_species, k_list)
    return results


def _predictions_of(output_dict):
    return output_dict["final_pred_labels"] if output_dict["final_pred_labels"] is not None else output_dict["merged"]


def main(argv=None):
    """Reference entry (:282-359): config -> ``load_clip_model`` -> checkpoint (unless ``model_config.load_ckpt`` is false) ->
    threshold search and tables on the val splits -> the same threshold on the test splits.  The HDF5 splits are not available:
    the seven splits (seen / val-unseen / test-unseen keys, seen and unseen val queries, seen and unseen test queries) come from
    ``SyntheticEvalLoader`` with distinct seeds.  The reference's last membership check passes the test-unseen species list twice
    (:358-359); here the unseen queries are checked against val + test unseen species in both places.  ``hip_eval=gpu`` (default
    host) scores on the GPU.  Returns ``{"val": (seen, unseen), "test": (seen, unseen)}`` output dictionaries."""
    from bioscanclip.util.config import load_config
    from bioscanclip.util.synthetic import SyntheticEvalLoader
    from bioscanclip.util.util import load_model_and_checkpoint
    here = os.path.dirname(os.path.abspath(__file__))
    argv = list(sys.argv[1:] if argv is None else argv)
    args = load_config(os.path.join(here, "..", "bioscanclip", "config"), argv)
    eval_mode(args)
    root, entropy, eval_batch = shard_source(args, argv)
    mc = args.model_config
    if getattr(mc, "for_open_clip", False):
        raise NotImplementedError("the open_clip branch is not part of the HIP-accelerated path")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("method-one evaluation runs on one GPU")
    if root is not None:
        from bioscanclip.util import shards
        shards.protocol_splits(root, METHOD_ONE_SPLITS)
    if not torch.cuda.is_available():
        raise RuntimeError("method_one_eval needs a ROCm GPU: the encoders and the top-k search run in libbsclip_hip.so")
    global K_LIST
    K_LIST = _k_list(args)
    device = torch.device("cuda", 0)
    print("Construct dataloader...")
    if root is not None:
        from bioscanclip.hip.protocols import ProtocolRoot
        proto = ProtocolRoot(root, METHOD_ONE_SPLITS, batch_size=eval_batch, entropy=entropy, device=device)
        original_model, _ = load_model_and_checkpoint(args, device)
        original_model.eval()
        return method_1_from_shards(args, original_model, proto, device)
    bs, n = 40, int(getattr(args, "synthetic_eval_batches", 2))    # the reference evaluates at batch 40 (:295)
    mk = lambda seed: SyntheticEvalLoader(bs, n, with_text=False, seed=seed)
    seen_keys, val_unseen_keys, test_unseen_keys = mk(5301), mk(5302), mk(5303)
    seen_val, unseen_val, seen_test, unseen_test = mk(5304), mk(5305), mk(5306), mk(5307)
    original_model, _ = load_model_and_checkpoint(args, device)
    original_model.eval()

    seen_species = get_all_unique_species_from_dataloader(seen_keys)
    unseen_species = (get_all_unique_species_from_dataloader(val_unseen_keys)
                      + get_all_unique_species_from_dataloader(test_unseen_keys))
    results, threshold = {}, None
    for part, seen, unseen in (("val", seen_val, unseen_val), ("test", seen_test, unseen_test)):
        results[part] = method_1_inference_and_eval_for_seen_and_unseen(args, original_model, seen, unseen, seen_keys, val_unseen_keys,
                                                                        test_unseen_keys, device, searched_threshold=threshold)
        threshold = results[part][0]['best_threshold']              # the val threshold is the test splits' searched_threshold
        print_acc_for_google_doc(*results[part], K_LIST=K_LIST)
        print("For seen")
        check_for_acc_about_correct_predict_seen_or_unseen(_predictions_of(results[part][0]), seen_species)
        print("For unseen")
        check_for_acc_about_correct_predict_seen_or_unseen(_predictions_of(results[part][1]), unseen_species)
    return results


if __name__ == '__main__':
    main()
