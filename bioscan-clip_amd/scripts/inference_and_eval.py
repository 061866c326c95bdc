"""Retrieval evaluation (reference scripts/inference_and_eval.py): feature extraction on the HIP encoders, exact
inner-product top-k search on the GPU (``bsclip_topk_ip`` instead of faiss ``IndexFlatIP``), micro / macro top-k accuracy.

Mirrored entry points (same names, argument meaning and return shapes as the reference):
    calculate_silhouette_score :407-411   (``inference_and_eval_setting.silhouette=true``; ``bsclip_silhouette_samples``, GPU only)
    make_prediction            :414-445
    top_k_micro_accuracy       :448-464
    top_k_macro_accuracy       :467-511
    inference_and_print_result :633-715   (accuracy table only; the csv / plotting side is control plane, out of scope)
    get_features_and_label     :734-784
    main                       :786-871   (config -> load_clip_model -> checkpoint unless load_ckpt=false -> features -> table;
                                           splits from the synthetic evaluation loaders, feature cache as .npz)

``eval_shards=<root>`` evaluates a directory of shard splits (``shards.eval_splits``; ``eval_split=val|test``) instead of the synthetic
loaders: every split is walked once with all towers per batch (``bioscanclip/hip/features.py``), and with ``hip_eval=gpu`` the features,
key indices and label ids never leave the GPU (``retrieval.evaluate_resident``).

``hip_eval=gpu`` (default ``host``) selects ``inference_and_print_result_gpu``: the same cell table with one key index per key type
(built once, searched by every query type and both splits), labels as int32 ids, and hit matching / per-class counting as HIP
kernels (``bioscanclip/hip/retrieval.py``); the tables are equal to the host path's, bit for bit.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from bioscanclip.epoch.inference_epoch import get_feature_and_label  # noqa: E402
from bioscanclip.hip import ops  # noqa: E402
from bioscanclip.hip.retrieval import KEY_FEATURES, LEVELS, QUERY_FEATURES, print_accuracy_table, to_gpu  # noqa: E402

All_TYPE_OF_FEATURES_OF_QUERY = QUERY_FEATURES
All_TYPE_OF_FEATURES_OF_KEY = KEY_FEATURES


def search_topk(query_feature, keys_feature, max_k, device=None):
    """L2-normalise both sides and return (similarities f32 [Q, max_k], indices int64 [Q, max_k]) as numpy arrays.

    The arithmetic of ``normalize`` + ``IndexFlatIP.add`` + ``.search`` (:415-422) on the GPU.  There is no CPU path: without
    the HIP library or a GPU this raises.
    """
    sims, idx = ops.topk_ip(to_gpu(query_feature, device), to_gpu(keys_feature, device), int(max_k))
    return sims.cpu().numpy(), idx.cpu().numpy()


def calculate_silhouette_score(args, image_features, labels):
    """Reference :407-411 with sklearn's ``silhouette_samples`` on the GPU (``bioscanclip/hip/silhouette.py``): ``labels[1]`` is the
    list of label dicts; prints one line per level and returns ``{level: mean}``.  Runs on the GPU whatever ``hip_eval`` says."""
    from bioscanclip.hip.silhouette import silhouette_by_level
    label_list = [labels[1][i] for i in range(len(labels[1]))]
    by_level = silhouette_by_level(image_features, label_list, levels=LEVELS)
    for level in LEVELS:
        print(f"The silhouette score for {level} level is : {by_level[level]['mean']}")
    return {level: by_level[level]["mean"] for level in LEVELS}


def make_prediction(query_feature, keys_feature, keys_label, with_similarity=False, with_indices=False, max_k=5):
    similarities, indices = search_topk(query_feature, keys_feature, max_k)
    pred_list = [{level: [keys_label[i][level] for i in key_indices] for level in LEVELS} for key_indices in indices]
    out = [pred_list]
    if with_similarity:
        out.append(similarities)
    if with_indices:
        out.append(indices)
    return out[0] if len(out) == 1 else out


def _hits(pred_list, gt_list, k, level):
    return [gt[level] in pred[level][:k] for pred, gt in zip(pred_list, gt_list)]


def top_k_micro_accuracy(pred_list, gt_list, k_list=None):
    # like the reference, k_list has no default here: None is not iterable (:451)
    total = len(pred_list)
    return {k: {level: sum(_hits(pred_list, gt_list, k, level)) * 1.0 / total for level in LEVELS} for k in k_list}


def top_k_macro_accuracy(pred_list, gt_list, k_list=None):
    if k_list is None:
        k_list = [1, 3, 5]
    macro, per_class = {}, {}
    for k in k_list:
        macro[k], per_class[k] = {}, {}
        for level in LEVELS:
            seen, right = {}, {}
            for hit, gt in zip(_hits(pred_list, gt_list, k, level), gt_list):
                name = gt[level]
                seen[name] = seen.get(name, 0) + 1
                right[name] = right.get(name, 0) + int(hit)
            per_class[k][level] = {name: right[name] * 1.0 / seen[name] for name in seen}
            total = 0
            for name in seen:  # same summation order as the reference (:499-508)
                total = total + right[name] * 1.0 / seen[name]
            macro[k][level] = total / len(seen)
    return macro, per_class


def get_features_and_label(dataloader, model, device, for_key_set=False, for_open_clip=False):
    model.eval()
    _, lang, _ = get_feature_and_label(dataloader, model, device, type_of_feature="text", for_open_clip=for_open_clip)
    _, dna, _ = get_feature_and_label(dataloader, model, device, type_of_feature="dna", for_open_clip=for_open_clip)
    names, image, labels = get_feature_and_label(dataloader, model, device, type_of_feature="image",
                                                 for_open_clip=for_open_clip)
    split = {
        "file_name_list": names,
        "encoded_dna_feature": dna,
        "encoded_image_feature": image,
        "encoded_language_feature": lang,
        "averaged_feature": None,
        "concatenated_feature": None,
        "label_list": labels,
        "all_key_features": None,
        "all_key_features_label": None,
    }
    if dna is not None and image is not None:
        split["averaged_feature"] = np.mean([image, dna], axis=0)
        split["concatenated_feature"] = np.concatenate((image, dna), axis=1)
    if for_key_set and image is not None and dna is not None and lang is not None:
        split["all_key_features"] = np.concatenate((image, dna, lang), axis=0)
        split["all_key_features_label"] = labels + labels + labels
    return split


def print_micro_and_macro_acc(acc_dict, k_list, args=None):
    print_accuracy_table(acc_dict, k_list)


def inference_and_print_result(keys_dict, seen_dict, unseen_dict, args=None, small_species_list=None, k_list=None):
    if k_list is None:
        k_list = [1, 3, 5]
    max_k = k_list[-1]
    acc_dict, per_class_acc, pred_dict = {}, {}, {}
    keys_label = keys_dict["label_list"]
    for q in All_TYPE_OF_FEATURES_OF_QUERY:
        if q not in seen_dict:
            continue
        acc_dict[q], per_class_acc[q], pred_dict[q] = {}, {}, {}
        for kf in All_TYPE_OF_FEATURES_OF_KEY:
            if kf not in keys_dict:
                continue
            acc_dict[q][kf], per_class_acc[q][kf], pred_dict[q][kf] = {}, {}, {}
            keys, seen, unseen = keys_dict[kf], seen_dict[q], unseen_dict[q]
            if keys is None:
                continue
            if kf == "all_key_features":
                keys_label = keys_dict["all_key_features_label"]  # sticks for later key types, as in the reference (:666)
            if seen is None or unseen is None or keys.shape[-1] != seen.shape[-1] or keys.shape[-1] != unseen.shape[-1]:
                continue
            preds = {"seen": make_prediction(seen, keys, keys_label, max_k=max_k),
                     "unseen": make_prediction(unseen, keys, keys_label, max_k=max_k)}
            gts = {"seen": seen_dict["label_list"], "unseen": unseen_dict["label_list"]}
            pred_dict[q][kf] = {"curr_seen_pred_list": preds["seen"], "curr_unseen_pred_list": preds["unseen"]}
            for s in ("seen", "unseen"):
                macro, per_class = top_k_macro_accuracy(preds[s], gts[s], k_list=k_list)
                acc_dict[q][kf][s] = {"micro_acc": top_k_micro_accuracy(preds[s], gts[s], k_list=k_list),
                                      "macro_acc": macro}
                per_class_acc[q][kf][s] = per_class
    print_micro_and_macro_acc(acc_dict, k_list, args)
    return acc_dict, per_class_acc, pred_dict


HIP_EVAL_MODES = ("host", "gpu")


def eval_mode(args):
    """``hip_eval=host`` (default) or ``gpu``; anything else is refused."""
    mode = str(getattr(args, "hip_eval", "host"))
    if mode not in HIP_EVAL_MODES:
        raise ValueError(f"hip_eval must be one of {HIP_EVAL_MODES}, not {mode!r}")
    return mode


def select_eval(args):
    """``hip_eval=host`` (default): ``inference_and_print_result``; ``hip_eval=gpu``: ``inference_and_print_result_gpu``."""
    return inference_and_print_result_gpu if eval_mode(args) == "gpu" else inference_and_print_result


def _k_list(args):
    """``args.inference_and_eval_setting.k_list``; a configuration without the setting gets 1, 3, 5."""
    ies = getattr(args, "inference_and_eval_setting", None)
    return list(getattr(ies, "k_list", [1, 3, 5])) if ies is not None else [1, 3, 5]


def _silhouette(args):
    """``args.inference_and_eval_setting.silhouette`` (default false): print the silhouette scores of both query splits' image
    features after the accuracy table."""
    return bool(getattr(getattr(args, "inference_and_eval_setting", None), "silhouette", False))


def inference_and_print_result_gpu(keys_dict, seen_dict, unseen_dict, args=None, small_species_list=None, k_list=None,
                                   with_predictions=False):
    """``inference_and_print_result`` with the evaluation resident on the GPU: same cell loop, skip rules, printed table, ``acc_dict``
    and ``per_class_acc``.  Every key type's index is built once and every query feature uploaded once; the labels are encoded to
    int32 ids once per call.  ``pred_dict[q][kf]`` holds the int64 ``[Q, max_k]`` GPU index tensors (``curr_seen_indices`` /
    ``curr_unseen_indices``); ``with_predictions=True`` builds the host path's string lists from them instead."""
    from bioscanclip.hip.retrieval import HostSplit, encode_labels, score_cells
    if k_list is None:
        k_list = [1, 3, 5]
    label_lists = {"label_list": keys_dict["label_list"], "all_key_features_label": keys_dict.get("all_key_features_label") or [],
                   "seen": seen_dict["label_list"], "unseen": unseen_dict["label_list"]}
    arrays, vocab = encode_labels(*label_lists.values(), levels=LEVELS)
    label_ids = dict(zip(label_lists, arrays))
    keys = HostSplit(dict(keys_dict, all_key_features_label=label_lists["all_key_features_label"]),
                     {name: label_ids[name] for name in ("label_list", "all_key_features_label")})
    seen, unseen = HostSplit(seen_dict, {"label_list": label_ids["seen"]}), HostSplit(unseen_dict, {"label_list": label_ids["unseen"]})
    acc_dict, per_class_acc, pred_dict = score_cells(keys, seen, unseen, k_list, vocab, with_predictions=with_predictions)
    print_micro_and_macro_acc(acc_dict, k_list, args)
    return acc_dict, per_class_acc, pred_dict


EVAL_SPLITS = ("val", "test")


def shard_eval_loaders(args, with_text, which=None, batch_size=24):
    """The (keys, seen, unseen) evaluation loaders of ``eval_shards=<root>`` (``shards.eval_splits``): ``ShardLoader`` in evaluation mode
    (Resize -> CenterCrop, no shuffle) at the reference's batch 24 (:846); ``eval_split=val|test`` (default val) picks the query
    splits and ``hip_jpeg_entropy=host|gpu`` (default host) says where a JPEG shard's streams are Huffman-decoded."""
    from bioscanclip.util import shards
    which = str(getattr(args, "eval_split", "val")) if which is None else which
    if which not in EVAL_SPLITS:
        raise ValueError(f"eval_split must be one of {EVAL_SPLITS}, not {which!r}")
    entropy = getattr(args, "hip_jpeg_entropy", None)
    entropy = "host" if entropy is None or entropy == "" else str(entropy)
    if entropy not in shards.ENTROPY_MODES:
        raise ValueError(f"hip_jpeg_entropy must be one of {shards.ENTROPY_MODES}, got {entropy!r}")
    return [shards.ShardLoader(path, batch_size, for_training=False, shuffle=False, with_text=with_text, entropy=entropy)
            for path in shards.eval_splits(str(args.eval_shards), which)]


def main(argv=None):
    """Reference entry (scripts/inference_and_eval.py:786-871): config -> ``load_clip_model`` -> checkpoint
    (``model_config.ckpt_path`` unless ``model_config.load_ckpt`` is false, :839-843) -> features of the key / seen / unseen
    splits -> accuracy table.  The HDF5 splits are not available here: the splits come from the synthetic
    evaluation loaders, or with ``eval_shards=<root>`` from a directory of shard splits (``shard_eval_loaders``); extracted features
    are cached as ``.npz`` (h5py is absent) under the reference's directory layout
    (``extracted_embedding/<dataset>/<model_output_name>/``) and reused with ``load_inference=true`` (:797-833).
    ``hip_operands=fp16`` (default bf16) runs the three encoders on fp16 operands (``set_operand_format``); the cache records the
    format it was extracted with and is reused only by a run of the same format.  ``hip_eval=gpu`` (default host) scores the
    table with ``inference_and_print_result_gpu``.  Shard splits are walked once (``features.extract_split``); with ``hip_eval=gpu``
    their features, key indices and label ids stay on the GPU through the scoring (``retrieval.evaluate_resident``)."""
    from bioscanclip.hip.engine import OPERAND_FORMATS, set_operand_format
    from bioscanclip.util.config import load_config
    from bioscanclip.util.synthetic import SyntheticEvalLoader
    from bioscanclip.util.util import load_model_and_checkpoint
    here = os.path.dirname(os.path.abspath(__file__))
    args = load_config(os.path.join(here, "..", "bioscanclip", "config"), list(sys.argv[1:] if argv is None else argv))
    mc = args.model_config
    evaluate_splits = select_eval(args)
    from_shards = getattr(args, "eval_shards", None) not in (None, "")
    which = str(getattr(args, "eval_split", "val"))
    if from_shards and which not in EVAL_SPLITS:
        raise ValueError(f"eval_split must be one of {EVAL_SPLITS}, not {which!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("inference_and_eval needs a ROCm GPU: the encoders and the top-k search run in libbsclip_hip.so")
    device = torch.device("cuda", 0)
    k_list = _k_list(args)
    root = str(getattr(args, "project_root_path", "."))
    folder = os.path.join(root, "extracted_embedding", str(getattr(mc, "dataset", "synthetic")), str(mc.model_output_name))
    feats_path = os.path.join(folder, f"extracted_feature_from_{which if from_shards else 'val'}_split.npz")
    operands = str(getattr(args, "hip_operands", "bf16"))
    if operands not in OPERAND_FORMATS:
        raise ValueError(f"hip_operands must be one of {OPERAND_FORMATS}, not {operands!r}")
    splits, resident = None, None
    if getattr(args, "load_inference", False) and os.path.exists(feats_path):
        z = np.load(feats_path, allow_pickle=True)
        cached = str(z["operands"]) if "operands" in z.files else "bf16"   # caches from before the switch were extracted on bf16
        if cached == operands:
            splits = [z[k].item() for k in ("keys", "seen", "unseen")]
        else:
            print(f"Cached features were extracted with {cached} operands, this run uses {operands}: extracting again")
    if splits is None:
        print("Initialize model...")
        model, _ = load_model_and_checkpoint(args, device)
        set_operand_format(model, operands)
        model.eval()
        with_text = hasattr(mc, "language")
        if from_shards:
            from bioscanclip.hip.features import extract_splits
            resident = extract_splits(shard_eval_loaders(args, with_text, which), model, device, index=eval_mode(args) == "gpu")
            if eval_mode(args) == "host" or getattr(args, "save_inference", False):
                splits = [split.as_dict() for split in resident]
        else:
            bs, n = 24, int(getattr(args, "synthetic_eval_batches", 2))   # the reference evaluates at batch 24 (:846)
            mk = lambda seed: SyntheticEvalLoader(bs, n, with_text=with_text, seed=seed)
            splits = [get_features_and_label(mk(4321), model, device, for_key_set=True),
                      get_features_and_label(mk(4322), model, device), get_features_and_label(mk(4323), model, device)]
        if getattr(args, "save_inference", False):
            os.makedirs(folder, exist_ok=True)
            np.savez(feats_path, keys=np.array(splits[0], dtype=object), seen=np.array(splits[1], dtype=object),
                     unseen=np.array(splits[2], dtype=object), operands=np.array(operands))
    if resident is not None and eval_mode(args) == "gpu":
        from bioscanclip.hip.retrieval import evaluate_resident
        result = evaluate_resident(*resident, k_list=k_list, args=args)
        queries = [(s.tables["encoded_image_feature"], s.file_name_list, s.label_dicts()) for s in resident[1:]]
    else:
        keys_dict, seen_dict, unseen_dict = splits
        result = evaluate_splits(keys_dict, seen_dict, unseen_dict, args, small_species_list=None, k_list=k_list)
        queries = [(s["encoded_image_feature"], s["file_name_list"], s["label_list"]) for s in (seen_dict, unseen_dict)]
    if _silhouette(args):
        for image_features, names, label_list in queries:
            calculate_silhouette_score(args, image_features, (names, label_list))
    return result


if __name__ == "__main__":
    main()
