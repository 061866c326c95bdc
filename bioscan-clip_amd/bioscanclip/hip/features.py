"""One-pass feature extraction of an evaluation split, resident on the GPU.

``get_features_and_label`` (scripts/inference_and_eval.py, reference :734-784) walks a loader once per modality, downloads every feature
to a float64 array and leaves the scoring to upload them again.  On a shard loader each walk decodes and transforms every picture.
``extract_split`` walks the loader once: per batch every tower the model has runs exactly as ``get_feature_and_label`` runs it (the same
encoder call, then ``HF.l2_normalize(out.float())``), one ``bsclip_feature_rows`` launch files the batch into the split's device tables
(with the averaged and concatenated features), and for a key set ``bsclip_retrieval_index_append`` turns the same rows into the search
operand of every key type.  The label ids come straight from the shard's byte arrays (``shards.taxonomy_ids``).

    keys, seen, unseen = extract_splits([keys_loader, seen_loader, unseen_loader], model, device)
    acc_dict, per_class_acc, pred_dict = retrieval.evaluate_resident(keys, seen, unseen, [1, 3, 5])

``SplitFeatures.as_dict()`` is the host dictionary of ``get_features_and_label`` for everything that still wants it (``hip_eval=host``,
the ``.npz`` cache, ``calculate_silhouette_score``).
"""
import numpy as np
import torch

from . import functional as HF
from . import ops
from .retrieval import LEVELS, Labels, RetrievalIndex, decode_labels

_TABLE_OF = {"image": "encoded_image_feature", "dna": "encoded_dna_feature", "text": "encoded_language_feature"}


class SplitFeatures:
    """One split after ``extract_split``: ``tables[name]`` (f32 GPU ``[N, D]``, ``[N, 2 D]`` for the concatenated and ``[3 N, D]`` for the
    all-keys feature, or None where ``get_features_and_label`` has None), ``label_ids`` int32 ``[N, L]`` with their ``vocab``,
    ``file_name_list`` and, for a key set, ``indices[name]`` -- the ``RetrievalIndex`` of every key type, filled during the walk.
    The methods ``has`` / ``feature`` / ``query`` / ``index`` / ``labels`` / ``label_dicts`` are what ``retrieval.score_cells`` reads."""

    def __init__(self, file_name_list, tables, label_ids, vocab, indices, device, confidences=None, class_indices=None):
        self.file_name_list, self.tables, self.label_ids, self.vocab = file_name_list, tables, label_ids, vocab
        self.indices, self.device = indices, device
        self.confidences, self.class_indices = confidences, class_indices    # method two: [N, k] of the classifier that rode along
        self._labels = {}

    def has(self, name):
        return name in self.tables

    def feature(self, name):
        return self.tables[name]

    query = feature

    def index(self, name):
        if name not in self.indices:       # a query split searched as keys: built from the resident table, once
            self.indices[name] = RetrievalIndex(self.tables[name])
        return self.indices[name]

    def labels(self, name="label_list"):
        """The ``Labels`` of the split (uploaded once), or of the all-keys set: the same ids three times over."""
        if name not in self._labels:
            ids = self.label_ids if name == "label_list" else np.tile(self.label_ids, (3, 1))
            self._labels[name] = Labels(ids, self.device)
        return self._labels[name]

    def label_dicts(self, name="label_list"):
        dicts = decode_labels(self.label_ids, self.vocab, LEVELS)
        return dicts if name == "label_list" else dicts * 3

    def as_dict(self):
        """The dictionary ``get_features_and_label`` returns: float64 arrays holding the f32 values, label dictionaries, and for a key
        set with all three towers ``all_key_features`` with ``all_key_features_label = labels * 3``."""
        host = lambda t: None if t is None else t.cpu().numpy().astype(np.float64)
        labels = self.label_dicts()
        split = {"file_name_list": list(self.file_name_list)}
        for name in ("encoded_dna_feature", "encoded_image_feature", "encoded_language_feature", "averaged_feature", "concatenated_feature"):
            split[name] = host(self.tables[name])
        split["label_list"] = labels
        split["all_key_features"] = host(self.tables["all_key_features"])
        split["all_key_features_label"] = None if self.tables["all_key_features"] is None else labels + labels + labels
        return split


def _loader_labels(loader, labels):
    """(int32 ids in the loader's sample order, vocab) from ``labels`` = (ids of the whole shard, vocab), or from the shard alone."""
    from bioscanclip.util import shards
    if labels is None:
        arrays, vocab = shards.taxonomy_ids([loader.shard], LEVELS)
        labels = (arrays[0], vocab)
    ids, vocab = labels
    if len(ids) != len(loader.shard):
        raise ValueError(f"{len(ids)} label rows for a shard of {len(loader.shard)} samples")
    order = np.asarray(loader.indices(), dtype=np.int64)
    return np.ascontiguousarray(np.asarray(ids, dtype=np.int32)[order]), vocab


def extract_split(loader, model, device, for_key_set=False, index=True, labels=None, towers=None, classifier=None, n_classes=None,
                  top_k=5, append_to=None):
    """One walk over ``loader`` (a ``ShardLoader(for_training=False)``): the features of every tower ``model`` has, in device tables.

    ``towers``: run only these of ``"image"``, ``"dna"``, ``"text"`` (each must exist in the model); the other towers' tables stay
    None, as for a model without them.  The seen / unseen protocols need the image tower for their query splits and seen keys and
    the DNA tower for their unseen keys, nothing else.
    ``classifier`` (method two; ``n_classes`` = its C): the same walk also runs this image classifier on every batch and
    ``bsclip_class_softmax_topk`` writes its ``top_k`` confidences and class indices into rows ``[row0, row0 + B)`` of the split's
    ``confidences`` f32 / ``class_indices`` int64 ``[N, top_k]`` tables.
    ``append_to = {table name: (RetrievalIndex, first row)}``: every batch's rows of that table are also appended to an index the
    caller owns, from that row on -- one index over the key splits of several walks.

    ``labels``: ``(ids, vocab)`` of the loader's whole shard as ``shards.taxonomy_ids`` returns them for it -- pass the ids encoded
    together with the other splits' so that the three share one vocabulary (``extract_splits`` does); default: the shard on its own.
    ``for_key_set``: with all three towers the image, DNA and text tables are the three thirds of one ``[3 N, D]`` allocation, which
    then is ``all_key_features`` without a copy; and, unless ``index`` is false, every key type's ``RetrievalIndex`` is filled batch by
    batch.  Returns a ``SplitFeatures``."""
    device = torch.device(device)
    encoders = {"image": model.image_encoder, "dna": model.dna_encoder, "text": model.language_encoder}
    if towers is None:
        towers = [m for m, enc in encoders.items() if enc is not None]
    else:
        towers = [m for m in encoders if m in tuple(towers)]
        absent = [m for m in towers if encoders[m] is None]
        if absent or len(towers) != len(tuple(towers)):
            raise ValueError(f"extract_split: towers must name encoders of the model (image, dna, text); the model has no {absent}")
    if not towers:
        raise ValueError("extract_split: the model has no encoder")
    if classifier is not None and (n_classes is None or not 1 <= int(top_k) <= min(16, int(n_classes))):
        raise ValueError("extract_split: a classifier needs n_classes and 1 <= top_k <= min(16, n_classes)")
    append_to = dict(append_to or {})
    if "text" in towers and not getattr(loader, "with_text", True):
        raise ValueError("extract_split: the model has a text tower but the loader was built with with_text=False")
    label_ids, vocab = _loader_labels(loader, labels)
    N = len(label_ids)
    if N < 1:
        raise ValueError("extract_split: the split is empty")
    both, every = "image" in towers and "dna" in towers, len(towers) == 3
    tables = dict.fromkeys([*_TABLE_OF.values(), "averaged_feature", "concatenated_feature", "all_key_features"])
    indices, names, row0 = {}, [], 0
    conf = class_idx = None
    if classifier is not None:
        conf = torch.empty(N, int(top_k), dtype=torch.float32, device=device)
        class_idx = torch.empty(N, int(top_k), dtype=torch.int64, device=device)

    def allocate(D):
        new = lambda rows, width: torch.empty(rows, width, dtype=torch.float32, device=device)
        if for_key_set and every:
            tables["all_key_features"] = new(3 * N, D)
            for k, m in enumerate(("image", "dna", "text")):       # the order of np.concatenate((image, dna, lang), axis=0)
                tables[_TABLE_OF[m]] = tables["all_key_features"][k * N:(k + 1) * N]
        else:
            for m in towers:
                tables[_TABLE_OF[m]] = new(N, D)
        if both:
            tables["averaged_feature"], tables["concatenated_feature"] = new(N, D), new(N, 2 * D)
        if for_key_set and index:
            for name, t in tables.items():
                if t is not None:
                    indices[name] = RetrievalIndex.empty(t.shape[0], t.shape[1], device)

    model.eval()
    with torch.no_grad():
        for processid, image, dna, input_ids, token_type_ids, attention_mask, _ in loader:
            out = {}
            if classifier is not None:
                if row0 + image.shape[0] > N:
                    raise RuntimeError(f"extract_split: the loader yielded more than its {N} samples")
                ops.class_softmax_topk(classifier(image.to(device)), int(n_classes), int(top_k),
                                       out=(conf[row0:row0 + image.shape[0]], class_idx[row0:row0 + image.shape[0]]))
            if "image" in towers:
                out["image"] = HF.l2_normalize(encoders["image"](image.to(device)).float())
            if "dna" in towers:
                out["dna"] = HF.l2_normalize(encoders["dna"](dna.to(device)).float())
            if "text" in towers:
                out["text"] = HF.l2_normalize(encoders["text"]({"input_ids": input_ids.to(device), "token_type_ids": token_type_ids.to(device),
                                                                "attention_mask": attention_mask.to(device)}).float())
            out = {m: t.contiguous() for m, t in out.items()}
            B, D = out[towers[0]].shape
            if row0 == 0:
                allocate(D)
            if row0 + B > N:
                raise RuntimeError(f"extract_split: the loader yielded more than its {N} samples")
            ops.feature_rows(out.get("image"), out.get("dna"), out.get("text"), row0,
                             *[tables[_TABLE_OF[m]] if m in out else None for m in ("image", "dna", "text")],
                             t_avg=tables["averaged_feature"], t_cat=tables["concatenated_feature"])
            for name, idx in indices.items():
                if name == "all_key_features":
                    for k in range(3):
                        idx.append(tables[name][k * N + row0:k * N + row0 + B], k * N + row0)
                else:
                    idx.append(tables[name][row0:row0 + B], row0)
            for name, (idx, first) in append_to.items():
                idx.append(tables[name][row0:row0 + B], int(first) + row0)
            names += list(processid)
            row0 += B
    if row0 != N:
        raise RuntimeError(f"extract_split: the loader yielded {row0} of its {N} samples")
    return SplitFeatures(names, tables, label_ids, vocab, indices, device, confidences=conf, class_indices=class_idx)


def extract_splits(loaders, model, device, index=True):
    """``extract_split`` of the (keys, seen, unseen) loaders with their labels encoded together (one vocabulary, the ids
    ``retrieval.encode_labels`` gives the three label lists in that order): what ``retrieval.evaluate_resident`` takes."""
    from bioscanclip.util import shards
    arrays, vocab = shards.taxonomy_ids([ld.shard for ld in loaders], LEVELS)
    return [extract_split(ld, model, device, for_key_set=(i == 0), index=index, labels=(ids, vocab))
            for i, (ld, ids) in enumerate(zip(loaders, arrays))]
