"""GPU-resident retrieval evaluation: a key index built once per key set (faiss ``index.add`` once, many ``search``), label matching
and per-class counting as HIP kernels on integer label ids, and the host assembly of the accuracy tables from those integers.

What the reference does per (query type, key type, split) cell in ``make_prediction`` / ``top_k_micro_accuracy`` /
``top_k_macro_accuracy`` (scripts/inference_and_eval.py:414-511) on lists of strings happens here on int32 ids:

    index = RetrievalIndex(keys)                                      # normalise + split the keys once
    (key_ids, query_ids), vocab = encode_labels(key_labels, query_labels)
    acc, per_class = evaluate(index, key_ids, queries, query_ids, [1, 3, 5], vocab=vocab)

The kernels return integers only (first hit rank per query and level, per-class histograms); the ratios are formed here in float64
in the reference's order of operations, so the tables equal the string path's bit for bit.  There is no CPU path for the search
and the counting: without the HIP library or a GPU they raise.
"""
import numpy as np
import torch

from . import ops

LEVELS = ["order", "family", "genus", "species"]


def to_gpu(x, device=None, dtype=np.float32):
    """A numpy array (made contiguous ``dtype``, uploaded to ``device``, default ``"cuda"``) or a tensor (left where and what it is)
    as a contiguous tensor: what the wrappers in ``ops`` take."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=dtype)).to(torch.device(device if device is not None else "cuda"))
    return x.contiguous()


def encode_labels(*label_lists, levels=None):
    """Map the strings of each level to dense int32 ids shared by all the given label lists (each a list of ``{level: name}``).

    Returns ``(arrays, vocab)``: one int32 ``[N, L]`` array per label list and ``vocab[level]`` = the names in id order (ids are
    handed out in order of first appearance, per level).  No name is special: equal strings get equal ids and nothing else does.
    """
    levels = list(LEVELS if levels is None else levels)
    table = {lv: {} for lv in levels}
    arrays = []
    for labels in label_lists:
        ids = np.empty((len(labels), len(levels)), dtype=np.int32)
        for j, lv in enumerate(levels):
            t = table[lv]
            ids[:, j] = [t.setdefault(lab[lv], len(t)) for lab in labels]
        arrays.append(ids)
    return arrays, {lv: list(table[lv]) for lv in levels}


def decode_labels(ids, vocab, levels=None):
    """Inverse of ``encode_labels`` for one array: the list of ``{level: name}``."""
    levels = list(vocab if levels is None else levels)
    return [{lv: vocab[lv][i] for lv, i in zip(levels, row)} for row in np.asarray(ids).tolist()]


class Labels:
    """One split's label ids, int32 ``[N, L]``: the host copy, the GPU copy (uploaded once) and, for the query role, what the
    assembly needs of them -- per level the class range and the classes in order of first appearance."""

    def __init__(self, ids, device=None):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2 or not 1 <= ids.shape[1] <= 8:
            raise ValueError("label ids must be [N, L] with 1 <= L <= 8")
        if ids.size and ids.min() < 0:
            raise ValueError("label ids must be >= 0")
        self.ids = ids
        self.dev = torch.from_numpy(ids).to(torch.device(device if device is not None else "cuda"))
        self._order = None

    @classmethod
    def of(cls, labels, device=None):
        """``labels`` itself when it is a ``Labels`` already, else the ``Labels`` of that int32 array on ``device``."""
        return labels if isinstance(labels, cls) else cls(labels, device)

    @property
    def level_offsets(self):
        sizes = (self.ids.max(axis=0) + 1) if len(self.ids) else np.zeros(self.ids.shape[1], dtype=np.int64)
        return [0] + np.cumsum(sizes, dtype=np.int64).tolist()

    @property
    def class_order(self):
        if self._order is None:
            self._order = [first_appearance_order(self.ids[:, j]) for j in range(self.ids.shape[1])]
        return self._order


def first_appearance_order(ids):
    """The distinct values of a 1-D id array in order of first appearance (the iteration order of the reference's ``seen`` dict)."""
    u, first = np.unique(ids, return_index=True)
    return u[np.argsort(first, kind="stable")]


class RetrievalIndex:
    """``faiss.IndexFlatIP(d).add(normalize(keys))`` kept on the GPU: the keys (f32 GPU tensor or numpy array, ``[K, D]``) are
    uploaded, L2-normalised and split into the search kernels' operand once; ``search`` only reads it."""

    def __init__(self, keys, device=None):
        keys = to_gpu(keys, device)
        self.K, self.D = int(keys.shape[0]), int(keys.shape[1])
        self.device = keys.device
        self.index = ops.retrieval_index_build(keys)

    @classmethod
    def empty(cls, K, D, device=None):
        """An index of K keys of width D with no row written yet (a zero-filled operand): ``append`` fills it as the keys arrive.
        Once every row in ``[0, K)`` has been appended it is, bit for bit, ``RetrievalIndex(keys)`` of the whole table."""
        self = cls.__new__(cls)
        self.K, self.D = int(K), int(D)
        self.index = ops.retrieval_index_empty(self.K, self.D, torch.device(device if device is not None else "cuda"))
        self.device = self.index.device
        return self

    def append(self, rows, row0):
        """``rows`` (f32 GPU ``[n, D]``) become the keys ``[row0, row0 + n)``."""
        ops.retrieval_index_append(self.index, self.K, rows, int(row0))

    def search(self, queries, k):
        """(similarities f32 ``[Q, k]``, indices int64 ``[Q, k]``) as GPU tensors -- what ``ops.topk_ip(queries, keys, k)`` returns."""
        return ops.topk_ip_indexed(to_gpu(queries, self.device), self.index, self.K, int(k))

    def key_labels(self, labels):
        """``labels`` (``Labels`` or int32 ``[K', L]``, in key order) as the ``Labels`` of this index's keys; K' < K raises."""
        labels = Labels.of(labels, self.device)
        if labels.ids.shape[0] < self.K:
            raise ValueError(f"{labels.ids.shape[0]} key labels for an index of {self.K} keys")
        return labels


def assemble_accuracy(seen, right, query_ids, level_offsets, k_list, class_order=None, vocab=None, levels=None):
    """Micro / macro / per-class accuracy from the integer counts, in the reference's arithmetic (:448-511).

    ``seen`` int ``[C]`` and ``right`` int ``[nk, C]`` are the per-class histograms over the flat class range laid out by
    ``level_offsets``; ``query_ids`` int ``[Q, L]``.  Per level: micro = (sum of ``right`` over the level) * 1.0 / Q; per class
    ``right * 1.0 / seen``; macro = the running sum of those in order of first appearance among the queries, divided by the number
    of classes seen -- float64 throughout, as Python does on the reference's ints.  Classes are named through ``vocab`` (else by id).
    """
    query_ids = np.asarray(query_ids)
    Q, L = query_ids.shape
    levels = list((vocab if vocab is not None else LEVELS[:L]) if levels is None else levels)
    if len(levels) != L:
        raise ValueError(f"{L} label columns but {len(levels)} level names")
    if class_order is None:
        class_order = [first_appearance_order(query_ids[:, j]) for j in range(L)]
    seen, right = np.asarray(seen), np.asarray(right)
    micro, macro, per_class = {}, {}, {}
    for i, k in enumerate(k_list):
        micro[k], macro[k], per_class[k] = {}, {}, {}
        for j, lv in enumerate(levels):
            lo, hi = level_offsets[j], level_offsets[j + 1]
            micro[k][lv] = int(right[i, lo:hi].sum()) * 1.0 / Q
            order = class_order[j]
            ratios = right[i, lo + order].astype(np.float64) / seen[lo + order].astype(np.float64)
            names = [vocab[lv][c] for c in order.tolist()] if vocab is not None else order.tolist()
            per_class[k][lv] = dict(zip(names, ratios.tolist()))
            macro[k][lv] = float(np.cumsum(ratios)[-1]) / len(order)   # cumsum adds left to right, like the reference's loop
    return {"micro_acc": micro, "macro_acc": macro}, per_class


def checked_k_list(k_list):
    """``k_list`` as a list: 1 to 8 values, each >= 1 (what ``bsclip_retrieval_class_counts`` takes)."""
    k_list = list(k_list)
    if not 1 <= len(k_list) <= 8 or min(k_list) < 1:
        raise ValueError("k_list: 1 to 8 values, each >= 1")
    return k_list


def score_hit_ranks(hit_rank, labels, k_list, depth, flag=None, vocab=None, levels=None):
    """The accuracy tables of one cell from its hit ranks (int32 GPU ``[Q, L]``, each below ``depth`` or equal to it for no hit)
    and the query ``Labels``: class counts, ONE download, the error-word check, ``assemble_accuracy``.  A k of ``k_list`` above
    ``depth`` counts hits in the whole list, like the reference's ``pred[:k]``.  ``flag``: the int32 ``[1]`` word the kernels before
    this one ORed their errors into (default: none so far).  Returns ``(acc, per_class)`` as ``evaluate`` does."""
    k_list = checked_k_list(k_list)
    offsets = labels.level_offsets
    C, nk = offsets[-1], len(k_list)
    buf = torch.empty(1 + (1 + nk) * C, dtype=torch.int32, device=hit_rank.device)   # [flag | seen | right]: one download per cell
    word = buf[:1].zero_() if flag is None else buf[:1].copy_(flag)
    ops.retrieval_class_counts(hit_rank, labels.dev, offsets, [min(k, depth) for k in k_list], flag=word, out=buf[1:])
    host = buf.cpu().numpy()
    ops.check_retrieval_flag(int(host[0]))
    return assemble_accuracy(host[1:1 + C], host[1 + C:].reshape(nk, C), labels.ids, offsets, k_list, class_order=labels.class_order,
                             vocab=vocab, levels=levels)


def evaluate(index, key_label_ids, queries, query_label_ids, k_list, max_k=None, vocab=None, levels=None, return_indices=False):
    """One cell of the accuracy table on the GPU: search ``queries`` in ``index``, match labels, count per class.

    ``key_label_ids`` / ``query_label_ids``: int32 ``[K', L]`` (K' >= the index's K) / ``[Q, L]`` as numpy arrays or ``Labels``
    (uploaded once, reusable across cells).  ``max_k`` (default ``max(k_list)``) is the search depth; a k above it counts hits in
    the whole list, like the reference's ``pred[:k]``.  Returns ``({"micro_acc": {k: {level: float}}, "macro_acc": {...}},
    per_class)`` with ``per_class[k][level][class] = float`` -- the structures of ``top_k_micro_accuracy`` /
    ``top_k_macro_accuracy`` -- and, with ``return_indices``, the int64 ``[Q, max_k]`` GPU tensor of key indices as a third item.
    """
    k_list = checked_k_list(k_list)                                   # before the search, which takes its depth from it
    max_k = max(k_list) if max_k is None else int(max_k)
    kl, ql = index.key_labels(key_label_ids), Labels.of(query_label_ids, index.device)
    _, idx = index.search(queries, max_k)
    if idx.shape[0] != ql.ids.shape[0] or kl.ids.shape[1] != ql.ids.shape[1]:
        raise ValueError("query labels do not match the queries, or key and query labels differ in levels")
    flag = torch.zeros(1, dtype=torch.int32, device=idx.device)
    hit_rank = ops.retrieval_hit_ranks(idx, kl.dev, ql.dev, flag=flag)
    acc, per_class = score_hit_ranks(hit_rank, ql, k_list, max_k, flag=flag, vocab=vocab, levels=levels)
    return (acc, per_class, idx) if return_indices else (acc, per_class)


# ---- the accuracy table of three splits (inference_and_print_result, reference scripts/inference_and_eval.py:633-715) ------------

QUERY_FEATURES = ["encoded_image_feature", "encoded_dna_feature", "encoded_language_feature", "averaged_feature", "concatenated_feature"]
KEY_FEATURES = QUERY_FEATURES + ["all_key_features"]


class HostSplit:
    """One split given as the host dictionary of ``get_features_and_label`` plus its encoded label ids (``ids[name]`` for ``name`` in
    ``label_list`` / ``all_key_features_label``), in the form ``score_cells`` reads: every feature uploaded once, every key type's
    index built once, every label array uploaded once.  ``features.SplitFeatures`` offers the same five methods on tables that
    never left the GPU."""

    def __init__(self, split, ids):
        self.split, self.ids = split, ids
        self._gpu, self._index, self._labels = {}, {}, {}

    def has(self, name):
        return name in self.split

    def feature(self, name):
        return self.split[name]

    def query(self, name):
        if name not in self._gpu:
            self._gpu[name] = to_gpu(self.split[name])
        return self._gpu[name]

    def index(self, name):
        if name not in self._index:
            self._index[name] = RetrievalIndex(self.split[name])
        return self._index[name]

    def labels(self, name="label_list"):
        if name not in self._labels:
            self._labels[name] = Labels(self.ids[name])
        return self._labels[name]

    def label_dicts(self, name="label_list"):
        return self.split[name]


def score_cells(keys, seen, unseen, k_list, vocab, with_predictions=False):
    """The cell loop of ``inference_and_print_result`` on splits resident on the GPU (``HostSplit`` or ``features.SplitFeatures``):
    the same order, skip rules and sticky ``all_key_features_label`` rule.  Returns ``(acc_dict, per_class_acc, pred_dict)``;
    ``pred_dict[q][kf]`` holds the int64 ``[Q, max_k]`` GPU index tensors (``curr_seen_indices`` / ``curr_unseen_indices``), or with
    ``with_predictions`` the host path's string lists (``curr_seen_pred_list`` / ``curr_unseen_pred_list``)."""
    max_k = k_list[-1]
    acc_dict, per_class_acc, pred_dict = {}, {}, {}
    keys_label = "label_list"
    for q in QUERY_FEATURES:
        if not seen.has(q):
            continue
        acc_dict[q], per_class_acc[q], pred_dict[q] = {}, {}, {}
        for kf in KEY_FEATURES:
            if not keys.has(kf):
                continue
            acc_dict[q][kf], per_class_acc[q][kf], pred_dict[q][kf] = {}, {}, {}
            key_f, seen_f, unseen_f = keys.feature(kf), seen.feature(q), unseen.feature(q)
            if key_f is None:
                continue
            if kf == "all_key_features":
                keys_label = "all_key_features_label"  # sticks for later key types, as in the reference (:666)
            if seen_f is None or unseen_f is None or key_f.shape[-1] != seen_f.shape[-1] or key_f.shape[-1] != unseen_f.shape[-1]:
                continue
            for s, split in (("seen", seen), ("unseen", unseen)):
                acc, per_class, idx = evaluate(keys.index(kf), keys.labels(keys_label), split.query(q), split.labels(), k_list,
                                               max_k=max_k, vocab=vocab, levels=LEVELS, return_indices=True)
                acc_dict[q][kf][s], per_class_acc[q][kf][s] = acc, per_class
                if with_predictions:
                    names = keys.label_dicts(keys_label)
                    pred_dict[q][kf][f"curr_{s}_pred_list"] = [{level: [names[i][level] for i in row] for level in LEVELS}
                                                              for row in idx.cpu().numpy()]
                else:
                    pred_dict[q][kf][f"curr_{s}_indices"] = idx
    return acc_dict, per_class_acc, pred_dict


def print_accuracy_table(acc_dict, k_list):
    """The printed table of the reference's ``print_micro_and_macro_acc``: one line per (query type, key type, kind, k)."""
    for q in QUERY_FEATURES:
        for kf in KEY_FEATURES:
            cell = acc_dict.get(q, {}).get(kf)
            if not cell:
                continue
            for kind in ("micro_acc", "macro_acc"):
                for k in k_list:
                    nums = [round(cell[s][kind][k][level], 4) for s in ("seen", "unseen") for level in LEVELS]
                    print(f"Query_feature: {q}||Key_feature: {kf}||{kind} top-{k}\t" + "\t".join(map(str, nums)))


def evaluate_resident(keys, seen, unseen, k_list=None, args=None, with_predictions=False):
    """``inference_and_print_result_gpu`` on three ``features.SplitFeatures``: the tables, the key indices filled during extraction and
    the ``Labels`` are read where they are -- nothing is downloaded, uploaded or encoded again.  The three splits must share one
    vocabulary (``features.extract_splits``, or ``shards.taxonomy_ids`` over the three shards).  Same cell loop (``score_cells``),
    printed table and return value."""
    if k_list is None:
        k_list = [1, 3, 5]
    if not (keys.vocab == seen.vocab == unseen.vocab):
        raise ValueError("evaluate_resident: the three splits were encoded with different vocabularies; encode their labels together "
                         "(features.extract_splits, or shards.taxonomy_ids over the three shards)")
    result = score_cells(keys, seen, unseen, k_list, keys.vocab, with_predictions=with_predictions)
    print_accuracy_table(result[0], k_list)
    return result
