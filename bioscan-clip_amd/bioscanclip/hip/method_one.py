"""GPU-resident method-one evaluation (reference scripts/method_one_eval.py): an image query is searched in the seen keys (image
features) and in the unseen keys (DNA features); rank slot r keeps the seen-key prediction when its similarity is above a threshold
and takes the unseen-key prediction otherwise; the threshold is the one that maximises the harmonic mean of the splits' top-1
species micro accuracy.

On int32 label ids (``retrieval.encode_labels``) the two prediction lists of a query are two bit masks per level -- bit r of
``A[q, l]`` / ``B[q, l]`` says whether the r-th seen-key / unseen-key hit carries the query's own label -- and everything the
reference rebuilds as lists of strings for each of its 1 000 thresholds is ``(A & s) | (B & ~s)`` with ``s`` the selection mask:

    seen_index, unseen_index = RetrievalIndex(seen_key_image_features), RetrievalIndex(unseen_key_dna_features)
    split = MethodOneSplit.from_queries(seen_index, seen_key_labels, unseen_index, unseen_key_labels, query_features, query_labels)
    counts, totals = sweep([split_a, split_b], thresholds)            # one launch per split, one download
    t = pick_threshold(counts, totals, thresholds)                    # host, the reference's arithmetic
    acc, per_class = merged_accuracy(split, t, [1, 3, 5], vocab)      # merge -> class counts -> assemble_accuracy
    shares = member_share(split, t, member_table)                     # check_for_acc_about_correct_predict_seen_or_unseen

The kernels return integers only; the ratios are formed on the host in float64 in the reference's order of operations, so every
number equals the string path's with ``==``.  There is no CPU path for the searches, the masks, the merge and the sweep.
"""
import numpy as np
import torch

from . import ops
from .retrieval import LEVELS, Labels, score_hit_ranks, to_gpu


class MethodOneSplit:
    """One query split: the results of its image queries' two searches (``from_queries`` runs them against indices the caller built
    once and shares between splits), and what the merge needs of them, all on the GPU -- ``sim`` f32 ``[Q, k]`` (seen-key
    similarities), ``A`` / ``B`` int32 ``[Q, L]``, the int64 index tensors of both searches, the query ``Labels`` and the error word
    the mask kernels OR into.  Member masks are made on demand per member table (``member_masks``)."""

    def __init__(self, sim, idx_seen, seen_key_labels, idx_unseen, unseen_key_labels, query_labels, levels=None):
        dev = sim.device
        self.seen_keys, self.unseen_keys, self.labels = (Labels.of(x, dev) for x in (seen_key_labels, unseen_key_labels, query_labels))
        if sim.shape[0] != self.labels.ids.shape[0] or idx_seen.shape != sim.shape or idx_unseen.shape != sim.shape:
            raise ValueError("sim, idx_seen and idx_unseen must be [Q, k] for the Q query labels")
        self.sim, self.idx_seen, self.idx_unseen = sim, idx_seen, idx_unseen
        self.Q, self.k = int(sim.shape[0]), int(sim.shape[1])
        self.levels = list(LEVELS[:self.labels.ids.shape[1]] if levels is None else levels)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.A = ops.retrieval_match_bits(idx_seen, self.seen_keys.dev, self.labels.dev, flag=self.flag)
        self.B = ops.retrieval_match_bits(idx_unseen, self.unseen_keys.dev, self.labels.dev, flag=self.flag)
        self._members = {}

    @classmethod
    def from_queries(cls, seen_index, seen_key_labels, unseen_index, unseen_key_labels, queries, query_labels, max_k=5, levels=None):
        """Search the image ``queries`` (numpy or GPU tensor ``[Q, D]``) in the seen-key index (image features) and in the
        unseen-key index (DNA features), ``max_k`` deep; the key labels are ``Labels`` (or int32 arrays) in key order."""
        queries = to_gpu(queries, seen_index.device)
        seen_key_labels, unseen_key_labels = seen_index.key_labels(seen_key_labels), unseen_index.key_labels(unseen_key_labels)
        sim, idx_seen = seen_index.search(queries, int(max_k))
        _, idx_unseen = unseen_index.search(queries, int(max_k))
        return cls(sim, idx_seen, seen_key_labels, idx_unseen, unseen_key_labels, query_labels, levels=levels)

    def member_masks(self, member, level="species"):
        """(mA, mB) int32 ``[Q]``: bit r set exactly when the r-th seen-key / unseen-key hit's id at ``level`` is listed in
        ``member`` (int32 0/1 over that level's ids, numpy or GPU tensor).  Cached per table object."""
        key = (id(member), level)
        if key not in self._members:
            l = self.levels.index(level)
            table = to_gpu(member, self.sim.device, dtype=np.int32)
            self._members[key] = (member, ops.retrieval_match_bits(self.idx_seen, self.seen_keys.dev, member=table, level=l, flag=self.flag),
                                  ops.retrieval_match_bits(self.idx_unseen, self.unseen_keys.dev, member=table, level=l, flag=self.flag))
        return self._members[key][1:]


def linspace_thresholds(num_intervals=1000):
    """The reference's grid: ``np.linspace(0, 1, num_intervals)``, float64."""
    return np.linspace(0, 1, num_intervals)


def sweep(splits, thresholds, level="species", k=1):
    """Per split and threshold, the number of queries whose merged top-``k`` list holds their own ``level`` label: one sweep launch
    per split, one download.  Returns ``(counts int64 [n_splits, T], totals [n_splits])``."""
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    dev = splits[0].sim.device
    thr_dev = torch.from_numpy(thr).to(dev)
    n, T = len(splits), thr.shape[0]
    buf = torch.zeros(n * T + n, dtype=torch.int32, device=dev)       # [counts | one error word per split]
    for i, sp in enumerate(splits):
        ops.retrieval_threshold_sweep(sp.sim, sp.A, sp.B, sp.levels.index(level), min(int(k), sp.k), thr_dev, out=buf[i * T:(i + 1) * T])
        buf[n * T + i:n * T + i + 1].copy_(sp.flag)
    host = buf.cpu().numpy()
    for word in host[n * T:].tolist():
        ops.check_retrieval_flag(int(word))
    return host[:n * T].reshape(n, T).astype(np.int64), [sp.Q for sp in splits]


def harmonic_mean(values):
    """0 when any term is 0, otherwise ``len / sum(1 / a)`` summed left to right (reference :121-128)."""
    total = 0
    for v in values:
        if v == 0:
            return 0
        total = total + 1 / v
    return len(values) / total


def pick_threshold(counts, totals, thresholds):
    """Host only: the first threshold whose harmonic mean over the splits' accuracies ``count * 1.0 / total`` is strictly greater
    than every earlier one (the running maximum starts at -inf), as ``search_threshold_with_harmonic_mean`` picks it."""
    best, top = None, float("-inf")
    for j, t in enumerate(thresholds):
        score = harmonic_mean([int(row[j]) * 1.0 / total for row, total in zip(counts, totals)])
        if score > top:
            top, best = score, t
    return best


def merged_accuracy(split, threshold, k_list, vocab=None):
    """The accuracy tables of the merged lists at ``threshold``: merge, class counts, ``assemble_accuracy``; one download.  Returns
    ``({"micro_acc": ..., "macro_acc": ...}, per_class_acc)`` like ``retrieval.evaluate``."""
    hit_rank = ops.retrieval_merge_hit_ranks(split.sim, split.A, split.B, threshold)
    return score_hit_ranks(hit_rank, split.labels, k_list, split.k, flag=split.flag, vocab=vocab, levels=split.levels)


def member_share(split, threshold, member, ks=(1, 3, 5), level="species"):
    """For each k' of ``ks`` the share of queries whose merged top-k' ``level`` predictions hold a listed id (``member``: int32 0/1
    over the level's ids): the merge over the member masks, counted by the sweep kernel at the single threshold; one download."""
    mA, mB = split.member_masks(member, level)
    dev = split.sim.device
    thr = torch.tensor([float(threshold)], dtype=torch.float64, device=dev)
    buf = torch.zeros(len(ks) + 1, dtype=torch.int32, device=dev)
    for j, k in enumerate(ks):
        ops.retrieval_threshold_sweep(split.sim, mA, mB, 0, min(int(k), split.k), thr, out=buf[j:j + 1])
    buf[len(ks):].copy_(split.flag)
    host = buf.cpu().numpy().tolist()
    ops.check_retrieval_flag(int(host[-1]))
    return {k: host[j] * 1.0 / split.Q for j, k in enumerate(ks)}


def merged_predictions(split, threshold, seen_key_names, unseen_key_names):
    """The merged lists as the host path builds them, ``[{level: [name] * k}]``, from the index tensors (one download each) and
    the keys' label dicts; only ``with_predictions=True`` asks for them."""
    sim = split.sim.cpu().numpy().tolist()
    ia, ib = split.idx_seen.cpu().numpy().tolist(), split.idx_unseen.cpu().numpy().tolist()
    out = []
    for s_row, a_row, b_row in zip(sim, ia, ib):
        picks = [seen_key_names[a] if s > threshold else unseen_key_names[b] for s, a, b in zip(s_row, a_row, b_row)]
        out.append({lv: [p[lv] for p in picks] for lv in split.levels})
    return out
