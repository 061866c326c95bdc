"""GPU-resident method-two evaluation (reference scripts/method_two_fine_tuning_and_eval.py): a copy of the image encoder fine-tuned
as a species classifier gives, per image query, its five highest softmax confidences (:57-62); the same query, encoded by the
original model, is searched in the DNA keys of the unseen species; rank slot r keeps the classifier's prediction when its confidence
is above a threshold and takes the search's otherwise (:88-114); the threshold is the one of ``np.linspace(0, 1, 1001)`` with the best
seen / unseen harmonic mean (:177-204).

On label ids the classifier side is a "search" already: class c is a key whose labels are row c of an int32 class table ``[C, L]``
made from ``idx_to_all_labels``, the predicted class indices are the key indices and the confidences the similarities.  So a split is
a ``MethodOneSplit`` and method one's ``sweep``, ``pick_threshold``, ``merged_accuracy``, ``member_share`` and ``merged_predictions``
apply unchanged (they are re-exported here):

    conf, idx, gt = classifier_confidences(classifier, loader, device, C)            # logits -> bsclip_class_softmax_topk, on the GPU
    split = MethodTwoSplit.from_classifier(conf, idx, class_table, unseen_index, unseen_key_labels, query_features, query_labels)
    thresholds = linspace_thresholds(1000)                                           # 1001 points
    counts, totals = sweep([seen_split, unseen_split], thresholds)
    t = pick_threshold(counts, totals, thresholds)
    acc, per_class = merged_accuracy(split, t, [1, 3, 5], vocab)

Order inside a query's k slots: by logit descending, ties to the lower class index (``ops.class_softmax_topk``).
"""
import numpy as np
import torch

from . import ops
from ..epoch.eval_epoch import convert_label_dict_to_list_of_dict
from .method_one import (MethodOneSplit, member_share, merged_accuracy, merged_predictions, pick_threshold,  # noqa: F401
                         sweep)
from .retrieval import Labels, to_gpu

try:  # optional, as in the epoch drivers
    from tqdm import tqdm
except Exception:  # pragma: no cover
    tqdm = None


def linspace_thresholds(num_intervals=1000):
    """The reference's method-two grid (:179): ``np.linspace(0, 1, num_intervals + 1)``, float64 -- ``num_intervals + 1`` points,
    one more than method one's ``np.linspace(0, 1, num_intervals)``."""
    return np.linspace(0, 1, num_intervals + 1)


def classifier_confidences(classifier, dataloader, device, C, k=5):
    """Reference :41-71 without the download: per batch ``classifier(x)`` under ``no_grad`` and ``ops.class_softmax_topk`` on its
    ``C`` logits.  Returns ``(conf f32 [Q, k], idx int64 [Q, k], gt_labels)`` with both tensors on the GPU."""
    confs, idxs, gt_labels = [], [], []
    steps = dataloader if tqdm is None else tqdm(dataloader, total=len(dataloader))
    with torch.no_grad():
        for batch in steps:
            output = classifier(batch[1].to(device))
            conf, idx = ops.class_softmax_topk(output, int(C), int(k))
            confs.append(conf)
            idxs.append(idx)
            gt_labels += convert_label_dict_to_list_of_dict(batch[6])
    if not confs:
        raise ValueError("classifier_confidences: the dataloader is empty")
    return torch.cat(confs), torch.cat(idxs), gt_labels


class MethodTwoSplit(MethodOneSplit):
    """One query split of method two: ``MethodOneSplit`` with the classifier in the seen-key role -- ``sim`` are the confidences,
    ``idx_seen`` the predicted class indices, ``seen_keys`` the class table."""

    def __init__(self, conf, class_idx, class_table, idx_unseen, unseen_key_labels, query_labels, levels=None):
        class_table = Labels.of(class_table, conf.device)
        if conf.dim() != 2 or conf.shape[1] > class_table.ids.shape[0]:
            raise ValueError("conf must be [Q, k] with k <= the C rows of the class table")
        super().__init__(conf.contiguous(), class_idx.contiguous(), class_table, idx_unseen, unseen_key_labels, query_labels, levels=levels)

    @classmethod
    def from_classifier(cls, conf, class_idx, class_table, unseen_index, unseen_key_labels, query_features, query_labels, levels=None):
        """``conf`` / ``class_idx`` from ``classifier_confidences``; ``query_features`` (numpy or GPU tensor ``[Q, D]``) are the
        ORIGINAL model's image features of the same queries, searched ``k`` deep in the unseen-key ``RetrievalIndex`` (DNA
        features); ``class_table`` / ``unseen_key_labels`` / ``query_labels`` are ``Labels`` or int32 arrays ``[., L]``."""
        query_features = to_gpu(query_features, unseen_index.device)
        if query_features.shape[0] != conf.shape[0]:
            raise ValueError("one row of query features per row of confidences")
        unseen_key_labels = unseen_index.key_labels(unseen_key_labels)
        _, idx_unseen = unseen_index.search(query_features, int(conf.shape[1]))
        return cls(conf, class_idx, class_table, idx_unseen, unseen_key_labels, query_labels, levels=levels)
