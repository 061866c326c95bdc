"""Silhouette scores of the embeddings on the GPU (reference scripts/inference_and_eval.py:403-411): sklearn's
``silhouette_samples(image_features, gt_list)`` with the euclidean metric, once per taxonomic level, and the reference's
``avg_list`` of the result.

    by_level = silhouette_by_level(image_features, label_list)        # {level: {"samples": float64 [N], "mean": float}}

The classes of a level are the distinct label strings (equal strings are one class wherever they sit in the taxonomy).  The samples
are sorted by class id -- a stable argsort and an ``index_select``, plumbing -- so that every class is one contiguous row range;
``bsclip_silhouette_samples`` computes the N^2 distances from differences in f32 and reduces them per (sample, class) in one pass,
and the result is scattered back to the original order.  The mean is formed on the host in float64 as the reference forms it:
``sum(l) * 1.0 / len(l)``, a left-to-right Python sum over the samples in their original order.  There is no CPU path: without the
HIP library or a GPU these functions raise.
"""
import numpy as np
import torch

from . import ops
from .retrieval import LEVELS


def class_segments(ids):
    """``(perm, seg_start)`` for a 1-D integer id sequence (numpy, list or tensor): ``perm`` int64 [N] is the stable argsort of the
    ids (within a class the original order is kept), ``seg_start`` int32 [C + 1] the row ranges of the C distinct ids in the sorted
    order, ``seg_start[0] == 0`` and ``seg_start[-1] == N``.  Ids need not be dense.  Both on the device of ``ids``."""
    ids = torch.as_tensor(ids)
    if ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64) or ids.numel() == 0:
        raise ValueError("class_segments: a non-empty 1-D sequence of integer ids")
    perm = torch.argsort(ids, stable=True)
    _, counts = torch.unique_consecutive(ids[perm], return_counts=True)
    seg_start = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=ids.device)
    seg_start[1:] = torch.cumsum(counts, 0)
    return perm, seg_start


def dense_ids(labels):
    """int32 ids of any sequence of hashable labels, handed out in order of first appearance (as ``retrieval.encode_labels``
    does per level), and the number of classes."""
    table = {}
    ids = np.asarray([table.setdefault(lab, len(table)) for lab in labels], dtype=np.int32)
    return ids, len(table)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("the silhouette score needs a ROCm GPU: the distances and their reduction run in libbsclip_hip.so")
    return torch.device("cuda", torch.cuda.current_device())


def upload_features(features):
    """The features (numpy array or tensor of any float dtype, [N, D]) as an f32 GPU tensor [N, D rounded up to 4], zero-padded --
    which leaves every distance as it is -- and D."""
    if torch.is_tensor(features) and features.is_cuda:
        dev = features.device
    else:
        dev = _device()
        features = torch.as_tensor(np.ascontiguousarray(features))
    if features.dim() != 2 or not features.dtype.is_floating_point or features.shape[1] < 1:
        raise ValueError("silhouette: features must be a float array [N, D] with D >= 1")
    N, D = features.shape
    x = torch.zeros(N, (D + 3) // 4 * 4, dtype=torch.float32, device=dev)
    x[:, :D] = features.to(dev).to(torch.float32)
    return x, D


def _check_class_count(C, N):
    if not 1 < C < N:  # sklearn's check_number_of_labels and its message
        raise ValueError(f"Number of labels is {C}. Valid values are 2 to n_samples - 1 (inclusive)")


def _samples(x, D, labels):
    """One level on uploaded features: float64 numpy [N] in the original order."""
    N = x.shape[0]
    if len(labels) != N:
        raise ValueError(f"{len(labels)} labels for {N} samples")
    ids, C = dense_ids(labels)
    _check_class_count(C, N)
    perm, seg_start = class_segments(torch.from_numpy(ids).to(x.device))
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    out_sorted = ops.silhouette_samples(x.index_select(0, perm), seg_start, D, flag=flag)
    buf = torch.empty(N + 1, dtype=torch.int32, device=x.device)   # [samples (f32 bits) | flag]: one download per level
    buf[:N].view(torch.float32).index_copy_(0, perm, out_sorted)
    buf[N:].copy_(flag)
    host = buf.cpu().numpy()
    ops.check_silhouette_flag(int(host[N]))
    return host[:N].view(np.float32).astype(np.float64)


def avg_list(samples):
    """The reference's ``sum(l) * 1.0 / len(l)`` on float64 values: Python's left-to-right sum."""
    values = np.asarray(samples, dtype=np.float64).tolist()
    return sum(values) * 1.0 / len(values)


def silhouette_samples(features, labels):
    """sklearn's ``silhouette_samples(features, labels)`` (euclidean) on the GPU: float64 numpy [N], original order.  ``features``:
    numpy array or GPU tensor [N, D] of any float dtype, converted to f32 once; ``labels``: any sequence of N hashable values.
    Fewer than 2 or more than N - 1 distinct labels, and non-finite features, raise ``ValueError`` as sklearn does."""
    x, D = upload_features(features)
    return _samples(x, D, list(labels))


def silhouette_by_level(features, label_list, levels=LEVELS):
    """``{level: {"samples": float64 [N], "mean": float}}`` for ``label_list`` = N dicts ``{level: name}``: the features are
    uploaded once, every level is one launch.  A level with fewer than 2 or more than N - 1 classes raises as sklearn does."""
    x, D = upload_features(features)
    out = {}
    for level in levels:
        samples = _samples(x, D, [lab[level] for lab in label_list])
        out[level] = {"samples": samples, "mean": avg_list(samples)}
    return out
