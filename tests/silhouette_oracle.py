"""The silhouette tests' own oracle and the baseline their tolerance comes from.

``silhouette_f64``: sklearn's ``silhouette_samples`` (euclidean) restated in numpy float64 with the distances from differences,
formed in row chunks (no [N, N, D] array).  ``silhouette_f32_baseline``: the same formula in float32 on the CPU --
``torch.cdist(..., compute_mode="donot_use_mm_for_euclid_dist")``, float32 sums -- i.e. what a straightforward f32 implementation
of the difference form gives.  ``gate``: the GPU tolerance of one case, 4 x the baseline's worst |s - s_f64| on that case's inputs,
never less than 16 x 2^-24 (the factor and the floor of tests/test_59_method_two_gpu.py).
"""
import numpy as np
import torch

FLOOR = 16 * 2.0 ** -24
CHUNK_ELEMENTS = 1 << 23          # at most this many float64 differences at a time


def dense_ids(labels):
    """int64 ids in order of first appearance and the class count, for any sequence of hashable labels."""
    table = {}
    return np.asarray([table.setdefault(lab, len(table)) for lab in labels], dtype=np.int64), len(table)


def _scores(sums, counts, ids, xp):
    """s from the per-(sample, class) distance sums [N, C], in the dtype of ``sums``."""
    N = len(ids)
    rows = xp.arange(N)
    own_n = counts[ids]
    a = sums[rows, ids] / (own_n - 1)                       # 0 / 0 for a singleton: replaced below
    means = sums / counts[None, :]
    means[rows, ids] = xp.inf
    b = means.min(1) if xp is np else means.min(1).values
    s = (b - a) / (xp.maximum(a, b))
    s = xp.nan_to_num(s, nan=0.0)
    s[own_n == 1] = 0.0
    return s


def silhouette_f64(features, labels):
    """float64 [N]: the silhouette coefficient of every sample, sklearn's definition, distances from differences in float64."""
    x = np.asarray(features, dtype=np.float64)
    ids, C = dense_ids(labels)
    N, D = x.shape
    if not 1 < C < N:
        raise ValueError(f"Number of labels is {C}. Valid values are 2 to n_samples - 1 (inclusive)")
    onehot = np.zeros((N, C))
    onehot[np.arange(N), ids] = 1.0
    sums = np.empty((N, C))
    step = max(1, CHUNK_ELEMENTS // (N * D))
    for r0 in range(0, N, step):
        diff = x[r0:r0 + step, None, :] - x[None, :, :]
        dist = np.sqrt(np.einsum("rnd,rnd->rn", diff, diff))   # d(i, i) is exactly 0: every difference is
        sums[r0:r0 + step] = dist @ onehot
    with np.errstate(divide="ignore", invalid="ignore"):
        return _scores(sums, onehot.sum(0), ids, np)


def silhouette_f32_baseline(features, labels):
    """float64 view of the float32 result of the same formula: torch CPU ``cdist`` without the matrix-multiply form, f32 sums."""
    x = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32))
    ids, C = dense_ids(labels)
    N = x.shape[0]
    dist = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist")
    onehot = torch.zeros(N, C, dtype=torch.float32)
    onehot[torch.arange(N), torch.from_numpy(ids)] = 1.0
    s = _scores(dist @ onehot, onehot.sum(0), torch.from_numpy(ids), torch)
    return s.numpy().astype(np.float64)


def gate(features, labels, want=None):
    """(tolerance, the baseline's worst error) for one case; ``want`` = ``silhouette_f64`` of the same inputs if already computed."""
    want = silhouette_f64(features, labels) if want is None else want
    err = float(np.max(np.abs(silhouette_f32_baseline(features, labels) - want)))
    return max(4 * err, FLOOR), err


def avg_list(values):
    """The reference's ``sum(l) * 1.0 / len(l)``: Python's left-to-right float sum."""
    values = np.asarray(values, dtype=np.float64).tolist()
    return sum(values) * 1.0 / len(values)
