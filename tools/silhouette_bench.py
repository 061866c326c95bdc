"""Times the silhouette scores on the GPU (``bioscanclip/hip/silhouette.py``, ``bsclip_silhouette_samples``).

    python tools/silhouette_bench.py [--out profiles/silhouette_bench.json] [--n 16384] [--dim 768] [--sklearn-n 4096]

N samples of D features (a centre per species plus noise) with four label levels of about 20 / 500 / 3 000 / 8 000 classes, the
species sizes skewed so that the largest order holds thousands of samples.  Recorded: the host clock around ``silhouette_by_level``
from the numpy features on (upload, sort, four launches, download, the means), device synchronised, for each of ``--runs`` runs after
one untimed run; the time of the launch per level from device events around it (the segment check and the main kernel), the
arithmetic it stands for (3 N^2 D f32 operations: a subtract, a multiply and an add per feature and pair) over that time, and that
rate's share of the f32 vector peak (157.3 TFLOP/s).  Where sklearn imports, its ``silhouette_samples`` is timed once on the first
``--sklearn-n`` samples at the species level, on the host, as measured; it is quadratic in the samples and nothing is extrapolated.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from eval_bench_common import append_line, timed  # noqa: E402

LEVELS = ["order", "family", "genus", "species"]
CLASSES = {"order": 20, "family": 500, "genus": 3000, "species": 8000}
PEAK_F32_VECTOR = 157.3e12


def make_inputs(N, D, seed=0):
    rng = np.random.default_rng(seed)
    S = CLASSES["species"]
    p = 1.0 / (np.arange(S) + 10.0)
    species = np.concatenate([np.arange(S), rng.choice(S, size=N - S, p=p / p.sum())]) if N > S else rng.integers(0, S, size=N)
    species = species[rng.permutation(N)]
    genus = species % CLASSES["genus"]
    family = genus % CLASSES["family"]
    order = np.minimum(family // 8, CLASSES["order"] - 1)                 # the last order takes about two thirds of the samples
    labels = [{"order": f"o{o}", "family": f"f{f}", "genus": f"g{g}", "species": f"s{s}"}
              for o, f, g, s in zip(order.tolist(), family.tolist(), genus.tolist(), species.tolist())]
    centres = rng.standard_normal((S, D)).astype(np.float32)
    x = centres[species] + np.float32(0.5) * rng.standard_normal((N, D)).astype(np.float32)
    return x, labels


def kernel_times(x, labels, repeats):
    """Per level: (milliseconds of one launch from events, best of ``repeats``; classes; the largest class)."""
    from bioscanclip.hip import ops
    from bioscanclip.hip.silhouette import class_segments, dense_ids, upload_features
    xg, D = upload_features(x)
    out = {}
    for lv in LEVELS:
        ids, C = dense_ids([lab[lv] for lab in labels])
        perm, seg = class_segments(torch.from_numpy(ids).to(xg.device))
        xs = xg.index_select(0, perm)
        flag = torch.zeros(1, dtype=torch.int32, device=xg.device)
        ops.silhouette_samples(xs, seg, D, flag=flag)                     # untimed
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.silhouette_samples(xs, seg, D, flag=flag)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ops.check_silhouette_flag(int(flag.item()))
        out[lv] = {"kernel_ms": min(ms), "kernel_runs_ms": ms, "classes": C, "largest_class": int(np.bincount(ids).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_bench.json"))
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--sklearn-n", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("silhouette_bench needs a ROCm GPU: nothing is timed without one")
    from bioscanclip.hip.silhouette import silhouette_by_level
    x, labels = make_inputs(a.n, a.dim)
    timed(silhouette_by_level, x, labels)                                  # untimed: code objects, allocator
    runs, means = [], None
    for _ in range(a.runs):
        t, by_level, _ = timed(silhouette_by_level, x, labels)
        runs.append(t)
        now = {lv: by_level[lv]["mean"] for lv in LEVELS}
        if means is not None and now != means:
            raise RuntimeError("two runs gave different means")
        means = now
    levels = kernel_times(x, labels, a.runs)
    ops_per_level = 3.0 * a.n * a.n * a.dim
    for lv in LEVELS:
        rate = ops_per_level / (levels[lv]["kernel_ms"] * 1e-3)
        levels[lv].update(f32_tflops=rate / 1e12, share_of_f32_vector_peak=rate / PEAK_F32_VECTOR, mean=means[lv])
    line = {"metric": "silhouette_by_level_seconds", "gpu_s": min(runs), "gpu_runs_s": runs, "samples": a.n, "dim": a.dim,
            "levels": levels, "f32_ops_per_level": ops_per_level,
            "clock": "gpu_s: host perf_counter around silhouette_by_level from the numpy features on (upload, sort, one launch per "
                     "level, download, means), device synchronised, best of the runs listed after one untimed run; kernel_ms: device "
                     "events around one bsclip_silhouette_samples launch, best of the runs listed; f32_tflops = 3 N^2 D / kernel time"}
    try:
        from sklearn.metrics import silhouette_samples as sk
        n = min(a.sklearn_n, a.n)
        gt = [lab["species"] for lab in labels[:n]]
        t = time.perf_counter()
        ref = sk(x[:n], gt)
        line.update(sklearn_s=time.perf_counter() - t, sklearn_samples=n, sklearn_level="species", sklearn_classes=len(set(gt)))
        from bioscanclip.hip.silhouette import silhouette_samples
        tg, got, _ = timed(silhouette_samples, x[:n], gt)
        line.update(gpu_same_input_s=tg, max_abs_diff_vs_sklearn_f32=float(np.max(np.abs(got - ref.astype(np.float64)))))
    except ImportError:
        line.update(sklearn_s=None)
    if os.path.exists(a.out):
        os.remove(a.out)
    append_line(a.out, line)


if __name__ == "__main__":
    main()
