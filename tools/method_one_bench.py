"""Times the whole method-one evaluation (scripts/method_one_eval.py from features on: both searches of both splits, the threshold
search over ``np.linspace(0, 1, 1000)``, the accuracy tables and the membership check) on the host path and on the GPU path.

    python tools/method_one_bench.py [--keys 21118] [--queries 2048] [--gpu-queries 16384] [--repeats 2] [--out profiles/method_one_bench.json]

Two query splits (seen and unseen species) of ``--queries`` image queries each against ``--keys`` seen keys (image features) and as
many unseen keys (DNA features); features are random with planted neighbours, labels a four-level taxonomy.  The host path rebuilds
every merged list for every threshold in Python and its cost is linear in the number of queries, so the two paths are compared at
2 x 2 048 queries by default -- not at the 2 x 16 384 of ``tools/retrieval_eval_bench.py`` -- and the GPU path alone is timed at
2 x ``--gpu-queries`` as well.  Both paths get the same numpy features and are timed with a host clock around the whole call (each
ends in a download); the runs alternate host, GPU after one untimed GPU-path run.  Their outputs are compared for equality before
anything is reported.  Appends one JSON line to ``--out`` and prints it.  A tool, not a gate: no test asserts a time.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import method_one_eval as M  # noqa: E402
from retrieval_eval_bench import tree_hash  # noqa: E402

TABLE_KEYS = ("micro_acc", "macro_acc", "per_class_acc")


def label(s):
    return {"order": f"o{s % 19}", "family": f"f{s % 494}", "genus": f"g{s % 3441}", "species": f"s{s}"}


def make_sets(rng, n_keys, n_queries, n_species, dim):
    centres = {m: rng.standard_normal((n_species, dim)) for m in ("image", "dna")}
    n_seen = n_species * 3 // 4                                   # the unseen queries' species are not among the seen keys
    seen_sp, unseen_sp = rng.integers(0, n_seen, n_keys), rng.integers(n_seen, n_species, n_keys)
    seen_keys = centres["image"][seen_sp] + rng.standard_normal((n_keys, dim))
    unseen_keys = centres["dna"][unseen_sp] + rng.standard_normal((n_keys, dim))
    queries = []
    for lo, hi in ((0, n_seen), (n_seen, n_species)):
        sp = rng.integers(lo, hi, n_queries)
        queries.append((centres["image"][sp] + 0.6 * centres["dna"][sp] + rng.standard_normal((n_queries, dim)),
                        [label(s) for s in sp.tolist()]))
    return seen_keys, [label(s) for s in seen_sp.tolist()], unseen_keys, [label(s) for s in unseen_sp.tolist()], queries


def host_path(args, sets, species_list):
    seen_keys, seen_key_labels, unseen_keys, unseen_key_labels, queries = sets
    inputs = []
    for feats, gt in queries:
        pred_a, sim = M.make_prediction(feats, seen_keys, seen_key_labels, with_similarity=True, max_k=M.MAX_K)
        pred_b = M.make_prediction(feats, unseen_keys, unseen_key_labels, max_k=M.MAX_K)
        inputs.append((pred_a, sim.tolist(), pred_b, gt))
    outs = M.score_predictions_on_host(args, *inputs)
    return outs, [M.check_for_acc_about_correct_predict_seen_or_unseen(o["final_pred_labels"], species_list) for o in outs]


def gpu_path(args, sets, species_list):
    outs = M.score_features_on_gpu(args, *sets)
    return outs, [M.check_for_acc_about_correct_predict_seen_or_unseen(o["merged"], species_list) for o in outs]


def timed(fn, *a):
    sink = io.StringIO()
    torch.cuda.synchronize()
    t = time.perf_counter()
    with contextlib.redirect_stdout(sink):
        outs, shares = fn(*a)
    torch.cuda.synchronize()
    return time.perf_counter() - t, outs, shares


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=21118)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--gpu-queries", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--species", type=int, default=8355)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "method_one_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("method_one_bench needs a ROCm GPU: a time taken elsewhere says nothing about the evaluation")
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=[1, 3, 5]))
    rng = np.random.default_rng(0)
    sets = make_sets(rng, a.keys, a.queries, a.species, a.dim)
    species_list = sorted({lab["species"] for lab in sets[3]})
    timed(gpu_path, args, sets, species_list)                     # untimed: code objects, allocator
    host_s, gpu_s, tables_equal, threshold_equal = [], [], True, True
    for _ in range(a.repeats):
        th, out_h, share_h = timed(host_path, args, sets, species_list)
        tg, out_g, share_g = timed(gpu_path, args, sets, species_list)
        tables_equal &= all(g[k] == h[k] for h, g in zip(out_h, out_g) for k in TABLE_KEYS) and share_h == share_g
        threshold_equal &= all(g["best_threshold"] == h["best_threshold"] for h, g in zip(out_h, out_g))
        host_s.append(th)
        gpu_s.append(tg)
    if not (tables_equal and threshold_equal):
        raise RuntimeError("the GPU path's outputs differ from the host path's: nothing to time")
    big = make_sets(rng, a.keys, a.gpu_queries, a.species, a.dim)
    big_species = sorted({lab["species"] for lab in big[3]})
    timed(gpu_path, args, big, big_species)
    big_s = [timed(gpu_path, args, big, big_species)[0] for _ in range(a.repeats)]
    line = {"metric": "method_one_eval_seconds", "host_s": min(host_s), "gpu_s": min(gpu_s), "host_over_gpu": min(host_s) / min(gpu_s),
            "host_runs_s": host_s, "gpu_runs_s": gpu_s, "queries_per_split": a.queries, "splits": 2,
            "gpu_large_s": min(big_s), "gpu_large_runs_s": big_s, "gpu_large_queries_per_split": a.gpu_queries,
            "keys_per_index": a.keys, "dim": a.dim, "species": a.species, "k_list": [1, 3, 5], "thresholds": 1000,
            "tables_equal": bool(tables_equal), "best_threshold_equal": bool(threshold_equal),
            "best_threshold": float(out_h[0]["best_threshold"]),
            "top1_species": [out_h[0]["micro_acc"][1]["species"], out_h[1]["micro_acc"][1]["species"]],
            "clock": "host perf_counter around the whole evaluation from features on, device synchronised; best of the runs listed; "
                     "the host path is timed at queries_per_split only (its cost is linear in the queries)",
            "tree_hash": tree_hash()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
