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
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import method_one_eval as M  # noqa: E402
from eval_bench_common import append_line, compare_and_time, label  # noqa: E402


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
    big = make_sets(rng, a.keys, a.gpu_queries, a.species, a.dim)
    times = compare_and_time(host_path, gpu_path, (args, sets, species_list), (args, big, sorted({lab["species"] for lab in big[3]})),
                                a.repeats)
    line = {"metric": "method_one_eval_seconds", **times, "queries_per_split": a.queries, "gpu_large_queries_per_split": a.gpu_queries,
            "keys_per_index": a.keys, "dim": a.dim, "species": a.species, "thresholds": 1000,
            "clock": "host perf_counter around the whole evaluation from features on, device synchronised; best of the runs listed; "
                     "the host path is timed at queries_per_split only (its cost is linear in the queries)"}
    append_line(a.out, line)


if __name__ == "__main__":
    main()
