"""Times the whole retrieval evaluation (the accuracy table of scripts/inference_and_eval.py) on the host path and on the
GPU-resident path, at BIOSCAN-1M evaluation size: 21 118 keys, 16 384 seen + 16 384 unseen queries, three modalities -- all five
query feature types against all six key types (21 cells that pass the dimension rule, two splits each).

    python tools/retrieval_eval_bench.py [--keys 21118] [--queries 16384] [--repeats 2] [--out profiles/retrieval_eval_bench.json]

Features are random with planted neighbours (a centre per species plus noise), labels a four-level taxonomy with repeated species.
Both paths get the same numpy splits, as ``get_features_and_label`` returns them, and are timed with a host clock around the whole
call (each ends in a download, so the device is idle when the clock stops); the runs alternate host, GPU, host, GPU after one
untimed GPU-path run that loads the code objects both paths share.  The two tables are compared for equality before anything is
reported.  Appends one JSON line (both times, the ratio, the hash of the product sources) to ``--out`` and prints it.  A tool, not
a gate: no test asserts a time.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import inference_and_eval as E  # noqa: E402
from eval_bench_common import append_line, timed  # noqa: E402


def make_split(rng, n, species, centres, noise, for_key_set=False):
    """One split in the layout of ``get_features_and_label``: float64 features, a list of label dicts."""
    labels = [{"order": f"o{s % 19}", "family": f"f{s % 494}", "genus": f"g{s % 3441}", "species": f"s{s}"} for s in species.tolist()]
    feat = {m: centres[m][species] + noise * rng.standard_normal((n, centres[m].shape[1])) for m in ("image", "dna", "lang")}
    split = {"file_name_list": [str(i) for i in range(n)], "label_list": labels, "encoded_image_feature": feat["image"],
             "encoded_dna_feature": feat["dna"], "encoded_language_feature": feat["lang"],
             "averaged_feature": np.mean([feat["image"], feat["dna"]], axis=0),
             "concatenated_feature": np.concatenate((feat["image"], feat["dna"]), axis=1),
             "all_key_features": None, "all_key_features_label": None}
    if for_key_set:
        split["all_key_features"] = np.concatenate((feat["image"], feat["dna"], feat["lang"]), axis=0)
        split["all_key_features_label"] = labels + labels + labels
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=21118)
    ap.add_argument("--queries", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--species", type=int, default=8355)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_eval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("retrieval_eval_bench needs a ROCm GPU: a time taken elsewhere says nothing about the evaluation")
    rng = np.random.default_rng(0)
    k_list = [1, 3, 5]
    n_seen_species = a.species * 3 // 4     # the unseen queries' species are not among the keys
    centres = {m: rng.standard_normal((a.species, a.dim)) for m in ("image", "dna", "lang")}
    splits = (make_split(rng, a.keys, rng.integers(0, n_seen_species, a.keys), centres, 1.0, for_key_set=True),
              make_split(rng, a.queries, rng.integers(0, n_seen_species, a.queries), centres, 1.0),
              make_split(rng, a.queries, rng.integers(n_seen_species, a.species, a.queries), centres, 1.0))
    timed(E.inference_and_print_result_gpu, *splits, k_list=k_list)   # untimed: code objects, allocator
    host_s, gpu_s = [], []
    for _ in range(a.repeats):
        th, (acc_h, pc_h, _), out_h = timed(E.inference_and_print_result, *splits, k_list=k_list)
        tg, (acc_g, pc_g, _), out_g = timed(E.inference_and_print_result_gpu, *splits, k_list=k_list)
        if not (acc_h == acc_g and pc_h == pc_g and out_h == out_g):
            raise RuntimeError("the GPU path's tables differ from the host path's: nothing to time")
        host_s.append(th)
        gpu_s.append(tg)
    cells = sum(bool(acc_h[q][kf]) for q in acc_h for kf in acc_h[q])
    line = {"metric": "retrieval_eval_table_seconds", "host_s": min(host_s), "gpu_s": min(gpu_s), "host_over_gpu": min(host_s) / min(gpu_s),
            "host_runs_s": host_s, "gpu_runs_s": gpu_s, "cells": cells, "keys": a.keys, "queries_per_split": a.queries, "dim": a.dim,
            "species": a.species, "k_list": k_list, "tables_equal": True,
            "top1_species_seen_image_to_dna": acc_h["encoded_image_feature"]["encoded_dna_feature"]["seen"]["micro_acc"][1]["species"],
            "clock": "host perf_counter around the whole call, device synchronised; best of the runs listed"}
    append_line(a.out, line)


if __name__ == "__main__":
    main()
