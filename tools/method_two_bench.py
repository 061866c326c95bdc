"""Times the method-two evaluation (scripts/method_two_fine_tuning_and_eval.py) from confidences and features on -- the DNA search of
both splits, the threshold search over ``np.linspace(0, 1, 1001)``, the accuracy tables and the membership check -- on the host path
and on the GPU path, and ``bsclip_class_softmax_topk`` alone on a logits block.

    python tools/method_two_bench.py [--keys 21118] [--queries 2048] [--gpu-queries 16384] [--classes 916] [--repeats 2] [--out profiles/method_two_bench.json]

Two query splits (seen and unseen species) of ``--queries`` image queries each: random classifier logits over ``--classes`` seen
species with the query's own class favoured (seen split only), and random image features with planted neighbours among ``--keys``
unseen keys (DNA features).  Both paths start from the same GPU logits and numpy features: the host path downloads the confidences
(``.tolist()``), looks the label lists up and rebuilds every merged list for every threshold in Python; the GPU path keeps everything
on the GPU.  The host path's cost is linear in the queries, so the two are compared at 2 x ``--queries`` and the GPU path alone is
timed at 2 x ``--gpu-queries`` as well.  Host clock around the whole call (each ends in a download), runs alternated after one
untimed GPU-path run; the outputs are compared for equality before anything is reported.  Appends one JSON line to ``--out`` and
prints it.  A tool, not a gate: no test asserts a time.
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

import method_two_fine_tuning_and_eval as M  # noqa: E402
from bioscanclip.hip import ops  # noqa: E402
from eval_bench_common import append_line, compare_and_time, label  # noqa: E402


def make_sets(rng, n_keys, n_queries, n_classes, n_unseen, dim):
    """(idx_to_all_labels, unseen keys, their labels, per split (logits GPU [Q, C], image features, gt labels))"""
    idx_to_all_labels = {c: label(c) for c in range(n_classes)}
    centres = {m: rng.standard_normal((n_unseen, dim)) for m in ("image", "dna")}
    unseen_sp = rng.integers(0, n_unseen, n_keys)
    unseen_keys = centres["dna"][unseen_sp] + rng.standard_normal((n_keys, dim))
    unseen_key_labels = [label(n_classes + s) for s in unseen_sp.tolist()]
    splits = []
    for seen in (True, False):
        sp = rng.integers(0, n_classes if seen else n_unseen, n_queries)
        logits = rng.standard_normal((n_queries, n_classes)).astype(np.float32) * np.float32(2.0)
        if seen:
            logits[np.arange(n_queries), sp] += (6.0 * rng.random(n_queries)).astype(np.float32)
            feats = rng.standard_normal((n_queries, dim))
        else:
            feats = centres["image"][sp] + 0.6 * centres["dna"][sp] + rng.standard_normal((n_queries, dim))
        gt = [label(s if seen else n_classes + s) for s in sp.tolist()]
        buf = torch.zeros(n_queries, (n_classes + 127) // 128 * 128, dtype=torch.float32, device="cuda")   # the head's padded layout
        buf[:, :n_classes] = torch.from_numpy(logits).cuda()
        splits.append((buf[:, :n_classes], feats, gt))
    return idx_to_all_labels, unseen_keys, unseen_key_labels, splits


def confidences(splits, C):
    return [ops.class_softmax_topk(logits, C, M.MAX_K) + (gt,) for logits, _, gt in splits]


def host_path(args, sets, species_list):
    idx_to_all_labels, unseen_keys, unseen_key_labels, splits = sets
    inputs = []
    for (conf, idx, gt), (_, feats, _) in zip(confidences(splits, len(idx_to_all_labels)), splits):
        pred_a = [{lv: [idx_to_all_labels[i][lv] for i in row] for lv in M.LEVELS} for row in idx.tolist()]
        inputs.append((pred_a, conf.tolist(), M.make_prediction(feats, unseen_keys, unseen_key_labels, max_k=M.MAX_K), gt))
    outs = M.score_predictions_on_host(args, *inputs)
    return outs, [M.check_for_acc_about_correct_predict_seen_or_unseen(o["final_pred_labels"], species_list) for o in outs]


def gpu_path(args, sets, species_list):
    idx_to_all_labels, unseen_keys, unseen_key_labels, splits = sets
    outs = M.score_confidences_on_gpu(args, confidences(splits, len(idx_to_all_labels)), idx_to_all_labels, unseen_keys, unseen_key_labels,
                                      [feats for _, feats, _ in splits])
    return outs, [M.check_for_acc_about_correct_predict_seen_or_unseen(o["merged"], species_list) for o in outs]


def kernel_us(logits, C, k, iters=200):
    """Mean time of one ``class_softmax_topk`` launch on ``logits``, by events around ``iters`` back-to-back launches."""
    for _ in range(10):
        ops.class_softmax_topk(logits, C, k)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        ops.class_softmax_topk(logits, C, k)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=21118)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--gpu-queries", type=int, default=16384)
    ap.add_argument("--classes", type=int, default=916)
    ap.add_argument("--unseen-species", type=int, default=2089)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "method_two_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("method_two_bench needs a ROCm GPU: a time taken elsewhere says nothing about the evaluation")
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=[1, 3, 5]))
    rng = np.random.default_rng(0)
    sets = make_sets(rng, a.keys, a.queries, a.classes, a.unseen_species, a.dim)
    species_list = sorted({lab["species"] for lab in sets[2]})
    big = make_sets(rng, a.keys, a.gpu_queries, a.classes, a.unseen_species, a.dim)
    times = compare_and_time(host_path, gpu_path, (args, sets, species_list), (args, big, sorted({lab["species"] for lab in big[2]})),
                                a.repeats)
    line = {"metric": "method_two_eval_seconds", **times, "queries_per_split": a.queries, "gpu_large_queries_per_split": a.gpu_queries,
            "softmax_topk_us": kernel_us(big[3][0][0], a.classes, M.MAX_K), "softmax_topk_rows": a.gpu_queries,
            "keys_per_index": a.keys, "classes": a.classes, "unseen_species": a.unseen_species, "dim": a.dim, "thresholds": 1001,
            "clock": "host perf_counter around the whole evaluation from logits and features on, device synchronised; best of the runs "
                     "listed; the host path is timed at queries_per_split only (its cost is linear in the queries); softmax_topk_us: "
                     "events around 200 back-to-back launches on softmax_topk_rows x classes logits, k = 5"}
    append_line(a.out, line)


if __name__ == "__main__":
    main()
