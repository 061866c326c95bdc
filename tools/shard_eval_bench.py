"""Times the evaluation of a directory of shard splits: the one-pass resident path (``features.extract_splits`` +
``retrieval.evaluate_resident``) against the three-pass path it stands beside (``get_features_and_label`` per split +
``inference_and_print_result_gpu``) over the same ``ShardLoader``s, in one process.

    python tools/shard_eval_bench.py [--keys 4096] [--queries 2048] [--image-size 256] [--rounds 2] [--out profiles/shard_eval_bench.json]

The tool writes its own evaluation root into a temporary directory (removed at the end): raw shards of random pictures of
``--image-size`` squared, random barcodes of 600-720 bases and random text tokens, ``--keys`` keys and 2 x ``--queries`` queries with a
synthetic taxonomy; the model is the full-depth I+D+T configuration with its initial weights.  Both paths run the same encoder
calls on the same batches of 24, so what differs is the loader work (every split read, copied and transformed once instead of three
times), the feature traffic (device tables instead of float64 arrays down and f32 arrays up) and the label encoding (ids from the
shard's arrays instead of Python dictionaries).  One untimed run of each path, then the two alternate for ``--rounds`` rounds; host
clock around the whole evaluation from the construction of the loaders to the accuracy tables, device synchronised; the tables of
every run are compared for equality before anything is reported.  It is measured with the loader and the model alone: no training
step shares the GPU or the host.  Appends one JSON line to ``--out`` and prints it.  A tool, not a gate: no test asserts a time.
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import inference_and_eval as E  # noqa: E402
from bioscanclip.hip.features import extract_splits  # noqa: E402
from bioscanclip.hip.retrieval import evaluate_resident  # noqa: E402
from bioscanclip.util import shards  # noqa: E402
from eval_bench_common import append_line, label, timed  # noqa: E402

BATCH, TEXT_LEN, CHUNK = 24, 20, 512


def write_split(path, rng, n, species, size):
    """One raw shard of ``n`` samples whose species are drawn from ``species``; pictures are generated ``CHUNK`` at a time."""
    def pictures():
        for i0 in range(0, n, CHUNK):
            yield from rng.integers(0, 256, (min(CHUNK, n - i0), size, size, 3), dtype=np.uint8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    barcodes = [bases[rng.integers(0, 4, int(m))].tobytes() for m in rng.integers(600, 721, n)]
    labels = [label(int(s)) for s in rng.choice(species, n)]
    shards.write_shard(path, pictures(), barcodes, rng.integers(1000, 30000, (n, TEXT_LEN)), np.zeros((n, TEXT_LEN), np.int64),
                       np.ones((n, TEXT_LEN), np.int64), [f"P{i:07d}" for i in range(n)],
                       taxonomy={lv: [lab[lv] for lab in labels] for lv in shards.LEVELS}, split=os.path.basename(path))


def loaders(root):
    return [shards.ShardLoader(p, BATCH, for_training=False, shuffle=False, with_text=True) for p in shards.eval_splits(root)]


def one_pass(root, model, device, k_list):
    return evaluate_resident(*extract_splits(loaders(root), model, device), k_list=k_list)


def three_pass(root, model, device, k_list):
    splits = [E.get_features_and_label(ld, model, device, for_key_set=(i == 0)) for i, ld in enumerate(loaders(root))]
    return E.inference_and_print_result_gpu(*splits, k_list=k_list)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_eval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("shard_eval_bench needs a ROCm GPU: a time taken elsewhere says nothing about the evaluation")
    from bioscanclip.model.simple_clip import load_clip_model
    from bioscanclip.util.config import load_config
    device = torch.device("cuda", 0)
    cfg = load_config(os.path.join(ROOT, "bioscan-clip_amd", "bioscanclip", "config"),
                      ["model_config=lora_vit_lora_barcode_bert_lora_bert_ssl"])
    torch.manual_seed(0)
    model = load_clip_model(cfg, device).to(device).eval()
    rng = np.random.default_rng(0)
    k_list = [1, 3, 5]
    root = tempfile.mkdtemp(prefix="bsclip_eval_root_")
    try:
        seen_species, unseen_species = np.arange(0, 900), np.arange(900, 1100)
        write_split(os.path.join(root, "all_keys"), rng, a.keys, np.arange(0, 1100), a.image_size)
        write_split(os.path.join(root, "val_seen"), rng, a.queries, seen_species, a.image_size)
        write_split(os.path.join(root, "val_unseen"), rng, a.queries, unseen_species, a.image_size)
        ref = timed(three_pass, root, model, device, k_list)[1]            # untimed: code objects, allocator, page cache
        timed(one_pass, root, model, device, k_list)
        one_s, three_s, equal = [], [], True
        for _ in range(a.rounds):
            t3, out3, _ = timed(three_pass, root, model, device, k_list)
            t1, out1, _ = timed(one_pass, root, model, device, k_list)
            equal &= out1[0] == out3[0] == ref[0] and out1[1] == out3[1] == ref[1]
            three_s.append(t3)
            one_s.append(t1)
        if not equal:
            raise RuntimeError("the one-pass tables differ from the three-pass tables: nothing to time")
    finally:
        shutil.rmtree(root, ignore_errors=True)
    samples = a.keys + 2 * a.queries
    line = {"metric": "shard_eval_seconds", "one_pass_s": min(one_s), "three_pass_s": min(three_s),
            "three_over_one": min(three_s) / min(one_s), "one_pass_runs_s": one_s, "three_pass_runs_s": three_s,
            "one_pass_samples_per_s": samples / min(one_s), "three_pass_samples_per_s": samples / min(three_s),
            "tables_equal": bool(equal), "keys": a.keys, "queries_per_split": a.queries, "image_size": a.image_size, "batch": BATCH,
            "towers": "image+dna+text, full depth, initial weights", "shards": "raw", "k_list": k_list,
            "top1_species_image_to_image": [ref[0]["encoded_image_feature"]["encoded_image_feature"][s]["micro_acc"][1]["species"]
                                            for s in ("seen", "unseen")],
            "clock": "host perf_counter around the whole evaluation (loaders built, splits walked, tables assembled), device "
                     "synchronised; one untimed run of each path, then three-pass and one-pass alternate; best of the runs listed; "
                     "loader and model alone, nothing else on the GPU"}
    append_line(a.out, line)


if __name__ == "__main__":
    main()
