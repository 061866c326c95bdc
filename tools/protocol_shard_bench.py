"""Times the seen / unseen protocols and a fine-tuning epoch fed from a protocol root of shards, in one process.

    python tools/protocol_shard_bench.py [--keys 4096] [--queries 2048] [--train 2048] [--species 500] [--image-size 256]
                                         [--rounds 2] [--out profiles/protocol_shard_bench.json]

The tool writes its own protocol root into a temporary directory (removed at the end): raw shards of random pictures of
``--image-size`` squared and random barcodes of 600-720 bases; ``--keys`` samples per key split, ``--queries`` per query split (two per
part), ``--train`` in ``train_seen``; ``--species`` species, the last fifth of them unseen.  The model is the full-depth image + DNA
configuration with its initial weights.  Two things are measured, each with one untimed run of either side and then ``--rounds`` timed
runs that alternate:

  (a) method one and method two, val and test parts, with ``hip_eval=gpu`` scoring on both sides: the resident path
      (``method_1_from_shards`` / ``method_2_from_shards``: one walk per split with the one tower it needs, key indices appended as the
      batches arrive, nothing downloaded) against the loader-walk path (``method_1_inference_and_eval_for_seen_and_unseen`` /
      ``method_2_inference_and_eval_for_seen_and_unseen`` on ``ShardLoader(for_training=False)`` loaders: one walk per split and use,
      float64 features down and f32 features up, label dictionaries).  The tables of every run are compared for equality before
      anything is reported.
  (b) one epoch of ``fine_tuning_epoch_image_and_dna`` over ``train_seen`` at batch 64: targets from the resident class-index column
      against ``label_batch_to_species_idx`` (``list.index`` per sample) on the loader's label dictionaries, for class lists of
      C = ``--species`` and C = 8 000 names: ``train_seen``'s species at the end, names that never occur in front of them, so that
      every look-up scans past those.  The weights move from run to run, which the time does not depend on; that both kinds of
      target give the same losses and parameters is what tests/test_69_protocol_shards_gpu.py checks.

Host clock around each whole call from the construction of its loaders on, device synchronised.  Appends one JSON line to ``--out``
and prints it.  A tool, not a gate: no test asserts a time.
"""
import argparse
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import method_one_eval as M1  # noqa: E402
import method_two_fine_tuning_and_eval as M2  # noqa: E402
from bioscanclip.epoch import fine_tuning_epoch as fte  # noqa: E402
from bioscanclip.hip.optim import FusedAdamW  # noqa: E402
from bioscanclip.hip.protocols import ProtocolRoot  # noqa: E402
from bioscanclip.util import shards  # noqa: E402
from bioscanclip.util.util import EncoderWithExtraLayer  # noqa: E402
from eval_bench_common import TABLE_KEYS, append_line, label, timed  # noqa: E402

EVAL_BATCH, TRAIN_BATCH, CHUNK, PADDED_C = 40, 64, 512, 8000


def write_split(path, rng, n, species, size):
    """One raw shard of ``n`` samples whose species are drawn from ``species``; pictures are generated ``CHUNK`` at a time."""
    def pictures():
        for i0 in range(0, n, CHUNK):
            yield from rng.integers(0, 256, (min(CHUNK, n - i0), size, size, 3), dtype=np.uint8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    barcodes = [bases[rng.integers(0, 4, int(m))].tobytes() for m in rng.integers(600, 721, n)]
    labels = [label(int(s)) for s in rng.choice(species, n)]
    zeros = np.zeros((n, 4), np.int64)
    shards.write_shard(path, pictures(), barcodes, zeros, zeros, zeros, [f"P{i:07d}" for i in range(n)],
                       taxonomy={lv: [lab[lv] for lab in labels] for lv in shards.LEVELS}, split=os.path.basename(path))


class Collated:
    """Slot 6 of a ``ShardLoader(for_training=False)`` batch as ``{level: [names]}``: what ``label_batch_to_species_idx`` indexes."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield (*batch[:6], {lv: [d[lv] for d in batch[6]] for lv in shards.LEVELS})


def note(*what):
    """Progress on stderr: the runs are long and the JSON line comes last."""
    print(*what, file=sys.stderr, flush=True)


def _args(mc):
    return types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=[1, 3, 5]), hip_eval="gpu", activate_wandb=False,
                                 model_config=mc)


def proto_of(root, device):
    return ProtocolRoot(root, shards.PROTOCOL_SPLITS, batch_size=EVAL_BATCH, device=device)


def resident(root, args, model, classifier, device):
    proto = proto_of(root, device)
    label_map, rows, class_table = proto.sorted_class_list("train_seen")
    return (M1.method_1_from_shards(args, model, proto, device),
            M2.method_2_from_shards(args, classifier, model, proto, label_map, rows, class_table, device))


def loader_walk(root, args, model, classifier, device):
    proto = proto_of(root, device)
    label_map, rows, _ = proto.sorted_class_list("train_seen")
    ld = lambda name: proto.loader(name, labels=None)
    one, two, t1, t2 = {}, {}, None, None
    for part, seen, unseen in M1.PARTS:
        one[part] = M1.method_1_inference_and_eval_for_seen_and_unseen(args, model, ld(seen), ld(unseen), ld("seen_keys"), ld("val_unseen_keys"),
                                                                       ld("test_unseen_keys"), device, searched_threshold=t1)
        two[part] = M2.method_2_inference_and_eval_for_seen_and_unseen(args, classifier, model, ld(seen), ld(unseen), ld("val_unseen_keys"),
                                                                       ld("test_unseen_keys"), label_map, rows, device, searched_threshold=t2)
        t1, t2 = one[part][0]["best_threshold"], two[part][0]["best_threshold"]
    return one, two


def same_tables(a, b):
    return all(x[k] == y[k] for ra, rb in zip(a, b) for part in ("val", "test") for x, y in zip(ra[part], rb[part])
               for k in TABLE_KEYS + ("best_threshold",))


def epoch(root, classes, pair, optimizer, device, resident_targets):
    proto = ProtocolRoot(root, ("train_seen",), batch_size=TRAIN_BATCH, device=device)
    train = proto.loader("train_seen", labels="ids" if resident_targets else None, shuffle=True)
    targets_of = proto.targets(classes, "train_seen") if resident_targets else None
    return fte.fine_tuning_epoch_image_and_dna(types.SimpleNamespace(activate_wandb=False), *pair, train if resident_targets else Collated(train),
                                               optimizer, nn.CrossEntropyLoss(), classes, 0, device, targets_of=targets_of)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--train", type=int, default=2048)
    ap.add_argument("--species", type=int, default=500)
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "protocol_shard_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("protocol_shard_bench needs a ROCm GPU: a time taken elsewhere says nothing about the protocols")
    from bioscanclip.model.simple_clip import load_clip_model
    from bioscanclip.util.config import load_config
    device = torch.device("cuda", 0)
    cfg = load_config(os.path.join(ROOT, "bioscan-clip_amd", "bioscanclip", "config"), ["model_config=lora_vit_lora_barcode_bert_ssl"])
    torch.manual_seed(0)
    model = load_clip_model(cfg, device).to(device).eval()
    tuned = load_clip_model(cfg, device).to(device)
    tuned.load_state_dict(model.state_dict())
    rng = np.random.default_rng(0)
    n_unseen = max(a.species // 5, 1)
    seen_species, unseen_species = np.arange(0, a.species - n_unseen), np.arange(a.species - n_unseen, a.species)
    args = _args(cfg.model_config)
    root = tempfile.mkdtemp(prefix="bsclip_protocol_root_")
    try:
        sizes = {"train_seen": a.train, "seen_keys": a.keys, "val_unseen_keys": a.keys, "test_unseen_keys": a.keys}
        for name in shards.PROTOCOL_SPLITS:
            species = unseen_species if "unseen" in name else seen_species
            write_split(os.path.join(root, name), rng, sizes.get(name, a.queries), species, a.image_size)
        proto = proto_of(root, device)
        C = len(proto.sorted_class_list("train_seen")[0])
        classifier = M2.ViTWIthExtraLayer(tuned.image_encoder, nn.Linear(int(getattr(cfg.model_config, "output_dim", 768)), C)).to(device).eval()
        note("root written")
        ref = timed(loader_walk, root, args, model, classifier, device)[1]      # untimed: code objects, allocator, page cache
        timed(resident, root, args, model, classifier, device)
        res_s, walk_s, equal = [], [], True
        for _ in range(a.rounds):
            tw, out_w, _ = timed(loader_walk, root, args, model, classifier, device)
            tr, out_r, _ = timed(resident, root, args, model, classifier, device)
            equal &= same_tables(out_r, out_w) and same_tables(out_w, ref)
            walk_s.append(tw)
            res_s.append(tr)
            note(f"protocols: loader walk {tw:.2f} s, resident {tr:.2f} s")
        if not equal:
            raise RuntimeError("the resident tables differ from the loader-walk tables: nothing to time")

        seen_classes = proto.first_appearance_classes("train_seen")
        epochs = {}
        for C_list in (a.species, PADDED_C):
            classes = [f"absent-{i}" for i in range(C_list - len(seen_classes))] + seen_classes
            tuned = load_clip_model(cfg, device).to(device)                   # an encoder pair and an optimizer of its own per class list
            pair = (EncoderWithExtraLayer(tuned.image_encoder, nn.Linear(768, C_list)).to(device),
                    EncoderWithExtraLayer(tuned.dna_encoder, nn.Linear(768, C_list)).to(device))
            optimizer = FusedAdamW([p for m in pair for p in m.parameters() if p.requires_grad], lr=1e-3)
            timed(epoch, root, classes, pair, optimizer, device, False)
            timed(epoch, root, classes, pair, optimizer, device, True)
            index_s, column_s = [], []
            for _ in range(a.rounds):
                index_s.append(timed(epoch, root, classes, pair, optimizer, device, False)[0])
                column_s.append(timed(epoch, root, classes, pair, optimizer, device, True)[0])
                note(f"epoch, C = {C_list}: list.index {index_s[-1]:.2f} s, resident {column_s[-1]:.2f} s")
            epochs[str(C_list)] = {"list_index_s": min(index_s), "resident_s": min(column_s), "list_index_runs_s": index_s,
                                   "resident_runs_s": column_s, "steps": -(-a.train // TRAIN_BATCH)}
    finally:
        shutil.rmtree(root, ignore_errors=True)
    samples = 3 * a.keys + 4 * a.queries
    line = {"metric": "protocol_shard_seconds", "resident_s": min(res_s), "loader_walk_s": min(walk_s),
            "walk_over_resident": min(walk_s) / min(res_s), "resident_runs_s": res_s, "loader_walk_runs_s": walk_s,
            "tables_equal": bool(equal), "protocols": "method one + method two, val and test parts, hip_eval=gpu scoring on both sides",
            "samples_in_the_seven_evaluation_splits": samples, "keys_per_key_split": a.keys, "queries_per_split": a.queries,
            "train_seen": a.train, "species": a.species, "classifier_classes": C, "image_size": a.image_size, "eval_batch": EVAL_BATCH,
            "fine_tuning_epoch": epochs, "train_batch": TRAIN_BATCH,
            "best_threshold": [float(ref[0]["val"][0]["best_threshold"]), float(ref[1]["val"][0]["best_threshold"])],
            "towers": "image+dna, full depth, initial weights", "shards": "raw",
            "clock": "host perf_counter around each whole call (loaders built, splits walked, tables assembled / one epoch), device "
                     "synchronised; one untimed run of either side, then the two alternate; best of the runs listed; loader and model "
                     "alone, nothing else on the GPU"}
    append_line(a.out, line)


if __name__ == "__main__":
    main()
