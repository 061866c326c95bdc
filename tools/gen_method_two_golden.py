"""Pins the method-two evaluation: writes ``tests/golden/method_two.json`` by running the IMPORTED REFERENCE's own functions
(``scripts/method_two_fine_tuning_and_eval.py``: ``load_all_seen_species_name_and_create_label_map``,
``inference_with_fine_tuned_image_encoder``, ``search_threshold_with_harmonic_mean``, ``get_final_pred_and_acc``,
``check_for_acc_about_correct_predict_seen_or_unseen``, ``print_acc_for_google_doc``) on small seeded inputs.

    python tools/gen_method_two_golden.py --reference <checkout of the reference>

Runs only where the reference checkout exists, never on the GPU box; ``oracle/`` is left as it is and this tool imports the reference
the way ``tools/gen_method_one_golden.py`` does (its ``import_reference``, pointed at the other script).

The fixture holds data only.  The seen-label input is a list of collated label batches (a train-seen loader's labels) and the
reference's ``label_to_index_dict`` / ``idx_to_all_labels`` made of it.  Two splits ("seen" and "unseen" queries) of 40 queries,
k = 5: the classifier's predicted class indices, the label lists the reference derives from them through ``idx_to_all_labels``, the
confidences, the DNA-search predicted label lists, the ground truth; a species list.  The reference's outputs: the best threshold
over 1 000 intervals (1 001 thresholds), micro / macro / per-class accuracy and the merged predictions at that threshold, the lines
of the membership check and of ``print_acc_for_google_doc``.

The confidences come out of the reference's own ``F.softmax`` + ``torch.topk`` + ``.tolist()`` (:57-64), applied to seeded f32
logits handed to it as the "images" of a loader whose "classifier" is the identity: float32 values, rows descending, each row
summing to at most 1.  Planted rows give 1.0 / 0.0 (one finite logit), 0.5 twice (two equal finite logits) -- 0.0, 0.5 and 1.0 lie on
``np.linspace(0, 1, 1001)`` exactly, where the comparison is strict -- and a row of equal values (all logits equal: 1 / C each).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LEVELS = ["order", "family", "genus", "species"]
Q, K_DEPTH, K_LIST, BATCH = 40, 5, [1, 3, 5], 20
SEEN = ["s10", "s2", "s1", "s33", "s4", "s0", "s7"]        # sorted() is not their order of appearance ("s10" < "s2")
UNSEEN = ["u0", "u1", "u2", "u3"]


class passthrough:
    """tqdm stand-in: iterates what it is given, accepts ``total=`` and ``set_description``."""

    def __init__(self, it=(), **kw):
        self.it = it

    def __iter__(self):
        return iter(self.it)

    def set_description(self, *a, **kw):
        pass


def label(species):
    """One taxonomy for seen and unseen species: the higher levels are shared, so a wrong species can be right at its genus."""
    n = int(species[1:])
    return {"order": f"o{n % 2}", "family": f"f{n % 3}", "genus": f"g{n % 4}", "species": species}


def collate(labels):
    return {lv: [lab[lv] for lab in labels] for lv in LEVELS}


def loader_of(logits, gt):
    """Batches in the reference's 7-tuple layout whose "image" is the logits block (the classifier under test is the identity)."""
    import torch
    return [([f"q{i}" for i in range(a, a + BATCH)], torch.from_numpy(logits[a:a + BATCH]), None, None, None, None, collate(gt[a:a + BATCH]))
            for a in range(0, Q, BATCH)]


def search_predictions(rng, gt, p_right):
    """The DNA search against unseen keys: every slot is an unseen species' label; it is the query's own with probability ``p_right``
    (never for a seen query)."""
    out = []
    for g in gt:
        slots = [label(g["species"] if g["species"] in UNSEEN and rng.random() < p_right else UNSEEN[int(rng.integers(len(UNSEEN)))])
                 for _ in range(K_DEPTH)]
        out.append({lv: [s[lv] for s in slots] for lv in LEVELS})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "method_two.json"))
    a = ap.parse_args()
    import gen_method_one_golden as g1
    import importlib.util
    g1.import_reference(a.reference)                               # the stubs, sys.path, and the neighbour script
    spec = importlib.util.spec_from_file_location("ref_method_two", os.path.join(a.reference, "scripts", "method_two_fine_tuning_and_eval.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    ref.tqdm = passthrough
    import torch

    rng = np.random.default_rng(23)
    # the seen-label input: three collated batches, every seen species at least once, in no particular order
    draws = [SEEN[i] for i in rng.permutation(len(SEEN))] + [SEEN[int(i)] for i in rng.integers(len(SEEN), size=11)]
    seen_label_batches = [collate([label(s) for s in draws[i:i + 6]]) for i in range(0, len(draws), 6)]
    label_to_index_dict, idx_to_all_labels = ref.load_all_seen_species_name_and_create_label_map(
        [(None, None, None, None, None, None, b) for b in seen_label_batches])
    C = len(label_to_index_dict)
    assert C == len(SEEN) and list(label_to_index_dict) == sorted(SEEN)

    splits = {}
    for name, pool, peak, p_search in (("seen", SEEN, 3.0, 0.0), ("unseen", UNSEEN, 0.8, 0.65)):
        gt = [label(pool[int(i)]) for i in rng.integers(len(pool), size=Q)]
        logits = rng.standard_normal((Q, C)).astype(np.float32) * np.float32(1.2)
        for q, g in enumerate(gt):                                # a seen query's own class is favoured; an unseen query has none
            col = label_to_index_dict.get(g["species"], int(rng.integers(C)))
            logits[q, col] += np.float32(peak * rng.random())
        ninf = np.float32(-np.inf)
        logits[0] = ninf; logits[0, 3] = 0.0                       # confidences 1.0, 0.0, 0.0, 0.0, 0.0
        logits[1] = ninf; logits[1, [1, 5]] = 2.0                  # 0.5, 0.5, 0.0, 0.0, 0.0
        logits[2] = 0.25                                           # all equal: 1 / C five times
        conf, pred_a, gt_out = ref.inference_with_fine_tuned_image_encoder(lambda x: x, loader_of(logits, gt), label_to_index_dict,
                                                                           idx_to_all_labels, "cpu")
        idx = torch.topk(torch.softmax(torch.from_numpy(logits), dim=-1), k=K_DEPTH, dim=1, largest=True, sorted=True).indices.tolist()
        assert pred_a == [{lv: [idx_to_all_labels[i][lv] for i in row] for lv in idx_to_all_labels[0]} for row in idx]
        assert gt_out == gt
        splits[name] = {"class_indices": idx, "pred_labels_from_a": pred_a, "pred_confidence_from_a": conf,
                        "pred_labels_from_b": search_predictions(rng, gt, p_search), "gt_labels": gt}

    grid = np.linspace(0, 1, 1001).tolist()
    flat = [v for sp in splits.values() for row in sp["pred_confidence_from_a"] for v in row]
    assert all(float(np.float32(v)) == v for v in flat) and {0.0, 0.5, 1.0} <= set(flat) and {0.0, 0.5, 1.0} <= set(grid)
    for sp in splits.values():
        for row in sp["pred_confidence_from_a"]:
            assert row == sorted(row, reverse=True) and sum(row) <= 1.0, row
    assert any(len(set(row)) == 1 for sp in splits.values() for row in sp["pred_confidence_from_a"])

    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=K_LIST))
    data = list(splits.values())
    best = ref.search_threshold_with_harmonic_mean(args, data, num_intervals=1000)
    assert 0.0 < float(best) < 1.0, f"best threshold {best} is not strictly inside (0, 1): choose other seeds"
    species_list = ["s2", "s33", "u1"]
    out = {"k_list": K_LIST, "num_intervals": 1000, "best_threshold": float(best), "species_list": species_list,
           "seen_label_batches": seen_label_batches, "label_to_index_dict": label_to_index_dict,
           "idx_to_all_labels": {str(k): v for k, v in idx_to_all_labels.items()}, "splits": {}}
    results = []
    for name, sp in splits.items():
        res = ref.get_final_pred_and_acc(args, sp["pred_labels_from_a"], sp["pred_confidence_from_a"], sp["pred_labels_from_b"],
                                         sp["gt_labels"], best_threshold=best)
        results.append(res)
        sink = io.StringIO()
        with contextlib.redirect_stdout(sink):
            ref.check_for_acc_about_correct_predict_seen_or_unseen(res["final_pred_labels"], species_list)
        out["splits"][name] = dict(sp, micro_acc={str(k): v for k, v in res["micro_acc"].items()},
                                   macro_acc={str(k): v for k, v in res["macro_acc"].items()},
                                   per_class_acc={str(k): v for k, v in res["per_class_acc"].items()},
                                   final_pred_labels=res["final_pred_labels"], membership_lines=sink.getvalue().splitlines())
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        ref.print_acc_for_google_doc(results[0], results[1], K_LIST=K_LIST)
    out["google_doc_lines"] = sink.getvalue().splitlines()
    out["_meta"] = {"numpy": np.__version__, "torch": torch.__version__, "reference": "bioscan-ml/bioscan-clip @ 2024-10-24",
                    "functions": "scripts/method_two_fine_tuning_and_eval.py: load_all_seen_species_name_and_create_label_map, "
                                 "inference_with_fine_tuned_image_encoder, search_threshold_with_harmonic_mean, get_final_pred_and_acc, "
                                 "check_for_acc_about_correct_predict_seen_or_unseen, print_acc_for_google_doc"}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("wrote", a.out, os.path.getsize(a.out), "bytes; best threshold", float(best),
          "top-1 species", {n: out["splits"][n]["micro_acc"]["1"]["species"] for n in out["splits"]})


if __name__ == "__main__":
    main()
