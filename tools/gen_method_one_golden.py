"""Pins the method-one evaluation: writes ``tests/golden/method_one.json`` by running the IMPORTED REFERENCE's own functions
(``scripts/method_one_eval.py``: ``search_threshold_with_harmonic_mean``, ``get_final_pred_and_acc``,
``check_for_acc_about_correct_predict_seen_or_unseen``) on small seeded inputs.

    python tools/gen_method_one_golden.py [--reference /root/reference]

Runs only where the reference checkout exists, never on the GPU box; ``oracle/gen_golden.py`` is left as it is and this tool
imports the reference the same way: the real ``transformers`` first, packages the reference imports but this path does not need as
``MagicMock``.  Three more stubs are needed for this script: ``bioscanclip.util.dataset`` (the script asks it for a loader that
does not exist), ``hydra.main`` (a decorator that returns the function) and ``tqdm`` (a pass-through with ``set_description``).

The fixture holds data only: two splits ("seen" and "unseen" queries) of 40 queries, k = 5, three classes per level -- the
predicted label lists of both searches, the similarities, the ground truth, a species list -- and the reference's outputs: the best
threshold over 1 000 intervals, micro / macro / per-class accuracy and the merged predictions at that threshold, and the lines
the membership check prints.  The similarities are float32 values (what faiss returns and ``.tolist()`` widens), so the GPU path
can be fed the same numbers; among them are 0.0 and 1.0 (both on ``np.linspace(0, 1, 1000)`` exactly, where the comparison is
strict), values below 0 and above 1, and an unsorted row.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = ["order", "family", "genus", "species"]
Q, K_DEPTH, N_CLASSES, K_LIST = 40, 5, 3, [1, 3, 5]


def import_reference(ref_root):
    sys.dont_write_bytecode = True
    import importlib.machinery
    from transformers import BertConfig, BertForMaskedLM, BertModel  # noqa: F401  (real, and resolved before anything is stubbed)
    for name in ["torchtext", "torchtext.vocab", "timm", "timm.models", "timm.models.vision_transformer", "open_clip", "loratorch",
                 "loratorch.layers", "clip", "faiss", "wandb", "torchvision", "torchvision.transforms", "seaborn", "h5py", "umap",
                 "plotly", "plotly.express", "hydra", "omegaconf", "matplotlib", "matplotlib.pyplot", "PIL", "sklearn.metrics"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = MagicMock(__spec__=importlib.machinery.ModuleSpec(name, None))
    sys.modules["bioscanclip.util.dataset"] = MagicMock()
    sys.modules["hydra"].main = lambda *a, **kw: (lambda fn: fn)

    class passthrough(list):
        def set_description(self, *a, **kw):
            pass

    try:
        import tqdm  # noqa: F401
    except Exception:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
        sys.modules["tqdm"].__spec__ = importlib.machinery.ModuleSpec("tqdm", None)
        sys.modules["tqdm"].tqdm = passthrough
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ref_root, "scripts"))     # the script imports its neighbour inference_and_eval
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_method_one_eval", os.path.join(ref_root, "scripts", "method_one_eval.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    ref.tqdm = passthrough     # no progress bar: the loop only iterates it and calls set_description
    return ref


def label(rng, species=None):
    """A label dict; the levels are drawn independently, so a prediction can be right at one level and wrong at the next."""
    out = {lv: f"{lv[0]}{int(rng.integers(N_CLASSES))}" for lv in LEVELS}
    if species is not None:
        out["species"] = f"s{species}"
    return out


def predictions(rng, gt, p_right):
    """Per query ``{level: [name] * k}``: each slot repeats the query's own label with probability ``p_right``, per level."""
    out = []
    for g in gt:
        slots = [{lv: (g[lv] if rng.random() < p_right else label(rng)[lv]) for lv in LEVELS} for _ in range(K_DEPTH)]
        out.append({lv: [s[lv] for s in slots] for lv in LEVELS})
    return out


def make_split(rng, lo, hi, p_seen_keys, p_unseen_keys):
    gt = [label(rng, species=i % N_CLASSES) for i in range(Q)]
    sim = np.sort(rng.uniform(lo, hi, size=(Q, K_DEPTH)).astype(np.float32), axis=1)[:, ::-1].copy()
    return {"gt_label": gt, "pred_labels_from_search_with_seen_keys": predictions(rng, gt, p_seen_keys),
            "pred_labels_from_search_with_unseen_keys": predictions(rng, gt, p_unseen_keys), "sim": sim}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "method_one.json"))
    a = ap.parse_args()
    ref = import_reference(a.reference)
    rng = np.random.default_rng(17)
    # seen queries: high similarities, the seen-key search mostly right; unseen queries: lower ones, the unseen-key search right
    splits = {"seen": make_split(rng, 0.35, 1.1, 0.7, 0.1), "unseen": make_split(rng, -0.15, 0.75, 0.05, 0.6)}
    s = splits["seen"]["sim"]
    s[0] = [1.0, 1.0, 0.5, 0.0, 0.0]                      # 0.0 and 1.0 lie on the grid: `>` is strict there
    s[1] = [0.4, 0.9, -0.3, 1.2, 0.6]                     # unsorted, below 0 and above 1
    u = splits["unseen"]["sim"]
    u[0] = [1.0, 0.0, 0.0, -0.5, -1.0]
    u[1] = np.float32(500 / 999)                          # next to a grid value, not on it (500 / 999 is no float32)
    args = types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=K_LIST))
    data = [{"pred_labels_from_search_with_seen_keys": sp["pred_labels_from_search_with_seen_keys"],
             "pred_labels_from_search_with_unseen_keys": sp["pred_labels_from_search_with_unseen_keys"],
             "pred_similarity_from_search_with_seen_keys": sp["sim"].tolist(), "gt_label": sp["gt_label"]} for sp in splits.values()]
    best = ref.search_threshold_with_harmonic_mean(args, data, num_intervals=1000)
    species_list = ["s0", "s2"]
    out = {"k_list": K_LIST, "num_intervals": 1000, "best_threshold": float(best), "species_list": species_list, "splits": {}}
    for (name, sp), d in zip(splits.items(), data):
        res = ref.get_final_pred_and_acc(args, d["pred_labels_from_search_with_seen_keys"], d["pred_similarity_from_search_with_seen_keys"],
                                         d["pred_labels_from_search_with_unseen_keys"], d["gt_label"], best_threshold=best)
        sink = io.StringIO()
        with contextlib.redirect_stdout(sink):
            ref.check_for_acc_about_correct_predict_seen_or_unseen(res["final_pred_labels"], species_list)
        out["splits"][name] = {
            "gt_label": d["gt_label"], "pred_labels_from_search_with_seen_keys": d["pred_labels_from_search_with_seen_keys"],
            "pred_labels_from_search_with_unseen_keys": d["pred_labels_from_search_with_unseen_keys"],
            "pred_similarity_from_search_with_seen_keys": d["pred_similarity_from_search_with_seen_keys"],
            "micro_acc": {str(k): v for k, v in res["micro_acc"].items()}, "macro_acc": {str(k): v for k, v in res["macro_acc"].items()},
            "per_class_acc": {str(k): v for k, v in res["per_class_acc"].items()}, "final_pred_labels": res["final_pred_labels"],
            "membership_lines": sink.getvalue().splitlines()}
    import torch
    out["_meta"] = {"numpy": np.__version__, "torch": torch.__version__, "reference": "bioscan-ml/bioscan-clip @ 2024-10-24",
                    "functions": "scripts/method_one_eval.py: search_threshold_with_harmonic_mean, get_final_pred_and_acc, "
                                 "check_for_acc_about_correct_predict_seen_or_unseen"}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("wrote", a.out, os.path.getsize(a.out), "bytes; best threshold", float(best),
          "top-1 species", {n: out["splits"][n]["micro_acc"]["1"]["species"] for n in out["splits"]})


if __name__ == "__main__":
    main()
