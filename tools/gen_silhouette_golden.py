"""Pins the silhouette scores: writes ``tests/golden/silhouette.json`` by running the IMPORTED REFERENCE's own
``calculate_silhouette_score`` (``scripts/inference_and_eval.py``:407-411, sklearn's ``silhouette_samples`` and ``avg_list``) on one
small seeded case.

    python tools/gen_silhouette_golden.py --reference <checkout of bioscan-ml/bioscan-clip>

Runs only where the reference checkout exists, never on the GPU box.  The reference is imported the way
``tools/gen_method_one_golden.py`` imports it: the real ``transformers`` first, packages the reference imports but this path does
not need as ``MagicMock``; sklearn is real.  ``calculate_silhouette_score`` only prints, so the per-sample values are taken where it
computes them: the name ``silhouette_samples`` in the reference module is wrapped by a recorder that calls sklearn's function
unchanged and keeps what it returned.

The fixture holds data only: N = 48 float32 feature rows of D = 16 (as float64 lists, exactly the float32 values), the 48
four-level label dicts, and per level sklearn's per-sample values and the line the reference printed.  The reference function is
handed the float32 values widened to float64, so the recorded values are sklearn's float64 path (on float32 input sklearn returns
float32 values).  The labels hold the cases the GPU path must get right: a species with one member (silhouette 0), the genus string
"not_classified" under two families (one class, as sklearn sees equal strings) and classes of unequal sizes.  Near-duplicate rows
are left out on purpose: sklearn's float64 distances are the Gram form, whose own error on such a pair (about 1e-11 here) would be
pinned with it; the GPU tests cover that case against the difference-form oracle.
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
N, D = 48, 16


def import_reference(ref_root):
    sys.dont_write_bytecode = True
    import importlib.machinery
    import importlib.util
    from transformers import BertConfig, BertForMaskedLM, BertModel  # noqa: F401  (real, and resolved before anything is stubbed)
    import sklearn.metrics  # noqa: F401  (real: the function under record)
    import sklearn.preprocessing  # noqa: F401
    for name in ["torchtext", "torchtext.vocab", "timm", "timm.models", "timm.models.vision_transformer", "open_clip", "loratorch",
                 "loratorch.layers", "clip", "faiss", "wandb", "torchvision", "torchvision.transforms", "seaborn", "h5py", "umap",
                 "plotly", "plotly.express", "hydra", "omegaconf", "matplotlib", "matplotlib.pyplot", "PIL"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = MagicMock(__spec__=importlib.machinery.ModuleSpec(name, None))
    sys.modules["bioscanclip.util.dataset"] = MagicMock()
    sys.modules["hydra"].main = lambda *a, **kw: (lambda fn: fn)
    try:
        import tqdm  # noqa: F401
    except Exception:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
        sys.modules["tqdm"].__spec__ = importlib.machinery.ModuleSpec("tqdm", None)
        sys.modules["tqdm"].tqdm = list
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ref_root, "scripts"))
    spec = importlib.util.spec_from_file_location("ref_inference_and_eval", os.path.join(ref_root, "scripts", "inference_and_eval.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def make_case():
    """(features float32 [N, D], label dicts).  Taxonomy: 2 orders, 4 families, genera of which "not_classified" sits under families
    f1 and f2, 9 species of sizes 1 .. 9 or so; the features are a centre per species plus noise, so the scores are not all alike."""
    rng = np.random.default_rng(61)
    species = [  # (order, family, genus, species, members)
        ("o0", "f0", "g0", "s0", 9), ("o0", "f0", "g0", "s1", 7), ("o0", "f0", "g1", "s2", 6),
        ("o0", "f1", "not_classified", "s3", 5), ("o0", "f1", "g2", "s4", 1),            # s4: a singleton species (and genus)
        ("o1", "f2", "not_classified", "s5", 6), ("o1", "f2", "g3", "s6", 4),
        ("o1", "f3", "g4", "s7", 8), ("o1", "f3", "g4", "s8", 2)]
    assert sum(s[4] for s in species) == N
    labels, rows = [], []
    for o, f, g, s, n in species:
        centre = rng.standard_normal(D) * 1.5 + {"o0": 0.0, "o1": 2.0}[o]
        for _ in range(n):
            labels.append({"order": o, "family": f, "genus": g, "species": s})
            rows.append(centre + 0.6 * rng.standard_normal(D))
    x = np.asarray(rows, dtype=np.float32)
    order = rng.permutation(N)                                                             # the classes are not contiguous
    return x[order], [labels[i] for i in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "silhouette.json"))
    a = ap.parse_args()
    ref = import_reference(a.reference)
    x, labels = make_case()
    recorded = []
    sklearn_fn = ref.silhouette_samples

    def recorder(features, gt_list, **kw):
        out = sklearn_fn(features, gt_list, **kw)
        recorded.append(np.asarray(out))
        return out
    ref.silhouette_samples = recorder
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        ref.calculate_silhouette_score(None, x.astype(np.float64), (None, labels))
    lines = sink.getvalue().splitlines()
    assert len(recorded) == len(lines) == len(LEVELS) and all(r.dtype == np.float64 and r.shape == (N,) for r in recorded)
    import sklearn
    out = {"N": N, "D": D, "levels": LEVELS, "features": x.astype(np.float64).tolist(), "labels": labels,
           "samples": {lv: r.tolist() for lv, r in zip(LEVELS, recorded)}, "printed_lines": lines,
           "_meta": {"numpy": np.__version__, "sklearn": sklearn.__version__, "reference": "bioscan-ml/bioscan-clip @ 2024-10-24",
                     "functions": "scripts/inference_and_eval.py: calculate_silhouette_score, avg_list",
                     "input": "the float32 features widened to float64 (sklearn's float64 path)"}}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    for ln in lines:
        print(ln)


if __name__ == "__main__":
    main()
