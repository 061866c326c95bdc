"""Silhouette scores on the GPU: ``bsclip_silhouette_samples`` and ``bioscanclip/hip/silhouette.py`` against the tests' float64
oracle (tests/silhouette_oracle.py), against sklearn's values pinned in tests/golden/silhouette.json, and through
``scripts/inference_and_eval.py``.

Bar: per case max |s - s_f64| <= max(4 x the worst error of the f32 CPU baseline -- ``torch.cdist`` without the matrix-multiply form,
f32 sums -- on the same inputs, 16 x 2^-24 = 9.54e-7).  The baseline is evaluated inside the test.  In every kernel case the labels
are shuffled (the sort and the scatter back are exercised), the output buffer is NaN-filled with spare rows that must stay NaN, the
feature buffer's padding columns hold NaN (they are not features), and the call is made twice and must return the same bits.
Measured on an MI355X, kernel vs f64 / f32 baseline vs f64 / gate: (5, 3, 2) 5.9e-8 / 1.0e-7 / 9.5e-7; (67, 24, 5) 3.5e-8 / 1.5e-7 /
9.5e-7; (300, 768, 37) 1.4e-7 / 2.5e-7 / 1.0e-6; near-duplicates (130, 768, 9) 6.0e-8 / 1.6e-7 / 9.5e-7; (513, 100, 200) 1.4e-7 /
2.1e-7 / 9.5e-7; (4 100, 8, 2) 3.1e-8 / 2.9e-6 / 1.1e-5 (the baseline's f32 sums over 4 000 members show there); the golden fixture's
four levels 2.4e-8 .. 5.2e-8 against sklearn's float64 values (gate 9.5e-7).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
LEVELS = ["order", "family", "genus", "species"]
SPARE = 7


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- the cases -------------------------------------------------------------------------------------------------------------------

def _labels(rng, N, C, spread=None):
    """N ids with every one of the C classes present; ``spread``: the extra N - C members fall into the first ``spread`` classes
    only (the others stay singletons)."""
    return np.concatenate([np.arange(C), rng.integers(0, C if spread is None else spread, size=N - C)])


def _clustered(rng, ids, D, noise=0.7, shift=0.0):
    centres = rng.standard_normal((int(ids.max()) + 1, D))
    return (centres[ids] + noise * rng.standard_normal((len(ids), D)) + shift).astype(np.float32)


def _shuffled(rng, x, ids):
    order = rng.permutation(len(ids))
    return np.ascontiguousarray(x[order]), ids[order]


def _case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "tiny":                 # (5, 3, 2): smaller than any tile, D padded
        ids = np.asarray([0, 0, 0, 1, 1])
        x = _clustered(rng, ids, 3)
    elif name == "ragged":             # (67, 24, 5): ragged in rows, columns and K
        ids = _labels(rng, 67, 5)
        x = _clustered(rng, ids, 24)
    elif name == "real_d":             # (300, 768, 37): the real D
        ids = _labels(rng, 300, 37)
        x = _clustered(rng, ids, 768)
    elif name == "near_duplicates":    # (130, 768, 9): cluster centre + 0.7 noise + 3.0; every odd row its predecessor + 1e-4 noise
        ids = _labels(rng, 130, 9)
        ids[1::2] = ids[0::2]
        assert len(set(ids.tolist())) == 9
        x = _clustered(rng, ids, 768, noise=0.7, shift=3.0)
        x[1::2] = x[0::2] + np.float32(1e-4) * rng.standard_normal((65, 768)).astype(np.float32)
        x[11] = x[10]                  # one pair is exactly equal
    elif name == "many_classes":       # (513, 100, 200): more classes than a tile has columns, 79 singletons, classes across tile edges
        ids = _labels(rng, 513, 200, spread=140)
        x = _clustered(rng, ids, 100)
    elif name == "long_sums":          # (4100, 8, 2): one class of 4 000 members
        ids = np.concatenate([np.zeros(4000, dtype=np.int64), np.ones(100, dtype=np.int64)])
        x = _clustered(rng, ids, 8)
    else:
        raise KeyError(name)
    return _shuffled(rng, x, ids)


CASES = {"tiny": (5, 3, 2), "ragged": (67, 24, 5), "real_d": (300, 768, 37), "near_duplicates": (130, 768, 9),
         "many_classes": (513, 100, 200), "long_sums": (4100, 8, 2)}


def _kernel(x, ids):
    """The raw path with the buffers the docstring describes: float64 [N] in the original order."""
    from bioscanclip.hip import ops
    from bioscanclip.hip.silhouette import class_segments, dense_ids
    N, D = x.shape
    dense, _ = dense_ids(ids.tolist())     # first-appearance ids, as the public functions hand them out: the same class order
    perm, seg = class_segments(torch.from_numpy(dense).cuda())
    ld = (D + 3) // 4 * 4 + 4
    buf = torch.full((N, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :D] = torch.from_numpy(x).cuda().index_select(0, perm)
    outs = []
    for _ in range(2):
        out = torch.full((N + SPARE,), float("nan"), dtype=torch.float32, device="cuda")
        got = ops.silhouette_samples(buf, seg, D, out=out)
        assert got.shape == (N,) and got.data_ptr() == out.data_ptr()
        assert torch.isnan(out[N:]).all(), "rows beyond N were written"
        outs.append(out[:N].clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "a second call returned other bits"
    assert not torch.isnan(outs[0]).any()
    s = torch.empty(N, dtype=torch.float32, device="cuda")
    s[perm] = outs[0]
    return s.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_the_float64_oracle(name):
    import silhouette_oracle as O
    from bioscanclip.hip.silhouette import silhouette_samples
    x, ids = _case(name)
    N, D, C = CASES[name]
    assert x.shape == (N, D) and len(set(ids.tolist())) == C and x.dtype == np.float32
    want = O.silhouette_f64(x, ids.tolist())
    tol, base_err = O.gate(x, ids.tolist(), want)
    got = _kernel(x, ids)
    err = float(np.max(np.abs(got - want)))
    print(f"{name} {CASES[name]}: kernel vs f64 {err:.3e}, f32 baseline vs f64 {base_err:.3e}, gate {tol:.3e}")
    assert err <= tol, f"{name}: max |s - s_f64| {err:.3e} above the gate {tol:.3e} (f32 baseline {base_err:.3e})"
    sizes = np.bincount(ids)
    assert (got[sizes[ids] == 1] == 0.0).all()                              # singleton classes give exactly 0
    if name == "near_duplicates":
        assert len(np.unique(x, axis=0)) == N - 1 and np.isfinite(got).all()   # the exactly equal pair is there
    # the public function: strings as labels, the same kernel, the same bits
    public = silhouette_samples(x, [f"c{i}" for i in ids.tolist()])
    assert public.dtype == np.float64 and np.array_equal(public, got)
    assert np.array_equal(silhouette_samples(torch.from_numpy(x).cuda().double(), ids.tolist()), got)   # a GPU tensor, another dtype


def test_zero_quotient_and_exact_diagonal():
    """a = b = 0 gives 0 (``nan_to_num``), a class on one point against a far one gives exactly 1: d(i, i) and d of equal rows are 0."""
    from bioscanclip.hip.silhouette import silhouette_samples
    x = np.asarray([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [3.0, 4.0], [3.0, 4.0]], dtype=np.float32) + np.float32(1000.25)
    assert silhouette_samples(x, ["a", "a", "b", "c", "c"]).tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]


# ---- the pinned reference outputs ----------------------------------------------------------------------------------------------

def test_golden_fixture_all_four_levels():
    import silhouette_oracle as O
    from bioscanclip.hip.silhouette import silhouette_by_level
    with open(os.path.join(ROOT, "tests", "golden", "silhouette.json")) as f:
        gold = json.load(f)
    x = np.asarray(gold["features"], dtype=np.float32)
    by_level = silhouette_by_level(x, gold["labels"])
    assert list(by_level) == LEVELS
    for lv, line in zip(LEVELS, gold["printed_lines"]):
        want = np.asarray(gold["samples"][lv])
        tol, base_err = O.gate(x, [lab[lv] for lab in gold["labels"]], want)
        got = by_level[lv]["samples"]
        err = float(np.max(np.abs(got - want)))
        print(f"golden {lv}: kernel vs sklearn f64 {err:.3e}, f32 baseline {base_err:.3e}, gate {tol:.3e}")
        assert got.dtype == np.float64 and got.shape == (48,) and err <= tol
        assert (got[want == 0.0] == 0.0).all()
        total = 0.0
        for v in got.tolist():                                              # the mean is formed as the reference forms it
            total += v
        assert by_level[lv]["mean"] == total * 1.0 / 48
        pinned = float(line.split(" is : ")[1])
        assert pinned == O.avg_list(want) and abs(by_level[lv]["mean"] - pinned) <= tol
    assert list(silhouette_by_level(x, gold["labels"], levels=["genus"])) == ["genus"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_raise_value_error():
    from bioscanclip.hip.silhouette import silhouette_by_level, silhouette_samples
    rng = np.random.default_rng(3)
    x = rng.standard_normal((20, 12)).astype(np.float32)
    labels = [i % 4 for i in range(20)]
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_samples(x, [0] * 20)
    with pytest.raises(ValueError, match="Number of labels is 20"):
        silhouette_samples(x, list(range(20)))
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[13, 5] = bad
        with pytest.raises(ValueError, match="NaN or an infinity"):
            silhouette_samples(y, labels)
    with pytest.raises(ValueError, match="labels for 20 samples"):
        silhouette_samples(x, labels[:-1])
    dicts = [{"order": "o", "family": f"f{i % 2}", "genus": f"g{i % 3}", "species": f"s{i}"} for i in range(20)]
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_by_level(x, dicts)                                       # one order
    with pytest.raises(ValueError, match="Number of labels is 20"):
        silhouette_by_level(x, dicts, levels=["family", "species"])         # every species its own
    assert np.isfinite(silhouette_samples(x, labels)).all()                  # and the good call still works afterwards


@pytest.mark.parametrize("seg", [[0, 9, 5, 20], [0, 5, 9, 19], [1, 5, 9, 20], [0, 5, 1000000, 20], [0, -3, 9, 20], [0, 5, 9, 21]])
def test_corrupted_segments_set_flag_bit_1_and_nothing_is_computed(seg):
    from bioscanclip.hip import ops
    x = torch.randn(20, 12, device="cuda")
    seg_start = torch.tensor(seg, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((20 + SPARE,), float("nan"), dtype=torch.float32, device="cuda")
    ops.silhouette_samples(x, seg_start, out=out, flag=flag)
    assert int(flag.item()) == 2
    assert torch.isnan(out).all()
    with pytest.raises(ValueError, match="seg_start"):
        ops.check_silhouette_flag(int(flag.item()))
    with pytest.raises(ValueError, match="seg_start"):
        ops.silhouette_samples(x, seg_start)                                # without a caller's flag the wrapper raises itself


# ---- the script ----------------------------------------------------------------------------------------------------------------

def test_inference_and_eval_script_prints_the_scores(tmp_path, capsys):
    import inference_and_eval
    import silhouette_oracle as O
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", f"project_root_path={tmp_path}",
              "debug_flag=false", "synthetic_eval_batches=1"]
    capsys.readouterr()
    inference_and_eval.main(common + ["save_inference=true", "inference_and_eval_setting.silhouette=true"])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "silhouette" in ln]
    assert len(lines) == 8 and [ln.split()[4] for ln in lines] == LEVELS * 2
    assert out.index("Query_feature") < out.index("The silhouette score")   # after the accuracy table
    import glob
    cached = glob.glob(os.path.join(tmp_path, "extracted_embedding", "*", "*", "extracted_feature_from_val_split.npz"))
    assert len(cached) == 1
    z = np.load(cached[0], allow_pickle=True)
    at = 0
    for split in ("seen", "unseen"):
        d = z[split].item()
        x = np.asarray(d["encoded_image_feature"], dtype=np.float32)
        for lv in LEVELS:
            labels = [lab[lv] for lab in d["label_list"]]
            want = O.silhouette_f64(x, labels)
            tol, base_err = O.gate(x, labels, want)
            got = float(lines[at].split(" is : ")[1])
            assert lines[at].startswith(f"The silhouette score for {lv} level is : ")
            print(f"script {split} {lv}: mean {got!r}, oracle {O.avg_list(want)!r}, gate {tol:.3e}")
            assert abs(got - O.avg_list(want)) <= tol
            at += 1
    inference_and_eval.main(common + ["load_inference=true"])              # without the setting: no such line
    assert "silhouette" not in capsys.readouterr().out
