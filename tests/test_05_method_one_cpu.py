"""CPU checks of the method-one evaluation (scripts/method_one_eval.py): the host functions reproduce the reference's outputs pinned
in tests/golden/method_one.json (written by tools/gen_method_one_golden.py from the imported reference) with ``==``, the threshold
choice from integer counts, the host-side validation of the three new entry points, and the documents."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
ENTRY_POINTS = ("bsclip_retrieval_match_bits", "bsclip_retrieval_merge_hit_ranks", "bsclip_retrieval_threshold_sweep")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "method_one.json")) as f:
        return json.load(f)


def _args(k_list):
    return types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=list(k_list)))


def _by_int(d):
    return {int(k): v for k, v in d.items()}


def _split_data(gold):
    keys = ("pred_labels_from_search_with_seen_keys", "pred_similarity_from_search_with_seen_keys",
            "pred_labels_from_search_with_unseen_keys")
    return [dict({k: sp[k] for k in keys}, gt_label=sp["gt_label"]) for sp in gold["splits"].values()]


def test_fixture_has_the_cases_it_is_meant_to_pin(gold):
    grid = set(np.linspace(0, 1, gold["num_intervals"]).tolist())
    sims = [row for sp in gold["splits"].values() for row in sp["pred_similarity_from_search_with_seen_keys"]]
    flat = [v for row in sims for v in row]
    assert any(v in grid for v in flat) and min(flat) < 0 and max(flat) > 1
    assert any(row != sorted(row, reverse=True) for row in sims)
    assert all(float(np.float32(v)) == v for v in flat)                 # float32 values: the GPU path can be fed the same numbers
    assert all(len(sp["gt_label"]) == 40 for sp in gold["splits"].values()) and len(gold["splits"]) == 2


def test_host_threshold_search_equals_reference(gold):
    import method_one_eval as M
    best = M.search_threshold_with_harmonic_mean(_args(gold["k_list"]), _split_data(gold), num_intervals=gold["num_intervals"])
    assert best == gold["best_threshold"]
    assert 0 < best < 1


def test_host_tables_merged_lists_and_membership_equal_reference(gold, capsys):
    import method_one_eval as M
    args = _args(gold["k_list"])
    for sp in gold["splits"].values():
        out = M.get_final_pred_and_acc(args, sp["pred_labels_from_search_with_seen_keys"], sp["pred_similarity_from_search_with_seen_keys"],
                                       sp["pred_labels_from_search_with_unseen_keys"], sp["gt_label"],
                                       best_threshold=gold["best_threshold"])
        assert out["micro_acc"] == _by_int(sp["micro_acc"])
        assert out["macro_acc"] == _by_int(sp["macro_acc"])
        assert out["per_class_acc"] == _by_int(sp["per_class_acc"])
        assert out["final_pred_labels"] == sp["final_pred_labels"]
        assert out["gt_labels"] == sp["gt_label"] and out["best_threshold"] == gold["best_threshold"]
        final, gt = M.make_final_pred(args, sp["pred_labels_from_search_with_seen_keys"], sp["pred_similarity_from_search_with_seen_keys"],
                                      sp["pred_labels_from_search_with_unseen_keys"], sp["gt_label"], gold["best_threshold"])
        assert final == sp["final_pred_labels"] and gt is sp["gt_label"]
        capsys.readouterr()
        shares = M.check_for_acc_about_correct_predict_seen_or_unseen(out["final_pred_labels"], gold["species_list"])
        assert capsys.readouterr().out.splitlines() == sp["membership_lines"]
        assert [f"for k = {k}: {shares[k]}" for k in (1, 3, 5)] == sp["membership_lines"]


def test_threshold_search_needs_k_1(gold):
    import method_one_eval as M
    with pytest.raises(KeyError):
        M.search_threshold_with_harmonic_mean(_args([3, 5]), _split_data(gold), num_intervals=3)


def test_decide_prediction_is_strict_and_a_nan_takes_the_search_list():
    import method_one_eval as M
    first = [{"species": ["a0", "a1", "a2", "a3"], "genus": ["A0", "A1", "A2", "A3"]}]
    second = [{"species": ["b0", "b1", "b2", "b3"], "genus": ["B0", "B1", "B2", "B3"]}]
    got = M.decide_prediction_with_threshold(None, first, [[0.5, 0.25, float("nan"), 0.75]], second, 0.5)
    assert got == [{"species": ["b0", "b1", "b2", "a3"], "genus": ["B0", "B1", "B2", "A3"]}]


def test_harmonic_mean():
    import method_one_eval as M
    assert M.harmonic_mean([0.5, 0.25]) == 2 / (1 / 0.5 + 1 / 0.25)
    assert M.harmonic_mean([0.3, 0, 0.9]) == 0 and M.harmonic_mean([0.0]) == 0
    assert M.harmonic_mean([0.7]) == 1 / (1 / 0.7)


def test_pick_threshold_from_integer_counts():
    from bioscanclip.hip.method_one import pick_threshold
    thr = np.linspace(0, 1, 5)
    # a zero accuracy gives harmonic mean 0: threshold 1 (40 and 0 right) loses to threshold 2 (10 and 10) although its sum is larger
    assert pick_threshold([[0, 40, 10, 3, 0], [7, 0, 10, 3, 0]], [40, 40], thr) == thr[2]
    # ties keep the first threshold; different totals per split
    assert pick_threshold([[5, 8, 8, 8, 2], [3, 9, 9, 9, 1]], [10, 30], thr) == thr[1]
    # all zero: 0 > -inf holds once, for the first threshold
    assert pick_threshold([[0, 0, 0], [0, 0, 0]], [4, 4], [0.2, 0.1, 0.3]) == 0.2
    # a single threshold, a single split
    assert pick_threshold([[3]], [4], [0.25]) == 0.25
    # the arithmetic is the reference's: count * 1.0 / Q per split, then len / sum(1 / a), strictly greater wins
    counts, totals = [[13, 14], [29, 27]], [37, 41]
    hm = [2 / (1 / (c0 * 1.0 / 37) + 1 / (c1 * 1.0 / 41)) for c0, c1 in zip(*counts)]
    assert pick_threshold(counts, totals, [0.1, 0.9]) == (0.9 if hm[1] > hm[0] else 0.1)


def test_hip_eval_bogus_raises_before_any_loader_is_touched(monkeypatch):
    import method_one_eval as M
    from bioscanclip.util import synthetic

    def boom(*a, **kw):
        raise AssertionError("a loader was built")
    monkeypatch.setattr(synthetic, "SyntheticEvalLoader", boom)
    with pytest.raises(ValueError, match="hip_eval"):
        M.main(["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", "hip_eval=bogus"])

    class Loader:
        def __iter__(self):
            raise AssertionError("a loader was read")
    with pytest.raises(ValueError, match="hip_eval"):
        M.method_1_inference_and_eval_for_seen_and_unseen(types.SimpleNamespace(hip_eval="bogus"), None, Loader(), Loader(), Loader(),
                                                          Loader(), Loader(), "cuda")


# ---- host validation of the entry points, without a GPU ------------------------------------------------------------------------

def _lib():
    from bioscanclip.hip import lib
    return lib, lib.load()


def test_match_bits_validation():
    lib, h = _lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)
    call = lambda idx=one, Q=4, k=5, keys=one, K=7, ql=one, L=4, member=None, C=0, level=0, bits=one, flag=one: \
        h.bsclip_retrieval_match_bits(idx, Q, k, keys, K, ql, L, member, C, level, bits, flag, None)
    for kw, word in [(dict(k=17), "k=17"), (dict(k=0), "k=0"), (dict(L=9), "L=9"), (dict(L=0), "L=0"), (dict(Q=0), "Q=0"), (dict(K=0), "K=0"),
                     (dict(idx=None), "null"), (dict(keys=None), "null"), (dict(ql=None), "null"), (dict(bits=None), "null"),
                     (dict(flag=None), "null"), (dict(member=one, C=3, level=4), "level"), (dict(member=one, C=3, level=-1), "level"),
                     (dict(member=one, C=0), "C=0"), (dict(bits=odd), "aligned"), (dict(idx=ctypes.c_void_p(20)), "aligned"),
                     (dict(member=odd, C=3), "aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())


def test_merge_hit_ranks_validation():
    lib, h = _lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)
    call = lambda sim=one, Q=4, k=5, A=one, B=one, L=4, t=0.5, out=one: \
        h.bsclip_retrieval_merge_hit_ranks(sim, Q, k, A, B, L, ctypes.c_double(t), out, None)
    for kw, word in [(dict(k=17), "k=17"), (dict(k=0), "k=0"), (dict(L=9), "L=9"), (dict(L=0), "L=0"), (dict(Q=0), "Q=0"),
                     (dict(sim=None), "null"), (dict(A=None), "null"), (dict(B=None), "null"), (dict(out=None), "null"),
                     (dict(sim=odd), "aligned"), (dict(A=odd), "aligned"), (dict(out=odd), "aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())


def test_threshold_sweep_validation():
    lib, h = _lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)
    call = lambda sim=one, Q=4, k=5, A=one, B=one, L=4, level=3, kp=1, thr=one, T=10, counts=one: \
        h.bsclip_retrieval_threshold_sweep(sim, Q, k, A, B, L, level, kp, thr, T, counts, None)
    for kw, word in [(dict(k=17), "k=17"), (dict(L=9), "L=9"), (dict(level=4), "level=4"), (dict(level=-1), "level"), (dict(kp=0), "k_prime"),
                     (dict(Q=0), "Q=0"), (dict(T=0), "T=0"), (dict(sim=None), "null"), (dict(A=None), "null"), (dict(B=None), "null"),
                     (dict(thr=None), "null"), (dict(counts=None), "null"), (dict(thr=ctypes.c_void_p(20)), "aligned"),
                     (dict(counts=odd), "aligned"), (dict(sim=odd), "aligned")]:
        assert call(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())


def test_ops_wrappers_refuse_cpu_tensors():
    import torch
    from bioscanclip.hip import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.retrieval_match_bits(torch.zeros(2, 5, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32))
    z = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.retrieval_merge_hit_ranks(torch.zeros(2, 5), z, z, 0.5)
    with pytest.raises(ValueError, match="GPU"):
        ops.retrieval_threshold_sweep(torch.zeros(2, 5), z, z, 3, 1, torch.zeros(3, dtype=torch.float64))


def test_header_and_integration_name_each_entry_point():
    hdr = open(os.path.join(ROOT, "include", "bsclip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in ENTRY_POINTS:
        assert hdr.count(fn) >= 1 and fn in doc, fn
    block = hdr[hdr.index("Method-one evaluation"):hdr.index("int bsclip_retrieval_threshold_sweep")]
    for word in ("match_bits:", "merge_hit_ranks:", "threshold_sweep:", "decide_prediction_with_threshold",
                 "search_threshold_with_harmonic_mean", "check_for_acc_about_correct_predict_seen_or_unseen"):
        assert word in block, word
    from bioscanclip.hip import lib
    assert lib.load().bsclip_abi_version() == 10
