"""CPU checks of the method-two evaluation (scripts/method_two_fine_tuning_and_eval.py): the host functions reproduce the
reference's outputs pinned in tests/golden/method_two.json (written by tools/gen_method_two_golden.py from the imported reference)
with ``==``, the fixture holds the cases it is meant to pin, the threshold grid has ``num_intervals + 1`` points, the classifier
wrapper keeps the reference's ``state_dict`` keys, and ``bsclip_class_softmax_topk`` is exported and validates on the host."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
SPLIT_KEYS = ("pred_labels_from_a", "pred_confidence_from_a", "pred_labels_from_b", "gt_labels")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "method_two.json")) as f:
        return json.load(f)


def _args(k_list):
    return types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=list(k_list)))


def _by_int(d):
    return {int(k): v for k, v in d.items()}


def _split_data(gold):
    return [{k: sp[k] for k in SPLIT_KEYS} for sp in gold["splits"].values()]


def test_fixture_has_the_cases_it_is_meant_to_pin(gold):
    grid = np.linspace(0, 1, gold["num_intervals"] + 1).tolist()
    rows = [row for sp in gold["splits"].values() for row in sp["pred_confidence_from_a"]]
    flat = [v for row in rows for v in row]
    assert all(float(np.float32(v)) == v for v in flat)                 # float32 values: the GPU path can be fed the same numbers
    for v in (0.0, 0.5, 1.0):                                           # on the grid exactly, where the comparison is strict
        assert v in flat and v in grid
    assert all(row == sorted(row, reverse=True) and sum(row) <= 1.0 and min(row) >= 0.0 for row in rows)   # softmax shape
    assert any(len(set(row)) == 1 for row in rows)                      # a row of equal values
    assert 0 < gold["best_threshold"] < 1 and gold["best_threshold"] in grid
    assert len(gold["splits"]) == 2
    C = len(gold["label_to_index_dict"])
    for sp in gold["splits"].values():
        assert len(sp["gt_labels"]) == 40 and np.asarray(sp["class_indices"]).shape == (40, 5)
        assert all(len(set(row)) == 5 and 0 <= min(row) and max(row) < C for row in sp["class_indices"])
        # the label lists are the class indices looked up in idx_to_all_labels
        for row, pred in zip(sp["class_indices"], sp["pred_labels_from_a"]):
            assert pred == {lv: [gold["idx_to_all_labels"][str(i)][lv] for i in row] for lv in pred}


def test_label_map_equals_reference(gold):
    import method_two_fine_tuning_and_eval as M
    loader = [(None, None, None, None, None, None, b) for b in gold["seen_label_batches"]]
    label_to_index_dict, idx_to_all_labels = M.load_all_seen_species_name_and_create_label_map(loader)
    assert label_to_index_dict == gold["label_to_index_dict"] and list(label_to_index_dict) == list(gold["label_to_index_dict"])
    assert idx_to_all_labels == {int(k): v for k, v in gold["idx_to_all_labels"].items()}
    assert M._class_list(label_to_index_dict) == sorted(label_to_index_dict)       # position in the class list == the map's value
    batch = gold["seen_label_batches"][0]
    want = [gold["label_to_index_dict"][s] for s in batch["species"]]
    assert M.label_batch_to_species_idx(batch, label_to_index_dict).tolist() == want
    assert M.label_to_index(batch["species"][0], label_to_index_dict) == want[0]
    assert sorted(M.get_all_unique_species_from_dataloader(loader)) == sorted(label_to_index_dict)


def test_host_threshold_search_equals_reference(gold):
    import method_two_fine_tuning_and_eval as M
    best = M.search_threshold_with_harmonic_mean(_args(gold["k_list"]), _split_data(gold), num_intervals=gold["num_intervals"])
    assert best == gold["best_threshold"]
    assert 0 < best < 1
    seen, unseen = [tuple(sp[k] for k in SPLIT_KEYS) for sp in gold["splits"].values()]
    outs = M.score_predictions_on_host(_args(gold["k_list"]), seen, unseen, num_intervals=gold["num_intervals"])
    assert [o["best_threshold"] for o in outs] == [gold["best_threshold"]] * 2


def test_host_tables_merged_lists_and_printed_lines_equal_reference(gold, capsys):
    import method_two_fine_tuning_and_eval as M
    args = _args(gold["k_list"])
    outs = []
    for sp in gold["splits"].values():
        out = M.get_final_pred_and_acc(args, sp["pred_labels_from_a"], sp["pred_confidence_from_a"], sp["pred_labels_from_b"],
                                       sp["gt_labels"], best_threshold=gold["best_threshold"])
        outs.append(out)
        assert out["micro_acc"] == _by_int(sp["micro_acc"])
        assert out["macro_acc"] == _by_int(sp["macro_acc"])
        assert out["per_class_acc"] == _by_int(sp["per_class_acc"])
        assert out["final_pred_labels"] == sp["final_pred_labels"]
        assert out["gt_labels"] == sp["gt_labels"] and out["best_threshold"] == gold["best_threshold"]
        final, gt = M.make_final_pred(args, sp["pred_labels_from_a"], sp["pred_confidence_from_a"], sp["pred_labels_from_b"],
                                      sp["gt_labels"], gold["best_threshold"])
        assert final == sp["final_pred_labels"] and gt is sp["gt_labels"]
        assert M.decide_prediction_with_threshold(args, sp["pred_labels_from_a"], sp["pred_confidence_from_a"],
                                                  sp["pred_labels_from_b"], gold["best_threshold"]) == sp["final_pred_labels"]
        capsys.readouterr()
        M.check_for_acc_about_correct_predict_seen_or_unseen(out["final_pred_labels"], gold["species_list"])
        assert capsys.readouterr().out.splitlines() == sp["membership_lines"]
    capsys.readouterr()
    M.print_acc_for_google_doc(outs[0], outs[1], K_LIST=gold["k_list"])
    assert capsys.readouterr().out.splitlines() == gold["google_doc_lines"]
    assert len(gold["google_doc_lines"]) == 6


def test_search_grid_has_one_point_more_than_intervals():
    import method_two_fine_tuning_and_eval as M
    from bioscanclip.hip import method_one, method_two
    for n in (1, 4, 1000):
        grid = method_two.linspace_thresholds(n)
        assert grid.dtype == np.float64 and len(grid) == n + 1 and grid.tolist() == np.linspace(0, 1, n + 1).tolist()
    assert len(method_two.linspace_thresholds()) == 1001 and len(method_one.linspace_thresholds()) == 1000
    # the host search walks the same grid: with 4 intervals the thresholds are 0, .25, .5, .75, 1 -- only 0.25 separates these splits
    a = {"species": ["x"], "order": ["x"], "family": ["x"], "genus": ["x"]}
    b = {"species": ["y"], "order": ["y"], "family": ["y"], "genus": ["y"]}
    data = [{"pred_labels_from_a": [a], "pred_confidence_from_a": [[0.3]], "pred_labels_from_b": [b], "gt_labels": [{k: "x" for k in a}]},
            {"pred_labels_from_a": [a], "pred_confidence_from_a": [[0.2]], "pred_labels_from_b": [b], "gt_labels": [{k: "y" for k in a}]}]
    assert M.search_threshold_with_harmonic_mean(_args([1]), data, num_intervals=4) == 0.25
    assert M.search_threshold_with_harmonic_mean(_args([1]), data, num_intervals=3) == 0.0     # 0, 1/3, 2/3, 1: none separates them
    assert M.harmonic_mean([0.5, 0.25]) == 2 / (1 / 0.5 + 1 / 0.25) and M.harmonic_mean([0.3, 0]) == 0


def test_vit_with_extra_layer_keeps_the_reference_state_dict():
    import method_two_fine_tuning_and_eval as M
    from bioscanclip.util.util import EncoderWithExtraLayer
    vit = nn.Sequential(nn.Linear(4, 768))
    m = M.ViTWIthExtraLayer(vit, nn.Linear(768, 7))
    assert list(m.state_dict()) == ["vit.0.weight", "vit.0.bias", "new_linear_layer.weight", "new_linear_layer.bias"]
    assert isinstance(m, EncoderWithExtraLayer) and m.encoder is vit and m.vit is vit
    assert len(list(m.parameters())) == 4 and [n for n, _ in m.named_children()] == ["vit", "new_linear_layer"]
    # a state_dict saved by the reference's class (plain nn.Module with the same two attributes) loads strictly
    ref = nn.Module()
    ref.vit, ref.new_linear_layer = nn.Sequential(nn.Linear(4, 768)), nn.Linear(768, 7)
    m.load_state_dict(ref.state_dict())
    assert torch.equal(m.new_linear_layer.weight, ref.new_linear_layer.weight) and torch.equal(m.vit[0].bias, ref.vit[0].bias)
    assert torch.equal(m.get_feature(torch.ones(2, 4)), vit(torch.ones(2, 4)))
    # EncoderWithExtraLayer's behaviour: no torch compute path
    with pytest.raises(RuntimeError, match="no_grad"):
        m(torch.ones(2, 4))
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        m(torch.ones(2, 4))
    with pytest.raises(NotImplementedError):
        M.ViTWIthExtraLayer(vit, nn.Sequential(nn.Linear(768, 7), nn.Softmax(dim=-1)))


def test_script_has_the_reference_names_and_refuses_what_it_does_not_run(monkeypatch):
    import method_two_fine_tuning_and_eval as M
    for name in ("ViTWIthExtraLayer", "inference_with_fine_tuned_image_encoder", "decide_prediction_with_threshold", "make_final_pred",
                 "inference_with_original_image_encoder_and_dna_encoder", "harmonic_mean", "search_threshold_with_harmonic_mean",
                 "get_final_pred_and_acc", "method_2_inference_and_eval_for_seen_and_unseen", "get_all_unique_species_from_dataloader",
                 "load_all_seen_species_name_and_create_label_map", "label_to_index", "label_batch_to_species_idx", "fine_tuning_epoch",
                 "evaluate_epoch", "print_acc_for_google_doc", "check_for_acc_about_correct_predict_seen_or_unseen", "main"):
        assert callable(getattr(M, name)), name
    from bioscanclip.util import synthetic

    def boom(*a, **kw):
        raise AssertionError("a loader was built")
    monkeypatch.setattr(synthetic, "SyntheticEvalLoader", boom)
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false"]
    with pytest.raises(ValueError, match="hip_eval"):
        M.main(common + ["hip_eval=bogus"])
    with pytest.raises(NotImplementedError, match="open_clip"):
        M.main(common + ["model_config.for_open_clip=true"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one GPU"):
        M.main(common)
    with pytest.raises(ValueError, match="hip_eval"):
        M.method_2_inference_and_eval_for_seen_and_unseen(types.SimpleNamespace(hip_eval="bogus"), None, None, None, None, None, None, {},
                                                          {}, "cuda")


# ---- the entry point, without a GPU ----------------------------------------------------------------------------------------------

def test_entry_point_is_exported_declared_and_abi_stays_10():
    import re
    from bioscanclip.hip import lib
    h = lib.load()
    assert "bsclip_class_softmax_topk" in lib.SIGNATURES and hasattr(h, "bsclip_class_softmax_topk")
    assert lib.SIGNATURES["bsclip_class_softmax_topk"] == lib.SIGNATURES["bsclip_class_topk"]
    assert h.bsclip_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "bsclip.h")).read()
    assert re.search(r"\bint bsclip_class_softmax_topk\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    block = text[text.index("class_softmax_topk:"):text.index("int bsclip_class_softmax_topk")]
    for word in ("method_two_fine_tuning_and_eval.py:57-62", "ties to the lower class index", "LOGIT descending", "NaN"):
        assert word in block, word
    assert "bsclip_class_softmax_topk" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_class_softmax_topk_validates_on_the_host():
    from bioscanclip.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(64)        # non-null and 16-byte aligned: every check below comes before any dereference or launch

    def call(logits=one, ldc=132, B=4, C=130, k=5, conf=one, idx=one):
        return h.bsclip_class_softmax_topk(logits, ldc, B, C, k, conf, idx, None)

    for kw in ({"logits": None}, {"conf": None}, {"idx": None}):
        assert call(**kw) == -1 and "null pointer" in lib.last_error(), kw
    assert call(C=3, k=5, ldc=4) == -1 and "k=5" in lib.last_error()         # k > C
    assert call(k=17) == -1 and "k=17" in lib.last_error()                   # k > 16
    assert call(k=0) == -1 and "k=0" in lib.last_error()
    assert call(ldc=128) == -1 and "ldc=128" in lib.last_error()             # ldc < C
    assert call(ldc=134) == -1 and "ldc=134" in lib.last_error()             # ldc % 4 != 0
    assert call(logits=ctypes.c_void_p(72)) == -1 and "aligned" in lib.last_error()     # misaligned logits
    assert call(idx=ctypes.c_void_p(68)) == -1 and "aligned" in lib.last_error()
    assert call(B=0) == -1 and "B=0" in lib.last_error()
    assert call(C=0) == -1 and "C=0" in lib.last_error()
    for message in (lib.last_error(),):
        assert message.startswith("bsclip_class_softmax_topk")


def test_ops_wrapper_refuses_cpu_tensors():
    from bioscanclip.hip import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.class_softmax_topk(torch.zeros(2, 8), 8, 5)
