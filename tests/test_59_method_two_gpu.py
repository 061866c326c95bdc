"""Method-two evaluation on the GPU: ``bsclip_class_softmax_topk`` against numpy, the GPU protocol against the pinned reference
outputs (tests/golden/method_two.json) and against the host path of the same script, end to end on one pair of models.

Kernel bar.  Indices: exactly a numpy stable sort by (-logit, index) of the f32 logits.  Confidences: against the float64 softmax of
the same f32 logits; the tolerance is four times the max relative error that torch's CPU f32 ``F.softmax`` shows against that float64
value on the same inputs (the kernel's summation order differs from torch's -- per-lane partials, rescale, wave tree -- and ``expf``
is a few ulp), never less than 16 x 2^-24 = 9.54e-7.  The relative bound covers entries whose float64 value is at least 1e-30;
smaller ones are held to 1e-30 absolutely.  Measured on an MI355X: torch's error 5.9e-7 .. 1.24e-6 over the random cases (tolerance
2.4e-6 .. 5.0e-6), the kernel's worst selected entry 2.2e-7 .. 6.4e-7; special rows torch 3.1e-7 .. 6.7e-7, kernel 8.9e-8 .. 1.7e-7.
Everything after the kernel is ``==``.
"""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
LEVELS = ["order", "family", "genus", "species"]
FLOOR = 16 * 2.0 ** -24
TINY = 1e-30
B_LIST, K_LIST_KERNEL, B_MAX = (1, 3, 5, 41), (1, 5, 8, 9, 16), 41


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _args(k_list, **kw):
    return types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=list(k_list)), **kw)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------

def _padded(logits, pad):
    """The f32 [B, C] logits as a view into a GPU buffer [B, C rounded up to 128] whose padding columns hold ``pad``."""
    B, C = logits.shape
    buf = torch.full((B, (C + 127) // 128 * 128), pad, dtype=torch.float32, device="cuda")
    buf[:, :C] = torch.from_numpy(logits).cuda()
    return buf[:, :C]


def _reference(logits):
    """(order [B, C] by (-logit, index), float64 softmax [B, C], tolerance) for f32 logits without NaN."""
    order = np.argsort(-logits.astype(np.float64), axis=1, kind="stable")
    with np.errstate(invalid="ignore", over="ignore"):
        z = logits.astype(np.float64)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p64 = e / e.sum(axis=1, keepdims=True)
    p32 = F.softmax(torch.from_numpy(logits), dim=-1).numpy().astype(np.float64)
    big = p64 >= TINY
    torch_err = float(np.max(np.abs(p32[big] - p64[big]) / p64[big]))
    return order, p64, max(4 * torch_err, FLOOR), torch_err


def _check(conf, idx, order, p64, tol, k, what):
    conf, idx = conf.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    assert np.array_equal(idx, order[:len(idx), :k]), f"{what}: indices differ from the stable sort by (-logit, index)"
    want = np.take_along_axis(p64[:len(idx)], idx, axis=1)
    big = want >= TINY
    rel = float(np.max(np.abs(conf[big] - want[big]) / want[big])) if big.any() else 0.0
    small = float(np.max(np.abs(conf[~big] - want[~big]))) if (~big).any() else 0.0
    assert rel <= tol and small <= TINY, f"{what}: max relative error {rel:.3e} (tolerance {tol:.3e}), small entries off by {small:.3e}"
    return rel


@pytest.mark.parametrize("C", [5, 11, 63, 64, 65, 257, 916, 1027])      # 1027: more than one 1024-column trip of the first pass
def test_class_softmax_topk_matches_numpy(C):
    """B in {1, 3, 5, 41} (partial workgroups of four rows), k in {1, 5, 8, 9, 16} (both register-list sizes), ldc = C rounded up to
    128 with the padding filled with +1e30 and with NaN: padding must not show in any output."""
    from bioscanclip.hip import ops
    rng = np.random.default_rng(1000 + C)
    logits = (rng.standard_normal((B_MAX, C)) * 3.0).astype(np.float32)
    logits[7, C // 2] = logits[7, 0]                                     # an exact tie inside a row: the lower index comes first
    order, p64, tol, torch_err = _reference(logits)
    worst = 0.0
    for pad in (1e30, float("nan")):
        for B in B_LIST:
            view = _padded(logits[:B], pad)
            for k in [k for k in K_LIST_KERNEL if k <= C]:
                conf, idx = ops.class_softmax_topk(view, C, k)
                assert conf.shape == (B, k) and conf.dtype == torch.float32 and idx.dtype == torch.int64
                worst = max(worst, _check(conf, idx, order, p64, tol, k, f"C={C} B={B} k={k} pad={pad}"))
    print(f"C={C}: torch CPU f32 softmax vs f64 {torch_err:.3e}, tolerance {tol:.3e}, kernel vs f64 {worst:.3e}")


@pytest.mark.parametrize("C", [11, 257, 916, 1027])
def test_class_softmax_topk_special_rows(C):
    from bioscanclip.hip import ops
    rng = np.random.default_rng(2000 + C)
    rows = {}
    x = (rng.standard_normal((8, C)) * 2.0).astype(np.float32)
    rows["scaled"], x[0] = 0, (rng.standard_normal(C) * 1e4).astype(np.float32)     # logits of +-1e4: the maximum is subtracted
    rows["scaled_neg"], x[1] = 1, -np.abs(x[0]) - np.float32(1e4)
    rows["equal"], x[2] = 2, np.float32(-3.75)
    rows["peaked"] = 3
    x[3, C // 3] = 200.0                                                 # expf(-200 +- a few) is 0 in f32: the sum is exactly 1
    rows["ninf"] = 4
    x[4, 3:] = -np.inf                                                   # three finite logits, then -inf entries among the winners
    rows["tied"] = 5
    n_tied = min(C - 1, 300)                                             # more than TOPK_CAND = 256 at the maximum where C allows:
    tied_cols = np.sort(rng.permutation(C)[:n_tied])                     # the exact fallback scan
    x[5, tied_cols] = 9.0
    rows["plain"], rows["nan"] = 6, 7
    nan_col = C - 1
    finite = x[:7]
    order, p64, tol, torch_err = _reference(finite)
    x[7, nan_col] = np.nan
    view = _padded(x, float("nan"))
    for k in [k for k in (1, 5, 8, 9, 16) if k <= C]:
        conf, idx = ops.class_softmax_topk(view, C, k)
        again_conf, again_idx = ops.class_softmax_topk(view, C, k)
        assert torch.equal(conf.view(torch.int32), again_conf.view(torch.int32)) and torch.equal(idx, again_idx), "a second call differs"
        rel = _check(conf[:7], idx[:7], order, p64, tol, k, f"C={C} k={k} special rows")
        c, i = conf.cpu().numpy(), idx.cpu().numpy()
        assert i[rows["equal"]].tolist() == list(range(k))
        assert np.allclose(c[rows["equal"]], 1.0 / C, rtol=tol, atol=0)
        assert c[rows["peaked"], 0] == 1.0 and i[rows["peaked"], 0] == C // 3 and (c[rows["peaked"], 1:] == 0).all()
        assert (c[rows["ninf"], 3:] == 0).all() and i[rows["ninf"], 3:].tolist() == list(range(3, k))
        assert i[rows["tied"]].tolist() == tied_cols[:k].tolist()
        # a NaN logit: NaN confidences for that row only, indices inside [0, C) and distinct
        assert np.isnan(c[rows["nan"]]).all() and not np.isnan(c[:7]).any()
        assert ((i[rows["nan"]] >= 0) & (i[rows["nan"]] < C)).all() and len(set(i[rows["nan"]].tolist())) == k
    print(f"C={C} special rows: torch CPU f32 softmax vs f64 {torch_err:.3e}, tolerance {tol:.3e}, kernel vs f64 (k=16 or C) {rel:.3e}")


# ---- the protocol on the pinned reference outputs -------------------------------------------------------------------------------

def _rows(pred_list):
    """[{level: [name] * k}] -> the k label dicts of every query, flattened: a key table whose row q * k + r is slot r of query q"""
    return [{lv: p[lv][r] for lv in LEVELS} for p in pred_list for r in range(len(p["species"]))]


def test_gpu_path_equals_the_pinned_reference_outputs(capsys):
    """The fixture's class indices, confidences and class table go into ``MethodTwoSplit`` as they are; its DNA-search label lists
    become a key table (row q * k + r = slot r of query q, idx = arange)."""
    import method_two_fine_tuning_and_eval as M
    from bioscanclip.hip.method_two import (MethodTwoSplit, linspace_thresholds, member_share, merged_accuracy, merged_predictions,
                                            pick_threshold, sweep)
    from bioscanclip.hip.retrieval import Labels, encode_labels
    with open(os.path.join(ROOT, "tests", "golden", "method_two.json")) as f:
        gold = json.load(f)
    parts = list(gold["splits"].values())
    class_rows = [gold["idx_to_all_labels"][str(c)] for c in range(len(gold["idx_to_all_labels"]))]
    unseen_rows = [r for sp in parts for r in _rows(sp["pred_labels_from_b"])]
    arrays, vocab = encode_labels(class_rows, unseen_rows, *[sp["gt_labels"] for sp in parts], levels=LEVELS)
    class_table, unseen_ids = Labels(arrays[0]), Labels(arrays[1])
    splits, start = [], 0
    for sp, ids in zip(parts, arrays[2:]):
        conf = np.asarray(sp["pred_confidence_from_a"], dtype=np.float32)
        assert conf.astype(np.float64).tolist() == sp["pred_confidence_from_a"]
        class_idx = torch.tensor(sp["class_indices"], dtype=torch.int64, device="cuda")
        idx_b = torch.arange(start, start + conf.size, dtype=torch.int64, device="cuda").reshape(conf.shape)
        start += conf.size
        splits.append(MethodTwoSplit(torch.from_numpy(conf).cuda(), class_idx, class_table, idx_b, unseen_ids, ids, levels=LEVELS))
    by_int = lambda d: {int(k): v for k, v in d.items()}
    # the module's own functions, one by one
    thresholds = linspace_thresholds(gold["num_intervals"])
    counts, totals = sweep(splits, thresholds)
    best = pick_threshold(counts, totals, thresholds)
    assert best == gold["best_threshold"] and totals == [40, 40]
    member = np.asarray([int(name in gold["species_list"]) for name in vocab["species"]], dtype=np.int32)
    for split, sp in zip(splits, parts):
        acc, per_class = merged_accuracy(split, best, gold["k_list"], vocab)
        assert acc["micro_acc"] == by_int(sp["micro_acc"]) and acc["macro_acc"] == by_int(sp["macro_acc"])
        assert per_class == by_int(sp["per_class_acc"])
        shares = member_share(split, best, member)
        assert [f"for k = {k}: {shares[k]}" for k in (1, 3, 5)] == sp["membership_lines"]
        assert merged_predictions(split, best, class_rows, unseen_rows) == sp["final_pred_labels"]
    # and through the script
    args = _args(gold["k_list"], hip_eval="gpu")
    for with_predictions in (False, True):
        outs = M.score_splits_on_gpu(args, splits, [sp["gt_labels"] for sp in parts], vocab, class_rows, unseen_rows,
                                     with_predictions=with_predictions, num_intervals=gold["num_intervals"], grid=linspace_thresholds)
        for out, sp in zip(outs, parts):
            assert out["best_threshold"] == gold["best_threshold"]
            assert out["micro_acc"] == by_int(sp["micro_acc"]) and out["macro_acc"] == by_int(sp["macro_acc"])
            assert out["per_class_acc"] == by_int(sp["per_class_acc"]) and out["gt_labels"] == sp["gt_labels"]
            if with_predictions:
                assert out["final_pred_labels"] == sp["final_pred_labels"]
            else:
                assert out["final_pred_labels"] is None and out["merged"].split.A.is_cuda
            capsys.readouterr()
            M.check_for_acc_about_correct_predict_seen_or_unseen(out["merged"], gold["species_list"])
            assert capsys.readouterr().out.splitlines() == sp["membership_lines"]
        capsys.readouterr()
        M.print_acc_for_google_doc(*outs, K_LIST=gold["k_list"])
        assert capsys.readouterr().out.splitlines() == gold["google_doc_lines"]
    with pytest.raises(ValueError, match="class table"):
        MethodTwoSplit(torch.zeros(2, 5, device="cuda"), torch.zeros(2, 5, dtype=torch.int64, device="cuda"), arrays[0][:3],
                       torch.zeros(2, 5, dtype=torch.int64, device="cuda"), unseen_ids, arrays[2][:2])


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def _synthetic_model():
    from bioscanclip.model import arch, simple_clip
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from oracle import synth
    model = simple_clip.SimpleCLIP(LoRA_ViT_timm(arch.VisionTransformerParams(depth=2), r=4, num_classes=768),
                                   LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=2)), r=4,
                                                     num_classes=768), None)
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), 43))
    return model.to("cuda")


TABLE_KEYS = ("best_threshold", "micro_acc", "macro_acc", "per_class_acc", "gt_labels")


def test_fine_tune_then_gpu_path_equals_host_path(capsys):
    """One epoch of 2 training steps on a depth-2 model pair, then one evaluation batch of 40 per split: ``hip_eval=gpu`` equals
    ``hip_eval=host`` on the same models, the original model's features do not move, ``evaluate_epoch`` has its three keys."""
    import method_two_fine_tuning_and_eval as M
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.util.synthetic import SyntheticEvalLoader
    device = torch.device("cuda", torch.cuda.current_device())
    mk = lambda seed, bs=40, n=1: SyntheticEvalLoader(bs, n, with_text=False, seed=seed)
    train, seen_val, unseen_val, val_keys, test_keys = mk(7300, 8, 2), mk(7304), mk(7305), mk(7302), mk(7303)
    label_map, idx_to_all_labels = M.load_all_seen_species_name_and_create_label_map(train)
    C = len(label_map)
    assert C == 11 and list(label_map) == sorted(label_map)
    original, second = _synthetic_model(), _synthetic_model()
    second.load_state_dict(original.state_dict())
    original.eval()
    torch.manual_seed(5)
    classifier = M.ViTWIthExtraLayer(second.image_encoder, nn.Linear(768, C)).to(device)
    assert classifier.vit is not original.image_encoder
    for a, b in zip(original.image_encoder.state_dict().values(), classifier.vit.state_dict().values()):
        assert torch.equal(a, b)                                        # the copy starts from the original's parameters
    fixed = next(iter(seen_val))[1].to(device)
    classifier.eval()
    with torch.no_grad():
        before = original.image_encoder(fixed).clone()
        tuned_before = classifier.get_feature(fixed).clone()
    head_before = classifier.new_linear_layer.weight.detach().clone()
    classifier.train()
    optimizer = FusedAdamW([p for p in classifier.parameters() if p.requires_grad], lr=1e-3)
    args = _args([1, 3, 5], activate_wandb=False)
    loss, seen_result = M.fine_tuning_epoch(args, classifier, train, seen_val, unseen_val, optimizer, nn.CrossEntropyLoss(), device, label_map)
    assert np.isfinite(loss) and loss > 0
    assert sorted(seen_result) == ["top1_accuracy", "top3_accuracy", "top5_accuracy"]
    assert sorted(M.evaluate_epoch(classifier, unseen_val, device, label_map)) == ["top1_accuracy", "top3_accuracy", "top5_accuracy"]
    with torch.no_grad():
        after = original.image_encoder(fixed)
        tuned_after = classifier.get_feature(fixed)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32)), "fine-tuning moved the original model's image features"
    assert not torch.equal(tuned_before, tuned_after), "two training steps left the classifier's encoder where it was"
    assert not torch.equal(head_before, classifier.new_linear_layer.weight), "two training steps left the new Linear where it was"

    classifier.eval()
    run = lambda mode, **kw: M.method_2_inference_and_eval_for_seen_and_unseen(
        _args([1, 3, 5], hip_eval=mode), classifier, original, seen_val, unseen_val, val_keys, test_keys, label_map, idx_to_all_labels,
        device, **kw)
    host = run("host")
    gpu = run("gpu", with_predictions=True)
    lean = run("gpu")
    species_list = sorted({s for loader in (val_keys, test_keys) for s in M.get_all_unique_species_from_dataloader(loader)})[:6]
    for h, g, l in zip(host, gpu, lean):
        for key in TABLE_KEYS + ("final_pred_labels",):
            assert g[key] == h[key], key
        for key in TABLE_KEYS:
            assert l[key] == h[key], key
        assert l["final_pred_labels"] is None and len(h["final_pred_labels"]) == 40
        capsys.readouterr()
        host_share = M.check_for_acc_about_correct_predict_seen_or_unseen(h["final_pred_labels"], species_list)
        host_lines = capsys.readouterr().out
        gpu_share = M.check_for_acc_about_correct_predict_seen_or_unseen(l["merged"], species_list)
        assert capsys.readouterr().out == host_lines and gpu_share == host_share
    assert host[0]["best_threshold"] in np.linspace(0, 1, 1001).tolist()
    host_t, gpu_t = run("host", searched_threshold=0.123), run("gpu", searched_threshold=0.123)
    for h, g in zip(host_t, gpu_t):
        assert h["best_threshold"] == g["best_threshold"] == 0.123
        for key in TABLE_KEYS:
            assert g[key] == h[key], key


def test_method_two_script_main(monkeypatch, capsys):
    """``main`` on depth-2 synthetic models (``load_clip_model`` replaced): trains, evaluates val and test on the GPU path and
    prints the reference's rows."""
    import method_two_fine_tuning_and_eval as M
    from bioscanclip.model import simple_clip
    built = []

    def fake_load(args, device=None):
        built.append(_synthetic_model())
        return built[-1]
    monkeypatch.setattr(simple_clip, "load_clip_model", fake_load)
    capsys.readouterr()
    out = M.main(["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", "model_config.batch_size=8",
                  "synthetic_steps_per_epoch=2", "synthetic_eval_batches=1", "hip_eval=gpu"])
    text = capsys.readouterr().out
    assert len(built) == 2 and built[0] is not built[1]                 # the classifier's encoder is a second model
    assert len(out["history"]) == 1 and sorted(out["history"][0][1]) == ["top1_accuracy", "top3_accuracy", "top5_accuracy"]
    rows = [ln for ln in text.splitlines() if ln.startswith(" ")]
    assert len(rows) == 2 * 2 * 3 and all(len(r.split()) == 12 for r in rows)          # val + test, micro + macro, k = 1, 3, 5
    assert text.count("for k = ") == 12 and text.count("For unseen") == 2
    assert out["test"][0]["best_threshold"] == out["val"][0]["best_threshold"]
    for part in ("val", "test"):
        for o in out[part]:
            assert o["final_pred_labels"] is None and o["merged"].split.sim.is_cuda and len(o["gt_labels"]) == 40
