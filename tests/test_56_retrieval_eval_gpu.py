"""GPU-resident retrieval evaluation: the key index against the plain search, the hit-rank and class-count kernels against numpy
restatements, and `inference_and_print_result_gpu` / `hip_eval=gpu` against the host path.

Bar: equality.  The indexed search runs the kernels of `bsclip_topk_ip` on the same operands (`torch.equal` on scores and indices),
and everything after the scores is integer arithmetic, so the accuracy tables equal the host path's with `==` on the floats: no
tolerance and no near-tie exception anywhere in this file.
"""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import retrieval as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
LEVELS = ["order", "family", "genus", "species"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- the key index ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Q,K,D,k", [(300, 5000, 768, 5), (7, 1000, 768, 1), (1300, 2500, 768, 3), (64, 777, 1536, 16),
                                     (1, 5, 64, 5)])
def test_indexed_search_equals_plain_search(Q, K, D, k):
    from bioscanclip.hip import ops
    from bioscanclip.hip.retrieval import RetrievalIndex
    rng = np.random.RandomState(Q + K)
    q = rng.randn(Q, D).astype(np.float32) * 3.0
    keys = rng.randn(K, D).astype(np.float32) * 0.2
    keys[: min(Q, K) // 2] = q[: min(Q, K) // 2] * 0.5 + 0.3 * keys[: min(Q, K) // 2]  # a planted neighbour per query
    q2 = (rng.randn(Q, D) * 0.7 + 0.1).astype(np.float32)
    qd, q2d, kd = torch.from_numpy(q).cuda(), torch.from_numpy(q2).cuda(), torch.from_numpy(keys).cuda()
    index = RetrievalIndex(kd)
    before = index.index.clone()
    s1, i1 = index.search(qd, k)
    assert s1.is_cuda and i1.is_cuda and s1.dtype == torch.float32 and i1.dtype == torch.int64 and tuple(i1.shape) == (Q, k)
    s2, i2 = index.search(q2d, k)                  # a second query set against the same index
    s1b, i1b = index.search(qd, k)                 # the first again: the searches in between did not disturb the index
    assert torch.equal(index.index, before)
    ref_s, ref_i = ops.topk_ip(qd, kd, k)
    ref_s2, ref_i2 = ops.topk_ip(q2d, kd, k)
    assert torch.equal(s1, ref_s) and torch.equal(i1, ref_i)
    assert torch.equal(s2, ref_s2) and torch.equal(i2, ref_i2)
    assert torch.equal(s1b, s1) and torch.equal(i1b, i1)
    s_np, i_np = RetrievalIndex(keys).search(q, k)  # numpy in: uploaded once, same results
    assert torch.equal(s_np, ref_s) and torch.equal(i_np, ref_i)


def test_indexed_search_rejects_bad_arguments():
    from bioscanclip.hip import ops
    from bioscanclip.hip.retrieval import RetrievalIndex
    index = RetrievalIndex(torch.randn(30, 768, device="cuda"))
    q = torch.randn(4, 768, device="cuda")
    with pytest.raises(ValueError):
        index.search(q, 17)
    with pytest.raises(ValueError):
        RetrievalIndex(torch.randn(3, 768, device="cuda")).search(q, 5)   # k > K
    with pytest.raises(ValueError):
        index.search(torch.randn(4, 704, device="cuda"), 5)              # another D: not this index
    with pytest.raises(ValueError):
        ops.topk_ip_indexed(q, index.index, 300, 5)                      # a buffer too small for 300 keys
    with pytest.raises(ValueError):
        ops.retrieval_index_build(torch.randn(30, 768))                  # no CPU path


# ---- hit ranks -------------------------------------------------------------------------------------------------------------------

def _np_hit_ranks(idx, key_labels, query_labels):
    Q, k = idx.shape
    out = np.full(query_labels.shape, k, dtype=np.int32)
    for q in range(Q):
        for l in range(query_labels.shape[1]):
            for r in range(k):
                if key_labels[idx[q, r], l] == query_labels[q, l]:
                    out[q, l] = r
                    break
    return out


@pytest.mark.parametrize("k", [1, 3, 5, 16])
@pytest.mark.parametrize("L", [1, 4, 8])
def test_hit_ranks_equal_numpy(k, L):
    from bioscanclip.hip import ops
    rng = np.random.RandomState(100 * k + L)
    Q, K = 213, 97                                                     # Q not a multiple of the 16 queries per block
    key_labels = rng.randint(0, 6, size=(K, L)).astype(np.int32)       # few classes: duplicate labels among the top k
    query_labels = rng.randint(0, 6, size=(Q, L)).astype(np.int32)
    idx = rng.randint(0, K, size=(Q, k)).astype(np.int64)
    # query 0: its label appears only at the last rank, at every level; query 1: no match at all; query 2: every rank matches
    key_labels[0] = 50
    key_labels[1] = 51
    query_labels[0] = 50
    idx[0] = rng.randint(2, K, size=k)
    idx[0, k - 1] = 0
    query_labels[1] = 77
    query_labels[2] = 51
    idx[2] = 1
    idx[3] = K - 1                                                     # the last valid key
    ref = _np_hit_ranks(idx, key_labels, query_labels)
    assert (ref[0] == k - 1).all() and (ref[1] == k).all() and (ref[2] == 0).all()
    got = ops.retrieval_hit_ranks(torch.from_numpy(idx).cuda(), torch.from_numpy(key_labels).cuda(),
                                  torch.from_numpy(query_labels).cuda())
    assert got.dtype == torch.int32 and (got.cpu().numpy() == ref).all()


def test_hit_ranks_refuse_an_index_outside_the_keys():
    """idx == K (and a negative one) is flagged and not dereferenced: the key labels end exactly at K rows, and the entries of
    the other queries are still right."""
    from bioscanclip.hip import ops
    rng = np.random.RandomState(8)
    Q, K, k, L = 40, 33, 5, 4
    key_labels = rng.randint(0, 4, size=(K, L)).astype(np.int32)
    query_labels = rng.randint(0, 4, size=(Q, L)).astype(np.int32)
    idx = rng.randint(0, K, size=(Q, k)).astype(np.int64)
    kd, qd = torch.from_numpy(key_labels).cuda(), torch.from_numpy(query_labels).cuda()
    for bad in (K, -1, 2 ** 40):
        broken = idx.copy()
        broken[17, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.retrieval_hit_ranks(torch.from_numpy(broken).cuda(), kd, qd)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")       # caller-owned flag: no raise here, the word carries the error
        got = ops.retrieval_hit_ranks(torch.from_numpy(broken).cuda(), kd, qd, flag=flag).cpu().numpy()
        assert flag.item() & 1
        keep = np.arange(Q) != 17
        assert (got[keep] == _np_hit_ranks(idx, key_labels, query_labels)[keep]).all()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.retrieval_hit_ranks(torch.from_numpy(idx).cuda(), kd, qd, flag=flag)
    assert flag.item() == 0


# ---- class counts ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Q,sizes,k_list", [(5000, [7, 300, 20000, 20000], [1, 3, 5]), (777, [1], [2]),
                                            (16384, [3, 40, 900, 20000, 5, 5, 5, 5], [1, 2, 3, 4, 5, 8, 12, 16])])
def test_class_counts_equal_bincount(Q, sizes, k_list):
    from bioscanclip.hip import ops
    rng = np.random.RandomState(Q)
    L, nk = len(sizes), len(k_list)
    # labels drawn from the lower two thirds of each range (and the very last id once): many classes have no query
    query_labels = np.stack([rng.randint(0, max(1, 2 * n // 3), size=Q) for n in sizes], axis=1).astype(np.int32)
    query_labels[0] = np.asarray(sizes) - 1
    hit_rank = rng.randint(0, 17, size=(Q, L)).astype(np.int32)
    offsets = [0] + np.cumsum(sizes).tolist()
    C = offsets[-1]
    flat = query_labels + np.asarray(offsets[:-1])[None]
    ref_seen = np.bincount(flat.ravel(), minlength=C)
    ref_right = np.stack([np.bincount(flat[hit_rank < kk], minlength=C) for kk in k_list])
    assert (ref_seen == 0).sum() > 0 or C == 1
    hd, qd = torch.from_numpy(hit_rank).cuda(), torch.from_numpy(query_labels).cuda()
    seen, right = ops.retrieval_class_counts(hd, qd, offsets, k_list)
    assert seen.dtype == torch.int32 and tuple(seen.shape) == (C,) and tuple(right.shape) == (nk, C)
    assert (seen.cpu().numpy() == ref_seen).all() and (right.cpu().numpy() == ref_right).all()
    out = torch.full(((1 + nk) * C,), 123, dtype=torch.int32, device="cuda")   # the entry point clears its outputs
    seen2, right2 = ops.retrieval_class_counts(hd, qd, offsets, k_list, out=out)
    assert torch.equal(seen2, seen) and torch.equal(right2, right)


def test_class_counts_refuse_a_label_outside_its_level():
    from bioscanclip.hip import ops
    hit_rank = torch.zeros(10, 2, dtype=torch.int32, device="cuda")
    labels = torch.zeros(10, 2, dtype=torch.int32, device="cuda")
    labels[4, 0] = 3                                                   # level 0 has 3 classes: ids 0..2
    with pytest.raises(ValueError, match="outside"):
        ops.retrieval_class_counts(hit_rank, labels, [0, 3, 5], [1])
    labels[4, 0] = -1
    with pytest.raises(ValueError, match="outside"):
        ops.retrieval_class_counts(hit_rank, labels, [0, 3, 5], [1])


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def _host_and_gpu(keys_dict, seen_dict, unseen_dict, k_list, capsys):
    import inference_and_eval as host
    capsys.readouterr()
    ref = host.inference_and_print_result(keys_dict, seen_dict, unseen_dict, k_list=k_list)
    ref_out = capsys.readouterr().out
    got = host.inference_and_print_result_gpu(keys_dict, seen_dict, unseen_dict, k_list=k_list)
    got_out = capsys.readouterr().out
    with_pred = host.inference_and_print_result_gpu(keys_dict, seen_dict, unseen_dict, k_list=k_list, with_predictions=True)
    pred_out = capsys.readouterr().out
    assert got[0] == ref[0] and got[1] == ref[1]                       # acc_dict, per_class_acc: == on the nested dicts
    assert with_pred[0] == ref[0] and with_pred[1] == ref[1] and with_pred[2] == ref[2]
    assert got_out == ref_out and pred_out == ref_out and "micro_acc top-1" in ref_out
    return ref, got


def _split(rng, n, label_of, centres, with_all=False, noise=0.6):
    labels = [label_of(i) for i in range(n)]
    pick = np.asarray([int(lab["species"][1:]) for lab in labels])
    feats = {m: centres[m][pick] + noise * rng.randn(n, centres[m].shape[1]) for m in ("image", "dna", "lang")}
    split = {"file_name_list": [f"s{i}" for i in range(n)], "label_list": labels,
             "encoded_image_feature": feats["image"], "encoded_dna_feature": feats["dna"], "encoded_language_feature": feats["lang"],
             "averaged_feature": np.mean([feats["image"], feats["dna"]], axis=0),
             "concatenated_feature": np.concatenate((feats["image"], feats["dna"]), axis=1),
             "all_key_features": None, "all_key_features_label": None}
    if with_all:
        split["all_key_features"] = np.concatenate((feats["image"], feats["dna"], feats["lang"]), axis=0)
        split["all_key_features_label"] = labels + labels + labels
    return split


def test_eval_gpu_equals_host_on_three_synthetic_splits(capsys):
    """96 keys, 2 x 48 queries, all five feature types and the all-keys set.  Species repeat; the unseen species are absent from
    the keys and every query's family is named differently from every key's, so one level is wrong for every query."""
    rng = np.random.RandomState(21)
    centres = {m: rng.randn(24, 128) for m in ("image", "dna", "lang")}

    def key_label(i):
        sp = i % 12
        return {"order": f"o{sp % 2}", "family": f"f{sp % 4}", "genus": f"g{sp % 6}", "species": f"s{sp}"}

    def seen_label(i):
        return dict(key_label(i * 5 % 12), family=f"F{i % 3}")

    def unseen_label(i):
        sp = 12 + i % 9
        return {"order": f"o{sp % 2}", "family": f"F{sp % 4}", "genus": "not_classified" if i % 7 == 0 else f"g{sp % 6}",
                "species": f"s{sp}"}

    keys = _split(rng, 96, key_label, centres, with_all=True)
    keys["label_list"][5] = dict(keys["label_list"][5], genus="not_classified")   # matches the unseen queries' "not_classified"
    keys["all_key_features_label"] = keys["label_list"] * 3
    seen, unseen = _split(rng, 48, seen_label, centres), _split(rng, 48, unseen_label, centres)
    ref, got = _host_and_gpu(keys, seen, unseen, [1, 3, 5], capsys)
    acc = ref[0]
    assert sum(bool(acc[q][kf]) for q in acc for kf in acc[q]) == 4 * 5 + 1      # 768-d style cells + concatenated x concatenated
    cell = acc["encoded_image_feature"]["encoded_image_feature"]
    assert cell["seen"]["micro_acc"][5]["family"] == 0.0 and cell["seen"]["micro_acc"][1]["species"] > 0.5
    assert cell["unseen"]["micro_acc"][5]["species"] == 0.0
    idx = got[2]["encoded_dna_feature"]["all_key_features"]["curr_seen_indices"]
    assert idx.is_cuda and idx.dtype == torch.int64 and tuple(idx.shape) == (48, 5)
    # a k_list whose last entry is not its largest: the search depth is k_list[-1], like the host path
    _host_and_gpu(keys, seen, unseen, [5, 1, 3], capsys)


def test_eval_gpu_equals_host_on_the_golden_case(capsys):
    """The labels of tests/golden/retrieval.json (as test_55 and test_01 use them) with features around per-species centres."""
    with open(os.path.join(ROOT, "tests", "golden", "retrieval.json")) as f:
        gold = json.load(f)
    keys_label, gt_list, _, _ = R.retrieval_case(**gold["case"])
    rng = np.random.RandomState(1)
    centre = rng.randn(11, 768)
    feat = lambda labels: centre[[int(lab["species"][1:]) for lab in labels]] + 0.8 * rng.randn(len(labels), 768)
    keys = {"label_list": keys_label, "encoded_image_feature": feat(keys_label), "encoded_dna_feature": feat(keys_label)}
    seen = {"label_list": gt_list, "encoded_image_feature": feat(gt_list), "encoded_dna_feature": feat(gt_list)}
    unseen = {"label_list": gt_list[::-1], "encoded_image_feature": feat(gt_list[::-1]), "encoded_dna_feature": None}
    ref, _ = _host_and_gpu(keys, seen, unseen, gold["k_list"], capsys)
    assert ref[0]["encoded_image_feature"]["encoded_dna_feature"]["seen"]["micro_acc"][1]["species"] > 0.3
    assert ref[0]["encoded_dna_feature"]["encoded_image_feature"] == {}          # no unseen DNA queries: the cell is skipped
    # and the evaluation of one cell through the module's own interface, on the fixture's index lists
    from bioscanclip.hip.retrieval import RetrievalIndex, encode_labels, evaluate
    (key_ids, query_ids), vocab = encode_labels(keys_label, gt_list)
    acc, per_class = evaluate(RetrievalIndex(keys["encoded_image_feature"]), key_ids, seen["encoded_image_feature"], query_ids,
                              gold["k_list"], vocab=vocab)
    assert acc == ref[0]["encoded_image_feature"]["encoded_image_feature"]["seen"]
    assert per_class == ref[1]["encoded_image_feature"]["encoded_image_feature"]["seen"]


# ---- the scripts -----------------------------------------------------------------------------------------------------------------

def test_inference_and_eval_script_hip_eval_gpu(tmp_path, capsys):
    import inference_and_eval
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", f"project_root_path={tmp_path}",
              "debug_flag=false", "synthetic_eval_batches=1"]
    ref = inference_and_eval.main(common + ["save_inference=true"])            # the default: the host path
    ref_out = capsys.readouterr().out
    table = lambda out: [ln for ln in out.splitlines() if ln.startswith("Query_feature")]
    host_again = inference_and_eval.main(common + ["load_inference=true", "hip_eval=host"])
    assert table(capsys.readouterr().out) == table(ref_out)
    got = inference_and_eval.main(common + ["load_inference=true", "hip_eval=gpu"])   # the same features, scored on the GPU
    got_out = capsys.readouterr().out
    assert table(got_out) == table(ref_out) and len(table(ref_out)) > 0
    assert got[0] == ref[0] == host_again[0] and got[1] == ref[1]
    with pytest.raises(ValueError, match="hip_eval"):
        inference_and_eval.main(common + ["hip_eval=banana"])


def test_eval_phase_hip_eval_gpu(capsys):
    from bioscanclip.model import arch
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from bioscanclip.model.simple_clip import SimpleCLIP
    from bioscanclip.util.synthetic import SyntheticEvalLoader
    from oracle import synth
    import train_cl
    model = SimpleCLIP(LoRA_ViT_timm(arch.VisionTransformerParams(depth=2), r=4, num_classes=768),
                       LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=2)), r=4,
                                         num_classes=768), None)
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), 43))
    model.to("cuda")
    loaders = [SyntheticEvalLoader(8, 2, with_text=False, seed=s) for s in (11, 12, 13)]
    ref_acc, ref_pred = train_cl.eval_phase(model, "cuda", *loaders, [1, 3, 5], types.SimpleNamespace())
    ref_out = capsys.readouterr().out
    got_acc, got_pred = train_cl.eval_phase(model, "cuda", *loaders, [1, 3, 5], types.SimpleNamespace(hip_eval="gpu"))
    got_out = capsys.readouterr().out
    assert got_acc == ref_acc and got_out == ref_out and "macro_acc top-5" in ref_out
    assert "curr_seen_pred_list" in ref_pred["encoded_image_feature"]["encoded_dna_feature"]
    assert "curr_seen_indices" in got_pred["encoded_image_feature"]["encoded_dna_feature"]
    with pytest.raises(ValueError, match="hip_eval"):
        train_cl.eval_phase(model, "cuda", *loaders, [1, 3, 5], types.SimpleNamespace(hip_eval="banana"))
