"""Method-one evaluation on the GPU: the mask, merge and sweep kernels against numpy restatements, the GPU path against the pinned
reference outputs (tests/golden/method_one.json) and against the host path of the same script.

Bar: equality.  The kernels produce integers; the selection compares in float64 like the host path's Python floats; the ratios are
formed on the host in the reference's order.  So every comparison in this file is ``==`` / ``torch.equal``: no tolerance anywhere.
"""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
LEVELS = ["order", "family", "genus", "species"]
K_KEYS = 37


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _args(k_list, **kw):
    return types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=list(k_list)), **kw)


# ---- numpy restatements ----------------------------------------------------------------------------------------------------------

def np_match_bits(idx, key_labels, query_labels):
    k = idx.shape[1]
    eq = key_labels[idx] == query_labels[:, None, :]                      # [Q, k, L]
    return (eq.astype(np.int64) << np.arange(k)[None, :, None]).sum(axis=1).astype(np.int32)


def np_member_bits(idx, key_labels, member, level):
    k = idx.shape[1]
    on = member[key_labels[idx, level]] != 0                              # [Q, k]
    return (on.astype(np.int64) << np.arange(k)[None, :]).sum(axis=1).astype(np.int32)


def np_ctz(m, k):
    """lowest set bit below k, or k"""
    m = m.astype(np.int64) & ((1 << k) - 1)
    low = m & -m
    return np.where(m == 0, k, np.round(np.log2(np.maximum(low, 1)))).astype(np.int32)


def np_merge(sim, A, B, thr, k):
    """hit ranks [T, Q, L] at every threshold: float64 strict compare, NaN selects B"""
    with np.errstate(invalid="ignore"):
        sel = sim.astype(np.float64)[None, :, :] > np.asarray(thr, dtype=np.float64)[:, None, None]     # [T, Q, k]
    s = (sel.astype(np.int64) << np.arange(k)[None, None, :]).sum(axis=2)                                # [T, Q]
    A, B = A.astype(np.int64)[None], B.astype(np.int64)[None]
    return np_ctz((A & s[:, :, None]) | (B & ~s[:, :, None]), k)


def _case(Q, k, L, seed):
    rng = np.random.RandomState(seed)
    key_labels = rng.randint(0, 5, size=(K_KEYS, L)).astype(np.int32)
    query_labels = rng.randint(0, 5, size=(Q, L)).astype(np.int32)
    idx_a = rng.randint(0, K_KEYS, size=(Q, k)).astype(np.int64)
    idx_b = rng.randint(0, K_KEYS, size=(Q, k)).astype(np.int64)
    idx_a[-1] = K_KEYS - 1                                                 # the last valid key
    sim = rng.uniform(-0.3, 1.3, size=(Q, k)).astype(np.float32)           # unsorted rows, below 0 and above 1
    sim[rng.randint(0, Q), rng.randint(0, k)] = np.nan
    sim[0, 0] = np.float32(0.3)                                            # 0.3f = 0.300000011920929 as a double
    if Q > 2:
        sim[1] = np.float32(0.5)                                           # a whole row on one threshold
        sim[2, 0] = np.nan
    return key_labels, query_labels, idx_a, idx_b, sim


def _thresholds(sim, T, rng):
    x = float(np.float64(sim[0, 0]))                                       # the exact float64 value of an f32 similarity
    special = [x, float(np.nextafter(x, -np.inf)), float(np.nextafter(x, np.inf)), 0.5, 0.0, 1.0, -0.25]
    if T == 1:
        return np.asarray([special[1]])
    if T == 7:
        return np.asarray(special)
    thr = np.linspace(0, 1, T)
    rng.shuffle(thr)                                                       # any order
    thr[[3, T // 2, T - 1, 17, 200, 511, 640]] = special
    return thr


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("Q", [1, 67, 300])
def test_mask_merge_and_sweep_kernels_equal_numpy(Q, k, L):
    from bioscanclip.hip import ops
    rng = np.random.RandomState(1000 * Q + 10 * k + L)
    key_labels, query_labels, idx_a, idx_b, sim = _case(Q, k, L, 7 * Q + k + L)
    dev = lambda x: torch.from_numpy(x).cuda()
    kd, qd, simd = dev(key_labels), dev(query_labels), dev(sim)
    # match_bits: the numpy masks, no bit at or above k, and ctz = the hit ranks of the existing kernel on the same inputs
    A_ref, B_ref = np_match_bits(idx_a, key_labels, query_labels), np_match_bits(idx_b, key_labels, query_labels)
    A, B = ops.retrieval_match_bits(dev(idx_a), kd, qd), ops.retrieval_match_bits(dev(idx_b), kd, qd)
    assert A.dtype == torch.int32 and tuple(A.shape) == (Q, L)
    assert (A.cpu().numpy() == A_ref).all() and (B.cpu().numpy() == B_ref).all()
    assert (A.cpu().numpy() >> k == 0).all()
    hr = ops.retrieval_hit_ranks(dev(idx_a), kd, qd).cpu().numpy()
    assert (np_ctz(A.cpu().numpy(), k) == hr).all()
    zero = torch.zeros_like(A)
    for T in (1, 7, 1000):
        thr = _thresholds(sim, T, rng)
        thrd = dev(thr)
        level, k_primes = (L - 1) if T != 7 else 0, (1, 3, k + 2)
        for name, (a, b, a_ref, b_ref) in {"A,B": (A, B, A_ref, B_ref), "A=B": (A, A, A_ref, A_ref),
                                           "A=0": (zero, B, np.zeros_like(A_ref), B_ref)}.items():
            ref = np_merge(sim, a_ref, b_ref, thr, k)                      # [T, Q, L]
            probe = list(range(T)) if T <= 7 else [3, T // 2, T - 1, 17, 200, 511, 640, 0, 1]
            gpu_hits = {}
            for j in (range(T) if name == "A,B" else probe):
                got = ops.retrieval_merge_hit_ranks(simd, a, b, float(thr[j]))
                gpu_hits[j] = got
                assert (got.cpu().numpy() == ref[j]).all(), (name, T, j)
            for kp in k_primes:
                counts = ops.retrieval_threshold_sweep(simd, a, b, level, kp, thrd)
                again = ops.retrieval_threshold_sweep(simd, a, b, level, kp, thrd)
                assert torch.equal(counts, again)                          # two runs are bit-identical
                c = counts.cpu().numpy()
                assert c.dtype == np.int32 and c.shape == (T,)
                assert (c == (ref[:, :, level] < kp).sum(axis=1)).all(), (name, T, kp)
                derived = [int((h[:, level] < kp).sum()) for h in gpu_hits.values()]   # from merge_hit_ranks at thr[j]
                assert [int(c[j]) for j in gpu_hits] == derived, (name, T, kp)
            # the sweep adds to the caller's buffer
            out = torch.full((T,), 5, dtype=torch.int32, device="cuda")
            ops.retrieval_threshold_sweep(simd, a, b, level, 1, thrd, out=out)
            assert (out.cpu().numpy() - 5 == (ref[:, :, level] < 1).sum(axis=1)).all()


def test_selection_compares_in_float64():
    """One query, slot 0: the seen-key hit is right, the unseen-key hit is wrong.  At the float64 just below the f32 similarity the
    seen-key prediction is selected (a hit); at its exact float64 value it is not (strict).  In f32 both thresholds round to the
    similarity itself and the two cases could not differ."""
    from bioscanclip.hip import ops
    for value in (0.3, 0.7, 1e-3, -0.2, 1.0 + 2 ** -23):
        s32 = np.float32(value)
        x = float(np.float64(s32))
        below = float(np.nextafter(x, -np.inf))
        assert np.float32(below) == s32 and below < x
        sim = torch.tensor([[s32, 0.0]], dtype=torch.float32, device="cuda")
        A = torch.tensor([[1]], dtype=torch.int32, device="cuda")
        B = torch.tensor([[0]], dtype=torch.int32, device="cuda")
        assert ops.retrieval_merge_hit_ranks(sim, A, B, below).item() == 0
        assert ops.retrieval_merge_hit_ranks(sim, A, B, x).item() == 2
        thr = torch.tensor([below, x, float(np.nextafter(x, np.inf))], dtype=torch.float64, device="cuda")
        assert ops.retrieval_threshold_sweep(sim, A, B, 0, 1, thr).cpu().tolist() == [1, 0, 0]
        assert ops.retrieval_threshold_sweep(sim, B, A, 0, 1, thr).cpu().tolist() == [0, 1, 1]
    nan = torch.tensor([[float("nan"), float("nan")]], dtype=torch.float32, device="cuda")
    thr = torch.tensor([-1e30, 0.0, 1e30], dtype=torch.float64, device="cuda")
    assert ops.retrieval_threshold_sweep(nan, A, B, 0, 2, thr).cpu().tolist() == [0, 0, 0]       # a NaN always takes B
    assert ops.retrieval_threshold_sweep(nan, B, A, 0, 2, thr).cpu().tolist() == [1, 1, 1]


def test_match_bits_refuse_an_index_outside_the_keys():
    """idx == K (and a negative one) is flagged and not dereferenced: the key labels end exactly at K rows, and the other queries'
    masks are still right."""
    from bioscanclip.hip import ops
    key_labels, query_labels, idx, _, _ = _case(40, 5, 4, 3)
    kd, qd = torch.from_numpy(key_labels).cuda(), torch.from_numpy(query_labels).cuda()
    ref = np_match_bits(idx, key_labels, query_labels)
    for bad in (K_KEYS, -1, 2 ** 40):
        broken = idx.copy()
        broken[17, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.retrieval_match_bits(torch.from_numpy(broken).cuda(), kd, qd)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = ops.retrieval_match_bits(torch.from_numpy(broken).cuda(), kd, qd, flag=flag).cpu().numpy()
        assert flag.item() & 1
        keep = np.arange(40) != 17
        assert (got[keep] == ref[keep]).all()
        assert (got[17] == (ref[17] & ~(1 << 2))).all()                   # the bad slot's bit is zero, the row's other bits stand
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.retrieval_match_bits(torch.from_numpy(idx).cuda(), kd, qd, flag=flag)
    assert flag.item() == 0


def _hit_ranks_and_bits(Q, k, L, K, bad=None):
    """Both entry points on the same idx / key labels / query labels (6 classes, so ranks repeat), each with a caller-owned flag:
    (hit_rank [Q, L], bits [Q, L], the two flag words)."""
    from bioscanclip.hip import ops
    rng = np.random.RandomState(10000 * Q + 100 * k + L)
    key_labels = rng.randint(0, 6, size=(K, L)).astype(np.int32)          # exactly K rows: nothing to read at row K
    query_labels = rng.randint(0, 6, size=(Q, L)).astype(np.int32)
    idx = rng.randint(0, K, size=(Q, k)).astype(np.int64)
    if bad is not None:
        idx[bad] = K
    idx_d, kd, qd = torch.from_numpy(idx).cuda(), torch.from_numpy(key_labels).cuda(), torch.from_numpy(query_labels).cuda()
    flags = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
    hit_rank = ops.retrieval_hit_ranks(idx_d, kd, qd, flag=flags[0])
    bits = ops.retrieval_match_bits(idx_d, kd, qd, flag=flags[1])
    return hit_rank.cpu().numpy(), bits.cpu().numpy(), [f.item() for f in flags]


@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("Q", [1, 17, 213])    # one lane group; one past the 16 queries of a block; the size test_56 uses
def test_hit_ranks_equal_the_lowest_set_bit_of_match_bits(Q, k, L):
    """The two kernels share their opening (lane roles, idx bounds rule, label gather, per-level ballot): what one stores as a mask
    the other stores as its lowest set bit, or k where the mask is 0."""
    hit_rank, bits, flags = _hit_ranks_and_bits(Q, k, L, K=97)
    assert flags == [0, 0]
    assert hit_rank.shape == bits.shape == (Q, L)
    assert (bits >> k == 0).all()                                          # no bit at or above k, which np_ctz would not see
    assert (hit_rank == np_ctz(bits, k)).all()


def test_hit_ranks_and_match_bits_flag_the_same_bad_index():
    """An idx entry equal to K sets bit 1 of both callers' flags and is not dereferenced; every other query still agrees."""
    Q, k = 213, 5
    hit_rank, bits, flags = _hit_ranks_and_bits(Q, k, 8, K=97, bad=(100, 3))
    assert flags == [1, 1]
    keep = np.arange(Q) != 100
    assert (bits >> k == 0).all()
    assert (hit_rank[keep] == np_ctz(bits[keep], k)).all()


@pytest.mark.parametrize("Q,k,L", [(1, 1, 1), (67, 5, 4), (300, 16, 4)])
def test_member_masks_equal_numpy(Q, k, L):
    from bioscanclip.hip import ops
    key_labels, _, idx, _, _ = _case(Q, k, L, 11 + Q)
    kd, idxd = torch.from_numpy(key_labels).cuda(), torch.from_numpy(idx).cuda()
    member = np.asarray([1, 0, 0, 1, 0], dtype=np.int32)                  # labels are 0..4
    for level in range(L):
        got = ops.retrieval_match_bits(idxd, kd, member=torch.from_numpy(member).cuda(), level=level)
        assert tuple(got.shape) == (Q,) and (got.cpu().numpy() == np_member_bits(idx, key_labels, member, level)).all()
    # a table that ends before the largest label: flagged, not read, and the bit stays zero
    short = member[:4].copy()
    if (key_labels[idx, 0] == 4).any():
        with pytest.raises(ValueError, match="outside"):
            ops.retrieval_match_bits(idxd, kd, member=torch.from_numpy(short).cuda(), level=0)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = ops.retrieval_match_bits(idxd, kd, member=torch.from_numpy(short).cuda(), level=0, flag=flag).cpu().numpy()
        assert flag.item() == 2
        assert (got == np_member_bits(idx, key_labels, member * (np.arange(5) < 4), 0)).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------------

def _rows(pred_list):
    """[{level: [name] * k}] -> the k label dicts of every query, flattened: a key table whose row q * k + r is slot r of query q"""
    return [{lv: p[lv][r] for lv in LEVELS} for p in pred_list for r in range(len(p["species"]))]


def test_gpu_path_equals_the_pinned_reference_outputs(capsys):
    """The fixture's prediction lists become key tables (row q * k + r = slot r of query q, idx = arange), its similarities the f32
    ``sim``: from there on the GPU path runs as it does behind the searches."""
    import method_one_eval as M
    from bioscanclip.hip.method_one import MethodOneSplit
    from bioscanclip.hip.retrieval import Labels, encode_labels
    with open(os.path.join(ROOT, "tests", "golden", "method_one.json")) as f:
        gold = json.load(f)
    parts = list(gold["splits"].values())
    seen_rows = [r for sp in parts for r in _rows(sp["pred_labels_from_search_with_seen_keys"])]
    unseen_rows = [r for sp in parts for r in _rows(sp["pred_labels_from_search_with_unseen_keys"])]
    arrays, vocab = encode_labels(seen_rows, unseen_rows, *[sp["gt_label"] for sp in parts], levels=LEVELS)
    seen_ids, unseen_ids = Labels(arrays[0]), Labels(arrays[1])
    splits, start = [], 0
    for sp, ids in zip(parts, arrays[2:]):
        sim = np.asarray(sp["pred_similarity_from_search_with_seen_keys"], dtype=np.float32)
        assert sim.astype(np.float64).tolist() == sp["pred_similarity_from_search_with_seen_keys"]
        idx = torch.arange(start, start + sim.size, dtype=torch.int64, device="cuda").reshape(sim.shape)
        start += sim.size
        splits.append(MethodOneSplit(torch.from_numpy(sim).cuda(), idx, seen_ids, idx.clone(), unseen_ids, ids, levels=LEVELS))
    args = _args(gold["k_list"], hip_eval="gpu")
    by_int = lambda d: {int(k): v for k, v in d.items()}
    for with_predictions in (False, True):
        outs = M.score_splits_on_gpu(args, splits, [sp["gt_label"] for sp in parts], vocab, seen_rows, unseen_rows,
                                     with_predictions=with_predictions, num_intervals=gold["num_intervals"])
        for out, sp in zip(outs, parts):
            assert out["best_threshold"] == gold["best_threshold"]
            assert out["micro_acc"] == by_int(sp["micro_acc"]) and out["macro_acc"] == by_int(sp["macro_acc"])
            assert out["per_class_acc"] == by_int(sp["per_class_acc"]) and out["gt_labels"] == sp["gt_label"]
            if with_predictions:
                assert out["final_pred_labels"] == sp["final_pred_labels"]
            else:
                assert out["final_pred_labels"] is None and out["merged"].split.A.is_cuda
            capsys.readouterr()
            M.check_for_acc_about_correct_predict_seen_or_unseen(out["merged"], gold["species_list"])
            assert capsys.readouterr().out.splitlines() == sp["membership_lines"]
    with pytest.raises(KeyError):
        M.score_splits_on_gpu(_args([3, 5]), splits, [sp["gt_label"] for sp in parts], vocab, seen_rows, unseen_rows)


def _random_sets(seed, n_species=60, D=768, K=700):
    rng = np.random.RandomState(seed)
    centres = {m: rng.randn(n_species, D) for m in ("image", "dna")}
    lab = lambda s: {"order": f"o{s % 3}", "family": f"f{s % 7}", "genus": f"g{s % 19}", "species": f"s{s}"}
    seen_sp = rng.randint(0, 40, size=K)                                   # species 0..39 among the seen keys, 35..59 the unseen
    unseen_sp = rng.randint(35, n_species, size=K)
    seen_keys = centres["image"][seen_sp] + 0.9 * rng.randn(K, D)
    unseen_keys = centres["dna"][unseen_sp] + 0.9 * rng.randn(K, D)
    queries = []
    for Q, lo, hi in ((300, 0, 40), (513, 35, n_species)):
        sp = rng.randint(lo, hi, size=Q)
        # the image query leans towards its species' DNA centre too, so that the image-to-DNA search finds it
        queries.append((centres["image"][sp] + 0.6 * centres["dna"][sp] + 1.1 * rng.randn(Q, D), [lab(s) for s in sp.tolist()]))
    return seen_keys, [lab(s) for s in seen_sp.tolist()], unseen_keys, [lab(s) for s in unseen_sp.tolist()], queries


@pytest.mark.parametrize("seed", [3, 4])
def test_gpu_path_equals_host_path_on_random_sets(seed, capsys):
    """Q = 300 and 513 (the two splits), K = 700 keys per index, 768-d, the full grid of 1 000 thresholds on both paths."""
    import method_one_eval as M
    seen_keys, seen_key_labels, unseen_keys, unseen_key_labels, queries = _random_sets(seed)
    k_list, n = [1, 3, 5], 1000
    host_in = []
    for feats, gt in queries:
        pred_a, sim = M.make_prediction(feats, seen_keys, seen_key_labels, with_similarity=True, max_k=5)
        pred_b = M.make_prediction(feats, unseen_keys, unseen_key_labels, max_k=5)
        host_in.append((pred_a, sim.tolist(), pred_b, gt))
    ref = M.score_predictions_on_host(_args(k_list), *host_in, num_intervals=n)
    got = M.score_features_on_gpu(_args(k_list, hip_eval="gpu"), seen_keys, seen_key_labels, unseen_keys, unseen_key_labels, queries,
                                  with_predictions=True, num_intervals=n)
    lean = M.score_features_on_gpu(_args(k_list, hip_eval="gpu"), seen_keys, seen_key_labels, unseen_keys, unseen_key_labels, queries,
                                   num_intervals=n)
    assert 0 < ref[0]["best_threshold"] < 1 and ref[0]["micro_acc"][1]["species"] > 0.2 and ref[1]["micro_acc"][1]["species"] > 0.2
    species_list = sorted({lab["species"] for lab in unseen_key_labels})
    for r, g, l in zip(ref, got, lean):
        for key in ("best_threshold", "micro_acc", "macro_acc", "per_class_acc", "gt_labels", "final_pred_labels"):
            assert g[key] == r[key], key
        for key in ("best_threshold", "micro_acc", "macro_acc", "per_class_acc", "gt_labels"):
            assert l[key] == r[key], key
        assert l["final_pred_labels"] is None
        capsys.readouterr()
        host_share = M.check_for_acc_about_correct_predict_seen_or_unseen(r["final_pred_labels"], species_list)
        host_lines = capsys.readouterr().out
        gpu_share = M.check_for_acc_about_correct_predict_seen_or_unseen(l["merged"], species_list)
        assert capsys.readouterr().out == host_lines and gpu_share == host_share
    # a threshold handed in is used as it is, on both paths
    ref_t = M.score_predictions_on_host(_args(k_list), *host_in, searched_threshold=0.123)
    got_t = M.score_features_on_gpu(_args(k_list, hip_eval="gpu"), seen_keys, seen_key_labels, unseen_keys, unseen_key_labels, queries,
                                    searched_threshold=0.123)
    for r, g in zip(ref_t, got_t):
        assert g["best_threshold"] == r["best_threshold"] == 0.123 and g["micro_acc"] == r["micro_acc"] and g["macro_acc"] == r["macro_acc"]


def test_method_one_eval_script(monkeypatch, capsys):
    """``main`` on a depth-2 synthetic model (``load_clip_model`` replaced by one): ``hip_eval=gpu`` prints the rows ``hip_eval=host``
    prints, and returns the same tables."""
    import method_one_eval as M
    from bioscanclip.model import arch, simple_clip
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from oracle import synth
    model = simple_clip.SimpleCLIP(LoRA_ViT_timm(arch.VisionTransformerParams(depth=2), r=4, num_classes=768),
                                   LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=2)), r=4,
                                                     num_classes=768), None)
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), 43))
    model.to("cuda")
    monkeypatch.setattr(simple_clip, "load_clip_model", lambda args, device=None: model)
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", "synthetic_eval_batches=1"]
    capsys.readouterr()
    ref = M.main(common)                                                   # the default: the host path
    ref_out = capsys.readouterr().out
    got = M.main(common + ["hip_eval=gpu"])
    got_out = capsys.readouterr().out
    assert got_out == ref_out
    rows = [ln for ln in ref_out.splitlines() if ln.startswith(" ")]
    assert len(rows) == 2 * 2 * 3 and all(len(r.split()) == 12 for r in rows)          # val + test, micro + macro, k = 1, 3, 5
    assert ref_out.count("for k = ") == 12 and ref_out.count("For unseen") == 2
    for part in ("val", "test"):
        for r, g in zip(ref[part], got[part]):
            for key in ("best_threshold", "micro_acc", "macro_acc", "per_class_acc", "gt_labels"):
                assert g[key] == r[key], (part, key)
            assert g["final_pred_labels"] is None and len(r["final_pred_labels"]) == 40
    assert ref["test"][0]["best_threshold"] == ref["val"][0]["best_threshold"]
    with pytest.raises(ValueError, match="hip_eval"):
        M.main(common + ["hip_eval=bogus"])
