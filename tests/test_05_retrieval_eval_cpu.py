"""GPU-resident retrieval evaluation, the parts that need no GPU: label encoding, the host assembly of the accuracy tables from
integer counts (equal, with ``==`` on the floats, to the string path of oracle/retrieval.py), the host-side argument checks of the
new entry points, and the ``hip_eval`` switch."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest

from bioscanclip.hip import retrieval as E
from oracle import retrieval as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
LEVELS = ["order", "family", "genus", "species"]


def test_encode_labels_round_trips_dense_and_shared():
    keys_label, gt_list, _, _ = R.retrieval_case(seed=3, n_keys=50, n_query=30)
    gt_list = gt_list + [{"order": "not_classified", "family": "f0", "genus": "not_classified", "species": "only_here"}]
    (key_ids, query_ids), vocab = E.encode_labels(keys_label, gt_list)
    assert key_ids.dtype == np.int32 and key_ids.shape == (50, 4) and query_ids.shape == (31, 4)
    assert E.decode_labels(key_ids, vocab) == keys_label and E.decode_labels(query_ids, vocab) == gt_list
    for j, lv in enumerate(LEVELS):
        both = np.concatenate([key_ids[:, j], query_ids[:, j]])
        assert sorted(set(both.tolist())) == list(range(len(vocab[lv])))          # dense: every id in [0, n) is used
        assert len(set(vocab[lv])) == len(vocab[lv])
        names = [lab[lv] for lab in keys_label + gt_list]
        for a in range(len(both)):                                                # equal strings <=> equal ids, across the splits
            for b in (0, len(both) // 2, len(both) - 1):
                assert (both[a] == both[b]) == (names[a] == names[b])
    # "not_classified" is a name like any other: it matches itself and nothing else
    assert vocab["order"][query_ids[-1, 0]] == "not_classified" and vocab["genus"][query_ids[-1, 2]] == "not_classified"
    (a, b), v = E.encode_labels([{"s": "not_classified"}], [{"s": "not_classified"}, {"s": "x"}], levels=["s"])
    assert a.tolist() == [[0]] and b.tolist() == [[0], [1]] and v == {"s": ["not_classified", "x"]}


def _counts(indices, key_ids, query_ids, k_list):
    """The integers the kernels return, restated with numpy: first hit rank, then the per-class histograms."""
    Q, k = indices.shape
    L = key_ids.shape[1]
    match = key_ids[indices] == query_ids[:, None, :]                                   # [Q, k, L]
    hit_rank = np.where(match.any(axis=1), match.argmax(axis=1), k).astype(np.int32)    # [Q, L]
    sizes = query_ids.max(axis=0) + 1
    offsets = [0] + np.cumsum(sizes).tolist()
    C = offsets[-1]
    flat = query_ids + np.asarray(offsets[:-1])[None]
    seen = np.bincount(flat.ravel(), minlength=C)
    right = np.stack([np.bincount(flat[hit_rank < min(kk, k)], minlength=C) for kk in k_list])
    return hit_rank, offsets, seen, right


def _assemble_vs_oracle(keys_label, gt_list, indices, pred_list, k_list):
    (key_ids, query_ids), vocab = E.encode_labels(keys_label, gt_list)
    _, offsets, seen, right = _counts(np.asarray(indices), key_ids, query_ids, k_list)
    acc, per_class = E.assemble_accuracy(seen, right, query_ids, offsets, k_list, vocab=vocab)
    macro, ref_per_class = R.top_k_macro_accuracy(pred_list, gt_list, k_list)
    assert acc["micro_acc"] == R.top_k_micro_accuracy(pred_list, gt_list, k_list)     # == on floats: no tolerance
    assert acc["macro_acc"] == macro
    assert per_class == ref_per_class
    assert all(type(k) is int for k in acc["micro_acc"]) and type(acc["macro_acc"][k_list[0]]["order"]) is float
    return acc, per_class


@pytest.mark.parametrize("case", [dict(seed=5, n_keys=60, n_query=40, max_k=5), dict(seed=11, n_keys=500, n_query=333, max_k=5),
                                  dict(seed=2, n_keys=7, n_query=90, max_k=3)])
def test_host_assembly_equals_the_string_path(case):
    keys_label, gt_list, indices, pred_list = R.retrieval_case(**case)
    _assemble_vs_oracle(keys_label, gt_list, indices, pred_list, [1, 3, 5])
    _assemble_vs_oracle(keys_label, gt_list, indices, pred_list, [2])


def test_host_assembly_equals_the_golden_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "retrieval.json")) as f:
        gold = json.load(f)
    keys_label, gt_list, indices, pred_list = R.retrieval_case(**gold["case"])
    acc, per_class = _assemble_vs_oracle(keys_label, gt_list, indices, pred_list, gold["k_list"])
    ints = lambda d: {int(k): v for k, v in d.items()}
    assert acc["micro_acc"] == ints(gold["micro"]) and acc["macro_acc"] == ints(gold["macro"])
    assert per_class == ints(gold["per_class"])


def test_new_entry_points_validate_on_the_host():
    """Null pointers, k = 17, L = 9, nk = 9 and misaligned buffers are refused with -1 and a message before any launch."""
    from bioscanclip.hip import lib
    h = lib.load()
    a16, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    offs, ks = (ctypes.c_int32 * 10)(*range(0, 20, 2)), (ctypes.c_int32 * 9)(*range(1, 10))
    po, pk = ctypes.cast(offs, ctypes.c_void_p), ctypes.cast(ks, ctypes.c_void_p)

    def refused(rc, word):
        assert rc == -1 and word in lib.last_error(), (rc, lib.last_error())

    assert h.bsclip_retrieval_index_floats(0, 768) == -1 and h.bsclip_topk_ip_indexed_workspace_floats(4, 0, 768) == -1
    assert h.bsclip_retrieval_index_floats(300, 768) == 512 * 2 * 768
    assert (h.bsclip_topk_ip_workspace_floats(1300, 300, 768)
            == h.bsclip_retrieval_index_floats(300, 768) + h.bsclip_topk_ip_indexed_workspace_floats(1300, 300, 768))
    refused(h.bsclip_retrieval_index_build(None, 8, 64, a16, None), "null pointer")
    refused(h.bsclip_retrieval_index_build(a16, 8, 65, a16, None), "D=65")
    refused(h.bsclip_retrieval_index_build(a16, 8, 64, odd, None), "16-B aligned")
    refused(h.bsclip_topk_ip_indexed(a16, 4, None, 8, 64, 5, a16, a16, a16, None), "null pointer")
    refused(h.bsclip_topk_ip_indexed(a16, 4, a16, 30, 64, 17, a16, a16, a16, None), "k=17")
    refused(h.bsclip_topk_ip_indexed(a16, 4, a16, 3, 64, 5, a16, a16, a16, None), "k=5")
    refused(h.bsclip_topk_ip_indexed(a16, 4, odd, 30, 64, 5, a16, a16, a16, None), "16-B aligned")
    refused(h.bsclip_topk_ip_indexed(a16, 4, a16, 30, 64, 5, a16, a16, odd, None), "16-B aligned")
    refused(h.bsclip_retrieval_hit_ranks(a16, 4, 5, a16, 30, a16, 4, None, a16, None), "null pointer")
    refused(h.bsclip_retrieval_hit_ranks(a16, 4, 5, a16, 30, a16, 4, a16, None, None), "null pointer")
    refused(h.bsclip_retrieval_hit_ranks(a16, 4, 17, a16, 30, a16, 4, a16, a16, None), "k=17")
    refused(h.bsclip_retrieval_hit_ranks(a16, 4, 5, a16, 30, a16, 9, a16, a16, None), "L=9")
    refused(h.bsclip_retrieval_hit_ranks(odd, 4, 5, a16, 30, a16, 4, a16, a16, None), "aligned")
    refused(h.bsclip_retrieval_hit_ranks(a16, 4, 5, ctypes.c_void_p(4098), 30, a16, 4, a16, a16, None), "aligned")
    refused(h.bsclip_retrieval_class_counts(a16, a16, 4, 4, po, pk, 3, None, a16, a16, None), "null pointer")
    refused(h.bsclip_retrieval_class_counts(a16, a16, 4, 4, None, pk, 3, a16, a16, a16, None), "null pointer")
    refused(h.bsclip_retrieval_class_counts(a16, a16, 4, 9, po, pk, 3, a16, a16, a16, None), "L=9")
    refused(h.bsclip_retrieval_class_counts(a16, a16, 4, 4, po, pk, 9, a16, a16, a16, None), "nk=9")
    refused(h.bsclip_retrieval_class_counts(a16, a16, 4, 4, po, pk, 3, a16, ctypes.c_void_p(4097), a16, None), "aligned")
    bad = (ctypes.c_int32 * 5)(0, 4, 3, 6, 8)
    refused(h.bsclip_retrieval_class_counts(a16, a16, 4, 4, ctypes.cast(bad, ctypes.c_void_p), pk, 3, a16, a16, a16, None), "decrease")


def test_hip_eval_switch():
    import inference_and_eval as host
    import train_cl
    assert host.select_eval(None) is host.inference_and_print_result
    assert host.select_eval(types.SimpleNamespace(hip_eval="host")) is host.inference_and_print_result
    assert host.select_eval(types.SimpleNamespace(hip_eval="gpu")) is host.inference_and_print_result_gpu
    with pytest.raises(ValueError, match="hip_eval"):
        host.select_eval(types.SimpleNamespace(hip_eval="banana"))
    with pytest.raises(ValueError, match="hip_eval"):
        host.main(["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", "hip_eval=banana"])
    with pytest.raises(ValueError, match="hip_eval"):   # before any feature is extracted: the loaders are never touched
        train_cl.eval_phase(None, "cpu", None, None, None, [1, 3, 5], types.SimpleNamespace(hip_eval="banana"))
