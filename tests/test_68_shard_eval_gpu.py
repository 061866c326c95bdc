"""Evaluation from a directory of shard splits, on the GPU: `bsclip_feature_rows` and `bsclip_retrieval_index_append` against numpy and
against `bsclip_retrieval_index_build`, the one-pass extractor against the three-pass `get_features_and_label`, `evaluate_resident`
against both existing table functions, and the two scripts with `eval_shards=<root>` (raw and JPEG roots).

Bar: equality everywhere.  The two kernels copy f32 values (the half-sum `(a + b) * 0.5f` rounds once, like the f32 rounding of
numpy's float64 mean of two f32 values as long as the sum does not overflow -- features are unit vectors), an appended index row is
the row `bsclip_retrieval_index_build` writes, the extractor runs the same encoder calls on the same batches, and everything after
the search is integer arithmetic.  So bits are compared with `==` and no tolerance appears in this file.

`bsclip_feature_rows` takes `[N, D]` tables without a leading dimension, so a table cannot carry spare columns of its own: each table
here is a view into a NaN-filled allocation with guard floats in front of and behind it and rows outside `[row0, row0 + B)`, and all
of those must still be NaN afterwards."""
import os
import sys

import numpy as np
import pytest
import torch

import jpeg_model as jm
from oracle import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
TINY = os.path.join(ROOT, "tests", "golden", "tiny_shard")
LEVELS = ("order", "family", "genus", "species")
MODS = ("image", "dna", "text")
FEATURES = ("encoded_image_feature", "encoded_dna_feature", "encoded_language_feature", "averaged_feature", "concatenated_feature")
GUARD = 12           # floats in front of and behind every table: 48 bytes, so the view stays 16-byte aligned
NODROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- bsclip_feature_rows ---------------------------------------------------------------------------------------------------------

def _table(N, width):
    whole = torch.full((2 * GUARD + N * width,), float("nan"), dtype=torch.float32, device="cuda")
    return whole, whole[GUARD:GUARD + N * width].view(N, width)


@pytest.mark.parametrize("B,D,N,row0", [(1, 64, 7, 6), (5, 768, 53, 3), (24, 768, 53, 29)])
def test_feature_rows_equal_numpy_and_write_nothing_else(B, D, N, row0):
    """Every combination of present modalities, and with image and DNA every combination of the two derived tables."""
    from bioscanclip.hip import ops
    rng = np.random.default_rng(B * 1000 + D)
    host = {m: (rng.standard_normal((B, D)) * 0.04).astype(np.float32) for m in MODS}
    host["image"][0, :4] = [0.0, -0.0, 1.0, -0.75]            # signed zeros and a sum that cancels
    host["dna"][0, :4] = [-0.0, -0.0, -1.0, 0.75]
    host["image"][B - 1, D - 1], host["dna"][B - 1, D - 1] = np.float32(1.0), np.float32(2.0 ** -24)   # a half-sum that has to round
    dev = {m: torch.from_numpy(host[m]).cuda() for m in MODS}
    want = dict(host, avg=((host["image"].astype(np.float64) + host["dna"]) / 2).astype(np.float32),
                cat=np.concatenate((host["image"], host["dna"]), axis=1))
    ran = 0
    for mask in range(1, 8):
        present = [m for bit, m in enumerate(MODS) if mask >> bit & 1]
        both = "image" in present and "dna" in present
        for derived in ([("avg", "cat"), ("avg",), ("cat",), ()] if both else [()]):
            tables = {name: _table(N, 2 * D if name == "cat" else D) for name in (*present, *derived)}
            before = {name: _bits(whole) for name, (whole, _) in tables.items()}
            view = lambda name: tables[name][1] if name in tables else None
            ops.feature_rows(*[dev[m] if m in present else None for m in MODS], row0, *[view(m) for m in MODS],
                             t_avg=view("avg"), t_cat=view("cat"))
            torch.cuda.synchronize()
            for name, (whole, _) in tables.items():
                width = want[name].shape[1]
                expect = before[name].copy()
                assert (expect == before[name][0]).all() and np.isnan(expect.view(np.float32)).all()
                expect[GUARD + row0 * width:GUARD + (row0 + B) * width] = want[name].view(np.uint32).ravel()
                got = _bits(whole)
                assert np.array_equal(got, expect), (present, derived, name, int((got != expect).sum()))
            ran += 1
    assert ran == 7 + 2 * 3                                    # two of the seven combinations hold image and DNA


def test_feature_rows_wrapper_rejects_bad_tensors():
    from bioscanclip.hip import ops
    x = torch.zeros(4, 64, device="cuda")
    t = torch.zeros(8, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.feature_rows(x, None, None, 5, t_image=t)                       # row0 + B > N
    with pytest.raises(ValueError):
        ops.feature_rows(x, None, None, 0, t_image=torch.zeros(8, 128, device="cuda")[:, :64])   # not contiguous
    with pytest.raises(ValueError):
        ops.feature_rows(x, None, None, 0, t_image=t, t_avg=t.clone())       # a derived table without DNA
    with pytest.raises(ValueError):
        ops.feature_rows(x, x, None, 0, t_image=t)                           # an input without its table
    with pytest.raises(ValueError):
        ops.feature_rows(x, x.clone(), None, 0, t_image=t, t_dna=t.clone(), t_cat=t.clone())     # t_cat is [N, 2 D]


# ---- bsclip_retrieval_index_append -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [259, 24])
def test_appended_index_equals_the_built_index(K):
    """K = 259 crosses the 256-row pad (the index has 512 rows), K = 24 is one batch.  Chunks of 1, 5, 24, 64 in turn, walked forwards
    and backwards; a zero key row stays a zero row."""
    from bioscanclip.hip import lib, ops
    from bioscanclip.hip.retrieval import RetrievalIndex
    D = 768
    rng = np.random.default_rng(K)
    keys = (rng.standard_normal((K, D)) * 0.3).astype(np.float32)
    keys[K // 2] = 0.0
    kd = torch.from_numpy(keys).cuda()
    built = ops.retrieval_index_build(kd)
    assert built.numel() == lib.load().bsclip_retrieval_index_floats(K, D) == -(-K // 256) * 256 * 2 * D
    spans, row0 = [], 0
    while row0 < K:
        n = min((1, 5, 24, 64)[len(spans) % 4], K - row0)
        spans.append((row0, n))
        row0 += n
    queries = torch.from_numpy(rng.standard_normal((37, D)).astype(np.float32)).cuda()
    ref_s, ref_i = ops.topk_ip_indexed(queries, built, K, 5)
    for order in (spans, spans[::-1]):
        index = RetrievalIndex.empty(K, D)
        assert index.K == K and index.D == D and not index.index.any()
        for r0, n in order:
            index.append(kd[r0:r0 + n], r0)
        assert np.array_equal(_bits(index.index), _bits(built))             # the zero pad rows up to 256 / 512 included
        s, i = index.search(queries, 5)
        assert torch.equal(s, ref_s) and torch.equal(i, ref_i)
    plain_s, plain_i = ops.topk_ip(queries, kd, 5)
    assert torch.equal(ref_s, plain_s) and torch.equal(ref_i, plain_i)
    with pytest.raises(ValueError):
        index.append(kd[:2], K - 1)                                         # past the last key
    with pytest.raises(ValueError):
        index.append(kd[:2, :704].contiguous(), 0)                          # another width


# ---- the evaluation root, the model and the two extractions, made once ---------------------------------------------------------------

N_SPLIT, BATCH = 29, 24      # one full batch and a ragged one of 5


def _taxonomy(kind, n):
    def sp(i):
        return i % 10 if kind == "keys" else (3 * i + 1) % 10 if kind == "seen" else 10 + i % 4
    taxa = {"order": [f"o{sp(i) % 2}" for i in range(n)], "family": [f"f{sp(i) % 3}" for i in range(n)],
            "genus": [f"g{sp(i) % 5}" for i in range(n)], "species": [f"s{sp(i)}" for i in range(n)]}
    if kind == "unseen":
        taxa["genus"][2] = ""                                 # an empty name is a class like any other
        taxa["family"][4] = "o1"                              # a name that is also an order
    return taxa


def _write_root(root, n=N_SPLIT):
    from bioscanclip.util import shards
    tiny = shards.Shard(TINY)
    for k, (name, kind) in enumerate((("all_keys", "keys"), ("val_seen", "seen"), ("val_unseen", "unseen"))):
        pick = [(7 * k + i) % len(tiny) for i in range(n)]
        shards.write_shard(os.path.join(root, name), [tiny.image(i) for i in pick], [tiny.barcode(i) for i in pick],
                           np.array(tiny.input_ids)[pick], np.array(tiny.token_type_ids)[pick], np.array(tiny.attention_mask)[pick],
                           [f"{kind[0].upper()}{i:03d}" for i in range(n)], taxonomy=_taxonomy(kind, n), split=name)
    return root


def _build():
    """Two-layer towers with text, synthetic weights, eval mode (the ``_build`` of test_90_dist_gpu.py)."""
    from bioscanclip.model import arch
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from bioscanclip.model.language_encoder import LoRA_bert
    from bioscanclip.model.simple_clip import SimpleCLIP
    img = LoRA_ViT_timm(arch.VisionTransformerParams(depth=2), r=4, num_classes=768)
    dna = LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=2, **NODROP)), r=4, num_classes=768)
    txt = LoRA_bert(arch.BertModelParams(arch.bert_small_config(num_hidden_layers=2, **NODROP)), r=4, num_classes=768)
    model = SimpleCLIP(img, dna, txt)
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=51))
    return model.cuda().eval()


def _loaders(root, **kw):
    from bioscanclip.util import shards
    return [shards.ShardLoader(p, BATCH, for_training=False, shuffle=False, with_text=True, **kw) for p in shards.eval_splits(root)]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return _write_root(str(tmp_path_factory.mktemp("eval_root")))


@pytest.fixture(scope="module")
def model():
    return _build()


@pytest.fixture(scope="module")
def extracted(root, model):
    """(one-pass SplitFeatures of the three splits, three-pass dictionaries of fresh identical loaders), bf16 operands."""
    import inference_and_eval as host
    from bioscanclip.hip.features import extract_splits
    resident = extract_splits(_loaders(root), model, "cuda")
    three_pass = [host.get_features_and_label(ld, model, "cuda", for_key_set=(i == 0)) for i, ld in enumerate(_loaders(root))]
    return resident, three_pass


def _assert_same_split(got, ref):
    assert set(got) == set(ref)
    assert got["file_name_list"] == ref["file_name_list"] and len(ref["file_name_list"]) == N_SPLIT
    assert got["label_list"] == ref["label_list"] and got["all_key_features_label"] == ref["all_key_features_label"]
    for name in (*FEATURES, "all_key_features"):
        if ref[name] is None:
            assert got[name] is None, name
            continue
        assert got[name].dtype == np.float64 and got[name].shape == ref[name].shape, name
        a, b = got[name].astype(np.float32), ref[name].astype(np.float32)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, int((a != b).sum()))


def test_one_pass_extraction_equals_three_passes(extracted):
    resident, three_pass = extracted
    for i, (split, ref) in enumerate(zip(resident, three_pass)):
        _assert_same_split(split.as_dict(), ref)
        assert (ref["all_key_features"] is not None) == (i == 0)
        assert all(t.is_cuda and t.dtype == torch.float32 for t in split.tables.values() if t is not None)
    keys = resident[0]
    all_keys = keys.tables["all_key_features"]
    assert tuple(all_keys.shape) == (3 * N_SPLIT, 768)
    for k, name in enumerate(FEATURES[:3]):                    # the three towers' tables are the thirds of that allocation: no copy
        assert keys.tables[name].data_ptr() == all_keys.data_ptr() + k * N_SPLIT * 768 * 4
    assert set(keys.indices) == {*FEATURES, "all_key_features"} and resident[1].indices == {}
    from bioscanclip.hip import ops
    for name, index in keys.indices.items():                   # filled batch by batch: the index of the whole table, bit for bit
        assert np.array_equal(_bits(index.index), _bits(ops.retrieval_index_build(keys.tables[name].contiguous()))), name
    assert keys.vocab is resident[1].vocab is resident[2].vocab and keys.label_ids.dtype == np.int32


def test_one_pass_extraction_equals_three_passes_on_fp16_operands(root, model, extracted):
    import inference_and_eval as host
    from bioscanclip.hip.engine import set_operand_format
    from bioscanclip.hip.features import extract_split
    set_operand_format(model, "fp16")
    try:
        loader, again = _loaders(root)[0], _loaders(root)[0]
        got = extract_split(loader, model, "cuda", for_key_set=True).as_dict()
        ref = host.get_features_and_label(again, model, "cuda", for_key_set=True)
    finally:
        set_operand_format(model, "bf16")
    _assert_same_split(got, ref)
    bf16 = extracted[1][0]["encoded_image_feature"]
    assert not np.array_equal(ref["encoded_image_feature"], bf16)          # the other format did run


def test_extract_split_refusals(root, model):
    from bioscanclip.hip.features import extract_split
    from bioscanclip.util import shards
    no_text = shards.ShardLoader(shards.eval_splits(root)[1], BATCH, for_training=False, shuffle=False, with_text=False)
    with pytest.raises(ValueError, match="with_text"):
        extract_split(no_text, model, "cuda")
    with pytest.raises(ValueError, match="label rows"):
        extract_split(_loaders(root)[1], model, "cuda", labels=(np.zeros((3, 4), np.int32), {}))


# ---- the tables --------------------------------------------------------------------------------------------------------------------

def test_evaluate_resident_equals_both_table_functions(extracted, capsys):
    import inference_and_eval as host
    from bioscanclip.hip.retrieval import evaluate_resident
    resident, three_pass = extracted
    capsys.readouterr()
    ref = host.inference_and_print_result(*three_pass, k_list=[1, 3, 5])
    ref_out = capsys.readouterr().out
    via_dicts = host.inference_and_print_result_gpu(*three_pass, k_list=[1, 3, 5])
    dict_out = capsys.readouterr().out
    got = evaluate_resident(*resident, k_list=[1, 3, 5])
    got_out = capsys.readouterr().out
    with_pred = evaluate_resident(*resident, k_list=[1, 3, 5], with_predictions=True)
    pred_out = capsys.readouterr().out
    assert got[0] == ref[0] == via_dicts[0] and got[1] == ref[1] == via_dicts[1]
    assert with_pred[0] == ref[0] and with_pred[1] == ref[1] and with_pred[2] == ref[2]
    assert got_out == ref_out == dict_out == pred_out and "macro_acc top-5" in ref_out
    acc = ref[0]
    assert sum(bool(acc[q][kf]) for q in acc for kf in acc[q]) == 4 * 5 + 1   # every 768-wide pair and concatenated x concatenated
    idx = got[2]["encoded_dna_feature"]["all_key_features"]["curr_seen_indices"]
    assert idx.is_cuda and idx.dtype == torch.int64 and tuple(idx.shape) == (N_SPLIT, 5) and int(idx.max()) < 3 * N_SPLIT
    cell = acc["encoded_image_feature"]["encoded_image_feature"]
    assert cell["unseen"]["micro_acc"][5]["species"] == 0.0                 # no unseen species among the keys
    assert "" in ref[1]["encoded_image_feature"]["encoded_image_feature"]["unseen"][1]["genus"]
    _, again = extracted
    assert evaluate_resident(*resident, k_list=[5, 1, 3])[0] == host.inference_and_print_result(*again, k_list=[5, 1, 3])[0]
    capsys.readouterr()


def test_evaluate_resident_refuses_separately_encoded_splits(root, model):
    from bioscanclip.hip.features import extract_split
    from bioscanclip.hip.retrieval import evaluate_resident
    loaders = _loaders(root)
    alone = [extract_split(ld, model, "cuda", for_key_set=(i == 0), index=False) for i, ld in enumerate(loaders[:2])]
    assert alone[0].vocab != alone[1].vocab
    with pytest.raises(ValueError, match="vocabular"):
        evaluate_resident(alone[0], alone[1], alone[1])


# ---- the scripts -------------------------------------------------------------------------------------------------------------------

CONFIG = ["model_config=lora_vit_lora_barcode_bert_lora_bert_ssl", "model_config.load_ckpt=false", "debug_flag=false"]


def _table_lines(out):
    return [ln for ln in out.splitlines() if ln.startswith("Query_feature")]


def test_inference_and_eval_script_on_a_shard_root(root, model, tmp_path, monkeypatch, capsys):
    """``eval_shards=<root>``: ``hip_eval=gpu`` (resident) equals ``hip_eval=host`` (``as_dict`` into the host path), a saved cache gives
    the same table through both, and the silhouette lines are the same.  ``load_clip_model`` is replaced by the two-layer model."""
    import inference_and_eval
    from bioscanclip.model import simple_clip
    monkeypatch.setattr(simple_clip, "load_clip_model", lambda args, device=None: model)
    common = CONFIG + [f"project_root_path={tmp_path}", f"eval_shards={root}", "inference_and_eval_setting.silhouette=true"]
    capsys.readouterr()
    got = inference_and_eval.main(common + ["hip_eval=gpu", "save_inference=true"])
    got_out = capsys.readouterr().out
    ref = inference_and_eval.main(common + ["hip_eval=host"])
    ref_out = capsys.readouterr().out
    assert got[0] == ref[0] and got[1] == ref[1]
    assert _table_lines(got_out) == _table_lines(ref_out) and len(_table_lines(ref_out)) == 21 * 2 * 3
    silhouette = lambda out: [ln for ln in out.splitlines() if ln.startswith("The silhouette score")]
    assert silhouette(got_out) == silhouette(ref_out) and len(silhouette(ref_out)) == 8
    assert "curr_seen_indices" in got[2]["encoded_image_feature"]["encoded_dna_feature"]
    assert "curr_seen_pred_list" in ref[2]["encoded_image_feature"]["encoded_dna_feature"]
    cache = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith(".npz")]
    assert [os.path.basename(p) for p in cache] == ["extracted_feature_from_val_split.npz"]
    for mode in ("gpu", "host"):
        loaded = inference_and_eval.main(common + [f"hip_eval={mode}", "load_inference=true"])
        out = capsys.readouterr().out
        assert "Initialize model" not in out and loaded[0] == ref[0] and loaded[1] == ref[1]
        assert _table_lines(out) == _table_lines(ref_out) and silhouette(out) == silhouette(ref_out)
    with pytest.raises(ValueError, match="eval_split"):
        inference_and_eval.main(common + ["eval_split=train"])
    with pytest.raises(ValueError, match="test_seen"):
        inference_and_eval.main(common + ["eval_split=test"])             # the root has no test splits


def test_inference_and_eval_script_on_a_jpeg_root_equals_its_raw_twin(model, tmp_path, monkeypatch, capsys):
    """A JPEG root of the tests/golden/jpeg fixtures (with a sync index) and a raw root of the pixels they decode to: the same
    ``acc_dict``, with the streams Huffman-decoded on the loader threads and on the device."""
    import inference_and_eval
    from bioscanclip.model import simple_clip
    from bioscanclip.util import shards
    monkeypatch.setattr(simple_clip, "load_clip_model", lambda args, device=None: model)
    tiny = shards.Shard(TINY)
    items = [(nm, jm.model_pixels(coef, qtab, rec)) for nm, coef, qtab, rec in jm.decode_all()]   # test_66: the kernel's pixels, bit for bit
    for k, (name, kind) in enumerate((("all_keys", "keys"), ("val_seen", "seen"), ("val_unseen", "unseen"))):
        n = (11, 7, 5)[k]
        pick = [items[(3 * k + i) % len(items)] for i in range(n)]
        common = dict(barcodes=[tiny.barcode(5 * k + i) for i in range(n)], input_ids=np.array(tiny.input_ids[5 * k:5 * k + n]),
                      token_type_ids=np.array(tiny.token_type_ids[5 * k:5 * k + n]),
                      attention_mask=np.array(tiny.attention_mask[5 * k:5 * k + n]), processid=[f"{name}{i}" for i in range(n)],
                      taxonomy=_taxonomy(kind, n), split=name)
        shards.write_shard(str(tmp_path / "jpeg" / name), [jm.fixture_bytes(nm) for nm, _ in pick], image_codec="jpeg",
                           jpeg_sync_mcus=shards.DEFAULT_JPEG_SYNC_MCUS, **common)
        shards.write_shard(str(tmp_path / "raw" / name), [px for _, px in pick], **common)
    run = lambda kind, *more: inference_and_eval.main(CONFIG + [f"project_root_path={tmp_path}", f"eval_shards={tmp_path / kind}",
                                                                "hip_eval=gpu", "inference_and_eval_setting.k_list=[1,3]", *more])
    capsys.readouterr()
    raw = run("raw")
    raw_out = capsys.readouterr().out
    on_host = run("jpeg")
    host_out = capsys.readouterr().out
    on_gpu = run("jpeg", "hip_jpeg_entropy=gpu")
    gpu_out = capsys.readouterr().out
    assert on_host[0] == raw[0] and on_gpu[0] == raw[0] and on_host[1] == raw[1] and on_gpu[1] == raw[1]
    assert _table_lines(host_out) == _table_lines(raw_out) == _table_lines(gpu_out) and len(_table_lines(raw_out)) == 21 * 2 * 2
    with pytest.raises(ValueError, match="sync index"):
        run("raw", "hip_jpeg_entropy=gpu")                                 # a raw shard has no streams to decode


def test_train_cl_evaluates_the_val_splits_of_a_shard_root(root, tmp_path, monkeypatch, capsys):
    """``train_cl.py eval_shards=<root>``: one epoch of one step, then ``eval_phase`` on the root's val splits, the ``overall_acc`` line
    and ``best.pth``; then once more with ``hip_eval=gpu``."""
    import train_cl
    monkeypatch.setattr(train_cl, "load_clip_model", lambda args, device=None: _build().train())
    common = CONFIG + ["model_config.batch_size=8", "model_config.epochs=1", "synthetic_steps_per_epoch=1", f"eval_shards={root}",
                       "save_ckpt=true", f"project_root_path={tmp_path}"]
    capsys.readouterr()
    torch.manual_seed(3)
    losses = train_cl.main(common)
    out = capsys.readouterr().out
    assert len(losses) == 1 and "epoch 0: overall_acc" in out and len(_table_lines(out)) == 21 * 2 * 3
    ck = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith(".pth")]
    assert any(p.endswith("last.pth") for p in ck) and any(p.endswith("best.pth") for p in ck)
    train_cl.main(common + ["hip_eval=gpu", "save_ckpt=false"])             # the resident scoring: the same table layout
    out_gpu = capsys.readouterr().out
    assert "epoch 0: overall_acc" in out_gpu and len(_table_lines(out_gpu)) == 21 * 2 * 3
