"""Method one, method two and supervised fine-tuning from a protocol root of shards, on the GPU.

Every root is written here with `write_shard`: 8 splits of 20 samples (batch 8 leaves a ragged batch of 4), 32 x 48 raw pictures, 660-nt
barcodes, 6 species over 3 genera.  Five species are seen (the fifth only once per split), the sixth is absent from `train_seen` and
fills the unseen query splits; the unseen key splits hold it next to the fifth species, so their search has two answers to choose from.

Bar: equality everywhere.  The resident paths run the same encoder and classifier calls on the same batches as the loader-walk
functions they are compared with, an appended index row is the row `bsclip_retrieval_index_build` writes (test_68), and everything
after the searches is integer arithmetic; the fine-tuning runs differ only in where their target integers come from.  So tables are
compared with `==`, tensors bit for bit, and no tolerance appears in this file."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import jpeg_model as jm
from oracle import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
NODROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
N, BATCH = 20, 8
SPECIES = ["Aus one", "Aus two", "Bus one", "Bus two", "Cus rare", "Cus new"]       # genus = the first word
CONFIG = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", "debug_flag=false", f"eval_batch_size={BATCH}"]
TABLE_KEYS = ("best_threshold", "micro_acc", "macro_acc", "per_class_acc", "gt_labels")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _species_of(name, k):
    if name in ("val_unseen", "test_unseen"):
        return [5] * N
    if name.endswith("unseen_keys"):
        return [5 if (i + k) % 3 else 4 for i in range(N)]
    return [4 if i == 7 else (i + k) % 4 for i in range(N)]               # the fifth species: one sample per seen split


def _taxonomy(species_ids):
    names = [SPECIES[s] for s in species_ids]
    genus = [s.split(" ")[0] for s in names]
    return {"order": ["Diptera"] * len(names), "family": ["Fam-" + g[0] if g != "Cus" else "Fam-A" for g in genus], "genus": genus,
            "species": names}


def _write_split(path, name, species_ids, seed, images=None, **kw):
    from bioscanclip.util import shards
    rng = np.random.default_rng(seed)
    n = len(species_ids)
    if images is None:
        images = [rng.integers(0, 256, (32, 48, 3), dtype=np.uint8) for _ in range(n)]
    barcodes = ["".join(rng.choice(list("ACGT"), 660)) for _ in range(n)]
    zeros = np.zeros((n, 4), dtype=np.int64)
    shards.write_shard(os.path.join(path, name), images, barcodes, zeros, zeros, zeros, [f"{name}-{i:02d}" for i in range(n)],
                       taxonomy=_taxonomy(species_ids), split=name, **kw)


def _write_root(path, species_of=_species_of):
    from bioscanclip.util import shards
    for k, name in enumerate(shards.PROTOCOL_SPLITS):
        _write_split(path, name, species_of(name, k), seed=100 + k)
    return path


def _build():
    """Two-layer image and DNA towers, synthetic weights, no dropout, eval mode."""
    from bioscanclip.model import arch
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from bioscanclip.model.simple_clip import SimpleCLIP
    img = LoRA_ViT_timm(arch.VisionTransformerParams(depth=2), r=4, num_classes=768)
    dna = LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=2, **NODROP)), r=4, num_classes=768)
    model = SimpleCLIP(img, dna, None)
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=69))
    return model.cuda().eval()


def _args(mode="host", k_list=(1, 3, 5)):
    return types.SimpleNamespace(inference_and_eval_setting=types.SimpleNamespace(k_list=list(k_list)), hip_eval=mode, activate_wandb=False)


class _Collated:
    """A loader whose slot 6 is the collated form ``{level: [names]}`` of the label dictionaries the wrapped ``ShardLoader`` yields:
    what ``label_batch_to_species_idx`` and the species-list functions index by level."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield (*batch[:6], {lv: [d[lv] for d in batch[6]] for lv in ("order", "family", "genus", "species")})


def _loader(root, name, batch=BATCH, **kw):
    """The loader the unchanged functions are handed: label dictionaries in slot 6."""
    from bioscanclip.util import shards
    return shards.ShardLoader(os.path.join(root, name), batch, for_training=False, shuffle=False, with_text=False, **kw)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return _write_root(str(tmp_path_factory.mktemp("protocol_root")))


@pytest.fixture(scope="module")
def model():
    return _build()


@pytest.fixture()
def one_model(model, monkeypatch):
    from bioscanclip.model import simple_clip
    monkeypatch.setattr(simple_clip, "load_clip_model", lambda args, device=None: model)
    return model


def _species_lists(root):
    import method_one_eval as M
    seen = M.get_all_unique_species_from_dataloader(_Collated(_loader(root, "seen_keys")))
    unseen = (M.get_all_unique_species_from_dataloader(_Collated(_loader(root, "val_unseen_keys")))
              + M.get_all_unique_species_from_dataloader(_Collated(_loader(root, "test_unseen_keys"))))
    return seen, unseen


def _assert_same_results(got, ref, root, capsys):
    import method_one_eval as M
    seen_species, unseen_species = _species_lists(root)
    assert set(seen_species) == set(SPECIES[:5]) and set(unseen_species) == set(SPECIES[4:])
    for part in ("val", "test"):
        for g, r, listed in zip(got[part], ref[part], (seen_species, unseen_species)):
            for key in TABLE_KEYS:
                assert g[key] == r[key], (part, key)
            assert len(g["gt_labels"]) == N
            shares = [M.check_for_acc_about_correct_predict_seen_or_unseen(M._predictions_of(o), listed) for o in (g, r)]
            assert shares[0] == shares[1] and sorted(shares[0]) == [1, 3, 5], part
    assert got["test"][0]["best_threshold"] == got["val"][0]["best_threshold"]
    capsys.readouterr()


# ---- method one --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def method_one_reference(root, model):
    """The unchanged function on shard loaders of the root, host scoring: val, then test at val's threshold."""
    import method_one_eval as M
    ref, threshold = {}, None
    for part in ("val", "test"):
        ref[part] = M.method_1_inference_and_eval_for_seen_and_unseen(
            _args("host"), model, _loader(root, f"{part}_seen"), _loader(root, f"{part}_unseen"), _loader(root, "seen_keys"),
            _loader(root, "val_unseen_keys"), _loader(root, "test_unseen_keys"), torch.device("cuda", 0), searched_threshold=threshold)
        threshold = ref[part][0]["best_threshold"]
    return ref


@pytest.mark.parametrize("mode", ["gpu", "host"])
def test_method_one_from_a_protocol_root(root, one_model, method_one_reference, mode, capsys):
    import method_one_eval as M
    got = M.main(CONFIG + [f"eval_shards={root}", f"hip_eval={mode}"])
    text = capsys.readouterr().out
    assert text.count("for k = ") == 12 and len([ln for ln in text.splitlines() if ln.startswith(" ")]) == 2 * 2 * 3
    _assert_same_results(got, method_one_reference, root, capsys)
    acc = got["val"][1]["micro_acc"]
    assert 0.0 < got["val"][0]["micro_acc"][5]["order"] and set(acc[1]) == {"order", "family", "genus", "species"}
    if mode == "gpu":
        split = got["val"][0]["merged"].split
        assert split.sim.is_cuda and tuple(split.sim.shape) == (N, 5) and got["val"][0]["final_pred_labels"] is None
        assert int(split.idx_unseen.max()) < 2 * N                       # one index over both unseen key splits


def test_method_one_on_a_jpeg_root_equals_its_raw_twin(one_model, tmp_path, capsys):
    """The tests/golden/jpeg fixtures as a JPEG root with a sync index, Huffman-decoded on the device, against a raw root of the
    pixels they decode to."""
    import method_one_eval as M
    from bioscanclip.util import shards
    items = [(nm, jm.model_pixels(coef, qtab, rec)) for nm, coef, qtab, rec in jm.decode_all()]
    n = 9
    for k, name in enumerate(M.METHOD_ONE_SPLITS):
        pick = [items[(2 * k + i) % len(items)] for i in range(n)]
        ids = _species_of(name, k)[:n]
        _write_split(str(tmp_path / "jpeg"), name, ids, seed=200 + k, images=[jm.fixture_bytes(nm) for nm, _ in pick], image_codec="jpeg",
                     jpeg_sync_mcus=4)
        _write_split(str(tmp_path / "raw"), name, ids, seed=200 + k, images=[px for _, px in pick])
    run = lambda kind, *more: M.main(CONFIG + [f"eval_shards={tmp_path / kind}", "hip_eval=gpu", *more])
    raw, on_gpu = run("raw"), run("jpeg", "hip_jpeg_entropy=gpu")
    for part in ("val", "test"):
        for g, r in zip(on_gpu[part], raw[part]):
            for key in TABLE_KEYS:
                assert g[key] == r[key], (part, key)
            assert torch.equal(g["merged"].split.sim, r["merged"].split.sim)
    with pytest.raises(ValueError, match="sync index"):
        run("raw", "hip_jpeg_entropy=gpu")                                 # a raw shard has no streams to decode
    capsys.readouterr()


# ---- method two --------------------------------------------------------------------------------------------------------------------

def _classifier(encoder_model, C, seed=11):
    import method_two_fine_tuning_and_eval as M
    torch.manual_seed(seed)
    head = nn.Linear(768, C)
    with torch.no_grad():
        head.weight.mul_(40.0)                                            # confidences that spread over the threshold grid
    return M.ViTWIthExtraLayer(encoder_model.image_encoder, head).cuda()


@pytest.mark.parametrize("mode", ["gpu", "host"])
def test_method_two_from_a_protocol_root(root, model, tmp_path, monkeypatch, mode, capsys):
    import method_two_fine_tuning_and_eval as M
    from bioscanclip.hip import ops
    from bioscanclip.model import simple_clip
    device = torch.device("cuda", 0)
    label_map, idx_to_all_labels = M.load_all_seen_species_name_and_create_label_map(_Collated(_loader(root, "train_seen")))
    C = len(label_map)
    assert C == 5 and list(label_map) == sorted(SPECIES[:5])
    saved = _classifier(_build(), C)
    torch.save(saved.state_dict(), str(tmp_path / "last.pth"))            # no training: the script resumes from this file
    saved.eval()
    built = []
    monkeypatch.setattr(simple_clip, "load_clip_model", lambda args, device=None: built.append(_build()) or built[-1])
    got = M.main(CONFIG + [f"eval_shards={root}", f"hip_eval={mode}", f"model_config.fine_tuning_set.fine_tune_model_output_dir={tmp_path}"])
    capsys.readouterr()
    assert len(built) == 2 and got["history"] == []
    ref, threshold = {}, None
    for part in ("val", "test"):
        ref[part] = M.method_2_inference_and_eval_for_seen_and_unseen(
            _args("host"), saved, model, _loader(root, f"{part}_seen"), _loader(root, f"{part}_unseen"), _loader(root, "val_unseen_keys"),
            _loader(root, "test_unseen_keys"), label_map, idx_to_all_labels, device, searched_threshold=threshold)
        threshold = ref[part][0]["best_threshold"]
    _assert_same_results(got, ref, root, capsys)
    assert ref["val"][0]["best_threshold"] in np.linspace(0, 1, 1001).tolist()
    if mode == "gpu":
        for part, kind, out in (("val", "seen", got["val"][0]), ("test", "unseen", got["test"][1])):
            confs, idxs = [], []
            with torch.no_grad():
                for batch in _loader(root, f"{part}_{kind}"):
                    conf, idx = ops.class_softmax_topk(saved(batch[1].cuda()), C, 5)
                    confs.append(conf)
                    idxs.append(idx)
            split = out["merged"].split
            assert tuple(split.sim.shape) == (N, 5) and split.sim.is_cuda
            assert torch.equal(split.sim.view(torch.int32), torch.cat(confs).view(torch.int32)) and torch.equal(split.idx_seen, torch.cat(idxs))
            assert len(torch.unique(split.sim)) > N                       # real confidences, not a constant


# ---- fine-tuning targets -----------------------------------------------------------------------------------------------------------

def _pair(C, seed=5):
    from bioscanclip.util.util import EncoderWithExtraLayer
    m = _build()
    torch.manual_seed(seed)
    return (EncoderWithExtraLayer(m.image_encoder, nn.Linear(768, C)).cuda(), EncoderWithExtraLayer(m.dna_encoder, nn.Linear(768, C)).cuda())


def _one_epoch(proto, classes, resident):
    """One epoch of both classifiers over shuffled ``train_seen`` at batch 8, then ``evaluate_epoch`` of both on ``val_seen``: returns
    (epoch loss, per-step loss terms, trainable parameters, evaluation dictionaries)."""
    from bioscanclip.epoch import fine_tuning_epoch as fte
    from bioscanclip.hip.optim import FusedAdamW
    device = torch.device("cuda", 0)
    img, dna = _pair(len(classes))
    terms = []
    for m in (img, dna):
        def loss(x, target, flag=None, _loss=m.loss):
            terms.append(_loss(x, target, flag=flag))
            return terms[-1]
        m.loss = loss
    opt = FusedAdamW([p for m in (img, dna) for p in m.parameters() if p.requires_grad], lr=1e-3)
    labels = "ids" if resident else None
    train = proto.loader("train_seen", labels=labels, batch_size=BATCH, shuffle=True, seed=3)
    train.set_epoch(1)
    collated = (lambda ld: ld) if resident else _Collated
    torch.manual_seed(77)
    mean = fte.fine_tuning_epoch_image_and_dna(_args(), img, dna, collated(train), opt, nn.CrossEntropyLoss(), classes, 0, device,
                                               targets_of=proto.targets(classes, "train_seen") if resident else None)
    val_targets = proto.targets(classes, "val_seen") if resident else None
    evals = [fte.evaluate_epoch(m, collated(proto.loader("val_seen", labels=labels, batch_size=BATCH)), device, classes, modality=mod,
                                targets_of=val_targets) for m, mod in ((img, "image"), (dna, "dna"))]
    params = {f"{w}.{k}": p.detach().clone() for w, m in (("image", img), ("dna", dna)) for k, p in m.named_parameters() if p.requires_grad}
    return mean, [t.detach().clone() for t in terms], params, evals


def test_resident_targets_train_and_evaluate_as_list_index_targets(root):
    from bioscanclip.hip.protocols import ProtocolRoot
    proto = ProtocolRoot(root, ("train_seen", "val_seen"), batch_size=BATCH)
    classes = [SPECIES[i] for i in (2, 4, 0, 3, 1)]                        # not the order of first appearance: the look-up table works
    assert sorted(classes) == sorted(proto.first_appearance_classes("train_seen"))
    got_mean, got_terms, got_params, got_evals = _one_epoch(proto, classes, resident=True)
    ref_mean, ref_terms, ref_params, ref_evals = _one_epoch(proto, classes, resident=False)
    assert len(ref_terms) == 2 * 3 and len(got_terms) == len(ref_terms)    # 3 steps (8 + 8 + 4), two classifiers
    for step, (a, b) in enumerate(zip(got_terms, ref_terms)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"loss term {step}: {a.item()} vs {b.item()}"
    assert got_mean == ref_mean and np.isfinite(ref_mean) and ref_mean > 0
    assert set(got_params) == set(ref_params) and len(ref_params) > 4
    for name in ref_params:
        assert torch.equal(got_params[name], ref_params[name]), name
    assert got_evals == ref_evals and sorted(ref_evals[0]) == ["top1_accuracy", "top3_accuracy", "top5_accuracy"]
    assert ref_evals[0]["top5_accuracy"] == 1.0                            # five classes


def test_species_outside_the_class_list_raises(tmp_path, monkeypatch):
    """Training: the fused cross-entropy's flag word, read at the end of the epoch.  Evaluation: the counting kernel's range check."""
    import supervised_fine_tune
    from bioscanclip.epoch import fine_tuning_epoch as fte
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.hip.protocols import ProtocolRoot
    from bioscanclip.model import simple_clip
    root = str(tmp_path)
    _write_split(root, "train_seen", _species_of("train_seen", 0), seed=1)
    _write_split(root, "val_seen", [5 if i == 13 else s for i, s in enumerate(_species_of("val_seen", 4))], seed=2)   # one stranger
    device = torch.device("cuda", 0)
    proto = ProtocolRoot(root, ("train_seen", "val_seen"), batch_size=BATCH)
    classes = proto.first_appearance_classes("train_seen")
    assert proto.class_columns(classes, "val_seen")[0].tolist().count(-1) == 1
    img, _ = _pair(len(classes))
    with pytest.raises(ValueError, match="outside"):
        fte.evaluate_epoch(img, proto.loader("val_seen"), device, classes, targets_of=proto.targets(classes, "val_seen"))
    opt = FusedAdamW([p for p in img.parameters() if p.requires_grad], lr=1e-3)
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        fte.fine_tuning_epoch(_args(), img, proto.loader("train_seen"), opt, nn.CrossEntropyLoss(), classes[:4], 0, device,
                              targets_of=proto.targets(classes[:4], "train_seen"))
    monkeypatch.setattr(simple_clip, "load_clip_model", lambda args, device=None: _build())
    with pytest.raises(ValueError, match="outside"):
        supervised_fine_tune.main(CONFIG + [f"dataset={root}", f"model_config.batch_size={BATCH}"])


# ---- supervised_fine_tune.py -------------------------------------------------------------------------------------------------------

def test_supervised_fine_tune_on_a_protocol_root(root, monkeypatch, capsys):
    import supervised_fine_tune as S
    from bioscanclip.epoch import fine_tuning_epoch as fte
    from bioscanclip.model import simple_clip
    from bioscanclip.util.util import EncoderWithExtraLayer
    monkeypatch.setattr(simple_clip, "load_clip_model", lambda args, device=None: _build())
    wrapped = []
    monkeypatch.setattr(S, "EncoderWithExtraLayer", lambda enc, head: wrapped.append(EncoderWithExtraLayer(enc, head)) or wrapped[-1])
    rows = S.main(CONFIG + [f"dataset={root}", "fine_tune_epochs=1", f"model_config.batch_size={BATCH}"])
    text = capsys.readouterr().out
    assert "5 species in the training labels" in text and len(rows) == 1 and len(wrapped) == 2
    epoch, loss, acc_i, acc_d = rows[0]
    assert epoch == 0 and np.isfinite(loss) and loss > 0
    classes = [SPECIES[i] for i in (0, 1, 2, 3, 4)]                        # train_seen's species in order of first appearance
    assert wrapped[0].new_linear_layer.out_features == 5
    device = torch.device("cuda", 0)
    for m, modality, acc in ((wrapped[0], "image", acc_i), (wrapped[1], "dna", acc_d)):
        assert acc == fte.evaluate_epoch(m, _Collated(_loader(root, "val_seen")), device, classes, k_values=[1, 3, 5], modality=modality)
        assert acc["top5_accuracy"] == 1.0
