"""CPU checks of the supervised fine-tuning path (no GPU here): the ABI of the classifier entry points, their host-side argument
validation, the reference-compatible surface of ``EncoderWithExtraLayer`` and the epoch drivers' refusals."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_classifier_entry_points():
    from bioscanclip.hip import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsclip.h")).read(), flags=re.S)
    for name in ("bsclip_ce_fwd_bwd", "bsclip_class_topk"):
        assert re.search(r"\bint " + name + r"\s*\(", hdr), f"{name} is not declared in include/bsclip.h"
        assert name in lib.SIGNATURES and hasattr(lib.load(), name)
    assert lib.load().bsclip_abi_version() == 10
    # the header states the tie rule and cites the reference sites the entry points replace
    text = open(os.path.join(ROOT, "include", "bsclip.h")).read()
    assert "Ties resolve to the" in text and "lower class index" in text and "fine_tuning_epoch.py:27" in text and "fine_tuning_epoch.py:60" in text


def test_ce_fwd_bwd_validates_on_the_host():
    from bioscanclip.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(64)        # non-null and 16-byte aligned: every check below comes before any dereference or launch

    def ce(logits=one, ldc=132, targets=one, B=4, C=130, loss=one, row_loss=one, dl=one, ld_d=132, dl3=one, ld_d3=3 * 192, flag=one):
        return h.bsclip_ce_fwd_bwd(logits, ldc, targets, B, C, loss, row_loss, dl, ld_d, dl3, ld_d3, flag, None)

    for kw in ({"logits": None}, {"targets": None}, {"loss": None}, {"row_loss": None}, {"flag": None}):
        assert ce(**kw) == -1 and "null pointer" in lib.last_error(), kw
    assert ce(C=0) == -1 and "C=0" in lib.last_error()
    assert ce(B=0) == -1 and "B=0" in lib.last_error()
    assert ce(ldc=128) == -1 and "ldc=128" in lib.last_error()              # ldc < C
    assert ce(ldc=131) == -1 and "ldc=131" in lib.last_error()              # not a multiple of 4
    assert ce(ld_d=129) == -1 and "ld_d=129" in lib.last_error()
    assert ce(ld_d3=3 * 128) == -1 and "ld_d3=384" in lib.last_error()       # C = 130 rounds up to 192 columns per part
    for kw in ({"logits": ctypes.c_void_p(68)}, {"dl": ctypes.c_void_p(72)}, {"dl3": ctypes.c_void_p(68)}, {"targets": ctypes.c_void_p(66)},
               {"flag": ctypes.c_void_p(65)}):
        assert ce(**kw) == -1 and "aligned" in lib.last_error(), kw


def test_class_topk_validates_on_the_host():
    from bioscanclip.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(64)

    def topk(logits=one, ldc=132, B=4, C=130, k=5, scores=one, idx=one):
        return h.bsclip_class_topk(logits, ldc, B, C, k, scores, idx, None)

    for kw in ({"logits": None}, {"scores": None}, {"idx": None}):
        assert topk(**kw) == -1 and "null pointer" in lib.last_error(), kw
    assert topk(C=0) == -1 and "C=0" in lib.last_error()
    assert topk(k=17) == -1 and "k=17" in lib.last_error()
    assert topk(k=0) == -1 and "k=0" in lib.last_error()
    assert topk(C=3, k=5, ldc=4) == -1 and "k=5" in lib.last_error()         # k > C
    assert topk(ldc=128) == -1 and "ldc=128" in lib.last_error()
    assert topk(ldc=130) == -1 and "ldc=130" in lib.last_error()
    assert topk(logits=ctypes.c_void_p(72)) == -1 and "aligned" in lib.last_error()
    assert topk(idx=ctypes.c_void_p(68)) == -1 and "aligned" in lib.last_error()


def test_encoder_with_extra_layer_keeps_the_reference_state_dict():
    from bioscanclip.util.util import EncoderWithExtraLayer
    enc = nn.Sequential(nn.Linear(4, 768))
    m = EncoderWithExtraLayer(enc, nn.Linear(768, 7))
    keys = list(m.state_dict())
    assert [k for k in keys if not k.startswith("encoder.")] == ["new_linear_layer.weight", "new_linear_layer.bias"]
    assert [k for k in keys if k.startswith("encoder.")] == ["encoder.0.weight", "encoder.0.bias"]
    assert tuple(m.state_dict()["new_linear_layer.weight"].shape) == (7, 768)
    m2 = EncoderWithExtraLayer(nn.Sequential(nn.Linear(4, 768)), nn.Linear(768, 7))
    m2.load_state_dict(m.state_dict())                       # strict
    assert torch.equal(m2.new_linear_layer.bias, m.new_linear_layer.bias)
    assert torch.equal(m.get_feature(torch.ones(2, 4)), enc(torch.ones(2, 4)))
    with pytest.raises(NotImplementedError):
        EncoderWithExtraLayer(enc, nn.Sequential(nn.Linear(768, 7), nn.Softmax(dim=-1)))   # the MLP + Softmax head is out of scope
    # no torch compute path: a forward that would record a gradient raises, and CPU tensors are refused by the head
    with pytest.raises(RuntimeError, match="no_grad"):
        m(torch.ones(2, 4))
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        m(torch.ones(2, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        m.loss(torch.ones(2, 4), torch.zeros(2, dtype=torch.int64))


def test_label_batch_to_species_idx_is_list_index():
    from bioscanclip.epoch.fine_tuning_epoch import label_batch_to_species_idx
    classes = ["s3", "s1", "s2", "s1"]                       # a duplicate: list.index returns the first position
    batch = {"species": ["s1", "s2", "s3", "s1"], "genus": ["g"] * 4}
    got = label_batch_to_species_idx(batch, classes)
    assert got.dtype == torch.int64 and got.tolist() == [classes.index(s) for s in batch["species"]] == [1, 2, 0, 1]
    with pytest.raises(ValueError):
        label_batch_to_species_idx({"species": ["unseen"]}, classes)


@pytest.mark.parametrize("criterion", [nn.CrossEntropyLoss(label_smoothing=0.1), nn.CrossEntropyLoss(reduction="sum"),
                                       nn.CrossEntropyLoss(weight=torch.ones(3)), nn.CrossEntropyLoss(ignore_index=0), nn.NLLLoss(),
                                       lambda out, t: out.sum()])
def test_epoch_drivers_refuse_a_non_default_criterion(criterion):
    from bioscanclip.epoch import fine_tuning_epoch as fte
    from bioscanclip.util.util import EncoderWithExtraLayer
    m = EncoderWithExtraLayer(nn.Sequential(nn.Linear(4, 768)), nn.Linear(768, 3))

    class Args:
        activate_wandb = False

    def loader():
        raise AssertionError("the criterion must be refused before a batch is drawn")
        yield

    class Loader:
        def __len__(self):
            return 1

        def __iter__(self):
            return loader()

    with pytest.raises(NotImplementedError, match="no torch compute fallback"):
        fte.fine_tuning_epoch(Args(), m, Loader(), None, criterion, ["a", "b", "c"], 0, "cpu")
    with pytest.raises(NotImplementedError, match="no torch compute fallback"):
        fte.fine_tuning_epoch_image_and_dna(Args(), m, m, Loader(), None, criterion, ["a", "b", "c"], 0, "cpu")


def test_epoch_drivers_refuse_a_text_classifier_and_bad_k():
    from bioscanclip.epoch import fine_tuning_epoch as fte
    from bioscanclip.util.util import EncoderWithExtraLayer
    m = EncoderWithExtraLayer(nn.Sequential(nn.Linear(4, 768)), nn.Linear(768, 3))
    with pytest.raises(NotImplementedError, match="text"):
        fte.fine_tuning_epoch(None, m, [], None, nn.CrossEntropyLoss(), ["a"], 0, "cpu", modality="language")
    with pytest.raises(ValueError):
        fte.evaluate_epoch(m, [], "cpu", ["a"] * 40, k_values=[1, 17])
