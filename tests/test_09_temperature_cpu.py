"""The trainable temperature (``model_config.trainable_temperature``) without a GPU: the host validation of
``bsclip_infonce_fwd_bwd_ts``, the ``logit_scale`` parameter of ``load_clip_model``, checkpoints with and without it, and the
refusal of more than one rank."""
import ctypes
import math
import os
import sys

import pytest
import torch

from helpers import skip_param_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bioscan-clip_amd")
CONFIG = "model_config=lora_vit_lora_barcode_bert_ssl"


def test_host_validation_names_the_argument():
    """Every bad argument is refused with -1 before any launch (there is no GPU here), and the message says which one."""
    from bioscanclip.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(16)                      # non-null, 16-byte aligned: never dereferenced on the host
    ptrs = lambda n: (ctypes.c_void_p * n)(*[16] * n)

    def call(nmod=2, N=8, row0=0, n_local=8, log_scale=one, scale_out=one, workspace=one):
        return h.bsclip_infonce_fwd_bwd_ts(ptrs(max(nmod, 1)), nmod, one, N, 768, log_scale, row0, n_local, one, ptrs(max(nmod, 1)),
                                           scale_out, workspace, None)

    assert call(log_scale=None) == -1
    assert "log_scale_dev" in lib.last_error()
    assert call(scale_out=None) == -1
    assert "scale_out" in lib.last_error()
    assert call(workspace=ctypes.c_void_p(20)) == -1
    assert "workspace" in lib.last_error()
    assert call(row0=4, n_local=5) == -1
    assert "row0=4" in lib.last_error() and "n_local=5" in lib.last_error()
    assert call(N=0, n_local=0) == -1
    assert "N=0" in lib.last_error()
    assert call(nmod=1) == -1
    assert "nmod=1" in lib.last_error() and "Too less element" in lib.last_error()
    for msg in ("bsclip_infonce_fwd_bwd_ts",):
        assert msg in lib.last_error()


def _config(*extra):
    from bioscanclip.util.config import load_config
    return load_config(os.path.join(PKG, "bioscanclip", "config"), [CONFIG, *extra])


def _load(*extra):
    from bioscanclip.model.simple_clip import load_clip_model
    with skip_param_init():
        return load_clip_model(_config(*extra))


def test_load_clip_model_creates_the_parameter_only_when_asked():
    on = _load("model_config.trainable_temperature=true")
    assert "logit_scale" in dict(on.named_parameters()) and on.logit_scale.requires_grad
    assert "logit_scale" in on.state_dict()
    assert on.logit_scale.dtype == torch.float32 and on.logit_scale.numel() == 1
    assert abs(float(on.logit_scale.detach()) - math.log(1 / 0.07)) < 1e-6
    assert torch.equal(on.state_dict()["logit_scale"], torch.tensor(math.log(1 / 0.07)))
    absent = _load()
    off = _load("model_config.trainable_temperature=false")
    for m in (absent, off):
        assert "logit_scale" not in dict(m.named_parameters()) and not hasattr(m, "logit_scale")
    assert list(off.state_dict()) == list(absent.state_dict())
    assert sorted(on.state_dict()) == sorted(list(absent.state_dict()) + ["logit_scale"])


def test_checkpoints_with_and_without_the_temperature(tmp_path, monkeypatch, capsys):
    """A checkpoint without ``logit_scale`` loads when the option is on (initial value kept, one line printed); one with the key
    restores it; a model built without the option ignores the key."""
    from bioscanclip.model import simple_clip
    from bioscanclip.util.util import load_model_and_checkpoint
    plain = _load()
    sd = {k: v.clone() for k, v in plain.state_dict().items()}
    without, with_t = str(tmp_path / "without.pth"), str(tmp_path / "with.pth")
    torch.save(sd, without)
    torch.save(dict(sd, logit_scale=torch.tensor(3.25)), with_t)
    real = simple_clip.load_clip_model

    def quick(args, device=None):
        with skip_param_init():
            return real(args, device)

    monkeypatch.setattr(simple_clip, "load_clip_model", quick)
    cpu = torch.device("cpu")
    on = "model_config.trainable_temperature=true"
    capsys.readouterr()
    model, loaded = load_model_and_checkpoint(_config(on, f"model_config.ckpt_path={without}"), cpu)
    out = capsys.readouterr().out
    assert loaded and abs(float(model.logit_scale.detach()) - math.log(1 / 0.07)) < 1e-6
    assert out.count("logit_scale") >= 1 and len([ln for ln in out.splitlines() if "no logit_scale" in ln]) == 1
    key = next(iter(sd))
    assert torch.equal(model.state_dict()[key], sd[key])
    model, _ = load_model_and_checkpoint(_config(on, f"model_config.ckpt_path={with_t}"), cpu)
    assert float(model.logit_scale.detach()) == 3.25
    assert "no logit_scale" not in capsys.readouterr().out
    model, _ = load_model_and_checkpoint(_config(f"model_config.ckpt_path={with_t}"), cpu)
    assert not hasattr(model, "logit_scale") and list(model.state_dict()) == list(sd)
    # any other missing or extra key is still refused
    broken = dict(sd)
    broken.pop(key)
    torch.save(broken, str(tmp_path / "broken.pth"))
    with pytest.raises(RuntimeError, match="does not match"):
        load_model_and_checkpoint(_config(on, f"model_config.ckpt_path={tmp_path / 'broken.pth'}"), cpu)


def test_contrastive_loss_takes_a_float_or_a_parameter():
    from bioscanclip.model.loss_func import ContrastiveLoss, GlobalBatchContrastiveLoss
    t = torch.nn.Parameter(torch.tensor(math.log(1 / 0.07)))
    crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), t)
    assert crit.logit_scale is t
    assert list(crit.parameters()) == [] and "logit_scale" not in crit.state_dict()   # the model owns it
    assert abs(float(crit.current_scale()) - 1 / 0.07) < 1e-5
    fixed = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 20.0)
    assert fixed.logit_scale == 20.0 and float(fixed.current_scale()) == 20.0 and fixed.current_scale().dim() == 0
    with pytest.raises(ValueError, match="not built for more than one rank"):
        GlobalBatchContrastiveLoss(torch.nn.CrossEntropyLoss(), logit_scale=t, overlap=False)
    with pytest.raises(RuntimeError, match="GPU"):   # no CPU compute path for the learnable form either
        crit(torch.zeros(4, 768), torch.zeros(4, 768), None, torch.arange(4))


def test_flat_buffers_finds_the_temperature_buffer():
    """The buffer ``SimpleCLIP.bind_temperature`` builds (here by hand: it needs a GPU parameter) is what ``flat_buffers`` returns."""
    from bioscanclip.hip.dist import flat_buffers
    from bioscanclip.hip.engine import FlatParams
    from bioscanclip.model.simple_clip import SimpleCLIP
    model = SimpleCLIP(None, None, None)
    assert flat_buffers(model) == []
    model.logit_scale = torch.nn.Parameter(torch.tensor(2.5))
    model.bind_temperature()                      # a CPU parameter: nothing to build
    assert flat_buffers(model) == []
    model._temperature_flat = FlatParams([model.logit_scale], torch.device("cpu"))
    (flat,) = flat_buffers(model)
    assert flat.data.numel() == 4 and flat.valid() and float(model.logit_scale.detach()) == 2.5
    flat.grad.fill_(1.5)
    assert float(model.logit_scale.grad) == 1.5 and model.logit_scale.grad.shape == ()


def test_train_cl_refuses_more_than_one_rank(monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="not built for more than one rank"):
        train_cl.main([CONFIG, "model_config.trainable_temperature=true"])
