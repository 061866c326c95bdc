"""The sigmoid (SigLIP) contrastive loss (``model_config.contrastive_loss: sigmoid``) without a GPU: the host validation of
``bsclip_sigmoid_loss_fwd_bwd``, its ctypes row against the header, the config key, the ``logit_scale`` / ``logit_bias`` parameters of
``load_clip_model``, checkpoints with and without them on both kinds of model, the flat buffer, and the refusal of more than one rank."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

from helpers import skip_param_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bioscan-clip_amd")
CONFIG = "model_config=lora_vit_lora_barcode_bert_ssl"
SIGMOID = "model_config.contrastive_loss=sigmoid"
LN10 = math.log(10.0)


def test_host_validation_names_the_argument():
    """Every bad argument is refused with -1 before any launch (there is no GPU here), and the message says which one."""
    from bioscanclip.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(16)                      # non-null, 16-byte aligned: never dereferenced on the host
    ptrs = lambda n, v=16: (ctypes.c_void_p * n)(*[v] * n)

    def call(nmod=2, N=8, D=768, row0=0, n_local=8, z="ok", labels=one, log_scale=one, bias=one, loss=one, dz="ok", aux=one,
             workspace=one):
        z = ptrs(max(nmod, 1)) if z == "ok" else z
        dz = ptrs(max(nmod, 1)) if dz == "ok" else dz
        return h.bsclip_sigmoid_loss_fwd_bwd(z, nmod, labels, N, D, log_scale, bias, row0, n_local, loss, dz, aux, workspace, None)

    cases = [(dict(log_scale=None), ["log_scale_dev"]),
             (dict(bias=None), ["bias_dev"]),
             (dict(aux=None), ["aux_out"]),
             (dict(log_scale=ctypes.c_void_p(18)), ["log_scale_dev", "4-B"]),
             (dict(bias=ctypes.c_void_p(18)), ["bias_dev", "4-B"]),
             (dict(aux=ctypes.c_void_p(18)), ["aux_out", "4-B"]),
             (dict(z=None), ["z is null"]),
             (dict(labels=None), ["labels"]),
             (dict(loss=None), ["loss_out"]),
             (dict(workspace=None), ["workspace"]),
             (dict(workspace=ctypes.c_void_p(20)), ["workspace", "16-B"]),
             (dict(D=512), ["D=512"]),
             (dict(row0=4, n_local=5), ["row0=4", "n_local=5"]),
             (dict(N=0, n_local=0), ["N=0"]),
             (dict(N=16385, n_local=8), ["N=16385"]),
             (dict(nmod=1), ["nmod=1", "Too less element"]),
             (dict(nmod=4), ["nmod=4"]),
             (dict(z=(ctypes.c_void_p * 2)(16, None)), ["z[1]"]),
             (dict(z=(ctypes.c_void_p * 2)(16, 24)), ["z[1]", "16-B"]),
             (dict(dz=(ctypes.c_void_p * 2)(16, None)), ["dz[1]"]),
             (dict(dz=(ctypes.c_void_p * 2)(16, 24)), ["dz[1]", "16-B"])]
    for kw, words in cases:
        assert call(**kw) == -1, kw
        msg = lib.last_error()
        assert "bsclip_sigmoid_loss_fwd_bwd" in msg, (kw, msg)
        for w in words:
            assert w in msg, (kw, msg)


def test_ctypes_row_matches_the_header():
    """The argument list of the header's declaration, type by type, is the ctypes row; the ABI version stays 10."""
    from bioscanclip.hip import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsclip.h")).read(), flags=re.S)
    m = re.search(r"int\s+bsclip_sigmoid_loss_fwd_bwd\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["z", "nmod", "labels", "N", "D", "log_scale_dev", "bias_dev", "row0", "n_local", "loss_out", "dz", "aux_out",
                     "workspace", "stream"]

    def ctype(a):
        if "* const*" in a:
            return ctypes.POINTER(ctypes.c_void_p)
        return ctypes.c_void_p if "*" in a else ctypes.c_int

    restype, argtypes = lib.SIGNATURES["bsclip_sigmoid_loss_fwd_bwd"]
    assert restype is ctypes.c_int and list(argtypes) == [ctype(a) for a in args]
    assert lib.load().bsclip_abi_version() == 10


def _config(*extra):
    from bioscanclip.util.config import load_config
    return load_config(os.path.join(PKG, "bioscanclip", "config"), [CONFIG, *extra])


def _load(*extra):
    from bioscanclip.model.simple_clip import load_clip_model
    with skip_param_init():
        return load_clip_model(_config(*extra))


def test_contrastive_loss_key_parsing():
    from bioscanclip.model.simple_clip import contrastive_loss_kind, sigmoid_init
    assert contrastive_loss_kind(_config()) == "infonce"
    assert contrastive_loss_kind(_config("model_config.contrastive_loss=infonce")) == "infonce"
    assert contrastive_loss_kind(_config(SIGMOID)) == "sigmoid"
    with pytest.raises(ValueError, match="contrastive_loss"):
        contrastive_loss_kind(_config("model_config.contrastive_loss=triplet"))
    with pytest.raises(ValueError, match="trainable_temperature"):
        contrastive_loss_kind(_config(SIGMOID, "model_config.trainable_temperature=true"))
    assert sigmoid_init(_config(SIGMOID)) == (LN10, -10.0)
    assert sigmoid_init(_config(SIGMOID, "model_config.sigmoid_log_scale=1.5", "model_config.sigmoid_bias=-4")) == (1.5, -4.0)


def test_load_clip_model_creates_the_parameters_only_for_sigmoid():
    on = _load(SIGMOID)
    params = dict(on.named_parameters())
    for key, want in (("logit_scale", LN10), ("logit_bias", -10.0)):
        p = params[key]
        assert p.requires_grad and p.dtype == torch.float32 and p.shape == ()
        assert torch.equal(on.state_dict()[key], torch.tensor(want))
    absent = _load()
    infonce = _load("model_config.contrastive_loss=infonce")
    for m in (absent, infonce):
        assert not hasattr(m, "logit_scale") and not hasattr(m, "logit_bias")
    assert list(infonce.state_dict()) == list(absent.state_dict())
    assert sorted(on.state_dict()) == sorted(list(absent.state_dict()) + ["logit_scale", "logit_bias"])
    over = _load(SIGMOID, "model_config.sigmoid_log_scale=2.0", "model_config.sigmoid_bias=-3.5")
    assert float(over.logit_scale.detach()) == 2.0 and float(over.logit_bias.detach()) == -3.5
    # the learnable temperature alone still brings no bias
    temp = _load("model_config.trainable_temperature=true")
    assert hasattr(temp, "logit_scale") and not hasattr(temp, "logit_bias")
    with pytest.raises(ValueError, match="contrastive_loss"):
        _load("model_config.contrastive_loss=hinge")


def test_criterion_refuses_more_than_one_rank_and_too_few_modalities():
    from bioscanclip.model.loss_func import SigmoidContrastiveLoss
    t, b = torch.nn.Parameter(torch.tensor(LN10)), torch.nn.Parameter(torch.tensor(-10.0))
    crit = SigmoidContrastiveLoss(t, b)
    assert crit.logit_scale is t and crit.logit_bias is b
    assert list(crit.parameters()) == [] and not crit.state_dict()          # the model owns both
    assert abs(float(crit.current_scale()) - 10.0) < 1e-5 and float(crit.current_bias()) == -10.0
    with pytest.raises(ValueError, match="not built for more than one rank"):
        SigmoidContrastiveLoss(t, b, world_size=2)
    with pytest.raises(ValueError, match="Too less element for calculating the contrastive loss."):
        crit(torch.zeros(4, 768), None, None, torch.arange(4))
    with pytest.raises(RuntimeError, match="GPU"):                           # no CPU compute path
        crit(torch.zeros(4, 768), torch.zeros(4, 768), None, torch.arange(4))
    with pytest.raises(TypeError, match="logit_bias"):
        SigmoidContrastiveLoss(t, -10.0)


def test_train_cl_refuses_more_than_one_rank_before_the_model_is_built(monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(train_cl, "load_clip_model", lambda *a, **k: pytest.fail("the model was built"))
    with pytest.raises(ValueError, match="not built for more than one rank"):
        train_cl.main([CONFIG, SIGMOID])
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(ValueError, match="contrastive_loss"):
        train_cl.main([CONFIG, "model_config.contrastive_loss=margin"])


def test_checkpoints_with_and_without_the_scalars(tmp_path, monkeypatch, capsys):
    """Loading tolerates the two keys' absence or presence on both kinds of model: a sigmoid model keeps its initial values when the
    checkpoint lacks them (one line each) and restores them when it has them; a default model ignores them; anything else missing is
    still refused."""
    from bioscanclip.model import simple_clip
    from bioscanclip.util.util import load_model_and_checkpoint
    plain = _load()
    sd = {k: v.clone() for k, v in plain.state_dict().items()}
    without, with_tb, with_t = (str(tmp_path / n) for n in ("without.pth", "with_tb.pth", "with_t.pth"))
    torch.save(sd, without)
    torch.save(dict(sd, logit_scale=torch.tensor(3.25), logit_bias=torch.tensor(-7.5)), with_tb)
    torch.save(dict(sd, logit_scale=torch.tensor(3.25)), with_t)
    real = simple_clip.load_clip_model

    def quick(args, device=None):
        with skip_param_init():
            return real(args, device)

    monkeypatch.setattr(simple_clip, "load_clip_model", quick)
    cpu = torch.device("cpu")
    capsys.readouterr()
    model, loaded = load_model_and_checkpoint(_config(SIGMOID, f"model_config.ckpt_path={without}"), cpu)
    out = capsys.readouterr().out
    assert loaded and float(model.logit_scale.detach()) == torch.tensor(LN10).item() and float(model.logit_bias.detach()) == -10.0
    assert len([ln for ln in out.splitlines() if "no logit_scale" in ln]) == 1
    assert len([ln for ln in out.splitlines() if "no logit_bias" in ln]) == 1
    key = next(iter(sd))
    assert torch.equal(model.state_dict()[key], sd[key])
    model, _ = load_model_and_checkpoint(_config(SIGMOID, f"model_config.ckpt_path={with_tb}"), cpu)
    assert float(model.logit_scale.detach()) == 3.25 and float(model.logit_bias.detach()) == -7.5
    assert "has no" not in capsys.readouterr().out
    model, _ = load_model_and_checkpoint(_config(SIGMOID, f"model_config.ckpt_path={with_t}"), cpu)     # a temperature-only checkpoint
    assert float(model.logit_scale.detach()) == 3.25 and float(model.logit_bias.detach()) == -10.0
    model, _ = load_model_and_checkpoint(_config(f"model_config.ckpt_path={with_tb}"), cpu)             # the default model ignores both
    assert not hasattr(model, "logit_scale") and not hasattr(model, "logit_bias") and list(model.state_dict()) == list(sd)
    model, _ = load_model_and_checkpoint(_config("model_config.trainable_temperature=true", f"model_config.ckpt_path={with_tb}"), cpu)
    assert float(model.logit_scale.detach()) == 3.25 and not hasattr(model, "logit_bias")
    broken = dict(sd)
    broken.pop(key)
    torch.save(broken, str(tmp_path / "broken.pth"))
    with pytest.raises(RuntimeError, match="does not match"):
        load_model_and_checkpoint(_config(SIGMOID, f"model_config.ckpt_path={tmp_path / 'broken.pth'}"), cpu)


def test_flat_buffer_of_one_and_of_two_scalars():
    """A temperature-only model still binds a 4-float buffer; with the bias it is 8 floats, t at 0 and b at 4, and ``flat_buffers``
    returns it.  (``bind_temperature`` itself needs GPU parameters: the buffers are built by hand here, as it builds them.)"""
    from bioscanclip.hip.dist import flat_buffers
    from bioscanclip.hip.engine import FlatParams
    from bioscanclip.model.simple_clip import SimpleCLIP
    model = SimpleCLIP(None, None, None)
    model.logit_scale = torch.nn.Parameter(torch.tensor(2.5))
    model.bind_temperature()                      # CPU parameters: nothing to build
    assert flat_buffers(model) == []
    model._temperature_flat = FlatParams([model.logit_scale], torch.device("cpu"))
    (flat,) = flat_buffers(model)
    assert flat.data.numel() == 4 and flat.valid()
    both = SimpleCLIP(None, None, None)
    both.logit_scale = torch.nn.Parameter(torch.tensor(LN10))
    both.logit_bias = torch.nn.Parameter(torch.tensor(-10.0))
    both.bind_temperature()
    assert flat_buffers(both) == []
    both._temperature_flat = FlatParams([both.logit_scale, both.logit_bias], torch.device("cpu"))
    (flat,) = flat_buffers(both)
    assert flat.data.numel() == 8 and flat.offsets == [0, 4] and flat.valid()
    assert flat.data.tolist() == [torch.tensor(LN10).item(), 0, 0, 0, -10.0, 0, 0, 0]
    flat.grad[4] = 1.5
    assert float(both.logit_bias.grad) == 1.5 and float(both.logit_scale.grad) == 0.0 and both.logit_bias.grad.shape == ()
