"""Gradient-norm clipping and overflow-safe steps without a GPU: the host validation of the new entry points, the
partial-count query, the ``train_cl`` keys and ``FusedAdamW``'s refusals."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bioscan-clip_amd")
CONFIG = "model_config=lora_vit_lora_barcode_bert_ssl"

ONE = ctypes.c_void_p(64)        # non-null, 16-byte aligned: never dereferenced on the host
ODD4 = ctypes.c_void_p(68)       # 4-byte aligned only
ODD1 = ctypes.c_void_p(65)       # not even 4-byte aligned


def _refused(rc, *words):
    from bioscanclip.hip import lib
    assert rc == -1
    msg = lib.last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_grad_sumsq_partial_host_validation():
    from bioscanclip.hip import lib
    h = lib.load()
    name = "bsclip_grad_sumsq_partial"
    _refused(h.bsclip_grad_sumsq_partial(None, 8, ONE, None), name, "g is null")
    _refused(h.bsclip_grad_sumsq_partial(ONE, 8, None, None), name, "partial is null")
    _refused(h.bsclip_grad_sumsq_partial(ONE, 0, ONE, None), name, "n=0")
    _refused(h.bsclip_grad_sumsq_partial(ONE, -3, ONE, None), name, "n=-3")
    _refused(h.bsclip_grad_sumsq_partial(ODD4, 8, ONE, None), name, "g must be 16-byte aligned")
    _refused(h.bsclip_grad_sumsq_partial(ONE, 8, ODD4, None), name, "partial must be 8-byte aligned")


def test_grad_clip_finish_host_validation():
    from bioscanclip.hip import lib
    h = lib.load()
    name = "bsclip_grad_clip_finish"
    _refused(h.bsclip_grad_clip_finish(None, 4, 1.0, ONE, None), name, "partial is null")
    _refused(h.bsclip_grad_clip_finish(ONE, 4, 1.0, None, None), name, "state is null")
    _refused(h.bsclip_grad_clip_finish(ONE, 0, 1.0, ONE, None), name, "n_partial=0")
    _refused(h.bsclip_grad_clip_finish(ODD4, 4, 1.0, ONE, None), name, "partial must be 8-byte aligned")
    _refused(h.bsclip_grad_clip_finish(ONE, 4, 1.0, ODD4, None), name, "state must be 16-byte aligned")
    for bad in (0.0, -1.0, float("-inf"), float("nan")):
        _refused(h.bsclip_grad_clip_finish(ONE, 4, bad, ONE, None), name, "max_norm")


def test_counter_add_if_host_validation():
    from bioscanclip.hip import lib
    h = lib.load()
    name = "bsclip_counter_add_if"
    _refused(h.bsclip_counter_add_if(None, 1, ONE, None), name, "counter is null")
    _refused(h.bsclip_counter_add_if(ONE, 1, None, None), name, "cond is null")
    _refused(h.bsclip_counter_add_if(ODD1, 1, ONE, None), name, "4-byte aligned")
    _refused(h.bsclip_counter_add_if(ONE, 1, ODD1, None), name, "4-byte aligned")


def test_adamw_step_clip_host_validation():
    from bioscanclip.hip import lib
    h = lib.load()
    name = "bsclip_adamw_step_clip"

    def call(p=ONE, g=ONE, m=ONE, v=ONE, n=8, hyper=ONE, state=ONE):
        return h.bsclip_adamw_step_clip(p, g, m, v, n, hyper, state, 0.9, 0.999, 1e-8, 0.01, None)

    for k in ("p", "g", "m", "v"):
        _refused(call(**{k: None}), name, "p, g, m, v")
        _refused(call(**{k: ODD1}), name, "4-byte aligned")
    _refused(call(hyper=None), name, "hyper_dev is null")
    _refused(call(state=None), name, "state is null")
    _refused(call(state=ODD4), name, "state must be 16-byte aligned")
    _refused(call(n=0), name, "n=0")
    _refused(call(n=-1), name, "n=-1")


def test_grad_norm_partials_is_positive_monotone_and_capped():
    from bioscanclip.hip import lib, ops
    h = lib.load()
    assert h.bsclip_grad_norm_partials(0) == -1 and "n=0" in lib.last_error()
    assert h.bsclip_grad_norm_partials(-5) == -1
    with pytest.raises(ValueError, match="positive"):
        ops.grad_norm_partials(0)
    sizes = sorted({1, 3, 4, 5, 255, 1024, 1025, *(2 ** k + d for k in range(2, 36) for d in (-1, 0, 1))})
    counts = [h.bsclip_grad_norm_partials(n) for n in sizes]
    assert counts[0] == 1 and all(c >= 1 for c in counts)
    assert all(a <= b for a, b in zip(counts, counts[1:]))                     # monotone in n
    cap = counts[-1]
    assert cap == h.bsclip_grad_norm_partials(2 ** 40) and 1 < cap <= 4096     # capped: a huge buffer gets no more workgroups
    assert [h.bsclip_grad_norm_partials(n) for n in sizes] == counts           # a pure function of n
    assert ops.grad_norm_partials(1025) == h.bsclip_grad_norm_partials(1025)


def _config(*extra):
    from bioscanclip.util.config import load_config
    return load_config(os.path.join(PKG, "bioscanclip", "config"), [CONFIG, *extra])


def test_train_cl_grad_clip_options():
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl
    assert train_cl.grad_clip_options(_config()) == (None, False)                                       # absent: off
    assert train_cl.grad_clip_options(_config("model_config.grad_clip_norm=0.5")) == (0.5, True)
    assert train_cl.grad_clip_options(_config("model_config.grad_clip_norm=2")) == (2.0, True)
    assert train_cl.grad_clip_options(_config("model_config.skip_nonfinite_steps=true")) == (None, True)
    assert train_cl.grad_clip_options(_config("model_config.skip_nonfinite_steps=false")) == (None, False)
    assert train_cl.grad_clip_options(_config("model_config.grad_clip_norm=1.5", "model_config.skip_nonfinite_steps=false")) == (1.5, True)
    for bad in ("0", "-1.0", "0.0", ".nan", "abc", "true"):
        with pytest.raises(ValueError, match="grad_clip_norm"):
            train_cl.grad_clip_options(_config(f"model_config.grad_clip_norm={bad}"))


def test_train_cl_refuses_a_bad_norm_before_the_model_is_built(monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl

    def never(*a, **k):
        raise AssertionError("the model must not be built")

    monkeypatch.setattr(train_cl, "load_clip_model", never)
    monkeypatch.setattr(train_cl, "main_process", never)
    with pytest.raises(ValueError, match="grad_clip_norm"):
        train_cl.main([CONFIG, "model_config.grad_clip_norm=-0.5"])


def test_fused_adamw_grad_clip_arguments():
    from bioscanclip.hip.optim import FusedAdamW
    params = lambda: [torch.nn.Parameter(torch.zeros(4))]
    plain = FusedAdamW(params(), lr=1e-3)
    assert not plain.grad_clip_enabled()
    assert FusedAdamW(params(), max_grad_norm=None, skip_nonfinite=False).grad_clip_enabled() is False
    on = FusedAdamW(params(), lr=1e-3, max_grad_norm=0.5, skip_nonfinite=True)
    assert on.grad_clip_enabled() and on._max_norm == 0.5
    monitor = FusedAdamW(params(), skip_nonfinite=True)
    assert monitor.grad_clip_enabled() and monitor._max_norm == math.inf
    with pytest.raises(ValueError, match="skip_nonfinite"):      # a non-finite norm cannot be clipped
        FusedAdamW(params(), max_grad_norm=1.0)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        plain.set_grad_clip(1.0, skip_nonfinite=False)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW(params(), max_grad_norm=bad, skip_nonfinite=True)
        with pytest.raises(ValueError, match="max_grad_norm"):
            plain.set_grad_clip(bad)
    assert not plain.grad_clip_enabled()                         # a refused call changes nothing
    assert plain.set_grad_clip(2.0) is plain and plain.grad_clip_enabled() and plain._max_norm == 2.0   # skip_nonfinite defaults to on
    plain.set_grad_clip(None, skip_nonfinite=False)
    assert not plain.grad_clip_enabled()
    stats = on.grad_stats()                                      # before the first step: nothing seen
    assert set(stats) == {"steps", "skipped", "clipped", "norm_mean", "norm_max", "norm_last", "coef_last"}
    assert stats["steps"] == stats["skipped"] == stats["clipped"] == 0


def test_step_without_the_options_launches_what_it_always_did():
    """With the options off ``step()`` is the plain optimizer: one ``bsclip_adamw_step`` per flat buffer, none of the new entry points
    (recorded without a GPU through tests/launch_trace.py)."""
    from launch_trace import recording
    from bioscanclip.hip.engine import FlatParams
    from bioscanclip.hip.optim import FusedAdamW
    cpu = torch.device("cpu")
    groups = [[torch.nn.Parameter(torch.zeros(5, 3)), torch.nn.Parameter(torch.zeros(7))], [torch.nn.Parameter(torch.zeros(()))]]
    opt = FusedAdamW([p for g in groups for p in g], lr=1e-3)
    opt._flats = [FlatParams(g, cpu) for g in groups]
    with recording() as rec:
        opt.step()
        opt.step()
    names = [name for name, _ in rec.calls]
    assert names == ["bsclip_adamw_step"] * 4
    assert [args[10] for _, args in rec.calls] == ["1", "1", "2", "2"]       # the host step count travels as an argument
