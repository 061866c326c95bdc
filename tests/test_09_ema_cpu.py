"""The weight average (EMA) of the fused AdamW step without a GPU: ``FusedAdamW``'s launch sequences with the average
on, pinned by tests/golden/optim_ema_trace.json (tools/gen_optim_ema_trace_golden.py; scenarios in tests/optim_ema_trace.py), its
refusals, the ``train_cl`` keys, and the host checks of the two new entry points and their ``ops`` wrappers."""
import ctypes
import json
import os
import sys

import pytest
import torch

from helpers import load_golden
from optim_ema_trace import SCENARIOS, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bioscan-clip_amd")
CONFIG = "model_config=lora_vit_lora_barcode_bert_ssl"

ONE = ctypes.c_void_p(64)        # non-null, 16-byte aligned: never dereferenced on the host
ODD4 = ctypes.c_void_p(68)       # 4-byte aligned only
ODD1 = ctypes.c_void_p(65)       # not even 4-byte aligned


def _ptr(k):
    """Distinct 16-byte-aligned addresses 4 KiB apart: ranges of up to 1024 floats at them share no byte."""
    return ctypes.c_void_p(4096 * (k + 1))


# ------------------------------------------------------------------------------------------------------------ launch traces
@pytest.fixture(scope="module")
def golden():
    return load_golden("optim_ema_trace")


def test_golden_holds_exactly_the_scenarios(golden):
    assert sorted(golden) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_optim_ema_trace(name, golden, monkeypatch):
    from bioscanclip.hip.optim import FusedAdamW
    got, want = json.loads(json.dumps(trace(name, FusedAdamW, monkeypatch.setattr))), golden[name]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}: call {i} differs"
    assert len(got["calls"]) == len(want["calls"]), f"{name}: {len(got['calls'])} calls, golden has {len(want['calls'])}"
    assert got["raises"] is None and want["raises"] is None
    for k, (g, w) in enumerate(zip(got["steps"], want["steps"])):
        assert g == w, f"{name}: state after step {k + 1} differs"
    assert len(got["steps"]) == len(want["steps"]) == 3


def test_every_update_is_one_ema_launch_per_buffer(golden):
    """With the average on ``adamw_step_ema`` replaces the three update entry points in every mode, one launch per flat buffer and
    step; the record pointer is there exactly when clipping is on, and then ``counter_add_if`` stands before each update."""
    for name, rec in golden.items():
        names = [c.split("(")[0] for c in rec["calls"]]
        assert not {"bsclip_adamw_step", "bsclip_adamw_step_dev", "bsclip_adamw_step_clip", "bsclip_swap_f32"} & set(names), name
        assert names.count("bsclip_adamw_step_ema") == 6, name
        clip = "clip" in name
        for i, c in enumerate(rec["calls"]):
            if c.startswith("bsclip_adamw_step_ema("):
                args = c[c.index("(") + 1:-1].split(", ")
                assert (args[7] != "None") == clip, (name, c)
                assert (names[i - 1] == "bsclip_counter_add_if") == clip, (name, i)


def test_the_average_starts_as_the_parameters_and_survives_rebuild_and_checkpoint(golden):
    """The stand-in kernel writes nothing: after the first steps ``st["ema"]`` is the pattern the flat buffers held before the first
    update, and after an engine rebuild / ``load_state_dict`` the pattern written into the average before."""
    first = [" ".join(repr(0.25 * i - (k + 1)) for i in range(n)) for k, n in enumerate((24, 4))]
    for name, rec in golden.items():
        for step in rec["steps"][:2]:
            assert [s["ema"] for s in step] == first, name
    for name in ("rebuild_plain", "rebuild_clip"):
        want = [" ".join(repr(2.0 * i + 0.5) for i in range(1, n + 1)) for n in (24, 4)]
        assert [s["ema"] for s in golden[name]["steps"][2]] == want, name
    # a checkpoint carries the values of the parameters' own elements; the alignment padding between them belongs to no parameter
    got = [s["ema"].split() for s in golden["checkpoint_plain"]["steps"][2]]
    assert got[0][:15] == [repr(2.0 * i + 0.5) for i in range(1, 16)] and got[0][16:23] == [repr(2.0 * i + 0.5) for i in range(17, 24)]
    assert got[1][0] == "2.5"
    for name in ("plain", "device_hyper"):      # without clipping the step word is the host's count, filled eagerly
        assert [s["hyper"][1] for s in golden[name]["steps"][2]] == [3, 3]


# ------------------------------------------------------------------------------------------------------------ refusals
def _two_buffer_optimizer(**kw):
    from bioscanclip.hip.optim import FusedAdamW
    from optim_trace import _optimizer
    return _optimizer(FusedAdamW, "plain", **kw)


def test_set_ema_arguments():
    from bioscanclip.hip.optim import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert not FusedAdamW(p).ema_enabled() and FusedAdamW(p).ema_effective_decay() is None
    opt = FusedAdamW(p, ema_decay=0.999)
    assert opt.ema_enabled() and opt._ema_warmup is True
    assert FusedAdamW(p, ema_decay=0.5, ema_warmup=False)._ema_warmup is False
    assert opt.set_ema(None) is opt and not opt.ema_enabled()
    assert opt.set_ema(0.25, warmup=False).ema_enabled() and opt.ema_effective_decay() == 0.25
    assert opt.set_ema(0.999).ema_effective_decay() == pytest.approx(0.1)      # warm-up, no step applied yet: (1 + 0) / (10 + 0)
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), "x", "0.5", True, False):
        with pytest.raises(ValueError, match=r"ema_decay=.* strictly inside \(0, 1\)"):
            FusedAdamW(p, ema_decay=bad)
        with pytest.raises(ValueError, match=r"ema_decay=.* strictly inside \(0, 1\)"):
            FusedAdamW(p).set_ema(bad)


def test_set_ema_after_a_step_is_refused(monkeypatch):
    from launch_trace import Recorder
    Recorder().install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    for first in (None, 0.999):
        opt = _two_buffer_optimizer().set_ema(first)
        opt.step()
        with pytest.raises(RuntimeError, match="set_ema: call before the first step"):
            opt.set_ema(0.99)
        with pytest.raises(RuntimeError, match="set_ema: call before the first step"):
            opt.set_ema(None)
        assert opt.ema_enabled() == (first is not None)


def test_ema_with_sharded_state_is_refused(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 1)
    opt = _two_buffer_optimizer().set_ema(0.999)
    with pytest.raises(RuntimeError, match=r"EMA.*sharded optimizer state \(shard_state\).*only its slice"):
        opt.shard_state()
    assert opt._shard is None
    opt = _two_buffer_optimizer().shard_state()
    assert opt._shard == (1, 2, None)
    with pytest.raises(RuntimeError, match=r"EMA.*sharded optimizer state \(shard_state\).*only its slice"):
        opt.set_ema(0.999)
    assert not opt.ema_enabled()
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)      # one rank: nothing is sharded, nothing to refuse
    assert _two_buffer_optimizer().set_ema(0.999).shard_state().ema_enabled()


def test_ema_with_a_loose_trainable_tensor_is_refused(monkeypatch):
    from launch_trace import Recorder
    rec = Recorder()
    rec.install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    opt = _two_buffer_optimizer(loose=True).set_ema(0.999)
    with pytest.raises(RuntimeError, match=r"EMA.*every trainable tensor in an engine's flat buffer"):
        opt.step()
    assert rec.calls == []


def test_ema_weights_refusals_and_swaps(monkeypatch):
    from launch_trace import Recorder
    rec = Recorder()
    rec.install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    off = _two_buffer_optimizer()
    with pytest.raises(RuntimeError, match="ema_weights: the weight average is off"):
        with off.ema_weights():
            pass
    opt = _two_buffer_optimizer().set_ema(0.999)
    with opt.ema_weights():                     # before the first step the average equals the weights: nothing is launched
        pass
    assert rec.calls == []
    opt.step()
    rec.calls.clear()
    with pytest.raises(KeyError):               # swapped back also when the body raises
        with opt.ema_weights():
            assert [c[0] for c in rec.calls] == ["bsclip_swap_f32"] * 2
            with pytest.raises(RuntimeError, match="already inside"):
                with opt.ema_weights():
                    pass
            with pytest.raises(RuntimeError, match="no step inside an ema_weights"):
                opt.step()
            raise KeyError("body")
    assert [c[0] for c in rec.calls] == ["bsclip_swap_f32"] * 4
    assert [c[1][2] for c in rec.calls] == ["24", "4", "24", "4"]
    assert rec.calls[0][1][:2] == rec.calls[2][1][:2] and rec.calls[0][1][0] != rec.calls[0][1][1]
    opt.step()                                  # and the optimizer steps again


def test_effective_decay_follows_the_step_count(monkeypatch):
    from launch_trace import Recorder
    Recorder().install(monkeypatch.setattr)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    opt = _two_buffer_optimizer().set_ema(0.5)
    want = [2 / 11, 3 / 12, 4 / 13, 5 / 14, 6 / 15, 7 / 16, 8 / 17, 9 / 18, 0.5, 0.5]     # (1 + t) / (10 + t) reaches 1/2 at t = 8
    for t, w in enumerate(want, start=1):
        opt.step()
        assert opt.ema_effective_decay() == pytest.approx(w, abs=1e-15), t


# ------------------------------------------------------------------------------------------------------------ train_cl keys
def _config(*extra):
    from bioscanclip.util.config import load_config
    return load_config(os.path.join(PKG, "bioscanclip", "config"), [CONFIG, *extra])


def test_train_cl_ema_options():
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl
    assert train_cl.ema_options(_config()) == (None, True)                                          # absent: off
    assert train_cl.ema_options(_config("model_config.ema_decay=0.999")) == (0.999, True)
    assert train_cl.ema_options(_config("model_config.ema_decay=0.5", "model_config.ema_warmup=false")) == (0.5, False)
    assert train_cl.ema_options(_config("model_config.ema_decay=0.9999", "model_config.ema_warmup=true")) == (0.9999, True)
    assert train_cl.ema_options(_config("model_config.ema_warmup=false")) == (None, False)
    for bad in ("0", "1", "1.0", "0.0", "-0.1", "1.5", ".nan", "x", "true"):
        with pytest.raises(ValueError, match="ema_decay"):
            train_cl.ema_options(_config(f"model_config.ema_decay={bad}"))
    for bad in ("maybe", "2"):
        with pytest.raises(ValueError, match="ema_warmup"):
            train_cl.ema_options(_config("model_config.ema_decay=0.999", f"model_config.ema_warmup={bad}"))
    # sharded optimizer state: more than one rank AND full fine-tuning
    sharded = _config("model_config.ema_decay=0.999", "model_config.disable_lora=true")
    assert train_cl.ema_options(sharded, 1) == (0.999, True)
    assert train_cl.ema_options(_config("model_config.ema_decay=0.999"), 8) == (0.999, True)
    assert train_cl.ema_options(_config("model_config.disable_lora=true"), 8) == (None, True)
    with pytest.raises(ValueError, match=r"ema_decay.*sharded optimizer state.*world_size=8"):
        train_cl.ema_options(sharded, 8)


@pytest.mark.parametrize("extra, env, match", [(["model_config.ema_decay=1.0"], {}, "ema_decay must be a number strictly inside"),
                                               (["model_config.ema_decay=0.999", "model_config.disable_lora=true"],
                                                {"WORLD_SIZE": "2", "RANK": "0"}, "sharded optimizer state")])
def test_train_cl_refuses_before_the_model_is_built(extra, env, match, monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl

    def never(*a, **k):
        raise AssertionError("the model must not be built")

    monkeypatch.setattr(train_cl, "load_clip_model", never)
    monkeypatch.setattr(train_cl, "main_process", never)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(ValueError, match=match):
        train_cl.main([CONFIG, *extra])


# ------------------------------------------------------------------------------------------------------------ host checks
def _refused(rc, *words):
    from bioscanclip.hip import lib
    assert rc == -1
    msg = lib.last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_adamw_step_ema_host_validation():
    from bioscanclip.hip import lib
    h = lib.load()
    name = "bsclip_adamw_step_ema"
    base = dict(p=_ptr(0), g=_ptr(1), m=_ptr(2), v=_ptr(3), ema=_ptr(4), n=8, hyper=ONE, state=None, decay=0.999, warm=1)

    def call(**kw):
        a = dict(base, **kw)
        return h.bsclip_adamw_step_ema(a["p"], a["g"], a["m"], a["v"], a["ema"], a["n"], a["hyper"], a["state"], 0.9, 0.999, 1e-8, 0.01,
                                       a["decay"], a["warm"], None)

    for k in ("p", "g", "m", "v"):
        _refused(call(**{k: None}), name, "p, g, m, v")
        _refused(call(**{k: ODD1}), name, "4-byte aligned")
    _refused(call(ema=None), name, "ema is null")
    _refused(call(ema=ODD1), name, "4-byte aligned")
    _refused(call(hyper=None), name, "hyper_dev is null")
    _refused(call(state=ODD4), name, "clip_state must be 16-byte aligned")
    _refused(call(n=0), name, "n=0")
    _refused(call(n=-1), name, "n=-1")
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        _refused(call(decay=bad), name, "ema_decay", "strictly inside (0, 1)")
    for k in ("p", "g", "m", "v"):      # the same range, and a range that starts inside the other's n floats
        _refused(call(ema=base[k]), name, "ema must not alias")
        _refused(call(ema=ctypes.c_void_p(base[k].value + 28)), name, "ema must not alias")
        _refused(call(ema=ctypes.c_void_p(base[k].value - 28)), name, "ema must not alias")


def test_swap_f32_host_validation():
    from bioscanclip.hip import lib
    h = lib.load()
    name = "bsclip_swap_f32"
    a, b = _ptr(0), _ptr(1)
    _refused(h.bsclip_swap_f32(None, b, 8, None), name, "null pointer")
    _refused(h.bsclip_swap_f32(a, None, 8, None), name, "null pointer")
    _refused(h.bsclip_swap_f32(a, b, 0, None), name, "n=0")
    _refused(h.bsclip_swap_f32(a, b, -2, None), name, "n=-2")
    _refused(h.bsclip_swap_f32(ODD1, b, 8, None), name, "4-byte aligned")
    _refused(h.bsclip_swap_f32(a, ODD1, 8, None), name, "4-byte aligned")
    _refused(h.bsclip_swap_f32(a, a, 8, None), name, "same or overlapping")
    _refused(h.bsclip_swap_f32(a, ctypes.c_void_p(a.value + 28), 8, None), name, "same or overlapping")
    _refused(h.bsclip_swap_f32(ctypes.c_void_p(a.value + 4), a, 8, None), name, "same or overlapping")
    _refused(h.bsclip_swap_f32(a, b, 1025, None), name, "same or overlapping")     # 4 KiB apart: 1025 floats reach into b


def test_ops_wrappers_host_checks(monkeypatch):
    from launch_trace import Recorder
    from bioscanclip.hip import ops
    rec = Recorder()
    rec.install(monkeypatch.setattr)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32)
    p, g, m, v, ema = (f32(8) for _ in range(5))
    hyper, state = torch.zeros(2, dtype=torch.int32), torch.zeros(12, dtype=torch.int32)
    args = (0.9, 0.999, 1e-8, 0.01, 0.999, True)
    ops.adamw_step_ema(p, g, m, v, ema, hyper, None, *args)
    ops.adamw_step_ema(p, g, m, v, ema, hyper, state, *args)
    assert [c[0] for c in rec.calls] == ["bsclip_adamw_step_ema"] * 2 and rec.calls[0][1][7] == "None" and rec.calls[1][1][7] != "None"
    assert rec.calls[0][1][-3:] == ["0.999", "1", "None"]
    for k, other in enumerate((p, g, m, v)):
        with pytest.raises(ValueError, match="ema must not alias"):
            ops.adamw_step_ema(p, g, m, v, other, hyper, None, *args)
    big = f32(16)
    with pytest.raises(ValueError, match="ema must not alias"):          # views of one storage that overlap
        ops.adamw_step_ema(big[:8], g, m, v, big[4:12], hyper, None, *args)
    with pytest.raises(ValueError, match="ema must be a flat f32 buffer of p's size"):
        ops.adamw_step_ema(p, g, m, v, f32(7), hyper, None, *args)
    with pytest.raises(ValueError, match="ema must be a flat f32 buffer of p's size"):
        ops.adamw_step_ema(p, g, m, v, torch.zeros(8, dtype=torch.float64), hyper, None, *args)
    with pytest.raises(ValueError, match="ema must be a flat f32 buffer of p's size"):
        ops.adamw_step_ema(p, g, m, v, f32(16)[::2], hyper, None, *args)
    with pytest.raises(ValueError, match="flat f32 buffers"):
        ops.adamw_step_ema(p, f32(9), m, v, ema, hyper, None, *args)
    with pytest.raises(ValueError, match="hyper must be a device pair"):
        ops.adamw_step_ema(p, g, m, v, ema, torch.zeros(1, dtype=torch.int32), None, *args)
    with pytest.raises(ValueError, match="adamw_step_ema: state must be"):
        ops.adamw_step_ema(p, g, m, v, ema, hyper, torch.zeros(4, dtype=torch.int32), *args)
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError, match="ema_decay"):
            ops.adamw_step_ema(p, g, m, v, ema, hyper, None, 0.9, 0.999, 1e-8, 0.01, bad, True)
    n_calls = len(rec.calls)
    a, b = f32(8), f32(8)
    ops.swap_f32(a, b)
    assert rec.calls[-1][0] == "bsclip_swap_f32" and rec.calls[-1][1][2] == "8"
    ops.swap_f32(big[:8], big[8:])                                           # neighbours in one storage share no byte
    for x, y, msg in ((a, a, "same or overlapping"), (big[:8], big[4:12], "same or overlapping"), (a, f32(9), "same non-zero size"),
                      (a, torch.zeros(8, dtype=torch.float64), "f32 buffers"), (torch.zeros(8, dtype=torch.int32), b, "f32 buffers"),
                      (f32(16)[::2], b, "contiguous"), (f32(0), f32(0), "non-zero size")):
        with pytest.raises(ValueError, match=msg):
            ops.swap_f32(x, y)
    assert len(rec.calls) == n_calls + 2
