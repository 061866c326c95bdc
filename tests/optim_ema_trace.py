"""``FusedAdamW``'s eager launch sequences with the weight average (EMA) on, recorded without a GPU: tests/optim_trace.py's
two-buffer set-up and its helpers, with ``set_ema`` called before the first step.

``trace(name, FusedAdamW, setattr_)`` returns what tests/golden/optim_ema_trace.json pins (tools/gen_optim_ema_trace_golden.py writes
it, tests/test_09_ema_cpu.py compares): ``calls`` and ``raises`` as in tests/optim_trace.py, and in ``steps`` after every step per flat
buffer additionally ``ema``, the average itself.  The kernel is the stand-in, so the average stays what the host left there: the
parameters as the first step found them (the ``copy_`` at allocation really runs; ``PARAMS`` writes a pattern into the flat buffers
first), and after an engine rebuild / a ``load_state_dict`` the pattern written into it before.
"""
import torch

from launch_trace import Recorder
from optim_trace import CPU, LR_BEFORE_STEP_2, _optimizer, _pattern, _snapshot

# name -> (kind, mode of tests/optim_trace.py, ema_decay, ema_warmup)
SCENARIOS = {"plain": ("steps", "plain", 0.999, True), "device_hyper": ("steps", "device_hyper", 0.9999, False),
             "clip": ("steps", "clip", 0.999, True), "device_hyper_and_clip": ("steps", "device_hyper_and_clip", 0.99, False),
             "rebuild_plain": ("rebuild", "plain", 0.999, True), "rebuild_clip": ("rebuild", "clip", 0.999, True),
             "checkpoint_plain": ("checkpoint", "plain", 0.999, True)}


def _params(opt):
    """A pattern in every flat buffer (the parameters are views of it): what the average starts as."""
    for k, f in enumerate(opt._flats):
        f.data.copy_(torch.arange(f.data.numel(), dtype=torch.float32) * 0.25 - (k + 1))


def _ema_pattern(st):
    st["ema"].copy_(torch.arange(1, st["ema"].numel() + 1, dtype=torch.float32) * 2.0 + 0.5)


def _snapshot_ema(opt, moments):
    out = _snapshot(opt, moments)
    for s, st in zip(out, opt._flat_state.values()):
        s["ema"] = " ".join(repr(x) for x in st["ema"].tolist())
    return out


def trace(name, FusedAdamW, setattr_):
    """One scenario's record.  ``setattr_(target, name, value)``: ``monkeypatch.setattr`` in a test."""
    from bioscanclip.hip import ops
    kind, mode, decay, warmup = SCENARIOS[name]
    rec = Recorder()
    rec.install(setattr_)
    setattr_(torch.cuda, "is_current_stream_capturing", lambda: False)
    setattr_(ops, "grad_norm_partials", lambda n: max(1, -(-int(n) // 8192)))
    opt = _optimizer(FusedAdamW, mode).set_ema(decay, warmup)
    _params(opt)
    moments = kind in ("rebuild", "checkpoint")
    steps, raises = [], None
    for k in (1, 2, 3):
        if k == 2:
            opt.param_groups[0]["lr"] = LR_BEFORE_STEP_2
        if k == 3 and moments:
            for st in opt._flat_state.values():
                _pattern(st)
                _ema_pattern(st)
                if "hyper" in st and opt.grad_clip_enabled():
                    st["hyper"][1:2].fill_(2)      # what the two recorded counter_add_if launches would have left
            if kind == "rebuild":
                from bioscanclip.hip.engine import FlatParams
                opt._flats = [FlatParams(f.params, CPU) for f in opt._flats]
            else:
                sd = opt.state_dict()
                opt = _optimizer(FusedAdamW, mode).set_ema(decay, warmup)
                opt.load_state_dict(sd)
        try:
            opt.step()
        except RuntimeError as e:
            raises = str(e)
            break
        steps.append(_snapshot_ema(opt, moments))
    return {"calls": rec.lines(), "steps": steps, "raises": raises}
