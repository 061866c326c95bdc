"""``FusedAdamW``'s eager launch sequences, recorded without a GPU (tests/launch_trace.py stands in for the library).

``trace(name, FusedAdamW, setattr_)`` runs one scenario of ``SCENARIOS`` on CPU tensors and returns what
tests/golden/optim_trace.json pins (tools/gen_optim_trace_golden.py writes it, tests/test_09_optim_trace_cpu.py compares):

    calls   ``Recorder.lines()`` of every step, with a ``sync_updated_slices()`` line where the sharded optimizer broadcasts
    steps   after every step, per entry of ``_flat_state`` in its order: the host's ``step``, the two ``hyper`` words (lr bits, step
            word; the ``fill_`` calls really run on CPU tensors), ``lr_staged``, when sharded ``slice``, and in the scenarios that write
            a pattern into them the moments
    raises  the message of the step that refused, or None

Two flat buffers, ``FlatParams([5x3, 7])`` = 24 floats and ``FlatParams([scalar])`` = 4 floats, each in a param group of its own with
its own lr, betas, eps and weight decay; three steps, ``param_groups[0]["lr"]`` changed before the second.  The capture-time branches
(the ``counter_add`` node, no lr staging, no allocation) are not reachable on CPU tensors: tests/test_30 and tests/test_31 pin them on
the GPU, replay against eager bit for bit.
"""
import torch

from launch_trace import Recorder

CPU = torch.device("cpu")
MODES = {"plain": {}, "device_hyper": {"device_hyper": True}, "clip": {"max_grad_norm": 0.5, "skip_nonfinite": True},
         "monitor": {"skip_nonfinite": True}, "device_hyper_and_clip": {"device_hyper": True, "max_grad_norm": 0.5, "skip_nonfinite": True}}
# name -> (kind, mode)
SCENARIOS = {m: ("steps", m) for m in MODES}
SCENARIOS.update({f"sharded_{m}": ("sharded", m) for m in ("plain", "device_hyper", "clip")})
SCENARIOS.update({f"rebuild_{m}": ("rebuild", m) for m in ("plain", "clip")})
SCENARIOS["checkpoint_plain"] = ("checkpoint", "plain")
SCENARIOS.update({f"loose_{m}": ("loose", m) for m in ("plain", "device_hyper", "clip")})

HYPERS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0),
          dict(lr=4e-3, betas=(0.7, 0.9), eps=1e-5, weight_decay=0.05)]
LR_BEFORE_STEP_2 = 5e-4


def _optimizer(FusedAdamW, mode, loose=False):
    from bioscanclip.hip.engine import FlatParams
    kw = dict(MODES[mode])
    device_hyper = kw.pop("device_hyper", False)
    shapes = [[(5, 3), (7,)], [()]]
    groups = [[torch.nn.Parameter(torch.zeros(s)) for s in g] for g in shapes]
    flat_groups = list(groups)
    if loose:      # a trainable tensor with a gradient in no flat buffer, in a group of its own
        groups.append([torch.nn.Parameter(torch.zeros(3))])
        groups[2][0].grad = torch.zeros(3)
    opt = FusedAdamW([dict(params=g, **h) for g, h in zip(groups, HYPERS)], **kw)
    opt.enable_device_hyper(device_hyper)
    opt._flats = [FlatParams(g, CPU) for g in flat_groups]
    return opt


def _pattern(st):
    n = st["m"].numel()
    st["m"].copy_(torch.arange(1, n + 1, dtype=torch.float32))
    st["v"].copy_(torch.arange(1, n + 1, dtype=torch.float32) * 0.5)


def _snapshot(opt, moments):
    out = []
    for st in opt._flat_state.values():
        s = {"step": st["step"], "hyper": st["hyper"].tolist() if "hyper" in st else None, "lr_staged": st.get("lr_staged")}
        if opt._shard is not None:
            s["slice"] = list(st["slice"])
        if moments:
            s["moments"] = [" ".join(repr(x) for x in st[k].tolist()) for k in ("m", "v")]      # one line each in the golden file
        out.append(s)
    return out


def trace(name, FusedAdamW, setattr_):
    """One scenario's record.  ``setattr_(target, name, value)``: ``monkeypatch.setattr`` in a test."""
    from bioscanclip.hip import ops
    kind, mode = SCENARIOS[name]
    rec = Recorder()
    rec.install(setattr_)
    setattr_(torch.cuda, "is_current_stream_capturing", lambda: False)          # asked unguarded before the one capture query; no device here
    setattr_(ops, "grad_norm_partials", lambda n: max(1, -(-int(n) // 8192)))   # the stand-in library answers 0
    opt = _optimizer(FusedAdamW, mode, loose=kind == "loose")
    if kind == "sharded":      # rank 1 of 2: floats 12..24 of the first buffer, an empty slice of the second
        opt._shard = (1, 2, None)
        setattr_(opt, "sync_updated_slices", lambda: rec.calls.append(("sync_updated_slices", [])))
    moments = kind in ("rebuild", "checkpoint")
    steps, raises = [], None
    for k in (1, 2, 3):
        if k == 2:
            opt.param_groups[0]["lr"] = LR_BEFORE_STEP_2
        if k == 3 and moments:
            for st in opt._flat_state.values():
                _pattern(st)
                if "hyper" in st and opt.grad_clip_enabled():
                    st["hyper"][1:2].fill_(2)      # what the two recorded counter_add_if launches would have left
            if kind == "rebuild":      # every flat buffer replaced by a new one over the same parameters
                from bioscanclip.hip.engine import FlatParams
                opt._flats = [FlatParams(f.params, CPU) for f in opt._flats]
            else:                      # a new optimizer over new parameters of the same shapes, loaded from the old one's state_dict()
                sd = opt.state_dict()
                opt = _optimizer(FusedAdamW, mode)
                opt.load_state_dict(sd)
        try:
            opt.step()
        except RuntimeError as e:
            raises = str(e)
            break
        steps.append(_snapshot(opt, moments))
    return {"calls": rec.lines(), "steps": steps, "raises": raises}
