"""The weight average (EMA) of the fused AdamW step on the GPU.

Kernel bars.  (1) With lr = 0, a zero gradient, decay 1/2 and integer-valued operands every term of ``e + w (p - e)`` is dyadic and exact
in f32 with or without FMA contraction, so after k launches ``ema == p + (ema0 - p) / 2^k`` bit for bit, on every element.  (2) On random
operands ``p``, ``m``, ``v`` carry the bits of ``adamw_step_dev`` / ``adamw_step_clip`` (the same body), and the average lies within
``8 * 2^-24 * max(|ema_old|, |p_new|)`` of the f64 value formed from the kernel's own ``p_new`` and ``w = float32(1 - d_t)``: the
rounding of ``p - e`` (<= 2^-24 * 2 max), of the product (w < 1), of the sum (<= 2^-24 * 2 max) and of ``w`` itself (2^-24 * 2 max) add
up to 7 * 2^-24 * max, contraction only removes one of them.  (3) A skipped step changes no bit.  (4) The swap is exact.
Sizes: ``adamw_grid``'s edges, read from its source comment; every buffer has NaN guard words behind it.
The optimizer, the captured step and the engines are held to bit equality against runs without the feature / without the swap.
"""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7FC00000
HP = (0.9, 0.999, 1e-8, 0.01)     # betas, eps, weight decay: torch.optim.AdamW's defaults
GUARD = 4
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as _ops
    return _ops


def _grid_constants():
    """(elements per workgroup, workgroups beyond which the kernels stride) from the comment on ``adamw_grid`` in csrc/optim.hip,
    checked against the function's own body."""
    src = open(os.path.join(ROOT, "bioscan-clip_amd", "csrc", "optim.hip")).read()
    fn = src[src.index("static unsigned adamw_grid("):]
    fn = fn[:fn.index("\n}") + 2]
    m = re.search(r"(\d+) elements per workgroup, grid-stride beyond (\d+) workgroups", fn)
    per, cap = int(m.group(1)), int(m.group(2))
    assert f"(n + {per - 1}) / {per}" in fn and f"blocks > {cap} ? {cap}" in fn
    return per, cap


PER, CAP = _grid_constants()
SIZES = [1, 3, 4, 5, PER - 1, PER, PER + 1, CAP * PER - 1, CAP * PER, CAP * PER + 1, 2 * CAP * PER + 3]


def test_sizes_are_the_grid_edges():
    assert (PER, CAP) == (256, 2048) and SIZES[-1] == 1048579


class _Guarded:
    """An f32 device buffer of n elements with NaN guard words behind it."""

    def __init__(self, values):
        n = values.numel()
        self.full = torch.empty(n + GUARD, dtype=torch.float32, device="cuda")
        self.full[:n].copy_(values)
        self.full[n:] = float("nan")
        self.t = self.full[:n]

    def check(self, what):
        assert torch.isnan(self.full[self.t.numel():]).all(), f"wrote behind {what}"


def _check(*named):
    for name, b in named:
        b.check(name)


def _hyper(lr, step):
    """[lr as f32 bits, step as a uint32 word] (step may exceed 2^31)."""
    h = torch.zeros(2, dtype=torch.int32, device="cuda")
    h.view(torch.float32)[0:1].fill_(lr)
    h[1:2].fill_(step - (1 << 32) if step >= 1 << 31 else step)
    return h


def _new_state():
    buf = torch.zeros(16, dtype=torch.int32, device="cuda")
    buf[12:] = NAN_BITS
    return buf


def _record(ops, g, max_norm):
    """The clip record of gradient ``g`` under ``max_norm``, made by the norm pass itself."""
    state = _new_state()
    partials = torch.empty(ops.grad_norm_partials(g.numel()), dtype=torch.float64, device="cuda")
    ops.grad_sumsq_partial(g, partials)
    ops.grad_clip_finish(partials, max_norm, state)
    return state


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _d_t(decay, warmup, t):
    decay = float(np.float32(decay))          # the decay travels as an f32 launch argument
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def _w(decay, warmup, t):
    return np.float32(1.0 - _d_t(decay, warmup, t))


def _ema_bound_ok(ema_old, p_new, ema_new, w):
    """Every element within 8 * 2^-24 * max(|ema_old|, |p_new|) of the f64 lerp."""
    e, p, got = (x.detach().cpu().numpy().astype(np.float64) for x in (ema_old, p_new, ema_new))
    want = e + float(w) * (p - e)
    bound = 8 * EPS24 * np.maximum(np.abs(e), np.abs(p))
    err = np.abs(got - want)
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (worst, got[worst], want[worst], err[worst], bound[worst])
    return want


# ------------------------------------------------------------------------------------------------------------ 1. exact average
@pytest.mark.parametrize("n", SIZES)
def test_average_is_exact_on_dyadic_operands(ops, n):
    gen = torch.Generator().manual_seed(1000 + n % 997)
    p0 = torch.randint(-1024, 1025, (n,), generator=gen).to(torch.float32)
    e0 = torch.randint(-1024, 1025, (n,), generator=gen).to(torch.float32)
    p, g, m, v, ema = _Guarded(p0), _Guarded(torch.zeros(n)), _Guarded(torch.zeros(n)), _Guarded(torch.zeros(n)), _Guarded(e0)
    hyper = _hyper(0.0, 1)
    p_bits = _bits(p.t)
    for k in range(1, 9):
        ops.adamw_step_ema(p.t, g.t, m.t, v.t, ema.t, hyper, None, 0.9, 0.999, 1e-8, 0.0, 0.5, False)
        want = (p0.double() + (e0.double() - p0.double()) / 2 ** k).to(torch.float32)
        assert torch.equal(want.double(), p0.double() + (e0.double() - p0.double()) / 2 ** k)       # the bar itself is an f32
        got = ema.t.cpu()
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        assert bad.numel() == 0, (n, k, bad[:4].flatten().tolist(), got[bad[0]], want[bad[0]])
        assert torch.equal(_bits(p.t), p_bits), (n, k)
        assert not m.t.any() and not v.t.any()
        _check(("p", p), ("g", g), ("m", m), ("v", v), ("ema", ema))


# ------------------------------------------------------------------------------------------------------------ 2. same update, bounded average
def _rand(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen) * 1e-2, m=torch.randn(n, generator=gen) * 1e-2,
                v=torch.rand(n, generator=gen) * 1e-3, ema=torch.randn(n, generator=gen))


def _crossing(decay):
    """The step count at which (1 + t) / (10 + t) reaches ``decay``: t = (10 decay - 1) / (1 - decay)."""
    return round((10 * decay - 1) / (1 - decay))


T_CROSS = _crossing(0.999)


def test_warmup_crossing_is_where_the_issue_puts_it():
    assert T_CROSS == 8990
    assert _d_t(0.999, True, T_CROSS - 1) < float(np.float32(0.999)) <= _d_t(0.999, True, T_CROSS + 1)
    assert _d_t(0.999, True, 1) == 2 / 11 and _d_t(0.999, True, (1 << 31) + 5) == float(np.float32(0.999))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_update_bits_and_bounded_average(ops, n, clip):
    r = _rand(n, 2000 + n % 991)
    bufs = {k: _Guarded(x) for k, x in r.items()}
    ref = {k: _Guarded(r[k]) for k in ("p", "m", "v")}
    hyper = _hyper(1e-3, 7)
    state = _record(ops, bufs["g"].t, 1e-6) if clip else None       # coef = 1e-6 / (|g| + 1e-6) < 1 for any gradient but zero
    if clip:
        assert int(state[0].item()) == 1 and 0 < float(state.view(torch.float32)[1].item()) < 1
        ops.adamw_step_clip(ref["p"].t, bufs["g"].t, ref["m"].t, ref["v"].t, hyper, state, *HP)
    else:
        ops.adamw_step_dev(ref["p"].t, bufs["g"].t, ref["m"].t, ref["v"].t, hyper, *HP)
    ops.adamw_step_ema(bufs["p"].t, bufs["g"].t, bufs["m"].t, bufs["v"].t, bufs["ema"].t, hyper, state, *HP, 0.999, True)
    for k in ("p", "m", "v"):
        assert torch.equal(_bits(bufs[k].t), _bits(ref[k].t)), (n, k)
    assert not torch.equal(_bits(bufs["p"].t), _bits(r["p"].cuda()))
    _ema_bound_ok(r["ema"], bufs["p"].t, bufs["ema"].t, _w(0.999, True, 7))
    _check(*bufs.items(), *ref.items())
    if clip:
        assert (state[12:] == NAN_BITS).all()


@pytest.mark.parametrize("t", [1, T_CROSS - 1, T_CROSS, T_CROSS + 1, (1 << 31) + 5])
def test_warmup_follows_the_unsigned_step_word(ops, t):
    n = PER + 1
    r = _rand(n, 3000 + t % 983)
    bufs = {k: _Guarded(x) for k, x in r.items()}
    ref = {k: _Guarded(r[k]) for k in ("p", "m", "v")}
    hyper = _hyper(1e-3, t)
    ops.adamw_step_dev(ref["p"].t, bufs["g"].t, ref["m"].t, ref["v"].t, hyper, *HP)
    ops.adamw_step_ema(bufs["p"].t, bufs["g"].t, bufs["m"].t, bufs["v"].t, bufs["ema"].t, hyper, None, *HP, 0.999, True)
    for k in ("p", "m", "v"):
        assert torch.equal(_bits(bufs[k].t), _bits(ref[k].t)), (t, k)
    w = _w(0.999, True, t)
    if t == 1:
        assert w == np.float32(1.0 - 2 / 11)
    if t > T_CROSS:
        assert w == np.float32(1.0 - float(np.float32(0.999)))
    want = _ema_bound_ok(r["ema"], bufs["p"].t, bufs["ema"].t, w)
    if t == 1:      # a word read as signed, or a warm-up that is ignored, is far outside the bound: w would be 0.001 instead of 0.818
        wrong = r["ema"].double().numpy() + float(_w(0.999, False, t)) * (bufs["p"].t.cpu().double().numpy() - r["ema"].double().numpy())
        assert np.abs(wrong - want).max() > 0.1
    _check(*bufs.items(), *ref.items())


def test_warmup_off_uses_the_decay_itself(ops):
    n = 1025
    r = _rand(n, 3500)
    bufs = {k: _Guarded(x) for k, x in r.items()}
    hyper = _hyper(1e-3, 1)
    ops.adamw_step_ema(bufs["p"].t, bufs["g"].t, bufs["m"].t, bufs["v"].t, bufs["ema"].t, hyper, None, *HP, 0.9, False)
    _ema_bound_ok(r["ema"], bufs["p"].t, bufs["ema"].t, _w(0.9, False, 1))
    _check(*bufs.items())


# ------------------------------------------------------------------------------------------------------------ 3. skipped step
@pytest.mark.parametrize("n", [5, PER + 1, CAP * PER + 1])
def test_skipped_step_keeps_every_bit(ops, n):
    r = _rand(n, 4000 + n % 977)
    r["g"][n // 2] = float("nan")                     # a non-finite value in the input data: the record says skip
    bufs = {k: _Guarded(x) for k, x in r.items()}
    hyper = _hyper(1e-3, 3)
    state = _record(ops, bufs["g"].t, 1.0)
    assert int(state[0].item()) == 0
    before = {k: _bits(b.full) for k, b in bufs.items()}
    ops.counter_add_if(hyper[1:2], 1, state[0:1])     # what the optimizer issues ahead of the update
    ops.adamw_step_ema(bufs["p"].t, bufs["g"].t, bufs["m"].t, bufs["v"].t, bufs["ema"].t, hyper, state, *HP, 0.999, True)
    for k, b in bufs.items():
        assert torch.equal(_bits(b.full), before[k]), (n, k)
    assert int(hyper[1].item()) == 3
    assert float(hyper.view(torch.float32)[0].item()) == float(np.float32(1e-3))


# ------------------------------------------------------------------------------------------------------------ 4. swap
@pytest.mark.parametrize("n", SIZES)
def test_swap_is_exact_and_an_involution(ops, n):
    gen = torch.Generator().manual_seed(5000 + n % 971)
    a0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)      # every bit pattern, NaNs included
    b0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    a, b = _Guarded(a0.view(torch.float32)), _Guarded(b0.view(torch.float32))
    a.full[:n].view(torch.int32).copy_(a0)            # bit copies: a float copy may quiet a signalling NaN
    b.full[:n].view(torch.int32).copy_(b0)
    ops.swap_f32(a.t, b.t)
    assert torch.equal(_bits(a.t).cpu(), b0) and torch.equal(_bits(b.t).cpu(), a0)
    _check(("a", a), ("b", b))
    ops.swap_f32(a.t, b.t)
    assert torch.equal(_bits(a.t).cpu(), a0) and torch.equal(_bits(b.t).cpu(), b0)
    _check(("a", a), ("b", b))


# ------------------------------------------------------------------------------------------------------------ 5. the optimizer
SHAPES = [[(37, 5), (11,)], [(64, 9), (3, 3), (130,)]]     # two flat buffers, odd sizes: padded slices


def _make_optimizer(values, **kw):
    """A ``FusedAdamW`` over two GPU ``FlatParams`` buffers holding ``values`` (one list of tensors per buffer)."""
    from bioscanclip.hip.engine import FlatParams
    from bioscanclip.hip.optim import FusedAdamW
    groups = [[torch.nn.Parameter(v.clone().cuda()) for v in group] for group in values]
    flats = [FlatParams(g, torch.device("cuda")) for g in groups]
    params = [p for g in groups for p in g]
    opt = FusedAdamW(params, lr=2e-3, **kw)
    opt._flats = flats
    return opt, params, flats


@pytest.fixture(scope="module")
def seeded():
    """Initial values and six steps of gradients, shared and never written."""
    gen = torch.Generator().manual_seed(600)
    values = [[torch.randn(s, generator=gen) for s in group] for group in SHAPES]
    grads = [[torch.randn(s, generator=gen) * 0.02 for group in SHAPES for s in group] for _ in range(6)]
    return values, grads


def _run(opt, params, grads, steps, lr_change_at=3):
    for k in steps:
        if k == lr_change_at:
            opt.param_groups[0]["lr"] = 7e-4
        opt.zero_grad()
        for p, g in zip(params, grads[k]):
            p.grad.copy_(g.cuda())
        opt.step()
        yield k


def _state_bits(opt, flats, keys=("m", "v", "ema")):
    sts = list(opt._flat_state.values())
    return [_bits(f.data) for f in flats] + [_bits(st[k]) for st in sts for k in keys if k in st]


def test_average_does_not_perturb_training_and_follows_the_recurrence(ops, seeded):
    values, grads = seeded
    on, p_on, f_on = _make_optimizer(values, ema_decay=0.99)
    off, p_off, f_off = _make_optimizer(values)
    off.enable_device_hyper(True)
    init = [f.data.clone() for f in f_on]
    ref = [f.data.cpu().numpy().astype(np.float64) for f in f_on]       # the f64 recurrence, on the kernel's own parameters
    slack = [np.zeros_like(r) for r in ref]
    for (k, _) in zip(_run(on, p_on, grads, range(6)), _run(off, p_off, grads, range(6))):
        t = k + 1
        assert torch.equal(torch.cat(_state_bits(on, f_on, ("m", "v"))), torch.cat(_state_bits(off, f_off, ("m", "v")))), k
        assert on.ema_effective_decay() == _d_t(0.99, True, t) == (1 + t) / (10 + t)
        w = float(_w(0.99, True, t))
        for i, (f, st) in enumerate(zip(f_on, on._flat_state.values())):
            p_new = f.data.cpu().numpy().astype(np.float64)
            slack[i] += 8 * EPS24 * np.maximum(np.abs(ref[i]), np.abs(p_new))
            ref[i] = ref[i] + w * (p_new - ref[i])
            got = st["ema"].cpu().numpy().astype(np.float64)
            assert (np.abs(got - ref[i]) <= slack[i]).all(), (k, i)
            if k == 0:      # the average started as the parameters before the first update
                first = init[i].cpu().numpy().astype(np.float64)
                assert (np.abs(got - (first + w * (p_new - first))) <= 8 * EPS24 * np.maximum(np.abs(first), np.abs(p_new))).all()
    for p in p_on:          # published per parameter, as views of the flat average
        assert on.state[p]["ema"].shape == p.shape and on.state[p]["ema"].data_ptr() != p.data_ptr()
    assert not torch.equal(on._flat_state[id(f_on[0])]["ema"], f_on[0].data)


def test_skipped_step_is_skipped_by_the_average_and_the_warmup(ops, seeded):
    values, grads = seeded
    runs = {}
    for name, steps in (("with_nan", range(6)), ("without", [0, 1, 2, 4, 5])):
        opt, params, flats = _make_optimizer(values, ema_decay=0.99, max_grad_norm=0.5, skip_nonfinite=True)
        g = [[x.clone() for x in step] for step in grads]
        g[3][4].view(-1)[17] = float("nan")                 # step 3's gradient is not finite (when that step is taken at all)
        for k in _run(opt, params, g, steps, lr_change_at=None):
            if name == "with_nan" and k == 2:
                before = _state_bits(opt, flats) + [_bits(st["hyper"]) for st in opt._flat_state.values()]
            if name == "with_nan" and k == 3:
                after = _state_bits(opt, flats) + [_bits(st["hyper"]) for st in opt._flat_state.values()]
                assert all(torch.equal(a, b) for a, b in zip(before, after))
                assert opt.ema_effective_decay() == (1 + 3) / (10 + 3)
        assert [int(st["hyper"][1].item()) for st in opt._flat_state.values()] == [5, 5]
        assert opt.ema_effective_decay() == (1 + 5) / (10 + 5)
        runs[name] = _state_bits(opt, flats)
        assert opt.grad_stats()["skipped"] == (1 if name == "with_nan" else 0)
    assert all(torch.equal(a, b) for a, b in zip(runs["with_nan"], runs["without"]))      # as if the skipped step had not happened


def test_ema_weights_swaps_in_place_and_restores(ops, seeded):
    values, grads = seeded
    opt, params, flats = _make_optimizer(values, ema_decay=0.9, ema_warmup=False)
    with opt.ema_weights():                                  # before the first step: nothing to swap
        assert all(torch.equal(p.detach().cpu(), v) for p, v in zip(params, [v for g in values for v in g]))
    list(_run(opt, params, grads, range(3)))
    raw = [_bits(f.data) for f in flats]
    avg = [_bits(st["ema"]) for st in opt._flat_state.values()]
    ptrs = [f.data.data_ptr() for f in flats]
    assert all(not torch.equal(a, b) for a, b in zip(raw, avg))
    with opt.ema_weights():
        assert all(torch.equal(_bits(f.data), a) for f, a in zip(flats, avg))
        assert all(torch.equal(_bits(st["ema"]), r) for st, r in zip(opt._flat_state.values(), raw))
        for f in flats:                                      # the parameters are views of the flat buffer: they ARE the average
            for p, o in zip(f.params, f.offsets):
                assert torch.equal(p.detach().reshape(-1), f.data[o:o + p.numel()])
        with pytest.raises(RuntimeError, match="no step inside"):
            opt.step()
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    assert all(torch.equal(_bits(f.data), r) for f, r in zip(flats, raw))
    assert all(torch.equal(_bits(st["ema"]), a) for st, a in zip(opt._flat_state.values(), avg))
    assert [f.data.data_ptr() for f in flats] == ptrs and all(f.valid() for f in flats)


def test_state_dict_round_trip_continues_the_average(ops, seeded):
    values, grads = seeded
    full, p_full, f_full = _make_optimizer(values, ema_decay=0.99)
    list(_run(full, p_full, grads, range(4)))
    first, p_first, f_first = _make_optimizer(values, ema_decay=0.99)
    list(_run(first, p_first, grads, range(3)))
    sd = first.state_dict()
    assert all("ema" in s and int(s["step"]) == 3 for s in sd["state"].values())
    now = [[p.detach().cpu() for p in f.params] for f in f_first]
    resumed, p_res, f_res = _make_optimizer(now, ema_decay=0.99)
    resumed.param_groups[0]["lr"] = first.param_groups[0]["lr"]
    resumed.load_state_dict(sd)
    list(_run(resumed, p_res, grads, [3]))
    assert all(torch.equal(a, b) for a, b in zip(_state_bits(resumed, f_res), _state_bits(full, f_full)))
    assert resumed.ema_effective_decay() == full.ema_effective_decay() == 5 / 14


# ------------------------------------------------------------------------------------------------------------ 6. the captured step
@pytest.mark.parametrize("clip", [False, True])
def test_captured_step_equals_eager_with_the_average_on(ops, clip):
    from test_30_graph_gpu import _build
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    steps = 7                                 # graph run: 0-1 eager warm-up, 2 capture + first replay, 3-6 replays
    batches = [synth.synth_batch(8, seed=400 + s % 3) for s in range(steps)]
    runs = {}
    for mode in ("eager", "graph"):
        model = _build(92, False)
        kw = dict(max_grad_norm=0.5, skip_nonfinite=True) if clip else {}
        opt = FusedAdamW(model.parameters(), lr=1e-3, ema_decay=0.9, **kw)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=3e-3, total_steps=steps, pct_start=0.3, anneal_strategy="cos",
                                                    cycle_momentum=False)
        crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
        g = GraphedStep(model, opt, crit, warmup=2) if mode == "graph" else None
        for s in range(steps):
            image, dna, _, label = batches[s]
            image, dna, label = image.cuda(), dna.cuda(), label.cuda()
            if g is not None:
                g(image, dna, None, label)
                if s == 4:                    # between two replays: in and out of the averaged weights, nothing rebuilt
                    with opt.ema_weights():
                        torch.cuda.synchronize()
            else:
                opt.zero_grad()
                loss = crit(*model(image, dna, None), label)
                loss.backward()
                if opt.needs_attach():
                    opt.attach(model)
                opt.step()
            sched.step()
        if g is not None:
            assert g.graph is not None
        torch.cuda.synchronize()
        sts = list(opt._flat_state.values())
        assert sts and all("ema" in st for st in sts)
        assert [int(st["hyper"][1].item()) for st in sts] == [steps] * len(sts)
        assert opt.ema_effective_decay() == (1 + steps) / (10 + steps)
        runs[mode] = ({k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad},
                      [st[k].clone() for st in sts for k in ("m", "v", "ema")])
    for k, v in runs["eager"][0].items():
        assert torch.equal(v, runs["graph"][0][k]), k
    assert len(runs["eager"][1]) == len(runs["graph"][1])
    for i, (a, b) in enumerate(zip(runs["eager"][1], runs["graph"][1])):
        assert torch.equal(a, b), i


# ------------------------------------------------------------------------------------------------------------ 7. engines see the swap
@pytest.mark.parametrize("full_ft", [False, True])
def test_engines_read_the_swapped_weights(ops, full_ft):
    from test_30_graph_gpu import _build
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    model = _build(93, False, full_ft=full_ft)
    opt = FusedAdamW(model.parameters(), lr=1e-3, ema_decay=0.5, ema_warmup=False)
    crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07)
    for s in range(3):
        image, dna, _, label = synth.synth_batch(8, seed=500 + s)
        opt.zero_grad()
        crit(*model(image.cuda(), dna.cuda(), None), label.cuda()).backward()
        if opt.needs_attach():
            opt.attach(model)
        opt.step()
    image, dna, _, _ = synth.synth_batch(8, seed=510)
    image, dna = image.cuda(), dna.cuda()

    def features(m):
        m.eval()
        with torch.no_grad():
            return [x.detach().clone() for x in m(image, dna, None) if x is not None]

    raw = features(model)
    with opt.ema_weights():
        averaged = features(model)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    again = features(model)
    other = _build(94, False, full_ft=full_ft)
    other.load_state_dict(sd)
    loaded = features(other)
    assert len(raw) == len(averaged) == len(loaded) == 2
    for r, a, l, b in zip(raw, averaged, loaded, again):
        assert torch.isfinite(a).all()
        assert torch.equal(a, l)              # the engines computed on the average: a model that loaded it gives the same bits
        assert not torch.equal(a, r)
        assert torch.equal(b, r)              # and on the raw weights again after the block


# ------------------------------------------------------------------------------------------------------------ 8. the training script
def test_train_cl_with_ema_decay(ops, tmp_path, capsys):
    """Five captured-or-eager steps with the key on: the epoch line reports (1 + 5) / (10 + 5), and the evaluation runs (inside
    ``ema_weights()``) and reports its accuracy."""
    sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
    import train_cl
    capsys.readouterr()
    losses = train_cl.main(["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.batch_size=8", "model_config.epochs=1",
                            "synthetic_steps_per_epoch=5", "synthetic_eval=true", "synthetic_eval_batches=1",
                            "model_config.ema_decay=0.999", "debug_flag=true", f"project_root_path={tmp_path}"])
    out = capsys.readouterr().out
    assert len(losses) == 1 and math.isfinite(float(losses[0]))
    line = [ln for ln in out.splitlines() if ln.startswith("Epoch [0/1]")]
    assert len(line) == 1 and line[0].endswith(", ema decay: 0.400000"), out
    assert "epoch 0: overall_acc " in out
