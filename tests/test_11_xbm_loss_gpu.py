"""The cross-batch memory on the GPU: the ring writer (``bsclip_xbm_enqueue``), the InfoNCE over the own batch and the valid bank
slots (``bsclip_infonce_xbm_fwd_bwd``) against plain torch in float64 on the CPU, its reduction to ``bsclip_infonce_fwd_bwd_ts`` on
an empty bank, the invisibility of slots that are not valid, repeatability, the roles of every modality's gradient, a captured
graph that advances the ring, and ``train_cl.py`` with ``model_config.memory_bank_size``.

Inputs are in the trained regime of the temperature tests: z^m_i = prototype[label_i] + 0.5 noise (cosines of one class ~0.8).
Own labels come from about N / 3 classes; the bank's labels come from a window of classes shifted by half its width, so some own
rows have positives in the bank and some have none.  The bank is always filled through ``bsclip_xbm_enqueue`` -- what lies behind
its documented f32 rows belongs to the implementation -- and the oracle reads those documented rows back.

Gates (restated from tests/test_11_infonce_temperature_gpu.py, the same arithmetic: split-bf16 products, f32 softmax, f64 sums):
loss relative 2e-5; dz normwise relative 2e-4; dLoss/dt within (1 + 2 s) 2^-16 A, A = s/(P N) sum (cnt_i p_ij + T_ij) |G_ij| over all
keys; the scale within 2e-7 relative.  Measured |hip - f64| / gate of every case goes to test_20's parity log (``t20._log``), from
which ``tools/xbm_loss_bench.py --parity-log`` folds the worst ratios into profiles/xbm_loss_bench.json."""
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import load_golden, rel_err  # noqa: E402
import test_20_encoders_gpu as t20  # noqa: E402  (its parity log)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T07 = math.log(1 / 0.07)
LN100 = math.log(100.0)
F32 = torch.float32
D = 768
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture()
def ops():
    from bioscanclip.hip import ops as o
    return o


_log = t20._log


# ------------------------------------------------------------------------------------------------------------ inputs
def _classes(N):
    return max(2, N // 3)


_PROTO = {}


def _draw(n, lo, hi, nmod, seed):
    """n rows per modality around the prototypes of labels drawn from [lo, hi): (zs, labels) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if "proto" not in _PROTO:
        _PROTO["proto"] = torch.randn(1024, D, generator=torch.Generator().manual_seed(77))
    proto = _PROTO["proto"]
    labels = torch.randint(lo, hi, (n,), generator=g)
    zs = [proto[labels] + 0.5 * torch.randn(n, D, generator=g) for _ in range(nmod)]
    return zs, labels


_BATCH = {}


def _batch(N, nmod):
    if (N, nmod) not in _BATCH:
        zs, labels = _draw(N, 0, _classes(N), nmod, 2000 + N + nmod)
        _BATCH[(N, nmod)] = (zs, labels, [z.cuda() for z in zs], labels.cuda())
    return _BATCH[(N, nmod)]


class Bank:
    """A bank of Q slots with a NaN (labels: -7, state: -7) guard row around every buffer; ``fill`` is what the slots hold before
    anything is enqueued, behind the documented rows too."""

    def __init__(self, ops, Q, nmod, fill=NAN):
        self.Q, self.nmod = Q, nmod
        self.n = ops.xbm_bank_floats(Q)
        self.raw = [torch.full((self.n + 2 * D,), NAN, dtype=F32, device="cuda") for _ in range(nmod)]
        self.banks = [r[D:D + self.n] for r in self.raw]
        for b in self.banks:
            b.fill_(fill)
        self.raw_labels = torch.full((Q + 16,), -7, dtype=torch.int64, device="cuda")
        self.labels = self.raw_labels[8:8 + Q]
        self.raw_state = torch.full((2 + 8,), -7, dtype=torch.int32, device="cuda")
        self.state = self.raw_state[4:6]
        self.state.zero_()
        self._ws = {}

    def ws(self, ops, N):
        if N not in self._ws:
            self._ws[N] = torch.empty(ops.xbm_workspace_floats(N, self.Q, self.nmod), dtype=F32, device="cuda")
        return self._ws[N]

    def rows(self, m):
        return self.banks[m][:self.Q * D].view(self.Q, D)

    def guards_ok(self):
        ok = all(torch.isnan(r[:D]).all() and torch.isnan(r[D + self.n:]).all() for r in self.raw)
        ok = ok and (self.raw_labels[:8] == -7).all() and (self.raw_labels[8 + self.Q:] == -7).all()
        return bool(ok and (self.raw_state[:4] == -7).all() and (self.raw_state[6:] == -7).all())

    def enqueue(self, ops, zs, labels):
        ops.xbm_enqueue(zs, labels, self.banks, self.labels, self.state, self.ws(ops, zs[0].shape[0]))

    def snapshot(self):
        return [b.clone() for b in self.banks], self.labels.clone(), self.state.clone()


def _bank_with(ops, Q, nmod, filled, N, fill=NAN):
    """A bank holding ``filled`` rows (one enqueue), labels from the window [C/2, 3C/2) of the N-row batch's C classes."""
    bank = Bank(ops, Q, nmod, fill)
    if filled:
        C = _classes(N)
        zs, labels = _draw(filled, C // 2, C // 2 + C, nmod, 3000 + Q + filled + nmod)
        bank.enqueue(ops, [z.cuda() for z in zs], labels.cuda())
    return bank


def _run(ops, bank, N, t, want_dz=True, zs=None, labels=None):
    """One call on NaN-filled outputs with spare elements behind them; (loss, dzs, scale_out) after the pad guard."""
    if zs is None:
        _, _, zs, labels = _batch(N, bank.nmod)
    loss = torch.full((1 + 15,), NAN, device="cuda")
    so = torch.full((2 + 14,), NAN, device="cuda")
    bufs = [torch.full((N * D + D,), NAN, device="cuda") for _ in range(bank.nmod)] if want_dz else None
    dzs = [b[:N * D].view(N, D) for b in bufs] if want_dz else None
    tt = torch.tensor([t], dtype=F32, device="cuda")
    ops.infonce_xbm(zs, labels, tt, bank.banks, bank.labels, bank.state, loss[:1], dzs, so[:2], bank.ws(ops, N))
    torch.cuda.synchronize()
    assert torch.isnan(loss[1:]).all() and torch.isnan(so[2:]).all() and not torch.isnan(so[:2]).any()
    if want_dz:
        for b in bufs:
            assert torch.isnan(b[N * D:]).all() and not torch.isnan(b[:N * D]).any(), "dz: written past its end, or not fully written"
    return loss[:1], dzs, so[:2]


# ------------------------------------------------------------------------------------------------------------ the f64 oracle
def _oracle(zs, labels, keys, key_labels, t, dtype=torch.float64):
    """Plain torch on the CPU: zs own rows (any scale), keys[m] the valid bank rows of modality m (already normalised, detached),
    key_labels theirs.  Returns loss, dz per modality, dLoss/dt and the bar's A."""
    nmod, N = len(zs), zs[0].shape[0]
    zd = [z.detach().cpu().to(dtype).requires_grad_(True) for z in zs]
    td = torch.tensor(t, dtype=dtype, requires_grad=True)
    s = torch.exp(torch.clamp(td, 0.0, LN100))
    zn = [F.normalize(z, dim=1, eps=1e-12) for z in zd]
    lab = labels.cpu()
    all_lab = torch.cat([lab, key_labels.cpu()])
    T = (lab[:, None] == all_lab[None, :]).to(dtype)
    cnt = T.sum(1)
    total, A = 0.0, 0.0
    for a in range(nmod):
        for b in range(nmod):
            if a == b:
                continue
            C = torch.cat([zn[b], keys[b].detach().cpu().to(dtype)])
            G = zn[a] @ C.t()
            x = s * G
            total = total + (cnt * torch.logsumexp(x, dim=1) - (T * x).sum(1)).sum() / N
            with torch.no_grad():
                A += ((cnt[:, None] * torch.softmax(x, dim=1) + T) * G.abs()).sum().item()
    P = nmod * (nmod - 1)
    loss = total / P
    loss.backward()
    A *= s.item() / (P * N)
    return loss.item(), [z.grad for z in zd], td.grad.item(), A


def _oracle_for(bank, N, t, dtype=torch.float64):
    zs, labels, _, _ = _batch(N, bank.nmod)
    filled = int(bank.state[1])
    keys = [bank.rows(m)[:filled] for m in range(bank.nmod)]
    return _oracle(zs, labels, keys, bank.labels[:filled], t, dtype)


def _check(tag, loss, dzs, so, ref, t, extra=None):
    ref_loss, ref_dz, ref_dt, A = ref
    s = math.exp(min(max(t, 0.0), LN100))
    bar = (1 + 2 * s) * 2.0 ** -16 * A
    loss_err = abs(loss.item() - ref_loss) / abs(ref_loss)
    dz_each = [rel_err(d, r) for d, r in zip(dzs, ref_dz)]
    dt_err = abs(so[0].item() - ref_dt)
    rec = dict(test=tag, t=t, loss_over_gate=loss_err / 2e-5, dz_over_gate=max(dz_each) / 2e-4, dt_over_gate=dt_err / bar,
               loss_rel=loss_err, dz_rel=max(dz_each), dt_hip=so[0].item(), dt_f64=ref_dt, bar=bar, **(extra or {}))
    print(json.dumps(rec))
    _log(rec)
    assert abs(so[1].item() - s) <= 2e-7 * s
    assert loss_err < 2e-5, (loss.item(), ref_loss)
    assert max(dz_each) < 2e-4, dz_each
    assert dt_err <= bar, (so[0].item(), ref_dt, dt_err, bar)
    return dz_each


# ------------------------------------------------------------------------------------------------------------ 1. the ring
def test_ring_wraps_and_writes_what_is_documented(ops):
    """Q = 512, N = 192, four enqueues: the third wraps (576 > 512).  The enqueue normalises with the l2norm kernel's arithmetic
    (the same sums in the same order), so a slot is held to 1 ulp of ``bsclip_l2norm_fwd``'s row, and to 6 x 2^-23 relative of
    F.normalize in f64: a lane's 12 squares and the 6 shuffle adds leave at most 18 roundings of 2^-24 on the sum, halved by the
    square root (9), the root, the reciprocal and the product add one each: 12 x 2^-24."""
    Q, N, nmod = 512, 192, 3
    bank = Bank(ops, Q, nmod)
    want_rows = [torch.full((Q, D), NAN, dtype=torch.float64) for _ in range(nmod)]
    want_l2 = [torch.full((Q, D), NAN) for _ in range(nmod)]
    want_labels = torch.full((Q,), -1, dtype=torch.int64)
    touched = torch.zeros(Q, dtype=torch.bool)
    head = filled = 0
    for step in range(4):
        zs, labels = _draw(N, 0, 50, nmod, 500 + step)
        zs = [z * (0.1 + step) for z in zs]                                 # the scale must not matter
        zd = [z.cuda() for z in zs]
        bank.enqueue(ops, zd, labels.cuda())
        slots = (head + torch.arange(N)) % Q
        for m in range(nmod):
            want_rows[m][slots] = F.normalize(zs[m].double(), dim=1, eps=1e-12)
            y, inv = torch.empty(N, D, device="cuda"), torch.empty(N, device="cuda")
            ops.l2norm_fwd(zd[m], y, inv)
            want_l2[m][slots] = y.cpu()
        want_labels[slots] = labels
        touched[slots] = True
        head, filled = (head + N) % Q, min(filled + N, Q)
        torch.cuda.synchronize()
        assert bank.state.tolist() == [head, filled], step
        assert bank.guards_ok(), step
        assert torch.equal(bank.labels.cpu()[touched], want_labels[touched])
        assert (bank.labels.cpu()[~touched] == -7).all()
        for m in range(nmod):
            got = bank.rows(m).cpu()
            assert torch.isnan(got[~touched]).all(), (step, m)              # untouched slots keep their fill
            ulp = torch.finfo(F32).eps * want_l2[m][touched].abs()
            assert ((got[touched] - want_l2[m][touched]).abs() <= ulp).all(), (step, m)
            d64 = (got[touched].double() - want_rows[m][touched]).abs()
            assert (d64 <= 6 * 2.0 ** -23 * want_rows[m][touched].abs() + 1e-30).all(), (step, m, d64.max().item())
    assert step == 3 and touched.all() and filled == Q and head == (4 * N) % Q


# ------------------------------------------------------------------------------------------------------------ 2. the guard
@pytest.mark.parametrize("bad", [float("inf"), NAN])
def test_a_non_finite_row_leaves_everything_untouched(ops, bad):
    Q, N, nmod = 512, 192, 3
    bank = Bank(ops, Q, nmod)
    zs, labels = _draw(N, 0, 50, nmod, 600)
    bank.enqueue(ops, [z.cuda() for z in zs], labels.cuda())
    before = bank.snapshot()
    zs2, labels2 = _draw(N, 0, 50, nmod, 601)
    zs2[1][N - 3, 700] = bad                                                 # one value of one row of one modality
    bank.enqueue(ops, [z.cuda() for z in zs2], labels2.cuda())
    torch.cuda.synchronize()
    after = bank.snapshot()
    for x, y in zip(before[0], after[0]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))        # bit for bit, the NaN fill included
    assert torch.equal(before[1], after[1]) and torch.equal(before[2], after[2]) and bank.state.tolist() == [N, N]
    assert bank.guards_ok()
    zs2[1][N - 3, 700] = 0.0                                                # the same batch, finite: the ring moves again
    bank.enqueue(ops, [z.cuda() for z in zs2], labels2.cuda())
    assert bank.state.tolist() == [2 * N, 2 * N]


# ------------------------------------------------------------------------------------------------------------ 3. loss and gradients vs f64
_T_OF = {(5, 256, 192, 2): -0.5, (200, 1024, 1024, 3): 5.0, (64, 256, 0, 3): 5.0, (256, 1024, 192, 2): -0.5}   # the rest: t inside


@pytest.mark.parametrize("nmod", [2, 3])
@pytest.mark.parametrize("fill", ["0", "192", "Q"])
@pytest.mark.parametrize("Q", [256, 1024])
@pytest.mark.parametrize("N", [5, 64, 200, 256])
def test_loss_and_gradients_vs_f64(ops, N, Q, fill, nmod):
    filled = {"0": 0, "192": 192, "Q": Q}[fill]
    t = _T_OF.get((N, Q, filled, nmod), T07)
    bank = _bank_with(ops, Q, nmod, filled, N)
    assert bank.state.tolist() == [filled % Q, filled]
    ref = _oracle_for(bank, N, t)
    loss, dzs, so = _run(ops, bank, N, t)
    if not 0.0 <= t <= LN100:
        assert so[0].item() == 0.0 and ref[2] == 0.0
    _, labels, _, _ = _batch(N, nmod)
    in_bank = (labels[:, None] == bank.labels[:filled].cpu()[None, :]).any(1)
    if filled and N >= 64:
        assert in_bank.any() and not in_bank.all()                          # positives in the bank for some rows, none for others
    _check("xbm_vs_f64", loss, dzs, so, ref, t, dict(N=N, Q=Q, filled=filled, nmod=nmod))
    assert bank.guards_ok()


def test_one_launch_per_product_where_the_tile_is_not_128(ops):
    """The own logits, the bank logits and the dz-own products go as one batched launch over the pairs where the shape takes the
    128 x 128 tile, and product by product otherwise (as the bank logits of N = 1024 against Q = 16 384 do by size).  Forcing the
    256 x 256 ping-pong tile takes the second path at a small shape; the values are held to the same gates."""
    N, Q, nmod = 64, 256, 3
    bank = _bank_with(ops, Q, nmod, 192, N)
    ref = _oracle_for(bank, N, T07)
    ops.set_gemm_tile(4)
    try:
        loss, dzs, so = _run(ops, bank, N, T07)
    finally:
        ops.set_gemm_tile(0)
    _check("xbm_per_product", loss, dzs, so, ref, T07, dict(N=N, Q=Q, filled=192, nmod=nmod))


# ------------------------------------------------------------------------------------------------------------ 4. empty bank
@pytest.mark.parametrize("N,nmod", [(200, 3), (256, 2), (5, 2)])
def test_an_empty_bank_is_the_existing_loss(ops, N, nmod):
    bank = Bank(ops, 512, nmod)
    _, _, zd, ld = _batch(N, nmod)
    loss, dzs, so = _run(ops, bank, N, T07)
    ref_loss = torch.zeros(1, device="cuda")
    ref_dz = [torch.empty(N, D, device="cuda") for _ in range(nmod)]
    ref_so = torch.empty(2, device="cuda")
    ws = torch.empty(ops.infonce_workspace_floats(N, nmod), dtype=F32, device="cuda")
    ops.infonce_fwd_bwd_ts(zd, ld, torch.tensor([T07], device="cuda"), ref_loss, ref_dz, ref_so, workspace=ws)
    A = _oracle_for(bank, N, T07)[3]
    bar = (1 + 2 * math.exp(T07)) * 2.0 ** -16 * A
    assert so[1].item() == ref_so[1].item()
    assert abs(loss.item() - ref_loss.item()) < 2e-5 * abs(ref_loss.item())
    assert max(rel_err(d, r) for d, r in zip(dzs, ref_dz)) < 2e-4
    assert abs(so[0].item() - ref_so[0].item()) <= bar


# ------------------------------------------------------------------------------------------------------------ 5. invalid slots
def test_slots_that_are_not_valid_are_invisible(ops):
    """filled = 192 of Q = 512: NaN or zeros in the slots 192 .. 511 (behind the documented rows too: the bank starts as all-NaN or
    all-zero), and another tail of bank_labels, give the same bits -- and the values of the f64 oracle over the 192 valid rows."""
    Q, N, nmod = 512, 200, 3
    outs = []
    for fill, tail in ((NAN, None), (0.0, None), (NAN, 1)):
        bank = _bank_with(ops, Q, nmod, 192, N, fill)
        if tail is not None:
            bank.labels[192:] = _batch(N, nmod)[1][0].item()                 # a label that is a positive of row 0
        outs.append(_run(ops, bank, N, T07))
        if fill != fill:
            assert all(torch.isnan(bank.rows(m)[192:]).all() for m in range(nmod))
    for other in outs[1:]:
        assert torch.equal(outs[0][0], other[0]) and torch.equal(outs[0][2], other[2])
        for x, y in zip(outs[0][1], other[1]):
            assert torch.equal(x, y)
    _check("xbm_invalid_slots", *outs[0], _oracle_for(bank, N, T07), T07, dict(N=N, Q=Q, filled=192, nmod=nmod))


# ------------------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("N,Q,filled,nmod", [(200, 1024, 1024, 3), (64, 256, 192, 2)])
def test_two_calls_give_the_same_bits(ops, N, Q, filled, nmod):
    bank = _bank_with(ops, Q, nmod, filled, N)
    a = _run(ops, bank, N, T07)
    b = _run(ops, bank, N, T07)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    loss_only, _, so = _run(ops, bank, N, T07, want_dz=False)
    assert torch.equal(loss_only, a[0]) and so[0].item() == 0.0 and so[1].item() == a[2][1].item()


# ------------------------------------------------------------------------------------------------------------ 7. roles
def test_every_modality_gets_both_roles_and_the_bank_none(ops):
    """nmod = 3, each modality's dz against the oracle on its own.  The bank's rows differ per modality and the own rows' scales
    differ per modality, so a missing column-role term, or a bank column leaking into it, moves one modality past the gate.  A
    wrong oracle says by how much: the row role alone is 5 % or more away from the whole gradient, for every modality."""
    N, Q, nmod = 64, 256, 3
    bank = _bank_with(ops, Q, nmod, 192, N)
    ref = _oracle_for(bank, N, T07)
    loss, dzs, so = _run(ops, bank, N, T07)
    each = _check("xbm_roles", loss, dzs, so, ref, T07, dict(N=N, Q=Q, filled=192, nmod=nmod))
    assert len(each) == 3
    # the row role alone (what a kernel without the column term would return) is far outside the gate, for every modality
    zs, labels, _, _ = _batch(N, nmod)
    zd = [z.double().requires_grad_(True) for z in zs]
    zn = [F.normalize(z, dim=1) for z in zd]
    s = math.exp(T07)
    all_lab = torch.cat([labels, bank.labels[:192].cpu()])
    T = (labels[:, None] == all_lab[None, :]).double()
    total = 0.0
    for a in range(nmod):
        for b in range(nmod):
            if a != b:
                C = torch.cat([zn[b].detach(), bank.rows(b)[:192].cpu().double()])
                x = s * (zn[a] @ C.t())
                total = total + (T.sum(1) * torch.logsumexp(x, 1) - (T * x).sum(1)).sum() / N
    (total / 6).backward()
    for m in range(nmod):
        assert rel_err(zd[m].grad, ref[1][m]) > 0.05, m
        assert rel_err(dzs[m], zd[m].grad) > 0.05, m


# ------------------------------------------------------------------------------------------------------------ 8. captured graph
def test_a_captured_graph_advances_the_ring(ops):
    """Enqueue + loss captured once (XBM's order: the loss on the bank as it stands, then the enqueue), replayed three times with
    new embeddings staged into the static inputs: loss, dz, bank and state after each replay equal three eager steps bit for bit."""
    N, Q, nmod = 64, 256, 2
    steps = [_draw(N, 0, 20, nmod, 900 + s) for s in range(4)]
    tt = torch.tensor([T07], dtype=F32, device="cuda")

    def step(bank, zs, labels, loss, dzs, so):
        ops.infonce_xbm(zs, labels, tt, bank.banks, bank.labels, bank.state, loss, dzs, so, bank.ws(ops, N))
        ops.xbm_enqueue(zs, labels, bank.banks, bank.labels, bank.state, bank.ws(ops, N))

    def outputs():
        return torch.zeros(1, device="cuda"), [torch.empty(N, D, device="cuda") for _ in range(nmod)], torch.empty(2, device="cuda")

    eager = Bank(ops, Q, nmod)
    want = []
    for zs, labels in steps:
        out = outputs()
        step(eager, [z.cuda() for z in zs], labels.cuda(), *out)
        torch.cuda.synchronize()
        want.append((out, eager.snapshot()))

    graphed = Bank(ops, Q, nmod)
    static_z = [z.cuda().clone() for z in steps[0][0]]
    static_l = steps[0][1].cuda().clone()
    out = outputs()
    step(graphed, static_z, static_l, *out)                                  # step 0 eagerly: the workspace comes to exist
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(graphed, static_z, static_l, *out)
    torch.cuda.synchronize()
    assert graphed.state.tolist() == [N, N]                                  # the capture itself ran nothing
    for s in range(1, 4):
        for dst, src in zip(static_z, steps[s][0]):
            dst.copy_(src)
        static_l.copy_(steps[s][1])
        g.replay()
        torch.cuda.synchronize()
        (w_loss, w_dz, w_so), (w_banks, w_labels, w_state) = want[s]
        assert graphed.state.tolist() == w_state.tolist() == [((s + 1) * N) % Q, min((s + 1) * N, Q)], s
        assert torch.equal(out[0], w_loss) and torch.equal(out[2], w_so), s
        for x, y in zip(out[1], w_dz):
            assert torch.equal(x, y), s
        banks, labels, _ = graphed.snapshot()
        assert torch.equal(labels, w_labels), s
        for x, y in zip(banks, w_banks):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), s
    assert graphed.guards_ok()


def test_autograd_node_and_criterion(ops):
    """``functional.infonce_xbm`` returns the entry point's numbers and sends dLoss/dt to a learnable scale; the criterion computes
    on the bank as it stands and enqueues afterwards in train mode, reads only in eval mode, and keeps its buffers out of the state
    dict."""
    from bioscanclip.hip.functional import infonce_xbm
    from bioscanclip.model.loss_func import MemoryBankContrastiveLoss
    N, Q, nmod = 64, 256, 2
    _, _, zd, ld = _batch(N, nmod)
    param = torch.nn.Parameter(torch.tensor(T07, device="cuda"))
    crit = MemoryBankContrastiveLoss(torch.nn.CrossEntropyLoss(), param, memory_bank_size=Q)
    zs = [z.clone().requires_grad_(True) for z in zd]
    first = crit(zs[0], zs[1], None, ld)
    assert int(crit.filled()) == N and crit.filled().is_cuda and not crit.state_dict()
    plain = Bank(ops, Q, nmod)
    loss0, dz0, so0 = _run(ops, plain, N, T07)                               # the first step saw an empty bank
    assert torch.equal(first.detach().reshape(1), loss0) and torch.equal(first.scale_out, so0)
    (2 * first).backward()
    assert torch.equal(param.grad, 2 * so0[0]) and all(torch.equal(z.grad, 2 * d) for z, d in zip(zs, dz0))
    plain.enqueue(ops, zd, ld)
    loss1, _, _ = _run(ops, plain, N, T07)
    crit.eval()
    second = crit(zd[0], zd[1], None, ld)                                   # eval: the bank of one step, nothing enqueued
    assert torch.equal(second.detach().reshape(1), loss1) and int(crit.filled()) == N
    assert second.item() != first.item()
    node = infonce_xbm(zd, ld, param, crit.bank())
    assert torch.equal(node.detach().reshape(1), loss1)
    fixed = MemoryBankContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07, memory_bank_size=Q)
    assert abs(fixed(zd[0], zd[1], None, ld).item() - loss0.item()) < 2e-5 * loss0.item() and not fixed.state_dict()
    assert abs(fixed.current_scale().item() - 1 / 0.07) < 1e-5
    crit.reset()
    assert int(crit.filled()) == 0
    with pytest.raises(ValueError, match="the bank holds"):
        crit(zd[0], None, zd[1], ld)


# ------------------------------------------------------------------------------------------------------------ 9. script
_CHILD = """
import json, sys
sys.path.insert(0, {scripts!r})
import train_cl
for name, argv in {runs!r}:
    print("RUN " + name, flush=True)
    losses = train_cl.main(argv)
    print("LOSSES " + json.dumps([float(x) for x in losses]), flush=True)
"""


def test_train_cl_with_a_memory_bank(tmp_path):
    """One fresh child process runs ``train_cl.py`` with ``memory_bank_size=256`` (5 steps of 8: the captured step included) and
    then without the option."""
    scripts = os.path.join(ROOT, "bioscan-clip_amd", "scripts")
    golden = {k for k in load_golden("state_dict_keys")["keys"] if not k.startswith("language_encoder.")}
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.batch_size=8", "model_config.epochs=1",
              "synthetic_steps_per_epoch=5", "synthetic_eval=true", "synthetic_eval_batches=1", "save_ckpt=true", "debug_flag=false"]
    runs = [(name, common + extra + [f"project_root_path={tmp_path / name}"])
            for name, extra in (("bank", ["model_config.memory_bank_size=256"]), ("default", []))]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bioscan-clip_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-c", _CHILD.format(scripts=scripts, runs=runs)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    parts = res.stdout.split("RUN ")[1:]
    assert [p.split("\n", 1)[0] for p in parts] == ["bank", "default"]
    found, lines = {}, {}
    for name, out in zip(("bank", "default"), parts):
        losses = [ln for ln in out.splitlines() if ln.startswith("LOSSES ")]
        assert len(losses) == 1 and all(math.isfinite(x) for x in json.loads(losses[0][7:]))
        epoch = [ln for ln in out.splitlines() if ln.startswith("Epoch [")]
        assert len(epoch) == 1
        assert ("memory bank: 40/256" in epoch[0]) == (name == "bank"), epoch     # min(5 x 8, 256)
        assert ("memory bank" in out) == (name == "bank")
        ck = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path / name)) for f in fs if f == "last.pth"]
        assert ck
        found[name] = torch.load(ck[0], map_location="cpu")
        lines[name] = [re.sub(r"[-+]?\d[\d.e+-]*", "#", ln.replace(", memory bank: 40/256", ""))
                       for ln in out.splitlines()[1:] if ln and not ln.startswith(("LOSSES", "Last ckpt"))]
    assert set(found["bank"]) == set(found["default"]) == golden
    # with the option off the run prints the parent's lines: those of the run with it on less the bank count (numbers masked)
    assert lines["bank"] == lines["default"]
