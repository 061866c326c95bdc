"""The sigmoid (SigLIP) contrastive loss with a learnable scale and bias (``bsclip_sigmoid_loss_fwd_bwd``): loss, dLoss/dt, dLoss/db
and dz against f64 in the batched and the slab form, saturation, the own-rows shares, repeatability and pad guards, symmetry, and the
way up: autograd node, the two scalars' flat buffer under FusedAdamW, the captured step, ``train_cl.py``.

Inputs are in the trained regime (diagonal cosines ~0.8): z_m = base + 0.5 noise_m, labels arange(N) // 3 * 3.  The oracle is the
formula of include/bsclip.h in torch f64 with autograd (``_formula``).

Gates.  The split-bf16 product leaves 2^-16 relative on each cosine G.  To first order that moves a cell's term by s 2^-16 |w| |G|,
its w G by s 2^-16 |G| (|w| + s |G| / 4) and its w by s 2^-16 |G| / 4 (|d sigmoid| <= 1/4), which gives the derived bounds
  loss:     s 2^-16 / (P N) * sum |w| |G|
  dLoss/dt: s 2^-16 / (P N) * sum |G| (|w| + s |G| / 4)
  dLoss/db: s 2^-16 / (4 P N) * sum |G|
computed in f64 from the oracle's G and w over the directed pairs.  Each gate is its derived bound plus 4 x the error of a torch CPU
f32 evaluation of the same formula (f32 matmul, f32 sums) against f64 on the same inputs: the baseline for f32 evaluation and
accumulation order, with the factor test_61_silhouette uses as headroom for another order.  dz: rel_err <= 4 x the f32 baseline's
rel_err + 2 s 2^-16.  Measured / gate of every case goes to test_20's parity log (``t20._log``)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import load_golden, rel_err  # noqa: E402
from oracle import refcpu, synth  # noqa: E402
import test_20_encoders_gpu as t20  # noqa: E402  (its parity log)
import test_30_graph_gpu as t30  # noqa: E402  (its model builder)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_log = t20._log
LN10 = math.log(10.0)
LN100 = math.log(100.0)
T07 = math.log(1 / 0.07)
F32 = torch.float32
EPS16 = 2.0 ** -16
POINTS = [(LN10, -10.0), (T07, -5.0), (0.0, 0.0)]
SIZES = [(8, 3), (200, 3), (256, 2), (300, 2), (1100, 2)]   # smallest batched; N % 256 != 0; one full tile; Np = 512; two slabs


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture()
def ops():
    from bioscanclip.hip import ops as o
    return o


# ------------------------------------------------------------------------------------------------------------ inputs and oracle
_INPUTS, _ORACLE = {}, {}


def _inputs(N, nmod):
    key = (N, nmod)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(2000 + N + nmod)
        base = torch.randn(N, 768, generator=g)
        zs = [base + 0.5 * torch.randn(N, 768, generator=g) for _ in range(nmod)]
        label = torch.arange(N) // 3 * 3
        _INPUTS[key] = (zs, label, [z.cuda() for z in zs], label.cuda())
    return _INPUTS[key]


def _formula(zs, label, t, b, dtype):
    """The loss of include/bsclip.h in ``dtype`` on the CPU with autograd: (loss, [dz], dt, db, [G^{ab}], [w^{ab}]) over the directed pairs."""
    zd = [z.detach().to(dtype).clone().requires_grad_(True) for z in zs]     # fresh leaves: the shared inputs stay as they are
    td = torch.tensor(t, dtype=dtype, requires_grad=True)
    bd = torch.tensor(b, dtype=dtype, requires_grad=True)
    nmod, N = len(zs), zs[0].shape[0]
    s = torch.exp(torch.clamp(td, 0.0, LN100))
    zn = [F.normalize(z, dim=1) for z in zd]
    y = torch.where(label[:, None] == label[None, :], 1.0, -1.0).to(dtype)
    total, Gs, ws = 0.0, [], []
    for a in range(nmod):
        for c in range(nmod):
            if a != c:
                G = zn[a] @ zn[c].t()
                u = -y * (s * G + bd)
                total = total + (-F.logsigmoid(-u)).sum()        # softplus(u), the stable form
                Gs.append(G.detach())
                ws.append((-y * torch.sigmoid(u)).detach())
    loss = total / (nmod * (nmod - 1) * N)
    loss.backward()
    return loss.item(), [z.grad for z in zd], td.grad.item(), bd.grad.item(), Gs, ws


def _oracle(N, nmod, t, b):
    """f64 values, the derived bounds, the f32 baseline's errors and the sum |.| terms of the share test.  Computed once per case."""
    key = (N, nmod, t, b)
    if key not in _ORACLE:
        zs, label, _, _ = _inputs(N, nmod)
        loss, dz, dt, db, Gs, ws = _formula(zs, label, t, b, torch.float64)
        s = math.exp(min(max(t, 0.0), LN100))
        den = nmod * (nmod - 1) * N
        sum_wg = sum((w.abs() * G.abs()).sum().item() for G, w in zip(Gs, ws))
        sum_w = sum(w.abs().sum().item() for w in ws)
        bound = {"loss": s * EPS16 / den * sum_wg,
                 "dt": s * EPS16 / den * sum((G.abs() * (w.abs() + s * G.abs() / 4)).sum().item() for G, w in zip(Gs, ws)),
                 "db": s * EPS16 / (4 * den) * sum(G.abs().sum().item() for G in Gs)}
        l32, dz32, dt32, db32, _, _ = _formula(zs, label, t, b, torch.float32)
        base = {"loss": abs(l32 - loss), "dt": abs(dt32 - dt), "db": abs(db32 - db),
                "dz": [rel_err(a, r) for a, r in zip(dz32, dz)]}
        _ORACLE[key] = {"loss": loss, "dz": dz, "dt": dt, "db": db, "s": s, "bound": bound, "base": base,
                        "abs_dt": s / den * sum_wg, "abs_db": sum_w / den}
    return _ORACLE[key]


def _padded(numel, pad):
    buf = torch.full((numel + pad,), float("nan"), dtype=F32, device="cuda")
    return buf, buf[:numel]


def _run(ops, N, nmod, t, b, row0=0, n_local=None, want_dz=True, zd=None):
    """One call of the entry on NaN-filled outputs with spare elements behind them; returns (loss, dzs or None, aux) after checking
    that nothing was written past the ends and nothing was left unwritten (the pad guard)."""
    _, _, zin, ld = _inputs(N, nmod)
    zd = zin if zd is None else zd
    n_local = N if n_local is None else n_local
    ws = torch.empty(ops.infonce_workspace_floats(N, nmod), dtype=F32, device="cuda")
    loss_buf, loss = _padded(1, 63)
    aux_buf, aux = _padded(4, 60)
    bufs = [_padded(n_local * 768, 768) for _ in range(nmod)] if want_dz else None
    dzs = [v.view(n_local, 768) for _, v in bufs] if want_dz else None
    tt = torch.tensor([t], dtype=F32, device="cuda")
    bb = torch.tensor([b], dtype=F32, device="cuda")
    ops.sigmoid_loss_fwd_bwd(zd, ld, tt, bb, loss, dzs, aux, row0=row0, n_local=n_local, workspace=ws)
    torch.cuda.synchronize()
    assert torch.isnan(loss_buf[1:]).all() and not torch.isnan(loss).any(), "loss_out: written past its float, or not written"
    assert torch.isnan(aux_buf[4:]).all() and not torch.isnan(aux).any(), "aux_out: written past its four floats, or not fully written"
    if want_dz:
        for buf, v in bufs:
            assert torch.isnan(buf[n_local * 768:]).all() and not torch.isnan(v).any(), "dz: written past its end, or not fully written"
    assert tt.item() == torch.tensor(t, dtype=F32).item() and bb.item() == torch.tensor(b, dtype=F32).item()   # inputs untouched
    return loss, dzs, aux


def _check_against_f64(ops, N, nmod, t, b, what):
    o = _oracle(N, nmod, t, b)
    loss, dzs, aux = _run(ops, N, nmod, t, b)
    got = {"loss": loss.item(), "dt": aux[0].item(), "db": aux[2].item()}
    rec = {"test": what, "N": N, "nmod": nmod, "t": t, "b": b}
    failures = []
    for k in ("loss", "dt", "db"):
        gate = o["bound"][k] + 4 * o["base"][k]
        err = abs(got[k] - o[k])
        print(f"N={N} nmod={nmod} t={t:.4f} b={b}: {k} hip {got[k]:.9e} f64 {o[k]:.9e} |diff| {err:.3e} gate {gate:.3e} "
              f"(bound {o['bound'][k]:.3e} + 4 x f32 {o['base'][k]:.3e}) ratio {err / gate if gate else float('inf'):.4f}")
        rec.update({k + "_err": err, k + "_gate": gate, k + "_ratio": err / gate if gate else None})
        if not (math.isfinite(got[k]) and err <= gate):
            failures.append((k, got[k], o[k], err, gate))
    for m in range(nmod):
        gate = 4 * o["base"]["dz"][m] + 2 * o["s"] * EPS16
        err = rel_err(dzs[m], o["dz"][m])
        print(f"N={N} nmod={nmod} t={t:.4f} b={b}: dz[{m}] rel {err:.3e} gate {gate:.3e} ratio {err / gate:.4f}")
        rec.update({f"dz{m}_err": err, f"dz{m}_gate": gate, f"dz{m}_ratio": err / gate})
        if not (torch.isfinite(dzs[m]).all() and err <= gate):
            failures.append((f"dz[{m}]", err, gate))
    _log(rec)
    assert abs(aux[1].item() - o["s"]) <= 2e-7 * o["s"] and aux[3].item() == torch.tensor(b, dtype=F32).item()
    assert not failures, failures
    return loss, dzs, aux


# ------------------------------------------------------------------------------------------------------------ 1. against f64
@pytest.mark.parametrize("t,b", POINTS)
@pytest.mark.parametrize("N,nmod", SIZES)
def test_against_f64(ops, N, nmod, t, b):
    _check_against_f64(ops, N, nmod, t, b, "sigmoid_loss")


# ------------------------------------------------------------------------------------------------------------ 2. saturation
@pytest.mark.parametrize("b", [30.0, -30.0])
def test_saturation(ops, b):
    """t = 5 lies beyond the clamp (s is exactly 100, no gradient reaches t) and x = 100 G +- 30 reaches +-130."""
    N, nmod, t = 200, 3, 5.0
    zs, label, _, _ = _inputs(N, nmod)
    zn = [F.normalize(z, dim=1) for z in zs]
    x = 100.0 * (zn[0] @ zn[1].t()) + b
    if b > 0:   # the positives sit at x ~ 110: the naive log(1 + exp(x)) overflows in f32 (with b = -30 they sit at ~50, the rest at ~-30)
        assert x.max().item() > 100.0 and not torch.isfinite(torch.log(1 + torch.exp(x))).all()
    _, _, aux = _check_against_f64(ops, N, nmod, t, b, "sigmoid_loss_saturation")
    assert aux[1].item() == 100.0 and aux[0].item() == 0.0
    assert _oracle(N, nmod, t, b)["dt"] == 0.0


# ------------------------------------------------------------------------------------------------------------ 3. own rows
@pytest.mark.parametrize("N,nmod", [(256, 3), (1100, 2)])
def test_own_rows_shares(ops, N, nmod):
    """Each slice's dz is asserted equal to the whole call's rows bit for bit: a cell's logit, its w and the dz products run the same
    128 x 128 GEMM program with the same K loop for every row count at these sizes, so the accumulation order does not differ."""
    t, b = POINTS[0]
    o = _oracle(N, nmod, t, b)
    whole_loss, whole_dz, whole = _run(ops, N, nmod, t, b)
    tot_t = tot_b = 0.0
    for lo, hi in ((0, N // 4), (N // 4, 3 * N // 4), (3 * N // 4, N)):
        loss, dzs, aux = _run(ops, N, nmod, t, b, row0=lo, n_local=hi - lo)
        assert torch.equal(loss, whole_loss)
        assert aux[0].item() != 0.0 and aux[2].item() != 0.0
        assert aux[1].item() == whole[1].item() and aux[3].item() == whole[3].item()
        tot_t += aux[0].item()
        tot_b += aux[2].item()
        for d, w in zip(dzs, whole_dz):
            assert torch.equal(d, w[lo:hi])
    print(f"N={N}: dt whole {whole[0].item():.8e} shares {tot_t:.8e} (1e-5 sum|.| {1e-5 * o['abs_dt']:.3e}); "
          f"db whole {whole[2].item():.8e} shares {tot_b:.8e} (1e-5 sum|.| {1e-5 * o['abs_db']:.3e})")
    assert abs(tot_t - whole[0].item()) <= 1e-5 * o["abs_dt"]
    assert abs(tot_b - whole[2].item()) <= 1e-5 * o["abs_db"]
    loss, _, aux = _run(ops, N, nmod, t, b, want_dz=False)
    assert torch.equal(loss, whole_loss) and aux[0].item() == 0.0 and aux[2].item() == 0.0
    assert aux[1].item() == whole[1].item() and aux[3].item() == whole[3].item()
    loss, _, aux = _run(ops, N, nmod, t, b, row0=N // 2, n_local=0)
    assert torch.equal(loss, whole_loss) and aux[0].item() == 0.0 and aux[2].item() == 0.0


# ------------------------------------------------------------------------------------------------------------ 4. repeat, pad guards
@pytest.mark.parametrize("N,nmod", [(200, 3), (1100, 2)])
def test_repeat_gives_the_same_bits(ops, N, nmod):
    t, b = POINTS[1]
    first = _run(ops, N, nmod, t, b)       # _run holds the pad guards of loss_out, aux_out[4] and every dz
    second = _run(ops, N, nmod, t, b)
    assert torch.equal(first[0], second[0]) and torch.equal(first[2], second[2])
    for x, y in zip(first[1], second[1]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ 5. symmetry
def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("N", [200, 1100])
def test_swapping_two_modalities(ops, N):
    """The pair's logits are formed once for the loss, as zn^0 (zn^1)^T: after the swap they are the transposed product with the
    hi.lo and lo.hi parts of the split operands in the other K order, so loss and the scalar gradients are held to 1 f32 ulp, not to
    equal bits.  The backward forms both directed products, and those swap with the inputs: dz swaps bit for bit."""
    t, b = POINTS[0]
    _, _, zd, _ = _inputs(N, 2)
    loss, dzs, aux = _run(ops, N, 2, t, b)
    loss_s, dzs_s, aux_s = _run(ops, N, 2, t, b, zd=[zd[1], zd[0]])
    assert torch.equal(dzs[0], dzs_s[1]) and torch.equal(dzs[1], dzs_s[0])
    for name, x, y in (("loss", loss.item(), loss_s.item()), ("dt", aux[0].item(), aux_s[0].item()), ("db", aux[2].item(), aux_s[2].item())):
        print(f"N={N} {name}: {x:.9e} swapped {y:.9e} diff {abs(x - y):.3e} ulp {_ulp(max(abs(x), abs(y))):.3e}")
        assert abs(x - y) <= _ulp(max(abs(x), abs(y))), (name, x, y)
    assert aux[1].item() == aux_s[1].item() and aux[3].item() == aux_s[3].item()


# ------------------------------------------------------------------------------------------------------------ 6. autograd
def test_autograd_node(ops, monkeypatch):
    from bioscanclip.hip.functional import sigmoid_loss
    N, nmod = 200, 3
    t, b = POINTS[0]
    _, _, zd, ld = _inputs(N, nmod)
    calls = []
    real = ops.sigmoid_loss_fwd_bwd
    monkeypatch.setattr(ops, "sigmoid_loss_fwd_bwd", lambda *a, **k: (calls.append(k.get("n_local")), real(*a, **k))[1])
    pt = torch.nn.Parameter(torch.tensor(t, device="cuda"))
    pb = torch.nn.Parameter(torch.tensor(b, device="cuda"))
    zs = [z.clone().requires_grad_(True) for z in zd]
    loss = sigmoid_loss(zs, ld, pt, pb)
    assert len(calls) == 1                                            # one node, one call: the backward launches nothing
    (3 * loss).backward()
    assert len(calls) == 1
    raw_loss, dzs, aux = _run(ops, N, nmod, t, b)
    assert torch.equal(loss.detach().reshape(1), raw_loss) and torch.equal(loss.aux_out, aux)
    assert pt.grad.shape == pt.shape and torch.equal(pt.grad, 3 * aux[0])
    assert pb.grad.shape == pb.shape and torch.equal(pb.grad, 3 * aux[2])
    for z, d in zip(zs, dzs):
        assert torch.equal(z.grad, 3 * d)
    # only the scalars need a gradient
    pt.grad = pb.grad = None
    sigmoid_loss(zd, ld, pt, pb).backward()
    assert torch.equal(pt.grad, aux[0]) and torch.equal(pb.grad, aux[2])
    # only one input and the bias need one
    pb.grad = None
    z0 = zd[0].clone().requires_grad_(True)
    sigmoid_loss([z0, zd[1], zd[2]], ld, pt.detach(), pb).backward()
    assert torch.equal(z0.grad, dzs[0]) and torch.equal(pb.grad, aux[2]) and zd[1].grad is None
    # nothing needs one: loss only, no dz is formed and the shares are zero
    out = sigmoid_loss(zd, ld, pt.detach(), pb.detach())
    assert not out.requires_grad and torch.equal(out.reshape(1), raw_loss)
    assert out.aux_out[0].item() == 0.0 and out.aux_out[2].item() == 0.0 and out.aux_out[1].item() == aux[1].item()
    # the own rows of a gathered batch
    zs = [z.clone().requires_grad_(True) for z in zd]
    sigmoid_loss(zs, ld, pt.detach(), pb.detach(), row0=50, n_local=100).backward()
    assert torch.equal(zs[0].grad[50:150], dzs[0][50:150]) and not zs[0].grad[:50].any() and not zs[0].grad[150:].any()
    with pytest.raises(ValueError, match="log_scale"):
        sigmoid_loss(zd, ld, torch.zeros(2, device="cuda"), pb)
    with pytest.raises(ValueError, match="bias"):
        sigmoid_loss(zd, ld, pt, -10.0)
    with pytest.raises(ValueError, match="Too less element"):
        sigmoid_loss(zd[:1], ld, pt, pb)


def test_wrapper_checks(ops):
    _, _, zd, ld = _inputs(8, 3)
    ws = torch.empty(ops.infonce_workspace_floats(8, 3), dtype=F32, device="cuda")
    loss, aux, good = torch.zeros(1, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(1, device="cuda")
    for bad in (torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.float64), torch.zeros(1), 2.5):
        with pytest.raises(ValueError, match="log_scale"):
            ops.sigmoid_loss_fwd_bwd(zd, ld, bad, good, loss, None, aux, workspace=ws)
        with pytest.raises(ValueError, match="bias"):
            ops.sigmoid_loss_fwd_bwd(zd, ld, good, bad, loss, None, aux, workspace=ws)
    with pytest.raises(ValueError, match="aux_out"):
        ops.sigmoid_loss_fwd_bwd(zd, ld, good, good, loss, None, torch.zeros(3, device="cuda"), workspace=ws)
    with pytest.raises(ValueError, match="Too less element"):
        ops.sigmoid_loss_fwd_bwd(zd[:1], ld, good, good, loss, None, aux, workspace=ws)


# ------------------------------------------------------------------------------------------------------------ 7. optimizer
def _scalar_model():
    from bioscanclip.hip.dist import flat_buffers
    from bioscanclip.model.simple_clip import SimpleCLIP
    model = SimpleCLIP(None, None, None)
    model.logit_scale = torch.nn.Parameter(torch.tensor(LN10, device="cuda"))
    model.logit_bias = torch.nn.Parameter(torch.tensor(-10.0, device="cuda"))
    model.bind_temperature()
    (flat,) = flat_buffers(model)
    assert flat.data.numel() == 8 and flat.offsets == [0, 4] and flat.valid()
    assert model.logit_scale.grad.data_ptr() == flat.grad.data_ptr() and model.logit_bias.grad.data_ptr() == flat.grad.data_ptr() + 16
    return model, flat


@pytest.mark.parametrize("dev_hyper", [False, True])
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_fused_adamw_updates_both_scalars(dev_hyper, max_norm):
    """Three steps against ``refcpu.adamw_update`` in f64 (weight decay 0.01 applies to both).  With ``max_grad_norm`` the two
    gradients are the whole global norm: the recorded norm is theirs and the update runs on the clipped values."""
    from bioscanclip.hip.optim import FusedAdamW
    model, flat = _scalar_model()
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=max_norm, skip_nonfinite=max_norm is not None)
    opt.enable_device_hyper(dev_hyper)
    opt.attach(model)
    f64 = lambda x: torch.tensor(float(torch.tensor(x, dtype=F32)), dtype=torch.float64)
    ref = {k: (f64(v), torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)) for k, v in (("t", LN10), ("b", -10.0))}
    for step, (gt, gb) in enumerate(((0.75, -0.5), (-3.0, 4.0), (0.4, 0.3)), 1):
        opt.zero_grad()
        flat.grad[0] = gt
        flat.grad[4] = gb
        lr = 1e-3 * step
        opt.param_groups[0]["lr"] = lr
        opt.step()
        norm = math.hypot(float(f64(gt)), float(f64(gb)))
        coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
        if max_norm is not None:
            gs = opt.grad_stats()
            assert abs(gs["norm_last"] - norm) <= 1e-6 * norm and abs(gs["coef_last"] - coef) <= 1e-6, (step, gs, norm, coef)
        for k, g, p in (("t", gt, model.logit_scale), ("b", gb, model.logit_bias)):
            refcpu.adamw_update(ref[k][0], f64(g) * coef, ref[k][1], ref[k][2], step, lr)
            assert abs(p.item() - ref[k][0].item()) < 2e-6 * max(1.0, abs(ref[k][0].item())), (step, k, p.item(), ref[k][0].item())
    assert model.logit_scale.item() != torch.tensor(LN10, dtype=F32).item() and model.logit_bias.item() != -10.0
    assert (flat.data[1:4] == 0).all() and (flat.data[5:] == 0).all()          # the padding stays 0
    if max_norm is not None:
        gs = opt.grad_stats()
        assert (gs["steps"], gs["skipped"], gs["clipped"]) == (3, 0, 1)            # norms 0.90, 5.0 and 0.5: only the second is clipped


# ------------------------------------------------------------------------------------------------------------ 8. graph
def test_graphed_step_with_moving_scalars():
    """Six steps, eager against GraphedStep.  Before step 5 a checkpoint is loaded (the model's own weights, other values for the two
    scalars): the encoders drop their engines, the signature no longer matches the captured one, that step runs eagerly on the loaded
    scalars and the next one captures again.  A scalar buffer that was REPLACED (a parameter moved, as ``.to()`` moves it) changes
    the signature as well."""
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import SigmoidContrastiveLoss
    steps = 6
    batches = [synth.synth_batch(16, seed=300 + s % 3, with_text=False) for s in range(steps)]
    runs = {}
    for mode in ("eager", "graph"):
        model = t30._build(91, False)
        model.logit_scale = torch.nn.Parameter(torch.tensor(LN10, device="cuda"))
        model.logit_bias = torch.nn.Parameter(torch.tensor(-10.0, device="cuda"))
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        opt.enable_device_hyper(True)
        crit = SigmoidContrastiveLoss(model.logit_scale, model.logit_bias)
        g = GraphedStep(model, opt, crit, warmup=2) if mode == "graph" else None
        losses, ts, bs = [], [], []
        for s in range(steps):
            image, dna, _, label = batches[s]
            image, dna, label = image.cuda(), dna.cuda(), label.cuda()
            if s == 4:
                if g is not None:
                    assert g.graph is not None and g._signature() == g.captured_for
                ckpt = {k: v.clone() for k, v in model.state_dict().items()}
                ckpt.update(logit_scale=torch.tensor(2.0), logit_bias=torch.tensor(-8.0))
                model.load_state_dict(ckpt)
                assert model._temperature_flat.valid()                       # loaded in place: the scalars stay in their buffer
                if g is not None:
                    assert g._signature() != g.captured_for                  # caught: the step below must not replay
            t_before, b_before = model.logit_scale.item(), model.logit_bias.item()
            if s == 4:
                assert (t_before, b_before) == (2.0, -8.0)
            if g is not None:
                loss = g(image, dna, None, label)
                assert (g.graph is None) == (s in (0, 1, 4)), (s, g.graph)    # warm-up, and the eager step after the load
            else:
                opt.zero_grad()
                loss = crit(*model(image, dna, None), label)
                loss.backward()
                if opt.needs_attach():
                    opt.attach(model)
                opt.step()
            losses.append(loss.item())
            assert abs(crit.current_scale().item() - math.exp(t_before)) <= 1e-6 * math.exp(t_before), (mode, s)
            assert crit.current_bias().item() == b_before, (mode, s)                  # the values the step's forward used
            ts.append(model.logit_scale.item())
            bs.append(model.logit_bias.item())
        assert len(set(ts)) == steps and len(set(bs)) == steps                          # both move on every step, replays included
        assert ts[0] != torch.tensor(LN10, dtype=F32).item() and bs[0] != -10.0
        flat = model._temperature_flat
        assert flat.data.numel() == 8 and flat.valid()
        runs[mode] = (losses, ts, bs, {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad})
        if g is not None:
            assert g.graph is not None and (id(flat), None, flat.data.data_ptr()) in g._signature()
            model.logit_bias.data = model.logit_bias.data.clone()                       # the parameter left the buffer
            model.bind_temperature()
            assert model._temperature_flat is not flat and g._signature() != g.captured_for
    assert runs["eager"][0] == runs["graph"][0]
    assert runs["eager"][1] == runs["graph"][1] and runs["eager"][2] == runs["graph"][2]
    assert {"logit_scale", "logit_bias"} <= set(runs["eager"][3])
    for k, v in runs["eager"][3].items():
        assert torch.equal(v, runs["graph"][3][k]), k


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


def test_train_cl_with_the_sigmoid_loss(tmp_path):
    """One fresh child process runs ``train_cl.py`` with the sigmoid criterion and then with the default one."""
    import json
    scripts = os.path.join(ROOT, "bioscan-clip_amd", "scripts")
    golden = {k for k in load_golden("state_dict_keys")["keys"] if not k.startswith("language_encoder.")}
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.batch_size=8", "model_config.epochs=1",
              "synthetic_steps_per_epoch=2", "synthetic_eval=true", "synthetic_eval_batches=1", "save_ckpt=true", "debug_flag=false"]
    runs = [(name, common + extra + [f"project_root_path={tmp_path / name}"])
            for name, extra in (("sigmoid", ["model_config.contrastive_loss=sigmoid"]), ("default", []))]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bioscan-clip_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-c", _CHILD.format(scripts=scripts, runs=runs)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    parts = res.stdout.split("RUN ")[1:]
    assert [p.split("\n", 1)[0] for p in parts] == ["sigmoid", "default"]
    found = {}
    for name, out in zip(("sigmoid", "default"), parts):
        losses = [ln for ln in out.splitlines() if ln.startswith("LOSSES ")]
        assert len(losses) == 1 and all(math.isfinite(x) for x in json.loads(losses[0][7:]))
        epoch = [ln for ln in out.splitlines() if ln.startswith("Epoch [")]
        assert len(epoch) == 1
        assert ("logit scale:" in epoch[0] and "logit bias:" in epoch[0]) == (name == "sigmoid"), epoch
        assert ("logit scale:" in epoch[0] or "logit bias:" in epoch[0]) == (name == "sigmoid"), epoch
        ck = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path / name)) for f in fs if f == "last.pth"]
        assert ck
        found[name] = torch.load(ck[0], map_location="cpu")
    assert set(found["sigmoid"]) == golden | {"logit_scale", "logit_bias"}
    assert set(found["default"]) == golden
    t, b = found["sigmoid"]["logit_scale"], found["sigmoid"]["logit_bias"]
    assert t.shape == () and t.dtype == F32 and b.shape == () and b.dtype == F32
    assert t.item() != torch.tensor(LN10, dtype=F32).item() and abs(t.item() - LN10) < 0.01      # two AdamW steps at lr 1e-3
    assert b.item() != -10.0 and abs(b.item() + 10.0) < 0.01
