"""InfoNCE with a learnable logit scale (``bsclip_infonce_fwd_bwd_ts``): dLoss/dt against f64 in all three forms, the bits of the
fixed-scale entry, the clamp, the own-rows share, repeatability, pad guards, and the way up: autograd node, the temperature's flat
buffer under FusedAdamW, the captured step, ``train_cl.py``.

Inputs are in the trained regime (diagonal cosines ~0.8), where ``cnt p - T`` cancels: z_m = base + 0.5 noise_m.  The bar on dLoss/dt
is ``(1 + 2 s) 2^-16 A`` with ``A = s/(P N) sum (cnt_i p_ij + T_ij) |G_ij|`` in f64: the split-bf16 product leaves 2^-16 relative on
each cosine, which enters each term once directly and through p amplified by at most 2 s.  Measured |hip - f64| / bar per case goes
to test_20's parity log (``t20._log``)."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_golden, rel_err  # noqa: E402
from oracle import refcpu, synth  # noqa: E402
import test_20_encoders_gpu as t20  # noqa: E402  (its parity log)
import test_30_graph_gpu as t30  # noqa: E402  (its model builder)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_log = t20._log
T07 = math.log(1 / 0.07)
LN50 = math.log(50.0)
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture()
def ops():
    from bioscanclip.hip import ops as o
    yield o
    o.infonce_set_impl(0)


# ------------------------------------------------------------------------------------------------------------ inputs and oracle
_INPUTS, _ORACLE = {}, {}


def _inputs(N, nmod, dup):
    key = (N, nmod, dup)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + N + nmod)
        base = torch.randn(N, 768, generator=g)
        zs = [base + 0.5 * torch.randn(N, 768, generator=g) for _ in range(nmod)]
        label = torch.arange(N)
        if dup:
            label = label // 3 * 3
        _INPUTS[key] = (zs, label, [z.cuda() for z in zs], label.cuda())
    return _INPUTS[key]


def _oracle(N, nmod, t, dup):
    """f64: loss, dLoss/dz, dLoss/dt of refcpu.contrastive_loss at logit_scale = exp(t), and the bar's A.  Computed once per case."""
    key = (N, nmod, t, dup)
    if key not in _ORACLE:
        zs, label, _, _ = _inputs(N, nmod, dup)
        zd = [z.double().requires_grad_(True) for z in zs]
        td = torch.tensor(t, dtype=torch.float64, requires_grad=True)
        loss = refcpu.contrastive_loss(zd[0], zd[1], zd[2] if nmod == 3 else None, label, logit_scale=torch.exp(td))
        loss.backward()
        with torch.no_grad():
            s = math.exp(t)
            zn = [z / z.norm(dim=1, keepdim=True) for z in zd]
            T = (label[:, None] == label[None, :]).double()
            cnt = T.sum(1, keepdim=True)
            A = 0.0
            for a in range(nmod):
                for b in range(nmod):
                    if a != b:
                        G = zn[a] @ zn[b].t()
                        A += ((cnt * torch.softmax(s * G, dim=1) + T) * G.abs()).sum().item()
            A *= s / (nmod * (nmod - 1) * N)
        _ORACLE[key] = (loss.item(), [z.grad for z in zd], td.grad.item(), A)
    return _ORACLE[key]


def _padded(numel, pad):
    buf = torch.full((numel + pad,), float("nan"), dtype=F32, device="cuda")
    return buf, buf[:numel]


def _run(ops, N, nmod, t, dup, impl, row0=0, n_local=None, want_dz=True):
    """One call of the new entry on NaN-filled outputs with spare elements behind them; returns (loss, dzs or None, scale_out) after
    checking that nothing was written past the ends (the pad guard)."""
    _, _, zd, ld = _inputs(N, nmod, dup)
    n_local = N if n_local is None else n_local
    ops.infonce_set_impl(impl)
    ws = torch.empty(ops.infonce_workspace_floats(N, nmod), dtype=F32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    so_buf, so = _padded(2, 62)
    bufs = [_padded(n_local * 768, 768) for _ in range(nmod)] if want_dz else None
    dzs = [v.view(n_local, 768) for _, v in bufs] if want_dz else None
    tt = torch.tensor([t], dtype=F32, device="cuda")
    ops.infonce_fwd_bwd_ts(zd, ld, tt, loss, dzs, so, row0=row0, n_local=n_local, workspace=ws)
    torch.cuda.synchronize()
    assert torch.isnan(so_buf[2:]).all() and not torch.isnan(so).any(), "scale_out: written past its two floats, or not written"
    if want_dz:
        for b, v in bufs:
            assert torch.isnan(b[n_local * 768:]).all() and not torch.isnan(v).any(), "dz: written past its end, or not fully written"
    return loss, dzs, so


def _fixed(ops, N, nmod, scale, dup, impl, row0=0, n_local=None, want_dz=True):
    _, _, zd, ld = _inputs(N, nmod, dup)
    n_local = N if n_local is None else n_local
    ops.infonce_set_impl(impl)
    ws = torch.empty(ops.infonce_workspace_floats(N, nmod), dtype=F32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    dzs = [torch.empty(n_local, 768, device="cuda") for _ in range(nmod)] if want_dz else None
    ops.infonce_fwd_bwd(zd, ld, scale, loss, dzs, row0=row0, n_local=n_local, workspace=ws)
    return loss, dzs


# ------------------------------------------------------------------------------------------------------------ 1. gradient vs f64
CASES = [(8, 3, T07, True, 0),
         (200, 3, T07, True, 0),      # batched, N not a multiple of 256
         (256, 2, 0.0, False, 0),
         (300, 2, LN50, True, 1),     # slab, launch by launch, Np = 512
         (300, 2, LN50, True, 2),     # fused, two column tiles to merge
         (256, 3, T07, True, 2),      # fused, one tile
         (1100, 2, T07, True, 0)]     # more than one 1024-row slab


@pytest.mark.parametrize("N,nmod,t,dup,impl", CASES)
def test_temperature_gradient_vs_f64(ops, N, nmod, t, dup, impl):
    ref_loss, ref_dz, ref_dt, A = _oracle(N, nmod, t, dup)
    loss, dzs, so = _run(ops, N, nmod, t, dup, impl)
    s = math.exp(t)
    bar = (1 + 2 * s) * 2.0 ** -16 * A
    err = abs(so[0].item() - ref_dt)
    loss_err = abs(loss.item() - ref_loss) / abs(ref_loss)
    dz_err = max(rel_err(dzs[i], ref_dz[i]) for i in range(nmod))
    print(f"N={N} nmod={nmod} t={t:.4f} impl={impl}: dLoss/dt hip {so[0].item():.8e} f64 {ref_dt:.8e} |diff| {err:.3e} bar {bar:.3e} "
          f"ratio {err / bar:.4f}; loss rel {loss_err:.2e}; dz rel {dz_err:.2e}")
    _log({"test": "infonce_temperature", "N": N, "nmod": nmod, "t": t, "impl": impl, "dt_hip": so[0].item(), "dt_f64": ref_dt,
          "bar": bar, "ratio": err / bar, "bar_over_dt": bar / abs(ref_dt), "loss_rel": loss_err, "dz_rel": dz_err})
    assert abs(so[1].item() - s) <= 2e-7 * s
    assert loss_err < 2e-5, (loss.item(), ref_loss)
    assert dz_err < 2e-4
    assert err <= bar, (so[0].item(), ref_dt, err, bar)


# ------------------------------------------------------------------------------------------------------------ 2. same bits
@pytest.mark.parametrize("N,nmod,impl", [(200, 3, 0), (300, 2, 1), (300, 2, 2)])
@pytest.mark.parametrize("t", [T07, 0.0])
def test_same_bits_as_the_fixed_scale_entry(ops, N, nmod, impl, t):
    loss, dzs, so = _run(ops, N, nmod, t, True, impl)
    s = so[1].item()
    if t == 0.0:
        assert s == 1.0
    ref_loss, ref_dz = _fixed(ops, N, nmod, s, True, impl)
    assert torch.equal(loss, ref_loss)
    for a, b in zip(dzs, ref_dz):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 3. clamp
@pytest.mark.parametrize("t,s", [(-0.5, 1.0), (5.0, 100.0)])
def test_clamp(ops, t, s):
    loss, dzs, so = _run(ops, 200, 3, t, True, 0)
    assert so[1].item() == s and so[0].item() == 0.0
    ref_loss, ref_dz = _fixed(ops, 200, 3, s, True, 0)
    assert torch.equal(loss, ref_loss)
    for a, b in zip(dzs, ref_dz):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 4. own rows
@pytest.mark.parametrize("N,nmod,impl", [(256, 3, 0), (300, 2, 2)])
def test_own_rows_shares_add_up(ops, N, nmod, impl):
    _, _, _, A = _oracle(N, nmod, T07, True)
    whole_loss, _, whole = _run(ops, N, nmod, T07, True, impl)
    total = 0.0
    for lo, hi in ((0, N // 4), (N // 4, 3 * N // 4), (3 * N // 4, N)):
        loss, _, so = _run(ops, N, nmod, T07, True, impl, row0=lo, n_local=hi - lo)
        assert torch.equal(loss, whole_loss)
        assert so[0].item() != 0.0
        total += so[0].item()
    print(f"N={N} impl={impl}: whole {whole[0].item():.8e} sum of shares {total:.8e} 1e-5 A {1e-5 * A:.3e}")
    assert abs(total - whole[0].item()) <= 1e-5 * A
    loss, _, so = _run(ops, N, nmod, T07, True, impl, want_dz=False)
    assert torch.equal(loss, whole_loss) and so[0].item() == 0.0 and so[1].item() == whole[1].item()
    _, _, so = _run(ops, N, nmod, T07, True, impl, row0=N // 2, n_local=0)
    assert so[0].item() == 0.0


# ------------------------------------------------------------------------------------------------------------ 5. repeat
@pytest.mark.parametrize("N,nmod,impl", [(200, 3, 0), (300, 2, 1), (300, 2, 2)])
def test_repeat_gives_the_same_bits(ops, N, nmod, impl):
    a = _run(ops, N, nmod, T07, True, impl)
    b = _run(ops, N, nmod, T07, True, impl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


def test_wrapper_checks(ops):
    _, _, zd, ld = _inputs(8, 3, True)
    ws = torch.empty(ops.infonce_workspace_floats(8, 3), dtype=F32, device="cuda")
    loss, so = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
    for bad in (torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.float64), torch.zeros(1), 2.5):
        with pytest.raises(ValueError, match="log_scale"):
            ops.infonce_fwd_bwd_ts(zd, ld, bad, loss, None, so, workspace=ws)
    with pytest.raises(ValueError, match="scale_out"):
        ops.infonce_fwd_bwd_ts(zd, ld, torch.zeros(1, device="cuda"), loss, None, torch.zeros(1, device="cuda"), workspace=ws)
    with pytest.raises(ValueError, match="Too less element"):
        ops.infonce_fwd_bwd_ts(zd[:1], ld, torch.zeros(1, device="cuda"), loss, None, so, workspace=ws)


# ------------------------------------------------------------------------------------------------------------ 7. autograd
def test_autograd_node(ops, monkeypatch):
    from bioscanclip.hip.functional import infonce
    N, nmod = 200, 3
    _, _, zd, ld = _inputs(N, nmod, True)
    calls = []
    for name in ("infonce_fwd_bwd", "infonce_fwd_bwd_ts"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=real, **k: (calls.append(_n), _f(*a, **k))[1])
    param = torch.nn.Parameter(torch.tensor(T07, device="cuda"))
    zs = [z.clone().requires_grad_(True) for z in zd]
    loss = infonce(zs, ld, param)
    assert calls == ["infonce_fwd_bwd_ts"]
    (3 * loss).backward()
    _, dzs, so = _run(ops, N, nmod, T07, True, 0)
    assert torch.equal(loss.scale_out, so)
    assert param.grad.shape == param.shape and torch.equal(param.grad, 3 * so[0])
    for z, d in zip(zs, dzs):
        assert torch.equal(z.grad, 3 * d)
    # inputs that need no gradient: the temperature's is still formed
    param.grad = None
    infonce(zd, ld, param).backward()
    assert torch.equal(param.grad, so[0])
    # a float scale still takes the fixed-scale node and entry
    calls.clear()
    zs = [z.clone().requires_grad_(True) for z in zd]
    fixed = infonce(zs, ld, so[1].item())
    assert calls == ["infonce_fwd_bwd"] and not hasattr(fixed, "scale_out")
    assert torch.equal(fixed.detach(), loss.detach())
    with pytest.raises(ValueError, match="log scale"):
        infonce(zd, ld, torch.zeros(2, device="cuda"))


# ------------------------------------------------------------------------------------------------------------ 8. optimizer
@pytest.mark.parametrize("dev_hyper", [False, True])
def test_fused_adamw_updates_the_temperature_buffer(dev_hyper):
    from bioscanclip.hip.dist import flat_buffers
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.simple_clip import SimpleCLIP
    model = SimpleCLIP(None, None, None)
    model.logit_scale = torch.nn.Parameter(torch.tensor(T07, device="cuda"))
    model.bind_temperature()
    (flat,) = flat_buffers(model)
    assert flat.data.numel() == 4 and flat.valid() and model.logit_scale.grad.data_ptr() == flat.grad.data_ptr()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    opt.enable_device_hyper(dev_hyper)
    opt.attach(model)
    p, m, v = torch.tensor(T07, dtype=torch.float64), torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for step, g in enumerate((0.75, -0.2, 0.4), 1):
        opt.zero_grad()
        flat.grad[0] = g
        lr = 1e-3 * step
        opt.param_groups[0]["lr"] = lr
        opt.step()
        refcpu.adamw_update(p, torch.tensor(float(torch.tensor(g, dtype=F32)), dtype=torch.float64), m, v, step, lr)
        assert abs(model.logit_scale.item() - p.item()) < 1e-6, (step, model.logit_scale.item(), p.item())
    assert model.logit_scale.item() != T07 and (flat.data[1:] == 0).all()      # weight decay 0.01 applies to t; the padding stays 0


# ------------------------------------------------------------------------------------------------------------ 9. graph
def test_graphed_step_with_a_moving_temperature():
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    steps = 6
    batches = [synth.synth_batch(16, seed=300 + s % 3, with_text=False) for s in range(steps)]
    runs = {}
    for mode in ("eager", "graph"):
        model = t30._build(91, False)
        model.logit_scale = torch.nn.Parameter(torch.tensor(T07, device="cuda"))
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        opt.enable_device_hyper(True)
        crit = ContrastiveLoss(torch.nn.CrossEntropyLoss(), model.logit_scale)
        g = GraphedStep(model, opt, crit, warmup=2) if mode == "graph" else None
        snaps, scales = [], []
        for s in range(steps):
            image, dna, _, label = batches[s]
            image, dna, label = image.cuda(), dna.cuda(), label.cuda()
            t_before = model.logit_scale.item()
            if g is not None:
                g(image, dna, None, label)
            else:
                opt.zero_grad()
                loss = crit(*model(image, dna, None), label)
                loss.backward()
                if opt.needs_attach():
                    opt.attach(model)
                opt.step()
            cur = crit.current_scale()
            assert cur.is_cuda and cur.dim() == 0
            assert abs(cur.item() - math.exp(t_before)) <= 1e-6 * math.exp(t_before), (mode, s)   # the scale the step's forward used
            scales.append(cur.item())
            snaps.append({k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad})
        if g is not None:
            assert g.graph is not None
        assert "logit_scale" in snaps[0] and snaps[0]["logit_scale"].item() != torch.tensor(T07, dtype=F32).item()
        assert len(set(scales)) == steps                                       # the temperature moves on every step, replays included
        runs[mode] = (snaps, scales)
    assert runs["eager"][1] == runs["graph"][1]
    for s in range(steps):
        for k, v in runs["eager"][0][s].items():
            assert torch.equal(v, runs["graph"][0][s][k]), (s, k)


# ------------------------------------------------------------------------------------------------------------ 10. script
def test_train_cl_and_inference_with_a_trainable_temperature(tmp_path, capsys):
    scripts = os.path.join(ROOT, "bioscan-clip_amd", "scripts")
    sys.path.insert(0, scripts)
    import inference_and_eval
    import train_cl
    golden = {k for k in load_golden("state_dict_keys")["keys"] if not k.startswith("language_encoder.")}
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.batch_size=8", "model_config.epochs=1",
              "synthetic_steps_per_epoch=2", "synthetic_eval=true", "synthetic_eval_batches=1", "save_ckpt=true", "debug_flag=false"]
    found = {}
    for name, extra in (("on", ["model_config.trainable_temperature=true"]), ("off", [])):
        root = tmp_path / name
        capsys.readouterr()
        losses = train_cl.main(common + extra + [f"project_root_path={root}"])
        out = capsys.readouterr().out
        assert len(losses) == 1 and all(math.isfinite(float(x)) for x in losses)
        assert ("logit scale:" in out) == (name == "on")
        ck = [os.path.join(r, f) for r, _, fs in os.walk(str(root)) for f in fs if f == "last.pth"]
        assert ck
        found[name] = (ck[0], torch.load(ck[0], map_location="cpu"))
    assert set(found["on"][1]) == golden | {"logit_scale"}
    assert set(found["off"][1]) == golden
    t = found["on"][1]["logit_scale"]
    assert t.shape == () and t.dtype == F32 and t.item() != torch.tensor(T07, dtype=F32).item() and abs(t.item() - T07) < 0.01
    # the evaluation script never reads the temperature: a model built without the option loads the checkpoint that carries it
    acc, _, _ = inference_and_eval.main(["model_config=lora_vit_lora_barcode_bert_ssl", f"model_config.ckpt_path={found['on'][0]}",
                                         f"project_root_path={tmp_path}", "debug_flag=false", "synthetic_eval_batches=1"])
    assert acc["encoded_image_feature"]["encoded_dna_feature"]["seen"]["micro_acc"][1]
