"""GPU tests of the supervised fine-tuning path: the classifier head Linear(768, C) on the split-bf16 GEMM, the fused cross-entropy
(bsclip_ce_fwd_bwd), the class top-k (bsclip_class_topk) and the epoch drivers.

The oracle is torch's own definition in float64 on the CPU: ``F.linear`` + ``F.cross_entropy(reduction="mean")`` and its autograd.

Gates.  The head runs on split-bf16 operands (hi.hi + lo.hi + hi.lo, ~2^-16 per product), so it is not an f32 computation; each
quantity is gated at twice the larger of two measured relative distances to the f64 reference over the four shapes of
``SHAPES``: this head's and torch's own f32 computation on the same GPU.  Measured on an MI355X (worst of the four shapes):

    quantity   this head   torch f32   gate
    loss       3.97e-7     4.57e-8     7.9e-7
    dz         3.71e-6     6.30e-7     7.4e-6
    dW         3.58e-6     2.94e-7     7.1e-6
    db         1.21e-6     1.36e-7     2.4e-6

``loss`` is |got - ref| / |ref|, the gradients are Frobenius-norm relative distances.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import rel_err, skip_param_init  # noqa: E402

D = 768
SHAPES = [(3, 5), (33, 130), (64, 128), (256, 1213)]
# twice the larger measured distance (docstring table: 2 x 3.97e-7, 3.71e-6, 3.58e-6, 1.21e-6, rounded down to two digits)
GATES = {"loss": 7.9e-7, "dz": 7.4e-6, "dW": 7.1e-6, "db": 2.4e-6}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _case(B, C, z_scale=1.0, seed=0, bad=()):
    """Seeded inputs and the f64 reference (computed once per shape, shared, never modified).  ``bad``: (row, target) pairs that put
    an out-of-range target into the batch; the reference then covers the remaining rows only, divisor still B."""
    g = _gen(1000 * B + C + seed)
    z = torch.randn(B, D, generator=g) * z_scale
    W = torch.randn(C, D, generator=g) / math.sqrt(D)
    b = torch.randn(C, generator=g)
    t = torch.randint(0, C, (B,), generator=g)
    t[0], t[1] = 0, C - 1                            # the first and the last class are always among the targets
    keep = torch.ones(B, dtype=torch.bool)
    for r, v in bad:
        t[r] = v
        keep[r] = False
    zd, Wd, bd = z.double().requires_grad_(True), W.double().requires_grad_(True), b.double().requires_grad_(True)
    logits = F.linear(zd, Wd, bd)
    if bad:
        loss = F.cross_entropy(logits[keep], t[keep], reduction="sum") / B
    else:
        loss = F.cross_entropy(logits, t, reduction="mean")
    loss.backward()
    ref = {"loss": loss.detach(), "dz": zd.grad, "dW": Wd.grad, "db": bd.grad, "logits": logits.detach()}
    return z, W, b, t, ref


def _dist(got, ref):
    out = {"loss": abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))}
    for k in ("dz", "dW", "db"):
        out[k] = rel_err(got[k], ref[k])
    return out


def _poison_padding(B, C):
    """NaN-free garbage in everything the head's padded operand buffers hold beyond class C - 1: weight rows [C, Cn) of the split operand,
    their bias entries.  A head that read them as real classes would put e^(1e4) into every softmax."""
    from bioscanclip.hip import functional as HF
    ws = HF._head_workspace(B, C, torch.device("cuda", torch.cuda.current_device()))
    ws.w3[C:].fill_(1e4)
    ws.bias[C:].fill_(1e4)
    return ws


def _run_hip(z, W, b, t, flag=None, poison=True):
    from bioscanclip.hip import functional as HF
    zc = z.cuda().requires_grad_(True)
    Wc, bc = nn.Parameter(W.cuda()), nn.Parameter(b.cuda())
    if poison:
        _poison_padding(z.shape[0], W.shape[0])
    loss = HF.linear_cross_entropy(zc, Wc, bc, t.cuda(), flag=flag)
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach().cpu(), "dz": zc.grad.cpu(), "dW": Wc.grad.cpu(), "db": bc.grad.cpu()}


def _run_torch_f32(z, W, b, t):
    zc, Wc, bc = (x.cuda().requires_grad_(True) for x in (z, W, b))
    loss = F.cross_entropy(F.linear(zc, Wc, bc), t.cuda(), reduction="mean")
    loss.backward()
    return {"loss": loss.detach().cpu(), "dz": zc.grad.cpu(), "dW": Wc.grad.cpu(), "db": bc.grad.cpu()}


def measure():
    """The figures behind GATES: per shape, the distance of this head and of torch's f32 computation to the f64 reference."""
    rows = []
    for B, C in SHAPES:
        z, W, b, t, ref = _case(B, C)
        rows.append({"shape": (B, C), "hip": _dist(_run_hip(z, W, b, t), ref), "torch_f32": _dist(_run_torch_f32(z, W, b, t), ref)})
    return rows


def _assert_gated(d, what):
    print(what, d)
    for k, v in d.items():
        assert v <= GATES[k], f"{what}: {k} is {v:.3e} from the f64 reference, gate {GATES[k]:.3e}"


# ------------------------------------------------------------------------------------------------- 1. loss and gradients
@pytest.mark.parametrize("B,C", SHAPES)
def test_loss_and_gradients_match_f64(B, C):
    z, W, b, t, ref = _case(B, C)
    assert t[0] == 0 and t[1] == C - 1
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _run_hip(z, W, b, t, flag=flag)          # padded weight rows and bias entries hold 1e4: masked, not merely zero
    assert int(flag.item()) == 0
    _assert_gated(_dist(got, ref), f"head ({B}, {C})")


@pytest.mark.parametrize("B,C", [(3, 5), (33, 130), (256, 1213)])
def test_ce_kernel_reads_and_writes_inside_its_bounds(B, C):
    """bsclip_ce_fwd_bwd on buffers whose padding rows and columns are NaN: the logits buffer is untouched, NaN padding columns never
    reach the loss, and the outputs are written inside [B, C] (f32) / [B, 3 Cp] (split form, zeros in [C, Cp)) only."""
    from bioscanclip.hip import ops
    z, W, b, t, ref = _case(B, C)
    Cp, ld = (C + 63) // 64 * 64, (C + 127) // 128 * 128 + 4
    x32 = ref["logits"].float()
    buf = torch.full((B + 2, ld), float("nan"), device="cuda")
    buf[:B, :C] = x32.cuda()
    before = buf.clone()
    dl = torch.full((B + 2, ld), float("nan"), device="cuda")
    dl3 = torch.full((B + 2, 3 * Cp + 8), float("nan"), device="cuda", dtype=torch.bfloat16)
    loss = torch.full((3,), float("nan"), device="cuda")
    row_loss = torch.full((B + 1,), float("nan"), device="cuda")
    ops.ce_fwd_bwd(buf[:B], t.cuda().to(torch.int32), C, loss[:1], row_loss[:B], dl[:B], dl3[:B])
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), buf.view(torch.int32)), "the logits buffer was written"
    assert torch.isnan(dl[B:]).all() and torch.isnan(dl[:B, C:]).all(), "dlogits written outside [B, C]"
    assert torch.isnan(dl3[B:].float()).all() and torch.isnan(dl3[:B, 3 * Cp:].float()).all(), "split dlogits written outside [B, 3 Cp]"
    assert torch.isnan(loss[1:]).all() and torch.isnan(row_loss[B:]).all()
    # f64 cross-entropy of the same f32 logits: only the kernel's own f32 arithmetic separates the two.  exp / log / divide are
    # good to a few ulp (2^-23) and the argument x - max is rounded to 2^-24 |x - max| <= 1.2e-6 for |x - max| <= 20: 4e-6 bounds both.
    xd = x32.double().requires_grad_(True)
    want = F.cross_entropy(xd, t, reduction="mean")
    want.backward()
    assert abs(loss[0].item() - want.item()) <= 4e-6 * abs(want.item())
    assert rel_err(dl[:B, :C], xd.grad) <= 4e-6
    parts = dl3[:B, :3 * Cp].float().view(B, 3, Cp)
    assert torch.isfinite(parts).all() and (parts[:, :, C:] == 0).all(), "padded columns of the split operand must be zeros"
    assert torch.equal(parts[:, 0], parts[:, 2])                                  # [hi | lo | hi]
    assert torch.equal(parts[:, 0, :C], dl[:B, :C].bfloat16().float())            # hi = bf16(d)
    assert rel_err(parts[:, 0, :C].double() + parts[:, 1, :C].double(), dl[:B, :C].double()) <= 2.0 ** -16


# ------------------------------------------------------------------------------------------------- 2. extreme logits
def test_extreme_logits_are_finite_and_exact():
    """Logits up to +-1e4 and one row whose logits are all equal: the maximum is subtracted first, so nothing overflows; the equal row
    gives log C."""
    from bioscanclip.hip import functional as HF
    B, C = 64, 130
    g = _gen(77)
    z = torch.randn(B, D, generator=g) * 92.0            # logit std = 92 sqrt(768) ~ 2.5e3: the extremes pass 1e4
    W = torch.randn(C, D, generator=g)
    b = torch.full((C,), 0.5)
    z[5] = 0.0                                           # every logit of row 5 is the bias: 0.5
    t = torch.randint(0, C, (B,), generator=g)
    logits = F.linear(z.double(), W.double(), b.double())
    assert logits.abs().max() >= 1e4
    want = F.cross_entropy(logits, t, reduction="mean")
    got = _run_hip(z, W, b, t)
    ws = HF._head_workspace(B, C, torch.device("cuda", torch.cuda.current_device()))
    row5 = ws.row_loss[5].item()
    d = abs(got["loss"].item() - want.item()) / abs(want.item())
    print("extreme logits: loss", got["loss"].item(), "f64", want.item(), "distance", d, "row 5", row5, "log C", math.log(C))
    assert all(torch.isfinite(v).all() for v in got.values())
    assert abs(row5 - math.log(C)) <= 4 * 2.0 ** -24 * math.log(C)      # log(130.f) to a few f32 ulp
    assert d <= GATES["loss"], f"loss {d:.3e} from f64, gate {GATES['loss']:.3e}"


# ------------------------------------------------------------------------------------------------- 3. accumulation, determinism
def test_gradients_accumulate_and_repeat_bit_for_bit():
    from bioscanclip.hip import functional as HF
    B, C = 256, 1213                                       # the split-K form of the dW product
    z, W, b, t, _ = _case(B, C)
    Wc, bc, tc = nn.Parameter(W.cuda()), nn.Parameter(b.cuda()), t.cuda()

    def once():
        zc = z.cuda().requires_grad_(True)
        loss = HF.linear_cross_entropy(zc, Wc, bc, tc)
        loss.backward()
        return loss.detach().clone(), zc.grad.clone()

    l1, dz1 = once()
    dW1, db1 = Wc.grad.clone(), bc.grad.clone()
    l2, dz2 = once()                                       # no zero_grad in between: dW and db are accumulated
    assert torch.equal(l1, l2) and torch.equal(dz1, dz2), "the same call twice must give the same bits"
    assert torch.equal(Wc.grad, 2 * dW1) and torch.equal(bc.grad, 2 * db1), "two backward calls must leave twice the gradient"
    Wc.grad, bc.grad = None, None
    l3, dz3 = once()
    assert torch.equal(l3, l1) and torch.equal(dz3, dz1) and torch.equal(Wc.grad, dW1) and torch.equal(bc.grad, db1)


# ------------------------------------------------------------------------------------------------- 4. out-of-range targets
def test_out_of_range_targets_are_flagged_and_contribute_nothing():
    B, C = 33, 130
    bad = ((3, C), (7, -1))
    z, W, b, t, ref = _case(B, C, bad=bad)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _run_hip(z, W, b, t, flag=flag)
    assert int(flag.item()) & 1, "a target of C and a target of -1 must set the flag"
    assert (got["dz"][[3, 7]] == 0).all(), "rows with an out-of-range target must have an exactly zero gradient"
    assert (ref["dz"][[3, 7]] == 0).all()
    _assert_gated(_dist(got, ref), "head with out-of-range targets")


# ------------------------------------------------------------------------------------------------- 5. top-k
@functools.lru_cache(maxsize=None)
def _topk_case(B, C):
    """Inputs whose f64 logits decide every asserted position: no two of a row's 17 largest are closer than 1e-4 (asserted here, on the
    CPU), except the constructed exact ties -- class C - 3 duplicates class 2 (weight row and bias), and rows 0 .. 3 are pushed towards
    that class so that the tied pair leads their ranking."""
    seed = {(33, 130): 3, (256, 1213): 277}[(B, C)]     # found by a search on the CPU; the condition is asserted below
    g = _gen(seed)
    z = torch.randn(B, D, generator=g) * 3.0
    W = torch.randn(C, D, generator=g) / math.sqrt(D)
    b = torch.randn(C, generator=g)
    W[C - 3], b[C - 3] = W[2], b[2]
    z[:4] += 40.0 * W[2]
    logits = F.linear(z.double(), W.double(), b.double())
    logits[:, C - 3] = logits[:, 2]        # equal by construction; a BLAS may round the two columns' sums in different orders
    top = torch.sort(logits, dim=1, descending=True, stable=True)
    n = min(17, C)
    gaps = top.values[:, :n - 1] - top.values[:, 1:n]
    tie = ((top.indices[:, :n - 1] == 2) & (top.indices[:, 1:n] == C - 3))
    assert (gaps[tie] == 0).all() and tie[:4, 0].all(), "the constructed tie must lead rows 0 .. 3"
    assert (gaps[~tie] >= 1e-4).all(), f"seed {seed}: two of a row's top-17 f64 logits are closer than 1e-4"
    return z, W, b, top.indices


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("B,C", [(33, 130), (256, 1213)])
def test_class_topk_matches_f64_order(B, C, k):
    from bioscanclip.hip import functional as HF
    from bioscanclip.hip import ops
    z, W, b, order = _topk_case(B, C)
    _poison_padding(B, C)
    logits = HF.linear_logits(z.cuda(), W.cuda(), b.cuda())
    assert tuple(logits.shape) == (B, C)
    scores, idx = ops.class_topk(logits, C, k)
    assert torch.equal(idx.cpu(), order[:, :k]), "top-k indices differ from the f64 order (ties: lower class index first)"
    assert torch.equal(scores, torch.gather(logits, 1, idx))
    if k >= 2:
        assert (idx[:4, 0] == 2).all() and (idx[:4, 1] == C - 3).all(), "exact ties resolve to the lower class index"


# ------------------------------------------------------------------------------------------------- 6. end to end
E2E_B, E2E_C = 8, 5
SPECIES = [f"s{i}" for i in range(E2E_C)]


def _classifiers(seed=0):
    from oracle import synth
    import test_20_encoders_gpu as t20
    from bioscanclip.model import arch
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from bioscanclip.util.util import EncoderWithExtraLayer
    with skip_param_init():
        vit = LoRA_ViT_timm(arch.VisionTransformerParams(depth=2), r=4, num_classes=768)
    t20._load(vit, "image_encoder.", 13)
    bert = LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=2)), r=4, num_classes=768)
    sd = synth.synth_state_dict({"dna_encoder." + k: v for k, v in synth.shapes_of(bert).items()}, 11)
    bert.load_state_dict({k[len("dna_encoder."):]: v for k, v in sd.items()})
    torch.manual_seed(11 + seed)                 # the Linear's init and the dropout site seeds
    return (EncoderWithExtraLayer(vit, nn.Linear(768, E2E_C)).cuda(), EncoderWithExtraLayer(bert, nn.Linear(768, E2E_C)).cuda())


def _batches(n, same=False):
    from oracle import synth
    out = []
    for s in range(n):
        image, dna, _, _ = synth.synth_batch(E2E_B, seed=31 + (0 if same else s))
        zeros = torch.zeros(E2E_B, 20, dtype=torch.int64)
        species = [SPECIES[(i + (0 if same else s)) % E2E_C] for i in range(E2E_B)]
        out.append(([f"p{s}_{i}" for i in range(E2E_B)], image, dna, zeros, zeros, zeros, {"species": species}))
    return out


class _Args:
    activate_wandb = False


def _fixed_loss(clfs, batch):
    from bioscanclip.epoch.fine_tuning_epoch import label_batch_to_species_idx
    t = label_batch_to_species_idx(batch[6], SPECIES).cuda()
    for m in clfs:
        m.eval()
    with torch.no_grad():
        return sum(m.loss(x.cuda(), t).item() for m, x in zip(clfs, (batch[1], batch[2])))


def test_fine_tuning_epochs_train_and_evaluate():
    from bioscanclip.epoch import fine_tuning_epoch as fte
    from bioscanclip.hip import ops
    from bioscanclip.hip.optim import FusedAdamW
    img, dna = _classifiers()
    params = [p for m in (img, dna) for p in m.parameters() if p.requires_grad]
    opt = FusedAdamW(params, lr=1e-3)
    crit = nn.CrossEntropyLoss()
    dev = torch.device("cuda", torch.cuda.current_device())
    loss = fte.fine_tuning_epoch_image_and_dna(_Args(), img, dna, _batches(4), opt, crit, SPECIES, 0, dev)
    assert math.isfinite(loss) and loss > 0
    named = [(f"{w}.{k}", p) for w, m in (("image", img), ("dna", dna)) for k, p in m.named_parameters() if p.requires_grad]
    assert any(k.endswith("new_linear_layer.weight") for k, _ in named) and len(named) > 4
    for k, p in named:                            # the last step's gradients are still in place
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, f"{k}: gradient missing, zero or non-finite"
    fixed = _batches(1, same=True)[0]
    before = _fixed_loss((img, dna), fixed)
    fte.fine_tuning_epoch_image_and_dna(_Args(), img, dna, [fixed] * 10, opt, crit, SPECIES, 1, dev)
    after = _fixed_loss((img, dna), fixed)
    print("epoch loss", loss, "fixed batch before", before, "after 10 steps", after)
    assert after < before, f"10 steps on one batch did not lower its loss: {before} -> {after}"
    # one classifier, the single-modality driver
    one = fte.fine_tuning_epoch(_Args(), dna, _batches(2), opt, crit, SPECIES, 2, dev, modality="dna")
    assert math.isfinite(one)
    # evaluate_epoch against the same predictions scored with numpy on the host
    evalb = _batches(3)
    for modality, m, col in (("image", img, 1), ("dna", dna, 2)):
        acc = fte.evaluate_epoch(m, evalb, dev, SPECIES, k_values=[1, 3, 5], modality=modality)
        preds, targets = [], []
        with torch.no_grad():
            for batch in evalb:
                preds.append(ops.class_topk(m(batch[col].cuda()), E2E_C, 5)[1].cpu().numpy())
                targets.append(fte.label_batch_to_species_idx(batch[6], SPECIES).numpy())
        preds, targets = np.concatenate(preds), np.concatenate(targets)
        for k in (1, 3, 5):
            want = np.mean(np.any(preds[:, :k] == targets[:, None], axis=1))
            assert acc[f"top{k}_accuracy"] == want, f"{modality} top-{k}: {acc[f'top{k}_accuracy']} vs {want} on the host"
        assert acc["top5_accuracy"] == 1.0        # five classes: the target is always among the five


def test_encoder_gradients_come_from_the_heads_dz():
    """What this feature contributes is the head's dz; the encoders' backward is the existing one.  The encoder gradients of one
    fused step equal those of the same encoder fed the f64 reference head's dz by hand -- to the accuracy of that backward.  It runs
    on a bf16 gradient stream: the two dz differ in their last bits (the head's gated distance, ~4e-6), every bf16 rounding stage
    turns a relative difference d into ~sqrt(d x 2^-8) (the share of elements whose rounding flips, times the size of a flip), and
    after the stages of two layers the two passes are two independently rounded evaluations of one gradient.  Each is within the
    engine's own distance to the f32 oracle, which tests/test_20_encoders_gpu.py measures and gates for these 2-layer encoders
    (TOL: worst gradient tensor 2.7e-2 for the ViT, 3.0e-2 for BarcodeBERT); that documented error of the reference path is the gate
    here -- looser than 1e-3 for this reason.  A wrong dz (a missing 1 / B, a shifted row, a sign) is an O(1) distance.  Measured on an
    MI355X: worst tensor 5.3e-3 (ViT), 3.9e-3 (BarcodeBERT); the heads' own tensors 1.2e-4 and below."""
    from bioscanclip.epoch.fine_tuning_epoch import label_batch_to_species_idx
    clfs = _classifiers(seed=1)
    batch = _batches(1)[0]
    t = label_batch_to_species_idx(batch[6], SPECIES)
    import test_20_encoders_gpu as t20
    for m, x, gate in zip(clfs, (batch[1].cuda(), batch[2].cuda()), (t20.TOL["vit_L2"][1], t20.TOL["dna_L2"][1])):
        m.train()
        enc_params = {k: p for k, p in m.encoder.named_parameters() if p.requires_grad}

        def reset():
            for p in m.parameters():
                p.grad = None
            eng = getattr(m.encoder, "_engine", None)
            if eng is not None and getattr(eng, "_step_word", None) is not None:
                eng._step_word.zero_()            # both forwards draw the dropout masks of step 1

        m.get_feature(x)                          # builds the engine
        reset()
        m.loss(x, t.cuda()).backward()
        fused = {k: p.grad.detach().clone() for k, p in enc_params.items()}
        reset()
        feat = m.get_feature(x)
        zd = feat.detach().cpu().double().requires_grad_(True)
        lin = m.new_linear_layer
        F.cross_entropy(F.linear(zd, lin.weight.detach().cpu().double(), lin.bias.detach().cpu().double()), t).backward()
        feat.backward(zd.grad.float().cuda())
        torch.cuda.synchronize()
        for k, p in enc_params.items():
            d = rel_err(fused[k], p.grad)
            print("encoder gradient", type(m.encoder).__name__, k, d)
            assert fused[k].abs().max().item() > 0 and d <= gate, f"{k}: {d:.3e} (gate {gate:.1e}) between the fused step and the reference head's dz"
