"""fp16-operand inference (set_operand_format(model, "fp16")): the forward's 16-bit kernels against f32 arithmetic on fp16-decoded
inputs, the three towers against the f32 oracle, against the oracle that rounds to fp16 where the kernels round (tests/fp16_oracle.py)
and against the reference's golden outputs, the properties of the fp16 engines, and the inference path end to end.

Gates of the encoder cases (test_20's five, same seeded weights, inputs and NODROP configuration, eval mode, no autograd):
  (b) HIP vs the fp16-emulating oracle <= 1.5 x (c) that oracle's own resolution (f32 vs f64 accumulation), floor 5e-4 -- test_20's
      criterion;
  (a) HIP vs the f32 oracle <= 1/3 of the bf16 engine's distance on the same model and inputs, and under the caps the CPU study
      (tools/fp16_sensitivity.py) leads to expect: 3e-3 for the 12-layer towers (and their 2-layer forms), 1e-3 for the text tower;
  the golden outputs of the imported reference (tests/golden/encoders.json) at the same caps.
Measured values are appended to test_20's parity log, in its record shape (test_20's own _log).
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fp16_oracle import fp16_rounding  # noqa: E402
from helpers import check_summary, load_golden, rel_err, skip_param_init  # noqa: E402
from oracle import refcpu, synth  # noqa: E402
from test_20_encoders_gpu import _log  # noqa: E402  (the same parity log as test_20's encoder cases)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
SELF_FACTOR = 1.5
CAP = {"dna_L2": 3e-3, "dna_L12": 3e-3, "txt_L4": 1e-3, "vit_L2": 3e-3, "vit_L12": 3e-3}
F16 = torch.float16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _nrm(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


# ------------------------------------------------------------------------------------------------------------- kernels
def _attn_ref(qkv, B, S, heads, scale, key_bias=None):
    """f32 attention on the fp16-decoded operands: (ctx [B S, heads 64], lse [B, heads, S])."""
    x = qkv.float().view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (x[0] @ x[1].transpose(-1, -2)) * scale
    if key_bias is not None:
        s = s + key_bias.view(B, 1, 1, S)
    lse = torch.logsumexp(s, dim=-1)
    ctx = (torch.softmax(s, dim=-1) @ x[2]).permute(0, 2, 1, 3).reshape(B * S, heads * 64)
    return ctx, lse


@pytest.mark.parametrize("S,heads,q_rows,masked", [(197, 12, 0, False), (197, 12, 1, False), (133, 12, 0, False), (20, 8, 0, True),
                                                   (100, 3, 0, True), (161, 2, 0, False),    # 4 and 6 key blocks (generic forms)
                                                   (40, 2, 0, False), (70, 2, 0, True), (150, 2, 0, False), (200, 2, 0, True)])   # 2, 3, 5, 7
def test_attention_forward_fp16(S, heads, q_rows, masked):
    from bioscanclip.hip import ops
    B, scale = 3, 0.125
    g = torch.Generator().manual_seed(S + q_rows)
    qkv = (torch.randn(B * S, 3 * heads * 64, generator=g) * 1.5).to(F16).cuda()
    kb = None
    if masked:   # padded keys as the text tower sees them: HF's finfo.min bias
        mask = torch.ones(B, S, dtype=torch.int64)
        mask[0, 14:], mask[2, 7:] = 0, 0
        kb = torch.empty(B, S, device="cuda")
        ops.mask_to_bias(mask.cuda(), kb)
    ctx = torch.zeros(B * S, heads * 64, dtype=F16, device="cuda")
    lse = torch.zeros(B, heads, S, device="cuda")
    ops.attn_fwd(qkv, B, S, heads, scale, ctx, lse, key_bias=kb, q_rows=q_rows)
    torch.cuda.synchronize()
    rc, rl = _attn_ref(qkv.cpu(), B, S, heads, scale, None if kb is None else kb.cpu())
    rows = torch.arange(B) * S if q_rows == 1 else torch.arange(B * S)
    e_ctx = _nrm(ctx.cpu()[rows], rc[rows])
    lrows = (slice(None), slice(None), slice(0, 1) if q_rows == 1 else slice(None))
    e_lse = _nrm(lse.cpu()[lrows], rl[lrows])
    _log({"test": f"fp16_attn_fwd_S{S}_q{q_rows}{'_mask' if masked else ''}", "ctx_vs_f32": e_ctx, "lse_vs_f32": e_lse})
    assert e_ctx <= 5e-4 and e_lse <= 1e-5, (e_ctx, e_lse)
    with pytest.raises(RuntimeError, match="dropout"):
        ops.attn_fwd(qkv, B, S, heads, scale, ctx, lse, dropout=(0.1, 1))
    with pytest.raises(ValueError, match="must all be bf16 or all fp16"):
        ops.attn_fwd(qkv, B, S, heads, scale, torch.zeros_like(ctx, dtype=torch.bfloat16), lse)


@pytest.mark.parametrize("H", [768, 512])
@pytest.mark.parametrize("x_dtype", ["fp16", "f32"])
@pytest.mark.parametrize("lora", [False, True])
def test_layernorm_forward_fp16(H, x_dtype, lora):
    from bioscanclip.hip import ops
    from bioscanclip.hip.lib import KPAD
    M = 300
    g = torch.Generator().manual_seed(H + len(x_dtype) + lora)
    x32 = torch.randn(M, H, generator=g) * 3 + 0.5
    x = (x32.to(F16) if x_dtype == "fp16" else x32).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(H, generator=g)).cuda()
    A = (0.05 * torch.randn(8, H, generator=g)).cuda() if lora else None
    y = torch.full((M, H + KPAD), float("nan"), dtype=F16, device="cuda")
    yf = torch.zeros(M, H, device="cuda")
    st = torch.zeros(M, 2, device="cuda")
    ops.layernorm_fwd(x, gamma, beta, 1e-6, y_bf16=y, y_f32=yf, lora_a=A, stats=st)
    torch.cuda.synchronize()
    ref = torch.nn.functional.layer_norm(x.float().cpu(), (H,), gamma.cpu(), beta.cpu(), 1e-6)
    assert _nrm(y[:, :H].cpu(), ref) <= 5e-4
    assert _nrm(yf.cpu(), ref) <= 1e-6
    assert torch.equal(y[:, :H].cpu(), yf.cpu().to(F16))          # the fp16 operand is the RNE rounding of the f32 output
    if lora:
        t = yf.cpu() @ A.cpu().t()
        assert _nrm(y[:, H:H + 8].cpu(), t) <= 1e-3
        assert (y[:, H + 8:H + KPAD] == 0).all()                   # zeros up to KPAD
    else:
        assert torch.isnan(y[:, H:].float()).all()                 # nothing written past H without LoRA
    with pytest.raises(ValueError, match="must all be bf16 or all fp16"):
        ops.layernorm_fwd(x.to(torch.bfloat16), gamma, beta, 1e-6, y_bf16=y)


def test_im2col_split_fp16_reconstructs_the_image():
    from bioscanclip.hip import ops
    image, _, _, _ = synth.synth_batch(2, seed=23)
    image = (image - 0.45) * 4      # normalised-like range, both signs
    cols = torch.zeros(2 * 196, 2304, dtype=F16, device="cuda")
    ops.im2col_patch16(image.cuda(), cols)
    plain = torch.zeros(2 * 196, 768, dtype=F16, device="cuda")
    ops.im2col_patch16(image.cuda(), plain)
    torch.cuda.synchronize()
    ref = image.reshape(2, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(2 * 196, 768)
    c = cols.cpu()
    hi, lo = c[:, :768], c[:, 768:1536]
    assert torch.equal(hi, ref.to(F16)) and torch.equal(c[:, 1536:], hi) and torch.equal(plain.cpu(), hi)
    assert torch.equal(lo, (ref - hi.float()).to(F16))
    e = _nrm(hi.double() + lo.double(), ref)
    _log({"test": "fp16_im2col_split", "hi_plus_lo_vs_image": e})
    assert e <= 2 ** -21, e


def test_cls_rows_lora_columns_and_cast_fp16_exact():
    from bioscanclip.hip import ops
    B, S, H = 3, 197, 768
    g = torch.Generator().manual_seed(5)
    cls, pos = torch.randn(H, generator=g).cuda(), torch.randn(S, H, generator=g).cuda()
    x = torch.zeros(B * S, H, dtype=F16, device="cuda")
    ops.vit_cls_rows(x, cls, pos, B, S, H)
    w = torch.zeros(3 * H, H + 64, dtype=F16, device="cuda")
    bq, bv = torch.randn(H, 4, generator=g).cuda(), torch.randn(H, 4, generator=g).cuda() * 1e-3
    table = torch.tensor([[w.data_ptr(), bq.data_ptr(), bv.data_ptr()]], dtype=torch.int64, device="cuda")
    ops.waug_set_lora_layers(table, 1, w.stride(0), H, dtype=F16)
    # the cast: RNE ties, subnormals, overflow to inf, signed zero, NaN
    vals = torch.tensor([1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, 2 ** -20, -2 ** -24, 2 ** -25 * 1.5, 65504.0, 65520.0, 1e6, -1e6,
                         -0.0, float("nan"), 3.14159265], dtype=torch.float32)
    src = torch.cat([vals, torch.randn(1001, generator=g) * 300]).cuda()
    dst = torch.zeros(src.numel(), dtype=F16, device="cuda")
    ops.cast_f32_bf16(src, dst)
    torch.cuda.synchronize()
    xr = x.cpu().view(B, S, H)
    assert torch.equal(xr[:, 0], (cls + pos[0]).cpu().to(F16).expand(B, H)) and not xr[:, 1:].any()
    wc = w.cpu()
    assert torch.equal(wc[:H, H:H + 4], bq.cpu().to(F16)) and torch.equal(wc[2 * H:, H + 4:H + 8], bv.cpu().to(F16))
    assert not wc[H:2 * H].any() and not wc[:H, H + 4:].any() and not wc[:, :H].any()
    want = src.cpu().to(F16)
    d = dst.cpu().float()
    num = ~torch.isnan(src.cpu())
    assert torch.equal(dst.cpu().view(torch.int16)[num], want.view(torch.int16)[num]) and torch.isnan(d[~num]).all()
    assert d[0] == 1.0 and d[1] == 1.0 + 4 * 2 ** -11 and d[2] == 2 ** -20 and d[3] == -2 ** -24 and d[4] == 2 ** -24
    assert d[6] == float("inf") and d[7] == float("inf") and d[8] == -float("inf") and d[5] == 65504.0


# ------------------------------------------------------------------------------------------------------------- encoders
def _case(name):
    from bioscanclip.model import arch
    if name.startswith("vit"):
        from bioscanclip.model.image_encoder import LoRA_ViT_timm
        depth = int(name[5:])
        with skip_param_init():
            m = LoRA_ViT_timm(arch.VisionTransformerParams(depth=depth), r=4, num_classes=768)
        prefix, seed = "image_encoder.", 13
        image, _, _, _ = synth.synth_batch(2, seed=23)
        fn = lambda s, emulate=False, f64=False: refcpu.vit_encoder(s, image.double() if f64 else image, emulate_bf16=emulate)
        return m, prefix, seed, image.cuda(), fn, (f"vit.out.{depth}", f"vit_L{depth}")
    if name.startswith("dna"):
        from bioscanclip.model.dna_encoder import LoRA_barcode_bert
        layers = int(name[5:])
        with skip_param_init():
            m = LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=layers, **NODROP)), r=4,
                                  num_classes=768)
        _, dna, _, _ = synth.synth_batch(2, seed=21)
        fn = lambda s, emulate=False, f64=False: refcpu.barcode_bert_encoder(s, dna, emulate_bf16=emulate)
        return m, "dna_encoder.", 11, dna.cuda(), fn, (f"dna.out.{layers}", f"dna_L{layers}")
    from bioscanclip.model.language_encoder import LoRA_bert
    m = LoRA_bert(arch.BertModelParams(arch.bert_small_config(**NODROP)), r=4, num_classes=768)
    _, _, text, _ = synth.synth_batch(4, seed=22, with_text=True)
    fn = lambda s, emulate=False, f64=False: refcpu.bert_text_encoder(s, text, emulate_bf16=emulate)
    return m, "language_encoder.", 12, {k: v.cuda() for k, v in text.items()}, fn, ("txt.out", "txt_L4")


def _load(module, prefix, seed):
    sd = synth.synth_state_dict({prefix + k: v for k, v in synth.shapes_of(module).items()}, seed)
    module.load_state_dict({k[len(prefix):]: v for k, v in sd.items()})
    return sd


def _f64(sd):
    return {k: (v.detach().double() if v.is_floating_point() else v) for k, v in sd.items()}


def _eval_forward(m, x, fmt):
    from bioscanclip.hip.engine import set_operand_format
    set_operand_format(m, fmt)
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    return y.clone()


@pytest.mark.parametrize("name", ["vit_L2", "vit_L12", "dna_L2", "dna_L12", "txt_L4"])
def test_encoder_fp16_forward(name):
    m, prefix, seed, x, fn, (gkey, gname) = _case(name)
    sd = _load(m, prefix, seed)
    m.to("cuda").eval()
    y = _eval_forward(m, x, "fp16")
    assert m._engine.fp16 and m._engine.ws["x" if name.startswith("vit") else "qkv"][0].dtype == F16
    y_bf = _eval_forward(m, x, "bf16")
    with torch.no_grad():
        yo = fn(sd)
        with fp16_rounding():
            y_emu = fn(sd, emulate=True)
            y_emu64 = fn(_f64(sd), emulate=True, f64=True)
    e_f32, e_emu, e_self, e_bf = rel_err(y, yo), rel_err(y, y_emu), rel_err(y_emu, y_emu64), rel_err(y_bf, yo)
    rec = {"test": f"fp16_{name}", "emb_vs_f32_oracle": e_f32, "emb_vs_fp16_emulating_oracle": e_emu,
           "emulating_oracle_f32acc_vs_f64acc": e_self, "emulating_oracle_vs_f32_oracle": rel_err(y_emu, yo),
           "bf16_engine_vs_f32_oracle": e_bf, "cap": CAP[name]}
    _log(rec)
    assert torch.isfinite(y).all()
    assert e_emu < max(SELF_FACTOR * e_self, 5e-4), rec
    assert e_f32 <= e_bf / 3, rec
    assert e_f32 <= CAP[name], rec
    check_summary(gkey, y, load_golden("encoders")[gname]["out"], CAP[name], what=f"fp16 {name} ")


# ------------------------------------------------------------------------------------------------------------- properties
def test_fp16_properties_vit():
    """Headroom (every saved activation finite, largest |value| logged against 65504), bit-identical repeats, batch invariance,
    a bf16 -> fp16 -> bf16 round trip that leaves the bf16 engine as it was."""
    m, prefix, seed, _, _, _ = _case("vit_L12")
    _load(m, prefix, seed)
    m.to("cuda").eval()
    image, _, _, _ = synth.synth_batch(8, seed=31)
    image = image.cuda()
    y1 = _eval_forward(m, image, "fp16")
    head = {}
    for site, t in m._engine.anomaly_probes():
        assert t.dtype == F16 or t.dtype == torch.float32, site
        assert torch.isfinite(t.float()).all(), site
        head[site] = float(t.float().abs().max())
    _log({"test": "fp16_vit_L12_headroom", "max_abs_per_site": head, "fp16_max": 65504.0})
    assert max(head.values()) < 65504.0 / 16
    with torch.no_grad():
        y2 = m(image)
    assert torch.equal(y1, y2)                                               # two fp16 forwards: bit-identical
    big = torch.cat([image.cpu(), synth.synth_batch(248, seed=32)[0]])          # rows 0..7 are the B = 8 batch
    with torch.no_grad():
        yb = m(big.cuda())
    torch.cuda.synchronize()
    assert torch.equal(yb[:8], y1)                                           # B = 256 rows 0..7 == the B = 8 forward, bit for bit
    y_bf = _eval_forward(m, image, "bf16")
    fresh, _, _, _, _, _ = _case("vit_L12")
    _load(fresh, prefix, seed)
    fresh.to("cuda").eval()
    assert torch.equal(y_bf, _eval_forward(fresh, image, "bf16"))           # bf16 -> fp16 -> bf16 == a fresh bf16 model
    assert not torch.equal(y_bf, y1)


def test_fp16_refuses_training_and_incompatible_modes(monkeypatch):
    from bioscanclip.hip import engine
    m, prefix, seed, x, _, _ = _case("dna_L2")
    _load(m, prefix, seed)
    m.to("cuda")
    engine.set_operand_format(m, "fp16")
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"eval\(\).*no_grad"):
        m(x)
    m.eval()
    with pytest.raises(RuntimeError, match="fp16 backward is not built"):   # autograd would record the forward
        m(x)
    with torch.no_grad():
        m(x)                                                                   # eval + no_grad: fine
    engine.set_precision(m, "fp8")
    with torch.no_grad(), pytest.raises(ValueError, match="fp8"):
        m(x)
    engine.set_precision(m, "bf16")
    m.hip_full_ft = True
    with torch.no_grad(), pytest.raises(ValueError, match="full fine-tuning"):
        m(x)
    m.hip_full_ft = False
    for attr, val in (("EXACT_FORWARD", True), ("RESID_STREAM_BF16", False)):
        monkeypatch.setattr(engine, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="BSCLIP_PARITY"):
            m(x)
        monkeypatch.undo()
    with torch.no_grad():
        assert torch.isfinite(m(x)).all()
    # the text tower is switched too
    t, tp, ts, tx, _, _ = _case("txt_L4")
    _load(t, tp, ts)
    holder = torch.nn.ModuleDict({"language_encoder": t.to("cuda").eval()})
    engine.set_operand_format(holder, "fp16")
    assert t.hip_operands == "fp16"
    with torch.no_grad():
        t(tx)
    assert t._engine.fp16


# ------------------------------------------------------------------------------------------------------------- end to end
sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))


class _EvalLoader:
    """test_55's evaluation batches: 7-tuples with a dict of taxonomy-name lists."""

    def __init__(self, n_batches, B, seed):
        self.batches = []
        for s in range(n_batches):
            image, dna, text, _ = synth.synth_batch(B, seed=seed + s, with_text=True)
            lab = {lv: [f"{lv[0]}{(s * B + i) % m}" for i in range(B)] for lv, m in
                   zip(["order", "family", "genus", "species"], [2, 3, 5, 7])}
            self.batches.append(([f"P{s}_{i}" for i in range(B)], image, dna, text["input_ids"], text["token_type_ids"],
                                 text["attention_mask"], lab))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_get_features_fp16_matches_oracle():
    from bioscanclip.hip.engine import set_operand_format
    from bioscanclip.model import arch
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from bioscanclip.model.language_encoder import LoRA_bert
    from bioscanclip.model.simple_clip import SimpleCLIP
    import inference_and_eval as host
    model = SimpleCLIP(LoRA_ViT_timm(arch.VisionTransformerParams(depth=2), r=4, num_classes=768),
                       LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=2)), r=4,
                                         num_classes=768),
                       LoRA_bert(arch.BertModelParams(arch.bert_small_config()), r=4, num_classes=768))
    sd = synth.synth_state_dict(synth.shapes_of(model), 41)
    model.load_state_dict(sd)
    model.to("cuda")
    set_operand_format(model, "fp16")
    loader = _EvalLoader(2, 3, seed=50)
    split = host.get_features_and_label(loader, model, "cuda", for_key_set=True)
    assert all(getattr(model, e)._engine.fp16 for e in ("image_encoder", "dna_encoder", "language_encoder"))
    image = torch.cat([b[1] for b in loader.batches])
    dna = torch.cat([b[2] for b in loader.batches])
    text = {k: torch.cat([b[i] for b in loader.batches]) for k, i in
            [("input_ids", 3), ("token_type_ids", 4), ("attention_mask", 5)]}
    with torch.no_grad():
        ref = {"encoded_image_feature": (refcpu.l2_normalize(refcpu.vit_encoder(sd, image)), CAP["vit_L2"]),
               "encoded_dna_feature": (refcpu.l2_normalize(refcpu.barcode_bert_encoder(sd, dna)), CAP["dna_L2"]),
               "encoded_language_feature": (refcpu.l2_normalize(refcpu.bert_text_encoder(sd, text)), CAP["txt_L4"])}
    errs = {}
    for key, (r, cap) in ref.items():
        got = split[key]
        assert got.dtype == np.float64 and got.shape == (6, 768)
        errs[key] = float(np.linalg.norm(got - r.numpy()) / np.linalg.norm(r.numpy()))
        assert errs[key] <= cap, (key, errs[key])
    _log({"test": "fp16_get_features_I+D+T_L2", **errs})


def test_inference_and_eval_fp16_and_the_feature_cache(tmp_path, capsys):
    import inference_and_eval
    common = ["model_config=lora_vit_lora_barcode_bert_ssl", "model_config.load_ckpt=false", f"project_root_path={tmp_path}",
              "debug_flag=false", "synthetic_eval_batches=1"]
    acc, _, _ = inference_and_eval.main(common + ["hip_operands=fp16"])
    out = capsys.readouterr().out
    assert "Initialize model" in out and "micro_acc top-1" in out
    assert acc["encoded_image_feature"]["encoded_dna_feature"]["seen"]["micro_acc"][1]
    inference_and_eval.main(common + ["save_inference=true"])                     # a bf16 cache
    capsys.readouterr()
    inference_and_eval.main(common + ["hip_operands=fp16", "load_inference=true"])
    out = capsys.readouterr().out
    assert "extracting again" in out and "Initialize model" in out                # not reused by an fp16 run
    inference_and_eval.main(common + ["load_inference=true"])
    assert "Initialize model" not in capsys.readouterr().out                      # reused by a bf16 run
    with pytest.raises(ValueError, match="hip_operands"):
        inference_and_eval.main(common + ["hip_operands=fp8"])
