"""CPU checks of the fp16-operand backward of the LoRA ViT (training on fp16 operands): the gfx950 code object holds fp16 forms of the
attention backward (plain and LoRA partial-sum) that multiply on the fp16 matrix-core instruction only, the fp16 LayerNorm backward and
LoRA-gradient forms never convert with the round-toward-zero instruction, the bf16 backward forms still multiply and convert in bf16
only, every new flag carrier validates it on the host and is documented in the header, and the public switches refuse what is not
built (unknown tower names, fp16 training of the BERT towers)."""
import ctypes
import os
import re

import pytest

from test_07_fp16_forward_cpu import _lib, _mfmas, _select, kernels  # noqa: F401  (test_06's code-object reader, through test_07)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# template argument lists: attn_bwd_kernel's eighth parameter F16, layernorm_bwd_kernel's fourth, lora_grad_da_kernel's fourth
FP16_ATTN_BWD = r"attn_bwd_kernel<7, false, false, 32, false, (true|false), (true|false), true>"
BF16_ATTN_BWD = r"attn_bwd_kernel<\d+, (true|false), (true|false), \d+, (true|false), (true|false), (true|false)(, false)?>"
FP16_OTHER = {
    "layernorm backward": r"layernorm_bwd_kernel<768, true, (true|false), true>",
    "lora dA": r"lora_grad_da_kernel<768, false, false, true>",
    "scaled cast": r"cast_f32_f16_scaled_kernel",
}


def test_fp16_attention_backward_runs_on_fp16_matrix_cores(kernels):
    sel = _select(kernels, FP16_ATTN_BWD)
    lora = [k for k in sel if re.search(r"true, true, true>", k)]
    assert len(sel) == 3 and len(lora) == 1, sorted(sel)    # preloaded delta with / without the LoRA partials, the plain form
    for name, asm in sel.items():
        assert _mfmas(asm) == {"v_mfma_f32_32x32x16_f16"}, (name, _mfmas(asm))
        assert "v_cvt_pk_bf16_f32" not in asm, f"{name}: bf16 conversion in an fp16 kernel"
        assert "v_cvt_pkrtz_f16_f32" not in asm, f"{name}: round-toward-zero conversion"
        assert re.search(r"v_cvt_(pk_)?f16_f32", asm), name


@pytest.mark.parametrize("family", sorted(FP16_OTHER))
def test_fp16_backward_kernels_round_to_nearest(kernels, family):
    sel = _select(kernels, FP16_OTHER[family])
    assert sel, f"no fp16 {family} kernel in the library"
    for name, asm in sel.items():
        assert "v_cvt_pkrtz_f16_f32" not in asm, f"{name}: round-toward-zero conversion"
        assert "v_cvt_pk_bf16_f32" not in asm, f"{name}: bf16 conversion in an fp16 kernel"


def test_bf16_backward_kernels_unchanged(kernels):
    """The bf16 attention backward, LayerNorm backward and LoRA dA instantiations multiply and convert in bf16 only."""
    att = _select(kernels, BF16_ATTN_BWD)
    ln = _select(kernels, r"layernorm_bwd_kernel<\d+, (true|false), (true|false)(, false)?>")
    da = _select(kernels, r"lora_grad_da_kernel<\d+, (true|false), (true|false)(, false)?>")
    assert len(att) >= 40 and len(ln) == 8 and len(da) >= 5, (len(att), len(ln), len(da))
    for name, asm in att.items():
        assert _mfmas(asm) == {"v_mfma_f32_32x32x16_bf16"}, name
        assert not re.search(r"v_cvt_(pk_|pkrtz_)?f16_f32", asm), name
    for name, asm in {**ln, **da}.items():
        assert not re.search(r"v_cvt_(pk_|pkrtz_)?f16_f32", asm), name


def test_attention_backward_flag_validation():
    lib, h = _lib()
    F = lib.OPERANDS_FP16
    one = ctypes.c_void_p(16)
    bwd = lambda q_rows, kb=None, p=0.0, S=197: h.bsclip_attn_bwd(one, 3 * 768, one, 768, one, 2, S, 12, None, ctypes.c_float(0.125),
                                                                  one, 3 * 768, q_rows, kb, ctypes.c_float(p), 1, None)
    lora = lambda q_rows, kb=None, p=0.0: h.bsclip_attn_bwd_lora(one, 3 * 768, one, 768, one, 2, 197, 12, None, ctypes.c_float(0.125),
                                                                 one, 3 * 768, q_rows, kb, one, 64, one, one, one, ctypes.c_float(p), 1,
                                                                 None)
    for call in (bwd, lora):
        for bad in (0x200 | F, 0x200, F | 0x1000, -1):
            assert call(bad) == -1, hex(bad)
            assert "unknown bits" in lib.last_error()
        assert call(F, p=0.1) == -1 and "fp16" in lib.last_error() and "dropout" in lib.last_error()
        assert call(F | 1, kb=one) == -1 and "keep_bits" in lib.last_error()
    assert bwd(F, S=133) == -1 and "S = 197" in lib.last_error()
    assert bwd(F | 198) == -1 and "q_rows" in lib.last_error()


def test_layernorm_backward_flag_validation():
    lib, h = _lib()
    F = lib.OPERANDS_FP16
    one = ctypes.c_void_p(16)
    ln = lambda flag, p=0.0, ip=0.0, rf=1, H=768: h.bsclip_layernorm_bwd(one, H, flag, one, one, 4, H, one, H, one, H, None, None, 0,
                                                                         None, 0, one, H, ctypes.c_float(p), 1, ctypes.c_float(ip), 1, rf,
                                                                         None)
    for bad in (1 | F | 0x200, 0x400, F | 0x800):
        assert ln(bad) == -1, hex(bad)
        assert "unknown bits" in lib.last_error()
    assert ln(1 | F, p=0.1) == -1 and "dropout" in lib.last_error()
    assert ln(1 | F, ip=0.1) == -1 and "dropout" in lib.last_error()
    for rf in (0, 1 | 4, 1 | 8, 1 | 16):   # g_resid not 16-bit, f32 g_gemm, f32 / split operand output
        assert ln(1 | F, rf=rf) == -1 and "fp16" in lib.last_error(), rf
    assert ln(0 | F) == -1 and "fp16" in lib.last_error()       # an f32 x
    assert ln(1 | F, H=512) == -1 and "fp16" in lib.last_error()


def test_lora_grad_and_scale_entry_points_validation():
    lib, h = _lib()
    F = lib.OPERANDS_FP16
    one = ctypes.c_void_p(16)
    heads16 = lambda ops_, H=768: h.bsclip_lora_grad_heads_f16(one, 832, 394, H, 2, one, one, one, one, one, one, one, ops_, None)
    for bad in (F | 0x200, 0x400):
        assert heads16(bad) == -1 and "unknown bits" in lib.last_error(), hex(bad)
    assert heads16(13) == -1 and "BSCLIP_OPERANDS_FP16" in lib.last_error()      # the flag is required
    assert heads16(F | 65) == -1 and "s <= 64" in lib.last_error()
    assert heads16(F | 13, H=512) == -1 and "768" in lib.last_error()
    assert h.bsclip_cast_f32_f16_scaled(one, 4, 65, one, None) == -1 and "scale_log2" in lib.last_error()
    assert h.bsclip_cast_f32_f16_scaled(ctypes.c_void_p(20), 4, 13, one, None) == -1 and "aligned" in lib.last_error()
    assert h.bsclip_add_scaled_f32(one, 4, -65, one, None) == -1 and "scale_log2" in lib.last_error()
    assert h.bsclip_add_scaled_f32(one, 0, -13, one, None) == -1


def test_header_documents_each_backward_carrier():
    hdr = open(os.path.join(ROOT, "include", "bsclip.h")).read()
    block = hdr[hdr.index("#define BSCLIP_OPERANDS_FP16"):hdr.index("typedef struct bsclip_epi_args")]
    for fn, arg in [("bsclip_attn_bwd", "q_rows"), ("bsclip_attn_bwd_lora", "q_rows"), ("bsclip_layernorm_bwd", "x_bf16"),
                    ("bsclip_lora_grad_heads_f16", "operands")]:
        assert re.search(fn + r"\s+" + arg + r"\b", block), fn
    for fn in ("bsclip_cast_f32_f16_scaled", "bsclip_add_scaled_f32"):
        assert fn in block, fn
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "towers" in doc[doc.index("set_operand_format"):]


def test_set_operand_format_towers():
    import torch
    from bioscanclip.hip import engine
    img, dna, txt = torch.nn.Module(), torch.nn.Module(), torch.nn.Module()
    img.lora_vit, dna.lora_barcode_bert, txt.lora_bert = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    model = torch.nn.ModuleDict({"image_encoder": img, "dna_encoder": dna, "language_encoder": txt})
    for bad in (("images",), ("image", "text"), (), "vision"):
        with pytest.raises(ValueError, match="towers"):
            engine.set_operand_format(model, "fp16", towers=bad)
    assert not any(engine.wants_fp16(m) for m in (img, dna, txt))
    engine.set_operand_format(model, "fp16", towers=("image",))
    assert engine.wants_fp16(img) and not engine.wants_fp16(dna) and not engine.wants_fp16(txt)
    engine.set_operand_format(model, "fp16", towers=["dna", "language"])
    assert all(engine.wants_fp16(m) for m in (img, dna, txt))
    engine.set_operand_format(model, "bf16")
    assert not any(engine.wants_fp16(m) for m in (img, dna, txt))


def test_vit_accepts_fp16_training_and_berts_refuse_it():
    """The fp16 check lets the LoRA ViT train (it still refuses fp8, full fine-tuning, the f32 streams); the BERT towers keep
    refusing training with their message."""
    import torch
    from bioscanclip.hip import engine
    vit, bert = torch.nn.Module(), torch.nn.Module()
    vit.lora_vit, bert.lora_barcode_bert = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    for m in (vit, bert):
        m.hip_operands = "fp16"
        m.train()
    engine._check_fp16(vit)
    with pytest.raises(RuntimeError, match="fp16 backward is not built"):
        engine._check_fp16(bert)
    vit.hip_precision = "fp8"
    with pytest.raises(ValueError, match="fp8"):
        engine._check_fp16(vit)
    vit.hip_precision = "bf16"
    vit.hip_full_ft = True
    with pytest.raises(ValueError, match="full fine-tuning"):
        engine._check_fp16(vit)
    vit.hip_full_ft = False
    for attr, val, msg in (("EXACT_FORWARD", True, "BSCLIP_PARITY"), ("RESID_STREAM_BF16", False, "BSCLIP_PARITY"),
                           ("GRAD_STREAM_BF16", False, "BSCLIP_GRAD_STREAM")):
        prev = getattr(engine, attr)
        setattr(engine, attr, val)
        try:
            with pytest.raises(ValueError, match=msg):
                engine._check_fp16(vit)
        finally:
            setattr(engine, attr, prev)


@pytest.mark.parametrize("towers", ["dna", "image,language", "language"])
def test_train_cl_refuses_fp16_towers_without_a_backward(towers):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
    import train_cl
    with pytest.raises(ValueError, match="fp16 backward"):
        train_cl.main(["model_config=lora_vit_lora_barcode_bert_ssl", f"hip_fp16_towers={towers}"])
    with pytest.raises(ValueError, match="unknown tower"):
        train_cl.main(["model_config=lora_vit_lora_barcode_bert_ssl", "hip_fp16_towers=vision"])
