"""CPU checks of the fp16-operand forward (the 16-bit kernels other than the GEMMs, BSCLIP_OPERANDS_FP16 on their entry points):
the gfx950 code object holds fp16 forms of the attention forward on the fp16 matrix-core instruction, no fp16 kernel converts with
the round-toward-zero packed instruction, the bf16 forms still convert and multiply in bf16 only, every entry point that carries the
flag validates it on the host, and the public switch refuses unknown formats."""
import ctypes
import os
import re
import subprocess

import pytest

from test_06_fp16_cpu import LLVM_BIN, _gfx950_code_objects  # noqa: E402  (test_06's reader of the gfx950 code objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """demangled kernel name -> its disassembly, over every gfx950 code object of the product library."""
    from bioscanclip.hip import lib
    d = tmp_path_factory.mktemp("isa")
    funcs = {}
    for i, elf in enumerate(_gfx950_code_objects(lib.LIB_PATH, d)):
        path = d / f"co{i}.elf"
        path.write_bytes(elf)
        text = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "-C", str(path)], check=True, capture_output=True,
                              text=True).stdout
        for blk in re.split(r"\n(?=[0-9a-f]{16} <)", text):
            head = blk.split("\n", 1)[0]
            m = re.match(r"[0-9a-f]{16} <(?:void )?(.*)>:$", head)
            if m:
                funcs[m.group(1)] = blk
    assert funcs, "no gfx950 code found in the library"
    return funcs


def _select(kernels, pattern):
    return {k: v for k, v in kernels.items() if re.search(pattern, k)}


def _mfmas(asm):
    return set(re.findall(r"v_mfma\w*", asm))


# the fp16 forms added for the forward: template argument F16 = true (the attention forward's sixth, LayerNorm's fifth parameter)
FP16_ATTN = r"attn_fwd_kernel<\d+, false, \d+, false, false, true>"
FP16_FORWARD = {
    "attention": FP16_ATTN,
    "layernorm": r"layernorm_fwd_kernel<\d+, (true|false), (true|false), false, true>",
    "im2col": r"im2col_patch16_kernel<(true|false), true>",
    "cls rows": r"vit_cls_rows_kernel<true, true>",
    "cast": r"cast_f32_bf16_kernel<true>",
    "lora-b columns": r"waug_set_lora_layers_kernel<true>",
}


def test_fp16_attention_forward_runs_on_fp16_matrix_cores(kernels):
    sel = _select(kernels, FP16_ATTN)
    # the towers' eval-mode launches: S = 197 and 133 (last tile of 5 rows) and every other tile count (text lengths)
    nbs = {int(re.search(r"attn_fwd_kernel<(\d+), false, (\d+)", k).group(1)) for k in sel}
    tails = {int(re.search(r"attn_fwd_kernel<\d+, false, (\d+)", k).group(1)) for k in sel}
    assert nbs == set(range(1, 8)) and tails == {5, 32}, sorted(sel)
    for name, asm in sel.items():
        assert "v_mfma_f32_32x32x16_f16" in _mfmas(asm), name
        assert not any(m.endswith("bf16") for m in _mfmas(asm)), f"{name}: bf16 MFMA in an fp16 kernel"
        assert "v_cvt_pk_bf16_f32" not in asm, f"{name}: bf16 conversion in an fp16 kernel"
        assert re.search(r"v_cvt_(pk_)?f16_f32", asm), name


@pytest.mark.parametrize("family", sorted(FP16_FORWARD))
def test_fp16_forward_kernels_round_to_nearest(kernels, family):
    sel = _select(kernels, FP16_FORWARD[family])
    assert sel, f"no fp16 {family} kernel in the library"
    for name, asm in sel.items():
        assert "v_cvt_pkrtz_f16_f32" not in asm, f"{name}: round-toward-zero conversion"
        assert "v_cvt_pk_bf16_f32" not in asm, f"{name}: bf16 conversion in an fp16 kernel"


def test_bf16_forward_kernels_unchanged(kernels):
    """The bf16 attention forward and LayerNorm forward instantiations multiply and convert in bf16 only."""
    att = _select(kernels, r"attn_fwd_kernel<\d+, (true|false), \d+, (true|false), (true|false)(, false)?>")
    ln = _select(kernels, r"layernorm_fwd_kernel<\d+, (true|false), (true|false), (true|false)(, false)?>")
    assert len(att) >= 27 and len(ln) >= 16
    for name, asm in att.items():
        assert _mfmas(asm) == {"v_mfma_f32_32x32x16_bf16"}, name
        assert not re.search(r"v_cvt_(pk_|pkrtz_)?f16_f32", asm), name
    for name, asm in ln.items():
        assert not re.search(r"v_cvt_(pk_|pkrtz_)?f16_f32", asm), name


def _lib():
    from bioscanclip.hip import lib
    return lib, lib.load()


def test_attention_forward_flag_validation():
    lib, h = _lib()
    F = lib.OPERANDS_FP16
    one = ctypes.c_void_p(16)
    call = lambda q_rows, kb=None, p=0.0: h.bsclip_attn_fwd(one, 3 * 768, 2, 197, 12, None, ctypes.c_float(0.125), one, 768, one,
                                                           q_rows, kb, ctypes.c_float(p), 1, None)
    for bad in (0x200 | F, 0x200, F | 0x1000, -1):
        assert call(bad) == -1, hex(bad)
        assert "unknown bits" in lib.last_error()
    assert call(F, p=0.1) == -1 and "fp16" in lib.last_error() and "dropout" in lib.last_error()
    assert call(F | 1, kb=one) == -1 and "keep_bits" in lib.last_error()
    assert call(F | 198) == -1 and "q_rows" in lib.last_error()       # the low byte is still checked against S


def test_layernorm_forward_flag_validation():
    lib, h = _lib()
    F = lib.OPERANDS_FP16
    one = ctypes.c_void_p(16)
    ln = lambda flag, y3=None, p=0.0: h.bsclip_layernorm_fwd(one, 768, flag, 4, 768, one, one, ctypes.c_float(1e-6), one, 832, None,
                                                             y3, 2304 if y3 else 0, None, None, ctypes.c_float(p), 1, None)
    for bad in (1 | F | 0x200, 0x400, F | 0x800):
        assert ln(bad) == -1, hex(bad)
        assert "unknown bits" in lib.last_error()
    assert ln(1 | F, y3=one) == -1 and "y_split3" in lib.last_error()
    assert ln(0 | F, p=0.1) == -1 and "dropout" in lib.last_error()
    assert h.bsclip_layernorm_fwd_fp8(one, 768, 1 | F, 4, 768, one, one, ctypes.c_float(1e-6), one, 768, None, 0, None, None, None,
                                      ctypes.c_float(0.0), 1, None) == -1
    assert "fp8" in lib.last_error()


def test_embedding_entry_points_flag_validation():
    lib, h = _lib()
    F = lib.OPERANDS_FP16
    one = ctypes.c_void_p(16)
    for bad in (1 | F | 0x200, 0x200):
        assert h.bsclip_im2col_patch16(one, 2, one, 2304, bad, None) == -1 and "unknown bits" in lib.last_error()
        assert h.bsclip_vit_cls_rows(one, bad, one, one, 2, 197, 768, None) == -1 and "unknown bits" in lib.last_error()
        assert h.bsclip_waug_set_lora_layers(one, 2 | bad, 832, 768, None) == -1 and "unknown bits" in lib.last_error()
    assert h.bsclip_im2col_patch16(one, 2, one, 768, 1 | F, None) == -1 and "ld_cols" in lib.last_error()   # split needs 2304
    assert h.bsclip_vit_cls_rows(one, F, one, one, 2, 197, 768, None) == -1 and "16-bit stream" in lib.last_error()
    assert h.bsclip_waug_set_lora_layers(one, F, 832, 768, None) == -1 and "bad args" in lib.last_error()      # zero layers
    assert h.bsclip_cast_f32_f16(None, 4, one, None) == -1 and "bsclip_cast_f32_f16" in lib.last_error()
    counter = ctypes.c_void_p(16)
    assert h.bsclip_count_nonfinite(one, 4, F, counter, None) == -1       # the flag qualifies a 16-bit tensor only


def test_header_documents_the_flag_on_each_entry_point():
    hdr = open(os.path.join(ROOT, "include", "bsclip.h")).read()
    block = hdr[hdr.index("#define BSCLIP_OPERANDS_FP16"):hdr.index("typedef struct bsclip_epi_args")]
    for fn, arg in [("bsclip_attn_fwd", "q_rows"), ("bsclip_layernorm_fwd", "x_bf16"), ("bsclip_im2col_patch16", "split"),
                    ("bsclip_vit_cls_rows", "x_bf16"), ("bsclip_waug_set_lora_layers", "layers"), ("bsclip_count_nonfinite", "is_bf16")]:
        assert re.search(fn + r"\s+" + arg + r"\b", block), fn
    assert "bsclip_cast_f32_f16" in block
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "bsclip_cast_f32_f16" in doc and "set_operand_format" in doc


def test_set_operand_format_rejects_unknown_formats():
    import torch
    from bioscanclip.hip import engine
    m = torch.nn.Module()
    m.lora_vit = torch.nn.Linear(2, 2)
    for bad in ("fp8", "FP16", "f16", "", None, 16):
        with pytest.raises(ValueError, match="operand format"):
            engine.set_operand_format(m, bad)
    assert getattr(m, "hip_operands", "bf16") == "bf16"
    engine.set_operand_format(m, "fp16")
    assert m.hip_operands == "fp16" and m._engine is None and engine.wants_fp16(m)
    engine.set_operand_format(m, "bf16")
    assert not engine.wants_fp16(m)


def test_ops_wrappers_refuse_mixed_16_bit_formats():
    import torch
    from bioscanclip.hip import ops
    with pytest.raises(ValueError, match="must all be bf16 or all fp16"):
        ops._h16(torch.zeros(2, 768, dtype=torch.float16), torch.zeros(2, 832, dtype=torch.bfloat16), who="layernorm_fwd")
    assert ops._h16(torch.zeros(1, dtype=torch.float16), None, torch.zeros(1), who="x") == torch.float16
    assert ops._h16(torch.zeros(1), who="x") == torch.bfloat16
