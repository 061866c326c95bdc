"""CPU checks of the fp16-operand GEMMs (bsclip_gemm_bf16 | BSCLIP_OPERANDS_FP16): the gfx950 code object of libbsclip_hip.so holds
fp16 forms of the GEMM kernels that run on the fp16 matrix-core instruction and never convert with the round-toward-zero packed
instruction, and the entry point validates the flag on the host."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _gfx950_code_objects(so_path, tmp):
    """The gfx950 ELF images of every offload bundle in the library's .hip_fatbin section (one bundle per translation unit)."""
    sec, stripped = tmp / "fatbin.bin", tmp / "lib_copy.so"
    subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), f"--dump-section=.hip_fatbin={sec}", so_path, str(stripped)], check=True,
                   capture_output=True)
    fat = sec.read_bytes()
    out = []
    for m in re.finditer(re.escape(BUNDLE_MAGIC), fat):
        o = m.start()
        (count,) = struct.unpack_from("<Q", fat, o + 24)
        p = o + 32
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", fat, p)
            p += 24
            triple = fat[p:p + tlen].decode()
            p += tlen
            if "gfx950" in triple:
                out.append(fat[o + off:o + off + size])
    return out


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


# template argument lists of the fp16 forms: ping-pong OP 3, generic and persistent kernels' trailing F16 = true
FP16_GEMMS = {
    "ping-pong": r"gemm_nt_pp_kernel<\d+, (true|false), false, 0, 0, 3>",
    "generic": r"gemm_nt_kernel<\d+, \d+, \d+, \d+, \d+, (true|false), true>",
    "persistent": r"gemm_nt_pers_kernel<\d+, (true|false), false, (true|false), true>",
}


@pytest.mark.parametrize("family", sorted(FP16_GEMMS))
def test_fp16_gemm_kernels_use_fp16_matrix_cores_and_round_to_nearest(kernels, family):
    sel = _select(kernels, FP16_GEMMS[family])
    assert sel, f"no fp16 {family} GEMM kernel in the library"
    for name, asm in sel.items():
        assert re.search(r"v_mfma_f32_(16x16x32|32x32x16)_f16\b", asm), name
        assert "_bf16" not in " ".join(re.findall(r"v_mfma\w*", asm)), f"{name}: bf16 MFMA in an fp16 kernel"
        assert "v_cvt_pkrtz_f16_f32" not in asm, f"{name}: round-toward-zero conversion"
    # the 16-bit-output epilogues of the fp16 kernels convert to fp16 (RNE conversions), not to bf16
    outs = _select(kernels, r"gemm_nt_pp_kernel<(0|2|4|7|8), (true|false), false, 0, 0, 3>")
    assert len(outs) >= 5
    for name, asm in outs.items():
        assert re.search(r"v_cvt_(pk_)?f16_f32", asm), name
        assert "v_cvt_pk_bf16_f32" not in asm, name


def test_bf16_gemm_kernels_unchanged(kernels):
    sel = _select(kernels, r"gemm_nt_pp_kernel<\d+, (true|false), false, 0, 0, 0>")
    assert sel
    for name, asm in sel.items():
        assert re.search(r"v_mfma_f32_16x16x32_bf16\b", asm), name
        assert not re.search(r"v_mfma_f32_\w+_f16\b", asm), name


def test_fp16_flag_validation_without_gpu():
    """The flag is checked with the rest of the arguments on the host, before any launch: nulls, 16-byte alignment, shapes,
    unknown epilogues under the flag and unknown flag bits are refused."""
    from bioscanclip.hip import lib
    h = lib.load()
    F = lib.OPERANDS_FP16
    one = ctypes.c_void_p(16)
    a = lib.EpiArgs()
    assert h.bsclip_gemm_bf16(None, 64, one, 64, one, 128, 1, 128, 64, lib.EPI_BF16 | F, ctypes.byref(a), None) == -1
    assert "null operand" in lib.last_error()
    assert h.bsclip_gemm_bf16(ctypes.c_void_p(24), 64, one, 64, one, 128, 1, 128, 64, lib.EPI_BF16 | F, ctypes.byref(a), None) == -1
    assert "16-B alignment" in lib.last_error()
    assert h.bsclip_gemm_bf16(one, 64, one, 64, one, 128, 1, 128, 48, lib.EPI_F32 | F, ctypes.byref(a), None) == -1
    assert "multiple of 64" in lib.last_error()
    for bad in (lib.EPI_GELU_FP8 | F, 9 | F, lib.EPI_BF16 | 0x200, lib.EPI_BF16 | F | 0x200):
        assert h.bsclip_gemm_bf16(one, 64, one, 64, one, 128, 1, 128, 64, bad, ctypes.byref(a), None) == -1, hex(bad)
        assert "unknown epilogue" in lib.last_error()
    a.struct_size = 48
    assert h.bsclip_gemm_bf16(one, 64, one, 64, one, 128, 1, 128, 64, lib.EPI_BF16 | F, ctypes.byref(a), None) == -1
    assert "struct_size" in lib.last_error()
    a = lib.EpiArgs()
    a.dropout_p = 0.1
    assert h.bsclip_gemm_bf16(one, 64, one, 64, one, 128, 1, 128, 64, lib.EPI_BF16 | F, ctypes.byref(a), None) == -1
    assert "dropout" in lib.last_error()
    a = lib.EpiArgs()
    assert h.bsclip_gemm_bf16(one, 64, one, 64, one, 128, 1, 128, 64, lib.EPI_RESID_BF16 | F, ctypes.byref(a), None) == -1
    assert "RESID_BF16 needs resid" in lib.last_error()


def test_header_documents_the_flag():
    hdr = open(os.path.join(ROOT, "include", "bsclip.h")).read()
    m = re.search(r"#define BSCLIP_OPERANDS_FP16 (0x[0-9a-f]+)", hdr)
    from bioscanclip.hip import lib
    assert m and int(m.group(1), 16) == lib.OPERANDS_FP16
    assert lib.OPERANDS_FP16 > max(lib.EPI_BF16, lib.EPI_F32, lib.EPI_GELU_BF16, lib.EPI_RESID_F32, lib.EPI_DGELU_BF16, lib.EPI_PATCH_F32,
                                   lib.EPI_GELU_FP8, lib.EPI_RESID_BF16, lib.EPI_PATCH_BF16)
    assert "BSCLIP_OPERANDS_FP16" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
