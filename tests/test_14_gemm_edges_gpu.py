"""bsclip_gemm_bf16 / bsclip_gemm_splitk_f32 on operands whose product is exact (tests/gemm_exact.py), element by element against
f64 arithmetic: every row count around the MFMA block and the 128- / 256-row tiles, the N % 256 != 0 fallback of the 256-wide
tiles, the smallest output leading dimensions the entry points admit, the persistent kernel's tile walk, split-K on partial panels.

Linear epilogues (F32, BF16, RESID_F32, RESID_BF16, PATCH_*, split-K) are held to BIT EQUALITY with f64 -- f32 outputs equal it,
16-bit outputs are one round-to-nearest-even of it -- because no sum of these operands rounds in an f32 accumulator in any order
(tests/test_04_gemm_exact_cpu.py proves that, and that one dropped or doubled 8-element K chunk, a swapped row pair, a store 8
columns off, or -- in bf16 -- a truncating conversion changes an element; rows are distinct, values non-degenerate).  The two
non-linear epilogues are held to bars built from the output format's rounding and the kernel's documented table / decode error
(gemm_exact.gelu_bar, GELU_PRIME_BAR, dgelu_bar); a truncating fp16 conversion, which the exact fp16 sums cannot show, breaks the
DGELU bar at a quarter of the elements.  The CPU test shows the kernels' arithmetic restated in f32 inside each bar with room.
Every output lives in a sentinel-filled buffer with 3 spare rows and pad columns, all of which must still hold the sentinel.
Every toleranced figure is printed as a ``FIGURES {json}`` line before it is asserted (``pytest -s`` shows them)."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_exact as gx  # noqa: E402

DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
NAN = float("nan")
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    o.init_tables()
    return o


def _log(test, **figures):
    print("FIGURES " + json.dumps({"test": test, **figures}))


def _case(M, N, K, dtype):
    """The cached case on the GPU, with A as the [:, :K] view of a NaN-padded K + 16 wide buffer."""
    c = gx.ref64(M, N, K, gx.SEED, dtype, DEV)
    if not hasattr(c, "a_ld"):
        buf = torch.full((M, K + 16), NAN, dtype=dtype, device=DEV)
        buf[:, :K] = c.a
        c.a_ld = buf[:, :K]
    return c


EPILOGUES = ("f32", "resid32", "resid32_inplace", "h16", "h16_nobias", "resid16", "dgelu", "gelu")
PERS_EPILOGUES = ("f32", "h16", "gelu", "resid32", "dgelu", "resid16")      # the six the persistent kernel is instantiated for


def _run(ops, c, extra, which):
    """Each epilogue of ``which`` into sentinel-filled buffers with ldc = N + 4 + extra, ld_aux = N + 16 + extra,
    ld_resid = N + 4 + extra: the smallest bsclip_gemm_bf16's own checks accept when extra = 0 (ldc % 4, ld_aux % 16; the f32
    residual's 16-byte row pieces and the 16-bit residual's ld_resid % 4).  Returns {name: buffer} (+ name_aux)."""
    from bioscanclip.hip.lib import (EPI_BF16, EPI_DGELU_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_BF16, EPI_RESID_F32)
    M, N, h = c.M, c.N, c.dtype
    ldc, ld_aux, ld_res = N + 4 + extra, N + 16 + extra, N + 4 + extra
    a, b = c.a_ld, c.b
    outs = {}
    for name in which:
        buf, view = gx.strided(M, N, ldc, torch.float32 if name in ("f32", "resid32", "resid32_inplace") else h, device=DEV)
        if name == "f32":
            ops.gemm(a, b, view, EPI_F32, bias=c.bias, M=M)
        elif name == "resid32":
            _, r = gx.strided(M, N, ld_res, torch.float32, device=DEV)
            r[:M] = c.resid
            ops.gemm(a, b, view, EPI_RESID_F32, bias=c.bias, resid=r, M=M)
        elif name == "resid32_inplace":                       # C aliases resid, no bias: the loss gradient's accumulation
            view[:M] = c.resid
            ops.gemm(a, b, view, EPI_RESID_F32, resid=view, M=M)
        elif name == "h16":
            ops.gemm(a, b, view, EPI_BF16, bias=c.bias, M=M)
        elif name == "h16_nobias":
            ops.gemm(a, b, view, EPI_BF16, M=M)
        elif name == "resid16":
            _, r = gx.strided(M, N, ld_res, h, device=DEV)
            r[:M] = c.resid.to(h)
            ops.gemm(a, b, view, EPI_RESID_BF16, bias=c.bias, resid=r, M=M)
        elif name == "dgelu":
            abuf, aux = gx.strided(M, N, ld_aux, torch.uint8, device=DEV)
            aux[:M] = c.codes
            ops.gemm(a, b, view, EPI_DGELU_BF16, aux=aux, M=M)
            outs["dgelu_aux"] = abuf
        elif name == "gelu":
            abuf, aux = gx.strided(M, N, ld_aux, torch.uint8, device=DEV)
            ops.gemm(a, b, view, EPI_GELU_BF16, bias=c.bias, aux=aux, M=M)
            outs["gelu_aux"] = abuf
        outs[name] = buf
    return outs


EXACT = {"f32": "bias", "resid32": "bias_resid", "resid32_inplace": "resid", "h16": "bias", "h16_nobias": "acc", "resid16": "bias_resid"}


def _verify(c, outs, tag, worst):
    """Exact epilogues: asserted here.  Toleranced ones: err / bar goes into ``worst`` (with where it was seen); the caller prints
    the figures and then asserts them <= 1.  A NaN (an element never written) makes a ratio NaN, which fails that assertion."""
    M, N, h = c.M, c.N, c.dtype
    for name, buf in outs.items():
        assert gx.untouched(buf, M, N), f"{tag} {name}: an element outside [:M, :N] was written (spare rows / pad columns)"
        got = buf[:M, :N]
        if name in EXACT:
            want = c(EXACT[name]).float() if buf.dtype == torch.float32 else c.rounded(EXACT[name])
            assert torch.equal(got, want), f"{tag} {name}: {gx.first_diff(got, want)}"
        elif name == "dgelu_aux":
            assert torch.equal(got, c.codes), f"{tag}: the DGELU epilogue changed its side band"
        elif name == "dgelu":
            ratios = {"dgelu": gx.over_bar((got.double() - c("dgelu")).abs(), gx.dgelu_bar(c("acc"), c("dgelu"), h))}
        elif name == "gelu":
            ratios = {"gelu": (got.double() - c("gelu")).abs() / gx.gelu_bar(c("bias"), h)}
        elif name == "gelu_aux":
            ratios = {"gelu_prime": (got.double() * gx.DG8_STEP - gx.DG8_OFF - c("gelu_prime")).abs() / gx.GELU_PRIME_BAR}
        if name in ("dgelu", "gelu", "gelu_aux"):
            for k, r in ratios.items():
                r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
                top = r.max().item()
                if top >= worst.get(k, (-1.0,))[0]:
                    i, j = divmod(r.argmax().item(), N)
                    worst[k] = (top, f"{tag} at ({i}, {j})")


def _assert_bars(test, worst, **where):
    _log(test, **where, **{k + "_err_over_bar": v[0] for k, v in worst.items()}, **{k + "_at": v[1] for k, v in worst.items()})
    for k, (top, at) in worst.items():
        assert top <= 1.0, f"{k}: err / bar = {top} in {at}"


# -------------------------------------------------------------------------------------- a. rows x tiles x leading dimensions
@pytest.mark.parametrize("N,K", gx.ROWS_NK)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 8])
def test_gemm_exact_rows_tiles_strides(ops, tile, dtype, N, K):
    """Every epilogue of bsclip_gemm_bf16 at M = 1 .. 513 (gemm_exact.ROWS), twice: at the smallest leading dimensions the entry
    point admits and 64 wider.  N = 128 and 384 send tiles 3 / 4 / 8 to the 256x128 kernel (pick_tile) and are the 128-wide
    kernels' only odd column-tile counts; K = 64 is one K-tile (tile 8 falls back to the ping-pong kernel), 128 the persistent
    kernel's minimum, 192 and 832 odd counts.  Tile 5 has no fp16 form and runs as tile 4.

    Bars.  Linear epilogues: torch.equal with f64 (rounded once for 16-bit outputs).
    DGELU: |out - acc z| <= u |acc z| + |acc| 2^-22 with z = code * 1.26 / 255 - 0.13 in f64, u = 2^-8 (bf16) / 2^-11 (fp16): one
    rounding of the output, plus the kernel's f32 evaluation of z, which cancels near code 26 -- derivation in gemm_exact.dgelu_bar.
    GELU: |out - gelu(x)| <= u |gelu(x)| + 2e-6 max(|x|, 1) + 2^-21 |x| at the exact pre-activation x: the output's rounding, the
    Phi bound csrc/gemm_epilogue.h documents, a few f32 ulps of evaluation.  Side band: within half a code step + 6e-4 of gelu'(x)."""
    worst = {}
    try:
        ops.set_gemm_tile(tile)
        for M in gx.ROWS:
            c = _case(M, N, K, dtype)
            for extra in (0, 64):
                _verify(c, _run(ops, c, extra, EPILOGUES), f"tile {tile} M={M} N={N} K={K} ld+{extra}", worst)
    except BaseException:      # an exact comparison failed: the figures gathered so far still get printed
        _log("gemm_exact_rows_tiles_strides (incomplete)", tile=tile, dtype=str(dtype), N=N, K=K, **{k: v[0] for k, v in worst.items()})
        raise
    finally:
        ops.set_gemm_tile(0)
    _assert_bars("gemm_exact_rows_tiles_strides", worst, tile=tile, dtype=str(dtype), N=N, K=K)


# ------------------------------------------------------------------------------------------------------- b. patch epilogue
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", [1, 2, 4, 5, 8])
def test_gemm_patch_exact_and_class_rows_untouched(ops, tile, dtype):
    """PATCH_F32 / PATCH_16: row 196 b + p of the product, + bias + pos[1 + p], lands in row 197 b + 1 + p.  One image (fewer rows
    than any tile), then two and three (image boundaries inside the 256- and 128-row panels, last panels of 136 and 76 rows).
    Outputs are NaN-filled, so a class-token row 197 b that the kernel wrote -- zeros included -- is no longer NaN."""
    from bioscanclip.hip.lib import EPI_PATCH_BF16, EPI_PATCH_F32
    N, K = gx.PATCH_N, gx.PATCH_K
    try:
        ops.set_gemm_tile(tile)
        for M in gx.PATCH_M:
            c = _case(M, N, K, dtype)
            B = M // 196
            _, pos = gx.strided(197 - 3, N, N + 4, torch.float32, device=DEV)      # [197, N], ld_resid = N + 4
            pos[:] = c.pos
            rows = c.patch_rows()
            for epi, dt in ((EPI_PATCH_F32, torch.float32), (EPI_PATCH_BF16, dtype)):
                buf, view = gx.strided(197 * B, N, N + 4, dt, device=DEV)
                ops.gemm(c.a_ld, c.b, view, epi, bias=c.bias, resid=pos, M=M)
                tag = f"tile {tile} M={M} {dt}"
                want = c("patch").float() if dt == torch.float32 else c.rounded("patch")
                got = buf[rows, :N]
                assert torch.equal(got, want), f"{tag}: {gx.first_diff(got, want)}"
                assert torch.isnan(buf[0:197 * B:197, :N]).all(), f"{tag}: a class-token row was written"
                assert gx.untouched(buf, 197 * B, N), f"{tag}: spare rows / pad columns written"
    finally:
        ops.set_gemm_tile(0)


# ----------------------------------------------------------------------------------------------- c. persistent tile walk
@pytest.mark.parametrize("M,N,K", gx.PERS_MNK)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_persistent_walk_exact(ops, dtype, M, N, K):
    """The persistent kernel (tile 8) against f64, not against its sibling: 12 column tiles (super-columns of 6, last row panel of
    ONE row), 8 (super-columns of 4), 7 (prime: one super-column), 1 (the walk is over row panels only); grids of 1 and 5
    workgroups (every workgroup walks several tiles), exactly the tile count, 3 more (the launch clamps it) and the default of one
    per CU.  All six epilogues it has, bars as in test_gemm_exact_rows_tiles_strides, smallest leading dimensions, sentinels around
    every output.  Then bit equality with the ping-pong kernel (tile 4), the contract test_gemm_persistent_walks_tiles states."""
    c = _case(M, N, K, dtype)
    nt = (M + 255) // 256 * (N // 256)
    worst = {}
    try:
        ops.set_gemm_tile(4)
        ref = _run(ops, c, 0, PERS_EPILOGUES)
        ops.set_gemm_tile(8)
        for wgs in (1, 5, nt, nt + 3, 0):
            ops.set_gemm_persistent_grid(wgs)
            got = _run(ops, c, 0, PERS_EPILOGUES)
            _verify(c, got, f"persistent M={M} N={N} K={K} wgs={wgs}", worst)
            for k in ref:
                assert torch.equal(got[k][:M, :N], ref[k][:M, :N]), f"wgs={wgs} {k}: {gx.first_diff(got[k][:M, :N], ref[k][:M, :N])} (tile 8 vs 4)"
    except BaseException:
        _log("gemm_persistent_walk_exact (incomplete)", dtype=str(dtype), M=M, N=N, K=K, **{k: v[0] for k, v in worst.items()})
        raise
    finally:
        ops.set_gemm_tile(0)
        ops.set_gemm_persistent_grid(0)
    _assert_bars("gemm_persistent_walk_exact", worst, dtype=str(dtype), M=M, N=N, K=K)


# ----------------------------------------------------------------------------------------------------------- d. split-K
@pytest.mark.parametrize("M,splits", gx.SPLITK_M_SPLITS)
def test_gemm_splitk_exact_strided(ops, M, splits):
    """bsclip_gemm_splitk_f32 with ldc = N + 4 and partial row panels under splits > 1 (one row; 255; 257: a one-row second panel;
    300 unsplit).  C is preloaded with exact values, the slabs with NaN: a slab element that the reduction reads without the
    product kernel having written it turns its output NaN.  C == f64, bit for bit, twice."""
    N, K = gx.SPLITK_N, gx.SPLITK_K
    c = _case(M, N, K, torch.bfloat16)
    want = c("resid").float()
    outs = []
    for _ in range(2):
        buf, view = gx.strided(M, N, N + 4, torch.float32, device=DEV)
        view[:M] = c.resid
        partial = torch.full((splits * M * N,), NAN, device=DEV)
        ops.gemm_splitk_f32(c.a_ld, c.b, view[:M], splits, partial, K=K)
        got = buf[:M, :N]
        assert torch.equal(got, want), f"M={M} splits={splits}: {gx.first_diff(got, want)}"
        assert gx.untouched(buf, M, N), f"M={M} splits={splits}: spare rows / pad columns written"
        outs.append(got.clone())
    assert torch.equal(outs[0], outs[1])
