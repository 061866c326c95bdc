"""The claims tests/test_14_gemm_edges_gpu.py rests on, proven without a GPU (tests/gemm_exact.py holds the operands and bars):

* the operands survive bf16 and fp16 unchanged, an f32 accumulation of their products is exact in any order, and every linear
  epilogue's f64 value fits an f32 -- so the GPU test may ask for bit equality;
* rows are distinct and values non-degenerate, so one dropped K chunk, two swapped rows, a store 8 columns off or a truncating
  conversion each change an element of such a comparison;
* the kernels' table-driven GELU, restated in f32, stays inside the GPU test's GELU / gelu' bars over a dense sweep and over every
  pre-activation the GPU test produces, and the f32 gelu'-code decode stays inside the DGELU bar, with the room printed."""
import json
import math

import pytest
import torch

import gemm_exact as gx

DTYPES = [torch.bfloat16, torch.float16]


def _log(test, **figures):
    print("FIGURES " + json.dumps({"test": test, **figures}))


@pytest.mark.parametrize("dtype", DTYPES)
def test_operands_round_trip_and_are_the_same_in_both_formats(dtype):
    o = gx.operands(257, 384, 192, gx.SEED, dtype)
    for k in ("a", "b"):
        assert o[k].dtype == dtype
    for k in ("a", "b", "bias", "resid", "pos"):
        v = o[k].double()
        assert torch.equal(v.to(torch.bfloat16).double(), v) and torch.equal(v.to(torch.float16).double(), v), k
        assert torch.equal(v * 64, (v * 64).round()), f"{k}: not a multiple of 1/64"
    other = gx.operands(257, 384, 192, gx.SEED, DTYPES[1 - DTYPES.index(dtype)])
    assert all(torch.equal(o[k].double(), other[k].double()) for k in o)
    assert o["a"].double().abs().max() == 4 and (o["b"].double().abs().max() * 64) == 4
    assert o["codes"].min() == 0 and o["codes"].max() == 255


@pytest.mark.parametrize("K", [64, 832, 3072])
def test_f32_accumulation_is_exact_in_any_order(K):
    M, N = 129, 128
    c = gx.Exact(M, N, K, gx.SEED, torch.bfloat16, "cpu")
    a, b = c.a.float(), c.b.float()
    want = c("acc")
    assert torch.equal((a @ b.t()).double(), want)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    assert torch.equal((a[:, perm] @ b[:, perm].t()).double(), want)
    # a sequential f32 sum in steps of eight columns, the granularity of one lane's MFMA fragment, forwards and backwards
    for order in (range(0, K, 8), reversed(range(0, K, 8))):
        acc = torch.zeros(M, N)
        for k0 in order:
            acc = acc + a[:, k0:k0 + 8] @ b[:, k0:k0 + 8].t()
        assert torch.equal(acc.double(), want)


def test_partial_sums_stay_below_2_to_the_24_sixty_fourths():
    """|a b| <= 16/64 per term: K terms, a bias (<= 8/64) and a residual (<= 64/64) stay below 2^24 / 64 for every K up to 4096,
    far above the largest K a test uses (3072 here, 1536 in the split-K test, 832 elsewhere)."""
    k_max = max([3072, gx.SPLITK_K, gx.PATCH_K] + [k for _, k in gx.ROWS_NK] + [k for _, _, k in gx.PERS_MNK])
    assert k_max <= 4096 and 16 * 4096 + 8 + 64 < 2 ** 24
    c = gx.Exact(64, 128, 3072, gx.SEED, torch.bfloat16, "cpu")
    assert (c("bias_resid").abs().max() * 64) < 2 ** 24


def test_linear_epilogues_fit_an_f32():
    for (N, K) in gx.ROWS_NK:
        for dtype in DTYPES:
            c = gx.Exact(257, N, K, gx.SEED, dtype, "cpu")
            for name in ("acc", "bias", "bias_resid", "resid", "patch"):
                v = c(name)
                assert torch.equal(v.float().double(), v), (N, K, name)
            # one RNE: through f32 (exact) and straight from f64 agree
            assert torch.equal(c.rounded("bias"), c("bias").to(dtype))


def test_rows_are_distinct_and_preactivations_cover_the_gelu_table():
    figs = {}
    for (N, K) in gx.ROWS_NK + ((128, 3072),):
        c = gx.Exact(513, N, K, gx.SEED, torch.bfloat16, "cpu")
        assert torch.unique(c.a.float(), dim=0).shape[0] == 513, "rows of a repeat"
        assert torch.unique(c("acc"), dim=0).shape[0] == 513, "rows of the product repeat"
        assert torch.unique(c.b.float(), dim=0).shape[0] == N, "rows of b repeat"
        x = c("bias")
        figs[f"K{K}"] = dict(std=round(x.std().item(), 3), beyond8=round((x.abs() > 8).double().mean().item(), 4))
    _log("preactivation_spread", **figs)
    assert 0.80 < figs["K64"]["std"] < 0.88              # interior of the table: 0.84 expected (K 16/9 * 20/3 / 4096 + bias)
    assert 5.6 < figs["K3072"]["std"] < 6.0 and 0.15 < figs["K3072"]["beyond8"] < 0.19     # and both saturated ends


@pytest.mark.parametrize("dtype", DTYPES)
def test_subtle_errors_change_an_exact_comparison(dtype):
    """The errors the GPU test claims to catch, each applied to the reference: none of them survives torch.equal."""
    M, N, K = 129, 384, 192
    c = gx.Exact(M, N, K, gx.SEED, dtype, "cpu")
    a, b = c.a.double(), c.b.double()
    want32, want16 = c("bias").float(), c.rounded("bias")
    bias = c.bias.double()
    # one 8-element K chunk dropped / added twice, in ONE row
    for sign in (-1, 1):
        wrong = c("bias").clone()
        wrong[77] += sign * (a[77, 64:72] @ b[:, 64:72].t())
        assert not torch.equal(wrong.float(), want32) and not torch.equal(wrong.float().to(dtype), want16)
    # a swapped row pair (the last two rows: a one-row last panel), in every pair of neighbours
    for r in range(M - 1):
        assert not torch.equal(want32[r], want32[r + 1]) and not torch.equal(want16[r], want16[r + 1])
    # a store 8 columns off (any 4-column piece, any row)
    assert not torch.equal(want32[:, 8:], want32[:, :-8]) and (want32[:, 8:] != want32[:, :-8]).any(dim=1).all()
    # truncation instead of RNE of the 16-bit output.  bf16 (8 significant bits) rounds these sums, so the exact comparison sees
    # it; fp16 (11 bits) holds every multiple of 1/64 below 32 exactly and rounds nothing here -- in fp16 the rounding mode is held
    # by the DGELU bar below, whose products acc * z are not representable
    def trunc16(x):
        bits = x.view(torch.int32)
        if dtype == torch.bfloat16:
            return (bits & ~0xFFFF).view(torch.float32).to(dtype)
        return torch.where(x.abs() >= 2.0 ** -14, (bits & ~0x1FFF).view(torch.float32), x).to(dtype)
    if dtype == torch.bfloat16:
        assert not torch.equal(trunc16(want32), want16)
    else:
        assert torch.equal(want32.to(dtype).float(), want32)
    prod = c("dgelu").float()
    bar = gx.dgelu_bar(c("acc"), c("dgelu"), dtype)
    assert ((prod.to(dtype).double() - c("dgelu")).abs() <= bar).all()
    assert ((trunc16(prod).double() - c("dgelu")).abs() > bar).double().mean() > 0.25, "a truncating DGELU output passes its bar"


def test_strided_and_untouched():
    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.uint8):
        buf, view = gx.strided(5, 128, 132, dtype)
        assert buf.shape == (8, 132) and view.shape == (8, 128) and view.stride(0) == 132 and view.data_ptr() == buf.data_ptr()
        view[:5] = 1
        assert gx.untouched(buf, 5, 128)
        for r, col in ((5, 0), (7, 131), (0, 128), (4, 131)):
            b2 = buf.clone()
            b2[r, col] = 0
            assert not gx.untouched(b2, 5, 128), (dtype, r, col)


# ---------------------------------------------------------------------------------------------------------- the GELU bars
ROOM = 0.6   # share of a bar's non-rounding part the f32 restatement may use: the rest is for the GPU's fused / packed arithmetic


def _gelu_room(x32, dtype):
    """The f32 table restatement at pre-activations x32 (f32, exact in f64) against the GPU test's bars.  Each bar is a rounding
    the output format cannot avoid (one RNE to 16 bits: u |gelu|; the 8-bit code: half a step), which an honest kernel uses up
    entirely at some element, plus a term for the table and its f32 evaluation.  So two figures each: the total err / bar, which
    must stay below 1, and the error BEFORE the rounding over the second term alone, which is where room can be."""
    gl, dg = gx.gelu_table_f32(x32)
    x = x32.double()
    g, gp = gx.gelu64(x), gx.dgelu64(x)
    u = gx.UNIT_ROUNDOFF[dtype]
    band = gx.dg8_codes_f32(dg).double() * gx.DG8_STEP - gx.DG8_OFF
    return dict(gelu=((gl.to(dtype).double() - g).abs() / gx.gelu_bar(x, dtype)).max().item(),
                gelu_unrounded=((gl.double() - g).abs() / (gx.gelu_bar(x, dtype) - u * g.abs())).max().item(),
                band=((band - gp).abs() / gx.GELU_PRIME_BAR).max().item(),
                band_unrounded=((dg.double() - gp).abs() / (gx.GELU_PRIME_BAR - 0.5 * gx.DG8_STEP)).max().item())


def _gelu_room_ok(r):
    return r["gelu"] < 1 and r["band"] < 1 and r["gelu_unrounded"] < ROOM and r["band_unrounded"] < ROOM


def test_interpolation_formula_meets_the_documented_bounds():
    """In f64 (no evaluation error): Phi_i + d phi_i (1 - x_i d / 2) against Phi, phi_i (1 - x_i d) against phi.  The header of
    csrc/gemm_epilogue.h documents 2e-6 and 2e-4; as GELU and gelu' that is 2e-6 max(|x|, 1) and 2e-4 (1 + |x| phi-error)."""
    x = torch.linspace(-30, 30, 2 ** 21 + 1, dtype=torch.float64)
    i = torch.round(x * 16 + 128).clamp(0, 255)
    xi_tab = -8 + i / 16
    xi = torch.round(x * 16) / 16                 # the unsaturated grid point the kernel measures d from
    d = x - xi
    Phi_i = 0.5 * torch.erfc(-xi_tab / math.sqrt(2))
    phi_i = torch.exp(-0.5 * xi_tab * xi_tab) / math.sqrt(2 * math.pi)
    cdf = Phi_i + d * phi_i * (1 - xi * d / 2)
    pdf = phi_i * (1 - xi * d)
    e_gelu = ((x * cdf - gx.gelu64(x)).abs() / x.abs().clamp(min=1)).max().item()
    e_prime = (x * pdf + cdf - gx.dgelu64(x)).abs().max().item()
    _log("gelu_formula_f64", gelu_err_over_max_x_1=e_gelu, gelu_prime_err=e_prime)
    assert e_gelu < 2e-6 and e_prime < 2e-4


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_table_stays_inside_the_gpu_bars_dense_sweep(dtype):
    x = torch.cat([torch.linspace(-30, 30, 2 ** 21 + 1, dtype=torch.float64).float(),
                   torch.arange(-30 * 64, 30 * 64 + 1, dtype=torch.float32) / 64])       # + every pre-activation value possible
    r = _gelu_room(x, dtype)
    _log("gelu_table_room_dense", dtype=str(dtype), **r)
    assert _gelu_room_ok(r), "the f32 table restatement leaves no room under a GPU bar"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_and_dgelu_bars_hold_on_every_gpu_case(dtype):
    """Every pre-activation of test_gemm_exact_rows_tiles_strides and test_gemm_persistent_walk_exact through the f32 table, and
    every (acc, code) pair through the kernel's f32 decode  out = RNE16(acc * fma(code, f32(1.26 / 255), -f32(0.13)))."""
    cases = [(M, N, K) for (N, K) in gx.ROWS_NK for M in gx.ROWS] + list(gx.PERS_MNK)
    worst, n_subnormal = {}, 0
    step, off = torch.tensor(1.26 / 255, dtype=torch.float32), torch.tensor(0.13, dtype=torch.float32)
    for (M, N, K) in cases:
        c = gx.Exact(M, N, K, gx.SEED, dtype, "cpu")
        r = _gelu_room(c("bias").float(), dtype)
        # f32 decode; torch has no fused multiply-add, the f64 product rounded once is one (exact product, one rounding)
        z = (c.codes.double() * step.double() - off.double()).float()
        prod = c("acc").float() * z
        acc, ref = c("acc"), c("dgelu")
        r["dgelu"] = gx.over_bar((prod.to(dtype).double() - ref).abs(), gx.dgelu_bar(acc, ref, dtype)).max().item()
        r["dgelu_unrounded"] = gx.over_bar((prod.double() - ref).abs(), acc.abs() * 2.0 ** -22).max().item()
        if dtype == torch.float16:      # the subnormal outputs the DGELU bar's docstring speaks of do occur
            n_subnormal += ((ref.abs() < 2.0 ** -14) & (ref != 0)).sum().item()
        worst = {k: max(worst.get(k, 0.0), v) for k, v in r.items()}
    _log("gelu_dgelu_room_gpu_cases", dtype=str(dtype), fp16_subnormal_dgelu_outputs=n_subnormal, **worst)
    assert dtype != torch.float16 or n_subnormal > 0
    assert _gelu_room_ok(worst) and worst["dgelu"] < 1 and worst["dgelu_unrounded"] < 0.85   # 1.95e-7 / 2^-22 = 0.82 is the derived worst
