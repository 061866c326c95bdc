"""Operands whose GEMM is exact, and the f64 value of every epilogue of bsclip_gemm_bf16 on them.

``a`` holds integers in [-4, 4], ``b`` integers in [-4, 4] divided by 64, ``bias`` integers in [-8, 8] / 64, ``resid`` and ``pos``
integers in [-64, 64] / 64.  All of them are exactly representable in bf16 and in fp16 (at most 7 significant bits), every product
a * b is a multiple of 1/64, and every partial sum of K <= 4096 of them (plus bias, plus residual) is a multiple of 1/64 below
2^24 / 64 in magnitude: an f32 accumulator holds it exactly whatever the order of the additions, MFMA or not.  So the linear
epilogues of a correct kernel equal f64 arithmetic BIT FOR BIT (f32 outputs) or are ONE round-to-nearest-even of it (16-bit
outputs), and a test needs no tolerance: one dropped or doubled K chunk, two swapped rows, a store a few columns off or a
truncating conversion changes an element.  tests/test_04_gemm_exact_cpu.py proves these claims on the CPU.

Nothing here needs a GPU: every function computes on the device it is asked for with plain torch f64 / integer ops."""
import math

import torch

DG8_STEP, DG8_OFF = 1.26 / 255, 0.13          # the 8-bit gelu' side band: value = code * DG8_STEP - DG8_OFF (csrc/common.h)
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SENT8 = 0xA5                                  # sentinel byte of the uint8 side band


# the cases of tests/test_14_gemm_edges_gpu.py; tests/test_04_gemm_exact_cpu.py proves its bars over the same ones
SEED = 14
ROWS = (1, 8, 15, 16, 17, 127, 128, 129, 255, 256, 257, 513)     # below one MFMA row block, tile +- 1 for the 128- / 256-row tiles
ROWS_NK = ((128, 64), (384, 192), (256, 128), (768, 832))       # (N, K): N % 256 != 0 twice; 1, 3, 2 and 13 K-tiles
PATCH_M, PATCH_N, PATCH_K = (196, 392, 588), 768, 768
PERS_MNK = ((769, 3072, 128), (300, 2048, 192), (513, 1792, 128), (1300, 256, 832))
SPLITK_M_SPLITS, SPLITK_N, SPLITK_K = ((1, 2), (255, 3), (257, 8), (300, 1)), 256, 64 * 24


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int32)


def operands(M, N, K, seed, dtype):
    """dict of CPU tensors: a [M, K] and b [N, K] in ``dtype``; bias [N], resid [M, N], pos [197, N] in f32; codes [M, N] uint8
    (random gelu' codes for the DGELU epilogue).  The same values for bf16 and fp16."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
    a = _ints((M, K), -4, 4, g).float()
    b = _ints((N, K), -4, 4, g).float() / 64
    bias = _ints((N,), -8, 8, g).float() / 64
    resid = _ints((M, N), -64, 64, g).float() / 64
    pos = _ints((197, N), -64, 64, g).float() / 64
    codes = torch.randint(0, 256, (M, N), generator=g, dtype=torch.uint8)
    return dict(a=a.to(dtype), b=b.to(dtype), bias=bias, resid=resid, pos=pos, codes=codes)


def gelu64(x):
    """x Phi(x) in f64; erfc keeps the left tail from cancelling."""
    return 0.5 * x * torch.erfc(-x / math.sqrt(2))


def dgelu64(x):
    """Phi(x) + x phi(x) in f64."""
    return 0.5 * torch.erfc(-x / math.sqrt(2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


class Exact:
    """One case: its operands on ``device`` and the f64 value of each epilogue, computed when first asked for."""

    def __init__(self, M, N, K, seed, dtype, device):
        self.M, self.N, self.K, self.dtype = M, N, K, dtype
        for k, v in operands(M, N, K, seed, dtype).items():
            setattr(self, k, v.to(device))
        self._vals = {}

    def __call__(self, name):
        if name not in self._vals:
            self._vals[name] = self._compute(name)
        return self._vals[name]

    def _compute(self, name):
        if name == "acc":
            return self.a.double() @ self.b.double().t()
        if name == "bias":                                   # acc + bias
            return self("acc") + self.bias.double()
        if name == "bias_resid":                             # acc + bias + resid
            return self("bias") + self.resid.double()
        if name == "resid":                                  # acc + resid (the in-place accumulation, no bias)
            return self("acc") + self.resid.double()
        if name == "patch":                                  # [M, N]: row m is written to row patch_rows()[m] of the output
            return self("bias") + self.pos.double()[1 + torch.arange(self.M, device=self.pos.device) % 196]
        if name == "dgelu":                                  # acc * gelu'(code)
            return self("acc") * (self.codes.double() * DG8_STEP - DG8_OFF)
        if name == "gelu":                                   # gelu(acc + bias)
            return gelu64(self("bias"))
        if name == "gelu_prime":                             # gelu'(acc + bias): what the side band encodes
            return dgelu64(self("bias"))
        raise KeyError(name)

    def patch_rows(self):
        m = torch.arange(self.M, device=self.a.device)
        return 197 * (m // 196) + 1 + m % 196

    def rounded(self, name):
        """The 16-bit output of a linear epilogue: one RNE of the exact value (which an f32 holds exactly, so going through f32
        rounds once)."""
        return self(name).float().to(self.dtype)


_CACHE = {}


def ref64(M, N, K, seed, dtype, device="cpu"):
    """The case (operands + f64 epilogue values) for a shape; cached, so that a tile parametrisation computes it once."""
    key = (dtype, M, N, K, seed, str(device))
    if key not in _CACHE:
        _CACHE[key] = Exact(M, N, K, seed, dtype, device)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------- the kernels' GELU table
_LUT = {}


def _lut(device):
    if str(device) not in _LUT:
        x = -8.0 + torch.arange(256, dtype=torch.float64, device=device) / 16
        _LUT[str(device)] = ((0.5 * (1 + torch.erf(x / math.sqrt(2)))).float(),
                             (torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)).float())
    return _LUT[str(device)]


def gelu_table_f32(x):
    """gelu_lut2 of csrc/gemm_epilogue.h restated in torch f32, statement by statement: (gelu(x), gelu'(x)).  256 entries
    {Phi, phi} on a 1/16 grid over [-8, 8), nearest entry by RNE of t = 16 x + 128 saturated to [0, 255], first-order correction
    from the derivatives.  Exists to prove the GPU tests' bars on the CPU; never used as an expected value."""
    assert x.dtype == torch.float32
    Phi_t, phi_t = _lut(x.device)
    t = x * 16.0 + 128.0
    i = torch.round(t).clamp(0, 255).long()                 # torch.round: half to even, like v_cvt_pk_u8_f32
    Phi, phi = Phi_t[i], phi_t[i]
    fi = (t + 12582912.0) - 12582912.0                      # RNE(t), NOT saturated: d stays small, phi(+-8) ~ 5e-15 hides it
    d16 = t - fi
    e = d16 * phi
    xd = (fi * 0.00390625 - 0.5) * d16
    cdf = e * (0.0625 - xd * 0.03125) + Phi
    pdf = phi - xd * phi
    return x * cdf, x * pdf + cdf


def dg8_codes_f32(dg):
    """dg8_pack4 of csrc/common.h: the 8-bit code of a gelu' value, f32 arithmetic, RNE, saturated."""
    scale = torch.tensor(255.0, dtype=torch.float32) / torch.tensor(1.26, dtype=torch.float32)
    off = torch.tensor(0.13, dtype=torch.float32) * scale
    return torch.round(dg * scale.to(dg.device) + off.to(dg.device)).clamp(0, 255).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ the bars
def gelu_bar(x, dtype):
    """|out - gelu(x)| allowed for a 16-bit GELU output at exact pre-activation x (f64): one rounding of the output, the table's
    documented Phi error 2e-6 times |x| (at least 2e-6), a few f32 ulps of the evaluation."""
    return UNIT_ROUNDOFF[dtype] * gelu64(x).abs() + 2e-6 * x.abs().clamp(min=1.0) + 2.0 ** -21 * x.abs()


GELU_PRIME_BAR = 0.5 * DG8_STEP + 6e-4    # side band: half a code step + the table's phi error (tests/test_10_kernels_gpu.py)


def dgelu_bar(acc, ref, dtype):
    """|out - acc * z(code)| allowed for the DGELU output.  u |ref|: the one rounding of the output.  |acc| 2^-22: the kernel forms
    z = fma(code, f32(1.26 / 255), -f32(0.13)) in f32 -- 255 half-ulps of the step (5.9e-8), half an ulp of 0.13 (7.5e-9) and the
    fma's own rounding (<= 6.0e-8) make |z_f32 - z| <= 1.27e-7 absolute, which cancellation near code 26 (z = -1.5e-3) turns into
    a large relative error of z; the product's f32 rounding adds 2^-24 |acc z| <= 0.68e-7 |acc|; together 1.95e-7 |acc| < 2^-22 |acc|.
    (u |ref| is the rounding of a NORMAL number.  The only fp16 outputs below 2^-14 these operands can give are -+ z(26) / 64,
    -+ 2 z(26) / 64 and +- z(27) / 64, subnormals spaced 2^-24; they happen to lie within the bar of a representable value, which
    tests/test_04_gemm_exact_cpu.py checks over every case, so the bar needs no floor.)"""
    return UNIT_ROUNDOFF[dtype] * ref.abs() + acc.abs() * 2.0 ** -22


def over_bar(err, bar):
    """err / bar element by element; where the bar is zero (acc = 0: the DGELU output must be exactly zero) a zero error counts
    as 0 and any other as enormous."""
    return err / bar.clamp(min=1e-300)


# --------------------------------------------------------------------------------------------------- sentinel-filled buffers
def strided(rows, cols, ld, dtype, sentinel=None, device="cpu"):
    """(buf, view): a [rows + 3, ld] buffer filled with the sentinel (by default NaN; byte 0xA5 for uint8) and its [:, :cols]
    view, which ops.gemm takes as a matrix of leading dimension ld."""
    assert ld >= cols
    if sentinel is None:
        sentinel = SENT8 if dtype == torch.uint8 else float("nan")
    buf = torch.full((rows + 3, ld), sentinel, dtype=dtype, device=device)
    return buf, buf[:, :cols]


def untouched(buf, rows, cols):
    """True when every element of ``buf`` outside [:rows, :cols] still holds the sentinel."""
    def sent(t):
        return (t == SENT8).all().item() if t.dtype == torch.uint8 else torch.isnan(t).all().item()
    return sent(buf[rows:]) and sent(buf[:rows, cols:])


def first_diff(got, want):
    """For an assertion message: how many elements differ, and the first one's (row, column, got, want)."""
    bad = (got != want).nonzero()
    if bad.numel() == 0:
        return "equal"
    r, c = bad[0].tolist()
    return f"{bad.shape[0]} elements differ, first at ({r}, {c}): got {got[r, c].item()!r}, want {want[r, c].item()!r}"
