"""Inputs, f64 references, comparisons and bars for the kernels a training step launches beside the GEMMs, the attention, the row
reductions and the losses: the data movement of csrc/embed.hip, the pooling heads of csrc/heads.hip, l2norm (csrc/norm.hip), the
elementwise helpers of the fp16 backward, count_nonfinite / counter_add / mask_to_bias / gather_cast_rows and the AdamW update.

Two kinds of input.  EXACT inputs -- small integers, powers of two, values with few significant bits -- on which the operation has one
right answer in f32 (or in the 16-bit output format after ONE round-to-nearest-even): the kernel is held to BIT equality, -0 and +0
told apart, NaN matching NaN.  Every such reference asserts its own condition (``_exact``: magnitudes in units of the smallest step
below 2^24).  REAL-valued inputs where the arithmetic truly rounds (AdamW, l2norm, the softmax pooling, the token mean): there the
comparison is per ELEMENT, against an allowance made of a bar times a scale the element itself sets (its ulp, its own magnitude, its
row's largest magnitude) plus, for a bf16 output, half a bf16 ulp of the reference value.  Never a whole-tensor norm.

The bars (``BAR[key]``) are 4 x the worst distance between the f64 reference and the kernel's arithmetic restated in f32 on the CPU
(tests/test_04_tail_exact_cpu.py: same formula and association as the source, no fused multiply-adds, the wave butterfly in lane
order, exp correctly rounded to f32), over every case the GPU file runs; the factor covers fused multiply-adds, another association
of the wave reduction and the fast exponential.  ``MEASURED[key]`` are those worst distances; the CPU file asserts BAR == 4 x what it
measures today.  No figure comes from a GPU run.  AdamW is held step by step: each step's (p, m, v) against f64 of the f32 state that
step started from, so a trajectory's carried rounding never counts against a later step.

Inputs are functions of the element index (an integer hash), so any device builds the same values without a generator.
Nothing here needs a GPU: every function computes on the device its tensors live on with plain torch ops."""
import math
import struct

import torch

from gemm_exact import first_diff, strided, untouched  # noqa: F401  (the sentinel-buffer helpers, shared with the GEMM suites)

NAN = float("nan")
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
EXACT_LIMIT = 2.0 ** 24

# ---- grid caps, each read from the line named (no entry point reports them) ---------------------------------------------------------
CAST_CAP = 2048 * 256 * 4        # csrc/embed.hip bsclip_cast_f32_bf16 / _f16 / _f16_scaled: grid4x256(n, 2048), 4 elements a thread = 2^21
ADD_SCALED_CAP = 1024 * 256 * 4  # csrc/optim.hip bsclip_add_scaled_f32: grid4x256(n, 1024) = 2^20
ADAMW_CAP = 2048 * 256           # csrc/optim.hip adamw_grid: 2048 workgroups of 256 threads, one element each = 524 288
NONFINITE_CAP = 2048 * 256       # csrc/api.hip bsclip_count_nonfinite: "if (blocks > 2048) blocks = 2048"
IM2COL_CAP = 4096 * 256          # csrc/embed.hip bsclip_im2col_patch16: "if (blocks > 4096) blocks = 4096"; B * 196 * 96 items
DGELU_CAP = 4096 * 256           # csrc/heads.hip bsclip_dgelu_mul: the same cap over M * N / 4 items
IM2COL_ITEMS_PER_IMAGE = 196 * 96   # 18 816: B = 55 -> 1 034 880 < cap, B = 56 -> 1 053 696 > cap, B = 112 -> 2 107 392 > 2 cap


def _around(cap):
    return (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, cap - 1, cap, cap + 1, cap + 1027, 2 * cap + 5)


CAST_N = _around(CAST_CAP)
ADD_SCALED_N = _around(ADD_SCALED_CAP)
ADD_SCALED_K = (-64, -13, 0, 13, 64)
CAST_SCALED_K_ALL_N = (-13, 13)                 # at every n of CAST_N
CAST_SCALED_K_EXTRA = (-64, -20, 0, 64)         # at CAST_SCALED_EXTRA_N
CAST_SCALED_EXTRA_N = (1027, CAST_CAP + 1027)
ADAMW_N = (1, 63, 255, 256, 257, ADAMW_CAP - 1, ADAMW_CAP, ADAMW_CAP + 1, ADAMW_CAP + 259, 2 * ADAMW_CAP + 1)
IM2COL_B = {"bf16-split": (1, 55, 56, 112), "bf16": (1, 56), "fp16": (1, 56), "fp16-split": (1, 56)}
DGELU_MN = ((1366, 3072), (2731, 3072))         # 1 049 088 items (one past the cap's 1 048 576) and 2 097 408 (two passes past it)
SOFTMAX_BS = ((1, 1), (1, 2), (1, 3), (2, 4), (3, 5), (3, 7), (5, 133))
SOFTMAX_SCALES = (0.01, 3.0, 30.0, 50.0)
SOFTMAX_C = 768
MEANPOOL_H, MEANPOOL_S, MEANPOOL_B = (512, 768), (1, 7, 20), (1, 2, 3)   # B * H / 4 = 128, 192, 256, 384, 576: below, at, no multiple of 256
EMBED_H, EMBED_BS, EMBED_VOCAB = (512, 768), ((1, 1), (1, 3), (1, 5), (3, 43), (2, 133)), 37
L2_D, L2_M = (4, 512, 768), (1, 3, 4, 5, 37)
CLS_H, CLS_B, CLS_S = (512, 768), (1, 3), 5
WAUG_H, WAUG_LAYERS = (512, 768), 3
MASK_N = (1, 255, 256, 257, 1000)
GATHER_CASES = ((197, 196, 1, 393), (197, 1, 0, 3), (5, 3, 2, 7), (1, 1, 0, 5))   # (period_in, period_out, offset, rows_out); rows_out % 4 != 0
GATHER_H = (512, 768)
TRANSPOSE_R, TRANSPOSE_C = (1, 63, 64, 65, 130), (1, 64, 200)
TRANSPOSE_MODES = ("ld_in", "ld_out", "base_in", "base_out")

DG8_STEP, DG8_OFF = 1.26 / 255, 0.13          # tests/test_12_exact_kernels_gpu.py: gelu' codes, decode = code * step - 0.13
F32_MIN = -3.4028234663852886e38              # csrc/embed.hip mask_to_bias_kernel: finfo(float32).min

# ---- bars: MEASURED is what tests/test_04_tail_exact_cpu.py measures on the CPU restatement (test_bars_are_four_times_...), BAR = 4 x that
MEASURED = {
    "adamw_p_ulps": 4.254713406786323,
    "adamw_m_rel": 1.795696781507109e-07,
    "adamw_v_rel": 1.450424815732664e-07,
    "l2norm_fwd_row": 1.2278099678663688e-07,
    "l2norm_inv_rel": 1.188309947363322e-07,
    "l2norm_bwd_row": 1.0398735156971246e-07,
    "softmax_pooled_row": 2.5052537056758666e-07,
    "softmax_sum_rel": 2.2776046300254624e-07,
    "softmax_bwd_row": 2.084590836604486e-06,
    "meanpool_fwd_row": 1.7181093243339168e-07,
}
BAR = {k: 4.0 * v for k, v in MEASURED.items()}


def f32r(x):
    """The f32 value nearest to the Python float x, as a Python float: what a C ABI taking ``float`` receives."""
    return struct.unpack("f", struct.pack("f", x))[0]


# ---------------------------------------------------------------------------------------------------------------- inputs from hashes
def _hash(n, salt, device="cpu"):
    i = torch.arange(n, dtype=torch.int64, device=device)
    h = (i * 2654435761 + salt * 40503 + 12345) & 0x7FFFFFFF
    h = ((h ^ (h >> 15)) * 73244475) & 0x7FFFFFFF
    h = ((h ^ (h >> 13)) * 19349663) & 0x7FFFFFFF
    return h ^ (h >> 16)


def hash_ints(n, lo, hi, salt, device="cpu"):
    """n integers in [lo, hi] (int64), a function of (index, salt) alone."""
    return _hash(n, salt, device) % (hi - lo + 1) + lo


def hash_real(n, salt, device="cpu"):
    """n f64 values of roughly unit normal spread (four 20-bit uniforms summed), each exact in f64, a function of (index, salt) alone."""
    u = sum((_hash(n, 4 * salt + k, device) % (1 << 20)).double() for k in range(4)) / (1 << 20)
    return (u - 2.0) * math.sqrt(3.0)


def _exact(terms_abs, unit, what):
    top = float(terms_abs.max().item()) / unit
    assert top < EXACT_LIMIT, f"{what}: |terms| reach {top} units of {unit}, not below 2^24"
    return top


# ---------------------------------------------------------------------------------------------------------------------- comparisons
def _ibits(t):
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def bits_equal(got, want):
    """Same shape and dtype, the same bits in every element (+0 and -0 differ), except that any NaN matches any NaN."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not got.dtype.is_floating_point:
        return torch.equal(got, want)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and bool(((_ibits(got.contiguous()) == _ibits(want.contiguous())) | wn).all().item())


def bits_diff(got, want):
    """For an assertion message: the number of elements whose bits differ and the first one (flat index, got, want)."""
    g, w = got.contiguous().reshape(-1), want.contiguous().reshape(-1)
    bad = ((_ibits(g) != _ibits(w)) & ~(torch.isnan(g) & torch.isnan(w))).nonzero()
    if bad.numel() == 0:
        return "equal"
    i = int(bad[0])
    return f"{bad.shape[0]} of {g.numel()} elements differ, first at {i}: got {g[i].item()!r}, want {w[i].item()!r}"


def ulp32(x):
    """The f32 unit in the last place of |x| (f64 tensor), 2^-149 at and below the subnormals."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=F64), e - 24)


def half_ulp_bf16(x):
    """Half a bf16 unit in the last place of |x| (f64 tensor): what one rounding to bf16 may move the value by."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=F64), e - 9)


def worst(got, want, allowance):
    """max over elements of |got - want| / allowance (f64); an element whose allowance is 0 must be equal; NaN counts as infinite."""
    d = (got.double() - want.double()).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / allowance.double().expand_as(d))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max().item())


def rowmax(want):
    return want.double().abs().amax(dim=-1, keepdim=True)


def row_allowance(want, bar, bf16_out=False):
    """bar x the row's largest magnitude, plus half a bf16 ulp of the element for a bf16 output."""
    a = bar * rowmax(want).expand_as(want)
    return a + half_ulp_bf16(want) if bf16_out else a


# ---------------------------------------------------------------------------------------------------------------------------- casts
def _f32_from_bits(words):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).view(F32)


CAST_SPECIAL_BITS = (
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF,   # +-0, +-inf, NaN, +-largest finite
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,       # bf16 ties: 1 + 2^-8 (down to even), 1 + 3 2^-8 (up to even), both signs
    0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000,       # fp16 ties: 1 + 2^-11 (down), 1 + 3 2^-11 (up), both signs
    0x3FFFFFFF, 0x3FFF8000, 0x3FFFF000, 0xBFFFFFFF,       # round up into the next binade (bf16 tie to 2.0; fp16 tie to 2.0)
    0x477FEFFF, 0x477FF000, 0x477FF001, 0x477FE000, 0xC77FF000, 0x47800000,   # fp16 overflow: just below 65 520, the tie (-> inf), above; 65 504
    0x33800000, 0x33000000, 0x33000001, 0x33C00000, 0x38000000, 0x387FC000, 0x35866666, 0xB3000001,  # fp16 subnormals: 2^-24, ties 2^-25 / 3 2^-25
    0x00000001, 0x007FFFFF, 0x80000001, 0x00400000, 0x00800000,                       # f32 subnormals, the smallest normal
    0x1C800000, 0x1CFFF000, 0x58000000, 0x587FE000, 0x3F9E0419,   # 2^-70 / 2^49 / 1.2345: what 2^+-64 and 2^-20 carry into the fp16 (sub)normal range
)


def cast_input(n, salt=0, cap=CAST_CAP, device="cpu"):
    """n f32 values: magnitudes spread log-uniformly over 2^-30 .. 2^18 (fp16 subnormals, fp16 overflow) with 12 random mantissa bits
    kept below the 16-bit formats' last place, and the table of special values at the front, at the back (the n & 3 tail) and astride
    the end of the first grid-stride pass."""
    sp = _f32_from_bits(list(CAST_SPECIAL_BITS)).to(device)
    L = sp.numel()
    expo = hash_ints(n, -30, 18, 31 + salt, device).double()
    mant = 1.0 + hash_ints(n, 0, (1 << 23) - 1, 32 + salt, device).double() / (1 << 23)
    sign = 1.0 - 2.0 * hash_ints(n, 0, 1, 33 + salt, device).double()
    x = (sign * mant * torch.exp2(expo)).float()
    idx = torch.arange(n, device=device)
    k = min(n, L)
    x[:k] = sp[(idx[:k] + n) % L]
    x[n - k:] = sp[(idx[:k] * 5 + n) % L]             # 5 and len(table) are coprime: every value reaches the tail over the sizes
    if n > cap + L:
        x[cap - L // 2:cap - L // 2 + L] = sp
    return x


def cast_ref(src, dtype, scale_log2=0):
    """torch's own CPU conversion (round to nearest even) of src * 2^k formed in f32."""
    s = src.detach().cpu()
    if scale_log2:
        s = s * torch.tensor(2.0 ** scale_log2, dtype=F32)
    return s.to(dtype)


# ------------------------------------------------------------------------------------------------------------------ add_scaled_f32
def add_scaled_case(n, k, device="cpu"):
    """(in, out0, want): in = j 2^-k with integer |j| <= 512, out0 = +-(1000 .. 1031); out0 + in 2^k = out0 + j, exact."""
    j = hash_ints(n, -512, 512, 41 + k, device).double()
    out0 = (hash_ints(n, 1000, 1031, 42, device) * (2 * hash_ints(n, 0, 1, 43, device) - 1)).double()
    src = j * 2.0 ** -k
    assert torch.equal(src.float().double(), src), "add_scaled_f32: j 2^-k is not an f32"
    _exact(out0.abs() + j.abs(), 1.0, "add_scaled_f32")
    return src.float(), out0.float(), (out0 + j)


# --------------------------------------------------------------------------------------------------------------------------- AdamW
ADAMW_SETS = {   # name: (hyperparameters, first step word); three steps each
    "defaults": (dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, grad_scale=1.0), 1),
    "wd0": (dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, grad_scale=1.0), 2),
    "scale0.25": (dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, grad_scale=0.25), 1000),
    "late": (dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, grad_scale=1.0), 200000),
    "lr0": (dict(lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, grad_scale=1.0), 1),
}
ADAMW_STEPS = 3


def adamw_inputs(n, device="cpu"):
    """(p, m, v, g) f32 [n]: p ~ N(0, 1), m ~ 0.01 N, v ~ 1e-4 N^2 + 1e-12, g ~ 0.02 N; g = 0 where i % 97 == 5 or i % 89 == 11,
    v = 1e-30 where i % 101 == 7 or i % 89 == 11 (the last: both at once, denom = eps)."""
    i = torch.arange(n, device=device)
    p = hash_real(n, 1, device).float()
    m = (0.01 * hash_real(n, 2, device)).float()
    v = (1e-4 * hash_real(n, 3, device) ** 2 + 1e-12).float()
    g = (0.02 * hash_real(n, 4, device)).float()
    g[(i % 97 == 5) | (i % 89 == 11)] = 0.0
    v[(i % 101 == 7) | (i % 89 == 11)] = 1e-30
    return p, m, v, g


def adamw_grad(g, s):
    """The gradient of trajectory step s (0, 1, 2): the same values rotated by s places with alternating sign -- the same 2-norm."""
    return torch.roll(g, s) * (-1.0 if s % 2 else 1.0)


def adamw_step64(p, m, v, g, hp, t):
    """One step of torch.optim.AdamW's formula in f64 at step count t, on the hyperparameters AS F32 VALUES (the entry points take
    ``float``): decoupled decay, denom = sqrt(v) / sqrt(bc2) + eps.  Returns ((p, m, v) after, (p, m, v) scales): the magnitude each
    element's error is measured against -- for m and v the larger of the element before and after (an element that cancels to near zero
    is held to the precision of its terms), for p the largest of |p| before, |p| after and the step (lr / bc1) max|m| / denom."""
    lr, b1, b2, eps, wd, gs = (f32r(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "grad_scale"))
    p0, m0, v0 = p.double(), m.double(), v.double()
    gi = g.double() * gs
    m1 = b1 * m0 + (1.0 - b1) * gi
    v1 = b2 * v0 + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    p1 = p0 * (1.0 - lr * wd) - (lr / bc1) * (m1 / denom)
    ms, vs = torch.maximum(m0.abs(), m1.abs()), torch.maximum(v0.abs(), v1.abs())
    ps = torch.maximum(torch.maximum(p0.abs(), p1.abs()), (lr / bc1) * ms / denom)
    return (p1, m1, v1), (ps, ms, vs)


def adamw64(p, m, v, grads, hp, step0):
    """The f64 trajectory from (p, m, v): [(p, m, v) after step s], the state before the first step in front."""
    out = [(p.double(), m.double(), v.double())]
    for s, g in enumerate(grads):
        out.append(adamw_step64(*out[-1], g, hp, step0 + s)[0])
    return out


def adamw_allowances(scales):
    """(p, m, v) allowances of one step from adamw_step64's scales: BAR ulps of the p scale, BAR relative to the m and v scales."""
    ps, ms, vs = scales
    return BAR["adamw_p_ulps"] * ulp32(ps), BAR["adamw_m_rel"] * ms, BAR["adamw_v_rel"] * vs


def clip_max_norm(g64_norm, coef=0.25):
    """An f32 ``max_norm`` for which bsclip_grad_clip_finish's coef = (float)min(1, max_norm / (norm + 1e-6)) is EXACTLY ``coef`` (a power
    of two) with a margin of 1e-9 relative for the order of the f64 sum, or None when no f32 lands in the window."""
    word = struct.unpack("I", struct.pack("f", coef * (g64_norm + 1e-6)))[0]
    for k in (0, 1, -1, 2, -2):
        mn = struct.unpack("f", struct.pack("I", word + k))[0]
        q = mn / (g64_norm + 1e-6)
        if coef * (1 - 2.0 ** -26) * (1 + 1e-9) < q < coef * (1 + 2.0 ** -25) * (1 - 1e-9):
            return mn
    return None


def clip_gradient(g, coef=0.25):
    """(g', max_norm): g with its largest element grown by j / 1024 of itself, j = 0, 1, ..., until ``clip_max_norm`` finds a max_norm (the
    window is about a third of the spacing of f32 around max_norm, so a few tries do; a buffer of ONE element, whose norm moves on the
    same lattice as max_norm, has to reach another binade first)."""
    g = g.clone()
    i = int(g.abs().argmax())
    top = g[i].item()
    for j in range(8192):
        g[i] = top * (1.0 + j / 1024.0)
        mn = clip_max_norm(float(g.double().pow(2).sum().sqrt().item()), coef)
        if mn is not None:
            return g, mn
    raise AssertionError("clip_gradient: no max_norm found")


# ---------------------------------------------------------------------------------------------------------------- count_nonfinite
def nonfinite_case(n, dtype, device="cpu"):
    """(t, count): ordinary values with +-inf / NaN at the first and last element, either side of the end of the first grid-stride pass and
    at every 1009th element."""
    t = hash_real(n, 51, device).to(dtype)
    i = torch.arange(n, device=device)
    bad = (i % 1009 == 3) | (i == 0) | (i == n - 1) | (i == NONFINITE_CAP - 1) | (i == NONFINITE_CAP) | (i == 2 * NONFINITE_CAP)
    if n == 63:
        bad[:] = False                                       # one case with nothing to count
    kinds = torch.tensor([float("inf"), float("-inf"), NAN], device=device).to(dtype)
    t[bad] = kinds[i[bad] % 3]
    want = int(bad.sum().item())
    assert want == int((~torch.isfinite(t.float())).sum().item())
    return t, want


# --------------------------------------------------------------------------------------------------------------------------- im2col
def im2col_image(B, device="cpu"):
    """[B, 3, 224, 224] f32: integers of 16 significant bits times 2^-8 (|x| < 128), so hi = 16-bit(x) and lo = x - hi are both exact
    in bf16 and in fp16 and [hi | lo] holds x without loss; neighbouring pixels differ."""
    n = B * 3 * 224 * 224
    x = hash_ints(n, -(1 << 15) + 1, (1 << 15) - 1, 61, device).double() / 256.0
    return x.float().view(B, 3, 224, 224)


def im2col_ref(img, split, dtype):
    """out[b * 196 + py * 14 + px, c * 256 + ky * 16 + kx] = img[b, c, 16 py + ky, 16 px + kx] (F.unfold's order), rounded to ``dtype``;
    ``split``: [hi | lo | hi] with lo = dtype(x - hi).  Asserts that the split loses nothing."""
    B = img.shape[0]
    cols = img.view(B, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(B * 196, 768)
    hi = cols.to(dtype)
    if not split:
        return hi
    lo = (cols - hi.float()).to(dtype)
    assert torch.equal(hi.double() + lo.double(), cols.double()), "im2col: hi + lo != x"
    return torch.cat([hi, lo, hi], 1)


# ------------------------------------------------------------------------------------------------------------------------ dgelu_mul
def dgelu_case(M, N, device="cpu"):
    """(g [M, N] bf16, codes [M, N] uint8 with every code value in row 0, want bf16): want = bf16(g * f32(code * step32 - off32)), the
    kernel's single fma decode restated exactly (tests/test_12_exact_kernels_gpu.py test_dgelu_mul)."""
    g = (hash_ints(M * N, -1024, 1024, 71, device).float() / 64).view(M, N).to(BF16)        # exact in bf16: 11 bits
    codes = hash_ints(M * N, 0, 255, 72, device).to(torch.uint8).view(M, N)
    codes[0, :256] = torch.arange(256, device=device).to(torch.uint8)
    step32 = (torch.tensor(1.26, dtype=F32) / 255).double().item()
    off32 = torch.tensor(0.13, dtype=F32).double().item()
    d32 = (codes.double() * step32 - off32).float()
    return g, codes, (g.float() * d32).to(BF16)


# ------------------------------------------------------------------------------------------------------------------ softmax pooling
def softmax_logits(B, S, scale, device="cpu"):
    """[B * S, 768] f32 logits ~ scale N(0, 1); row 0's maximum sits in the last lane's last column (767), row 1 (if any) has two
    equal maxima (columns 5 and 700)."""
    C = SOFTMAX_C
    x = (scale * hash_real(B * S * C, 81 + int(scale * 100), device)).float().view(B * S, C)
    x[0, C - 1] = x[0].max() + abs(scale)
    if B * S > 1:
        x[1, 5] = x[1, 700] = x[1].max() + abs(scale)
    return x


def softmax_pool64(logits, B, S):
    """(pooled [B, C], stats [B S, 2] = (row max, sum exp(x - max)), p [B S, C]) of softmax(dim=-1).mean(tokens) in f64."""
    x = logits.double()
    m = x.amax(1, keepdim=True)
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    p = e / s
    return p.view(B, S, -1).mean(1), torch.cat([m, s], 1), p


def softmax_pool_bwd64(logits, d_pooled, B, S):
    """(dlogits [B S, C], the per-row denominator): dlogits = p (g - p . g), g = d_pooled[b] / S; the denominator is
    max(max|dlogits|, 0.1 max|p g|) per row (tests/test_12_exact_kernels_gpu.py: a peaked row's gradient cancels to far below its terms
    p g, which f32 forms to 2^-24 and cannot do better)."""
    _, _, p = softmax_pool64(logits, B, S)
    g = d_pooled.double().repeat_interleave(S, 0) / S
    d = p * (g - (p * g).sum(1, keepdim=True))
    denom = torch.maximum(d.abs().amax(1, keepdim=True), 0.1 * (p * g).abs().amax(1, keepdim=True))
    return d, denom


def softmax_stats32(logits, B, S):
    """The statistics the backward is given in both files: the f64 reference's (max, sum) rounded to f32."""
    return softmax_pool64(logits, B, S)[1].float()


def softmax_d_pooled(B, device="cpu"):
    return hash_real(B * SOFTMAX_C, 82, device).float().view(B, SOFTMAX_C)


# -------------------------------------------------------------------------------------------------------------------- token means
def meanpool_fwd_input(B, S, H, device="cpu"):
    """[B S, H] f32 ~ N(0.5, 1): the mean rounds."""
    return (hash_real(B * S * H, 131 + S, device) + 0.5).float().view(B * S, H)


def meanpool_bwd_case(B, S, H, device="cpu"):
    """(d_pooled [B, H] integers in [-1000, 1000], want f32 [B S, H]): d * (1.0f / S) in f32 -- one IEEE answer -- on every token row."""
    d = hash_ints(B * H, -1000, 1000, 91 + S, device).float().view(B, H)
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(S), dtype=F32)
    want = (d * inv.to(device)).repeat_interleave(S, 0)
    assert (want.double() - (d.double() / S).repeat_interleave(S, 0)).abs().le(2 * ulp32(want.double())).all()
    return d, want


# ----------------------------------------------------------------------------------------------------------------------- bert_embed
def embed_case(B, S, H, kind, types, device="cpu"):
    """Inputs of bsclip_bert_embed: ``kind`` "exact" (integer tables, |word| <= 1000, |pos| <= 100, |type| <= 10) or "real"; ``types``
    False for type_ids = None.  ids cover 0, vocab - 1, -1 and vocab + 5 (the kernel clamps), type ids {0, 1, 2, -1} (the kernel takes
    tt ? 1 : 0); the position table has S + 3 rows, the type table a third row of NaN that must never be read."""
    V, M = EMBED_VOCAB, B * S
    ids = hash_ints(M, 0, V - 1, 101, device)
    edge = torch.tensor([V + 5, -1, 0, V - 1], device=device)
    ids[:min(M, 4)] = edge[:min(M, 4)]
    if M >= 8:
        ids[-4:] = edge
    tt = None
    if types:
        tt = torch.tensor([0, 1, 2, -1], device=device)[hash_ints(M, 0, 3, 102, device)]
        tt[:min(M, 4)] = torch.tensor([2, -1, 1, 0], device=device)[:min(M, 4)]
    if kind == "exact":
        word = hash_ints(V * H, -1000, 1000, 103, device).float().view(V, H)
        pos = hash_ints((S + 3) * H, -100, 100, 104, device).float().view(S + 3, H)
        typ = hash_ints(3 * H, -10, 10, 105, device).float().view(3, H)
    else:
        word = hash_real(V * H, 103, device).float().view(V, H)
        pos = (0.3 * hash_real((S + 3) * H, 104, device)).float().view(S + 3, H)
        typ = (0.1 * hash_real(3 * H, 105, device)).float().view(3, H)
    typ[2] = NAN
    return dict(ids=ids.view(B, S), type_ids=None if tt is None else tt.view(B, S), word=word, pos=pos, typ=typ)


def embed_ref(c, clamp=True):
    """(f64 sums, the f32 restatement (word + pos) + type): ids clamped to [0, vocab - 1], type row = tt ? 1 : 0.  ``clamp`` False: the
    ids wrap instead (what the comparison must reject)."""
    ids, word, pos, typ = c["ids"], c["word"], c["pos"], c["typ"]
    B, S = ids.shape
    V = word.shape[0]
    i = (ids.clamp(0, V - 1) if clamp else ids % V).reshape(-1)
    t = torch.arange(B * S, device=ids.device) % S
    ty = (c["type_ids"].reshape(-1) != 0).long() if c["type_ids"] is not None else torch.zeros_like(i)
    w, p, y = word[i], pos[t], typ[ty]
    return w.double() + p.double() + y.double(), (w + p) + y


# --------------------------------------------------------------------------------------------------------------------------- l2norm
L2_EPS = 1e-12


def l2norm_rows(M, D, device="cpu"):
    """(x, dy) f32 [M, D] and the row kinds: "zero" (all zero), "tiny" (norm ~ 1e-15: below the eps clamp), "big" (squares sum to
    ~ 1e30), "ord" (~ N(0, 1))."""
    kinds = {1: ["ord"], 3: ["zero", "tiny", "big"], 4: ["ord", "zero", "tiny", "big"], 5: ["ord", "zero", "tiny", "big", "ord"]}.get(M)
    if kinds is None:
        kinds = ["ord"] * M
        kinds[5], kinds[17], kinds[M - 1] = "zero", "tiny", "big"
    x = hash_real(M * D, 111, device).view(M, D)
    scale = torch.tensor([{"ord": 1.0, "zero": 0.0, "tiny": 1e-15 / math.sqrt(D), "big": 1e15 / math.sqrt(D)}[k] for k in kinds],
                         dtype=F64, device=device)
    return (x * scale[:, None]).float(), hash_real(M * D, 112, device).view(M, D).float(), kinds


def l2norm_fwd64(x):
    """(y, inv_norm) of F.normalize(p=2, dim=-1, eps=1e-12) in f64: y = x / max(||x||, eps)."""
    x = x.double()
    inv = 1.0 / x.norm(dim=1, keepdim=True).clamp_min(L2_EPS)
    return x * inv, inv[:, 0]


def l2norm_bwd64(y, inv_norm, dy):
    """The kernel's documented formula dx = inv (dy - y (y . dy)) in f64: F.normalize's autograd wherever ||x|| > eps, and on an all-zero
    row (dx = dy / eps); on a clamped non-zero row autograd lacks the y (y . dy) term, |y|^2 of the answer."""
    y, dy = y.double(), dy.double()
    return inv_norm.double()[:, None] * (dy - y * (y * dy).sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------------------------- the small movers
def mask_case(n, device="cpu"):
    mask = torch.tensor([0, 1, 2, -1], device=device)[hash_ints(n, 0, 3, 121, device)]
    mask[0] = 0 if n % 2 else 1
    return mask, torch.where(mask != 0, torch.zeros(n, dtype=F32, device=device), torch.full((n,), F32_MIN, dtype=F32, device=device))


def gather_ref(src, rows_out, p_in, p_out, off):
    """dst[r] = bf16(src[(r / p_out) * p_in + off + r % p_out]) (csrc/fullft.hip gather_cast_rows_kernel)."""
    r = torch.arange(rows_out, device=src.device)
    return src[(r // p_out) * p_in + off + r % p_out].to(BF16)


def gather_src_rows(rows_out, p_in, p_out, off):
    """The rows ops.gather_cast_rows wants of src, and the last row the kernel reads + 1 (they agree: asserted on the CPU)."""
    need = (rows_out + p_out - 1) // p_out * p_in - (p_in - off - p_out)
    r = rows_out - 1
    return need, (r // p_out) * p_in + off + r % p_out + 1


def words16(rows, cols, salt, dtype=BF16, device="cpu"):
    """[rows, cols] 16-bit words, finite and pairwise distinct along rows and columns (bits = a hash below 0x7000 with the index mixed in)."""
    n = rows * cols
    bits = (hash_ints(n, 0, 0x3FFF, salt, device) ^ (torch.arange(n, device=device) & 0x3FFF)) + 0x0400
    return bits.to(torch.int16).view(dtype).view(rows, cols)


def real16_table(rows, cols, salt, device="cpu"):
    """f32 [rows, cols] ~ N(0, 1) whose first row starts with the cast table's special values (as many as fit)."""
    t = hash_real(rows * cols, salt, device).float().view(rows, cols)
    sp = _f32_from_bits(list(CAST_SPECIAL_BITS)).to(device)
    k = min(cols, sp.numel())
    t[0, :k] = sp[:k]
    return t
