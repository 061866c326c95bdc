"""Inputs on which the row and column reductions behind every trainable gradient are exact, and their f64 values.

LayerNorm gradients (bsclip_layernorm_bwd, bsclip_ln_param_grad).  ``x`` holds integers in [-3, 3], ``mean`` an integer in [-1, 1] and
``rstd`` a power of two in {1/2, 1, 2} per row (the entry points take ``stats`` as an input, so a test supplies them), ``gamma``
non-zero integers in [-2, 2], ``g_gemm`` and ``g_resid`` integers in [-2, 2], ``dt`` and ``lora_a`` integers in [-1, 1]: all of them
exact in bf16 and fp16.  Then xhat = (x - mean) rstd is a multiple of 1/2 with |xhat| <= 8, dy = g_gemm + dt . A (+ g_resid) an
integer with |dy| <= 12, and dy gamma, dy xhat, dy gamma xhat multiples of 1/2 -- so

* d_gamma[c] = sum_r dy xhat and d_beta[c] = sum_r dy are sums of at most M terms of at most 192 half-units each: below 2^24 units
  for M <= 32 773 plus the accumulators' initial value, so NO order of f32 additions rounds, for either H;
* for H = 512 the two row means c1 = sum(dy gamma) / 512 and c2 = sum(dy gamma xhat) / 512 are exact dyadics (multiples of 2^-9 and
  2^-10), xhat c2 a multiple of 2^-11 below 2^11, and dx = (dy gamma - c1 - xhat c2) rstd (+ g_resid) a multiple of 2^-12 below
  2^12: every step of bsclip_layernorm_bwd is exact in f32, with or without fused multiply-adds, in any order of the row sums;
* for H = 768 the two divisions round (1 / 768 is no dyadic) and the result carries a few f32 ulps: that case has a bar.

LoRA gradients (bsclip_lora_grad, bsclip_lora_grad_f32): dq and dv odd integers in {-3, -1, 1, 3}, ``y`` in [-3, 3], ``t`` in [-2, 2],
``lora_b`` fifteen odd entries (+-1, +-3) per column and zeros elsewhere, so every dt is a sum of fifteen odd numbers -- never zero,
|dt| <= 135 -- and every dA / dB sum stays below 2^24 at M = 24 583 (135 * 3 * 24 583 = 9 956 115 at the very worst).
Column sums and embedding gradients: integers in [-3, 3].

Every reference method ASSERTS that the sum of the magnitudes of its terms, in units of the smallest step, stays below 2^24: the
condition under which an f32 accumulator cannot round whatever the order.  Accumulating outputs start from +-(1000 .. 1031), which no
sum of a few rows cancels; (mean, rstd) differs from each row to the next and rows are pairwise distinct, so a dropped, doubled or
swapped row changes the answer.  tests/test_04_row_exact_cpu.py proves these claims on the CPU.

Nothing here needs a GPU: every function computes on the device its tensors live on with plain torch f64 / integer ops."""
import torch

from gemm_exact import first_diff, strided, untouched  # noqa: F401  (the sentinel-buffer helpers, shared with the GEMM suites)

SEED = 15
NAN = float("nan")
EXACT_LIMIT = 2.0 ** 24

# Grid caps, read from the sources (no entry point reports them).  One wave takes one row per pass.
LN_CAP = 256 * 8 * 4            # csrc/norm.hip ln_grid(M, 8): 256 * 8 workgroups of LN_BLOCK / 64 = 4 waves
LN_CAP_LORA_FWD = 256 * 5 * 4   # bsclip_layernorm_fwd with lora_a: ln_grid(M, 5)
LN_CAP_LORA_BWD = 256 * 4 * 4   # bsclip_layernorm_bwd with lora_a: ln_grid(M, 4)
PG_ROWS_PER_BLOCK, PG_MAX_BLOCKS = 32, 1024     # csrc/fullft.hip bsclip_ln_param_grad: ceil(M / 32) slabs, at most 1024
LG_ROWS_PER_BLOCK, LG_MAX_BLOCKS = 32, 768      # csrc/optim.hip lora_blocks

# the cases of tests/test_15_row_reductions_gpu.py; tests/test_04_row_exact_cpu.py proves its claims over the same ones
HS = (512, 768)
LN_BWD_M = (1, 3, 4, 5, 1031, LN_CAP_LORA_BWD + 3, 2 * LN_CAP_LORA_BWD + 1, LN_CAP + 3, 2 * LN_CAP + 1)
LN_BWD_M_ALL_FORMS = (5, LN_CAP_LORA_BWD + 3, LN_CAP + 3)
LN_FWD_M = (1, 3, 5, LN_CAP_LORA_FWD + 3, 2 * LN_CAP_LORA_FWD + 1, LN_CAP + 3, 2 * LN_CAP + 1)
LN_REAL_M = (1031, LN_CAP_LORA_BWD + 3, LN_CAP + 3)
PGRAD_M = (1, 3, 31, 32, 33, 225, 257, 1000, 1057, 32773)         # 1, 1, 1, 1, 2, 8, 9, 32, 34 and 1024 (capped) slabs
LORA_M = (1, 2, 3, 7, 65, 2077, 24583)
LORA_F32_M = (1, 7, 24583)
COLSUM_WIDE_N, COLSUM_WIDE_M = (8, 768), (1, 255, 256, 257, 768, 769, 1023, 1024, 1025, 1793)
COLSUM_NARROW_N, COLSUM_NARROW_M = (1, 33, 36), (1, 8, 9, 24, 25, 32, 33, 333)
TRANSPOSE_R, TRANSPOSE_C = (1, 63, 64, 65, 130), (64, 200)
EMBED_BS = ((1, 1), (1, 63), (1, 64), (1, 65), (3, 43), (17, 1), (3, 2731))      # the last: rows_per_block = ceil(8193 / 512) = 17
EMBED_H = (4, 512, 768, 1024)
EMBED_VOCAB = 37

# bsclip_layernorm_bwd's forms: (name, x, g_resid, g_gemm, lora, mode, dx_res, operand, engine).  Dtypes by name, None = absent;
# operand "split3" = [hi | lo | hi] in bf16.  ``engine``: a form the encoder engines launch, run at every M of LN_BWD_M; the others
# run at LN_BWD_M_ALL_FORMS.  The fp16 forms exist for H = 768 only (the entry point rejects them at 512).
LN_BWD_FORMS = (
    ("m0-lora", "f32", "f32", "bf16", True, 0, "f32", "bf16", True),
    ("m1-lora", "f32", "f32", "bf16", True, 1, "f32", "bf16", True),
    ("m0", "f32", "f32", "bf16", False, 0, "f32", "bf16", True),
    ("m1", "f32", "f32", "bf16", False, 1, "f32", "bf16", False),
    ("top", "f32", None, "bf16", False, 0, "f32", "bf16", True),
    ("resid-only", "f32", "f32", None, False, 1, "f32", "bf16", False),
    ("stream16-m0-lora", "bf16", "bf16", "bf16", True, 0, "bf16", "bf16", True),
    ("stream16-m0-lora-operand-only", "bf16", "bf16", "bf16", True, 0, None, "bf16", True),
    ("stream16-m1", "bf16", "bf16", "bf16", False, 1, "bf16", None, False),
    ("stream16-in-f32-out", "f32", "bf16", "bf16", True, 1, "f32", "bf16", False),
    ("stream-f32-in-16-out", "bf16", "f32", "bf16", False, 0, "bf16", "bf16", False),
    ("exact-f32-operand", "f32", "f32", "f32", True, 0, "f32", "f32", False),
    ("exact-split3-m0", "f32", "f32", "f32", False, 0, "f32", "split3", True),
    ("exact-split3-m1-lora", "f32", "f32", "f32", True, 1, "f32", "split3", False),
    ("exact-top", "f32", None, "f32", False, 0, "f32", None, True),
    ("fp16-m0-lora", "fp16", "fp16", "fp16", True, 0, "fp16", "fp16", True),
    ("fp16-m0-lora-operand-only", "fp16", "fp16", "fp16", True, 0, None, "fp16", True),
    ("fp16-m1", "fp16", "fp16", "fp16", False, 1, "fp16", "fp16", False),
    ("fp16-top", "fp16", None, "fp16", False, 0, None, "fp16", True),
)
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "split3": torch.bfloat16}


def ln_bwd_forms(H, M):
    """The forms of LN_BWD_FORMS that run at (H, M)."""
    return [f for f in LN_BWD_FORMS if (H == 768 or f[1] != "fp16") and (f[8] or M in LN_BWD_M_ALL_FORMS)]


# bsclip_ln_param_grad's forms: (x, mode, lora); g_gemm (bf16) and g_resid (f32) always given -- mode 0 must ignore g_resid
PGRAD_FORMS = tuple((x, mode, lora) for x in ("f32", "bf16") for mode in (0, 1) for lora in (False, True))
# bsclip_layernorm_fwd's instantiations outside fp8: (x, operand); each with and without lora_a
LN_FWD_FORMS = (("f32", "bf16"), ("bf16", "bf16"), ("f32", "fp16"), ("fp16", "fp16"), ("f32", "split3"), ("bf16", "split3"))

# bars (each from the number formats or from a test the suite already has, never from what a kernel gave)
BAR_LN_BWD = 5e-5                 # tests/test_10_kernels_gpu.py test_layernorm_fwd_bwd, there on the whole tensor, here per row
BAR_LN_FWD = 2e-5                 # test_10's TOL_F32
BAR_T = 4e-3                      # test_10's TOL_BF16
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def bar_16bit(dtype):
    """Per-row bar of a 16-bit output that has no f32 twin in the same call: one rounding of every element (the row's 2-norm moves by at
    most the unit roundoff) on top of the f32 bar."""
    return UNIT_ROUNDOFF[dtype] + BAR_LN_BWD


def offset_bar(base, ratio):
    """tests/test_12_exact_kernels_gpu.py's allowance for rows whose |mean| is ``ratio`` times their standard deviation: the f32 mean
    carries a few ulps of the offset into every output."""
    return base + 2.0 ** -21 * ratio


def _gen(*key):
    seed = SEED
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 62))


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _nonzero_ints(shape, hi, g):
    return (torch.randint(1, hi + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def _odd_ints(shape, g):   # -3, -1, 1, 3
    return (2 * torch.randint(0, 4, shape, generator=g) - 3).float()


def accumulator(shape, g):
    """What an accumulating output holds before the call: +-(1000 .. 1031)."""
    return (torch.randint(1000, 1032, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def _exact(terms_abs_sum, unit, what):
    top = terms_abs_sum.max().item() / unit
    assert top < EXACT_LIMIT, f"{what}: sum |terms| = {top} units of {unit}, not below 2^24"
    return top


def row_err(got, want):
    """max over rows of ||got - want||_2 / ||want||_2; a NaN (an element never written) counts as infinite."""
    got, want = got.double(), want.double()
    e = (got - want).norm(dim=1) / want.norm(dim=1).clamp_min(1e-30)
    return torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e).max().item()


def padded(t, pad, dtype=None):
    """``t`` [M, N] as the [:M, :N] view of a NaN-filled [M + 3, N + pad] buffer: an input with a leading dimension of its own."""
    dtype = dtype or t.dtype
    buf = torch.full((t.shape[0] + 3, t.shape[1] + pad), NAN, dtype=dtype, device=t.device)
    buf[:t.shape[0], :t.shape[1]] = t.to(dtype)
    return buf[:t.shape[0], :t.shape[1]]


def split3(v):
    """(hi, lo) of the split-bf16 operand of an f32 tensor: hi = bf16(v), lo = bf16(v - hi)."""
    hi = v.bfloat16()
    return hi, (v - hi.float()).bfloat16()


def nonzero_share(t):
    return (t != 0).double().mean().item()


# ------------------------------------------------------------------------------------------------------- LayerNorm gradients
class LnCase:
    """Exact inputs of bsclip_layernorm_bwd / bsclip_ln_param_grad for M rows of H columns, f32 tensors on ``device``."""

    def __init__(self, M, H, device="cpu"):
        g = _gen(1, M, H)
        self.M, self.H = M, H
        x = _ints((M, H), -3, 3, g)
        pair = torch.cumsum(torch.randint(1, 9, (M,), generator=g), 0) % 9          # never the same pair twice in a row
        mean, rstd = (pair // 3 - 1).float(), 2.0 ** (pair % 3 - 1).float()
        t = dict(x=x, stats=torch.stack([mean, rstd], 1).contiguous(), gamma=_nonzero_ints((H,), 2, g),
                 g_gemm=_ints((M, H), -2, 2, g), g_resid=_ints((M, H), -2, 2, g), dt=_ints((M, 8), -1, 1, g),
                 lora_a=_ints((8, H), -1, 1, g), dg0=accumulator((H,), g), db0=accumulator((H,), g))
        for k, v in t.items():
            setattr(self, k, v.to(device))

    def xhat(self):
        return (self.x.double() - self.stats[:, :1].double()) * self.stats[:, 1:].double()

    def dy(self, gg, lora, mode, gr):
        """The gradient at the LayerNorm's output as both kernels assemble it (f64): which terms exist, and the mode."""
        d = torch.zeros(self.M, self.H, dtype=torch.float64, device=self.x.device)
        if gg:
            d += self.g_gemm.double()
        if lora:
            d += self.dt.double() @ self.lora_a.double()
        if mode == 1 and gr:
            d += self.g_resid.double()
        return d

    def dx(self, gg=True, lora=True, mode=0, gr=True):
        """bsclip_layernorm_bwd's result in f64; for H = 512 asserted to be exactly what f32 arithmetic gives in any order."""
        H, xhat, rstd = self.H, self.xhat(), self.stats[:, 1:].double()
        dyg = self.dy(gg, lora, mode, gr) * self.gamma.double()
        c1, c2 = dyg.sum(1, keepdim=True) / H, (dyg * xhat).sum(1, keepdim=True) / H
        inner = dyg - c1 - xhat * c2
        d = inner * rstd
        if mode == 0 and gr:
            d = d + self.g_resid.double()
        _exact(dyg.abs().sum(1), 1.0, "layernorm_bwd c1")
        _exact((dyg * xhat).abs().sum(1), 0.5, "layernorm_bwd c2")
        if H == 512:
            _exact((xhat * c2).abs(), 2.0 ** -11, "layernorm_bwd xhat c2")
            _exact(inner.abs() + (dyg - c1).abs(), 2.0 ** -11, "layernorm_bwd dy gamma - c1 - xhat c2")
            _exact(d.abs() + inner.abs() * rstd, 2.0 ** -12, "layernorm_bwd dx")
            assert torch.equal(d.float().double(), d)
        return d

    def pgrad(self, gg=True, lora=True, mode=1, gr=True, calls=1):
        """(d_gamma, d_beta) after ``calls`` calls of bsclip_ln_param_grad on accumulators that held (dg0, db0): f64, exact in f32."""
        dy, xhat = self.dy(gg, lora, mode, gr), self.xhat()
        _exact(calls * (dy * xhat).abs().sum(0) + self.dg0.double().abs(), 0.5, "ln_param_grad d_gamma")
        _exact(calls * dy.abs().sum(0) + self.db0.double().abs(), 1.0, "ln_param_grad d_beta")
        return self.dg0.double() + calls * (dy * xhat).sum(0), self.db0.double() + calls * dy.sum(0)


def real_ln_inputs(M, H, offset, device="cpu"):
    """Real-valued rows for the toleranced LayerNorm comparisons: x ~ 2 N(0, 1) + 0.3, or -- ``offset`` -- N(0, 1) + 32 .. 64 (rows
    whose mean is 32 to 64 times their standard deviation), gamma ~ 1 + 0.1 N, beta ~ 0.1 N, A ~ 0.05 N, upstream gradients ~ N(0, 1)
    (g_gemm rounded to bf16, which fp16 users round again)."""
    g = _gen(2, M, H, int(offset))
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = n(M, H) + 32.0 * (1 + torch.rand(M, 1, generator=g)) if offset else n(M, H) * 2 + 0.3
    t = dict(x=x, gamma=1 + 0.1 * n(H), beta=0.1 * n(H), lora_a=0.05 * n(8, H), g_resid=n(M, H), g_gemm=n(M, H).bfloat16().float(),
             dt=n(M, 8))
    return {k: v.to(device) for k, v in t.items()}


def ln_fwd64(x, gamma, beta, eps):
    """(y, mean, rstd) of LayerNorm in f64."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    rstd = (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    return (x - mean) * rstd * gamma.double() + beta.double(), mean[:, 0], rstd[:, 0]


def ln_bwd64(x, gamma, eps, dy, res, mode):
    """bsclip_layernorm_bwd in f64 from x itself (its own statistics): dy is the assembled output gradient WITHOUT the residual."""
    x, g = x.double(), gamma.double()
    H = x.shape[1]
    mean = x.mean(1, keepdim=True)
    rstd = (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    xhat = (x - mean) * rstd
    dy = dy.double() + (res.double() if mode == 1 else 0)
    dyg = dy * g
    d = (dyg - dyg.sum(1, keepdim=True) / H - xhat * ((dyg * xhat).sum(1, keepdim=True) / H)) * rstd
    return d + (res.double() if mode == 0 else 0)


def mean_over_std(x):
    x = x.double()
    return (x.mean(1).abs() / x.std(1, unbiased=False)).max().item()


# ------------------------------------------------------------------------------------------------------------ LoRA gradients
class LoraCase:
    """Exact inputs of bsclip_lora_grad (bf16 rows: h_aug = [y | t]) and bsclip_lora_grad_f32 (t = y A^T rebuilt by the kernel)."""

    def __init__(self, M, H, device="cpu"):
        g = _gen(3, M, H)
        self.M, self.H = M, H
        lora_b = torch.zeros(2, H, 4)
        for half in range(2):
            for j in range(4):
                rows = torch.randperm(H, generator=g)[:15]
                lora_b[half, rows, j] = _odd_ints((15,), g)
        dqkv = _ints((M, 3 * H), -2, 2, g)                     # the k third, which no LoRA gradient reads
        dqkv[:, :H], dqkv[:, 2 * H:] = _odd_ints((M, H), g), _odd_ints((M, H), g)
        t = dict(dqkv=dqkv, y=_ints((M, H), -3, 3, g), t=_ints((M, 8), -2, 2, g), lora_b=lora_b,
                 lora_a=_ints((8, H), -1, 1, g), dA0=accumulator((8, H), g), dBq0=accumulator((H, 4), g), dBv0=accumulator((H, 4), g))
        for k, v in t.items():
            setattr(self, k, v.to(device))

    def grads(self, calls=1, f32_form=False):
        """(dt [M, 8], dA [8, H], dBq [H, 4], dBv [H, 4]) in f64 after ``calls`` calls.  ``f32_form``: t = y A^T."""
        H = self.H
        dq, dv, y = self.dqkv[:, :H].double(), self.dqkv[:, 2 * H:].double(), self.y.double()
        t = y @ self.lora_a.double().t() if f32_form else self.t.double()
        lb = self.lora_b.double()
        dt = torch.cat([dq @ lb[0], dv @ lb[1]], 1)
        _exact(torch.cat([dq.abs() @ lb[0].abs(), dv.abs() @ lb[1].abs()], 1), 1.0, "lora_grad dt")
        _exact(y.abs() @ self.lora_a.double().abs().t(), 1.0, "lora_grad_f32 t")
        _exact(calls * (dt.abs().t() @ y.abs()) + self.dA0.double().abs(), 1.0, "lora_grad dA")
        _exact(calls * (dq.abs().t() @ t[:, :4].abs()) + self.dBq0.double().abs(), 1.0, "lora_grad dBq")
        _exact(calls * (dv.abs().t() @ t[:, 4:].abs()) + self.dBv0.double().abs(), 1.0, "lora_grad dBv")
        return (dt, self.dA0.double() + calls * (dt.t() @ y), self.dBq0.double() + calls * (dq.t() @ t[:, :4]),
                self.dBv0.double() + calls * (dv.t() @ t[:, 4:]))


# -------------------------------------------------------------------------------------------- column sums, embedding gradients
def colsum_case(M, N, device="cpu"):
    """(g [M, N] integers in [-3, 3], out0 [N], f64 out0 + column sums)."""
    gen = _gen(4, M, N)
    g, out0 = _ints((M, N), -3, 3, gen), accumulator((N,), gen)
    _exact(g.abs().sum(0) + out0.abs(), 1.0, "colsum")
    return g.to(device), out0.to(device), (out0.double() + g.double().sum(0)).to(device)


def embed_case(B, S, H, variant, device="cpu"):
    """Inputs and f64 autograd result of bsclip_embed_grad on a vocabulary of EMBED_VOCAB rows with pad id 0.  ``variant``: "random"
    (ids in [-2, vocab + 1]: the kernel clamps them as the forward lookup does), "same" (every token holds id 5), each with "+types"
    for token-type ids.  Returns a dict: ids, type_ids (or None), d, the three initial tables and their expected f64 values; the pad
    row of the word table and the position rows >= S hold NaN before and after."""
    gen = _gen(5, B, S, H, len(variant))
    V, M = EMBED_VOCAB, B * S
    ids = torch.full((B, S), 5, dtype=torch.int64) if variant.startswith("same") else torch.randint(-2, V + 2, (B, S), generator=gen)
    if not variant.startswith("same") and M >= 3:
        ids.view(-1)[1], ids.view(-1)[2] = -2, V + 1               # below 0 and past the vocabulary, whatever the draw
    tt = torch.randint(0, 2, (B, S), generator=gen) if variant.endswith("+types") else None
    d = _ints((M, H), -3, 3, gen)
    word0, pos0, typ0 = accumulator((V, H), gen), accumulator((S + 3, H), gen), accumulator((2, H), gen)
    clamped = ids.clamp(0, V - 1)
    word = torch.zeros(V, H, dtype=torch.float64, requires_grad=True)
    pos = torch.zeros(S, H, dtype=torch.float64, requires_grad=True)
    typ = torch.zeros(2, H, dtype=torch.float64, requires_grad=True)
    e = torch.nn.functional.embedding(clamped, word, padding_idx=0) + pos[None] + \
        torch.nn.functional.embedding(tt if tt is not None else torch.zeros_like(ids), typ)
    (e.reshape(M, H) * d.double()).sum().backward()
    _exact(d.abs().sum(0) + 1031, 1.0, "embed_grad")        # every table entry sums a subset of the rows of d
    want_word, want_pos, want_typ = word0.double() + word.grad, pos0.double(), typ0.double() + typ.grad
    want_pos[:S] += pos.grad
    for tbl in (word0, want_word):
        tbl[0] = NAN
    for tbl in (pos0, want_pos):
        tbl[S:] = NAN
    out = dict(ids=ids, type_ids=tt, d=d, word0=word0, pos0=pos0, typ0=typ0, want_word=want_word, want_pos=want_pos, want_typ=want_typ)
    return {k: (v.to(device) if v is not None else None) for k, v in out.items()}


def same(got, want):
    """Bit equality of an f32 result with an f64 expectation, NaN sentinels matching NaN."""
    return torch.equal(torch.nan_to_num(got.double(), nan=-7e77), torch.nan_to_num(want.double(), nan=-7e77))
