"""The claims tests/test_15_row_reductions_gpu.py rests on, proven without a GPU (tests/row_exact.py holds the inputs, cases and bars):

* the inputs survive bf16 and fp16 unchanged and the sums of the magnitudes of every reduction's terms stay below 2^24 units for every
  case and row count the GPU file uses -- so it may ask for bit equality with f64;
* each kernel's arithmetic restated in torch f32 WITH its decomposition (rows per wave, the butterfly over the 64 lanes, wave order
  into LDS, slab order, the grouped slab reducers) equals f64 bit for bit, and so does the same sum in a random order;
* expected outputs are non-degenerate, and each of six mutations of a restatement -- a row skipped, a row taken twice, the last slab
  dropped, (mean, rstd) of two rows swapped, a 4-column lane piece stored 256 columns off, a truncating 16-bit conversion -- changes
  at least one element;
* for the toleranced comparisons (H = 768 on exact inputs, real-valued rows, the forward) the f32 restatement stays below HALF of each
  bar on the very inputs the GPU test uses; the share of every bar is printed as a ``FIGURES {json}`` line."""
import json

import pytest
import torch

import row_exact as rx

F32 = torch.float32


def _log(test, **figures):
    print("FIGURES " + json.dumps({"test": test, **figures}))


# ------------------------------------------------------------------------------------------ f32 restatements of the kernels
def wave_sum_f32(v):
    """Row sums of v [M, H] (f32) as the LayerNorm kernels form them: lane l holds columns 256 j + 4 l .. + 3 and adds
    (a + b) + (c + d) per j, then the xor butterfly over the 64 lanes (csrc/common.h wave_sum).  Returns [M, 1]."""
    M, H = v.shape
    p = v.reshape(M, H // 256, 64, 4)
    s = torch.zeros(M, 64, dtype=F32)
    for j in range(H // 256):
        s = s + ((p[:, j, :, 0] + p[:, j, :, 1]) + (p[:, j, :, 2] + p[:, j, :, 3]))
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, :1]


def assemble_dy_f32(gg, dt, lora_a, res, mode):
    """dy as layernorm_bwd_kernel assembles it: g_gemm, + dt . A in two groups of four ranks, + the residual gradient in mode 1."""
    dy = gg.clone() if gg is not None else torch.zeros_like(res)
    if dt is not None:
        for r0 in (0, 4):
            dy = dy + (((dt[:, r0:r0 + 1] * lora_a[r0] + dt[:, r0 + 1:r0 + 2] * lora_a[r0 + 1]) + dt[:, r0 + 2:r0 + 3] * lora_a[r0 + 2])
                       + dt[:, r0 + 3:r0 + 4] * lora_a[r0 + 3])
    if mode == 1 and res is not None:
        dy = dy + res
    return dy


def ln_bwd_f32(x, stats, gamma, dy, res, mode, rowsum=wave_sum_f32):
    """layernorm_bwd_kernel from the assembled dy on, statement by statement in f32 (no fused multiply-adds)."""
    H = x.shape[1]
    inv_h = torch.tensor(1.0 / H, dtype=F32)
    mean, rstd = stats[:, :1], stats[:, 1:]
    xhat = (x - mean) * rstd
    dyg = dy * gamma
    c1, c2 = rowsum(dyg) * inv_h, rowsum(dyg * xhat) * inv_h
    d = (dyg - c1 - xhat * c2) * rstd
    return d + res if (mode == 0 and res is not None) else d


def ln_fwd_f32(x, gamma, beta, eps, lora_a=None):
    """layernorm_fwd_kernel in f32: (y, stats [M, 2], t [M, 8] or None)."""
    H = x.shape[1]
    inv_h = torch.tensor(1.0 / H, dtype=F32)
    mean = wave_sum_f32(x) * inv_h
    v = x - mean
    rstd = torch.rsqrt(wave_sum_f32(v * v) * inv_h + torch.tensor(eps, dtype=F32))
    y = v * rstd * gamma + beta
    t = None
    if lora_a is not None:
        t = torch.cat([wave_sum_f32(y * lora_a[r]) for r in range(8)], 1)
    return y, torch.cat([mean, rstd], 1), t


def strided_reduce_f32(terms, nacc, per_block, groups, weights=None, drop_last_slab=False):
    """sum over rows of terms [M, W] (f32) in the decomposition the slab kernels share: accumulator a of ``nacc`` adds rows a, a + nacc,
    ... in order; ``per_block`` consecutive accumulators are added in order into one slab; thread group g of ``groups`` adds slabs g,
    g + groups, ... in order and the group sums are added g = 0, 1, ...  ``weights`` [M]: 0 skips a row, 2 takes it twice."""
    M, W = terms.shape
    if weights is not None:
        terms = terms * weights[:, None]
    iters = -(-M // nacc)
    t = torch.zeros(iters * nacc, W, dtype=F32)
    t[:M] = terms
    t = t.reshape(iters, nacc, W)
    acc = torch.zeros(nacc, W, dtype=F32)
    for i in range(iters):
        acc = acc + t[i]
    acc = acc.reshape(nacc // per_block, per_block, W)
    slabs = torch.zeros(nacc // per_block, W, dtype=F32)
    for w in range(per_block):
        slabs = slabs + acc[:, w]
    return slab_reduce_f32(slabs[:-1] if drop_last_slab else slabs, groups)


def slab_reduce_f32(slabs, groups):
    """slab_reduce_add_kernel (8 groups) / lora_grad_reduce_kernel (32): group g adds slabs g, g + groups, ... in order, then the group
    sums are added g = 0, 1, ..."""
    n, W = slabs.shape
    steps = -(-n // groups)
    s = torch.zeros(steps * groups, W, dtype=F32)
    s[:n] = slabs
    s = s.reshape(steps, groups, W)
    part = torch.zeros(groups, W, dtype=F32)
    for i in range(steps):
        part = part + s[i]
    total = torch.zeros(W, dtype=F32)
    for g in range(groups):
        total = total + part[g]
    return total


def embed_grad_f32(e, B, S, H):
    """bsclip_embed_grad: position rows summed over the batch in order; word row v from the tokens that hold v (ids clamped) in token
    order, the pad row 0 skipped; type rows from per-workgroup slabs over max(16, ceil(M / 512)) consecutive rows, through the slab
    reducer.  Rows that hold NaN (which the kernel must not touch) are left alone."""
    V, M = rx.EMBED_VOCAB, B * S
    ids = e["ids"].reshape(-1).clamp(0, V - 1)
    tt = e["type_ids"].reshape(-1) if e["type_ids"] is not None else torch.zeros(M, dtype=torch.int64)
    d = e["d"]
    pos, word, typ = e["pos0"].clone(), e["word0"].clone(), e["typ0"].clone()
    acc = torch.zeros(S, H, dtype=F32)
    for b in range(B):
        acc = acc + d[b * S:(b + 1) * S]
    pos[:S] = pos[:S] + acc
    for v in range(1, V):
        rows = (ids == v).nonzero().reshape(-1).tolist()
        acc = torch.zeros(H, dtype=F32)
        for r in rows:
            acc = acc + d[r]
        if rows:
            word[v] = word[v] + acc
    rpb = max(16, -(-M // 512))
    blocks = -(-M // rpb)
    slabs = torch.zeros(blocks, 2 * H, dtype=F32)
    for blk in range(blocks):
        for r in range(blk * rpb, min(M, (blk + 1) * rpb)):
            lo = H if tt[r] != 0 else 0
            slabs[blk, lo:lo + H] = slabs[blk, lo:lo + H] + d[r]
    return word, pos, typ + slab_reduce_f32(slabs, 8).reshape(2, H)


def pgrad_blocks(M):
    return min(-(-M // rx.PG_ROWS_PER_BLOCK), rx.PG_MAX_BLOCKS)


def lora_blocks(M):
    return max(1, min(-(-M // rx.LG_ROWS_PER_BLOCK), rx.LG_MAX_BLOCKS))


def pgrad_f32(c, lora, mode, weights=None, drop_last_slab=False, stats=None):
    """ln_pgrad_kernel + slab_reduce_add_kernel: 4 waves per workgroup, wave w of the grid takes rows w, w + nwaves, ..."""
    stats = c.stats if stats is None else stats
    dy = c.g_gemm.clone()
    if lora:
        for r in range(8):
            dy = dy + c.dt[:, r:r + 1] * c.lora_a[r]
    if mode == 1:
        dy = dy + c.g_resid
    xhat = (c.x - stats[:, :1]) * stats[:, 1:]
    terms = torch.cat([dy * xhat, dy], 1)
    blocks = pgrad_blocks(c.M)
    tot = strided_reduce_f32(terms, 4 * blocks, 4, 8, weights, drop_last_slab and blocks > 1)
    return c.dg0 + tot[:c.H], c.db0 + tot[c.H:]


def lora_grad_f32(c, weights=None, drop_last_slab=False, t=None):
    """bsclip_lora_grad on bf16 rows: dt per row; dB from wave PAIRS (2 per workgroup), dA from 4 waves per workgroup, both through
    lora_grad_reduce_kernel's 32 slab groups."""
    H, M = c.H, c.M
    t = c.t if t is None else t
    dq, dv = c.dqkv[:, :H], c.dqkv[:, 2 * H:]
    dt = torch.cat([dq @ c.lora_b[0], dv @ c.lora_b[1]], 1)
    blocks = lora_blocks(M)
    drop = drop_last_slab and blocks > 1
    db_terms = torch.cat([(dq[:, :, None] * t[:, None, :4]).reshape(M, 4 * H), (dv[:, :, None] * t[:, None, 4:]).reshape(M, 4 * H)], 1)
    db = strided_reduce_f32(db_terms, 2 * blocks, 2, 32, weights, drop)
    da = strided_reduce_f32((dt[:, :, None] * c.y[:, None, :]).reshape(M, 8 * H), 4 * blocks, 4, 32, weights, drop)
    return dt, c.dA0 + da.reshape(8, H), c.dBq0 + db[:4 * H].reshape(H, 4), c.dBv0 + db[4 * H:].reshape(H, 4)


def colsum_f32(g, out0, wide, weights=None):
    """colsum8_kernel (thread t adds rows t, t + 256, ...; 8 octets of 32 partials in order; the octets in order) or colsum_kernel (8 row
    groups, four unrolled accumulators each, folded pairwise, the groups in order)."""
    if wide:
        return out0 + strided_reduce_f32(g, 256, 32, 1, weights)
    if weights is not None:
        g = g * weights[:, None]
    M, N = g.shape
    part = torch.zeros(8, N, dtype=F32)
    for rg in range(8):
        s = [torch.zeros(N, dtype=F32) for _ in range(4)]
        r = rg
        while r + 24 < M:
            for u in range(4):
                s[u] = s[u] + g[r + 8 * u]
            r += 32
        while r < M:
            s[0] = s[0] + g[r]
            r += 8
        part[rg] = (s[0] + s[1]) + (s[2] + s[3])
    tot = torch.zeros(N, dtype=F32)
    for k in range(8):
        tot = tot + part[k]
    return out0 + tot


def one_rne(v64, dtype):
    return v64.float().to(dtype)


def truncated(v32, dtype):
    """v32 chopped (not rounded) to ``dtype``: the 16-bit value nearest to zero-wards."""
    r = v32.to(dtype)
    too_big = r.float().abs() > v32.abs()
    bits = r.view(torch.int16)
    return torch.where(too_big, bits - 1, bits).view(dtype)


def _distinct_dy(H, M):
    """(g_gemm?, lora?, mode, g_resid?) of the forms that run at (H, M), each once: what the values depend on (the formats hold the
    same integers)."""
    return sorted({(f[3] is not None, f[4], f[5], f[2] is not None) for f in rx.ln_bwd_forms(H, M)})


# --------------------------------------------------------------------------------------------------------- inputs and bounds
def test_inputs_survive_both_16_bit_formats():
    c, l = rx.LnCase(33, 512), rx.LoraCase(33, 512)
    for v in (c.x, c.g_gemm, c.g_resid, c.dt, c.lora_a, c.gamma, l.dqkv, l.y, l.t, l.lora_b, l.lora_a):
        d = v.double()
        assert torch.equal(d.to(torch.bfloat16).double(), d) and torch.equal(d.to(torch.float16).double(), d)
        assert torch.equal(d, d.round())
    assert set(c.stats[:, 1].tolist()) <= {0.5, 1.0, 2.0} and set(c.stats[:, 0].tolist()) <= {-1.0, 0.0, 1.0}
    assert c.x.abs().max() == 3 and c.gamma.abs().min() == 1 and c.gamma.abs().max() == 2
    assert (l.lora_b != 0).sum(1).eq(15).all() and l.dqkv[:, :512].abs().min() == 1


def test_worst_case_term_sums_stay_below_2_to_the_24():
    """A priori, whatever the random draw: the largest row counts against the largest possible terms."""
    assert max(rx.PGRAD_M) * 12 * 8 * 2 + 2 * 1031 < 2 ** 24                  # d_gamma in half-units: |dy| <= 12, |xhat| <= 8
    assert 2 * max(rx.LORA_M) * 135 * 3 + 1031 < 2 ** 25 and max(rx.LORA_M) * 135 * 3 + 1031 < 2 ** 24   # dA, one call
    assert 768 * 24 * 8 * 2 < 2 ** 24 and 8 * 192 * 2 ** 11 + 48 * 2 ** 11 < 2 ** 24      # c2 in half-units; xhat c2 in 2^-11
    assert max(rx.COLSUM_WIDE_M + rx.COLSUM_NARROW_M) * 3 + 1031 < 2 ** 24 and max(b * s for b, s in rx.EMBED_BS) * 3 + 1031 < 2 ** 24


@pytest.mark.parametrize("H", rx.HS)
def test_term_sums_of_every_case_stay_below_2_to_the_24(H):
    """The realised sums (each reference method asserts its own), for every M and every distinct dy the GPU file runs; the LoRA sums
    for TWO calls, which the GPU file's doubling check needs."""
    for M in rx.LN_BWD_M:       # (bsclip_ln_param_grad's sums: asserted where its restatement is compared, for every M and form)
        c = rx.LnCase(M, H)
        for gg, lora, mode, gr in _distinct_dy(H, M):
            c.dx(gg, lora, mode, gr)
    for M in rx.LORA_M:
        c = rx.LoraCase(M, H)
        c.grads(calls=2)
        if M in rx.LORA_F32_M:
            c.grads(calls=2, f32_form=True)


def test_colsum_transpose_and_embed_term_sums_and_restatements():
    for N, Ms in ((rx.COLSUM_WIDE_N, rx.COLSUM_WIDE_M), (rx.COLSUM_NARROW_N, rx.COLSUM_NARROW_M)):
        for n in N:
            for M in Ms:
                rx.colsum_case(M, n)
    for R in rx.TRANSPOSE_R:          # bsclip_transpose_colsum_bf16's inputs
        for C in rx.TRANSPOSE_C:
            g, out0, want = rx.colsum_case(R, C)
            slabs = torch.stack([g[r0:r0 + 64].sum(0) for r0 in range(0, R, 64)])       # one slab per 64 source rows
            assert torch.equal((out0 + slab_reduce_f32(slabs, 8)).double(), want)
    for B, S in rx.EMBED_BS:
        for variant in ("random", "random+types", "same", "same+types"):
            e = rx.embed_case(B, S, 4, variant)
            assert e["ids"].min() >= -2 and e["ids"].max() <= rx.EMBED_VOCAB + 1
            assert variant.startswith("same") or B * S < 3 or (e["ids"].min() < 0 and e["ids"].max() >= rx.EMBED_VOCAB)
            for got, k in zip(embed_grad_f32(e, B, S, 4), ("want_word", "want_pos", "want_typ")):
                assert rx.same(got, e[k]), (B, S, variant, k)


# -------------------------------------------------------------------------------------------------------- non-degeneracy
def _distinct_rows(t):
    probe = torch.rand(t.shape[1], generator=torch.Generator().manual_seed(1), dtype=torch.float64)     # a hash of each row
    return torch.unique(t.double() @ probe).numel() == t.shape[0]


@pytest.mark.parametrize("H", rx.HS)
def test_expected_outputs_are_non_degenerate(H):
    shares = {}
    for M in (1, 5, 1031, rx.LN_CAP + 3):
        c = rx.LnCase(M, H)
        assert _distinct_rows(c.x) and _distinct_rows(c.g_gemm) and _distinct_rows(torch.cat([c.x, c.stats], 1))
        assert (c.stats[1:] != c.stats[:-1]).any(1).all(), "(mean, rstd) repeats from one row to the next"
        for f in rx.ln_bwd_forms(H, 5):
            d = c.dx(f[3] is not None, f[4], f[5], f[2] is not None)
            shares[f"dx {f[0]} M={M}"] = rx.nonzero_share(d)
            assert _distinct_rows(d)
    for M in rx.PGRAD_M:
        c = rx.LnCase(M, H)
        for mode in (0, 1):
            for lora in (False, True):
                dg, db = c.pgrad(True, lora, mode, True)
                shares[f"d_gamma M={M} mode {mode} lora {lora}"], shares[f"d_beta M={M} mode {mode} lora {lora}"] = \
                    rx.nonzero_share(dg), rx.nonzero_share(db)
    for M in rx.LORA_M:
        c = rx.LoraCase(M, H)
        assert _distinct_rows(c.dqkv) and _distinct_rows(c.y)       # t has 5^8 possible rows: [y | t] is what is distinct
        for f32_form in (False, True):
            for k, v in zip(("dt", "dA", "dBq", "dBv"), c.grads(f32_form=f32_form)):
                shares[f"lora {k} M={M} f32 {f32_form}"] = rx.nonzero_share(v)
    low = min(shares, key=shares.get)
    _log("nonzero_share", H=H, lowest=shares[low], at=low)
    assert shares[low] >= 0.95, (low, shares[low])


def test_colsum_and_embed_outputs_are_non_degenerate():
    for n, M in ((768, 1), (768, 1793), (36, 333), (33, 9)):
        g, _, want = rx.colsum_case(M, n)
        assert rx.nonzero_share(want) >= 0.95 and _distinct_rows(g)
    for variant in ("random+types", "same"):
        e = rx.embed_case(3, 43, 512, variant)
        for k in ("want_word", "want_pos", "want_typ"):
            assert rx.nonzero_share(torch.nan_to_num(e[k], nan=1.0)) >= 0.95
        assert _distinct_rows(e["d"])


# --------------------------------------------------------------------- the restatements equal f64; the mutations change them
@pytest.mark.parametrize("M", [1, 5, 1031, rx.LN_CAP_LORA_BWD + 3])
def test_layernorm_bwd_restated_in_f32_is_f64_at_512_and_mutations_show(M):
    H = 512
    c = rx.LnCase(M, H)
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(M))
    for f in rx.ln_bwd_forms(H, 5):
        name, _, gr, gg, lora, mode = f[:6]
        want = c.dx(gg is not None, lora, mode, gr is not None)
        res = c.g_resid if gr is not None else None
        dy = assemble_dy_f32(c.g_gemm if gg is not None else None, c.dt if lora else None, c.lora_a, res, mode)
        got = ln_bwd_f32(c.x, c.stats, c.gamma, dy, res, mode)
        assert torch.equal(got.double(), want), (name, rx.first_diff(got.double(), want))
        anyorder = ln_bwd_f32(c.x, c.stats, c.gamma, dy, res, mode, rowsum=lambda v: v[:, perm].sum(1, keepdim=True))
        assert torch.equal(anyorder.double(), want), name
        assert torch.equal(want.float().double(), want)
        if M < 2:
            continue
        # (mean, rstd) of two neighbouring rows swapped; the previous row's rstd (what a stale register would hold)
        r = M // 2
        st = c.stats.clone()
        st[[r, r - 1]] = c.stats[[r - 1, r]]
        assert not torch.equal(ln_bwd_f32(c.x, st, c.gamma, dy, res, mode)[[r - 1, r]].double(), want[[r - 1, r]]), name
        st = c.stats.clone()
        st[1:, 1] = c.stats[:-1, 1]
        assert not torch.equal(ln_bwd_f32(c.x, st, c.gamma, dy, res, mode).double(), want), name
        # a row skipped (never written: still NaN), a row's result stored twice (into its neighbour as well)
        twice = got.clone()
        twice[r] = got[r - 1]
        assert not torch.equal(twice.double(), want)
        # a lane's 4-column piece stored 256 columns off
        off = got.clone()
        off[:, 256 + 8:256 + 12] = got[:, 8:12]
        assert not torch.equal(off.double(), want)
        # 16-bit operand outputs: one RNE; a truncating conversion differs, in either format
        for dt16 in (torch.bfloat16, torch.float16):
            rne = one_rne(want, dt16)
            assert torch.equal(rne, want.to(dt16)), "rounding through f32 and straight from f64 differ"
            assert not torch.equal(truncated(got, dt16), rne), (name, dt16)
        hi, lo = rx.split3(got)
        assert (lo != 0).any() and torch.equal((hi.double() + lo.double())[0, :8], (hi.float() + lo.float()).double()[0, :8])


@pytest.mark.parametrize("H", rx.HS)
@pytest.mark.parametrize("M", rx.PGRAD_M)
def test_ln_param_grad_restated_in_f32_is_f64_and_mutations_show(M, H):
    c = rx.LnCase(M, H)
    gen = torch.Generator().manual_seed(M)
    for mode in (0, 1):
        for lora in (False, True):
            want = c.pgrad(True, lora, mode, True)
            got = pgrad_f32(c, lora, mode)
            assert torch.equal(got[0].double(), want[0]) and torch.equal(got[1].double(), want[1]), (mode, lora)
            if (mode, lora) != (1, True):
                continue
            # any order: the rows shuffled through the same decomposition
            p = torch.randperm(M, generator=gen)
            c2 = rx.LnCase(M, H)
            for k in ("x", "stats", "g_gemm", "g_resid", "dt"):
                setattr(c2, k, getattr(c, k)[p].contiguous())
            shuffled = pgrad_f32(c2, lora, mode)
            assert torch.equal(shuffled[0], got[0]) and torch.equal(shuffled[1], got[1])
            for r in sorted({0, M // 2, M - 1}):
                for wt in (0.0, 2.0):                                            # row r skipped / taken twice
                    w = torch.ones(M)
                    w[r] = wt
                    mut = pgrad_f32(c, lora, mode, weights=w)
                    assert not torch.equal(mut[0], got[0]) and not torch.equal(mut[1], got[1]), (r, wt)
            if pgrad_blocks(M) > 1:
                mut = pgrad_f32(c, lora, mode, drop_last_slab=True)
                assert not torch.equal(mut[0], got[0]) and not torch.equal(mut[1], got[1])
            if M > 1:
                st = c.stats.clone()
                st[[M - 1, M - 2]] = c.stats[[M - 2, M - 1]]
                assert not torch.equal(pgrad_f32(c, lora, mode, stats=st)[0], got[0])


@pytest.mark.parametrize("H", rx.HS)
@pytest.mark.parametrize("M", rx.LORA_M)
def test_lora_grad_restated_in_f32_is_f64_and_mutations_show(M, H):
    c = rx.LoraCase(M, H)
    want = c.grads()
    got = lora_grad_f32(c)
    for k, a, b in zip(("dt", "dA", "dBq", "dBv"), got, want):
        assert torch.equal(a.double(), b), (k, rx.first_diff(a.double().reshape(a.shape[0], -1), b.reshape(a.shape[0], -1)))
    if M in rx.LORA_F32_M:
        t = c.y @ c.lora_a.t()
        for k, a, b in zip(("dt", "dA", "dBq", "dBv"), lora_grad_f32(c, t=t), c.grads(f32_form=True)):
            assert torch.equal(a.double(), b), ("f32 form", k)
    for r in sorted({0, M - 1}):
        for wt in (0.0, 2.0):
            w = torch.ones(M)
            w[r] = wt
            mut = lora_grad_f32(c, weights=w)
            assert all(not torch.equal(mut[i], got[i]) for i in (1, 2, 3)), (r, wt)
    if lora_blocks(M) > 1:
        mut = lora_grad_f32(c, drop_last_slab=True)
        assert all(not torch.equal(mut[i], got[i]) for i in (1, 2, 3))
    if M > 1:                                   # a refetched slot's t taken from the previous row
        t = c.t.clone()
        t[M - 1] = c.t[M - 2]
        mut = lora_grad_f32(c, t=t)
        assert not torch.equal(mut[2], got[2]) or not torch.equal(mut[3], got[3])


def test_colsum_restated_in_f32_is_f64_and_mutations_show():
    for wide, N, Ms in ((True, rx.COLSUM_WIDE_N, rx.COLSUM_WIDE_M), (False, rx.COLSUM_NARROW_N, rx.COLSUM_NARROW_M)):
        for n in N:
            for M in Ms:
                g, out0, want = rx.colsum_case(M, n)
                got = colsum_f32(g, out0, wide)
                assert torch.equal(got.double(), want), (wide, n, M)
                for r in sorted({0, M - 1}):
                    for wt in (0.0, 2.0):
                        w = torch.ones(M)
                        w[r] = wt
                        # a row of zeros (one column in 7 per row) cannot show; over >= 8 columns at least one element moves
                        assert n < 8 or not torch.equal(colsum_f32(g, out0, wide, weights=w), got), (n, M, r, wt)


# ------------------------------------------------------------------------------------- the toleranced cases: room under each bar
def _share(figs, key, err, bar):
    figs[key] = max(figs.get(key, 0.0), err / bar)


def _cast(t, name):
    return t.to(rx.DTYPE[name]).float()


def test_layernorm_bwd_768_on_exact_inputs_uses_under_half_its_bar():
    """The f32 arithmetic is held to half of the f32 bar.  A 16-bit output's bar IS one worst-case rounding (plus the f32 bar), which
    no choice of inputs halves: the rounded restatement is shown inside it, and its share printed."""
    H, figs, rounded = 768, {}, {}
    for M in rx.LN_BWD_M:
        c = rx.LnCase(M, H)
        for gg, lora, mode, gr in _distinct_dy(H, M):
            want = c.dx(gg, lora, mode, gr)
            res = c.g_resid if gr else None
            dy = assemble_dy_f32(c.g_gemm if gg else None, c.dt if lora else None, c.lora_a, res, mode)
            got = ln_bwd_f32(c.x, c.stats, c.gamma, dy, res, mode)
            _share(figs, "f32", rx.row_err(got, want), rx.BAR_LN_BWD)
            for dt16 in (torch.bfloat16, torch.float16):
                _share(rounded, str(dt16), rx.row_err(got.to(dt16), want), rx.bar_16bit(dt16))
    _log("layernorm_bwd_768_exact_inputs share of bar", **figs, **{"rounded " + k: v for k, v in rounded.items()})
    assert max(figs.values()) <= 0.5 and max(rounded.values()) < 1.0, (figs, rounded)


@pytest.mark.parametrize("offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("H", rx.HS)
def test_layernorm_on_real_rows_uses_under_half_of_each_bar(H, offset):
    """Forward (every M and x format of the GPU file) and backward (its M, modes and LoRA term) restated in f32 against f64.  The bar of
    the bf16 t block is test_10's TOL_BF16 = 4e-3, barely above ONE worst-case bf16 rounding (2^-8 = 3.9e-3): the f32 sums are held to
    half of it, the rounded block to all of it (eight values per row, so a row can come close), and its share is printed."""
    figs, rounded = {}, {}
    eps = 1e-6
    for M in sorted(set(rx.LN_FWD_M + rx.LN_REAL_M)):
        inp = rx.real_ln_inputs(M, H, offset)
        for xfmt in ("f32", "bf16", "fp16"):
            x = _cast(inp["x"], xfmt)
            ratio = rx.mean_over_std(x)
            y64, mean64, rstd64 = rx.ln_fwd64(x, inp["gamma"], inp["beta"], eps)
            y, stats, t = ln_fwd_f32(x, inp["gamma"], inp["beta"], eps, inp["lora_a"])
            if M in rx.LN_FWD_M:
                _share(figs, "fwd y", rx.row_err(y, y64), rx.offset_bar(1e-6, ratio) if offset else rx.BAR_LN_FWD)
                t64 = y64 @ inp["lora_a"].double().t()
                _share(figs, "fwd t", rx.row_err(t, t64), rx.BAR_T)
                _share(rounded, "fwd t bf16", rx.row_err(t.bfloat16(), t64), rx.BAR_T)
                _share(figs, "fwd mean", ((stats[:, 0].double() - mean64).abs() / (2.0 ** -20 * x.double().abs().amax(1))).max().item(), 1.0)
                _share(figs, "fwd rstd", (stats[:, 1].double() / rstd64 - 1).abs().max().item(), 1e-6)
            if M in rx.LN_REAL_M and xfmt != "fp16":
                bar = rx.offset_bar(rx.BAR_LN_BWD, ratio) if offset else rx.BAR_LN_BWD
                for mode in (0, 1):
                    for lora in (False, True):
                        dy = assemble_dy_f32(inp["g_gemm"], inp["dt"] if lora else None, inp["lora_a"], inp["g_resid"], mode)
                        got = ln_bwd_f32(x, stats, inp["gamma"], dy, inp["g_resid"], mode)
                        dy64 = inp["g_gemm"].double() + (inp["dt"].double() @ inp["lora_a"].double() if lora else 0)
                        want = rx.ln_bwd64(x, inp["gamma"], eps, dy64, inp["g_resid"], mode)
                        _share(figs, "bwd", rx.row_err(got, want), bar)
    _log("layernorm_real_rows share of bar", H=H, offset=offset, **figs, **rounded)
    assert max(figs.values()) <= 0.5 and max(rounded.values()) < 1.0, (figs, rounded)
