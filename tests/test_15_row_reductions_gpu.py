"""The row and column reductions that produce every trainable gradient -- bsclip_layernorm_bwd, bsclip_ln_param_grad (+ the slab
reducer), bsclip_lora_grad / _f32, bsclip_colsum, bsclip_transpose_colsum_bf16, bsclip_embed_grad -- and the bf16 / fp16 / split
instantiations of bsclip_layernorm_fwd, at every row count where their loops change path: one row, fewer rows than a prefetch is deep,
the unroll and tail boundaries, one row past the grid cap (the first waves take a second row, the rest do not), twice the cap, every
slab count around the reducers' groups.

Inputs come from tests/row_exact.py: integers and powers of two on which no sum rounds in f32 IN ANY ORDER, so the kernels are held to
BIT EQUALITY with f64 at any row count and grid decomposition -- f32 outputs equal it, 16-bit outputs are one round-to-nearest-even of
it, split operands its split (tests/test_04_row_exact_cpu.py proves the bounds, that the kernels' decompositions restated in f32 give
f64 exactly, and that a skipped, doubled or swapped row, a dropped slab, a misplaced lane piece or a truncating conversion changes an
element).  Tolerances only where the arithmetic truly rounds: bsclip_layernorm_bwd at H = 768 (1 / 768 is no dyadic), real-valued
rows, the forward -- each PER ROW, with the bars tests 10 and 12 use on whole tensors; the CPU file shows the f32 arithmetic under half
of each.  Every output lives in a NaN-filled buffer with spare rows and pad columns (or guard elements) that must still be NaN;
accumulators start from non-zero integers.  Every toleranced figure is printed as a ``FIGURES {json}`` line before it is asserted."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import row_exact as rx  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS = 1e-6


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    o.init_tables()
    return o


def _log(test, **figures):
    print("FIGURES " + json.dumps({"test": test, **figures}))


class Worst:
    """err / bar of every toleranced comparison of a test, the largest kept per key; printed, then asserted <= 1."""

    def __init__(self, test, **where):
        self.test, self.where, self.top = test, where, {}

    def add(self, key, err, bar, at):
        r = err / bar
        if r != r or r >= self.top.get(key, (-1.0, ""))[0]:
            self.top[key] = (float("inf") if r != r else r, at)

    def check(self):
        _log(self.test, **self.where, **{k + "_err_over_bar": v[0] for k, v in self.top.items()}, **{k + "_at": v[1] for k, v in self.top.items()})
        for k, (r, at) in self.top.items():
            assert r <= 1.0, f"{k}: err / bar = {r} at {at}"


def _guarded(init, tail=0):
    """(buf, view): ``init`` (any shape, contiguous f32) copied into the middle of a NaN-filled 1-D buffer with 8 guard elements in front
    and 8 + tail behind -- for the accumulators the wrappers want contiguous.  ``tail`` > 0: the view takes that many NaNs along (an
    output longer than what the kernel may write)."""
    n = init.numel()
    buf = torch.full((n + 16 + tail,), NAN, device=DEV)
    buf[8:8 + n] = init.reshape(-1)
    return buf, (buf[8:8 + n].view(init.shape) if tail == 0 else buf[8:8 + n + tail])


def _guards_intact(buf, n):
    return torch.isnan(buf[:8]).all().item() and torch.isnan(buf[8 + n:]).all().item()


_LN = {}


def _ln_case(M, H):
    if (M, H) not in _LN:
        _LN.clear()                                  # one case at a time: the largest holds 5 tensors of 32 773 x 768
        _LN[(M, H)] = rx.LnCase(M, H, DEV)
    return _LN[(M, H)]


_REAL = {}


def _real(M, H, offset):
    """row_exact.real_ln_inputs on the GPU, drawn once (the forward's 24 parametrisations share 28 input sets)."""
    if (M, H, offset) not in _REAL:
        _REAL[(M, H, offset)] = rx.real_ln_inputs(M, H, offset, DEV)
    return _REAL[(M, H, offset)]


# ------------------------------------------------------------------------------------------------------------ layernorm_bwd
def _run_ln_bwd(ops, H, M, form, x, stats, gamma, g_resid, g_gemm, dt, lora_a):
    """One call of ops.layernorm_bwd in ``form`` (row_exact.LN_BWD_FORMS) on f32 inputs cast to the form's formats, every matrix with a
    leading dimension of its own.  Returns {"dx": (buf, dtype) or None, "op": (buf, kind) or None}."""
    _, xf, gr, gg, lora, mode, dxf, opf, _ = form
    kw = {}
    if gr is not None:
        kw["g_resid"] = rx.padded(g_resid, 4, rx.DTYPE[gr])
    if gg is not None:
        kw["g_gemm"] = rx.padded(g_gemm, 12, rx.DTYPE[gg])
    if lora:
        kw["dt"], kw["lora_a"] = dt, lora_a
    out = {"dx": None, "op": None}
    if dxf is not None:
        buf, view = rx.strided(M, H, H + 4, rx.DTYPE[dxf], device=DEV)
        kw["dx_f32"] = view
        out["dx"] = buf
    if opf == "split3":
        buf, view = rx.strided(M, 3 * H, 3 * H + 8, BF16, device=DEV)
        kw["dx_split3"] = view
        out["op"] = buf
    elif opf is not None:
        buf, view = rx.strided(M, H, H + 8, rx.DTYPE[opf], device=DEV)
        kw["dx_bf16"] = view
        out["op"] = buf
    ops.layernorm_bwd(rx.padded(x, 8, rx.DTYPE[xf]), stats, gamma, mode, M=M, **kw)
    return out


def _check_ln_bwd(H, M, form, out, want, worst, exact):
    """``want``: f64 [M, H].  ``exact``: f32 outputs equal it, 16-bit outputs are one RNE of it, the split operand its split.  Otherwise
    f32 outputs are held per row to BAR_LN_BWD, and the operand must be the RNE / the split / the copy of the f32 output of the SAME
    call; a 16-bit output without an f32 twin is held to the bar plus one rounding (row_exact.bar_16bit)."""
    name, opf, dxf = form[0], form[7], form[6]
    tag = f"{name} H={H} M={M}"
    want32 = want.float()
    dx = op = None
    if out["dx"] is not None:
        assert rx.untouched(out["dx"], M, H), f"{tag}: dx_res wrote outside its M rows / H columns"
        dx = out["dx"][:M, :H]
    if out["op"] is not None:
        cols = 3 * H if opf == "split3" else H
        assert rx.untouched(out["op"], M, cols), f"{tag}: the operand output wrote outside its M rows / {cols} columns"
        op = out["op"][:M, :cols]
    if exact:
        if dx is not None:
            w = want32.to(dx.dtype)
            assert torch.equal(dx, w), f"{tag} dx_res: {rx.first_diff(dx, w)}"
        ref32 = want32
    else:
        if dx is not None:
            worst.add("dx_" + dxf, rx.row_err(dx, want), rx.BAR_LN_BWD if dxf == "f32" else rx.bar_16bit(dx.dtype), tag)
        ref32 = dx if (dx is not None and dxf == "f32") else None
    if op is None:
        return
    if opf == "split3":
        assert ref32 is not None
        hi, lo = rx.split3(ref32)
        assert torch.equal(op[:, :H], hi) and torch.equal(op[:, H:2 * H], lo) and torch.equal(op[:, 2 * H:], hi), f"{tag}: split operand"
    elif ref32 is not None:
        w = ref32.to(op.dtype)
        assert torch.equal(op, w), f"{tag} operand: {rx.first_diff(op, w)}"
    else:
        if dx is not None:     # both on the 16-bit stream: the same value rounded the same way
            assert torch.equal(op, dx), f"{tag}: operand and dx_res differ: {rx.first_diff(op, dx)}"
        worst.add("op_" + opf, rx.row_err(op, want), rx.bar_16bit(op.dtype), tag)


@pytest.mark.parametrize("M", rx.LN_BWD_M)
@pytest.mark.parametrize("H", rx.HS)
def test_layernorm_bwd_exact_inputs(ops, H, M):
    """bsclip_layernorm_bwd on exact inputs with supplied (mean, rstd).  Row counts: 1, 3, 4, 5 (fewer rows than a workgroup has waves,
    one workgroup, one wave of a second), 1031, cap + 3 (waves 0 .. 2 take a second row, the rest do not) and 2 cap + 1 for both
    caps -- 8192 rows without lora_a, 4096 with (row_exact.LN_CAP*, read from ln_grid's call sites).  The forms the engines launch
    at every M, all nineteen (fifteen at H = 512: no fp16) at M = 5 and at both cap + 3.
    H = 512: bit equality with f64.  H = 768: per-row 2-norm error below 5e-5 (test_10's bar, there on the whole tensor), the operand
    bit-equal to the rounding / split / copy of the f32 output of the same call."""
    c = _ln_case(M, H)
    worst = Worst("layernorm_bwd_exact_inputs", H=H, M=M)
    for form in rx.ln_bwd_forms(H, M):
        _, _, gr, gg, lora, mode = form[:6]
        out = _run_ln_bwd(ops, H, M, form, c.x, c.stats, c.gamma, c.g_resid, c.g_gemm, c.dt, c.lora_a)
        want = c.dx(gg is not None, lora, mode, gr is not None)
        _check_ln_bwd(H, M, form, out, want, worst, exact=(H == 512))
    worst.check()


REAL_FORMS = tuple(f for f in rx.LN_BWD_FORMS if f[0] in ("m0-lora", "m1-lora", "m0", "m1", "stream-f32-in-16-out"))


@pytest.mark.parametrize("offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("M", rx.LN_REAL_M)
@pytest.mark.parametrize("H", rx.HS)
def test_layernorm_bwd_real_rows(ops, H, M, offset):
    """Real-valued rows with the statistics ops.layernorm_fwd leaves, x as f32 and as bf16, both modes, with and without dt . A, at 1031
    rows and at cap + 3 of both caps, against f64 LayerNorm backward of the same (rounded) x.  Per row: 5e-5 on plain rows; on rows whose
    mean is 32 - 64 x their standard deviation 5e-5 + 2^-21 max |mean| / std (test_12's forward allowance: the f32 mean carries a few
    ulps of the offset).  The bf16 operand must be the RNE of the f32 output of the same call, bit for bit."""
    inp = _real(M, H, offset)
    worst = Worst("layernorm_bwd_real_rows", H=H, M=M, offset=offset)
    for form in REAL_FORMS:
        xf, lora, mode = form[1], form[4], form[5]
        x = inp["x"].to(rx.DTYPE[xf]).float()
        stats = torch.full((M + 2, 2), NAN, device=DEV)
        ops.layernorm_fwd(rx.padded(x, 8, rx.DTYPE[xf]), inp["gamma"], inp["beta"], EPS, stats=stats, M=M,
                          y_bf16=torch.empty(M, H, device=DEV, dtype=BF16))
        assert torch.isnan(stats[M:]).all() and not torch.isnan(stats[:M]).any()
        out = _run_ln_bwd(ops, H, M, form, x, stats, inp["gamma"], inp["g_resid"], inp["g_gemm"], inp["dt"], inp["lora_a"])
        dy = inp["g_gemm"].double() + (inp["dt"].double() @ inp["lora_a"].double() if lora else 0)
        want = rx.ln_bwd64(x, inp["gamma"], EPS, dy, inp["g_resid"], mode)
        tag = f"{form[0]} H={H} M={M}"
        bar = rx.offset_bar(rx.BAR_LN_BWD, rx.mean_over_std(x)) if offset else rx.BAR_LN_BWD
        assert rx.untouched(out["dx"], M, H) and rx.untouched(out["op"], M, H), tag
        dx, op = out["dx"][:M, :H], out["op"][:M, :H]
        if dx.dtype == F32:
            worst.add("dx_f32", rx.row_err(dx, want), bar, tag)
            assert torch.equal(op, dx.bfloat16()), f"{tag}: the operand is not the RNE of the f32 output: {rx.first_diff(op, dx.bfloat16())}"
        else:
            worst.add("dx_bf16", rx.row_err(dx, want), bar + rx.UNIT_ROUNDOFF[BF16], tag)
            assert torch.equal(op, dx), tag
    worst.check()


# ------------------------------------------------------------------------------------------------------------ layernorm_fwd
@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("xf,opf", rx.LN_FWD_FORMS)
@pytest.mark.parametrize("H", rx.HS)
def test_layernorm_fwd_16bit_and_split_instantiations(ops, H, xf, opf, lora):
    """The bf16, fp16 and split3 forms of bsclip_layernorm_fwd (fp8 has test_layernorm_fwd_fp8) at M = 1, 3, 5, cap + 3 and 2 cap + 1
    for both caps -- 8192 rows, 5120 with lora_a: past cap + 3 the one-row-ahead prefetch of the first waves loads a second row and no
    other wave may.  Plain rows and rows whose mean is 32 - 64 x their standard deviation.  Per row: y_f32 against f64 at test_10's
    TOL_F32 (offset rows: test_12's 1e-6 + 2^-21 ratio), the 16-bit operand bit-equal to the RNE of y_f32, the split operand its split,
    t = y A^T at TOL_BF16, columns [H + 8, H + 64) zero, mean within 2^-20 max |x| and rstd within 1e-6 (test_12's stats bars)."""
    worst = Worst("layernorm_fwd_instantiations", H=H, x=xf, operand=opf, lora=lora)
    h16 = F16 if "fp16" in (xf, opf) else BF16
    for M in rx.LN_FWD_M:
        for offset in (False, True):
            inp = _real(M, H, offset)
            x = inp["x"].to(rx.DTYPE[xf]).float()
            tag = f"M={M} offset={offset}"
            kw, ybuf, y3buf = {}, None, None
            ycols = H + (64 if lora else 0)
            if opf != "split3" or lora:
                ybuf, kw["y_bf16"] = rx.strided(M, ycols, ycols + 8, h16, device=DEV)
            if opf == "split3":
                y3buf, kw["y_split3"] = rx.strided(M, 3 * H, 3 * H + 8, BF16, device=DEV)
            y32 = torch.full((M + 3, H), NAN, device=DEV)
            stats = torch.full((2 * M + 4,), NAN, device=DEV)
            ops.layernorm_fwd(rx.padded(x, 8, rx.DTYPE[xf]), inp["gamma"], inp["beta"], EPS, y_f32=y32, stats=stats, M=M,
                              lora_a=inp["lora_a"] if lora else None, **kw)
            y64, mean64, rstd64 = rx.ln_fwd64(x, inp["gamma"], inp["beta"], EPS)
            assert torch.isnan(y32[M:]).all() and torch.isnan(stats[2 * M:]).all(), f"{tag}: rows >= M of y_f32 / stats written"
            bar = rx.offset_bar(1e-6, rx.mean_over_std(x)) if offset else rx.BAR_LN_FWD
            worst.add("y_f32", rx.row_err(y32[:M], y64), bar, tag)
            st = stats[:2 * M].view(M, 2).double()
            worst.add("mean", ((st[:, 0] - mean64).abs() / (2.0 ** -20 * x.double().abs().amax(1))).max().item(), 1.0, tag)
            worst.add("rstd", (st[:, 1] / rstd64 - 1).abs().max().item(), 1e-6, tag)
            if ybuf is not None:
                assert rx.untouched(ybuf, M, ycols), f"{tag}: the operand wrote outside its M rows / {ycols} columns"
                w = y32[:M].to(h16)
                assert torch.equal(ybuf[:M, :H], w), f"{tag}: the operand is not the RNE of y_f32: {rx.first_diff(ybuf[:M, :H], w)}"
                if lora:
                    worst.add("t", rx.row_err(ybuf[:M, H:H + 8], y64 @ inp["lora_a"].double().t()), rx.BAR_T, tag)
                    assert (ybuf[:M, H + 8:H + 64] == 0).all(), f"{tag}: columns [H + 8, H + 64) are not zero"
            if y3buf is not None:
                assert rx.untouched(y3buf, M, 3 * H), f"{tag}: the split operand wrote outside its M rows / 3H columns"
                hi, lo = rx.split3(y32[:M])
                assert torch.equal(y3buf[:M, :H], hi) and torch.equal(y3buf[:M, H:2 * H], lo) and torch.equal(y3buf[:M, 2 * H:3 * H], hi), tag
    worst.check()


# ------------------------------------------------------------------------------------------------------------ ln_param_grad
@pytest.mark.parametrize("M", rx.PGRAD_M)
@pytest.mark.parametrize("H", rx.HS)
def test_ln_param_grad_exact(ops, H, M):
    """bsclip_ln_param_grad at 1, 1, 1, 1, 2, 8, 9, 32, 34 and 1024 slabs (M = 1 .. 32 773; ceil(M / 32) workgroups, capped at
    PG_MAX_BLOCKS = 1024, where every wave walks nine rows): the slab reducer's eight groups with no slab, one each, one more, its
    4-way unrolled loop exactly filled, its tail.  x as f32 and bf16, both modes (mode 0 must ignore g_resid), with and without
    dt . A, strided x / g_gemm / g_resid.  d_gamma and d_beta, which start from non-zero integers: bit-equal to f64, twice."""
    c = _ln_case(M, H)
    gg, gr = rx.padded(c.g_gemm, 12, BF16), rx.padded(c.g_resid, 4)
    for xf, mode, lora in rx.PGRAD_FORMS:
        x = rx.padded(c.x, 8, rx.DTYPE[xf])
        want_g, want_b = c.pgrad(True, lora, mode, True)
        for call in range(2):
            (gbuf, dg), (bbuf, db) = _guarded(c.dg0), _guarded(c.db0)
            ops.ln_param_grad(x, c.stats, mode, dg, db, g_resid=gr, g_gemm=gg, dt=c.dt if lora else None, lora_a=c.lora_a if lora else None, M=M)
            tag = f"H={H} M={M} x {xf} mode {mode} lora {lora} call {call}"
            assert torch.equal(dg.double(), want_g), f"{tag} d_gamma: {rx.first_diff(dg.double()[None], want_g[None])}"
            assert torch.equal(db.double(), want_b), f"{tag} d_beta: {rx.first_diff(db.double()[None], want_b[None])}"
            assert _guards_intact(gbuf, H) and _guards_intact(bbuf, H), f"{tag}: wrote beside d_gamma / d_beta"


# ---------------------------------------------------------------------------------------------------------------- lora_grad
def _check_lora(tag, got, want):
    for k, a, b in zip(("dt", "dA", "dBq", "dBv"), got, want):
        a, b = a.double().reshape(a.shape[0], -1), b.reshape(a.shape[0], -1)
        assert torch.equal(a, b), f"{tag} {k}: {rx.first_diff(a, b)}"


@pytest.mark.parametrize("M", rx.LORA_M)
@pytest.mark.parametrize("H", rx.HS)
def test_lora_grad_bf16_exact(ops, H, M):
    """bsclip_lora_grad on bf16 rows at M = 1, 2, 3, 7 (fewer rows than the three-deep prefetch has slots times wave pairs: a pair
    fetches one, two or no rows ahead), 65 (three workgroups, the last with one row), 2077 and 24 583 (LG_MAX_BLOCKS = 768 workgroups,
    every pair walks sixteen rows + seven of them a seventeenth).  dt, dA, dBq, dBv bit-equal to f64; dt rows >= M untouched; a second
    call doubles what the accumulators received, exactly."""
    c = rx.LoraCase(M, H, DEV)
    dqkv = rx.padded(c.dqkv, 4, BF16)
    hbuf = torch.full((M + 3, H + 16), NAN, device=DEV, dtype=BF16)
    hbuf[:M, :H], hbuf[:M, H:H + 8] = c.y.to(BF16), c.t.to(BF16)
    dt = torch.full((M + 3, 8), NAN, device=DEV)
    bufs = [_guarded(c.dA0), _guarded(c.dBq0), _guarded(c.dBv0)]
    for call in (1, 2):
        dt[:] = NAN
        ops.lora_grad(dqkv, hbuf[:, :H + 8], M, H, c.lora_b, dt, *[v for _, v in bufs])
        _check_lora(f"H={H} M={M} call {call}", (dt[:M], *[v for _, v in bufs]), c.grads(calls=call))
        assert torch.isnan(dt[M:]).all(), "dt rows >= M written"
        assert all(_guards_intact(b, v.numel()) for b, v in bufs), "wrote beside dA / dBq / dBv"


@pytest.mark.parametrize("M", rx.LORA_F32_M)
@pytest.mark.parametrize("H", rx.HS)
def test_lora_grad_f32_exact(ops, H, M):
    """bsclip_lora_grad_f32 (the same kernels on f32 rows, t = y A^T rebuilt first) on the same inputs: dA and dB bit-equal to f64,
    doubled exactly by a second call."""
    c = rx.LoraCase(M, H, DEV)
    dqkv, y = rx.padded(c.dqkv, 4), rx.padded(c.y, 4)
    (abuf, dA), (bbuf, dB) = _guarded(c.dA0), _guarded(torch.stack([c.dBq0, c.dBv0]))
    for call in (1, 2):
        ops.lora_grad_f32(dqkv, y, M, H, c.lora_a, c.lora_b, dA, dB)
        want = c.grads(calls=call, f32_form=True)
        _check_lora(f"H={H} M={M} call {call}", (dA, dB[0], dB[1]), want[1:])
        assert _guards_intact(abuf, 8 * H) and _guards_intact(bbuf, 8 * H), "wrote beside dA / dB"


# ------------------------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
def test_colsum_exact(ops, wide, dtype):
    """bsclip_colsum.  Wide kernel (N % 8 == 0, ld % 8 == 0): N = 8 and 768 at M around its 256-row stride and the 4-way unrolled loop's
    bound r + 768 < M (1, 255 .. 257, 768, 769, 1023 .. 1025, 1793).  Narrow kernel: N = 1, 33, 36 at M around its 8-row stride and
    r + 24 < M (1, 8, 9, 24, 25, 32, 33, 333).  ld > N; out starts from non-zero integers; bit-equal to f64; out[N:] untouched."""
    Ns, Ms, pad = (rx.COLSUM_WIDE_N, rx.COLSUM_WIDE_M, 8) if wide else (rx.COLSUM_NARROW_N, rx.COLSUM_NARROW_M, 4)
    for N in Ns:
        for M in Ms:
            g, out0, want = rx.colsum_case(M, N, DEV)
            gp = rx.padded(g, pad, dtype)
            assert (N % 8 == 0 and gp.stride(0) % 8 == 0) == wide      # bsclip_colsum's choice of kernel
            buf, out = _guarded(out0, tail=5)
            ops.colsum(gp, M, N, out)
            assert torch.equal(out[:N].double(), want), f"N={N} M={M}: {rx.first_diff(out[:N].double()[None], want[None])}"
            assert _guards_intact(buf, N), f"N={N} M={M}: out[N:] or the guards written"


@pytest.mark.parametrize("C", rx.TRANSPOSE_C)
@pytest.mark.parametrize("R", rx.TRANSPOSE_R)
def test_transpose_colsum_exact(ops, R, C):
    """bsclip_transpose_colsum_bf16 (the slab reducer's third user: ceil(R / 64) slabs) at R = 1, 63, 64, 65, 130: the transpose equal,
    nothing written outside [C, R], the column sums bit-equal to f64 on top of what the output held."""
    g, out0, want = rx.colsum_case(R, C, DEV)
    src = rx.padded(g, 8, BF16)
    ld_out = (R + 7) // 8 * 8 + 8
    dbuf = torch.full((C + 3, ld_out), NAN, device=DEV, dtype=BF16)
    buf, out = _guarded(out0)
    ops.transpose_colsum_bf16(src, R, C, dbuf[:, :R], out)
    assert torch.equal(dbuf[:C, :R], src.t()) and rx.untouched(dbuf, C, R)
    assert torch.equal(out.double(), want), rx.first_diff(out.double()[None], want[None])
    assert _guards_intact(buf, C)


# --------------------------------------------------------------------------------------------------------------- embed_grad
@pytest.mark.parametrize("H", rx.EMBED_H)
@pytest.mark.parametrize("B,S", rx.EMBED_BS)
def test_embed_grad_exact(ops, B, S, H):
    """bsclip_embed_grad on a vocabulary of 37 with pad id 0: one token, a ragged / full / ragged second 64-token ballot chunk (63, 64,
    65 tokens), 129 tokens in three sequences, seventeen one-token sequences, and 8193 tokens (rows_per_block = 17, one past the 16
    that every smaller case uses; 482 slabs).  Random ids reaching below 0 and past the vocabulary (clamped as the kernel documents),
    every token holding the same id, type ids present and absent.  The three tables start from non-zero integers; bit-equal to f64
    autograd on the clamped ids; the pad row and the position rows >= S (NaN before) untouched; two calls bit-identical."""
    for variant in ("random", "random+types", "same", "same+types"):
        e = rx.embed_case(B, S, H, variant, DEV)
        outs = []
        for _ in range(2):
            dw, dp = e["word0"].clone(), e["pos0"].clone()
            dty = torch.full((3, H), NAN, device=DEV)
            dty[:2] = e["typ0"]
            ops.embed_grad(e["ids"], e["type_ids"], e["d"], dw, dp, dty, pad_id=0)
            outs.append((dw, dp, dty))
        tag = f"B={B} S={S} H={H} {variant}"
        dw, dp, dty = outs[0]
        assert rx.same(dw, e["want_word"]), f"{tag} word: {rx.first_diff(torch.nan_to_num(dw.double(), nan=-1.0), torch.nan_to_num(e['want_word'], nan=-1.0))}"
        assert rx.same(dp, e["want_pos"]), f"{tag} position: {rx.first_diff(torch.nan_to_num(dp.double(), nan=-1.0), torch.nan_to_num(e['want_pos'], nan=-1.0))}"
        assert torch.equal(dty[:2].double(), e["want_typ"]) and torch.isnan(dty[2]).all(), f"{tag} type: {rx.first_diff(dty[:2].double(), e['want_typ'])}"
        assert torch.isnan(dw[0]).all() and torch.isnan(dp[S:]).all(), f"{tag}: the pad row or a position row >= S was written"
        assert all(rx.same(a, b) for a, b in zip(outs[0], outs[1])), f"{tag}: two calls differ"
