"""Every kernel a training step launches beside the GEMMs, the attention, the row reductions and the losses, through
bioscanclip.hip.ops, EVERY ELEMENT against f64 at the sizes where their loops change path (cases, references and bars:
tests/tail_exact.py; the proofs: tests/test_04_tail_exact_cpu.py).

Kernels and path-change sizes (source lines: tail_exact.py's constants):
* bsclip_cast_f32_bf16 / _f16 / _f16_scaled -- n & 3 tails, one element either side of the 2^21-element grid cap, two passes past it;
* bsclip_add_scaled_f32 -- the same around 2^20, scale_log2 in {-64, -13, 0, 13, 64}, out non-zero before;
* bsclip_adamw_step / _step_dev / _step_clip and bsclip_count_nonfinite -- around 524 288 elements (2048 workgroups of 256);
* bsclip_im2col_patch16, four forms -- B = 55 (largest under the cap of 4096 workgroups), 56, 112 (two full extra passes);
* bsclip_dgelu_mul -- 1366 x 3072 and 2731 x 3072 (one and two passes past 4096 workgroups), strided operands;
* bsclip_softmax_meanpool_fwd / _bwd -- S < 4 (waves that own no token), flat to peaked logits, a maximum in the last lane's last
  column, two equal maxima, dlogits with a row stride > C;
* bsclip_meanpool_tokens_fwd / _bwd, bsclip_bert_embed (clamped ids, type ids {0, 1, 2, -1} and None), bsclip_l2norm_fwd / _bwd (a zero
  row, a row under the eps clamp, squares summing to 1e30), bsclip_vit_cls_rows, bsclip_waug_set_lora_layers (three layers in one
  launch), bsclip_mask_to_bias, bsclip_gather_cast_rows, bsclip_transpose_bf16's element kernel (an ld that is no multiple of 8, a
  base one element off), bsclip_counter_add (wrap-around).

BIT equality with the reference for everything that has one right answer (the casts, add_scaled_f32, im2col, bert_embed, the token
mean's backward, the movers, the counters).  Per element or per row bars for AdamW, l2norm, the softmax pooling and the token mean:
tail_exact.BAR, 4 x the f32 restatement's distance from f64 measured on the CPU (test_04_tail_exact_cpu.py), plus half a bf16 ulp of
the reference for bf16 outputs.  Every output lives in a NaN- (or sentinel-) filled buffer with guard elements, spare rows and pad
columns that must be unchanged afterwards.  Every toleranced figure is printed as a ``FIGURES {json}`` line before it is asserted.

Observed on the MI355X (err / bar, worst over all cases of the key; a figure of 1 would be the bar):

    key                  err / bar
    adamw p              0.21
    adamw m              0.22
    adamw v              0.25
    l2norm fwd y         0.25
    l2norm fwd inv_norm  0.25
    l2norm bwd dx        0.21
    softmax pooled       0.24
    softmax stats sum    0.25
    softmax bwd dlogits  0.996  (bf16 output: the half ulp of the rounding is most of the allowance)
    meanpool fwd         0.999  (bf16 output, the same)
"""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import tail_exact as tx  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32, F64, BF16, F16 = tx.F32, tx.F64, tx.BF16, tx.F16
GUARD = 8                    # guard elements in front of and behind every output: 16 bytes of a 16-bit format, 32 of f32
NAN_BITS = 0x7FC00000


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

    def add(self, key, ratio, at):
        if ratio != ratio or ratio >= self.top.get(key, (-1.0, ""))[0]:
            self.top[key] = (float("inf") if ratio != ratio else ratio, at)

    def check(self):
        _log(self.test, **self.where, **{k + "_err_over_bar": v[0] for k, v in self.top.items()}, **{k + "_at": v[1] for k, v in self.top.items()})
        for k, (r, at) in self.top.items():
            assert r <= 1.0, f"{k}: err / bar = {r} at {at}"


class Guarded:
    """A [rows + spare, ld] matrix of ``dtype`` in the middle of a NaN-filled flat buffer, GUARD elements in front and behind (the base
    stays 16-byte aligned); ``view`` is its [:rows, :cols] (or, with ld == cols, the contiguous [rows + spare, cols] / [rows, cols])."""

    def __init__(self, rows, cols, dtype=F32, ld=None, spare=3, fill=NAN):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.flat = torch.full((2 * GUARD + (rows + spare) * self.ld,), fill, dtype=dtype, device=DEV)
        self.body = self.flat[GUARD:GUARD + (rows + spare) * self.ld].view(rows + spare, self.ld)
        self.fill = fill

    @property
    def out(self):           # what the kernel may write
        return self.body[:self.rows, :self.cols]

    def exact(self):         # the contiguous [rows, cols] view (ld == cols) for wrappers that want the exact shape
        assert self.ld == self.cols
        return self.body[:self.rows]

    def intact(self):
        def sent(t):
            return bool((torch.isnan(t) if self.fill != self.fill else t == self.fill).all().item())
        return sent(self.flat[:GUARD]) and sent(self.flat[GUARD + self.body.numel():]) and sent(self.body[self.rows:]) and \
            sent(self.body[:self.rows, self.cols:])


def _same(got, want, what):
    assert tx.bits_equal(got, want.to(got.device)), f"{what}: {tx.bits_diff(got, want.to(got.device))}"


# ------------------------------------------------------------------------------------------------------------------------- casts
@pytest.mark.parametrize("dtype,ks", [(BF16, (0,)), (F16, (0,)), (F16, tx.CAST_SCALED_K_ALL_N)], ids=["bf16", "fp16", "fp16-scaled"])
def test_casts_bit_equal_at_every_tail_and_pass(ops, dtype, ks):
    """out = one round-to-nearest-even of in (* 2^k, exact in f32), bit for bit torch's CPU conversion: specials, ties, overflow, fp16
    and f32 subnormals in the vector body, in the n & 3 tail and astride the first pass's end."""
    scaled = len(ks) > 1
    for n in tx.CAST_N:
        x = tx.cast_input(n)
        xd = x.to(DEV)
        for k in ks + (tx.CAST_SCALED_K_EXTRA if scaled and n in tx.CAST_SCALED_EXTRA_N else ()):
            g = Guarded(1, n, dtype, spare=0)
            dst = g.body[0]
            if scaled:
                ops.cast_f32_f16_scaled(xd, dst, k)
            else:
                ops.cast_f32_bf16(xd, dst)
            torch.cuda.synchronize()
            _same(dst.cpu(), tx.cast_ref(x, dtype, k), f"cast to {dtype} n={n} k={k}")
            assert g.intact(), f"cast to {dtype} n={n} k={k}: wrote outside its n elements"
    if scaled:
        with pytest.raises(RuntimeError):
            ops.cast_f32_f16_scaled(xd, dst, 65)
        with pytest.raises(RuntimeError):
            ops.cast_f32_f16_scaled(xd, dst, -65)


@pytest.mark.parametrize("k", tx.ADD_SCALED_K)
def test_add_scaled_f32_bit_equal(ops, k):
    """out += in * 2^k on inputs where product and sum are exact; out starts from +-(1000 .. 1031)."""
    for n in tx.ADD_SCALED_N:
        src, out0, want = tx.add_scaled_case(n, k, DEV)
        g = Guarded(1, n, F32, spare=0)
        out = g.body[0]
        out.copy_(out0)
        ops.add_scaled_f32(src, out, k)
        torch.cuda.synchronize()
        _same(out, want.float(), f"add_scaled_f32 n={n} k={k}")
        assert g.intact(), f"add_scaled_f32 n={n} k={k}: wrote outside its n elements"
    with pytest.raises(RuntimeError):
        ops.add_scaled_f32(src, out, 65)


# ------------------------------------------------------------------------------------------------------------------------- AdamW
_ADAMW = {}


def _adamw_case(n):
    """(p, m, v, g, max_norm) on the GPU, built once per n: tail_exact.adamw_inputs with the gradient's largest element nudged so that
    an f32 max_norm exists for which the clip record's coef is exactly 0.25."""
    if n not in _ADAMW:
        p, m, v, g = tx.adamw_inputs(n)
        g, max_norm = tx.clip_gradient(g)
        _ADAMW[n] = tuple(t.to(DEV) for t in (p, m, v, g)) + (max_norm,)
    return _ADAMW[n]


def _hyper(lr, step):
    """[lr as f32 bits, step word, two sentinel words]."""
    h = torch.full((4,), -77, dtype=torch.int32, device=DEV)
    h.view(F32)[0:1].fill_(lr)
    h[1:2].fill_(step)
    return h


def _clip_record(ops, grad, max_norm):
    """The record bsclip_grad_clip_finish leaves for ``grad`` (twelve words, four NaN-bit guard words behind them)."""
    state = torch.zeros(16, dtype=torch.int32, device=DEV)
    state[12:] = NAN_BITS
    count = ops.grad_norm_partials(grad.numel())
    partials = torch.full((count + 2,), NAN, dtype=F64, device=DEV)
    ops.grad_sumsq_partial(grad, partials[:count])
    ops.grad_clip_finish(partials[:count], max_norm, state)
    assert torch.isnan(partials[count:]).all() and (state[12:] == NAN_BITS).all()
    return state


@pytest.mark.parametrize("name", list(tx.ADAMW_SETS))
@pytest.mark.parametrize("entry", ["step", "step_dev", "step_clip"])
def test_adamw_every_element_against_f64(ops, entry, name):
    """Three steps from non-zero (m, v) at every n around the grid cap; each step's p, m, v are held per element to f64 AdamW
    (torch.optim.AdamW's formula on the f32 hyperparameters) of the state that step started from.  The device step word is advanced by
    bsclip_counter_add; the clip path reads coef = 0.25 / 1 and apply = 1 from a record bsclip_grad_clip_finish wrote."""
    hp, step0 = tx.ADAMW_SETS[name]
    worst = Worst("adamw", entry=entry, set=name)
    for n in tx.ADAMW_N:
        p0, m0, v0, g, max_norm = _adamw_case(n)
        bufs = [Guarded(1, n, F32, spare=0) for _ in range(3)]
        p, m, v = (b.body[0] for b in bufs)
        for t, src in zip((p, m, v), (p0, m0, v0)):
            t.copy_(src)
        hyper = _hyper(hp["lr"], step0)
        for s in range(tx.ADAMW_STEPS):
            gr = tx.adamw_grad(g, s).contiguous()
            before = (p.clone(), m.clone(), v.clone())
            want, scales = tx.adamw_step64(*before, gr, hp, step0 + s)
            args = (hp["beta1"], hp["beta2"], hp["eps"], hp["wd"])
            if entry == "step":
                ops.adamw_step(p, gr, m, v, hp["lr"], *args, step0 + s, hp["grad_scale"])
            elif entry == "step_dev":
                ops.adamw_step_dev(p, gr, m, v, hyper, *args, hp["grad_scale"])
            else:
                state = _clip_record(ops, gr, max_norm if hp["grad_scale"] == 0.25 else float("inf"))
                words = state.cpu()
                assert words[0].item() == 1 and words[1:2].view(F32).item() == hp["grad_scale"], (n, s, words[:4].tolist())
                ops.adamw_step_clip(p, gr, m, v, hyper, state, *args)
            ops.counter_add(hyper[1:2], 1)
            torch.cuda.synchronize()
            assert hyper.cpu().tolist()[1:] == [step0 + s + 1, -77, -77]
            for key, got, w, allow in zip("pmv", (p, m, v), want, tx.adamw_allowances(scales)):
                worst.add(key, tx.worst(got, w, allow), f"n={n} step={step0 + s}")
            if hp["lr"] == 0.0:
                _same(p, before[0], f"adamw {entry} lr=0 n={n}: p")
            assert all(b.intact() for b in bufs), f"adamw {entry} n={n}: wrote outside its n elements"
    worst.check()


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "fp16"])
def test_count_nonfinite_is_exact(ops, dtype):
    for n in tx.ADAMW_N:
        t, want = tx.nonfinite_case(n, dtype, DEV)
        counter = torch.tensor([-77, 1000, -77], dtype=torch.int32, device=DEV)
        ops.count_nonfinite(t, counter[1:2])
        ops.count_nonfinite(t, counter[1:2])
        assert counter.tolist() == [-77, 1000 + 2 * want, -77], (n, want, counter.tolist())


def test_counter_add_wraps(ops):
    c = torch.tensor([-77, -1, -77, 5, 0, -77], dtype=torch.int32, device=DEV)      # -1 is 2^32 - 1
    ops.counter_add(c[1:2], 1)
    ops.counter_add(c[3:4], -1)              # the wrapper masks the increment to 32 bits
    ops.counter_add(c[4:5], -1)
    assert c.tolist() == [-77, 0, -77, 4, -1, -77]


def test_mask_to_bias(ops):
    for n in tx.MASK_N:
        mask, want = tx.mask_case(n, DEV)
        g = Guarded(1, n, F32, spare=0)
        ops.mask_to_bias(mask, g.body[0])
        _same(g.body[0], want, f"mask_to_bias n={n}")
        assert g.intact()


# ------------------------------------------------------------------------------------------------------------- im2col, dgelu_mul
@pytest.mark.parametrize("form,B", [(f, B) for f, Bs in tx.IM2COL_B.items() for B in Bs])
def test_im2col_bit_equal(ops, form, B):
    dtype, split = (F16 if "fp16" in form else BF16), "split" in form
    img = tx.im2col_image(B, DEV)
    want = tx.im2col_ref(img, split, dtype)
    g = Guarded(B * 196, 2304 if split else 768, dtype)
    ops.im2col_patch16(img, g.body)
    torch.cuda.synchronize()
    _same(g.out, want, f"im2col {form} B={B}")
    assert g.intact(), f"im2col {form} B={B}: wrote outside its B * 196 rows"


@pytest.mark.parametrize("M,N", tx.DGELU_MN)
def test_dgelu_mul_past_the_grid_cap(ops, M, N):
    g, codes, want = tx.dgelu_case(M, N, DEV)
    gb, gv = tx.strided(M, N, N + 4, BF16, device=DEV)
    cb, cv = tx.strided(M, N, N + 8, torch.uint8, device=DEV)
    ob, ov = tx.strided(M, N, N + 12, BF16, device=DEV)
    gv[:M], cv[:M] = g, codes
    ops.dgelu_mul(gv, cv, M, N, ov)
    torch.cuda.synchronize()
    _same(ov[:M].contiguous(), want, f"dgelu_mul {M} x {N}")
    assert tx.untouched(ob, M, N)


# --------------------------------------------------------------------------------------------------------------- softmax pooling
@pytest.mark.parametrize("B,S", tx.SOFTMAX_BS)
def test_softmax_meanpool_fwd_bwd(ops, B, S):
    C, M = tx.SOFTMAX_C, B * S
    worst = Worst("softmax_meanpool", B=B, S=S)
    dp = torch.full((B + 1, C), NAN, device=DEV)
    dp[:B] = tx.softmax_d_pooled(B, DEV)
    for scale in tx.SOFTMAX_SCALES:
        logits = torch.full((M + 2, C), NAN, device=DEV)
        logits[:M] = tx.softmax_logits(B, S, scale, DEV)
        pooled64, stats64, _ = tx.softmax_pool64(logits[:M], B, S)
        pg, sg = Guarded(B, C), Guarded(1, 2 * M, spare=0)
        ops.softmax_meanpool_fwd(logits, B, S, pg.body, sg.body[0])
        torch.cuda.synchronize()
        stats = sg.body[0].view(M, 2)
        assert torch.equal(stats[:, 0].double(), stats64[:, 0]), f"scale={scale}: the row maxima are not the maxima"
        worst.add("sum", tx.worst(stats[:, 1], stats64[:, 1], tx.BAR["softmax_sum_rel"] * stats64[:, 1]), f"scale={scale}")
        worst.add("pooled", tx.worst(pg.out, pooled64, tx.row_allowance(pooled64, tx.BAR["softmax_pooled_row"])), f"scale={scale}")
        assert pg.intact() and sg.intact()
        d64, denom = tx.softmax_pool_bwd64(logits[:M], dp[:B], B, S)
        db, dv = tx.strided(M, C, C + 8, BF16, device=DEV)
        ops.softmax_meanpool_bwd(logits, tx.softmax_stats32(logits[:M], B, S).contiguous(), dp, B, S, dv)
        torch.cuda.synchronize()
        worst.add("dlogits", tx.worst(dv[:M], d64, tx.BAR["softmax_bwd_row"] * denom + tx.half_ulp_bf16(d64)), f"scale={scale}")
        assert tx.untouched(db, M, C)
    worst.check()


# ------------------------------------------------------------------------------------------------------------------- token means
@pytest.mark.parametrize("H", tx.MEANPOOL_H)
def test_meanpool_tokens_fwd_bwd(ops, H):
    worst = Worst("meanpool_tokens", H=H)
    for S in tx.MEANPOOL_S:
        for B in tx.MEANPOOL_B:
            x = torch.full((B * S + 2, H), NAN, device=DEV)
            x[:B * S] = tx.meanpool_fwd_input(B, S, H, DEV)
            want = x[:B * S].double().view(B, S, H).mean(1)
            ob, ov = tx.strided(B, H, H + 8, BF16, device=DEV)
            ops.meanpool_tokens_fwd(x, B, S, ov)
            torch.cuda.synchronize()
            worst.add("fwd", tx.worst(ov[:B], want, tx.row_allowance(want, tx.BAR["meanpool_fwd_row"], bf16_out=True)), f"S={S} B={B}")
            assert tx.untouched(ob, B, H)
            d, want = tx.meanpool_bwd_case(B, S, H, DEV)
            db, dv = tx.strided(B, H, H + 4, F32, device=DEV)
            dv[:B] = d
            g = Guarded(B * S, H)
            ops.meanpool_tokens_bwd(dv, B, S, g.body)
            torch.cuda.synchronize()
            _same(g.out, want, f"meanpool_tokens_bwd H={H} S={S} B={B}")
            assert g.intact()
    worst.check()


# -------------------------------------------------------------------------------------------------------------------- bert_embed
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("H", tx.EMBED_H)
def test_bert_embed_bit_equal(ops, H, kind):
    for B, S in tx.EMBED_BS:
        for types in (False, True):
            c = tx.embed_case(B, S, H, kind, types, DEV)
            ref64, ref32 = tx.embed_ref(c)
            g = Guarded(B * S, H)
            ops.bert_embed(c["ids"], c["type_ids"], c["word"], c["pos"], c["typ"], g.body)
            torch.cuda.synchronize()
            _same(g.out, ref32, f"bert_embed {kind} H={H} B={B} S={S} types={types}")
            if kind == "exact":
                assert torch.equal(g.out.double(), ref64)
            assert g.intact()


# ------------------------------------------------------------------------------------------------------------------------ l2norm
@pytest.mark.parametrize("D", tx.L2_D)
def test_l2norm_fwd_bwd_per_row(ops, D):
    worst = Worst("l2norm", D=D)
    for M in tx.L2_M:
        x, dy, kinds = tx.l2norm_rows(M, D, DEV)
        y64, inv64 = tx.l2norm_fwd64(x)
        yg, ig = Guarded(M, D, spare=0), Guarded(1, M, spare=0)
        ops.l2norm_fwd(x, yg.exact(), ig.body[0])
        torch.cuda.synchronize()
        worst.add("y", tx.worst(yg.out, y64, tx.row_allowance(y64, tx.BAR["l2norm_fwd_row"])), f"M={M}")
        worst.add("inv_norm", tx.worst(ig.body[0], inv64, tx.BAR["l2norm_inv_rel"] * inv64), f"M={M}")
        if "zero" in kinds:
            assert (yg.out[kinds.index("zero")] == 0).all()
        yin, iin = y64.float().contiguous(), inv64.float().contiguous()
        dx64 = tx.l2norm_bwd64(yin, iin, dy)
        dg = Guarded(M, D, spare=0)
        ops.l2norm_bwd(yin, iin, dy, dg.exact())
        torch.cuda.synchronize()
        worst.add("dx", tx.worst(dg.out, dx64, tx.row_allowance(dx64, tx.BAR["l2norm_bwd_row"])), f"M={M}")
        assert yg.intact() and ig.intact() and dg.intact()
    worst.check()


# -------------------------------------------------------------------------------------------------------------- the small movers
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("H", tx.CLS_H)
def test_vit_cls_rows_touch_token_0_only(ops, H, dtype):
    S = tx.CLS_S
    cls = tx.real16_table(1, H, 171, DEV)[0].contiguous()
    pos = tx.hash_real((S + 1) * H, 172, DEV).float().view(S + 1, H)
    want = (cls + pos[0]).to(dtype)
    for B in tx.CLS_B:
        g = Guarded(B * S, H, dtype)
        ops.vit_cls_rows(g.body, cls, pos, B, S, H)
        torch.cuda.synchronize()
        x = g.out.view(B, S, H)
        _same(x[:, 0].contiguous(), want.expand(B, H).contiguous(), f"vit_cls_rows {dtype} H={H} B={B}")
        assert torch.isnan(x[:, 1:]).all() and g.intact(), f"vit_cls_rows {dtype} H={H} B={B}: a row other than token 0 was written"


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,pad", [(H, pad) for H in tx.WAUG_H for pad in (64, 72)])
def test_waug_set_lora_layers_three_layers(ops, H, pad, dtype):
    ld, L = H + pad, tx.WAUG_LAYERS
    ws = [Guarded(3 * H, ld, dtype, spare=1) for _ in range(L)]
    bq = [tx.real16_table(H, 4, 181 + i, DEV) for i in range(L)]
    bv = [tx.real16_table(H, 4, 191 + i, DEV) for i in range(L)]
    table = torch.tensor([[w.body.data_ptr(), q.data_ptr(), v.data_ptr()] for w, q, v in zip(ws, bq, bv)], dtype=torch.int64, device=DEV)
    ops.waug_set_lora_layers(table, L, ld, H, dtype)
    torch.cuda.synchronize()
    for i, w in enumerate(ws):
        _same(w.body[:H, H:H + 4].contiguous(), bq[i].to(dtype), f"waug layer {i}: B_q")
        _same(w.body[2 * H:3 * H, H + 4:H + 8].contiguous(), bv[i].to(dtype), f"waug layer {i}: B_v")
        rest = w.flat.clone()
        body = rest[GUARD:GUARD + w.body.numel()].view_as(w.body)
        body[:H, H:H + 4] = NAN
        body[2 * H:3 * H, H + 4:H + 8] = NAN
        assert torch.isnan(rest).all(), f"waug layer {i}: wrote outside the two LoRA-B blocks"
    with pytest.raises(RuntimeError):
        ops.waug_set_lora_layers(table, L, H + 4, H, dtype)


@pytest.mark.parametrize("H", tx.GATHER_H)
def test_gather_cast_rows(ops, H):
    for p_in, p_out, off, rows in tx.GATHER_CASES:
        need, _ = tx.gather_src_rows(rows, p_in, p_out, off)
        sb, sv = tx.strided(need, H, H + 4, F32, device=DEV)
        sv[:need] = tx.hash_real(need * H, 201, DEV).float().view(need, H)
        want = tx.gather_ref(sv[:need], rows, p_in, p_out, off)
        db, dv = tx.strided(rows, H, H + 8, BF16, device=DEV)
        ops.gather_cast_rows(sv[:need], rows, p_in, p_out, off, dv)
        torch.cuda.synchronize()
        _same(dv[:rows].contiguous(), want, f"gather_cast_rows {(p_in, p_out, off, rows)} H={H}")
        assert tx.untouched(db, rows, H)


def _up8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("mode", tx.TRANSPOSE_MODES)
def test_transpose_element_kernel(ops, mode):
    """bsclip_transpose_bf16 on operands the 16-byte kernel cannot take -- a leading dimension that is no multiple of 8, or a base one
    element (2 bytes) off a 16-byte boundary: the element kernel moves every word, and only those."""
    for R in tx.TRANSPOSE_R:
        for C in tx.TRANSPOSE_C:
            ld_in = _up8(C) + (3 if mode == "ld_in" else 8)
            ld_out = _up8(R) + (3 if mode == "ld_out" else 8)
            off_in, off_out = GUARD + (mode == "base_in"), GUARD + (mode == "base_out")
            sflat = torch.full((2 * GUARD + 1 + R * ld_in,), NAN, dtype=BF16, device=DEV)
            dflat = torch.full((2 * GUARD + 1 + C * ld_out,), NAN, dtype=BF16, device=DEV)
            src = sflat[off_in:off_in + R * ld_in].view(R, ld_in)[:, :C]
            dst = dflat[off_out:off_out + C * ld_out].view(C, ld_out)[:, :R]
            assert (src.data_ptr() % 16 != 0 or dst.data_ptr() % 16 != 0 or ld_in % 8 != 0 or ld_out % 8 != 0)
            src.copy_(tx.words16(R, C, 211, device=DEV))
            ops.transpose_bf16(src, R, C, dst)
            torch.cuda.synchronize()
            _same(dst.contiguous(), src.t().contiguous(), f"transpose {mode} R={R} C={C}")
            rest = dflat.clone()
            rest[off_out:off_out + C * ld_out].view(C, ld_out)[:, :R] = NAN
            assert torch.isnan(rest).all(), f"transpose {mode} R={R} C={C}: wrote outside its C x R block"
