"""The exact mode's encoder gates have teeth: a kernel that drops the lo term of ONE split-bf16 operand must fail them.

Each case wraps one ``ops`` function so that on its first matching call of the step -- after the kernel has run -- the lo block of
its split output is zeroed.  That is exactly what a kernel that loses the lo term produces: that one product falls back to plain
bf16 operands (2^-9 instead of 2^-16).  Before zeroing, the wrapper checks that the block really is the lo block (elementwise
|block| <= 2^-8 |hi|, and not all zero), so a wrong offset cannot zero a hi block and "pass" for the wrong reason.  The mutations
only change values inside valid tensors.

Each mutated run goes through test_20's exact-mode helper on vit_L2, txt_L4 and dna_L2 and must exceed at least one of the
EXACT_FACTOR x measured gates of test_20 (EXACT_MEASURED).  Every distance is logged next to the verdict of the old 1e-3 gate.
Measured 2026-10-16 (profiles/r07_exact_gates.jsonl): every mutation exceeds a 1.5x gate by 5.8x or more; the forward sites move the
embedding 23-170x past its gate, the backward sites (split3_transpose, dgelu_split3, attn_bwd_f32) leave the embedding alone and
move the worst gradient 5.8-32x past its gate.  The old 1e-3 gates missed 6 of the 23: the QKV dX weight and the attention
backward's dqkv split in txt_L4 and dna_L2, the fc1 dX operand (dgelu_split3) in vit_L2 and txt_L4.
The kernel-level tests of the same outputs are tests/test_12_exact_kernels_gpu.py (split3_weight, layernorm_fwd y_split3,
gelu_split3) and tests/test_10_kernels_gpu.py (attention ctx / dqkv splits, split3_transpose, dgelu_split3, split3_rows)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_20_encoders_gpu as t20  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _arg(a, k, i, name, default=None):
    return a[i] if len(a) > i else k.get(name, default)


# site -> (ops function, does this call produce the split?, (hi block, lo block) of that call's output)
def _ln_blocks(a, k, r):          # layernorm_fwd(x, gamma, beta, eps, ..., M=None, y_split3=None): [hi | lo | hi], K = H
    H, y3 = a[1].numel(), k["y_split3"]
    M = k.get("M") or a[0].shape[0]
    return y3[:M, :H], y3[:M, H:2 * H]


def _attn_fwd_blocks(a, k, r):    # attn_fwd_f32(qkv, B, S, heads, ...): ctx_split3 [hi | lo | hi], K = heads 64
    K, M, c3 = a[3] * 64, a[1] * a[2], k["ctx_split3"]
    return c3[:M, :K], c3[:M, K:2 * K]


def _attn_bwd_blocks(a, k, r):    # attn_bwd_f32(qkv, dctx, ctx, lse, B, S, heads, ...): dqkv_split3 [hi | lo | hi], K = 3 heads 64
    K, M, d3 = 3 * a[6] * 64, a[4] * a[5], k["dqkv_split3"]
    return d3[:M, :K], d3[:M, K:2 * K]


def _act_blocks(dst_index):       # gelu_split3(z, dst, ...) / dgelu_split3(dact, z, dst=...): [hi | lo | hi], K = N, M rows
    def blocks(a, k, r):
        z = a[0] if dst_index == 1 else a[1]
        dst = _arg(a, k, dst_index, "dst")
        N, M = z.shape[1], k.get("M") or z.shape[0]
        return dst[:M, :N], dst[:M, N:2 * N]
    return blocks


def _weight_blocks(a, k, r):      # split3_weight(w, dst, lora_a, lora_b): rows [hi | hi | lo]
    K, dst = a[0].shape[1], a[1]
    return dst[:, :K], dst[:, 2 * K:]


def _transpose_blocks(a, k, r):   # split3_transpose(src, dst_flat, order=1, ...) -> [C, 3 Rp] rows [hi | hi | lo]
    Rp = r.shape[1] // 3
    return r[:, :Rp], r[:, 2 * Rp:]


def _rows_blocks(a, k, r):        # split3_rows(src, dst, M, K) -> [M, 3K] = [hi | lo | hi]
    K = r.shape[1] // 3
    return r[:, :K], r[:, K:2 * K]


SITES = {
    "split3_weight_qkv_lora": ("split3_weight", lambda a, k: _arg(a, k, 2, "lora_a") is not None, _weight_blocks),
    "layernorm_fwd_y_split3": ("layernorm_fwd", lambda a, k: k.get("y_split3") is not None, _ln_blocks),
    "attn_fwd_f32_ctx_split3": ("attn_fwd_f32", lambda a, k: k.get("ctx_split3") is not None, _attn_fwd_blocks),
    "gelu_split3_dst": ("gelu_split3", lambda a, k: _arg(a, k, 1, "dst") is not None, _act_blocks(1)),
    "split3_transpose_qkv_dx": ("split3_transpose", lambda a, k: _arg(a, k, 2, "order") == 1 and _arg(a, k, 4, "lora_a") is not None,
                                _transpose_blocks),
    "dgelu_split3_dst": ("dgelu_split3", lambda a, k: _arg(a, k, 2, "dst") is not None, _act_blocks(2)),
    "attn_bwd_f32_dqkv_split3": ("attn_bwd_f32", lambda a, k: k.get("dqkv_split3") is not None, _attn_bwd_blocks),
    # the first row split of a BERT step is the head's (_ex_gemm: the text head's pooled rows, the DNA MLM head's transform input)
    "head_rows_ex_gemm": ("split3_rows", lambda a, k: True, _rows_blocks),
}
CASES = ["vit_L2", "txt_L4", "dna_L2"]
# the head row split exists in the BERT towers only (the ViT's first row split is its last block's CLS rows)
PARAMS = [(site, case) for site in SITES for case in CASES if not (site == "head_rows_ex_gemm" and case.startswith("vit"))]


def _drop_lo_once(monkeypatch, site):
    from bioscanclip.hip import ops
    name, match, blocks = SITES[site]
    orig = getattr(ops, name)
    hits = []

    def wrapper(*a, **k):
        r = orig(*a, **k)
        if not hits and match(a, k):
            hi, lo = blocks(a, k, r)
            assert hi.shape == lo.shape and lo.numel() > 0
            assert (lo.float().abs() <= 2 ** -8 * hi.float().abs()).all(), f"{site}: the block to zero is not the lo block"
            assert (lo != 0).any(), f"{site}: the lo block is already zero"
            lo.zero_()
            hits.append(tuple(lo.shape))
        return r
    monkeypatch.setattr(ops, name, wrapper)
    return hits


@pytest.mark.parametrize("site,case", PARAMS)
def test_dropping_one_lo_term_fails_the_exact_gates(site, case, monkeypatch):
    hits = _drop_lo_once(monkeypatch, site)
    e, g = t20.exact_encoder_distances(case, monkeypatch, log_name=f"exact_gate_mutation {site} {case}")
    assert len(hits) == 1, f"{site} was never called with a split output in {case}"
    m_e, m_g = t20.EXACT_MEASURED[case]
    gate_e, gate_g = t20.EXACT_FACTOR * m_e, t20.EXACT_FACTOR * m_g
    caught = e > gate_e or g > gate_g
    t20._log({"test": f"exact_gate_mutation_verdict {site} {case}", "zeroed": hits[0], "emb_vs_f32_oracle": e, "worst_grad": g,
              "gate_emb": gate_e, "gate_grad": gate_g, "emb_over_gate": e / gate_e, "grad_over_gate": g / gate_g,
              "caught_by_measured_gates": caught, "caught_by_old_1e-3": e >= 1e-3 or g >= 1e-3})
    assert caught, (site, case, e, g, gate_e, gate_g)
