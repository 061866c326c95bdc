// Multi-pair soft-target InfoNCE (gfx950): ContrastiveLoss.forward, bioscanclip/model/loss_func.py:29-54, with
// construct_label_metrix (:18-21), forward + backward in one call.
//
// loss = 1/(P N) * sum over directed pairs (a,b), a != b, of  sum_i [ cnt_i * LSE_j(s z^a_i . z^b_j) - sum_j T_ij s z^a_i . z^b_j ]
// (every directed matrix appears twice in the reference's list, which leaves the mean unchanged).
//
// The temperature (s = 1/0.07) amplifies logit error 14x, so the N x N products must be f32-accurate, but they
// should still run on the bf16 MFMA GEMM.  Each f32 operand x is split x = hi + lo (two bf16) and the product is
// formed as hi.hi + hi.lo + lo.hi by concatenating along K ([hi|hi|lo] x [hi|lo|hi]^T): one MFMA product with K = 3*768,
// relative error ~2^-16.  The second F.normalize (loss_func.py:43-44) and its Jacobian are applied here.
//
// Fused form (default; north_star's "fused logits kernel"): the logits are never written to memory.
//   pass 1, one launch per directed pair (a,b): the 256x256 ping-pong GEMM streams z^b's tiles through LDS, keeps the logits
//     tile in its MFMA accumulators and reduces row max / sum exp / sum_j T_ij x_ij in place -- in-lane, two xor shuffles
//     across the lanes that share a row, LDS across the four waves (gemm.hip, EPI_LSE_PART) -- to one (max, sum, dot) triple
//     per row and column tile; infonce_combine_kernel merges the N/256 triples of a row into LSE_i and the loss term.
//     The column statistics of (a,b) are the row statistics of the transposed pass (b,a).
//   pass 2 (only the rank's own rows): the same product again, its epilogue turns the accumulator tile into dL/dG
//     (EPI_LOSS_W: needs LSE of both directions) and writes it as the split-bf16 operand of the gradient GEMM
//     dz^a += W z^b, accumulated in f32.
// Slab form (bsclip_infonce_set_impl(1), kept for A/B timing and as a second implementation to test against): logits in row
// slabs of <= 1024 rows as f32 in the workspace, a separate row-reduce / dL/dG kernel reads them back.
// Batched slab form (the default up to 1024 padded rows, i.e. one slab): the slab form's arithmetic with the logits of all directed
// pairs kept side by side and one launch per stage over all modalities / pairs (see g_infonce_impl below).
//
// Sigmoid (SigLIP) loss with a learnable scale and bias (bsclip_sigmoid_loss_fwd_bwd, further down): the same prep kernels, split
// products and l2norm backward with elementwise kernels of its own (sig_*), in the batched and the slab form; no fused form.
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ void split_bf(float x, bf16_t& hi, bf16_t& lo) {
    hi = f2bf(x);
    lo = f2bf(x - bf2f(hi));
}

// The kernels below come in two launch forms that share their per-row code (the *_rows / *_tile / *_elems device functions): one
// launch per modality or directed pair (the slab form), and one launch over all of them with the modality / pair on a second grid
// dimension (the batched form at Np <= SLAB_ROWS).  Up to three separately allocated source tensors go by value:
struct ModPtrs {
    const float* z[3];
};
// directed pair p in [0, nmod (nmod - 1)) in the order of the (a, b) loops: a = p / (nmod - 1), b skips a
__device__ __host__ __forceinline__ void pair_ab(int p, int nmod, int& a, int& b) {
    a = p / (nmod - 1);
    b = p % (nmod - 1);
    b += (b >= a);
}

// One wave per row i in [0, Np): zn = z/max(||z||,eps) (rows >= N are zero), inv, PA = [hi|hi|lo], PB = [hi|lo|hi]
__device__ __forceinline__ void loss_prep_rows(const float* __restrict__ z, int N, int Np, int D, float* __restrict__ zn,
                                               float* __restrict__ inv, bf16_t* __restrict__ PA, bf16_t* __restrict__ PB) {
    const int lane = threadIdx.x & 63;
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (row >= Np) return;
    float scale = 0.f;
    if (row < N) {
        float ss = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(z + (size_t)row * D + c);
            ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        }
        ss = wave_sum(ss);
        scale = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
    if (lane == 0) inv[row] = scale;
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < N) v = *reinterpret_cast<const f32x4*>(z + (size_t)row * D + c) * scale;
        *reinterpret_cast<f32x4*>(zn + (size_t)row * D + c) = v;
        bf16_t h[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split_bf(v[i], h[i], l[i]);
        const uint2 hh = {(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
        const uint2 ll = {(unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16)};
        bf16_t* pa = PA + (size_t)row * 3 * D + c;
        bf16_t* pb = PB + (size_t)row * 3 * D + c;
        *reinterpret_cast<uint2*>(pa) = hh;
        *reinterpret_cast<uint2*>(pa + D) = hh;
        *reinterpret_cast<uint2*>(pa + 2 * D) = ll;
        *reinterpret_cast<uint2*>(pb) = hh;
        *reinterpret_cast<uint2*>(pb + D) = ll;
        *reinterpret_cast<uint2*>(pb + 2 * D) = hh;
    }
}
__global__ __launch_bounds__(256) void loss_prep_kernel(const float* __restrict__ z, int N, int Np, int D,
                                                         float* __restrict__ zn, float* __restrict__ inv,
                                                         bf16_t* __restrict__ PA, bf16_t* __restrict__ PB) {
    loss_prep_rows(z, N, Np, D, zn, inv, PA, PB);
}
// modality blockIdx.y; zn / inv / PA / PB are the workspace arrays of modality 0, one modality after the other
__global__ __launch_bounds__(256) void loss_prep_batched_kernel(ModPtrs src, int N, int Np, int D, float* __restrict__ zn,
                                                                 float* __restrict__ inv, bf16_t* __restrict__ PA,
                                                                 bf16_t* __restrict__ PB) {
    const size_t m = blockIdx.y;
    loss_prep_rows(src.z[m], N, Np, D, zn + m * Np * D, inv + m * Np, PA + m * Np * 3 * D, PB + m * Np * 3 * D);
}

// PBt[d, :] = [zn^T hi | zn^T lo | zn^T hi]  (bf16 [D, 3*Np]) through a 64x64 f32 LDS tile
__device__ __forceinline__ void loss_transpose_split_tile(const float* __restrict__ zn, int Np, int D, bf16_t* __restrict__ PBt) {
    __shared__ float tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;  // r over Np rows, c over D cols
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) tile[i][tx] = zn[(size_t)(r0 + i) * D + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const float v = tile[tx][i];  // zn[r0+tx][c0+i]
        bf16_t h, l;
        split_bf(v, h, l);
        bf16_t* dst = PBt + (size_t)(c0 + i) * 3 * Np + r0 + tx;
        dst[0] = h;
        dst[Np] = l;
        dst[2 * Np] = h;
    }
}
__global__ __launch_bounds__(256) void loss_transpose_split_kernel(const float* __restrict__ zn, int Np, int D,
                                                                    bf16_t* __restrict__ PBt) {
    loss_transpose_split_tile(zn, Np, D, PBt);
}
// modality blockIdx.z
__global__ __launch_bounds__(256) void loss_transpose_split_batched_kernel(const float* __restrict__ zn, int Np, int D,
                                                                            bf16_t* __restrict__ PBt) {
    const size_t m = blockIdx.z;
    loss_transpose_split_tile(zn + m * Np * D, Np, D, PBt + m * D * 3 * Np);
}

// cnt[i] = #{j : label_j == label_i}; one thread per i (N <= 8192: O(N^2) int compares, negligible)
__global__ void loss_count_kernel(const int64_t* __restrict__ labels, int N, float* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t li = labels[i];
    int c = 0;
    for (int j = 0; j < N; ++j) c += (labels[j] == li);
    cnt[i] = (float)c;
}

// One wave per row i < N of G (cosines, ld = Np): LSE_i of s*G over j < N, and contrib_i = cnt_i*LSE_i - sum_j T_ij s G_ij
// TS (trainable temperature): also tcontrib_i = sum_j (cnt_i p_ij - T_ij) G_ij, the row's term of dLoss/dt, from
// sum_j exp(x_ij - m) G_ij carried next to the sum of exponentials
template <bool TS>
__device__ __forceinline__ void loss_row_reduce_rows(const float* __restrict__ G, int row0, int nrows, int N, int Np, float s,
                                                     const int64_t* __restrict__ labels, const float* __restrict__ cnt,
                                                     float* __restrict__ lse, float* __restrict__ contrib,
                                                     float* __restrict__ tcontrib) {
    const int lane = threadIdx.x & 63;
    const int r = (blockIdx.x * 256 + threadIdx.x) >> 6;  // row inside the slab
    if (r >= nrows) return;
    const int row = row0 + r;
    const float* g = G + (size_t)r * Np;
    const int64_t li = labels[row];
    float m = -INFINITY;
    for (int j = lane; j < N; j += 64) m = fmaxf(m, g[j]);
    m = wave_max(m) * s;
    float se = 0.f, dot = 0.f, sg = 0.f;
    for (int j = lane; j < N; j += 64) {
        const float x = g[j] * s;
        se += __expf(x - m);
        if (labels[j] == li) dot += x;
        if constexpr (TS) sg += __expf(x - m) * g[j];
    }
    se = wave_sum(se);
    dot = wave_sum(dot);
    if constexpr (TS) sg = wave_sum(sg);
    const float l = m + __logf(se);
    if (lane == 0) {
        lse[row] = l;
        contrib[row] = cnt[row] * l - dot;
        if constexpr (TS) tcontrib[row] = cnt[row] * (sg / se) - dot / s;
    }
}
__global__ __launch_bounds__(256) void loss_row_reduce_kernel(const float* __restrict__ G, int row0, int nrows, int N,
                                                               int Np, float s, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ cnt, float* __restrict__ lse,
                                                               float* __restrict__ contrib) {
    loss_row_reduce_rows<false>(G, row0, nrows, N, Np, s, labels, cnt, lse, contrib, nullptr);
}
// the scale is sc[1], read here; tcontrib is indexed like contrib
__global__ __launch_bounds__(256) void loss_row_reduce_ts_kernel(const float* __restrict__ G, int row0, int nrows, int N,
                                                                  int Np, const float* __restrict__ sc,
                                                                  const int64_t* __restrict__ labels,
                                                                  const float* __restrict__ cnt, float* __restrict__ lse,
                                                                  float* __restrict__ contrib, float* __restrict__ tcontrib) {
    loss_row_reduce_rows<true>(G, row0, nrows, N, Np, sc[1], labels, cnt, lse, contrib, tcontrib);
}
// directed pair blockIdx.y: all N rows of its kept logits matrix G[p] ([Np, Np]); lse / contrib are indexed by slot a * nmod + b
__global__ __launch_bounds__(256) void loss_row_reduce_batched_kernel(const float* __restrict__ G, int nmod, int N, int Np, float s,
                                                                       const int64_t* __restrict__ labels,
                                                                       const float* __restrict__ cnt, float* __restrict__ lse,
                                                                       float* __restrict__ contrib) {
    const int p = blockIdx.y;
    int a, b;
    pair_ab(p, nmod, a, b);
    const size_t slot = a * nmod + b;
    loss_row_reduce_rows<false>(G + (size_t)p * Np * Np, 0, N, N, Np, s, labels, cnt, lse + slot * Np, contrib + slot * Np, nullptr);
}
__global__ __launch_bounds__(256) void loss_row_reduce_batched_ts_kernel(const float* __restrict__ G, int nmod, int N, int Np,
                                                                          const float* __restrict__ sc,
                                                                          const int64_t* __restrict__ labels,
                                                                          const float* __restrict__ cnt, float* __restrict__ lse,
                                                                          float* __restrict__ contrib,
                                                                          float* __restrict__ tcontrib) {
    const int p = blockIdx.y;
    int a, b;
    pair_ab(p, nmod, a, b);
    const size_t slot = a * nmod + b;
    loss_row_reduce_rows<true>(G + (size_t)p * Np * Np, 0, N, N, Np, sc[1], labels, cnt, lse + slot * Np, contrib + slot * Np,
                               tcontrib + slot * Np);
}

// W[i_local, j] = coef * ( cnt_i exp(sG - lse_ab[i]) + cnt_j exp(sG - lse_ba[j]) - 2 T_ij ), j < N, else 0,
// written as the split GEMM operand [hi | hi | lo] (bf16 [n_local, 3*Np]).
__device__ __forceinline__ void loss_w_elems(const float* __restrict__ G, int N, int Np, int row0, int n_local, float s,
                                             float coef, const int64_t* __restrict__ labels, const float* __restrict__ cnt,
                                             const float* __restrict__ lse_ab, const float* __restrict__ lse_ba,
                                             bf16_t* __restrict__ W) {
    const long total = (long)n_local * Np;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const int il = (int)(it / Np), j = (int)(it % Np);
        float w = 0.f;
        if (j < N) {
            const int i = row0 + il;
            const float x = G[(size_t)il * Np + j] * s;
            const float t = (labels[i] == labels[j]) ? 2.0f : 0.0f;
            w = coef * (cnt[i] * __expf(x - lse_ab[i]) + cnt[j] * __expf(x - lse_ba[j]) - t);
        }
        bf16_t h, l;
        split_bf(w, h, l);
        bf16_t* dst = W + (size_t)il * 3 * Np + j;
        dst[0] = h;
        dst[Np] = h;
        dst[2 * Np] = l;
    }
}
__global__ __launch_bounds__(256) void loss_w_kernel(const float* __restrict__ G, int N, int Np, int row0, int n_local,
                                                      float s, float coef, const int64_t* __restrict__ labels,
                                                      const float* __restrict__ cnt, const float* __restrict__ lse_ab,
                                                      const float* __restrict__ lse_ba, bf16_t* __restrict__ W) {
    loss_w_elems(G, N, Np, row0, n_local, s, coef, labels, cnt, lse_ab, lse_ba, W);
}
// the scale is sc[1], read here; coef = scale / den with den = P N, the host's division of the by-value form
__global__ __launch_bounds__(256) void loss_w_ts_kernel(const float* __restrict__ G, int N, int Np, int row0, int n_local,
                                                         const float* __restrict__ sc, float den,
                                                         const int64_t* __restrict__ labels, const float* __restrict__ cnt,
                                                         const float* __restrict__ lse_ab, const float* __restrict__ lse_ba,
                                                         bf16_t* __restrict__ W) {
    const float s = sc[1];
    loss_w_elems(G, N, Np, row0, n_local, s, s / den, labels, cnt, lse_ab, lse_ba, W);
}
// directed pair blockIdx.y: rows [row0, row0 + n_local) of its kept logits matrix G[p] -> W[p] ([n_local, 3 Np], w_stride apart)
__global__ __launch_bounds__(256) void loss_w_batched_kernel(const float* __restrict__ G, int nmod, int N, int Np, int row0,
                                                              int n_local, float s, float coef,
                                                              const int64_t* __restrict__ labels, const float* __restrict__ cnt,
                                                              const float* __restrict__ lse, bf16_t* __restrict__ W,
                                                              size_t w_stride) {
    const int p = blockIdx.y;
    int a, b;
    pair_ab(p, nmod, a, b);
    loss_w_elems(G + ((size_t)p * Np + row0) * Np, N, Np, row0, n_local, s, coef, labels, cnt, lse + (size_t)(a * nmod + b) * Np,
                 lse + (size_t)(b * nmod + a) * Np, W + p * w_stride);
}
__global__ __launch_bounds__(256) void loss_w_batched_ts_kernel(const float* __restrict__ G, int nmod, int N, int Np, int row0,
                                                                 int n_local, const float* __restrict__ sc, float den,
                                                                 const int64_t* __restrict__ labels,
                                                                 const float* __restrict__ cnt, const float* __restrict__ lse,
                                                                 bf16_t* __restrict__ W, size_t w_stride) {
    const int p = blockIdx.y;
    int a, b;
    pair_ab(p, nmod, a, b);
    const float s = sc[1];
    loss_w_elems(G + ((size_t)p * Np + row0) * Np, N, Np, row0, n_local, s, s / den, labels, cnt,
                 lse + (size_t)(a * nmod + b) * Np, lse + (size_t)(b * nmod + a) * Np, W + p * w_stride);
}

// loss = scale * sum over the directed pairs a != b of contrib[(a*nmod+b)*Np + i], i < N -- single workgroup, fixed order
// (bitwise reproducible).  Only entries pass 1 wrote are read: the (a,a) slots and the padding rows [N, Np) are skipped, so no
// hipMemsetAsync is needed (memset nodes inside a captured stream came back mis-ordered on replay: garbage loss, exact gradients)
__global__ __launch_bounds__(256) void loss_final_kernel(const float* __restrict__ contrib, int nmod, int Np, int N, float scale,
                                                          float* __restrict__ loss_out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int slot = 0; slot < nmod * nmod; ++slot) {
        if (slot / nmod == slot % nmod) continue;
        for (int i = threadIdx.x; i < N; i += 256) s += contrib[(size_t)slot * Np + i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] = red[0] * scale;
}

// ---- trainable temperature ----
// The scale lives in device memory as t = log s, so that a replayed graph sees each step's value.  loss_scale_kernel runs ahead of
// everything else and leaves s = exp(clamp(t, 0, ln 100)) (open_clip's range) in sc[1]; every later kernel reads it from there.
// The ends of the range are stored exactly (1 and 100), so that a clamped t gives the bits of the by-value entry at that scale.
constexpr float LN_100 = 4.60517018598809136804f;
__global__ void loss_scale_kernel(const float* __restrict__ log_scale, float* __restrict__ sc) {
    const float t = log_scale[0];
    sc[1] = t <= 0.f ? 1.0f : t >= LN_100 ? 100.0f : expf(t);
}
// loss_final_kernel's loss (the same sums in the same order: the same bits), then the rank's share of dLoss/dt:
// sc[0] = s * scale * sum over a != b and the own rows i in [row0, row0 + n_own) of tcontrib, 0 where the clamp is flat
// (t outside [0, ln 100]) or nothing is differentiated (n_own = 0).  One workgroup, fixed order, no atomics.
__global__ __launch_bounds__(256) void loss_final_ts_kernel(const float* __restrict__ contrib, const float* __restrict__ tcontrib,
                                                             int nmod, int Np, int N, int row0, int n_own, float scale,
                                                             const float* __restrict__ log_scale, float* __restrict__ sc,
                                                             float* __restrict__ loss_out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int slot = 0; slot < nmod * nmod; ++slot) {
        if (slot / nmod == slot % nmod) continue;
        for (int i = threadIdx.x; i < N; i += 256) s += contrib[(size_t)slot * Np + i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] = red[0] * scale;
    __syncthreads();
    float g = 0.f;
    for (int slot = 0; slot < nmod * nmod; ++slot) {
        if (slot / nmod == slot % nmod) continue;
        for (int i = row0 + threadIdx.x; i < row0 + n_own; i += 256) g += tcontrib[(size_t)slot * Np + i];
    }
    red[threadIdx.x] = g;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float t = log_scale[0];
        sc[0] = (n_own > 0 && t >= 0.f && t <= LN_100) ? red[0] * (sc[1] * scale) : 0.f;
    }
}

// merge the per-column-tile triples of pass 1: LSE_i = M + log sum_t s_t exp(m_t - M), contrib_i = cnt_i LSE_i - sum_t dot_t
// TS: the fourth float of a triple is sum_j exp(x_ij - m_t) G_ij over the tile; tcontrib_i as in loss_row_reduce_rows
template <bool TS>
__device__ __forceinline__ void infonce_combine_rows(const float* __restrict__ part, int N, int tiles, const float* __restrict__ cnt,
                                                     float* __restrict__ lse, float* __restrict__ contrib, float scale,
                                                     float* __restrict__ tcontrib) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const f32x4* p = reinterpret_cast<const f32x4*>(part) + (size_t)i * tiles;
    float m = -INFINITY;
    for (int t = 0; t < tiles; ++t) m = fmaxf(m, p[t][0]);
    float s = 0.f, dot = 0.f, sg = 0.f;
    for (int t = 0; t < tiles; ++t) {   // fixed order: bitwise reproducible
        const f32x4 v = p[t];
        s += v[0] == -INFINITY ? 0.f : v[1] * __expf(v[0] - m);
        if constexpr (TS) sg += v[0] == -INFINITY ? 0.f : v[3] * __expf(v[0] - m);
        dot += v[2];
    }
    const float l = m + __logf(s);
    lse[i] = l;
    contrib[i] = cnt[i] * l - dot;
    if constexpr (TS) tcontrib[i] = cnt[i] * (sg / s) - dot / scale;
}
__global__ __launch_bounds__(256) void infonce_combine_kernel(const float* __restrict__ part, int N, int tiles,
                                                              const float* __restrict__ cnt, float* __restrict__ lse,
                                                              float* __restrict__ contrib) {
    infonce_combine_rows<false>(part, N, tiles, cnt, lse, contrib, 0.f, nullptr);
}
__global__ __launch_bounds__(256) void infonce_combine_ts_kernel(const float* __restrict__ part, int N, int tiles,
                                                                 const float* __restrict__ cnt, float* __restrict__ lse,
                                                                 float* __restrict__ contrib, const float* __restrict__ sc,
                                                                 float* __restrict__ tcontrib) {
    infonce_combine_rows<true>(part, N, tiles, cnt, lse, contrib, sc[1], tcontrib);
}

// ---- sigmoid (SigLIP) loss: every cell (i, j) of a logits matrix is its own binary decision ----
// x = s G + b with s = exp(clamp(t, 0, ln 100)) as above, y = +1 where the labels agree and -1 elsewhere, term softplus(-y x),
// w = d term / dx = -y sigmoid(-y x).  t and b are read from device memory by every kernel that needs them (each forms the same s
// from the same t, so no kernel runs ahead of the others to leave it somewhere).  With u = -y x the one exponential taken is
// exp(-|u|) in (0, 1]: x reaches +-130 at s = 100 with a large |b|, where log(1 + exp(u)) and 1 / (1 + exp(-u)) overflow.
// The term is elementwise and G^{ba} = (G^{ab})^T, so the directed pairs (a, b) and (b, a) hold the same terms: the loss and the
// two scalar gradients are summed over the unordered pairs a < b and doubled.  The sums are carried in f64 (three adds per cell, a
// fixed order): the loss, dLoss/dt and dLoss/db then carry the rounding of their f32 terms and nothing from the order of summation.
__device__ __forceinline__ float sig_scale(const float* __restrict__ log_scale) {
    const float t = log_scale[0];
    return t <= 0.f ? 1.0f : t >= LN_100 ? 100.0f : expf(t);
}
__device__ __forceinline__ void sig_cell(float g, bool same, float s, float b, float& sp, float& w) {
    const float x = fmaf(s, g, b);
    const float u = same ? -x : x;
    const float e = expf(-fabsf(u));
    sp = fmaxf(u, 0.f) + log1pf(e);
    const float sg = (u >= 0.f ? 1.0f : e) / (1.0f + e);   // sigmoid(u)
    w = same ? -sg : sg;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per row i of a slab of G (cosines, ld = Np): part[3 i .. 3 i + 2] = sum_j over j < N of (softplus term, w, w G)
__device__ __forceinline__ void sig_row_reduce_rows(const float* __restrict__ G, int row0, int nrows, int N, int Np,
                                                    const float* __restrict__ log_scale, const float* __restrict__ bias,
                                                    const int64_t* __restrict__ labels, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int r = (blockIdx.x * 256 + threadIdx.x) >> 6;  // row inside the slab
    if (r >= nrows) return;
    const int row = row0 + r;
    const float* g = G + (size_t)r * Np;
    const int64_t li = labels[row];
    const float s = sig_scale(log_scale), b = bias[0];
    double asp = 0.0, aw = 0.0, awg = 0.0;
    for (int j = lane; j < N; j += 64) {
        float sp, w;
        sig_cell(g[j], labels[j] == li, s, b, sp, w);
        asp += (double)sp;
        aw += (double)w;
        awg += (double)w * (double)g[j];
    }
    asp = wave_sum_f64(asp);
    aw = wave_sum_f64(aw);
    awg = wave_sum_f64(awg);
    if (lane == 0) {
        double* p = part + (size_t)row * 3;
        p[0] = asp;
        p[1] = aw;
        p[2] = awg;
    }
}
__global__ __launch_bounds__(256) void sig_row_reduce_kernel(const float* __restrict__ G, int row0, int nrows, int N, int Np,
                                                              const float* __restrict__ log_scale, const float* __restrict__ bias,
                                                              const int64_t* __restrict__ labels, double* __restrict__ part) {
    sig_row_reduce_rows(G, row0, nrows, N, Np, log_scale, bias, labels, part);
}
// unordered pair blockIdx.y (a < b in the order (0,1), (0,2), (1,2)): all N rows of the kept logits matrix of the directed pair
// (a, b), G[a (nmod - 1) + b - 1]; part is [nu, Np, 3]
__global__ __launch_bounds__(256) void sig_row_reduce_batched_kernel(const float* __restrict__ G, int nmod, int N, int Np,
                                                                      const float* __restrict__ log_scale,
                                                                      const float* __restrict__ bias,
                                                                      const int64_t* __restrict__ labels, double* __restrict__ part) {
    const int u = blockIdx.y;
    const int a = u == 2 ? 1 : 0, b = u == 0 ? 1 : 2;
    const size_t p = a * (nmod - 1) + b - 1;
    sig_row_reduce_rows(G + p * Np * Np, 0, N, N, Np, log_scale, bias, labels, part + (size_t)u * Np * 3);
}

// W[i_local, j] = 2 s w_ij / den, j < N, else 0: dLoss/dG^{ab} + (dLoss/dG^{ba})^T with den = P N, as the split GEMM operand
// [hi | hi | lo] (bf16 [n_local, 3*Np]) of dzn^a = sum_b W^{ab} zn^b
__device__ __forceinline__ void sig_w_elems(const float* __restrict__ G, int N, int Np, int row0, int n_local,
                                            const float* __restrict__ log_scale, const float* __restrict__ bias, float den,
                                            const int64_t* __restrict__ labels, bf16_t* __restrict__ W) {
    const float s = sig_scale(log_scale), b = bias[0];
    const float coef = 2.0f * s / den;
    const long total = (long)n_local * Np;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const int il = (int)(it / Np), j = (int)(it % Np);
        float w = 0.f;
        if (j < N) {
            float sp;
            sig_cell(G[(size_t)il * Np + j], labels[row0 + il] == labels[j], s, b, sp, w);
            w *= coef;
        }
        bf16_t h, l;
        split_bf(w, h, l);
        bf16_t* dst = W + (size_t)il * 3 * Np + j;
        dst[0] = h;
        dst[Np] = h;
        dst[2 * Np] = l;
    }
}
__global__ __launch_bounds__(256) void sig_w_kernel(const float* __restrict__ G, int N, int Np, int row0, int n_local,
                                                     const float* __restrict__ log_scale, const float* __restrict__ bias, float den,
                                                     const int64_t* __restrict__ labels, bf16_t* __restrict__ W) {
    sig_w_elems(G, N, Np, row0, n_local, log_scale, bias, den, labels, W);
}
// directed pair blockIdx.y: rows [row0, row0 + n_local) of its kept logits matrix G[p] -> W[p] ([n_local, 3 Np], w_stride apart)
__global__ __launch_bounds__(256) void sig_w_batched_kernel(const float* __restrict__ G, int N, int Np, int row0, int n_local,
                                                             const float* __restrict__ log_scale, const float* __restrict__ bias,
                                                             float den, const int64_t* __restrict__ labels, bf16_t* __restrict__ W,
                                                             size_t w_stride) {
    const size_t p = blockIdx.y;
    sig_w_elems(G + (p * Np + row0) * Np, N, Np, row0, n_local, log_scale, bias, den, labels, W + p * w_stride);
}

// loss = two_over_den * sum over the nu unordered pairs and the rows i < N of part[.][i][0]; aux = (the own rows' share of dLoss/dt,
// s, the own rows' share of dLoss/db, b) with the shares summed over the rows [row0, row0 + n_own) -- single workgroup, fixed
// order, f64 (bitwise reproducible).  Only entries the row reductions wrote are read.
__global__ __launch_bounds__(256) void sig_final_kernel(const double* __restrict__ part, int nu, int Np, int N, int row0, int n_own,
                                                         double two_over_den, const float* __restrict__ log_scale,
                                                         const float* __restrict__ bias, float* __restrict__ loss_out,
                                                         float* __restrict__ aux) {
    __shared__ double red[3][256];
    double sp = 0.0, w = 0.0, wg = 0.0;
    for (int u = 0; u < nu; ++u) {
        const double* p = part + (size_t)u * Np * 3;
        for (int i = threadIdx.x; i < N; i += 256) sp += p[(size_t)i * 3];
        for (int i = row0 + threadIdx.x; i < row0 + n_own; i += 256) {
            w += p[(size_t)i * 3 + 1];
            wg += p[(size_t)i * 3 + 2];
        }
    }
    red[0][threadIdx.x] = sp;
    red[1][threadIdx.x] = w;
    red[2][threadIdx.x] = wg;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float t = log_scale[0];
        const float s = sig_scale(log_scale);
        loss_out[0] = (float)(red[0][0] * two_over_den);
        aux[0] = (n_own > 0 && t >= 0.f && t <= LN_100) ? (float)((double)s * red[2][0] * two_over_den) : 0.f;
        aux[1] = s;
        aux[2] = n_own > 0 ? (float)(red[1][0] * two_over_den) : 0.f;
        aux[3] = bias[0];
    }
}

// 0 = by size (default): below 2 048 padded rows a product is <= 8 x 8 tiles of the 256 x 256 GEMM -- at the bench's N = 256 ONE
// tile per directed pair, 255 CUs idle -- and the slab form on 128 x 128 tiles is faster (0.18 vs 0.28 ms at N = 256, 1.35 vs
// 1.27 at N = 2 048, 8.3 vs 4.5 at N = 8 192: profiles/r02_e_infonce_fused_vs_slab.log).  Up to SLAB_ROWS padded rows (one slab)
// the slab form is launched BATCHED: even on 128 x 128 tiles a product is 4 workgroups at N = 256, and the section is a strict
// chain of 41 such launches (nmod = 3) between the towers' forward and backward, where nothing overlaps with it.  The batched
// form keeps the logits of all directed pairs (pass 2 re-formed each one), and runs every stage as one launch over all
// modalities / pairs: 10 launches (9 at nmod = 2), the same device code per element, so the same bits as impl 1
// (tests/test_11_infonce_batched_gpu.py; timings: profiles/infonce_batched.jsonl);
// 1 = f32 logits slabs + separate reduce kernels, one launch per modality / pair / slab; 2 = fused epilogues
int g_infonce_impl = 0;
// BSCLIP_INFONCE_BATCHED=0: impl 0 takes the launch-by-launch slab form below SLAB_ROWS too (A/B switch, read once at load)
const bool g_infonce_batched_off = getenv("BSCLIP_INFONCE_BATCHED") && atoi(getenv("BSCLIP_INFONCE_BATCHED")) == 0;

inline int64_t align4(int64_t x) { return (x + 3) & ~(int64_t)3; }

constexpr int SLAB_ROWS = 1024;  // logits are formed [SLAB_ROWS x N] at a time: the N x N matrix never exists in HBM

struct Layout {
    int Np, slab;
    int64_t zn, inv, PA, PB, PBt, G, W, lse, contrib, cnt, dacc, part, total;
};

Layout make_layout(int N, int nmod, int D) {
    Layout L;
    L.Np = (N + 255) / 256 * 256;   // a whole number of 256-wide column tiles for the fused epilogues
    L.slab = L.Np < SLAB_ROWS ? L.Np : SLAB_ROWS;
    const int64_t Np = L.Np, SL = L.slab;
    int64_t o = 0;
    L.zn = o;      o += align4((int64_t)nmod * Np * D);
    L.inv = o;     o += align4((int64_t)nmod * Np);
    L.PA = o;      o += align4((int64_t)nmod * Np * 3 * D / 2);
    L.PB = o;      o += align4((int64_t)nmod * Np * 3 * D / 2);
    L.PBt = o;     o += align4((int64_t)nmod * D * 3 * Np / 2);
    // one slab (Np <= SLAB_ROWS): room for the logits and dL/dG of every directed pair at once (the batched form)
    const int64_t keep = Np <= SLAB_ROWS ? nmod * (nmod - 1) : 1;
    L.G = o;       o += align4(keep * SL * Np);
    L.W = o;       o += align4(keep * SL * 3 * Np / 2);
    L.lse = o;     o += align4((int64_t)nmod * nmod * Np);
    L.contrib = o; o += align4((int64_t)nmod * nmod * Np);
    L.cnt = o;     o += align4(Np);
    L.dacc = o;    o += align4((int64_t)nmod * Np * D);
    L.part = o;    o += align4(Np * (Np / 256) * 4);
    L.total = o;
    return L;
}

}  // namespace

extern "C" int64_t bsclip_infonce_workspace_floats(int N, int nmod) {
    if (N <= 0 || nmod < 2 || nmod > 3) return -1;
    return make_layout(N, nmod, 768).total;
}

// What the two entries share.  sc == nullptr: `scale` by value -- bsclip_infonce_fwd_bwd, launch for launch what it always was.
// sc != nullptr (bsclip_infonce_fwd_bwd_ts; sc is its scale_out): the same three forms with the scale read from sc[1] by every
// kernel that needs it, one launch (loss_scale_kernel) ahead of them, and pass 1 also leaves each row's term of dLoss/dt in
// `tcontrib`, which loss_final_ts_kernel sums over the rank's own rows.  tcontrib lies in the dacc region: pass 2 is its only
// other user and starts after the final kernel.  `fn` names the entry in the messages.
static int infonce_run(const char* fn, const float* const* z, int nmod, const int64_t* labels, int N, int D, float scale,
                       const float* log_scale_dev, float* sc, int row0, int n_local, float* loss_out, float* const* dz,
                       float* workspace, void* stream) {
    // reference error behaviour: loss_func.py:35-36 raises ValueError for < 2 modalities (mapped by the host layer)
    BSCLIP_REQUIRE(nmod >= 2 && nmod <= 3, "Too less element for calculating the contrastive loss.");
    BSCLIP_REQUIRE(z && labels && loss_out && workspace, "%s: null pointer", fn);
    BSCLIP_REQUIRE(D == 768, "%s: D=%d (supported: 768)", fn, D);
    BSCLIP_REQUIRE(N > 0 && N <= 16384 && row0 >= 0 && n_local >= 0 && row0 + n_local <= N,
                   "%s: N=%d row0=%d n_local=%d", fn, N, row0, n_local);
    BSCLIP_REQUIRE(aligned_to(16, workspace), "%s: workspace must be 16-B aligned", fn);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Layout L = make_layout(N, nmod, D);
    const int Np = L.Np;
    float* ws = workspace;
    float* zn = ws + L.zn;
    float* inv = ws + L.inv;
    bf16_t* PA = reinterpret_cast<bf16_t*>(ws + L.PA);
    bf16_t* PB = reinterpret_cast<bf16_t*>(ws + L.PB);
    bf16_t* PBt = reinterpret_cast<bf16_t*>(ws + L.PBt);
    float* G = ws + L.G;
    bf16_t* W = reinterpret_cast<bf16_t*>(ws + L.W);
    float* lse = ws + L.lse;
    float* contrib = ws + L.contrib;
    float* cnt = ws + L.cnt;
    float* dacc = ws + L.dacc;
    float* part = ws + L.part;
    float* tcontrib = dacc;   // sc only: [nmod * nmod, Np] like contrib (nmod Np D floats are there)
    const float den = (float)(nmod * (nmod - 1)) * (float)N;
    const bool fused = g_infonce_impl == 2 || (g_infonce_impl == 0 && Np >= 2048);
    const size_t opA = (size_t)Np * 3 * D;  // elements per modality in PA / PB
    const size_t opT = (size_t)D * 3 * Np;  // elements per modality in PBt
    const int ndir = nmod * (nmod - 1);
    const bool want_dz = dz && n_local > 0;
    const int n_own = want_dz ? n_local : 0;   // rows whose share of dLoss/dt is reported
    if (sc) hipLaunchKernelGGL(loss_scale_kernel, dim3(1), dim3(1), 0, s, log_scale_dev, sc);   // ahead of every reader of sc[1]
    // the batched form: one slab, and the GEMM would run every product on the 128x128 tile anyway (bsclip_gemm_set_tile can say no)
    const bool batched = g_infonce_impl == 0 && !g_infonce_batched_off && Np <= SLAB_ROWS &&
                         bsclip_gemm_batched_ok(N, Np, 3 * D, BSCLIP_EPI_F32) &&
                         (!want_dz || (bsclip_gemm_batched_ok(n_local, D, 3 * Np, BSCLIP_EPI_F32) &&
                                       bsclip_gemm_batched_ok(n_local, D, 3 * Np, BSCLIP_EPI_RESID_F32)));
    if (batched) {
        ModPtrs src{};
        for (int m = 0; m < nmod; ++m) {
            BSCLIP_REQUIRE(z[m], "%s: z[%d] is null", fn, m);
            src.z[m] = z[m];
        }
        hipLaunchKernelGGL(loss_prep_batched_kernel, dim3(ceil_div(Np, 4), nmod), dim3(256), 0, s, src, N, Np, D, zn, inv, PA, PB);
        if (want_dz)
            hipLaunchKernelGGL(loss_transpose_split_batched_kernel, dim3(D / 64, Np / 64, nmod), dim3(256), 0, s, zn, Np, D, PBt);
        hipLaunchKernelGGL(loss_count_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, s, labels, N, cnt);
        BSCLIP_LAUNCH_CHECK();

        // ---- pass 1: the logits of every directed pair, formed once and kept; row LSE + loss contribution ----
        const size_t g_stride = (size_t)Np * Np;                 // floats per pair in G
        const size_t w_stride = (size_t)L.slab * 3 * Np;         // bf16 elements per pair in W
        bsclip_gemm_batch gl{};
        for (int p = 0; p < ndir; ++p) {
            int a, b;
            pair_ab(p, nmod, a, b);
            gl.A[p] = PA + a * opA;
            gl.B[p] = PB + b * opA;
            gl.C[p] = G + p * g_stride;
        }
        int rc = bsclip_gemm_bf16_batched(gl, ndir, 3 * D, 3 * D, Np, N, Np, 3 * D, BSCLIP_EPI_F32, stream);
        if (rc) return rc;
        if (sc) {
            hipLaunchKernelGGL(loss_row_reduce_batched_ts_kernel, dim3(ceil_div(N, 4), ndir), dim3(256), 0, s, G, nmod, N, Np, sc,
                               labels, cnt, lse, contrib, tcontrib);
            hipLaunchKernelGGL(loss_final_ts_kernel, dim3(1), dim3(256), 0, s, contrib, tcontrib, nmod, Np, N, row0, n_own,
                               1.0f / ((float)ndir * (float)N), log_scale_dev, sc, loss_out);
        } else {
            hipLaunchKernelGGL(loss_row_reduce_batched_kernel, dim3(ceil_div(N, 4), ndir), dim3(256), 0, s, G, nmod, N, Np, scale,
                               labels, cnt, lse, contrib);
            hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, contrib, nmod, Np, N, 1.0f / ((float)ndir * (float)N),
                               loss_out);
        }
        BSCLIP_LAUNCH_CHECK();
        if (!want_dz) return BSCLIP_OK;

        // ---- pass 2: dL/dG of every pair from the kept logits, then dz_a = sum_b W_ab zn_b: the first partner written, the
        // second added (the association of the slab form: one K loop over both partners would round differently) ----
        const float coef = scale / ((float)ndir * (float)N);
        for (int a = 0; a < nmod; ++a) BSCLIP_REQUIRE(dz[a], "%s: dz[%d] is null", fn, a);
        long blocks = ((long)n_local * Np + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        if (sc)
            hipLaunchKernelGGL(loss_w_batched_ts_kernel, dim3((unsigned)blocks, ndir), dim3(256), 0, s, G, nmod, N, Np, row0, n_local,
                               sc, den, labels, cnt, lse, W, w_stride);
        else
            hipLaunchKernelGGL(loss_w_batched_kernel, dim3((unsigned)blocks, ndir), dim3(256), 0, s, G, nmod, N, Np, row0, n_local,
                               scale, coef, labels, cnt, lse, W, w_stride);
        for (int k = 0; k < nmod - 1; ++k) {   // k-th partner of every a: pair a * (nmod - 1) + k
            bsclip_gemm_batch gd{};
            for (int a = 0; a < nmod; ++a) {
                const int p = a * (nmod - 1) + k;
                int pa, b;
                pair_ab(p, nmod, pa, b);
                gd.A[a] = W + p * w_stride;
                gd.B[a] = PBt + b * opT;
                gd.C[a] = dacc + (size_t)a * Np * D;
            }
            rc = bsclip_gemm_bf16_batched(gd, nmod, 3 * Np, 3 * Np, D, n_local, D, 3 * Np,
                                          k == 0 ? BSCLIP_EPI_F32 : BSCLIP_EPI_RESID_F32, stream);
            if (rc) return rc;
        }
        // Jacobian of the in-loss F.normalize: dz = (g - zn (zn . g)) / ||z||
        bsclip_l2norm_bwd_batch nb{};
        for (int a = 0; a < nmod; ++a) {
            nb.y[a] = zn + ((size_t)a * Np + row0) * D;
            nb.inv_norm[a] = inv + (size_t)a * Np + row0;
            nb.dy[a] = dacc + (size_t)a * Np * D;
            nb.dx[a] = dz[a];
        }
        rc = bsclip_l2norm_bwd_batched(nb, nmod, n_local, D, stream);
        if (rc) return rc;
        BSCLIP_LAUNCH_CHECK();
        return BSCLIP_OK;
    }

    for (int m = 0; m < nmod; ++m) {
        BSCLIP_REQUIRE(z[m], "%s: z[%d] is null", fn, m);
        hipLaunchKernelGGL(loss_prep_kernel, dim3(ceil_div(Np, 4)), dim3(256), 0, s, z[m], N, Np, D,
                           zn + (size_t)m * Np * D, inv + (size_t)m * Np, PA + m * opA, PB + m * opA);
        if (dz && n_local > 0)
            hipLaunchKernelGGL(loss_transpose_split_kernel, dim3(D / 64, Np / 64), dim3(256), 0, s,
                               zn + (size_t)m * Np * D, Np, D, PBt + m * opT);
    }
    hipLaunchKernelGGL(loss_count_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, s, labels, N, cnt);
    BSCLIP_LAUNCH_CHECK();

    // ---- pass 1: row LSE + loss contribution of every directed pair ----
    for (int a = 0; a < nmod; ++a)
        for (int b = 0; b < nmod; ++b) {
            if (a == b) continue;
            const int slot = a * nmod + b;
            if (fused) {
                int rc = bsclip_gemm_infonce(0, PA + a * opA, 3 * D, PB + b * opA, 3 * D, nullptr, 0, N, Np, 3 * D, labels, cnt,
                                             nullptr, nullptr, part, scale, 0.f, N, 0, sc, stream);
                if (rc) return rc;
                if (sc)
                    hipLaunchKernelGGL(infonce_combine_ts_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, s, part, N, Np / 256, cnt,
                                       lse + (size_t)slot * Np, contrib + (size_t)slot * Np, sc, tcontrib + (size_t)slot * Np);
                else
                    hipLaunchKernelGGL(infonce_combine_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, s, part, N, Np / 256, cnt,
                                       lse + (size_t)slot * Np, contrib + (size_t)slot * Np);
                continue;
            }
            for (int r0 = 0; r0 < N; r0 += L.slab) {
                const int nr = N - r0 < L.slab ? N - r0 : L.slab;
                int rc = bsclip_gemm_bf16(PA + a * opA + (size_t)r0 * 3 * D, 3 * D, PB + b * opA, 3 * D, G, Np, nr, Np,
                                          3 * D, BSCLIP_EPI_F32, nullptr, stream);
                if (rc) return rc;
                if (sc)
                    hipLaunchKernelGGL(loss_row_reduce_ts_kernel, dim3(ceil_div(nr, 4)), dim3(256), 0, s, G, r0, nr, N, Np, sc,
                                       labels, cnt, lse + (size_t)slot * Np, contrib + (size_t)slot * Np,
                                       tcontrib + (size_t)slot * Np);
                else
                    hipLaunchKernelGGL(loss_row_reduce_kernel, dim3(ceil_div(nr, 4)), dim3(256), 0, s, G, r0, nr, N, Np, scale,
                                       labels, cnt, lse + (size_t)slot * Np, contrib + (size_t)slot * Np);
            }
        }
    if (sc)
        hipLaunchKernelGGL(loss_final_ts_kernel, dim3(1), dim3(256), 0, s, contrib, tcontrib, nmod, Np, N, row0, n_own,
                           1.0f / ((float)ndir * (float)N), log_scale_dev, sc, loss_out);
    else
        hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, contrib, nmod, Np, N, 1.0f / ((float)ndir * (float)N),
                           loss_out);
    BSCLIP_LAUNCH_CHECK();
    if (!dz || n_local == 0) return BSCLIP_OK;

    // ---- pass 2: d loss / d zn_a[rows row0 .. row0+n_local) = sum_b W_ab zn_b ----
    const float coef = scale / ((float)ndir * (float)N);
    for (int a = 0; a < nmod; ++a) {
        BSCLIP_REQUIRE(dz[a], "%s: dz[%d] is null", fn, a);
        float* da = dacc + (size_t)a * Np * D;
        bool first = true;
        for (int b = 0; b < nmod; ++b) {
            if (a == b) continue;
            for (int l0 = 0; l0 < n_local; l0 += L.slab) {  // row slabs of the rank's own rows
                const int nr = n_local - l0 < L.slab ? n_local - l0 : L.slab;
                int rc;
                if (fused) {
                    rc = bsclip_gemm_infonce(1, PA + a * opA + (size_t)(row0 + l0) * 3 * D, 3 * D, PB + b * opA, 3 * D, W, 3 * Np,
                                             nr, Np, 3 * D, labels, cnt, lse + (size_t)(a * nmod + b) * Np,
                                             lse + (size_t)(b * nmod + a) * Np, nullptr, scale, sc ? den : coef, N, row0 + l0, sc,
                                             stream);
                    if (rc) return rc;
                } else {
                    rc = bsclip_gemm_bf16(PA + a * opA + (size_t)(row0 + l0) * 3 * D, 3 * D, PB + b * opA, 3 * D, G, Np, nr, Np,
                                          3 * D, BSCLIP_EPI_F32, nullptr, stream);
                    if (rc) return rc;
                    long tot = (long)nr * Np;
                    long blocks = (tot + 255) / 256;
                    if (blocks > 4096) blocks = 4096;
                    if (sc)
                        hipLaunchKernelGGL(loss_w_ts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, G, N, Np, row0 + l0, nr, sc, den,
                                           labels, cnt, lse + (size_t)(a * nmod + b) * Np, lse + (size_t)(b * nmod + a) * Np, W);
                    else
                        hipLaunchKernelGGL(loss_w_kernel, dim3((unsigned)blocks), dim3(256), 0, s, G, N, Np, row0 + l0, nr, scale,
                                           coef, labels, cnt, lse + (size_t)(a * nmod + b) * Np,
                                           lse + (size_t)(b * nmod + a) * Np, W);
                }
                float* dar = da + (size_t)l0 * D;
                bsclip_epi_args ea{};
                ea.struct_size = sizeof(ea);
                ea.resid = dar;
                ea.ld_resid = D;
                rc = bsclip_gemm_bf16(W, 3 * Np, PBt + b * opT, 3 * Np, dar, D, nr, D, 3 * Np,
                                      first ? BSCLIP_EPI_F32 : BSCLIP_EPI_RESID_F32, first ? nullptr : &ea, stream);
                if (rc) return rc;
            }
            first = false;
        }
        // Jacobian of the in-loss F.normalize: dz = (g - zn (zn . g)) / ||z||
        int rc = bsclip_l2norm_bwd(zn + ((size_t)a * Np + row0) * D, inv + (size_t)a * Np + row0, da, n_local, D, dz[a],
                                   stream);
        if (rc) return rc;
    }
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_infonce_fwd_bwd(const float* const* z, int nmod, const int64_t* labels, int N, int D, float scale,
                                      int row0, int n_local, float* loss_out, float* const* dz, float* workspace,
                                      void* stream) {
    return infonce_run("bsclip_infonce_fwd_bwd", z, nmod, labels, N, D, scale, nullptr, nullptr, row0, n_local, loss_out, dz, workspace,
                       stream);
}

// Trainable temperature: the scale is exp(clamp(*log_scale_dev, 0, ln 100)), read on the device when the kernels run (bsclip.h).
extern "C" int bsclip_infonce_fwd_bwd_ts(const float* const* z, int nmod, const int64_t* labels, int N, int D,
                                         const float* log_scale_dev, int row0, int n_local, float* loss_out, float* const* dz,
                                         float* scale_out, float* workspace, void* stream) {
    // everything is checked before the first launch (infonce_run checks the rest ahead of its own)
    BSCLIP_REQUIRE(nmod >= 2 && nmod <= 3, "bsclip_infonce_fwd_bwd_ts: nmod=%d: Too less element for calculating the contrastive loss.",
                   nmod);
    BSCLIP_REQUIRE(log_scale_dev, "bsclip_infonce_fwd_bwd_ts: log_scale_dev is null");
    BSCLIP_REQUIRE(scale_out, "bsclip_infonce_fwd_bwd_ts: scale_out is null");
    BSCLIP_REQUIRE(aligned_to(4, log_scale_dev, scale_out), "bsclip_infonce_fwd_bwd_ts: log_scale_dev / scale_out must be 4-B aligned");
    BSCLIP_REQUIRE(z, "bsclip_infonce_fwd_bwd_ts: null pointer");
    for (int m = 0; m < nmod; ++m) {
        BSCLIP_REQUIRE(z[m], "bsclip_infonce_fwd_bwd_ts: z[%d] is null", m);
        BSCLIP_REQUIRE(!dz || n_local <= 0 || dz[m], "bsclip_infonce_fwd_bwd_ts: dz[%d] is null", m);
    }
    return infonce_run("bsclip_infonce_fwd_bwd_ts", z, nmod, labels, N, D, 0.f, log_scale_dev, scale_out, row0, n_local, loss_out, dz,
                       workspace, stream);
}

// Sigmoid (SigLIP) loss with a learnable scale and bias (bsclip.h).  The InfoNCE workspace and its prep kernels, products and l2norm
// backward; of the layout it uses zn / inv / PA / PB / PBt / G / W / dacc, and the row sums ([nu, Np, 3] f64, nu = nmod (nmod - 1) / 2)
// lie at the head of the dacc region, which pass 2 only writes after the final kernel has read them (as tcontrib above).  Two forms,
// the same device code per cell: batched (Np <= SLAB_ROWS: every stage one launch over all modalities / pairs, the logits of all
// directed pairs kept) and slab by slab.  bsclip_infonce_set_impl does not reach here: there is no fused-epilogue form.
// Pass 1 forms the logits of each unordered pair a < b once for the loss and the scalar gradients.  Pass 2 needs the own rows of
// every directed pair: dzn^a = sum_b (W^{ab} + (W^{ba})^T) zn^b = 2 sum_b W^{ab} zn^b over the own rows of W^{ab}, and the own
// rows of W^{ba} are columns of W^{ab} only when the own rows are all rows -- the reverse products are formed, not transposed.
extern "C" int bsclip_sigmoid_loss_fwd_bwd(const float* const* z, int nmod, const int64_t* labels, int N, int D,
                                           const float* log_scale_dev, const float* bias_dev, int row0, int n_local, float* loss_out,
                                           float* const* dz, float* aux_out, float* workspace, void* stream) {
    const char* fn = "bsclip_sigmoid_loss_fwd_bwd";
    // everything is checked before the first launch
    BSCLIP_REQUIRE(nmod >= 2 && nmod <= 3, "%s: nmod=%d: Too less element for calculating the contrastive loss.", fn, nmod);
    BSCLIP_REQUIRE(log_scale_dev, "%s: log_scale_dev is null", fn);
    BSCLIP_REQUIRE(bias_dev, "%s: bias_dev is null", fn);
    BSCLIP_REQUIRE(aux_out, "%s: aux_out is null", fn);
    BSCLIP_REQUIRE(aligned_to(4, log_scale_dev, bias_dev, aux_out), "%s: log_scale_dev / bias_dev / aux_out must be 4-B aligned", fn);
    BSCLIP_REQUIRE(z, "%s: z is null", fn);
    BSCLIP_REQUIRE(labels, "%s: labels is null", fn);
    BSCLIP_REQUIRE(loss_out, "%s: loss_out is null", fn);
    BSCLIP_REQUIRE(workspace, "%s: workspace is null", fn);
    BSCLIP_REQUIRE(D == 768, "%s: D=%d (supported: 768)", fn, D);
    BSCLIP_REQUIRE(N > 0 && N <= 16384 && row0 >= 0 && n_local >= 0 && row0 + n_local <= N, "%s: N=%d row0=%d n_local=%d", fn, N,
                   row0, n_local);
    BSCLIP_REQUIRE(aligned_to(16, workspace), "%s: workspace must be 16-B aligned", fn);
    const bool want_dz = dz && n_local > 0;
    for (int m = 0; m < nmod; ++m) {
        BSCLIP_REQUIRE(z[m], "%s: z[%d] is null", fn, m);
        BSCLIP_REQUIRE(aligned_to(16, z[m]), "%s: z[%d] must be 16-B aligned", fn, m);
        BSCLIP_REQUIRE(!want_dz || dz[m], "%s: dz[%d] is null", fn, m);
        BSCLIP_REQUIRE(!want_dz || aligned_to(16, dz[m]), "%s: dz[%d] must be 16-B aligned", fn, m);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Layout L = make_layout(N, nmod, D);
    const int Np = L.Np;
    float* ws = workspace;
    float* zn = ws + L.zn;
    float* inv = ws + L.inv;
    bf16_t* PA = reinterpret_cast<bf16_t*>(ws + L.PA);
    bf16_t* PB = reinterpret_cast<bf16_t*>(ws + L.PB);
    bf16_t* PBt = reinterpret_cast<bf16_t*>(ws + L.PBt);
    float* G = ws + L.G;
    bf16_t* W = reinterpret_cast<bf16_t*>(ws + L.W);
    float* dacc = ws + L.dacc;
    double* part = reinterpret_cast<double*>(dacc);   // [nu, Np, 3] f64 = 6 nu Np floats of the region's nmod Np D; 16-B aligned
    const int ndir = nmod * (nmod - 1), nu = ndir / 2;
    const float den = (float)ndir * (float)N;
    const double two_over_den = 2.0 / ((double)ndir * (double)N);
    const size_t opA = (size_t)Np * 3 * D;  // elements per modality in PA / PB
    const size_t opT = (size_t)D * 3 * Np;  // elements per modality in PBt
    const int n_own = want_dz ? n_local : 0;   // rows whose shares of dLoss/dt and dLoss/db are reported
    const bool batched = Np <= SLAB_ROWS && bsclip_gemm_batched_ok(N, Np, 3 * D, BSCLIP_EPI_F32) &&
                         (!want_dz || (bsclip_gemm_batched_ok(n_local, D, 3 * Np, BSCLIP_EPI_F32) &&
                                       bsclip_gemm_batched_ok(n_local, D, 3 * Np, BSCLIP_EPI_RESID_F32)));
    if (batched) {
        ModPtrs src{};
        for (int m = 0; m < nmod; ++m) src.z[m] = z[m];
        hipLaunchKernelGGL(loss_prep_batched_kernel, dim3(ceil_div(Np, 4), nmod), dim3(256), 0, s, src, N, Np, D, zn, inv, PA, PB);
        if (want_dz)
            hipLaunchKernelGGL(loss_transpose_split_batched_kernel, dim3(D / 64, Np / 64, nmod), dim3(256), 0, s, zn, Np, D, PBt);
        BSCLIP_LAUNCH_CHECK();

        // ---- pass 1: one launch forms the logits the call needs -- the unordered pairs for the loss, and with them the reverse
        // pairs when there is a backward (all N rows: one launch has one M) -- each at its directed-pair slot of G ----
        const size_t g_stride = (size_t)Np * Np;                 // floats per pair in G
        const size_t w_stride = (size_t)L.slab * 3 * Np;         // bf16 elements per pair in W
        bsclip_gemm_batch gl{};
        int nb = 0;
        for (int p = 0; p < ndir; ++p) {
            int a, b;
            pair_ab(p, nmod, a, b);
            if (!want_dz && a > b) continue;
            gl.A[nb] = PA + a * opA;
            gl.B[nb] = PB + b * opA;
            gl.C[nb] = G + p * g_stride;
            ++nb;
        }
        int rc = bsclip_gemm_bf16_batched(gl, nb, 3 * D, 3 * D, Np, N, Np, 3 * D, BSCLIP_EPI_F32, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(sig_row_reduce_batched_kernel, dim3(ceil_div(N, 4), nu), dim3(256), 0, s, G, nmod, N, Np, log_scale_dev,
                           bias_dev, labels, part);
        hipLaunchKernelGGL(sig_final_kernel, dim3(1), dim3(256), 0, s, part, nu, Np, N, row0, n_own, two_over_den, log_scale_dev,
                           bias_dev, loss_out, aux_out);
        BSCLIP_LAUNCH_CHECK();
        if (!want_dz) return BSCLIP_OK;

        // ---- pass 2: dL/dG of every directed pair from the kept logits, then dzn_a = sum_b W_ab zn_b: the first partner written,
        // the second added (the association of the slab form) ----
        long blocks = ((long)n_local * Np + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(sig_w_batched_kernel, dim3((unsigned)blocks, ndir), dim3(256), 0, s, G, N, Np, row0, n_local, log_scale_dev,
                           bias_dev, den, labels, W, w_stride);
        for (int k = 0; k < nmod - 1; ++k) {   // k-th partner of every a: pair a * (nmod - 1) + k
            bsclip_gemm_batch gd{};
            for (int a = 0; a < nmod; ++a) {
                const int p = a * (nmod - 1) + k;
                int pa, b;
                pair_ab(p, nmod, pa, b);
                gd.A[a] = W + p * w_stride;
                gd.B[a] = PBt + b * opT;
                gd.C[a] = dacc + (size_t)a * Np * D;
            }
            rc = bsclip_gemm_bf16_batched(gd, nmod, 3 * Np, 3 * Np, D, n_local, D, 3 * Np,
                                          k == 0 ? BSCLIP_EPI_F32 : BSCLIP_EPI_RESID_F32, stream);
            if (rc) return rc;
        }
        // Jacobian of the in-loss F.normalize: dz = (g - zn (zn . g)) / ||z||
        bsclip_l2norm_bwd_batch nbk{};
        for (int a = 0; a < nmod; ++a) {
            nbk.y[a] = zn + ((size_t)a * Np + row0) * D;
            nbk.inv_norm[a] = inv + (size_t)a * Np + row0;
            nbk.dy[a] = dacc + (size_t)a * Np * D;
            nbk.dx[a] = dz[a];
        }
        rc = bsclip_l2norm_bwd_batched(nbk, nmod, n_local, D, stream);
        if (rc) return rc;
        BSCLIP_LAUNCH_CHECK();
        return BSCLIP_OK;
    }

    for (int m = 0; m < nmod; ++m) {
        hipLaunchKernelGGL(loss_prep_kernel, dim3(ceil_div(Np, 4)), dim3(256), 0, s, z[m], N, Np, D, zn + (size_t)m * Np * D,
                           inv + (size_t)m * Np, PA + m * opA, PB + m * opA);
        if (want_dz)
            hipLaunchKernelGGL(loss_transpose_split_kernel, dim3(D / 64, Np / 64), dim3(256), 0, s, zn + (size_t)m * Np * D, Np, D,
                               PBt + m * opT);
    }
    BSCLIP_LAUNCH_CHECK();

    // ---- pass 1: the row sums of every unordered pair, slab by slab ----
    int u = 0;
    for (int a = 0; a < nmod; ++a)
        for (int b = a + 1; b < nmod; ++b, ++u)
            for (int r0 = 0; r0 < N; r0 += L.slab) {
                const int nr = N - r0 < L.slab ? N - r0 : L.slab;
                int rc = bsclip_gemm_bf16(PA + a * opA + (size_t)r0 * 3 * D, 3 * D, PB + b * opA, 3 * D, G, Np, nr, Np, 3 * D,
                                          BSCLIP_EPI_F32, nullptr, stream);
                if (rc) return rc;
                hipLaunchKernelGGL(sig_row_reduce_kernel, dim3(ceil_div(nr, 4)), dim3(256), 0, s, G, r0, nr, N, Np, log_scale_dev,
                                   bias_dev, labels, part + (size_t)u * Np * 3);
            }
    hipLaunchKernelGGL(sig_final_kernel, dim3(1), dim3(256), 0, s, part, nu, Np, N, row0, n_own, two_over_den, log_scale_dev, bias_dev,
                       loss_out, aux_out);
    BSCLIP_LAUNCH_CHECK();
    if (!want_dz) return BSCLIP_OK;

    // ---- pass 2: d loss / d zn_a[rows row0 .. row0+n_local) = sum_b W_ab zn_b ----
    for (int a = 0; a < nmod; ++a) {
        float* da = dacc + (size_t)a * Np * D;
        bool first = true;
        for (int b = 0; b < nmod; ++b) {
            if (a == b) continue;
            for (int l0 = 0; l0 < n_local; l0 += L.slab) {  // row slabs of the rank's own rows
                const int nr = n_local - l0 < L.slab ? n_local - l0 : L.slab;
                int rc = bsclip_gemm_bf16(PA + a * opA + (size_t)(row0 + l0) * 3 * D, 3 * D, PB + b * opA, 3 * D, G, Np, nr, Np, 3 * D,
                                          BSCLIP_EPI_F32, nullptr, stream);
                if (rc) return rc;
                long blocks = ((long)nr * Np + 255) / 256;
                if (blocks > 4096) blocks = 4096;
                hipLaunchKernelGGL(sig_w_kernel, dim3((unsigned)blocks), dim3(256), 0, s, G, N, Np, row0 + l0, nr, log_scale_dev,
                                   bias_dev, den, labels, W);
                float* dar = da + (size_t)l0 * D;
                bsclip_epi_args ea{};
                ea.struct_size = sizeof(ea);
                ea.resid = dar;
                ea.ld_resid = D;
                rc = bsclip_gemm_bf16(W, 3 * Np, PBt + b * opT, 3 * Np, dar, D, nr, D, 3 * Np,
                                      first ? BSCLIP_EPI_F32 : BSCLIP_EPI_RESID_F32, first ? nullptr : &ea, stream);
                if (rc) return rc;
            }
            first = false;
        }
        // Jacobian of the in-loss F.normalize: dz = (g - zn (zn . g)) / ||z||
        int rc = bsclip_l2norm_bwd(zn + ((size_t)a * Np + row0) * D, inv + (size_t)a * Np + row0, da, n_local, D, dz[a], stream);
        if (rc) return rc;
    }
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_infonce_set_impl(int impl) {
    BSCLIP_REQUIRE(impl >= 0 && impl <= 2, "bsclip_infonce_set_impl: %d (0 = by size, 1 = logits slabs, 2 = fused epilogues)", impl);
    g_infonce_impl = impl;
    return BSCLIP_OK;
}
