// Cross-batch memory (XBM, Wang et al., CVPR 2020) for the multi-pair InfoNCE of loss.hip (gfx950): the L2-normalised embeddings
// of the last steps stay on the GPU in a ring buffer per modality and enter the loss as extra key columns with no gradient.
//
//   x_ij = s <zn^a_i, k^b_j>,  j in C = the N own rows of b followed by the valid slots of b's bank,  T_ij = [label_i == label of j]
//   L^ab = 1/N sum_i ( cnt_i logsumexp_{j in C} x_ij - sum_{j in C} T_ij x_ij ),  loss = 1/P sum_{a != b} L^ab
//
// One modality's bank (bsclip_xbm_bank_floats(Q) = 3072 Q floats):
//   [0, 768 Q)        the normalised f32 rows by slot (the documented part)
//   [768 Q, 1920 Q)   bf16 [Q, 2304]: each row's split operand [hi | lo | hi], the B side of the logits product
//   [1920 Q, 3072 Q)  bf16 [768, 3 Q]: the transposed split operand [hi^T | lo^T | hi^T], the B side of dzn^a = W K^b
// Both split forms are written once at enqueue; a step never re-splits the bank.  head / filled live in device memory and are read
// by the kernels when they run, so a replayed graph advances the ring.
//
// The products are the library's own GEMMs on split-bf16 operands, as loss.hip forms them (hi.hi + hi.lo + lo.hi along K):
//   own logits    one product per UNORDERED pair a < b, read in both directions (G^{ba} = (G^{ab})^T)
//   bank logits   one product per ordered pair
//   dzn^a         W_own^{ab} zn^b (reduction over Np) plus W_bank^{ab} K^b (reduction over Q, up to 16 384): the latter is
//                 bsclip_gemm_splitk_f32 -- 256 x 768 outputs are three tiles, the split over the key dimension fills the chip and
//                 its partial tiles are added in a fixed order; the queries a that share a key modality b and lie next to each
//                 other in the workspace are stacked along M into one product ("runs": R = 2 at nmod = 2, 4 at nmod = 3)
// The own logits, the bank logits and the k-th partner's W_own product of every modality are each ONE launch over the pairs
// (bsclip_gemm_bf16_batched) where the shape takes the 128 x 128 tile, as at every N <= 1024 by default except the bank logits of
// ceil(N / 256) Q / 256 >= 192 tiles; one launch per product otherwise.
// Everything else is here: the ring writer, the row statistics (one WORKGROUP per row: a 16 K-column row on one wave would be the
// tail of the call), the f64 final reduction and dL/dG.  Invalid slots (slot >= filled) are selected out of the log-sum-exp, of T
// and of cnt, and their dL/dG is a stored 0; because 0 x NaN is NaN inside a product, the K^T operand of the slots that are not
// valid yet is zeroed by the call itself (xbm_scrub_kernel: nothing to do once the ring is full).
// No atomics; every sum runs in a fixed order.
//
// Launches at N = 256 (bsclip_infonce_xbm_fwd_bwd, with gradients): prep, transpose, scrub, own logits, bank logits, row statistics,
// final, dL/dG, nmod - 1 dz-own launches, 2 R split-K launches, l2norm backward = 8 + nmod + 2 R: 14 at nmod = 2, 19 at nmod = 3.
// bsclip_xbm_enqueue: 5.
#include <math.h>

#include "common.h"

namespace {

constexpr int XD = 768;                 // embedding width
constexpr int XK = 3 * XD;              // K of a split product over the embedding
constexpr float LN_100 = 4.60517018598809136804f;

struct XbmSrc {
    const float* z[3];
};
struct XbmBank {
    float* b[3];
};

__device__ __forceinline__ void split_bf(float x, bf16_t& hi, bf16_t& lo) {
    hi = f2bf(x);
    lo = f2bf(x - bf2f(hi));
}
__device__ __forceinline__ float xbm_scale(const float* __restrict__ log_scale) {
    const float t = log_scale[0];
    return t <= 0.f ? 1.0f : t >= LN_100 ? 100.0f : expf(t);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// directed pair p in [0, nmod (nmod - 1)): a = p / (nmod - 1), b skips a (the order of loss.hip)
__device__ __host__ __forceinline__ void pair_ab(int p, int nmod, int& a, int& b) {
    a = p / (nmod - 1);
    b = p % (nmod - 1);
    b += (b >= a);
}
__device__ __host__ __forceinline__ int pair_index(int a, int b, int nmod) { return a * (nmod - 1) + b - (b > a); }
// where the query modality a sits among the queries of key modality b: the (b, k) slot of the bank logits / dL/dG regions
__device__ __host__ __forceinline__ int key_slot(int a, int b, int nmod) { return b * (nmod - 1) + a - (a > b); }
// unordered pair lo < hi: (0,1), (0,2), (1,2) -> 0, 1, 2
__device__ __host__ __forceinline__ int upair_index(int lo, int hi) { return lo + hi - 1; }

// head as stored, brought into [0, Q) whatever the word holds: no slot index leaves the bank
__device__ __forceinline__ int xbm_head(const int* __restrict__ state, int Q) { return ((state[0] % Q) + Q) % Q; }
__device__ __forceinline__ bf16_t* bank_rows_split(float* bank, int Q) { return reinterpret_cast<bf16_t*>(bank + (size_t)Q * XD); }
__device__ __forceinline__ bf16_t* bank_cols_split(float* bank, int Q) {
    return reinterpret_cast<bf16_t*>(bank + (size_t)Q * XD + (size_t)Q * (XK / 2));
}

// ---- enqueue ----
// flags[m * N + row] = 1 if the row holds a non-finite value.  One wave per row, modality on blockIdx.y.
__global__ __launch_bounds__(256) void xbm_flag_kernel(XbmSrc src, int N, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (row >= N) return;
    const float* z = src.z[blockIdx.y] + (size_t)row * XD;
    float bad = 0.f;
    for (int c = lane * 4; c < XD; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) bad = fmaxf(bad, fabsf(v[i]) <= 3.402823466e38f ? 0.f : 1.f);   // false for NaN and Inf
    }
    bad = wave_max(bad);
    if (lane == 0) flags[blockIdx.y * N + row] = bad > 0.f ? 1 : 0;
}
// ok[0] = 1 if no row is flagged: one workgroup, a fixed order
__global__ __launch_bounds__(256) void xbm_decide_kernel(const int* __restrict__ flags, int n, int* __restrict__ ok) {
    __shared__ int red[256];
    int any = 0;
    for (int i = threadIdx.x; i < n; i += 256) any |= flags[i];
    red[threadIdx.x] = any;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] |= red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) ok[0] = red[0] ? 0 : 1;
}
// row i of modality blockIdx.y -> slot (head + i) % Q: zn = z / max(||z||, eps) in f32, its [hi | lo | hi] split, and the label
__global__ __launch_bounds__(256) void xbm_rows_kernel(XbmSrc src, const int64_t* __restrict__ labels, int N, int Q, XbmBank bank,
                                                        int64_t* __restrict__ bank_labels, const int* __restrict__ state,
                                                        const int* __restrict__ ok) {
    if (ok[0] == 0) return;
    const int lane = threadIdx.x & 63;
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (row >= N) return;
    const int m = blockIdx.y;
    const int slot = (xbm_head(state, Q) + row) % Q;
    const float* z = src.z[m] + (size_t)row * XD;
    float ss = 0.f;
    for (int c = lane * 4; c < XD; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + c);
        ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    ss = wave_sum(ss);
    const float scale = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    float* dst = bank.b[m] + (size_t)slot * XD;
    bf16_t* pb = bank_rows_split(bank.b[m], Q) + (size_t)slot * XK;
    for (int c = lane * 4; c < XD; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + c) * scale;
        *reinterpret_cast<f32x4*>(dst + c) = v;
        bf16_t h[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split_bf(v[i], h[i], l[i]);
        const uint2 hh = {(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
        const uint2 ll = {(unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16)};
        *reinterpret_cast<uint2*>(pb + c) = hh;
        *reinterpret_cast<uint2*>(pb + XD + c) = ll;
        *reinterpret_cast<uint2*>(pb + 2 * XD + c) = hh;
    }
    if (m == 0 && lane == 0) bank_labels[slot] = labels[row];
}
// the transposed split operand of the rows xbm_rows_kernel wrote, through a 64 x 64 f32 LDS tile: grid (768 / 64, ceil(N / 64), nmod)
__global__ __launch_bounds__(256) void xbm_cols_kernel(int N, int Q, XbmBank bank, const int* __restrict__ state,
                                                        const int* __restrict__ ok) {
    if (ok[0] == 0) return;
    __shared__ float tile[64][65];
    float* bk = bank.b[blockIdx.z];
    bf16_t* pt = bank_cols_split(bk, Q);
    const int head = xbm_head(state, Q);
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i;
        tile[i][tx] = r < N ? bk[(size_t)((head + r) % Q) * XD + c0 + tx] : 0.f;
    }
    __syncthreads();
    const int r = r0 + tx;
    if (r >= N) return;
    const int slot = (head + r) % Q;
    for (int i = ty; i < 64; i += 4) {
        bf16_t h, l;
        split_bf(tile[tx][i], h, l);
        bf16_t* dst = pt + (size_t)(c0 + i) * 3 * Q + slot;
        dst[0] = h;
        dst[Q] = l;
        dst[2 * Q] = h;
    }
}
// head and filled advance after every reader of the old head has run (stream order)
__global__ void xbm_state_kernel(int* __restrict__ state, int N, int Q, const int* __restrict__ ok) {
    if (ok[0] == 0) return;
    const int head = xbm_head(state, Q), filled = min(max(state[1], 0), Q);
    state[0] = (head + N) % Q;
    state[1] = filled + N < Q ? filled + N : Q;
}

// ---- loss ----
// One wave per row i in [0, Np) of modality blockIdx.y (loss.hip's prep): zn (rows >= N are zero), inv, PA = [hi|hi|lo], PB = [hi|lo|hi]
__global__ __launch_bounds__(256) void xbm_prep_kernel(XbmSrc src, int N, int Np, float* __restrict__ zn_all, float* __restrict__ inv_all,
                                                        bf16_t* __restrict__ PA_all, bf16_t* __restrict__ PB_all) {
    const size_t m = blockIdx.y;
    const float* z = src.z[m];
    float* zn = zn_all + m * Np * XD;
    const int lane = threadIdx.x & 63;
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (row >= Np) return;
    float scale = 0.f;
    if (row < N) {
        float ss = 0.f;
        for (int c = lane * 4; c < XD; c += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(z + (size_t)row * XD + c);
            ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        }
        ss = wave_sum(ss);
        scale = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
    if (lane == 0) inv_all[m * Np + row] = scale;
    bf16_t* pa = PA_all + (m * Np + row) * XK;
    bf16_t* pb = PB_all + (m * Np + row) * XK;
    for (int c = lane * 4; c < XD; c += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < N) v = *reinterpret_cast<const f32x4*>(z + (size_t)row * XD + c) * scale;
        *reinterpret_cast<f32x4*>(zn + (size_t)row * XD + c) = v;
        bf16_t h[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split_bf(v[i], h[i], l[i]);
        const uint2 hh = {(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
        const uint2 ll = {(unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16)};
        *reinterpret_cast<uint2*>(pa + c) = hh;
        *reinterpret_cast<uint2*>(pa + XD + c) = hh;
        *reinterpret_cast<uint2*>(pa + 2 * XD + c) = ll;
        *reinterpret_cast<uint2*>(pb + c) = hh;
        *reinterpret_cast<uint2*>(pb + XD + c) = ll;
        *reinterpret_cast<uint2*>(pb + 2 * XD + c) = hh;
    }
}
// PBt[m][d, :] = [zn^T hi | zn^T lo | zn^T hi] (bf16 [768, 3 Np]) through a 64 x 64 f32 LDS tile: grid (768 / 64, Np / 64, nmod)
__global__ __launch_bounds__(256) void xbm_transpose_kernel(const float* __restrict__ zn_all, int Np, bf16_t* __restrict__ PBt_all) {
    __shared__ float tile[64][65];
    const size_t m = blockIdx.z;
    const float* zn = zn_all + m * Np * XD;
    bf16_t* PBt = PBt_all + m * XD * 3 * Np;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) tile[i][tx] = zn[(size_t)(r0 + i) * XD + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        bf16_t h, l;
        split_bf(tile[tx][i], h, l);
        bf16_t* dst = PBt + (size_t)(c0 + i) * 3 * Np + r0 + tx;
        dst[0] = h;
        dst[Np] = l;
        dst[2 * Np] = h;
    }
}
// zero the K^T operand of the slots that are not valid: line blockIdx.x of the [768 x 3, Q] image of modality blockIdx.y
__global__ __launch_bounds__(256) void xbm_scrub_kernel(XbmBank bank, int Q, const int* __restrict__ state) {
    const int filled = min(max(state[1], 0), Q);
    bf16_t* line = bank_cols_split(bank.b[blockIdx.y], Q) + (size_t)blockIdx.x * Q;
    for (int j = filled + threadIdx.x; j < Q; j += 256) line[j] = 0;
}

// One workgroup per row i < N (blockIdx.x) of directed pair p (blockIdx.y) over the keys C: the N own columns, then the valid bank
// slots.  f32 per-thread partials, combined in f64 in a fixed order (lanes by xor shuffle, waves 0..3).  Writes lse, cnt and the
// row's terms of the loss (cnt LSE - dot) and of dLoss/dt (cnt sum_j p_ij G_ij - sum_j T_ij G_ij) as f64.
__global__ __launch_bounds__(256) void xbm_row_kernel(const float* __restrict__ Gown, const float* __restrict__ Gbank, int nmod, int N,
                                                       int Np, int Q, const float* __restrict__ log_scale,
                                                       const int64_t* __restrict__ labels, const int64_t* __restrict__ bank_labels,
                                                       const int* __restrict__ state, float* __restrict__ lse, float* __restrict__ cnt,
                                                       double* __restrict__ part) {
    __shared__ float smax[4];
    __shared__ double ssum[4][4];
    const int i = blockIdx.x, p = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int a, b;
    pair_ab(p, nmod, a, b);
    const int filled = min(max(state[1], 0), Q);
    const float s = xbm_scale(log_scale);
    // own block of the unordered pair: rows are the lower modality
    const float* go = Gown + (size_t)upair_index(a < b ? a : b, a < b ? b : a) * Np * Np;
    const size_t own_i = a < b ? (size_t)i * Np : (size_t)i, own_j = a < b ? 1 : (size_t)Np;
    const float* gb = Gbank + ((size_t)key_slot(a, b, nmod) * Np + i) * Q;
    const int64_t li = labels[i];
    float m = -INFINITY;
    for (int j = tid; j < N; j += 256) m = fmaxf(m, go[own_i + j * own_j]);
    for (int j = tid; j < filled; j += 256) m = fmaxf(m, gb[j]);
    m = wave_max(m);
    if (lane == 0) smax[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3])) * s;
    float se = 0.f, sg = 0.f, dot = 0.f, c = 0.f;
    for (int j = tid; j < N; j += 256) {
        const float g = go[own_i + j * own_j];
        const float x = g * s, e = __expf(x - m);
        se += e;
        sg += e * g;
        if (labels[j] == li) {
            dot += x;
            c += 1.f;
        }
    }
    for (int j = tid; j < filled; j += 256) {
        const float g = gb[j];
        const float x = g * s, e = __expf(x - m);
        se += e;
        sg += e * g;
        if (bank_labels[j] == li) {
            dot += x;
            c += 1.f;
        }
    }
    const double v[4] = {wave_sum_f64((double)se), wave_sum_f64((double)sg), wave_sum_f64((double)dot), wave_sum_f64((double)c)};
    if (lane == 0)
        for (int q = 0; q < 4; ++q) ssum[wave][q] = v[q];
    __syncthreads();
    if (tid == 0) {
        double t[4];
        for (int q = 0; q < 4; ++q) t[q] = ((ssum[0][q] + ssum[1][q]) + ssum[2][q]) + ssum[3][q];
        const float l = m + __logf((float)t[0]);
        const size_t o = (size_t)p * Np + i;
        lse[o] = l;
        cnt[o] = (float)t[3];
        part[o * 2] = t[3] * (double)l - t[2];
        part[o * 2 + 1] = t[3] * (t[1] / t[0]) - t[2] / (double)s;
    }
}

// loss = 1/(P N) sum of the rows' loss terms; scale_out = (dLoss/dt, s) -- one workgroup, f64, a fixed order
__global__ __launch_bounds__(256) void xbm_final_kernel(const double* __restrict__ part, int P, int Np, int N, int want_dt,
                                                         const float* __restrict__ log_scale, float* __restrict__ loss_out,
                                                         float* __restrict__ scale_out) {
    __shared__ double red[2][256];
    double sl = 0.0, st = 0.0;
    for (int p = 0; p < P; ++p)
        for (int i = threadIdx.x; i < N; i += 256) {
            const size_t o = ((size_t)p * Np + i) * 2;
            sl += part[o];
            st += part[o + 1];
        }
    red[0][threadIdx.x] = sl;
    red[1][threadIdx.x] = st;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double inv_den = 1.0 / ((double)P * (double)N);
        const float t = log_scale[0], s = xbm_scale(log_scale);
        loss_out[0] = (float)(red[0][0] * inv_den);
        scale_out[0] = (want_dt && t >= 0.f && t <= LN_100) ? (float)((double)s * red[1][0] * inv_den) : 0.f;
        scale_out[1] = s;
    }
}

// dL/dG of directed pair p = blockIdx.y over the [Np, Np + Q] cells of its key set, as the split operand [hi | hi | lo]; a thread owns
// one column and walks the rows blockIdx.z, blockIdx.z + gridDim.z, ...:
//   own  (j < Np):  coef ( cnt_i exp(x - lse_ab[i]) + cnt_j exp(x - lse_ba[j]) - 2 T_ij )   row role of (a, b) + column role of (b, a)
//   bank (j >= Np): coef ( cnt_i exp(x - lse_ab[i]) - T_ij ) for a valid slot; bank rows take no gradient, so there is no column role
// and a stored 0 for padding rows / columns and for slots that are not valid (selected: what lies in G there is never used).
__global__ __launch_bounds__(256) void xbm_w_kernel(const float* __restrict__ Gown, const float* __restrict__ Gbank, int nmod, int N,
                                                     int Np, int Q, const float* __restrict__ log_scale,
                                                     const int64_t* __restrict__ labels, const int64_t* __restrict__ bank_labels,
                                                     const int* __restrict__ state, const float* __restrict__ lse,
                                                     const float* __restrict__ cnt, bf16_t* __restrict__ Wown,
                                                     bf16_t* __restrict__ Wbank) {
    const int p = blockIdx.y;
    int a, b;
    pair_ab(p, nmod, a, b);
    const int filled = min(max(state[1], 0), Q);
    const float s = xbm_scale(log_scale);
    const float coef = s / ((float)(nmod * (nmod - 1)) * (float)N);
    const float* go = Gown + (size_t)upair_index(a < b ? a : b, a < b ? b : a) * Np * Np;
    const size_t si = a < b ? (size_t)Np : 1, sj = a < b ? 1 : (size_t)Np;
    const size_t ks = key_slot(a, b, nmod);
    const float* gb = Gbank + ks * Np * Q;
    bf16_t* wo = Wown + ks * Np * 3 * Np;
    bf16_t* wb = Wbank + ks * Np * 3 * Q;
    const float* lse_ab = lse + (size_t)p * Np;
    const float* cnt_ab = cnt + (size_t)p * Np;
    const float* lse_ba = lse + (size_t)pair_index(b, a, nmod) * Np;
    const float* cnt_ba = cnt + (size_t)pair_index(b, a, nmod) * Np;
    const int c = blockIdx.x * 256 + threadIdx.x;   // the column: own j = c < Np, bank slot j = c - Np
    if (c >= Np + Q) return;
    const bool own = c < Np;
    const int j = own ? c : c - Np;
    const bool col_ok = own ? j < N : j < filled;
    const int64_t lj = col_ok ? (own ? labels[j] : bank_labels[j]) : 0;
    const float cj = own && col_ok ? cnt_ba[j] : 0.f, lse_j = own && col_ok ? lse_ba[j] : 0.f;
    const int seg = own ? Np : Q;
    bf16_t* col = own ? wo + j : wb + j;
    for (int i = blockIdx.z; i < Np; i += gridDim.z) {
        float w = 0.f;
        if (i < N && col_ok) {
            const float x = (own ? go[i * si + j * sj] : gb[(size_t)i * Q + j]) * s;
            const bool same = labels[i] == lj;
            const float pr = cnt_ab[i] * __expf(x - lse_ab[i]);
            w = own ? coef * (pr + cj * __expf(x - lse_j) - (same ? 2.0f : 0.0f)) : coef * (pr - (same ? 1.0f : 0.0f));
        }
        bf16_t h, l;
        split_bf(w, h, l);
        bf16_t* dst = col + (size_t)i * 3 * seg;
        dst[0] = h;
        dst[seg] = h;
        dst[2 * seg] = l;
    }
}

inline int64_t align4(int64_t x) { return (x + 3) & ~(int64_t)3; }

// K-tiles (64 columns) of the 3 Q long reduction per split-K range: 6 up to Q = 4096, 12 above -- 2 .. 64 ranges
inline int xbm_splits(int Q) {
    const int kt = 3 * Q / 64;
    return kt / (Q <= 4096 ? 6 : 12);
}

struct XLayout {
    int Np;
    int64_t flags, ok, zn, inv, PA, PB, PBt, Gown, Gbank, Wown, Wbank, lse, cnt, part, dacc, partial, total;
};
XLayout xbm_layout(int N, int Q, int nmod) {
    XLayout L;
    L.Np = (N + 255) / 256 * 256;
    const int64_t Np = L.Np, P = nmod * (nmod - 1), nu = P / 2;
    int64_t o = 0;
    L.flags = o;   o += align4((int64_t)nmod * N);
    L.ok = o;      o += 4;
    L.zn = o;      o += align4(nmod * Np * XD);
    L.inv = o;     o += align4(nmod * Np);
    L.PA = o;      o += align4(nmod * Np * XK / 2);
    L.PB = o;      o += align4(nmod * Np * XK / 2);
    L.PBt = o;     o += align4(nmod * XD * 3 * Np / 2);
    L.Gown = o;    o += align4(nu * Np * Np);
    L.Gbank = o;   o += align4(P * Np * Q);
    L.Wown = o;    o += align4(P * Np * 3 * Np / 2);
    L.Wbank = o;   o += align4(P * Np * 3 * Q / 2);
    L.lse = o;     o += align4(P * Np);
    L.cnt = o;     o += align4(P * Np);
    L.part = o;    o += align4(P * Np * 4);   // f64 [P, Np, 2]
    L.dacc = o;    o += align4(nmod * Np * XD);
    L.partial = o; o += align4((int64_t)xbm_splits(Q) * (nmod - 1) * Np * XD);
    L.total = o;
    return L;
}

// nb <= 6 products C_i (+)= A_i B_i^T of one shape: ONE launch over all of them where the shape takes the 128 x 128 tile (the only
// form the batched launch has), one bsclip_gemm_bf16 per product otherwise -- the same workgroup program either way
int xbm_products(const bsclip_gemm_batch& t, int nb, int lda, int ldb, int ldc, int M, int N, int K, bool add, void* stream) {
    const int epi = add ? BSCLIP_EPI_RESID_F32 : BSCLIP_EPI_F32;
    if (bsclip_gemm_batched_ok(M, N, K, epi)) return bsclip_gemm_bf16_batched(t, nb, lda, ldb, ldc, M, N, K, epi, stream);
    for (int i = 0; i < nb; ++i) {
        bsclip_epi_args ea{};
        ea.struct_size = sizeof(ea);
        ea.resid = t.C[i];
        ea.ld_resid = ldc;
        const int rc = bsclip_gemm_bf16(t.A[i], lda, t.B[i], ldb, t.C[i], ldc, M, N, K, epi, add ? &ea : nullptr, stream);
        if (rc) return rc;
    }
    return BSCLIP_OK;
}

inline bool xbm_q_ok(int Q) { return Q >= 256 && Q <= 16384 && Q % 256 == 0; }

// what the two entry points check alike, in the order of bsclip.h; -1 names the argument
int xbm_check_common(const char* fn, const float* const* z, int nmod, const int64_t* labels, int N, int D, float* const* bank,
                     const int64_t* bank_labels, int Q, const int32_t* state_dev, const float* workspace) {
    BSCLIP_REQUIRE(nmod >= 2 && nmod <= 3, "%s: nmod=%d (2 or 3): Too less element for calculating the contrastive loss.", fn, nmod);
    BSCLIP_REQUIRE(D == XD, "%s: D=%d (supported: 768)", fn, D);
    BSCLIP_REQUIRE(N >= 1 && N <= 1024, "%s: N=%d (1 .. 1024)", fn, N);
    BSCLIP_REQUIRE(xbm_q_ok(Q), "%s: Q=%d (a multiple of 256 in 256 .. 16384)", fn, Q);
    BSCLIP_REQUIRE(N <= Q, "%s: N=%d exceeds Q=%d", fn, N, Q);
    BSCLIP_REQUIRE(z, "%s: z is null", fn);
    BSCLIP_REQUIRE(labels, "%s: labels is null", fn);
    BSCLIP_REQUIRE(bank, "%s: bank is null", fn);
    BSCLIP_REQUIRE(bank_labels, "%s: bank_labels is null", fn);
    BSCLIP_REQUIRE(state_dev, "%s: state_dev is null", fn);
    BSCLIP_REQUIRE(workspace, "%s: workspace is null", fn);
    BSCLIP_REQUIRE(aligned_to(8, labels, bank_labels), "%s: labels / bank_labels must be 8-B aligned", fn);
    BSCLIP_REQUIRE(aligned_to(4, state_dev), "%s: state_dev must be 4-B aligned", fn);
    BSCLIP_REQUIRE(aligned_to(16, workspace), "%s: workspace must be 16-B aligned", fn);
    for (int m = 0; m < nmod; ++m) {
        BSCLIP_REQUIRE(z[m], "%s: z[%d] is null", fn, m);
        BSCLIP_REQUIRE(aligned_to(16, z[m]), "%s: z[%d] must be 16-B aligned", fn, m);
        BSCLIP_REQUIRE(bank[m], "%s: bank[%d] is null", fn, m);
        BSCLIP_REQUIRE(aligned_to(16, bank[m]), "%s: bank[%d] must be 16-B aligned", fn, m);
    }
    return BSCLIP_OK;
}

}  // namespace

extern "C" int64_t bsclip_xbm_bank_floats(int Q) {
    if (!xbm_q_ok(Q)) return -1;
    return (int64_t)Q * XD + 2 * ((int64_t)Q * (XK / 2));
}

extern "C" int64_t bsclip_xbm_workspace_floats(int N, int Q, int nmod) {
    if (N < 1 || N > 1024 || !xbm_q_ok(Q) || N > Q || nmod < 2 || nmod > 3) return -1;
    return xbm_layout(N, Q, nmod).total;
}

extern "C" int bsclip_xbm_enqueue(const float* const* z, int nmod, const int64_t* labels, int N, int D, float* const* bank,
                                  int64_t* bank_labels, int Q, int32_t* state_dev, float* workspace, void* stream) {
    const char* fn = "bsclip_xbm_enqueue";
    int rc = xbm_check_common(fn, z, nmod, labels, N, D, bank, bank_labels, Q, state_dev, workspace);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const XLayout L = xbm_layout(N, Q, nmod);
    int* flags = reinterpret_cast<int*>(workspace + L.flags);
    int* ok = reinterpret_cast<int*>(workspace + L.ok);
    XbmSrc src{};
    XbmBank bk{};
    for (int m = 0; m < nmod; ++m) {
        src.z[m] = z[m];
        bk.b[m] = bank[m];
    }
    hipLaunchKernelGGL(xbm_flag_kernel, dim3(ceil_div(N, 4), nmod), dim3(256), 0, s, src, N, flags);
    hipLaunchKernelGGL(xbm_decide_kernel, dim3(1), dim3(256), 0, s, flags, nmod * N, ok);
    hipLaunchKernelGGL(xbm_rows_kernel, dim3(ceil_div(N, 4), nmod), dim3(256), 0, s, src, labels, N, Q, bk, bank_labels, state_dev, ok);
    hipLaunchKernelGGL(xbm_cols_kernel, dim3(XD / 64, ceil_div(N, 64), nmod), dim3(256), 0, s, N, Q, bk, state_dev, ok);
    hipLaunchKernelGGL(xbm_state_kernel, dim3(1), dim3(1), 0, s, state_dev, N, Q, ok);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_infonce_xbm_fwd_bwd(const float* const* z, int nmod, const int64_t* labels, int N, int D,
                                          const float* log_scale_dev, float* const* bank, const int64_t* bank_labels, int Q,
                                          const int32_t* state_dev, float* loss_out, float* const* dz, float* scale_out,
                                          float* workspace, void* stream) {
    const char* fn = "bsclip_infonce_xbm_fwd_bwd";
    // everything is checked before the first launch
    int rc = xbm_check_common(fn, z, nmod, labels, N, D, bank, bank_labels, Q, state_dev, workspace);
    if (rc) return rc;
    BSCLIP_REQUIRE(log_scale_dev, "%s: log_scale_dev is null", fn);
    BSCLIP_REQUIRE(loss_out, "%s: loss_out is null", fn);
    BSCLIP_REQUIRE(scale_out, "%s: scale_out is null", fn);
    BSCLIP_REQUIRE(aligned_to(4, log_scale_dev, loss_out, scale_out), "%s: log_scale_dev / loss_out / scale_out must be 4-B aligned", fn);
    const bool want_dz = dz != nullptr;
    for (int m = 0; m < nmod && want_dz; ++m) {
        BSCLIP_REQUIRE(dz[m], "%s: dz[%d] is null", fn, m);
        BSCLIP_REQUIRE(aligned_to(16, dz[m]), "%s: dz[%d] must be 16-B aligned", fn, m);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const XLayout L = xbm_layout(N, Q, nmod);
    const int Np = L.Np, P = nmod * (nmod - 1);
    float* ws = workspace;
    float* zn = ws + L.zn;
    float* inv = ws + L.inv;
    bf16_t* PA = reinterpret_cast<bf16_t*>(ws + L.PA);
    bf16_t* PB = reinterpret_cast<bf16_t*>(ws + L.PB);
    bf16_t* PBt = reinterpret_cast<bf16_t*>(ws + L.PBt);
    float* Gown = ws + L.Gown;
    float* Gbank = ws + L.Gbank;
    bf16_t* Wown = reinterpret_cast<bf16_t*>(ws + L.Wown);
    bf16_t* Wbank = reinterpret_cast<bf16_t*>(ws + L.Wbank);
    float* lse = ws + L.lse;
    float* cnt = ws + L.cnt;
    double* part = reinterpret_cast<double*>(ws + L.part);
    float* dacc = ws + L.dacc;
    float* partial = ws + L.partial;
    const size_t opA = (size_t)Np * XK;        // elements per modality in PA / PB
    const size_t opT = (size_t)XD * 3 * Np;    // elements per modality in PBt
    XbmSrc src{};
    XbmBank bk{};
    for (int m = 0; m < nmod; ++m) {
        src.z[m] = z[m];
        bk.b[m] = bank[m];
    }
    auto bank_rows = [&](int m) { return reinterpret_cast<const bf16_t*>(bank[m] + (size_t)Q * XD); };
    auto bank_cols = [&](int m) { return reinterpret_cast<const bf16_t*>(bank[m] + (size_t)Q * XD + (size_t)Q * (XK / 2)); };

    hipLaunchKernelGGL(xbm_prep_kernel, dim3(ceil_div(Np, 4), nmod), dim3(256), 0, s, src, N, Np, zn, inv, PA, PB);
    if (want_dz) {
        hipLaunchKernelGGL(xbm_transpose_kernel, dim3(XD / 64, Np / 64, nmod), dim3(256), 0, s, zn, Np, PBt);
        hipLaunchKernelGGL(xbm_scrub_kernel, dim3(XK, nmod), dim3(256), 0, s, bk, Q, state_dev);
    }
    BSCLIP_LAUNCH_CHECK();

    // ---- the logits: the own block of every unordered pair once, the bank block of every ordered pair ----
    bsclip_gemm_batch go{}, gb{};
    int nu = 0;
    for (int lo = 0; lo < nmod; ++lo)
        for (int hi = lo + 1; hi < nmod; ++hi, ++nu) {
            go.A[nu] = PA + lo * opA;
            go.B[nu] = PB + hi * opA;
            go.C[nu] = Gown + (size_t)upair_index(lo, hi) * Np * Np;
        }
    rc = xbm_products(go, nu, XK, XK, Np, N, Np, XK, false, stream);
    if (rc) return rc;
    for (int p = 0; p < P; ++p) {
        int a, b;
        pair_ab(p, nmod, a, b);
        gb.A[p] = PA + a * opA;
        gb.B[p] = bank_rows(b);
        gb.C[p] = Gbank + (size_t)key_slot(a, b, nmod) * Np * Q;
    }
    rc = xbm_products(gb, P, XK, XK, Q, N, Q, XK, false, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(xbm_row_kernel, dim3(N, P), dim3(256), 0, s, Gown, Gbank, nmod, N, Np, Q, log_scale_dev, labels, bank_labels,
                       state_dev, lse, cnt, part);
    hipLaunchKernelGGL(xbm_final_kernel, dim3(1), dim3(256), 0, s, part, P, Np, N, want_dz ? 1 : 0, log_scale_dev, loss_out, scale_out);
    BSCLIP_LAUNCH_CHECK();
    if (!want_dz) return BSCLIP_OK;

    // ---- dL/dG of every ordered pair, then dzn^a = sum_b ( W_own^{ab} zn^b + W_bank^{ab} K^b ) ----
    hipLaunchKernelGGL(xbm_w_kernel, dim3(ceil_div(Np + Q, 256), P, 64), dim3(256), 0, s, Gown, Gbank, nmod, N, Np, Q, log_scale_dev, labels,
                       bank_labels, state_dev, lse, cnt, Wown, Wbank);
    BSCLIP_LAUNCH_CHECK();
    // own keys: the k-th partner of every modality in one launch; the first partner is written, the second added
    for (int k = 0; k < nmod - 1; ++k) {
        bsclip_gemm_batch gd{};
        for (int a = 0; a < nmod; ++a) {
            int pa, b;
            pair_ab(a * (nmod - 1) + k, nmod, pa, b);
            gd.A[a] = Wown + (size_t)key_slot(a, b, nmod) * Np * 3 * Np;
            gd.B[a] = PBt + b * opT;
            gd.C[a] = dacc + (size_t)a * Np * XD;
        }
        rc = xbm_products(gd, nmod, 3 * Np, 3 * Np, XD, N, XD, 3 * Np, k > 0, stream);
        if (rc) return rc;
    }
    // bank keys: the split over the key dimension, its partial tiles added to the accumulator in a fixed order.  The queries a != b
    // of key modality b that lie next to each other, [a0, a0 + len), are stacked along M into one product ("runs": b = 0: {1, 2},
    // b = 1: {0}, {2}, b = 2: {0, 1} at nmod = 3); the padding rows [N, Np) between two of them hold zeros in W and whatever the
    // accumulator had, and nothing reads them
    struct Run {
        int b, a0, len;
    };
    Run runs[6];
    int nruns = 0;
    for (int b = 0; b < nmod; ++b)
        for (int a = 0; a < nmod; ++a) {
            if (a == b) continue;
            if (nruns && runs[nruns - 1].b == b && runs[nruns - 1].a0 + runs[nruns - 1].len == a) ++runs[nruns - 1].len;
            else runs[nruns++] = Run{b, a, 1};
        }
    const int splits = xbm_splits(Q);
    for (int r = 0; r < nruns; ++r) {
        const Run& R = runs[r];
        const int M = (R.len - 1) * Np + N;
        rc = bsclip_gemm_splitk_f32(Wbank + (size_t)key_slot(R.a0, R.b, nmod) * Np * 3 * Q, 3 * Q, bank_cols(R.b), 3 * Q,
                                    dacc + (size_t)R.a0 * Np * XD, XD, M, XD, 3 * Q, splits, partial, stream);
        if (rc) return rc;
    }
    // Jacobian of the in-loss F.normalize: dz = (g - zn (zn . g)) / ||z||
    bsclip_l2norm_bwd_batch nb{};
    for (int a = 0; a < nmod; ++a) {
        nb.y[a] = zn + (size_t)a * Np * XD;
        nb.inv_norm[a] = inv + (size_t)a * Np;
        nb.dy[a] = dacc + (size_t)a * Np * XD;
        nb.dx[a] = dz[a];
    }
    rc = bsclip_l2norm_bwd_batched(nb, nmod, N, XD, stream);
    if (rc) return rc;
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
