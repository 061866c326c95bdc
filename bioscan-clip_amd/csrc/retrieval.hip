// Exact inner-product top-k retrieval (gfx950) -- SURVEY.md 8f rank 1.
//
// Replaces faiss `IndexFlatIP(768).add(keys); .search(queries, max_k)` in `make_prediction`
// (reference scripts/inference_and_eval.py:414-445), including the sklearn `normalize(..., norm="l2")` of both sides
// (:416-417).  IndexFlatIP is brute force, so the restatement is exact: scores = Qn Kn^T, top max_k per query, ordered
// by descending score (ties: lower key index first).
//   * scores on the bf16 MFMA GEMM with f32-accurate split operands (x = hi + lo in bf16; hi.hi + hi.lo + lo.hi + lo.lo
//     along K = 4 D -- all four terms, so that a vector scores 1 against itself to f32 rounding), in slabs of <= 1024
//     queries so the [Q x K] matrix never exists in HBM;
//   * selection: one 64-lane wave per query row; every lane keeps a sorted top-k of its strided share in registers,
//     then k rounds of a wavefront arg-max (shuffles) merge the 64 lists.  HBM-bound: one pass over the score slab.
#include <math.h>

#include "common.h"

namespace {

constexpr int TOPK_SLAB = 1024;

// One wave per row i in [0, Np): x = z_i / ||z_i|| (zero rows and rows >= N give zeros), split x = hi + lo in bf16,
// P[i] = [lo|lo|hi|hi] (query side) or [lo|hi|lo|hi] (key side), bf16 [Np, 4 D].
template <bool KEY_SIDE>
__global__ __launch_bounds__(256) void normalize_split4_kernel(const float* __restrict__ z, int N, int Np, int D,
                                                                bf16_t* __restrict__ P) {
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
        scale = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;  // sklearn normalize leaves zero rows at zero
    }
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < N) v = *reinterpret_cast<const f32x4*>(z + (size_t)row * D + c) * scale;
        unsigned h[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bf16_t hi = f2bf(v[i]);
            h[i] = hi;
            l[i] = f2bf(v[i] - bf2f(hi));
        }
        const uint2 hh = {h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
        const uint2 ll = {l[0] | (l[1] << 16), l[2] | (l[3] << 16)};
        bf16_t* p = P + (size_t)row * 4 * D + c;
        // small terms first along K, so the f32 accumulator only becomes large for the last D columns (hi.hi)
        *reinterpret_cast<uint2*>(p) = ll;
        *reinterpret_cast<uint2*>(p + D) = KEY_SIDE ? hh : ll;
        *reinterpret_cast<uint2*>(p + 2 * D) = KEY_SIDE ? ll : hh;
        *reinterpret_cast<uint2*>(p + 3 * D) = hh;
    }
}

constexpr int TOPK_CAND = 256;  // candidate slots per row in LDS before the exact fallback scan takes over

// descending (value, then lower index first) insertion into a per-lane sorted list held in registers
template <int MAXK>
__device__ __forceinline__ void topk_insert(float (&v)[MAXK], int (&ix)[MAXK], float x, int xi) {
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
        const bool better = x > v[j] || (x == v[j] && xi < ix[j]);
        const float tv = better ? v[j] : x;
        const int ti = better ? ix[j] : xi;
        v[j] = better ? x : v[j];
        ix[j] = better ? xi : ix[j];
        x = tv;
        xi = ti;
    }
}

// One wave per query row.  Pass 1: every lane takes the maximum of its strided share (16-B loads, 4 in flight); the
// k-th largest of the 64 lane maxima is a threshold T with at least k elements >= T, so the row's top k all pass it.
// Pass 2: re-scan (the slab is L2 / Infinity-Cache resident) and compact the few elements >= T into LDS.  Pass 3: exact
// top-k of the candidates -- per-lane sorted lists in registers, then k rounds of a wavefront arg-max.  A row with more
// than TOPK_CAND candidates (many equal scores) falls back to inserting every element, which is exact for any input.
//
// SOFTMAX (bsclip_class_softmax_topk): out_s receives the softmax confidences of the k winners instead of their scores.  Pass 1
// also keeps ce_rows_kernel's per-lane running (max, sum exp) -- the lane maximum is that running maximum -- merged across the wave
// into M and S; the winners' logits are in registers at the pop loop, so conf = expf(x - M) / S needs no further pass over the row.
// Selection stays on the logits (softmax is monotone: distinct logits that round to equal confidences keep their order).  A NaN
// logit is selected as +inf (torch.topk ranks a NaN first), so every index stays inside [0, K); it makes S, and with it every
// confidence of its row, a NaN.
template <bool SOFTMAX>
__device__ __forceinline__ float topk_key(float x) {
    if constexpr (SOFTMAX) return x != x ? INFINITY : x;
    return x;
}

template <int MAXK, bool SOFTMAX = false>
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ scores, int ld, int nrows, int K, int k,
                                                         float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                         int out_ld) {
    __shared__ float cand_v[4][TOPK_CAND];
    __shared__ int cand_i[4][TOPK_CAND];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + w;
    if (r >= nrows) return;  // whole waves leave; no block-wide barrier below
    const float* row = scores + (size_t)r * ld;
    const int K4 = (K + 3) & ~3;  // ld is a multiple of 128, so the last 16-B chunk is readable; columns >= K are masked

    float m = -INFINITY;
    [[maybe_unused]] float ssum = 0.f, M = 0.f, S = 0.f;
    for (int c0 = lane * 4; c0 < K4; c0 += 1024) {
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * 256;
            x[u] = c < K4 ? *reinterpret_cast<const f32x4*>(row + c) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
        if constexpr (SOFTMAX) {
            float gm = -INFINITY;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + u * 256 + e < K) gm = fmaxf(gm, topk_key<true>(x[u][e]));
            if (gm > m) {  // the running maximum moves: rescale what has been summed (exp(-inf) = 0 on the first trip)
                ssum *= expf(m - gm);
                m = gm;
            }
            if (m > -INFINITY) {  // a share of -inf logits only adds nothing (and -inf - -inf is no exponent)
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) ssum += (c0 + u * 256 + e < K) ? expf(x[u][e] - m) : 0.f;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + u * 256 + e < K) m = fmaxf(m, x[u][e]);
        }
    }
    if constexpr (SOFTMAX) {
        M = wave_max(m);
        S = wave_sum(m == -INFINITY ? 0.f : ssum * expf(m - M));  // fixed shuffle tree: the same bits on every call
    }
    // T = k-th largest lane maximum (rank by value, ties by lane)
    int rank = 0;
    for (int j = 0; j < 64; ++j) {
        const float o = __shfl(m, j, 64);
        rank += (o > m || (o == m && j < lane)) ? 1 : 0;
    }
    const int kk = k < 64 ? k : 64;
    const unsigned long long sel = __ballot(rank == kk - 1);
    const float T = __shfl(m, __ffsll((long long)sel) - 1, 64);

    int count = 0;  // wave-uniform: every lane runs every trip and takes part in every ballot
    for (int base = 0; base < K4 && count <= TOPK_CAND; base += 256) {
        const int c0 = base + lane * 4;
        f32x4 x = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (c0 < K4) x = *reinterpret_cast<const f32x4*>(row + c0);
        bool hit = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[e] = topk_key<SOFTMAX>(x[e]);
            hit |= (c0 + e < K) && x[e] >= T;
        }
        if (__ballot(hit) == 0ull) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool h = (c0 + e < K) && x[e] >= T;
            const unsigned long long b = __ballot(h);
            const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
            if (h && pos < TOPK_CAND) {
                cand_v[w][pos] = x[e];
                cand_i[w][pos] = c0 + e;
            }
            count += __popcll(b);
        }
    }
    float v[MAXK];
    int ix[MAXK];
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
        v[j] = -INFINITY;
        ix[j] = 0x7fffffff;
    }
    if (count <= TOPK_CAND) {
        __builtin_amdgcn_wave_barrier();
        for (int c = lane; c < count; c += 64) topk_insert<MAXK>(v, ix, cand_v[w][c], cand_i[w][c]);
    } else {
        for (int c = lane; c < K; c += 64) topk_insert<MAXK>(v, ix, topk_key<SOFTMAX>(row[c]), c);
    }
    for (int o = 0; o < k; ++o) {
        float bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            const bool take = ov > bv || (ov == bv && oi < bi);
            bv = take ? ov : bv;
            bi = take ? oi : bi;
        }
        if (lane == 0) {
            if constexpr (SOFTMAX)
                out_s[(size_t)r * out_ld + o] = expf(bv - M) / S;
            else
                out_s[(size_t)r * out_ld + o] = bv;
            out_i[(size_t)r * out_ld + o] = bi;
        }
        if (ix[0] == bi) {  // the winning lane pops its head
#pragma unroll
            for (int j = 0; j + 1 < MAXK; ++j) {
                v[j] = v[j + 1];
                ix[j] = ix[j + 1];
            }
            v[MAXK - 1] = -INFINITY;
            ix[MAXK - 1] = 0x7fffffff;
        }
    }
}

inline int64_t al4(int64_t x) { return (x + 3) & ~(int64_t)3; }
inline int pad_keys(int n) { return (n + 255) / 256 * 256; }  // multiple of 256: the 256x256 ping-pong GEMM tile

}  // namespace

// top-k over the rows of a matrix the caller owns: the register lists hold 8 entries up to k = 8, 16 above
template <bool SOFTMAX>
static void launch_topk_rows(const float* m, int ld, int nrows, int K, int k, float* out_s, int64_t* out_i, hipStream_t s) {
    pick_bool(k <= 8, [&](auto small) {
        hipLaunchKernelGGL((topk_rows_kernel<decltype(small)::value ? 8 : 16, SOFTMAX>), dim3(ceil_div(nrows, 4)), dim3(256), 0, s, m, ld,
                           nrows, K, k, out_s, out_i, k);
    });
}

extern "C" int64_t bsclip_topk_ip_workspace_floats(int Q, int K, int D) {
    if (Q <= 0 || K <= 0 || D <= 0) return -1;
    const int64_t Kp = pad_keys(K), Qs = Q < TOPK_SLAB ? Q : TOPK_SLAB;
    // key operand bf16 [Kp, 4D] + query operand bf16 [Qs, 4D] + one f32 score slab [Qs, Kp]
    return al4(Kp * 2 * D) + al4(Qs * 2 * D) + al4(Qs * Kp);
}

// The query side shared by bsclip_topk_ip and bsclip_topk_ip_indexed: slabs of <= TOPK_SLAB queries against the prepared key
// operand kP (bf16 [pad_keys(K), 4 D]); ws holds the query operand and one score slab.
static int topk_search(const float* queries, int Q, const bf16_t* kP, int K, int D, int k, float* scores_out, int64_t* idx_out,
                       float* ws, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Kp = pad_keys(K);
    const int Qs = Q < TOPK_SLAB ? Q : TOPK_SLAB;
    bf16_t* qP = reinterpret_cast<bf16_t*>(ws); ws += al4((int64_t)Qs * 2 * D);
    float* sc = ws;
    for (int q0 = 0; q0 < Q; q0 += TOPK_SLAB) {
        const int nq = Q - q0 < TOPK_SLAB ? Q - q0 : TOPK_SLAB;
        hipLaunchKernelGGL((normalize_split4_kernel<false>), dim3(ceil_div(nq, 4)), dim3(256), 0, s,
                           queries + (size_t)q0 * D, nq, nq, D, qP);
        const int rc = bsclip_gemm_bf16(qP, 4 * D, kP, 4 * D, sc, Kp, nq, Kp, 4 * D, BSCLIP_EPI_F32, nullptr, stream);
        if (rc) return rc;
        launch_topk_rows<false>(sc, Kp, nq, K, k, scores_out + (size_t)q0 * k, idx_out + (size_t)q0 * k, s);
    }
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// The argument check of the two search entry points.  `indexed`: `keys` is the prebuilt key operand of bsclip_topk_ip_indexed, which
// the kernels read in 16-byte chunks; bsclip_topk_ip builds its own at the head of the workspace.
static int topk_check(const char* fn, const float* queries, const float* keys, int Q, int K, int D, int k, const float* scores_out,
                      const int64_t* idx_out, const float* workspace, bool indexed) {
    BSCLIP_REQUIRE(queries && keys && scores_out && idx_out && workspace, "%s: null pointer", fn);
    BSCLIP_REQUIRE(Q > 0 && K > 0 && D > 0 && D % 64 == 0, "%s: Q=%d K=%d D=%d (D %% 64 == 0)", fn, Q, K, D);
    BSCLIP_REQUIRE(k >= 1 && k <= 16 && k <= K, "%s: k=%d (1..16, <= K)", fn, k);
    BSCLIP_REQUIRE(aligned_to(16, workspace, indexed ? keys : nullptr), "%s: %sworkspace must be 16-B aligned", fn,
                   indexed ? "index and " : "");
    return BSCLIP_OK;
}

// The key operand of the search, bf16 [pad_keys(K), 4 D]: what bsclip_retrieval_index_build keeps and bsclip_topk_ip rebuilds per call.
static void build_key_operand(const float* keys, int K, int D, bf16_t* kP, void* stream) {
    const int Kp = pad_keys(K);
    hipLaunchKernelGGL((normalize_split4_kernel<true>), dim3(ceil_div(Kp, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       keys, K, Kp, D, kP);
}

extern "C" int bsclip_topk_ip(const float* queries, int Q, const float* keys, int K, int D, int k, float* scores_out,
                              int64_t* idx_out, float* workspace, void* stream) {
    if (const int rc = topk_check("bsclip_topk_ip", queries, keys, Q, K, D, k, scores_out, idx_out, workspace, false)) return rc;
    bf16_t* kP = reinterpret_cast<bf16_t*>(workspace);
    build_key_operand(keys, K, D, kP, stream);
    return topk_search(queries, Q, kP, K, D, k, scores_out, idx_out, workspace + al4((int64_t)pad_keys(K) * 2 * D), stream);
}

// ---- key index: the key operand of bsclip_topk_ip, built once and searched many times ------------------------------------------

extern "C" int64_t bsclip_retrieval_index_floats(int K, int D) {
    if (K <= 0 || D <= 0) return -1;
    return al4((int64_t)pad_keys(K) * 2 * D);
}

extern "C" int bsclip_retrieval_index_build(const float* keys, int K, int D, float* index, void* stream) {
    BSCLIP_REQUIRE(keys && index, "bsclip_retrieval_index_build: null pointer");
    BSCLIP_REQUIRE(K > 0 && D > 0 && D % 64 == 0, "bsclip_retrieval_index_build: K=%d D=%d (D %% 64 == 0)", K, D);
    BSCLIP_REQUIRE(aligned_to(16, keys, index),
                   "bsclip_retrieval_index_build: keys and index must be 16-B aligned");
    build_key_operand(keys, K, D, reinterpret_cast<bf16_t*>(index), stream);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// The key side for rows [row0, row0 + n) of an index the caller zero-filled: the rows a batch of key features becomes, written as
// they arrive.  A row's operand depends on that row alone (one wave per row), and the pad rows bsclip_retrieval_index_build writes
// are zero bits, so appends that cover [0, K) leave the buffer bsclip_retrieval_index_build(keys[K, D]) leaves.
extern "C" int bsclip_retrieval_index_append(const float* keys, int n, int D, float* index, int K_capacity, int row0, void* stream) {
    BSCLIP_REQUIRE(keys && index, "bsclip_retrieval_index_append: null pointer");
    BSCLIP_REQUIRE(n > 0 && K_capacity > 0 && D > 0 && D % 64 == 0, "bsclip_retrieval_index_append: n=%d K_capacity=%d D=%d (D %% 64 == 0)",
                   n, K_capacity, D);
    BSCLIP_REQUIRE(row0 >= 0 && (int64_t)row0 + n <= K_capacity, "bsclip_retrieval_index_append: row0=%d + n=%d exceeds K_capacity=%d",
                   row0, n, K_capacity);
    BSCLIP_REQUIRE(aligned_to(16, keys, index), "bsclip_retrieval_index_append: keys and index must be 16-B aligned");
    hipLaunchKernelGGL((normalize_split4_kernel<true>), dim3(ceil_div(n, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), keys, n,
                       n, D, reinterpret_cast<bf16_t*>(index) + (size_t)row0 * 4 * D);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// ---- feature tables: a batch of encoder outputs into rows [row0, row0 + B) of the split's resident tables ----------------------
// get_features_and_label (scripts/inference_and_eval.py:734-784) keeps, per split, the image / DNA / text features and two derived
// ones: averaged_feature = np.mean([image, dna], axis=0) and concatenated_feature = np.concatenate((image, dna), axis=1).

namespace {

struct FeatureRows {
    const float* in[3];  // image, dna, text: [B, D], nullable
    float* table[3];     // their [N, D] tables, null exactly where the input is
    float* avg;          // [N, D], nullable
    float* cat;          // [N, 2 D], nullable
};

// One lane per 16-byte chunk of a row; every branch on a pointer is kernel-uniform.  (a + b) * 0.5f: the sum rounds once and the
// halving is exact, which is the f32 rounding of the float64 mean numpy forms from two f32 values.
__global__ __launch_bounds__(256) void feature_rows_kernel(FeatureRows f, int B, int D4, int64_t row0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * D4) return;
    const int b = (int)(i / D4), c = (int)(i % D4) * 4, D = D4 * 4;
    const size_t src = (size_t)b * D + c, row = (size_t)(row0 + b);
    f32x4 v[3] = {};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (!f.in[m]) continue;
        v[m] = ld_stream(reinterpret_cast<const f32x4*>(f.in[m] + src));
        st_stream(f.table[m] + row * D + c, v[m]);
    }
    if (f.avg) st_stream(f.avg + row * D + c, (v[0] + v[1]) * 0.5f);
    if (f.cat) {
        st_stream(f.cat + row * 2 * D + c, v[0]);
        st_stream(f.cat + row * 2 * D + D + c, v[1]);
    }
}

}  // namespace

extern "C" int bsclip_feature_rows(const float* image, const float* dna, const float* text, int B, int D, int64_t row0, int64_t N,
                                   float* t_image, float* t_dna, float* t_text, float* t_avg, float* t_cat, void* stream) {
    BSCLIP_REQUIRE(B >= 1 && D >= 4 && D % 4 == 0, "bsclip_feature_rows: B=%d D=%d (B >= 1, D %% 4 == 0)", B, D);
    BSCLIP_REQUIRE(row0 >= 0, "bsclip_feature_rows: row0=%lld (>= 0)", (long long)row0);
    BSCLIP_REQUIRE(row0 <= N - B, "bsclip_feature_rows: row0=%lld + B=%d exceeds N=%lld", (long long)row0, B, (long long)N);
    BSCLIP_REQUIRE(image || dna || text, "bsclip_feature_rows: no input (image, dna and text are all null)");
    BSCLIP_REQUIRE(!image == !t_image, "bsclip_feature_rows: image and t_image must be given together");
    BSCLIP_REQUIRE(!dna == !t_dna, "bsclip_feature_rows: dna and t_dna must be given together");
    BSCLIP_REQUIRE(!text == !t_text, "bsclip_feature_rows: text and t_text must be given together");
    BSCLIP_REQUIRE(!t_avg || (image && dna), "bsclip_feature_rows: t_avg needs both image and dna");
    BSCLIP_REQUIRE(!t_cat || (image && dna), "bsclip_feature_rows: t_cat needs both image and dna");
    BSCLIP_REQUIRE(aligned_to(16, image, dna, text, t_image, t_dna, t_text, t_avg, t_cat),
                   "bsclip_feature_rows: inputs and tables must be 16-B aligned");
    const FeatureRows f = {{image, dna, text}, {t_image, t_dna, t_text}, t_avg, t_cat};
    const int64_t chunks = (int64_t)B * (D / 4);
    BSCLIP_REQUIRE(chunks <= (int64_t)0x7fffffff * 256, "bsclip_feature_rows: B=%d x D=%d is too large for one launch", B, D);
    hipLaunchKernelGGL(feature_rows_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), f, B,
                       D / 4, row0);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int64_t bsclip_topk_ip_indexed_workspace_floats(int Q, int K, int D) {
    if (Q <= 0 || K <= 0 || D <= 0) return -1;
    const int64_t Kp = pad_keys(K), Qs = Q < TOPK_SLAB ? Q : TOPK_SLAB;
    return al4(Qs * 2 * D) + al4(Qs * Kp);  // query operand bf16 [Qs, 4D] + one f32 score slab [Qs, Kp]
}

extern "C" int bsclip_topk_ip_indexed(const float* queries, int Q, const float* index, int K, int D, int k, float* scores_out,
                                      int64_t* idx_out, float* workspace, void* stream) {
    if (const int rc = topk_check("bsclip_topk_ip_indexed", queries, index, Q, K, D, k, scores_out, idx_out, workspace, true)) return rc;
    return topk_search(queries, Q, reinterpret_cast<const bf16_t*>(index), K, D, k, scores_out, idx_out, workspace, stream);
}

// ---- top-k over class logits (supervised fine-tuning: evaluate_epoch's argsort(output, descending)[:, :max(k)]) ---------------
// The selection kernel of the retrieval search on a logits matrix the caller owns: its 16-byte chunk loads need 16-byte aligned
// rows (ldc % 4 == 0) and ldc >= C rounded up to 4, which ldc >= C and ldc % 4 == 0 give; columns >= C are masked.

template <bool SOFTMAX>
static int class_topk_checked(const char* fn, const float* logits, int ldc, int B, int C, int k, float* out_s, int64_t* idx_out,
                              void* stream) {
    const char* out_name = SOFTMAX ? "conf_out" : "scores_out";
    BSCLIP_REQUIRE(logits && out_s && idx_out, "%s: null pointer", fn);
    BSCLIP_REQUIRE(B >= 1 && C >= 1, "%s: B=%d C=%d (both >= 1)", fn, B, C);
    BSCLIP_REQUIRE(k >= 1 && k <= 16 && k <= C, "%s: k=%d (1..16, <= C=%d)", fn, k, C);
    BSCLIP_REQUIRE(ldc >= C && ldc % 4 == 0, "%s: ldc=%d (>= C=%d, a multiple of 4)", fn, ldc, C);
    BSCLIP_REQUIRE(aligned_to(16, logits) && aligned_to(4, out_s) && aligned_to(8, idx_out),
                   "%s: logits must be 16-byte, %s 4-byte, idx_out 8-byte aligned", fn, out_name);
    launch_topk_rows<SOFTMAX>(logits, ldc, B, C, k, out_s, idx_out, static_cast<hipStream_t>(stream));
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_class_topk(const float* logits, int ldc, int B, int C, int k, float* scores_out, int64_t* idx_out,
                                 void* stream) {
    return class_topk_checked<false>("bsclip_class_topk", logits, ldc, B, C, k, scores_out, idx_out, stream);
}

// ---- softmax confidences of the k highest class logits (method two: reference scripts/method_two_fine_tuning_and_eval.py:57-62,
// `F.softmax(output, dim=-1)` then `torch.topk(..., k=5, dim=1, largest=True, sorted=True)`) -------------------------------------
// The selection kernel above with SOFTMAX set: the same layout contract as bsclip_class_topk.  Order: by logit descending, ties to the
// lower class index.

extern "C" int bsclip_class_softmax_topk(const float* logits, int ldc, int B, int C, int k, float* conf_out, int64_t* idx_out,
                                         void* stream) {
    return class_topk_checked<true>("bsclip_class_softmax_topk", logits, ldc, B, C, k, conf_out, idx_out, stream);
}

// ---- scoring on integer label ids (make_prediction's label lookup + top_k_micro_accuracy / top_k_macro_accuracy counts) -------

namespace {

constexpr int EVAL_MAX_LEVELS = 8;
constexpr int EVAL_MAX_K = 8;
constexpr int EVAL_FLAG_BAD_IDX = 1;    // an idx entry outside [0, K)
constexpr int EVAL_FLAG_BAD_LABEL = 2;  // a query label outside its level's class range

struct RankSlot {
    int q, r, sub;  // the query, the rank this lane owns and the query's 16-lane group inside the wave
    int64_t id;     // idx[q, r]
    bool ok;        // r < k of a query < Q and id inside [0, K)
};

// 16 lanes per query (4 queries per wave, 16 per block); lane r < k owns rank r.  An idx outside [0, K) is flagged, never dereferenced.
__device__ __forceinline__ RankSlot rank_slot(const int64_t* __restrict__ idx, int Q, int k, int K, int* __restrict__ flag) {
    const int lane = threadIdx.x & 63, sub = lane >> 4, r = lane & 15;
    const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool inq = q < Q && r < k;
    const int64_t id = inq ? idx[(size_t)q * k + r] : 0;
    const bool ok = inq && id >= 0 && id < K;
    if (inq && !ok) atomicOr(flag, EVAL_FLAG_BAD_IDX);
    return {q, r, sub, id, ok};
}

// Every lane gathers the L labels of its slot's key and a ballot per level says which ranks carry the query's label;
// store(q * L + l, g) receives the 16 bits of the query's lane group.
template <class Store>
__device__ __forceinline__ void match_levels(const RankSlot s, const int* __restrict__ key_labels, const int* __restrict__ query_labels,
                                             int Q, int L, Store store) {
    const int q = s.q, r = s.r, sub = s.sub;
    const int64_t id = s.id;
    const bool ok = s.ok;
    int kl[EVAL_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < EVAL_MAX_LEVELS; ++l) kl[l] = (ok && l < L) ? key_labels[(size_t)id * L + l] : 0;
#pragma unroll
    for (int l = 0; l < EVAL_MAX_LEVELS; ++l) {
        if (l >= L) break;  // wave-uniform
        const int ql = q < Q ? query_labels[(size_t)q * L + l] : 0;
        const unsigned long long b = __ballot(ok && kl[l] == ql);
        if (r == l && q < Q) store((size_t)q * L + l, (unsigned)(b >> (sub * 16)) & 0xffffu);
    }
}

// hit_rank[q, l] = the first rank whose level-l label equals the query's, or k
__global__ __launch_bounds__(256) void hit_ranks_kernel(const int64_t* __restrict__ idx, int Q, int k,
                                                         const int* __restrict__ key_labels, int K,
                                                         const int* __restrict__ query_labels, int L, int* __restrict__ hit_rank,
                                                         int* __restrict__ flag) {
    match_levels(rank_slot(idx, Q, k, K, flag), key_labels, query_labels, Q, L,
                 [=](size_t at, unsigned g) { hit_rank[at] = g ? __ffs(g) - 1 : k; });
}

struct CountCfg {
    int off[EVAL_MAX_LEVELS + 1];
    int kl[EVAL_MAX_K];
};

// blockIdx.y = level, one lane per query.  The lanes of a wave that hold the same class are counted with ballots and their
// first lane adds the sums, so a level with few classes (order) does not serialise Q atomics on a handful of addresses.
__global__ __launch_bounds__(256) void class_counts_kernel(const int* __restrict__ hit_rank, const int* __restrict__ query_labels,
                                                            int Q, int L, CountCfg cfg, int nk, int* __restrict__ seen,
                                                            int* __restrict__ right, int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int C = cfg.off[L];
    int c = -1, h = 0;
    if (q < Q) {
        const int lab = query_labels[(size_t)q * L + l];
        if (lab >= 0 && lab < cfg.off[l + 1] - cfg.off[l]) {
            c = cfg.off[l] + lab;
            h = hit_rank[(size_t)q * L + l];
        } else {
            atomicOr(flag, EVAL_FLAG_BAD_LABEL);
        }
    }
    unsigned long long todo = __ballot(c >= 0);  // wave-uniform loop: every lane runs every trip
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int c0 = __shfl(c, lead, 64);
        const bool same = c == c0;
        const unsigned long long m = __ballot(same);
        if (lane == lead) atomicAdd(seen + c0, __popcll(m));
        for (int j = 0; j < nk; ++j) {
            const unsigned long long hit = __ballot(same && h < cfg.kl[j]);
            if (lane == lead && hit) atomicAdd(right + (size_t)j * C + c0, __popcll(hit));
        }
        todo &= ~m;
    }
}


// ---- method-one evaluation (reference scripts/method_one_eval.py): label matches as bit masks, the merge at a threshold, the sweep --

constexpr int EVAL_SWEEP_CHUNK = 64;  // thresholds per block of the sweep (blockIdx.y)

// The lane layout of hit_ranks_kernel, but the ballot itself is the output: bit r of bits[q, l] is set exactly when the level-l
// label of key idx[q, r] equals the query's.  With a member table the only column read is `level` and bit r of bits[q] says
// whether that label is listed (member[label] != 0); a label outside [0, C) is flagged and never used as an index.
__global__ __launch_bounds__(256) void match_bits_kernel(const int64_t* __restrict__ idx, int Q, int k,
                                                          const int* __restrict__ key_labels, int K,
                                                          const int* __restrict__ query_labels, int L,
                                                          const int* __restrict__ member, int C, int level,
                                                          int* __restrict__ bits, int* __restrict__ flag) {
    const RankSlot s = rank_slot(idx, Q, k, K, flag);
    if (member) {  // kernel-uniform
        const int lab = s.ok ? key_labels[(size_t)s.id * L + level] : 0;
        const bool inr = s.ok && lab >= 0 && lab < C;
        if (s.ok && !inr) atomicOr(flag, EVAL_FLAG_BAD_LABEL);
        const unsigned long long b = __ballot(inr && member[lab] != 0);
        if (s.r == 0 && s.q < Q) bits[s.q] = (int)((unsigned)(b >> (s.sub * 16)) & 0xffffu);
        return;
    }
    match_levels(s, key_labels, query_labels, Q, L, [=](size_t at, unsigned g) { bits[at] = (int)g; });
}

// bit r set exactly when slot r takes the seen-key prediction: (double)sim[q, r] > t, strict, false for a NaN
__device__ __forceinline__ unsigned select_bits(const float* __restrict__ sim_row, int n, double t) {
    unsigned s = 0;
    for (int r = 0; r < n; ++r) s |= ((double)sim_row[r] > t ? 1u : 0u) << r;
    return s;
}

// One lane per query: the selection mask of its k slots, then per level the lowest set bit of (A & s) | (B & ~s), or k.
__global__ __launch_bounds__(256) void merge_hit_ranks_kernel(const float* __restrict__ sim, int Q, int k, const int* __restrict__ A,
                                                               const int* __restrict__ B, int L, double t,
                                                               int* __restrict__ hit_rank) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const unsigned s = select_bits(sim + (size_t)q * k, k, t);
    const unsigned low = (1u << k) - 1u;  // k <= 16
    for (int l = 0; l < L; ++l) {
        const unsigned a = (unsigned)A[(size_t)q * L + l], b = (unsigned)B[(size_t)q * L + l];
        const unsigned m = ((a & s) | (b & ~s)) & low;
        hit_rank[(size_t)q * L + l] = m ? __ffs(m) - 1 : k;
    }
}

// Brute force over (query, threshold): blockIdx.x takes 256 queries, one per lane, blockIdx.y EVAL_SWEEP_CHUNK thresholds.  A lane
// keeps its first kk = min(k', k) similarities as doubles and its two masks cut to kk bits; per threshold its count (0 or 1) is
// summed over the wave with a ballot and lane 0 adds it to counts[j].  Integer atomics: the sums do not depend on their order.
// `every` (k' > k): hit_rank <= k < k' holds for each query, whatever its masks.
__global__ __launch_bounds__(256) void threshold_sweep_kernel(const float* __restrict__ sim, int Q, int k, const int* __restrict__ A,
                                                               const int* __restrict__ B, int L, int level, int kk, bool every,
                                                               const double* __restrict__ thr, int T, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const unsigned low = (1u << kk) - 1u;  // kk <= 16
    double s[16];
    unsigned a = 0, b = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = (q < Q && r < kk) ? (double)sim[(size_t)q * k + r] : 0.0;
    if (q < Q) {
        a = (unsigned)A[(size_t)q * L + level] & low;
        b = (unsigned)B[(size_t)q * L + level] & low;
    }
    const int j0 = blockIdx.y * EVAL_SWEEP_CHUNK;
    const int j1 = j0 + EVAL_SWEEP_CHUNK < T ? j0 + EVAL_SWEEP_CHUNK : T;
    for (int j = j0; j < j1; ++j) {  // block-uniform
        const double t = thr[j];
        unsigned sel = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) sel |= (s[r] > t ? 1u : 0u) << r;  // slots >= kk hold 0.0 and are cut by a, b
        const unsigned long long hit = __ballot(q < Q && (every || ((a & sel) | (b & ~sel)) != 0u));
        if (lane == 0 && hit) atomicAdd(counts + j, __popcll(hit));
    }
}

}  // namespace

// the rank depth and level count every scoring entry point takes
#define EVAL_REQUIRE_K(fn) BSCLIP_REQUIRE(k >= 1 && k <= 16, fn ": k=%d (1..16)", k)
#define EVAL_REQUIRE_L(fn) BSCLIP_REQUIRE(L >= 1 && L <= EVAL_MAX_LEVELS, fn ": L=%d (1..%d)", L, EVAL_MAX_LEVELS)

extern "C" int bsclip_retrieval_hit_ranks(const int64_t* idx, int Q, int k, const int32_t* key_labels, int K,
                                          const int32_t* query_labels, int L, int32_t* hit_rank, int32_t* flag, void* stream) {
    BSCLIP_REQUIRE(idx && key_labels && query_labels && hit_rank && flag, "bsclip_retrieval_hit_ranks: null pointer");
    BSCLIP_REQUIRE(Q > 0 && K > 0, "bsclip_retrieval_hit_ranks: Q=%d K=%d", Q, K);
    EVAL_REQUIRE_K("bsclip_retrieval_hit_ranks");
    EVAL_REQUIRE_L("bsclip_retrieval_hit_ranks");
    BSCLIP_REQUIRE(aligned_to(8, idx) && aligned_to(4, key_labels, query_labels, hit_rank, flag),
                   "bsclip_retrieval_hit_ranks: idx must be 8-B aligned, the int32 buffers 4-B aligned");
    hipLaunchKernelGGL(hit_ranks_kernel, dim3(ceil_div(Q, 16)), dim3(256), 0, static_cast<hipStream_t>(stream), idx, Q, k,
                       key_labels, K, query_labels, L, hit_rank, flag);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_retrieval_class_counts(const int32_t* hit_rank, const int32_t* query_labels, int Q, int L,
                                             const int32_t* level_offsets, const int32_t* k_list, int nk, int32_t* seen,
                                             int32_t* right, int32_t* flag, void* stream) {
    BSCLIP_REQUIRE(hit_rank && query_labels && level_offsets && k_list && seen && right && flag,
                   "bsclip_retrieval_class_counts: null pointer");
    BSCLIP_REQUIRE(Q > 0, "bsclip_retrieval_class_counts: Q=%d", Q);
    EVAL_REQUIRE_L("bsclip_retrieval_class_counts");
    BSCLIP_REQUIRE(nk >= 1 && nk <= EVAL_MAX_K, "bsclip_retrieval_class_counts: nk=%d (1..%d)", nk, EVAL_MAX_K);
    BSCLIP_REQUIRE(aligned_to(4, hit_rank, query_labels, seen, right, flag),
                   "bsclip_retrieval_class_counts: the int32 buffers must be 4-B aligned");
    CountCfg cfg = {};
    BSCLIP_REQUIRE(level_offsets[0] == 0, "bsclip_retrieval_class_counts: level_offsets[0] must be 0");
    for (int l = 0; l <= L; ++l) {
        cfg.off[l] = level_offsets[l];
        BSCLIP_REQUIRE(l == 0 || cfg.off[l] >= cfg.off[l - 1], "bsclip_retrieval_class_counts: level_offsets must not decrease");
    }
    BSCLIP_REQUIRE(cfg.off[L] > 0, "bsclip_retrieval_class_counts: no classes");
    for (int j = 0; j < nk; ++j) {
        cfg.kl[j] = k_list[j];
        BSCLIP_REQUIRE(cfg.kl[j] >= 1, "bsclip_retrieval_class_counts: k_list[%d]=%d (>= 1)", j, cfg.kl[j]);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t C = (size_t)cfg.off[L];
    if (hipMemsetAsync(seen, 0, C * sizeof(int32_t), s) != hipSuccess ||
        hipMemsetAsync(right, 0, C * nk * sizeof(int32_t), s) != hipSuccess) {
        bsclip_set_error("bsclip_retrieval_class_counts: clearing the outputs failed: %s", hipGetErrorString(hipGetLastError()));
        return BSCLIP_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(class_counts_kernel, dim3(ceil_div(Q, 256), L), dim3(256), 0, s, hit_rank, query_labels, Q, L, cfg, nk,
                       seen, right, flag);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_retrieval_match_bits(const int64_t* idx, int Q, int k, const int32_t* key_labels, int K,
                                           const int32_t* query_labels, int L, const int32_t* member, int C, int level,
                                           int32_t* bits, int32_t* flag, void* stream) {
    BSCLIP_REQUIRE(idx && key_labels && bits && flag && (member || query_labels), "bsclip_retrieval_match_bits: null pointer");
    BSCLIP_REQUIRE(Q > 0 && K > 0, "bsclip_retrieval_match_bits: Q=%d K=%d", Q, K);
    EVAL_REQUIRE_K("bsclip_retrieval_match_bits");
    EVAL_REQUIRE_L("bsclip_retrieval_match_bits");
    if (member) {
        BSCLIP_REQUIRE(level >= 0 && level < L, "bsclip_retrieval_match_bits: level=%d (0 <= level < L=%d)", level, L);
        BSCLIP_REQUIRE(C > 0, "bsclip_retrieval_match_bits: C=%d member entries", C);
    }
    BSCLIP_REQUIRE(aligned_to(8, idx) && aligned_to(4, key_labels, query_labels, member, bits, flag),
                   "bsclip_retrieval_match_bits: idx must be 8-B aligned, the int32 buffers 4-B aligned");
    hipLaunchKernelGGL(match_bits_kernel, dim3(ceil_div(Q, 16)), dim3(256), 0, static_cast<hipStream_t>(stream), idx, Q, k,
                       key_labels, K, query_labels, L, member, C, level, bits, flag);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_retrieval_merge_hit_ranks(const float* sim, int Q, int k, const int32_t* A, const int32_t* B, int L,
                                                double threshold, int32_t* hit_rank, void* stream) {
    BSCLIP_REQUIRE(sim && A && B && hit_rank, "bsclip_retrieval_merge_hit_ranks: null pointer");
    BSCLIP_REQUIRE(Q > 0, "bsclip_retrieval_merge_hit_ranks: Q=%d", Q);
    EVAL_REQUIRE_K("bsclip_retrieval_merge_hit_ranks");
    EVAL_REQUIRE_L("bsclip_retrieval_merge_hit_ranks");
    BSCLIP_REQUIRE(aligned_to(4, sim, A, B, hit_rank),
                   "bsclip_retrieval_merge_hit_ranks: sim and the int32 buffers must be 4-B aligned");
    hipLaunchKernelGGL(merge_hit_ranks_kernel, dim3(ceil_div(Q, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), sim, Q, k, A,
                       B, L, threshold, hit_rank);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_retrieval_threshold_sweep(const float* sim, int Q, int k, const int32_t* A, const int32_t* B, int L, int level,
                                                int k_prime, const double* thresholds, int T, int32_t* counts, void* stream) {
    BSCLIP_REQUIRE(sim && A && B && thresholds && counts, "bsclip_retrieval_threshold_sweep: null pointer");
    BSCLIP_REQUIRE(Q > 0 && T > 0, "bsclip_retrieval_threshold_sweep: Q=%d T=%d", Q, T);
    EVAL_REQUIRE_K("bsclip_retrieval_threshold_sweep");
    EVAL_REQUIRE_L("bsclip_retrieval_threshold_sweep");
    BSCLIP_REQUIRE(level >= 0 && level < L, "bsclip_retrieval_threshold_sweep: level=%d (0 <= level < L=%d)", level, L);
    BSCLIP_REQUIRE(k_prime >= 1, "bsclip_retrieval_threshold_sweep: k_prime=%d (>= 1)", k_prime);
    BSCLIP_REQUIRE(aligned_to(4, sim, A, B, counts) && aligned_to(8, thresholds),
                   "bsclip_retrieval_threshold_sweep: thresholds must be 8-B aligned, sim and the int32 buffers 4-B aligned");
    const int kk = k_prime < k ? k_prime : k;  // the contract is hit_rank < k_prime: above k it holds for every query
    hipLaunchKernelGGL(threshold_sweep_kernel, dim3(ceil_div(Q, 256), ceil_div(T, EVAL_SWEEP_CHUNK)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), sim, Q, k, A, B, L, level, kk, k_prime > k, thresholds, T, counts);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
