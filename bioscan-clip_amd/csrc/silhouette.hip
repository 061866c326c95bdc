// Silhouette coefficients of class-sorted samples (gfx950).
//
// Replaces sklearn's `silhouette_samples(image_features, gt_list)` in `calculate_silhouette_score` (reference
// scripts/inference_and_eval.py:407-411): for sample i of class A with n_A members, a = sum_{j in A} d(i,j) / (n_A - 1),
// b = min over the other classes C of sum_{j in C} d(i,j) / n_C, s = (b - a) / max(a, b); s = 0 for a singleton class and where the
// quotient is no number.  d is the euclidean distance of the features as given.
//   * distances from DIFFERENCES, sum_k (x_ik - x_jk)^2 in f32 on the vector ALU (v_pk_add_f32 / v_pk_fma_f32): the Gram form
//     n_i + n_j - 2 x_i.x_j cancels for the near-duplicate embeddings of one species, the difference form does not;
//   * the caller sorts the rows by class, so the classes are the row ranges [seg_start[c], seg_start[c+1]).  A workgroup owns
//     SIL_TILE rows and walks the column tiles left to right; after a tile's K loop one lane per row adds the tile's distances, in
//     column order, to the running sum of the class the column lies in, and closes the class (mean, then own-class sum or minimum)
//     where the column crosses a boundary.  The carried sums are double.  Nothing of size N x C or N x N is written;
//   * no float atomics and one fixed order of every sum: a repeated call returns the same bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int SIL_TILE = 64;                 // rows per workgroup and columns per tile
constexpr int SIL_BK = 32;                   // features per staged chunk
constexpr int SIL_LDK = SIL_BK + 4;          // LDS row stride in floats: 9 16-byte slots, odd, so 16 rows 1 apart hit 16 slots
constexpr int SIL_LDD = SIL_TILE + 2;        // stride of the [column][row] distance tile
constexpr int SIL_FLAG_NONFINITE = 1;        // a distance that is no finite number
constexpr int SIL_FLAG_BAD_SEGMENTS = 2;     // seg_start is not a non-decreasing sequence from 0 to N

typedef __attribute__((ext_vector_type(2))) float f32x2;

// seg_start[0] == 0, seg_start[C] == N, no decrease: anything else sets SIL_FLAG_BAD_SEGMENTS and the main kernel, launched behind
// this one on the same stream, leaves without reading it
__global__ __launch_bounds__(256) void silhouette_check_segments_kernel(const int* __restrict__ seg_start, int C, int N,
                                                                         int* __restrict__ flag) {
    bool bad = false;
    for (int c = blockIdx.x * 256 + threadIdx.x; c <= C; c += gridDim.x * 256) {
        const int v = seg_start[c];
        bad |= v < 0 || v > N || (c == 0 && v != 0) || (c == C && v != N) || (c < C && seg_start[c + 1] < v);
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, SIL_FLAG_BAD_SEGMENTS);
}

// what one lane of the walk carries for its row
struct RowWalk {
    double run = 0.0;     // sum over the columns of the open class seen so far
    double own = 0.0;     // the closed sum over the row's own class
    double other = INFINITY;  // the smallest mean over the closed other classes
    bool bad = false;
};

// 256 threads: thread (ty, tx) = (tid / 16, tid % 16) holds the squared distances of rows ty + 16 i and columns tx + 16 j of the tile,
// i, j < 4, as two partial sums each (even and odd features: the two halves of the packed f32 instructions).
__global__ __launch_bounds__(256) void silhouette_kernel(const float* __restrict__ x, int ld, int N, int D,
                                                          const int* __restrict__ seg_start, int C, float* __restrict__ out,
                                                          int* __restrict__ flag) {
    __shared__ __attribute__((aligned(16))) float As[SIL_TILE * SIL_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[SIL_TILE * SIL_LDK];
    __shared__ float Ds[SIL_TILE * SIL_LDD];
    if (__atomic_load_n(flag, __ATOMIC_RELAXED) & SIL_FLAG_BAD_SEGMENTS) return;  // kernel-uniform: set before this launch or not at all

    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * SIL_TILE;
    const int ntiles = (N + SIL_TILE - 1) / SIL_TILE, nchunks = (D + SIL_BK - 1) / SIL_BK;

    // the walk: lane r of wave 0 owns row row0 + r; its class is the last c with seg_start[c] <= row
    const int wrow = row0 + tid;
    const bool walker = tid < SIL_TILE && wrow < N;
    int myc = 0;
    if (walker) {
        int lo = 0, hi = C;  // seg_start[lo] <= wrow < seg_start[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg_start[mid] <= wrow) lo = mid; else hi = mid;
        }
        myc = lo;
    }
    RowWalk w;
    int cls = 0, cls_end = seg_start[1];  // the open class and its end: the same in every lane

    // staging: slot s = tid + 256 u of a tile is 16 bytes, row s / 8, features 4 (s % 8) .. + 3 of the chunk
    f32x4 ra[2], rb[2];
    auto fetch = [&](int base_row, int k0, f32x4 (&r)[2]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int s = tid + 256 * u, row = base_row + (s >> 3), k = k0 + (s & 7) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < N && k < D) {  // ld % 4 == 0 and ld >= D: the 16 bytes at k lie inside the row
                v = *reinterpret_cast<const f32x4*>(x + (size_t)row * ld + k);
#pragma unroll
                for (int e = 1; e < 4; ++e)
                    if (k + e >= D) v[e] = 0.f;  // what lies between D and ld is not part of the features
            }
            r[u] = v;
        }
    };
    auto stage = [&](float* tile, const f32x4 (&r)[2], float sign) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int s = tid + 256 * u;
            *reinterpret_cast<f32x4*>(tile + (s >> 3) * SIL_LDK + (s & 7) * 4) = r[u] * sign;
        }
    };

    fetch(row0, 0, ra);
    fetch(0, 0, rb);
    for (int t = 0; t < ntiles; ++t) {
        const int col0 = t * SIL_TILE;
        f32x2 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x2{0.f, 0.f};

        for (int kc = 0; kc < nchunks; ++kc) {
            __syncthreads();  // the previous chunk's reads (and the previous tile's walk) are done
            stage(As, ra, 1.f);
            stage(Bs, rb, -1.f);  // the column side is kept negated: x_i + (-x_j) is x_i - x_j bit for bit and packs into v_pk_add_f32
            __syncthreads();
            // the next chunk's global loads fly during this chunk's arithmetic
            const bool last = kc + 1 == nchunks;
            if (!last || t + 1 < ntiles) {
                const int nk0 = last ? 0 : (kc + 1) * SIL_BK;
                fetch(row0, nk0, ra);
                fetch(last ? col0 + SIL_TILE : col0, nk0, rb);
            }
#pragma unroll
            for (int kq = 0; kq < SIL_BK / 4; ++kq) {
                f32x4 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4*>(As + (ty + 16 * i) * SIL_LDK + kq * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(Bs + (tx + 16 * j) * SIL_LDK + kq * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 d = a[i] + b[j];
                        const f32x2 d0 = {d[0], d[1]}, d1 = {d[2], d[3]};
                        acc[i][j] = __builtin_elementwise_fma(d0, d0, acc[i][j]);
                        acc[i][j] = __builtin_elementwise_fma(d1, d1, acc[i][j]);
                    }
            }
        }

        // distances of the tile, [column][row]; the diagonal is 0 whatever the arithmetic gave
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = ty + 16 * i, c = tx + 16 * j;
                const float dist = sqrtf(acc[i][j][0] + acc[i][j][1]);
                Ds[c * SIL_LDD + r] = (row0 + r == col0 + c) ? 0.f : dist;
            }
        __syncthreads();
        if (walker) {
            const int ncols = N - col0 < SIL_TILE ? N - col0 : SIL_TILE;
            for (int c = 0; c < ncols; ++c) {
                while (cls < C && col0 + c == cls_end) {  // lane-uniform: close the class that ends in front of this column
                    const int n = cls_end - seg_start[cls];
                    if (n > 0) {
                        if (cls == myc) w.own = w.run;
                        else w.other = fmin(w.other, w.run / (double)n);
                    }
                    w.run = 0.0;
                    ++cls;
                    cls_end = cls < C ? seg_start[cls + 1] : N + 1;
                }
                const float dist = Ds[c * SIL_LDD + tid];
                w.bad |= !(fabsf(dist) < INFINITY);
                w.run += (double)dist;
            }
        }
    }
    if (!walker) return;
    for (; cls < C; ++cls) {  // the class open at column N and the empty ones behind it
        const int n = seg_start[cls + 1] - seg_start[cls];
        if (n > 0) {
            if (cls == myc) w.own = w.run;
            else w.other = fmin(w.other, w.run / (double)n);
        }
        w.run = 0.0;
    }
    const int n_own = seg_start[myc + 1] - seg_start[myc];
    double s = 0.0;
    if (n_own > 1) {
        const double a = w.own / (double)(n_own - 1), b = w.other;
        const double m = fmax(a, b);
        s = (b - a) / m;
        if (!(m > 0.0) || s != s) s = 0.0;  // nan_to_num: a = b = 0, or no other class
    }
    out[wrow] = (float)s;
    if (w.bad) atomicOr(flag, SIL_FLAG_NONFINITE);
}

}  // namespace

extern "C" int bsclip_silhouette_samples(const float* x_sorted, int ld, int N, int D, const int32_t* seg_start, int C,
                                         float* out_sorted, int32_t* flag, void* stream) {
    BSCLIP_REQUIRE(x_sorted && seg_start && out_sorted && flag, "bsclip_silhouette_samples: null pointer");
    BSCLIP_REQUIRE(N >= 3, "bsclip_silhouette_samples: N=%d (>= 3)", N);
    BSCLIP_REQUIRE(C >= 2 && C <= N - 1, "bsclip_silhouette_samples: C=%d (2 .. N - 1 = %d)", C, N - 1);
    BSCLIP_REQUIRE(D >= 1, "bsclip_silhouette_samples: D=%d (>= 1)", D);
    BSCLIP_REQUIRE(ld >= D && ld % 4 == 0, "bsclip_silhouette_samples: ld=%d (>= D=%d, a multiple of 4)", ld, D);
    BSCLIP_REQUIRE(aligned_to(16, x_sorted) && aligned_to(4, seg_start, out_sorted, flag),
                   "bsclip_silhouette_samples: x_sorted must be 16-byte, seg_start, out_sorted and flag 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int check_blocks = ceil_div(C + 1, 256) < 64 ? ceil_div(C + 1, 256) : 64;
    hipLaunchKernelGGL(silhouette_check_segments_kernel, dim3(check_blocks), dim3(256), 0, s, seg_start, C, N, flag);
    hipLaunchKernelGGL(silhouette_kernel, dim3(ceil_div(N, SIL_TILE)), dim3(256), 0, s, x_sorted, ld, N, D, seg_start, C, out_sorted,
                       flag);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
