// Supervised fine-tuning head (gfx950): cross-entropy on integer targets over the class logits of
// `EncoderWithExtraLayer` (reference bioscanclip/util/util.py:13-25, epoch/fine_tuning_epoch.py:27,93:
// `criterion(output, target)` with nn.CrossEntropyLoss()).
//
// The logits [B, C] = z W^T + b come out of bsclip_gemm_bf16 on split-bf16 operands (bsclip_split3_rows x
// bsclip_split3_weight), so their buffer is padded: ldc >= C columns, of which the kernel reads [0, C) only -- a padded
// column is absent, not a logit of 0.  One wave per row:
//   pass 1  per-lane running (max, sum exp) over 16-byte chunks, merged across the wave; loss_r = log(sum) + (max - x_target)
//   pass 2  dlogits = (softmax - onehot) / B, written as f32 (bias gradient: bsclip_colsum; dW operand: bsclip_split3_transpose)
//           and as the split-bf16 A operand [hi | lo | hi] of the dz = dlogits W GEMM, whose padded columns [C, Cp) are zeros.
// The row is read twice; at the sizes of a label set (C in the thousands: <= 32 KB per row) the second read comes from L2.
// The mean over the B rows is a second, one-workgroup launch that sums row_loss in a fixed order: no float atomics, so an eager
// call and a replayed graph give the same bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int CE_FLAG_BAD_TARGET = 1;  // a target outside [0, C): never used as an index, the row contributes nothing

__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo) {
    hi = pack_bf2(x0, x1);
    lo = pack_bf2(x0 - __uint_as_float(hi << 16), x1 - __uint_as_float(hi & 0xffff0000u));
}

__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, int ldc, const int* __restrict__ targets,
                                                       int B, int C, int Cp, float* __restrict__ row_loss,
                                                       float* __restrict__ dlogits, int ld_d, bf16_t* __restrict__ d3, int ld_d3,
                                                       int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B) return;  // whole waves leave; no block-wide barrier below
    const float* row = logits + (size_t)r * ldc;
    const int t = targets[r];
    const bool valid = t >= 0 && t < C;

    // pass 1: ldc % 4 == 0 and ldc >= C, so the chunk that holds column C - 1 is readable; columns >= C are masked out
    float m = -INFINITY, s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + c);
        float gm = x[0];  // c < C
#pragma unroll
        for (int e = 1; e < 4; ++e) gm = (c + e < C) ? fmaxf(gm, x[e]) : gm;
        if (gm > m) {  // the running maximum moves: rescale what has been summed (exp(-inf) = 0 on the first chunk)
            s *= expf(m - gm);
            m = gm;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s += (c + e < C) ? expf(x[e] - m) : 0.f;
    }
    const float M = wave_max(m);
    const float S = wave_sum(m == -INFINITY ? 0.f : s * expf(m - M));
    if (lane == 0) {
        if (valid) {
            // log(S) + (M - x_t), not (M + log S) - x_t: at |logits| ~ 1e4 the second form rounds the loss to 1e-3
            row_loss[r] = logf(S) + (M - row[t]);
        } else {
            row_loss[r] = 0.f;
            atomicOr(flag, CE_FLAG_BAD_TARGET);
        }
    }
    if (dlogits == nullptr && d3 == nullptr) return;

    // pass 2
    const float invS = 1.0f / S, invB = 1.0f / (float)B;
    for (int c = lane * 4; c < Cp; c += 256) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid && c < C) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = expf(x[e] - M) * invS;
                d[e] = (c + e < C) ? (p - (c + e == t ? 1.0f : 0.f)) * invB : 0.f;
            }
        }
        if (dlogits != nullptr && c < C) {
            float* o = dlogits + (size_t)r * ld_d + c;
            if (c + 3 < C) {
                *reinterpret_cast<f32x4*>(o) = f32x4{d[0], d[1], d[2], d[3]};
            } else {  // the chunk straddles column C: the caller's padding stays as it is
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < C) o[e] = d[e];
            }
        }
        if (d3 != nullptr) {
            uint2 hi, lo;
            split2(d[0], d[1], hi.x, lo.x);
            split2(d[2], d[3], hi.y, lo.y);
            bf16_t* o = d3 + (size_t)r * ld_d3 + c;
            *reinterpret_cast<uint2*>(o) = hi;
            *reinterpret_cast<uint2*>(o + Cp) = lo;
            *reinterpret_cast<uint2*>(o + 2 * Cp) = hi;
        }
    }
}

// loss_out[0] = (sum_r row_loss[r]) / B: thread i sums rows i, i + 256, ... in that order, then a fixed tree over the 256 partials
__global__ __launch_bounds__(256) void ce_mean_kernel(const float* __restrict__ row_loss, int B, float* __restrict__ loss_out) {
    __shared__ float part[256];
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int r = tid; r < B; r += 256) acc += row_loss[r];
    part[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) loss_out[0] = part[0] / (float)B;
}

}  // namespace

extern "C" int bsclip_ce_fwd_bwd(const float* logits, int ldc, const int32_t* targets, int B, int C, float* loss_out,
                                 float* row_loss, float* dlogits, int ld_d, void* dlogits_split3, int ld_d3, int32_t* flag,
                                 void* stream) {
    BSCLIP_REQUIRE(logits && targets && loss_out && row_loss && flag, "bsclip_ce_fwd_bwd: null pointer");
    BSCLIP_REQUIRE(B >= 1 && C >= 1, "bsclip_ce_fwd_bwd: B=%d C=%d (both >= 1)", B, C);
    BSCLIP_REQUIRE(ldc >= C && ldc % 4 == 0, "bsclip_ce_fwd_bwd: ldc=%d (>= C=%d, a multiple of 4)", ldc, C);
    const int Cp = (C + 63) / 64 * 64;
    BSCLIP_REQUIRE(!dlogits || (ld_d >= C && ld_d % 4 == 0), "bsclip_ce_fwd_bwd: ld_d=%d (>= C=%d, a multiple of 4)", ld_d, C);
    BSCLIP_REQUIRE(!dlogits_split3 || (ld_d3 >= 3 * Cp && ld_d3 % 4 == 0),
                   "bsclip_ce_fwd_bwd: ld_d3=%d (>= 3 x %d = C rounded up to 64, three times; a multiple of 4)", ld_d3, Cp);
    BSCLIP_REQUIRE(aligned_to(16, logits, dlogits) && aligned_to(8, dlogits_split3) && aligned_to(4, targets, loss_out, row_loss, flag),
                   "bsclip_ce_fwd_bwd: logits / dlogits must be 16-byte, dlogits_split3 8-byte, the other buffers 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ce_rows_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, s, logits, ldc, targets, B, C, Cp, row_loss, dlogits, ld_d,
                       static_cast<bf16_t*>(dlogits_split3), ld_d3, flag);
    hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(256), 0, s, row_loss, B, loss_out);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
