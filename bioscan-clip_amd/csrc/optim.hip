// Trainable-parameter gradients that are not GEMM-shaped, and the optimiser (gfx950).
//   lora_grad : autograd of the rank-4 LoRA branches (image_encoder.py:44-47, dna_encoder.py:47-49) -- skinny
//               reductions over all M tokens, HBM-bound: one pass over dq/dv/t (dt + dB), one over y (dA).
//   colsum    : bias gradients of the trainable heads.
//   adamw     : torch.optim.AdamW defaults (scripts/train_cl.py:158), one launch over the flat trainable buffer.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ f32x4 ld_bf4(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return f32x4{bf2f(u.x & 0xffff), bf2f(u.x >> 16), bf2f(u.y & 0xffff), bf2f(u.y >> 16)};
}

// same 8-way transpose-reduce as norm.hip (lane group bits (5,4,3) ends up owning index r)
__device__ __forceinline__ float reduce8(float (&p)[8], int lane) {
    float q[4];
    const bool hi5 = lane & 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float send = hi5 ? p[i] : p[i + 4];
        const float keep = hi5 ? p[i + 4] : p[i];
        q[i] = keep + __shfl_xor(send, 32, 64);
    }
    float r2[2];
    const bool hi4 = lane & 16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float send = hi4 ? q[i] : q[i + 2];
        const float keep = hi4 ? q[i + 2] : q[i];
        r2[i] = keep + __shfl_xor(send, 16, 64);
    }
    const bool hi3 = lane & 8;
    float v = (hi3 ? r2[1] : r2[0]) + __shfl_xor(hi3 ? r2[0] : r2[1], 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

constexpr int LG_BLOCK = 256;

// One value in all four elements, in registers of its own (opaque to the compiler): the packed FMAs that follow take plain operands
// instead of broadcasting one half of a register pair through op_sel.
// Why (round 5, docs/HISTORY.md "the lost quarter-wave"): in the exact mode's three-tower step the BarcodeBERT tower's first
// bsclip_lora_grad_f32 of a backward -- and only that launch, the one that runs beside the other towers' first backward kernels --
// left, once in a few dozen steps, 16-80 words of its dA / dB slabs off by one row's contribution: always lanes 48-63, always the LOW
// half of a `v_pk_fma_f32 acc, y, d op_sel:[0,1,0]` whose multiplier is the HIGH register of a pair filled by a wave-uniform
// global_load_dwordx4 (dt[row, 0:8] / a row of dq), identical inputs, never reproducible with the kernel alone under synthetic load
// (tools/stress_lora_f32.py: 0 of 8 000).  tests/test_30's exact three-tower graph-vs-eager case failed in ~40 % of the suite runs;
// with the multipliers splatted first (this function) 120 of 120 iterations of tools/debug_graph_flake.py are bit-equal (before: a mismatch
// within 4 iterations in 9 of 10 runs).  The cause below the ISA is not established; the form that does not show it is kept.  (Also
// tried and NOT the cause: the cross-wave LDS sums as ds_add_f32 instead of ds_read2 / v_add / ds_write2 -- the flake stayed, and LDS
// float atomics cost the dA pass 111 instead of 23 us.)  The dt / dB pass pays for it (no packed FMAs left: 41 -> ~70 us); it only runs
// in the fp8 and exact configurations since the attention backward leaves those sums itself.
__device__ __forceinline__ f32x4 splat4(float v) {
    f32x4 s = {v, v, v, v};
    asm("" : "+v"(s));   // not volatile: as an ordering point between the row loads it cost the da kernel 111 instead of 23 us
    return s;
}

// 4-way transpose-reduce: lane bits (5,4) end up owning index r
__device__ __forceinline__ float reduce4(float (&p)[4], int lane) {
    float q[2];
    const bool hi5 = lane & 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float send = hi5 ? p[i] : p[i + 2];
        const float keep = hi5 ? p[i + 2] : p[i];
        q[i] = keep + __shfl_xor(send, 32, 64);
    }
    const bool hi4 = lane & 16;
    float v = (hi4 ? q[1] : q[0]) + __shfl_xor(hi4 ? q[0] : q[1], 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// pass 1: dt[M,8] = [dq.B_q | dv.B_v];  dBq[H,4] += dq^T t_q;  dBv[H,4] += dv^T t_v
// haug / ld_h: the bf16 block holding t -- the LN output row (t at column H, bf16 path) or the separate t_aug buffer
// (t at column 0, fp8 path; the caller passes haug = t_aug - H)
// The waves of a workgroup come in pairs: the even wave of a pair owns the q half of a row (dq, B_q, t_q), the odd wave the v
// half.  With both halves in one wave the kernel held 2 x (B + accumulators) = 192 VGPRs plus the rows in flight and ran at two
// waves per SIMD, HBM latency exposed (59 us for 155 MB); a half is 96 + rows, three waves per SIMD.
// F32IN (exact mode, round 5): dqkv is f32 [M, ld] and t comes from an f32 [M, 8] buffer (haug = that buffer, ld_h = 8) -- the same
// kernel on the exact backward's operands; the first f32 version (one workgroup per row group, 16 wave reductions per row, two
// barriers per four rows) took 640 us per layer at B = 256 against this kernel's 41 us on bf16 rows.
template <int H, bool F32IN = false>
__global__ __launch_bounds__(LG_BLOCK) void lora_grad_dt_db_kernel(const void* __restrict__ dqkv_, int ld,
                                                                    const void* __restrict__ haug_, int ld_h, int M,
                                                                    const float* __restrict__ lora_b,
                                                                    float* __restrict__ dt,
                                                                    float* __restrict__ partial) {
    const bf16_t* dqkv = static_cast<const bf16_t*>(dqkv_);
    const bf16_t* haug = static_cast<const bf16_t*>(haug_);
    constexpr int NV = H / 256;
    __shared__ float red[2 * NV * 16 * 64];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int is_v = wib & 1;
    const int pair = blockIdx.x * (LG_BLOCK / 128) + (wib >> 1);
    const int npairs = gridDim.x * (LG_BLOCK / 128);
    for (int i = threadIdx.x; i < 2 * NV * 16 * 64; i += LG_BLOCK) red[i] = 0.f;

    f32x4 bx[NV][4];  // [chunk][column-in-chunk] -> 4 ranks of this half's B
    f32x4 ax[NV][4];  // accumulators, same indexing
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = j * 256 + lane * 4 + i;
            bx[j][i] = *reinterpret_cast<const f32x4*>(lora_b + (size_t)(is_v * H + c) * 4);
            ax[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    // Rows are software-pipelined three deep: a wave keeps the loads of its next PF half-rows in flight while it reduces one.
    constexpr int PF = 3;
    using row_t = std::conditional_t<F32IN, f32x4, uint2>;
    row_t rx[PF][NV];
    row_t rt[PF];
    auto fetch = [&](int slot, int row) {
        if constexpr (F32IN) {
            const float* g = static_cast<const float*>(dqkv_) + (size_t)row * ld + is_v * 2 * H;
#pragma unroll
            for (int j = 0; j < NV; ++j) rx[slot][j] = *reinterpret_cast<const f32x4*>(g + j * 256 + lane * 4);
            rt[slot] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(haug_) + (size_t)row * ld_h + 4 * is_v);
        } else {
            const bf16_t* g = dqkv + (size_t)row * ld + is_v * 2 * H;
#pragma unroll
            for (int j = 0; j < NV; ++j) rx[slot][j] = *reinterpret_cast<const uint2*>(g + j * 256 + lane * 4);
            rt[slot] = *reinterpret_cast<const uint2*>(haug + (size_t)row * ld_h + H + 4 * is_v);  // this half's t (4), broadcast
        }
    };
#pragma unroll
    for (int p = 0; p < PF; ++p)
        if (pair + p * npairs < M) fetch(p, pair + p * npairs);
    auto body = [&](int slot, int row) {
        f32x4 dx[NV];
        f32x4 tx;
        if constexpr (F32IN) {
#pragma unroll
            for (int j = 0; j < NV; ++j) dx[j] = rx[slot][j];
            tx = rt[slot];
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j)
                dx[j] = f32x4{bf2f(rx[slot][j].x & 0xffff), bf2f(rx[slot][j].x >> 16), bf2f(rx[slot][j].y & 0xffff),
                              bf2f(rx[slot][j].y >> 16)};
            const uint2 tu = rt[slot];
            tx = f32x4{bf2f(tu.x & 0xffff), bf2f(tu.x >> 16), bf2f(tu.y & 0xffff), bf2f(tu.y >> 16)};
        }
        if (row + PF * npairs < M) fetch(slot, row + PF * npairs);
        f32x4 px = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 d4 = splat4(dx[j][i]);
                px += d4 * bx[j][i];
                ax[j][i] += d4 * tx;
            }
        float p[4] = {px[0], px[1], px[2], px[3]};
        const float tot = reduce4(p, lane);
        const float tl = __shfl(tot, ((lane >> 1) & 1) * 32 + (lane & 1) * 16, 64);
        if (lane < 4) dt[(size_t)row * 8 + 4 * is_v + lane] = tl;
    };
    for (int row = pair; row < M; row += PF * npairs) {  // slots are compile-time indices: registers, not scratch
#pragma unroll
        for (int p = 0; p < PF; ++p)
            if (row + p * npairs < M) body(p, row + p * npairs);
    }
    // cross-wave sum in wave order (no LDS atomics: the order of float adds is fixed): waves 0, 2 into the q region, 1, 3 into v
    float* mine = red + is_v * (NV * 16 * 64);
    for (int w = 0; w < LG_BLOCK / 64; ++w) {
        __syncthreads();
        if (wib == w) {
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mine[((j * 16 + i * 4 + r) * 64) + lane] += ax[j][i][r];
        }
    }
    __syncthreads();
    // per-workgroup partial slab (plain coalesced stores; summed in a fixed order by lora_grad_reduce_kernel)
    for (int idx = threadIdx.x; idx < 2 * NV * 16 * 64; idx += LG_BLOCK)
        partial[(size_t)blockIdx.x * (2 * NV * 16 * 64) + idx] = red[idx];
}

// pass 2: dA[8,H] += dt^T y.  Y_FP8: y is the fp8 e4m3 LN output (row stride ld_h bytes) instead of bf16; F16: y is IEEE fp16.
template <int H, bool Y_FP8 = false, bool Y_F32 = false, bool F16 = false>
__global__ __launch_bounds__(LG_BLOCK) void lora_grad_da_kernel(const void* __restrict__ haug_, int ld_h, int M,
                                                                 const float* __restrict__ dt,
                                                                 float* __restrict__ partial) {
    const bf16_t* haug = static_cast<const bf16_t*>(haug_);
    constexpr int NV = H / 256;
    __shared__ float red[8 * NV * 4 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * LG_BLOCK + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * LG_BLOCK) >> 6;
    for (int i = threadIdx.x; i < 8 * NV * 4 * 64; i += LG_BLOCK) red[i] = 0.f;
    f32x4 acc[8][NV];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // three rows per iteration: all their loads are issued before the first is consumed
    constexpr int PF = 3;
    for (int row0 = wave; row0 < M; row0 += PF * nwaves) {
        f32x4 d0[PF], d1[PF];
        std::conditional_t<Y_F32, f32x4, uint2> yr[PF][NV];
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int row = min(row0 + p * nwaves, M - 1);
            d0[p] = *reinterpret_cast<const f32x4*>(dt + (size_t)row * 8);
            d1[p] = *reinterpret_cast<const f32x4*>(dt + (size_t)row * 8 + 4);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                if constexpr (Y_F32) {
                    yr[p][j] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(haug_) + (size_t)row * ld_h + j * 256 + lane * 4);
                } else if constexpr (Y_FP8) {
                    yr[p][j].x = *reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(haug) +
                                                                    (size_t)row * ld_h + j * 256 + lane * 4);
                    yr[p][j].y = 0;
                } else {
                    yr[p][j] = *reinterpret_cast<const uint2*>(haug + (size_t)row * ld_h + j * 256 + lane * 4);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            if (row0 + p * nwaves >= M) break;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                f32x4 y;
                if constexpr (Y_F32)
                    y = yr[p][j];
                else if constexpr (Y_FP8)
                    y = f32x4{fp8_to_f32(yr[p][j].x, 0), fp8_to_f32(yr[p][j].x, 1), fp8_to_f32(yr[p][j].x, 2), fp8_to_f32(yr[p][j].x, 3)};
                else
                    y = f32x4{h2f<F16>(yr[p][j].x & 0xffff), h2f<F16>(yr[p][j].x >> 16), h2f<F16>(yr[p][j].y & 0xffff),
                              h2f<F16>(yr[p][j].y >> 16)};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[r][j] += splat4(d0[p][r]) * y;
                    acc[4 + r][j] += splat4(d1[p][r]) * y;
                }
            }
        }
    }
    const int wib = threadIdx.x >> 6;
    for (int w = 0; w < LG_BLOCK / 64; ++w) {
        __syncthreads();
        if (wib == w) {
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int j = 0; j < NV; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) red[(((r * NV + j) * 4 + i) * 64) + lane] += acc[r][j][i];
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 8 * NV * 4 * 64; idx += LG_BLOCK)
        partial[(size_t)blockIdx.x * (8 * NV * 4 * 64) + idx] = red[idx];
}

// t[row, 0:8] = y[row, :] . A[0:8, :]^T in f32 (exact mode: the forward folds W + B A into the weight, so t is rebuilt for the backward):
// one wave per row, A in LDS as in the LayerNorm kernels
template <int H>
__global__ __launch_bounds__(LG_BLOCK) void lora_t_f32_kernel(const float* __restrict__ y, int ld_y, int M, const float* __restrict__ A,
                                                              float* __restrict__ t) {
    constexpr int NV = H / 256;
    __shared__ __attribute__((aligned(16))) float sA[8 * H];
    for (int i = threadIdx.x * 4; i < 8 * H; i += LG_BLOCK * 4) *reinterpret_cast<f32x4*>(sA + i) = *reinterpret_cast<const f32x4*>(A + i);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * LG_BLOCK + threadIdx.x) >> 6, nwaves = (gridDim.x * LG_BLOCK) >> 6;
    for (int row = wave; row < M; row += nwaves) {
        asm volatile("" ::: "memory");   // sA is loop-invariant: keep its reads out of the registers
        f32x4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = *reinterpret_cast<const f32x4*>(y + (size_t)row * ld_y + j * 256 + lane * 4);
        float p[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(sA + r * H + j * 256 + lane * 4);
                d += (v[j][0] * a[0] + v[j][1] * a[1]) + (v[j][2] * a[2] + v[j][3] * a[3]);
            }
            p[r] = d;
        }
        const float tt = reduce8(p, lane);  // lane group (bits 5,4,3) owns r
        const float tl = __shfl(tt, ((lane >> 2) & 1) * 32 + ((lane >> 1) & 1) * 16 + (lane & 1) * 8, 64);
        if (lane < 8) t[(size_t)row * 8 + lane] = tl;
    }
}

// Sum the per-workgroup slabs in a fixed order (bitwise reproducible) and accumulate into dBq/dBv/dA.
// Slab A (8H floats): index k*64 + l, k = [is_v][j][i][r];  slab B (8H floats): index ((r*NV + j)*4 + i)*64 + l.
// Workgroup = 32 consecutive slab elements x 32 slab groups: thread (q, p) sums 4 consecutive elements (one 16-byte load per slab) of
// slabs p, p + 32, ... with four loads in flight; the 32 partial sums are combined in p order through LDS.  (Round 5: 4-byte loads
// over 8 groups of 96 slabs took 13 us for the step's 19 MB of dA slabs.)
// first_block = SLAB / 32 with a grid of SLAB / 32 workgroups sums the dA slabs only (bsclip_lora_grad_heads: dB comes from the
// attention kernel's partials).
// UNSCALE (fp16-operand backward, bsclip_lora_grad_heads_f16): the slabs hold 2^s times the gradient; each sum is multiplied by
// unscale = 2^-s (exact) before it is added to the gradient.
template <int H, bool UNSCALE = false>
__global__ __launch_bounds__(256) void lora_grad_reduce_kernel(const float* __restrict__ pa,
                                                                const float* __restrict__ pb, int nblocks,
                                                                float* __restrict__ dA, float* __restrict__ dBq,
                                                                float* __restrict__ dBv, int first_block = 0, float unscale = 1.f) {
    constexpr int NV = H / 256;
    constexpr int SLAB = 8 * H;
    __shared__ f32x4 red[32][8];
    const int q = threadIdx.x & 7, p = threadIdx.x >> 3;
    const int idx = (blockIdx.x + first_block) * 32 + q * 4;  // < 2*SLAB by construction (grid = 2*SLAB/32)
    const bool second = idx >= SLAB;
    const int e = second ? idx - SLAB : idx;
    const float* src = (second ? pb : pa) + e;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int b = p;
    for (; b + 96 < nblocks; b += 128) {   // four loads in flight; the adds keep the slab order
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(src + (size_t)(b + 32 * u) * SLAB);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += v[u];
    }
    for (; b < nblocks; b += 32) s += *reinterpret_cast<const f32x4*>(src + (size_t)b * SLAB);
    red[p][q] = s;
    __syncthreads();
    if (p != 0) return;
    s = red[0][q];
#pragma unroll
    for (int g = 1; g < 32; ++g) s += red[g][q];
    if constexpr (UNSCALE) s *= unscale;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ec = e + c;
        const int l = ec & 63, k = ec >> 6;
        if (!second) {
            const bool is_v = k >= NV * 16;
            const int kk = is_v ? k - NV * 16 : k;
            const int j = kk >> 4, ii = (kk >> 2) & 3, r = kk & 3;
            const int col = j * 256 + l * 4 + ii;
            float* dst = (is_v ? dBv : dBq) + (size_t)col * 4 + r;
            *dst += s[c];
        } else {
            const int ii = k & 3, j = (k >> 2) % NV, r = (k >> 2) / NV;
            dA[(size_t)r * H + j * 256 + l * 4 + ii] += s[c];
        }
    }
}

// Sums what bsclip_attn_bwd_lora left (attn.hip LoraPart), in a fixed order:
//   workgroups [0, nA):  dt[row][4 half : 4 half + 4] = sum_head dt_partial[head][half][row][0:4]   (thread = (row, half); 12 loads in flight)
//   the rest:            dB[q | v][head * 64 + d][j] += sum_item db_partial[item][q | v][j][d]   (as lora_grad_reduce_kernel: 32
//                        consecutive elements x 8 item groups per workgroup, combined in group order through LDS)
// UNSCALE: as lora_grad_reduce_kernel's, on the dB sums (dt stays in the scaled units of the gradient stream it feeds)
template <bool UNSCALE = false>
__global__ __launch_bounds__(256) void lora_heads_reduce_kernel(const float* __restrict__ dtp, const float* __restrict__ dbp, int M,
                                                                 int heads, int items, int nA, float* __restrict__ dt,
                                                                 float* __restrict__ dBq, float* __restrict__ dBv, float unscale = 1.f) {
    if ((int)blockIdx.x < nA) {
        const int g = blockIdx.x * 256 + threadIdx.x, row = g >> 1, half = g & 1;
        if (row >= M) return;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int hd = 0; hd < heads; hd += 4) {   // heads is a multiple of 4 (8 or 12)
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(dtp + (((size_t)(hd + u) * 2 + half) * M + row) * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
        *reinterpret_cast<f32x4*>(dt + (size_t)row * 8 + 4 * half) = s;
        return;
    }
    __shared__ float red[8][32];
    const int i = threadIdx.x & 31, p = threadIdx.x >> 5;
    const int e = ((int)blockIdx.x - nA) * 32 + i;   // < heads * 512 by construction
    const size_t stride = (size_t)heads * 512;
    const float* src = dbp + e;
    float s = 0.f;
    int b = p;
    for (; b + 56 < items; b += 64) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(b + 8 * u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < items; b += 8) s += src[(size_t)b * stride];
    red[p][i] = s;
    __syncthreads();
    if (p != 0) return;
    s = ((red[0][i] + red[1][i]) + (red[2][i] + red[3][i])) + ((red[4][i] + red[5][i]) + (red[6][i] + red[7][i]));
    if constexpr (UNSCALE) s *= unscale;
    const int hd = e >> 9, is_v = (e >> 8) & 1, j = (e >> 6) & 3, d = e & 63;
    float* dst = (is_v ? dBv : dBq) + (size_t)(hd * 64 + d) * 4 + j;
    *dst += s;
}

// out[n] += sum_r g[r, n] without atomics (bitwise reproducible) and without a workspace.
// Wide version (N % 8 == 0): one workgroup per 8 columns, thread t sums rows t, t+256, ... with one 16-B (bf16) / 2x16-B
// (f32) load per row, 4 rows in flight; the 256 partials are combined in a fixed order through LDS.  N/8 workgroups (96
// for N = 768) keep enough CUs busy for the one large caller, the MLM decoder bias gradient ([B*133, 768] bf16).
template <bool BF16>
__global__ __launch_bounds__(256) void colsum8_kernel(const void* __restrict__ g, int ld, int M, int N,
                                                       float* __restrict__ out) {
    __shared__ float part[256][9];
    __shared__ float part2[8][8];
    const int t = threadIdx.x;
    const int n0 = blockIdx.x * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto add_row = [&](int r) {
        if constexpr (BF16) {
            const u32x4 u = *reinterpret_cast<const u32x4*>(static_cast<const bf16_t*>(g) + (size_t)r * ld + n0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[2 * k] += bf2f(u[k] & 0xffff);
                s[2 * k + 1] += bf2f(u[k] >> 16);
            }
        } else {
            const float* p = static_cast<const float*>(g) + (size_t)r * ld + n0;
            const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[k] += a[k];
                s[4 + k] += b[k];
            }
        }
    };
    int r = t;
    for (; r + 768 < M; r += 1024) {
        add_row(r);
        add_row(r + 256);
        add_row(r + 512);
        add_row(r + 768);
    }
    for (; r < M; r += 256) add_row(r);
#pragma unroll
    for (int k = 0; k < 8; ++k) part[t][k] = s[k];
    __syncthreads();
    if (t < 64) {  // 8 columns x 8 row-octets: thread (c, o) sums partials 32*o .. 32*o+31 in order
        const int c = t & 7, o = t >> 3;
        float a = 0.f;
        for (int i = 0; i < 32; ++i) a += part[32 * o + i][c];
        part2[o][c] = a;
    }
    __syncthreads();
    if (t < 8) {
        float a = 0.f;
#pragma unroll
        for (int o = 0; o < 8; ++o) a += part2[o][t];
        out[n0 + t] += a;
    }
}

// Narrow fallback (any N): one workgroup per 32 columns, 8 row groups x 32 columns.
template <bool BF16>
__global__ __launch_bounds__(256) void colsum_kernel(const void* __restrict__ g, int ld, int M, int N,
                                                      float* __restrict__ out) {
    __shared__ float part[8][32];
    const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + c;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < N) {
        auto at = [&](int r) -> float {
            if constexpr (BF16) return bf2f(static_cast<const bf16_t*>(g)[(size_t)r * ld + n]);
            else return static_cast<const float*>(g)[(size_t)r * ld + n];
        };
        int r = rg;
        for (; r + 24 < M; r += 32) {
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += at(r + 8 * u);
        }
        for (; r < M; r += 8) s[0] += at(r);
    }
    part[rg][c] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (rg == 0 && n < N) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += part[k][c];
        out[n] += t;
    }
}

// The AdamW update of a workgroup's elements (grid-stride, 256 threads), the one body of the AdamW kernels below: what they compute
// stays equal bit for bit because it is the same code.
// EMA: the thread that stored p[i] also moves the weight average towards it, ema[i] += ema_w * (p[i] - ema[i]) --
// torch's lerp_(p, w) on the value still in its register; ema overlaps none of p, g, m, v.
template <bool EMA = false>
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, long n, float lr, float beta1, float beta2, float eps, float wd,
                                             float inv_bc1, float inv_sqrt_bc2, float grad_scale, float* __restrict__ ema = nullptr,
                                             float ema_w = 0.f) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float gi = g[i] * grad_scale;
        float pi = p[i] * (1.0f - lr * wd);
        const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        pi -= (lr * inv_bc1) * (mi / denom);
        p[i] = pi;
        if constexpr (EMA) {
            const float e = ema[i];
            ema[i] = e + ema_w * (pi - e);
        }
        m[i] = mi;
        v[i] = vi;
    }
}

// lr and step come from device memory: hyper[0] = lr (f32), hyper[1] = step count (uint32 bits, advanced by a
// bsclip_counter_add node of the captured step, so no in-flight node ever reads host memory); the bias corrections are
// formed in f64 like the host form does
struct AdamwHyper {
    float lr, inv_bc1, inv_sqrt_bc2;
};
__device__ __forceinline__ AdamwHyper adamw_hyper(const float* __restrict__ hyper, float beta1, float beta2) {
    const float lr = hyper[0];
    const double step = (double)reinterpret_cast<const unsigned*>(hyper)[1];
    const float inv_bc1 = (float)(1.0 / (1.0 - pow((double)beta1, step)));
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, step)));
    return {lr, inv_bc1, inv_sqrt_bc2};
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                     float beta1, float beta2, float eps, float wd, float inv_bc1,
                                                     float inv_sqrt_bc2, float grad_scale) {
    adamw_update(p, g, m, v, n, lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2, grad_scale);
}

__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, long n,
                                                         const float* __restrict__ hyper, float beta1, float beta2, float eps,
                                                         float wd, float grad_scale) {
    const AdamwHyper h = adamw_hyper(hyper, beta1, beta2);
    adamw_update(p, g, m, v, n, h.lr, beta1, beta2, eps, wd, h.inv_bc1, h.inv_sqrt_bc2, grad_scale);
}

}  // namespace

constexpr int LG_MAX_BLOCKS = 768;   // three 4-wave workgroups per CU

static int lora_blocks(int M) {   // >= 8 rows per wave, clamped to [1, LG_MAX_BLOCKS]
    const int blocks = ceil_div(M, 4 * 8);
    return blocks > LG_MAX_BLOCKS ? LG_MAX_BLOCKS : blocks < 1 ? 1 : blocks;
}
// the workspace's two slabs of per-block partial sums, each [LG_MAX_BLOCKS][8 H] floats: pa (dB) at the base, pb (dA) behind it
static size_t lora_slab_floats(int H) { return (size_t)LG_MAX_BLOCKS * 8 * H; }

extern "C" int64_t bsclip_lora_grad_workspace_floats(int H) { return (int64_t)(2 * lora_slab_floats(H)); }

extern "C" int bsclip_lora_grad(const void* dqkv, int ld_dqkv, const void* h, int ld_h, int M, int H,
                                const float* lora_b, float* dt, float* dA, float* dBq, float* dBv, float* workspace,
                                void* stream) {
    BSCLIP_REQUIRE(dqkv && h && lora_b && dt && dA && dBq && dBv && workspace && M > 0,
                   "bsclip_lora_grad: null/empty input");
    BSCLIP_REQUIRE(H == 768 || H == 512, "bsclip_lora_grad: H=%d (supported: 768, 512)", H);
    BSCLIP_REQUIRE(ld_dqkv >= 3 * H && ld_dqkv % 4 == 0 && ld_h >= H + 8 && ld_h % 8 == 0,
                   "bsclip_lora_grad: ld_dqkv=%d ld_h=%d", ld_dqkv, ld_h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = lora_blocks(M);
    const bf16_t* g = static_cast<const bf16_t*>(dqkv);
    const bf16_t* hh = static_cast<const bf16_t*>(h);
    float* pa = workspace;
    float* pb = workspace + lora_slab_floats(H);
    pick_int<768, 512>(H, [&](auto h_) {
        constexpr int HH = decltype(h_)::value;
        hipLaunchKernelGGL((lora_grad_dt_db_kernel<HH>), dim3(blocks), dim3(LG_BLOCK), 0, s, g, ld_dqkv, hh, ld_h, M, lora_b, dt, pa);
        hipLaunchKernelGGL((lora_grad_da_kernel<HH>), dim3(blocks), dim3(LG_BLOCK), 0, s, hh, ld_h, M, dt, pb);
        hipLaunchKernelGGL((lora_grad_reduce_kernel<HH>), dim3(16 * HH / 32), dim3(256), 0, s, pa, pb, blocks, dA, dBq, dBv);
    });
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// bsclip_lora_grad when the attention backward already left dt / dB as partial sums (bsclip_attn_bwd_lora): reduce them, then the dA pass.
// dt_partial f32 [heads][2][M][4], db_partial f32 [B * heads][2][4][64] (B sequences of M / B tokens; item = sequence * heads + head).
extern "C" int bsclip_lora_grad_heads(const void* h, int ld_h, int M, int H, int B, const float* dt_partial,
                                      const float* db_partial, float* dt, float* dA, float* dBq, float* dBv, float* workspace,
                                      void* stream) {
    BSCLIP_REQUIRE(h && dt_partial && db_partial && dt && dA && dBq && dBv && workspace && M > 0 && B > 0 && M % B == 0,
                   "bsclip_lora_grad_heads: null/empty input (M=%d B=%d)", M, B);
    BSCLIP_REQUIRE(H == 768 || H == 512, "bsclip_lora_grad_heads: H=%d (supported: 768, 512)", H);
    BSCLIP_REQUIRE(ld_h >= H && ld_h % 8 == 0, "bsclip_lora_grad_heads: ld_h=%d", ld_h);
    BSCLIP_REQUIRE(aligned_to(16, dt_partial, dt),
                   "bsclip_lora_grad_heads: dt_partial and dt must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int heads = H / 64;
    const int blocks = lora_blocks(M);
    const bf16_t* hh = static_cast<const bf16_t*>(h);
    float* pb = workspace + lora_slab_floats(H);
    const int nA = ceil_div(2 * M, 256);
    hipLaunchKernelGGL(lora_heads_reduce_kernel<false>, dim3(nA + heads * 512 / 32), dim3(256), 0, s, dt_partial, db_partial, M, heads, B, nA,
                       dt, dBq, dBv);
    pick_int<768, 512>(H, [&](auto h_) {
        constexpr int HH = decltype(h_)::value;
        hipLaunchKernelGGL((lora_grad_da_kernel<HH>), dim3(blocks), dim3(LG_BLOCK), 0, s, hh, ld_h, M, dt, pb);
        hipLaunchKernelGGL((lora_grad_reduce_kernel<HH>), dim3(8 * HH / 32), dim3(256), 0, s, (const float*)nullptr, pb, blocks, dA, dBq,
                           dBv, 8 * HH / 32);
    });
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// bsclip_lora_grad_heads on fp16 operands with the static gradient scale 2^s of the fp16 backward: operands = BSCLIP_OPERANDS_FP16 | s
// (s in the low byte, <= 64).  h (LN output) is fp16; the partials, dt and the dA slabs hold 2^s times the gradient; dt is left scaled
// (the LayerNorm backward's dt.A term adds it to the scaled gradient stream), dA / dBq / dBv receive the sums times 2^-s (exact in f32).
extern "C" int bsclip_lora_grad_heads_f16(const void* h, int ld_h, int M, int H, int B, const float* dt_partial,
                                          const float* db_partial, float* dt, float* dA, float* dBq, float* dBv, float* workspace,
                                          int operands, void* stream) {
    bool f16 = false;
    BSCLIP_REQUIRE(take_operands_flag(operands, f16), "bsclip_lora_grad_heads_f16: unknown bits in operands=0x%x", operands);
    BSCLIP_REQUIRE(f16 && operands <= 64, "bsclip_lora_grad_heads_f16: operands=0x%x must be BSCLIP_OPERANDS_FP16 | s, s <= 64",
                   operands);
    BSCLIP_REQUIRE(h && dt_partial && db_partial && dt && dA && dBq && dBv && workspace && M > 0 && B > 0 && M % B == 0,
                   "bsclip_lora_grad_heads_f16: null/empty input (M=%d B=%d)", M, B);
    BSCLIP_REQUIRE(H == 768, "bsclip_lora_grad_heads_f16: H=%d (the ViT's 768)", H);
    BSCLIP_REQUIRE(ld_h >= H && ld_h % 8 == 0, "bsclip_lora_grad_heads_f16: ld_h=%d", ld_h);
    BSCLIP_REQUIRE(aligned_to(16, dt_partial, dt, workspace, h),
                   "bsclip_lora_grad_heads_f16: h, dt_partial, dt and workspace must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float unscale = ldexpf(1.f, -operands);
    const int heads = H / 64;
    const int blocks = lora_blocks(M);
    const bf16_t* hh = static_cast<const bf16_t*>(h);
    float* pb = workspace + lora_slab_floats(H);
    const int nA = ceil_div(2 * M, 256);
    hipLaunchKernelGGL(lora_heads_reduce_kernel<true>, dim3(nA + heads * 512 / 32), dim3(256), 0, s, dt_partial, db_partial, M, heads, B,
                       nA, dt, dBq, dBv, unscale);
    hipLaunchKernelGGL((lora_grad_da_kernel<768, false, false, true>), dim3(blocks), dim3(LG_BLOCK), 0, s, hh, ld_h, M, dt, pb);
    hipLaunchKernelGGL((lora_grad_reduce_kernel<768, true>), dim3(8 * 768 / 32), dim3(256), 0, s, (const float*)nullptr, pb, blocks, dA,
                       dBq, dBv, 8 * 768 / 32, unscale);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// out[i] += 2^scale_log2 * in[i] (f32, 16-byte aligned): a weight gradient of the fp16-operand backward, formed in the 2^s units of its
// scaled operands, enters the gradient buffer at its true size (the multiply by a power of two is exact)
__global__ __launch_bounds__(256) void add_scaled_f32_kernel(const float* __restrict__ in, long n, float scale, float* __restrict__ out) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(in + 4 * i);
        f32x4 o = *reinterpret_cast<const f32x4*>(out + 4 * i);
        o += v * scale;
        *reinterpret_cast<f32x4*>(out + 4 * i) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        out[i] += in[i] * scale;
    }
}

extern "C" int bsclip_add_scaled_f32(const float* in, int64_t n, int scale_log2, float* out, void* stream) {
    BSCLIP_REQUIRE(in && out && n > 0, "bsclip_add_scaled_f32: bad args");
    BSCLIP_REQUIRE(scale_log2 >= -64 && scale_log2 <= 64, "bsclip_add_scaled_f32: scale_log2=%d (|k| <= 64)", scale_log2);
    BSCLIP_REQUIRE(aligned_to(16, in, out),
                   "bsclip_add_scaled_f32: in and out must be 16-byte aligned");
    hipLaunchKernelGGL(add_scaled_f32_kernel, dim3(grid4x256(n, 1024)), dim3(256), 0, static_cast<hipStream_t>(stream), in, (long)n,
                       ldexpf(1.f, scale_log2), out);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// exact mode (BSCLIP_PARITY=2): f32 dq / dv and the f32 LayerNorm output y; t = A y is rebuilt (the forward folds W + B A), then the
// kernels of bsclip_lora_grad on f32 rows.  workspace: [t: 8 M][dt: 8 M][slabs: LG_MAX_BLOCKS * 16 H] floats.
// Reference lora_layer.py:16-39 / image_encoder.py:44-47 / dna_encoder.py:47-49:
//   u_q = B_q^T dq, u_v = B_v^T dv;  dA_q += u_q y^T, dA_v += u_v y^T, dB_q += dq t_q^T, dB_v += dv t_v^T
extern "C" int64_t bsclip_lora_grad_f32_workspace_floats(int M, int H) {
    return M > 0 && H > 0 ? 16 * (int64_t)((M + 3) / 4 * 4) + (int64_t)(2 * lora_slab_floats(H)) : -1;
}

extern "C" int bsclip_lora_grad_f32(const float* dqkv, int ld_dqkv, const float* y, int ld_y, int M, int H, const float* lora_a,
                                    const float* lora_b, float* dA, float* dB, float* workspace, void* stream) {
    BSCLIP_REQUIRE(dqkv && y && lora_a && lora_b && dA && dB && workspace, "bsclip_lora_grad_f32: null pointer");
    BSCLIP_REQUIRE(M > 0 && (H == 768 || H == 512) && ld_dqkv >= 3 * H && ld_dqkv % 4 == 0 && ld_y >= H && ld_y % 4 == 0,
                   "bsclip_lora_grad_f32: M=%d H=%d ld_dqkv=%d ld_y=%d", M, H, ld_dqkv, ld_y);
    BSCLIP_REQUIRE(aligned_to(16, dqkv, y, lora_a, lora_b, workspace),
                   "bsclip_lora_grad_f32: dqkv, y, lora_a, lora_b and workspace must be 16-byte aligned (vector loads)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = lora_blocks(M);
    const size_t Mp = (size_t)(M + 3) / 4 * 4;
    float* t = workspace;
    float* dt = workspace + 8 * Mp;
    float* pa = workspace + 16 * Mp;
    float* pb = pa + lora_slab_floats(H);
    float* dBq = dB;
    float* dBv = dB + (size_t)H * 4;
    pick_int<768, 512>(H, [&](auto h_) {
        constexpr int HH = decltype(h_)::value;
        hipLaunchKernelGGL((lora_t_f32_kernel<HH>), dim3(blocks), dim3(LG_BLOCK), 0, s, y, ld_y, M, lora_a, t);
        hipLaunchKernelGGL((lora_grad_dt_db_kernel<HH, true>), dim3(blocks), dim3(LG_BLOCK), 0, s, dqkv, ld_dqkv, t, 8, M, lora_b, dt, pa);
        hipLaunchKernelGGL((lora_grad_da_kernel<HH, false, true>), dim3(blocks), dim3(LG_BLOCK), 0, s, y, ld_y, M, dt, pb);
        hipLaunchKernelGGL((lora_grad_reduce_kernel<HH>), dim3(16 * HH / 32), dim3(256), 0, s, pa, pb, blocks, dA, dBq, dBv);
    });
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// fp8 operand path (BASELINE configs[4]): y is the fp8 LN output [M, ld_y bytes], t the separate bf16 block [M, ld_t]
extern "C" int bsclip_lora_grad_fp8(const void* dqkv, int ld_dqkv, const void* y_fp8, int ld_y, const void* t_aug, int ld_t,
                                    int M, int H, const float* lora_b, float* dt, float* dA, float* dBq, float* dBv,
                                    float* workspace, void* stream) {
    BSCLIP_REQUIRE(dqkv && y_fp8 && t_aug && lora_b && dt && dA && dBq && dBv && workspace && M > 0,
                   "bsclip_lora_grad_fp8: null/empty input");
    BSCLIP_REQUIRE(H == 768 || H == 512, "bsclip_lora_grad_fp8: H=%d (supported: 768, 512)", H);
    BSCLIP_REQUIRE(ld_dqkv >= 3 * H && ld_dqkv % 4 == 0 && ld_y >= H && ld_y % 4 == 0 && ld_t >= 8 && ld_t % 8 == 0,
                   "bsclip_lora_grad_fp8: ld_dqkv=%d ld_y=%d ld_t=%d", ld_dqkv, ld_y, ld_t);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = lora_blocks(M);
    const bf16_t* g = static_cast<const bf16_t*>(dqkv);
    const bf16_t* tt = static_cast<const bf16_t*>(t_aug) - H;   // the kernel reads t at column H of its "haug" row
    const bf16_t* yy = static_cast<const bf16_t*>(y_fp8);
    float* pa = workspace;
    float* pb = workspace + lora_slab_floats(H);
    pick_int<768, 512>(H, [&](auto h_) {
        constexpr int HH = decltype(h_)::value;
        hipLaunchKernelGGL((lora_grad_dt_db_kernel<HH>), dim3(blocks), dim3(LG_BLOCK), 0, s, g, ld_dqkv, tt, ld_t, M, lora_b, dt, pa);
        hipLaunchKernelGGL((lora_grad_da_kernel<HH, true>), dim3(blocks), dim3(LG_BLOCK), 0, s, yy, ld_y, M, dt, pb);
        hipLaunchKernelGGL((lora_grad_reduce_kernel<HH>), dim3(16 * HH / 32), dim3(256), 0, s, pa, pb, blocks, dA, dBq, dBv);
    });
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_colsum(const void* g, int ld_g, int g_is_bf16, int M, int N, float* out, void* stream) {
    BSCLIP_REQUIRE(g && out && M > 0 && N > 0 && ld_g >= N, "bsclip_colsum: bad args");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool wide = N % 8 == 0 && ld_g % 8 == 0 && aligned_to(16, g);
    pick_bool(g_is_bf16 != 0, [&](auto bf) {
        constexpr bool BF = decltype(bf)::value;
        if (wide) hipLaunchKernelGGL((colsum8_kernel<BF>), dim3(N / 8), dim3(256), 0, s, g, ld_g, M, N, out);
        else hipLaunchKernelGGL((colsum_kernel<BF>), dim3(ceil_div(N, 32)), dim3(256), 0, s, g, ld_g, M, N, out);
    });
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

static unsigned adamw_grid(int64_t n) {   // AdamW kernels, swap_f32: 256 elements per workgroup, grid-stride beyond 2048 workgroups
    const int64_t blocks = (n + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

extern "C" int bsclip_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int step, float grad_scale,
                                 void* stream) {
    BSCLIP_REQUIRE(p && g && m && v && n > 0 && step >= 1, "bsclip_adamw_step: bad args (n=%ld step=%d)", (long)n, step);
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adamw_kernel, dim3(adamw_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v,
                       (long)n, lr, beta1, beta2, eps, weight_decay, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)),
                       grad_scale);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                                     float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
    BSCLIP_REQUIRE(p && g && m && v && hyper_dev && n > 0, "bsclip_adamw_step_dev: null/empty input");
    hipLaunchKernelGGL(adamw_dev_kernel, dim3(adamw_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v,
                       (long)n, hyper_dev, beta1, beta2, eps, weight_decay, grad_scale);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// ---- global gradient norm, clipping and overflow-safe steps ----------------------------------------------------------
// grad_sumsq : per-workgroup f64 sums of g^2 over one flat gradient buffer (one HBM pass, fixed order, no atomics)
// grad_clip_finish : one workgroup sums every buffer's partials in index order and leaves (apply, coef, norm, counters) in a device
//               record -- torch.nn.utils.clip_grad_norm_'s coefficient, GradScaler's "skip the step when the gradient is not finite"
// counter_add_if / adamw_clip : the step word and the update, both conditional on the record's `apply`
namespace {

constexpr int GN_BLOCK = 256;
constexpr long GN_SPAN = 8192;        // elements a workgroup owns at least: two rounds of four 16-byte loads per thread
constexpr long GN_MAX_PARTIALS = 1024;   // four workgroups per CU; beyond GN_SPAN * GN_MAX_PARTIALS elements the spans grow
constexpr int GC_TILE = 1024;         // partials staged through LDS per round of grad_clip_finish_kernel

__device__ __forceinline__ double sumsq4(f32x4 v) {   // the square of an f32 is exact in f64
    const double a = (double)v[0], b = (double)v[1], c = (double)v[2], d = (double)v[3];
    return (a * a + b * b) + (c * c + d * d);
}

// Workgroup b owns the 16-byte vectors [b * chunk, (b + 1) * chunk) of g (chunk = ceil((n / 4) / gridDim.x)); the last workgroup also
// owns the n % 4 tail elements.  Thread t takes vectors t, t + 256, ... of the chunk, four loads in flight; the 256 sums are combined
// in a fixed order: the lanes of a wave by xor-shuffles, the four waves in wave order through LDS.
__global__ __launch_bounds__(GN_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ partial) {
    __shared__ double red[GN_BLOCK / 64];
    const long nvec = n >> 2;
    const long chunk = (nvec + gridDim.x - 1) / gridDim.x;
    const long lo = min((long)blockIdx.x * chunk, nvec), hi = min(lo + chunk, nvec);
    const f32x4* src = reinterpret_cast<const f32x4*>(g);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long i = lo + threadIdx.x;
    for (; i + 3 * GN_BLOCK < hi; i += 4 * GN_BLOCK) {
        const f32x4 v0 = src[i], v1 = src[i + GN_BLOCK], v2 = src[i + 2 * GN_BLOCK], v3 = src[i + 3 * GN_BLOCK];
        s0 += sumsq4(v0);
        s1 += sumsq4(v1);
        s2 += sumsq4(v2);
        s3 += sumsq4(v3);
    }
    for (; i < hi; i += GN_BLOCK) s0 += sumsq4(src[i]);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < (n & 3)) {
        const double t = (double)g[(nvec << 2) + threadIdx.x];
        s1 += t * t;
    }
    double s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// state: twelve 4-byte words (include/bsclip.h).  The partials are staged through LDS a tile at a time and summed by ONE thread in
// index order: a few thousand dependent f64 adds at the most (three buffers at the cap), microseconds beside the pass that made them.
__global__ __launch_bounds__(GN_BLOCK) void grad_clip_finish_kernel(const double* __restrict__ partial, long n_partial, float max_norm,
                                                                     unsigned* __restrict__ state) {
    __shared__ double tile[GC_TILE];
    double total = 0.0;
    for (long base = 0; base < n_partial; base += GC_TILE) {
        const int cnt = (int)min((long)GC_TILE, n_partial - base);
        for (int k = threadIdx.x; k < cnt; k += GN_BLOCK) tile[k] = partial[base + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < cnt; ++k) total += tile[k];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const bool finite = isfinite(total);
    const double root = sqrt(total);
    const float norm = (float)root;
    const float coef = finite ? (float)fmin(1.0, (double)max_norm / (root + 1e-6)) : 0.f;
    const unsigned clipped = finite && coef < 1.f ? 1u : 0u;
    double* sums = reinterpret_cast<double*>(state + 8);   // state is 16-byte aligned
    state[0] = finite ? 1u : 0u;
    state[1] = __float_as_uint(coef);
    state[2] = __float_as_uint(norm);
    state[3] = clipped;
    state[4] += 1u;
    state[5] += finite ? 0u : 1u;
    state[6] += clipped;
    state[7] = 0u;
    if (finite) {
        sums[0] += (double)norm;
        sums[1] = fmax(sums[1], (double)norm);
    }
}

__global__ void counter_add_if_kernel(unsigned* p, unsigned inc, const unsigned* cond) {
    if (*cond != 0u) *p += inc;
}

// adamw_dev_kernel (the same adamw_hyper and adamw_update) with the gradient multiplied by the record's coef and nothing stored when
// the record says skip (state[0] == 0: the gradient was not finite)
__global__ __launch_bounds__(256) void adamw_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, long n,
                                                          const float* __restrict__ hyper, const unsigned* __restrict__ state,
                                                          float beta1, float beta2, float eps, float wd) {
    if (state[0] == 0u) return;
    const float grad_scale = __uint_as_float(state[1]);
    const AdamwHyper h = adamw_hyper(hyper, beta1, beta2);
    adamw_update(p, g, m, v, n, h.lr, beta1, beta2, eps, wd, h.inv_bc1, h.inv_sqrt_bc2, grad_scale);
}

// adamw_dev_kernel (CLIP = false, state unused) or adamw_clip_kernel (CLIP = true) with the weight average updated by the same thread
// (adamw_update<true>).  The average's weight w = 1 - d_t is one value per launch, formed in f64 from the step word like the bias
// corrections: t counts applied steps, this one included; warm-up caps the decay at (1 + t) / (10 + t).
template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, float* __restrict__ ema, long n,
                                                         const float* __restrict__ hyper, const unsigned* __restrict__ state,
                                                         float beta1, float beta2, float eps, float wd, float ema_decay,
                                                         int ema_warmup) {
    float grad_scale = 1.0f;
    if constexpr (CLIP) {
        if (state[0] == 0u) return;
        grad_scale = __uint_as_float(state[1]);
    }
    const AdamwHyper h = adamw_hyper(hyper, beta1, beta2);
    const double t = (double)reinterpret_cast<const unsigned*>(hyper)[1];
    const double d_t = ema_warmup ? fmin((double)ema_decay, (1.0 + t) / (10.0 + t)) : (double)ema_decay;
    const float w = (float)(1.0 - d_t);
    adamw_update<true>(p, g, m, v, n, h.lr, beta1, beta2, eps, wd, h.inv_bc1, h.inv_sqrt_bc2, grad_scale, ema, w);
}

__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

// true when the n-float ranges at a and b share no byte
inline bool disjoint_f32(const float* a, const float* b, int64_t n) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * sizeof(float);
    return x + bytes <= y || y + bytes <= x;
}

}  // namespace

extern "C" int64_t bsclip_grad_norm_partials(int64_t n) {
    if (n <= 0) {
        bsclip_set_error("bsclip_grad_norm_partials: n=%ld must be positive", (long)n);
        return -1;
    }
    const int64_t blocks = (n + GN_SPAN - 1) / GN_SPAN;
    return blocks > GN_MAX_PARTIALS ? GN_MAX_PARTIALS : blocks;
}

extern "C" int bsclip_grad_sumsq_partial(const float* g, int64_t n, double* partial, void* stream) {
    BSCLIP_REQUIRE(g, "bsclip_grad_sumsq_partial: g is null");
    BSCLIP_REQUIRE(partial, "bsclip_grad_sumsq_partial: partial is null");
    BSCLIP_REQUIRE(n > 0, "bsclip_grad_sumsq_partial: n=%ld must be positive", (long)n);
    BSCLIP_REQUIRE(aligned_to(16, g), "bsclip_grad_sumsq_partial: g must be 16-byte aligned (vector loads)");
    BSCLIP_REQUIRE(aligned_to(8, partial), "bsclip_grad_sumsq_partial: partial must be 8-byte aligned (f64)");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)bsclip_grad_norm_partials(n)), dim3(GN_BLOCK), 0,
                       static_cast<hipStream_t>(stream), g, (long)n, partial);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_grad_clip_finish(const double* partial, int64_t n_partial, float max_norm, void* state, void* stream) {
    BSCLIP_REQUIRE(partial, "bsclip_grad_clip_finish: partial is null");
    BSCLIP_REQUIRE(state, "bsclip_grad_clip_finish: state is null");
    BSCLIP_REQUIRE(n_partial > 0, "bsclip_grad_clip_finish: n_partial=%ld must be positive", (long)n_partial);
    BSCLIP_REQUIRE(max_norm > 0.f, "bsclip_grad_clip_finish: max_norm=%g must be positive (+inf: no clipping)", (double)max_norm);
    BSCLIP_REQUIRE(aligned_to(8, partial), "bsclip_grad_clip_finish: partial must be 8-byte aligned (f64)");
    BSCLIP_REQUIRE(aligned_to(16, state), "bsclip_grad_clip_finish: state must be 16-byte aligned");
    hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(GN_BLOCK), 0, static_cast<hipStream_t>(stream), partial, (long)n_partial,
                       max_norm, static_cast<unsigned*>(state));
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_counter_add_if(uint32_t* counter, uint32_t inc, const uint32_t* cond, void* stream) {
    BSCLIP_REQUIRE(counter, "bsclip_counter_add_if: counter is null");
    BSCLIP_REQUIRE(cond, "bsclip_counter_add_if: cond is null");
    BSCLIP_REQUIRE(aligned_to(4, counter, cond), "bsclip_counter_add_if: counter and cond must be 4-byte aligned");
    hipLaunchKernelGGL(counter_add_if_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), counter, inc, cond);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_adamw_step_clip(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, const void* state,
                                      float beta1, float beta2, float eps, float weight_decay, void* stream) {
    BSCLIP_REQUIRE(p && g && m && v, "bsclip_adamw_step_clip: null pointer among p, g, m, v");
    BSCLIP_REQUIRE(hyper_dev, "bsclip_adamw_step_clip: hyper_dev is null");
    BSCLIP_REQUIRE(state, "bsclip_adamw_step_clip: state is null");
    BSCLIP_REQUIRE(n > 0, "bsclip_adamw_step_clip: n=%ld must be positive", (long)n);
    BSCLIP_REQUIRE(aligned_to(4, p, g, m, v, hyper_dev), "bsclip_adamw_step_clip: p, g, m, v and hyper_dev must be 4-byte aligned");
    BSCLIP_REQUIRE(aligned_to(16, state), "bsclip_adamw_step_clip: state must be 16-byte aligned");
    hipLaunchKernelGGL(adamw_clip_kernel, dim3(adamw_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, (long)n,
                       hyper_dev, static_cast<const unsigned*>(state), beta1, beta2, eps, weight_decay);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_adamw_step_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* hyper_dev,
                                     const void* clip_state, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                                     int ema_warmup, void* stream) {
    BSCLIP_REQUIRE(p && g && m && v, "bsclip_adamw_step_ema: null pointer among p, g, m, v");
    BSCLIP_REQUIRE(ema, "bsclip_adamw_step_ema: ema is null");
    BSCLIP_REQUIRE(hyper_dev, "bsclip_adamw_step_ema: hyper_dev is null");
    BSCLIP_REQUIRE(n > 0, "bsclip_adamw_step_ema: n=%ld must be positive", (long)n);
    BSCLIP_REQUIRE(aligned_to(4, p, g, m, v, ema, hyper_dev), "bsclip_adamw_step_ema: p, g, m, v, ema and hyper_dev must be 4-byte aligned");
    BSCLIP_REQUIRE(aligned_to(16, clip_state), "bsclip_adamw_step_ema: clip_state must be 16-byte aligned (or NULL)");
    BSCLIP_REQUIRE(ema_decay > 0.f && ema_decay < 1.f, "bsclip_adamw_step_ema: ema_decay=%g must lie strictly inside (0, 1)",
                   (double)ema_decay);
    BSCLIP_REQUIRE(disjoint_f32(ema, p, n) && disjoint_f32(ema, g, n) && disjoint_f32(ema, m, n) && disjoint_f32(ema, v, n),
                   "bsclip_adamw_step_ema: ema must not alias p, g, m or v");
    pick_bool(clip_state != nullptr, [&](auto clip) {
        hipLaunchKernelGGL((adamw_ema_kernel<decltype(clip)::value>), dim3(adamw_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           p, g, m, v, ema, (long)n, hyper_dev, static_cast<const unsigned*>(clip_state), beta1, beta2, eps, weight_decay,
                           ema_decay, ema_warmup);
    });
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_swap_f32(float* a, float* b, int64_t n, void* stream) {
    BSCLIP_REQUIRE(a && b, "bsclip_swap_f32: null pointer");
    BSCLIP_REQUIRE(n > 0, "bsclip_swap_f32: n=%ld must be positive", (long)n);
    BSCLIP_REQUIRE(aligned_to(4, a, b), "bsclip_swap_f32: a and b must be 4-byte aligned");
    BSCLIP_REQUIRE(disjoint_f32(a, b, n), "bsclip_swap_f32: a and b must not be the same or overlapping ranges");
    hipLaunchKernelGGL(swap_f32_kernel, dim3(adamw_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, (long)n);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
