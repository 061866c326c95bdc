// What the GEMM kernels do to a finished piece of an output row -- the ONE definition the four kernel families share.
//
// Included by gemm.hip inside its anonymous namespace, ahead of the kernels.  Holds EpiArgs, the GELU table, and the row-piece
// epilogue in three steps:
//   epi_fetch / epi_cook   the second operand (residual row, gelu' codes, position row) of four output columns: raw words, then f32;
//   (dropout)              stays at the call site, see epi_finish_store;
//   epi_finish_store       + resid or * gelu', the patch-row remap, pack, store through the kernel's store policy.
// gemm_nt_kernel (epilogue_store below) applies them to accumulator registers, the 256-wide kernels (gemm_pp.h, gemm_duo.h,
// gemm_pers.h) to rows they read back from an LDS slab.  tests/test_70_configs_gpu.py and test_gemm_persistent_walks_tiles require
// a row's result not to depend on the kernel its shape selects: that holds because they all come through here.  The BF16 / GELU
// staging paths differ in slab geometry per kernel and live with their kernels.
// Every form in this file was chosen so that each kernel assembles to the instructions it had before the epilogues were shared
// (tools/asm_kernel_diff.py, profiles/gemm_epilogue_refactor.jsonl); the comments say where a plainer form did not.

struct EpiArgs {
    const float* bias;
    const float* resid;   // RESID_BF16: bf16 data behind the same pointer
    int ld_resid;
    unsigned char* aux;  // gelu' side band, 8-bit codes (common.h dg8_*)
    int ld_aux;
    DropCfg drop;  // RESID only: C = dropout(acc + bias) + resid  (HF BertSelfOutput / BertOutput)
    int n_total;   // logical row width for the dropout element index
    unsigned long long* diag;  // diagnostic build only: per-workgroup phase stamps (100 MHz wall clock)
    int pers_gw;               // persistent kernel: column tiles per super-column of its tile order (set by launch_pers)
    // fp8 main operands (OP != 0): C = epilogue(alpha[n] * (A8 . B8^T + A_aug . B_aug^T) + bias)
    union {
        const float* alpha;               // [N] dequantisation scale of output column n (activation scale x weight-row scale)
        // trainable temperature (EPI_LSE_PART_TS / EPI_LOSS_W_TS, never fp8; shares the slot so that no kernel's argument block
        // changes): scale_dev[1] is the logit scale, read when the kernel runs; `coef` then holds the divisor P N of scale / (P N)
        const float* scale_dev;
    };
    const bf16_t* a_aug;                  // bf16 [M, 64] K-augmentation block (LoRA t columns), nullable
    const bf16_t* b_aug;                  // bf16 [N, 64] matching weight columns (LoRA B / alpha[n])
    int ld_a_aug, ld_b_aug;
    // fused InfoNCE epilogues (EPI_LSE_PART / EPI_LOSS_W, internal: bsclip_gemm_infonce): the accumulator tile holds cosines
    const int64_t* labels;                // [>= n_valid]
    const float* cnt;                     // cnt[i] = #{j : label_j == label_i}
    const float* lse_row;                 // LSE of the rows of THIS product (a -> b), indexed by global row
    const float* lse_col;                 // LSE of the transposed product (b -> a), indexed by column
    float* part;                          // EPI_LSE_PART out: [M, tiles_n, 4] = (row max, sum exp, sum_j T_ij x_ij, -)
    float logit_scale, coef;              // x = logit_scale * cosine;  w = coef * (...)
    int n_valid, row_base;                // columns >= n_valid are padding; global row of local row 0
    // split-K (bsclip_gemm_splitk_f32; EPI_F32 without bias only): workgroups with blockIdx.y = z reduce K columns
    // [z K, (z + 1) K) of the operands into their own f32 slab C + z * split_stride
    long split_stride;
};
constexpr int EPI_LSE_PART = 100;  // internal epilogues, not part of the public enum
constexpr int EPI_LOSS_W = 101;
// the same two with the scale in device memory; pass 1 also fills part[..][3] = sum_j exp(x_ij - max) G_ij (for dLoss/dt)
constexpr int EPI_LSE_PART_TS = 102;
constexpr int EPI_LOSS_W_TS = 103;

// ---------------------------------------------------------------------------------------------------------------
// GELU table for the 256x256 kernel's epilogue
// ---------------------------------------------------------------------------------------------------------------
// The two-output GELU epilogue (gelu and gelu' of 128 values per lane) computed with exp + rcp was VALU-bound (~24
// instructions per value, 12 us per tile with no MFMA to hide behind), and a 16-B-per-entry interpolation table was bound by
// the LDS array instead: 64 lanes gathering random 16-B entries conflict ~3x per 16-lane group (phase stamps: 4.4 us per
// 64-row slab).  Entries are therefore 8 B -- {Phi(x_i), phi(x_i)}, nearest grid point, one ds_read_b64 per value -- and the
// neighbourhood comes from the derivatives, which are free: Phi' = phi, phi' = -x phi.
// Round 3: the epilogue is still VALU-bound (8.8 us of a 30-us fc1 tile), so the index arithmetic went on a diet.  256 entries on
// a 1/16 grid over [-8, 8): the index is ONE v_cvt_pk_u8_f32 (round to nearest even, saturating at 0 / 255) of t = 16 x + 128
// -- no clamp, no float->int->float round trip beyond v_cvt_f32_ubyte0 -- and saturated inputs are harmless because
// phi(+-8) ~ 5e-15 multiplies whatever distance they have from the last grid point.  With d = x - x_i, |d| <= 1/32:
//   Phi(x_i + d) = Phi_i + d phi_i (1 - x_i d / 2) + O(d^3 |phi''| / 6) <= 2e-6   (first order alone leaves 1.2e-4: a third of
//                                                                       the e4m3 / a tenth of the bf16 rounding of the output),
//   phi(x_i + d) = phi_i (1 - x_i d)               + O(d^2 phi / 2)     <= 2e-4   (8-bit code step of gelu': 4.9e-3).
// Computed once on the device in f64 with erf().
constexpr int GELU_LUT_N = 255;                       // last index
constexpr int GELU_LUT_BYTES = (GELU_LUT_N + 1) * 8;  // 2048
__device__ float2 g_gelu_lut[GELU_LUT_N + 1];

__global__ void gelu_lut_init_kernel() {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > GELU_LUT_N) return;
    const double x = -8.0 + i / 16.0;
    g_gelu_lut[i] = float2{(float)(0.5 * (1.0 + erf(x * 0.70710678118654752440))),
                           (float)(0.39894228040143267794 * exp(-0.5 * x * x))};
}

// Host side.  ensure_gelu_lut fills the table once per process, stream-ordered ahead of the first consumer on `s`.
bool g_lut_ready = false;
void launch_gelu_lut(hipStream_t s) { hipLaunchKernelGGL(gelu_lut_init_kernel, dim3(ceil_div(GELU_LUT_N + 1, 256)), dim3(256), 0, s); }
void ensure_gelu_lut(hipStream_t s) {
    if (g_lut_ready) return;
    launch_gelu_lut(s);
    g_lut_ready = true;
}

// Two values per call so that the arithmetic runs on the packed-f32 VALU (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32); the
// index conversions and the table address stay per value.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gelu_lut2(const char* lut, f32x2 x, f32x2& gl, f32x2& dg) {
    const f32x2 t = x * 16.0f + 128.0f;
    f32x2 Phi, phi;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned i = __builtin_amdgcn_cvt_pk_u8_f32(t[k], 0, 0u);   // nearest grid point (RNE), saturated to [0, 255]
        const float2 e = *reinterpret_cast<const float2*>(lut + i * 8);
        Phi[k] = e.x;
        phi[k] = e.y;
    }
    // the grid point as a float without a per-value conversion: (t + 1.5 * 2^23) - 1.5 * 2^23 = RNE(t) for |t| < 2^22, packed.
    // A saturated index keeps its small d here and takes its table entry from the end of the grid, where phi ~ 5e-15.
    f32x2 fi = t + 12582912.0f;
    asm volatile("" : "+v"(fi));   // keep the two additions apart
    fi -= 12582912.0f;
    const f32x2 d16 = t - fi;                       // 16 (x - x_i)
    const f32x2 e = d16 * phi;                      // 16 d phi_i
    const f32x2 xd = (fi * 0.00390625f - 0.5f) * d16;   // x_i d  (x_i / 16 = i / 256 - 1 / 2)
    const f32x2 cdf = e * (0.0625f - xd * 0.03125f) + Phi;   // Phi_i + d phi_i (1 - x_i d / 2)
    const f32x2 pdf = phi - xd * phi;                        // phi_i (1 - x_i d)
    gl = x * cdf;
    dg = x * pdf + cdf;
}

// 4 NV values per call: ALL the table gathers are issued before the first result is used.  Written pair by pair (above)
// the compiler waits for each pair's two ds_read_b64 before the next pair's go out -- 64 serial LDS round trips per 128 values and
// lane with two waves per SIMD to hide them: the GELU epilogue was bound by LDS LATENCY (4.8 us per 64-row slab; cutting its VALU
// count by a fifth changed nothing), not by the VALU or the LDS array.
template <int NV>   // NV vectors of four values
__device__ __forceinline__ void gelu_lut_batch(const char* lut, const f32x4 (&x)[NV], f32x4 (&gl)[NV], f32x4 (&dg)[NV]) {
    f32x4 t[NV], Phi[NV], phi[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) t[q] = x[q] * 16.0f + 128.0f;
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned i = __builtin_amdgcn_cvt_pk_u8_f32(t[q][c], 0, 0u);   // nearest grid point (RNE), saturated to [0, 255]
            const float2 e = *reinterpret_cast<const float2*>(lut + i * 8);
            Phi[q][c] = e.x;
            phi[q][c] = e.y;
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        // the grid point as a float without a per-value conversion: (t + 1.5 * 2^23) - 1.5 * 2^23 = RNE(t) for |t| < 2^22, packed.
        // A saturated index keeps its small d here and takes its table entry from the end of the grid, where phi ~ 5e-15.
        f32x4 fi = t[q] + 12582912.0f;
        asm volatile("" : "+v"(fi));   // keep the two additions apart
        fi -= 12582912.0f;
        const f32x4 d16 = t[q] - fi;                       // 16 (x - x_i)
        const f32x4 e = d16 * phi[q];                      // 16 d phi_i
        const f32x4 xd = (fi * 0.00390625f - 0.5f) * d16;  // x_i d  (x_i / 16 = i / 256 - 1 / 2)
        const f32x4 cdf = e * (0.0625f - xd * 0.03125f) + Phi[q];   // Phi_i + d phi_i (1 - x_i d / 2)
        const f32x4 pdf = phi[q] - xd * phi[q];                     // phi_i (1 - x_i d)
        gl[q] = x[q] * cdf;
        dg[q] = x[q] * pdf + cdf;
    }
}

// four 16-bit values (bf16, or fp16 when F16) <-> f32
template <bool F16 = false>
__device__ __forceinline__ f32x4 bf4_to_f32(uint2 u) {
    return f32x4{h2f<F16>(u.x & 0xffff), h2f<F16>(u.x >> 16), h2f<F16>(u.y & 0xffff), h2f<F16>(u.y >> 16)};
}
template <bool F16 = false>
__device__ __forceinline__ uint2 f32_to_bf4(f32x4 v) { return uint2{pack_h2<F16>(v[0], v[1]), pack_h2<F16>(v[2], v[3])}; }
constexpr bool epi_is_resid(int epi) { return epi == BSCLIP_EPI_RESID_F32 || epi == BSCLIP_EPI_RESID_BF16; }
constexpr bool epi_is_patch(int epi) { return epi == BSCLIP_EPI_PATCH_F32 || epi == BSCLIP_EPI_PATCH_BF16; }
constexpr bool epi_out_bf16_from_f32_slab(int epi) {
    return epi == BSCLIP_EPI_DGELU_BF16 || epi == BSCLIP_EPI_RESID_BF16 || epi == BSCLIP_EPI_PATCH_BF16;
}

// ---------------------------------------------------------------------------------------------------------------
// the row-piece epilogue: four columns n .. n + 3 of output row m
// ---------------------------------------------------------------------------------------------------------------
// The second operand as it lies in memory.  Kept apart from its conversion so that a kernel can hold several slabs' worth of the
// narrow forms in flight (the persistent kernel: 2 VGPRs per piece of bf16 residual, 1 per piece of gelu' codes) and nothing
// waits for a load where it is issued.  m must be a valid row (callers clamp it); epilogues without a second operand get zeros.
// (two words as a native vector: HIP's uint2 class, returned by value, costs the persistent kernel its register allocation)
typedef unsigned epi_u32x2 __attribute__((ext_vector_type(2)));
template <int EPI>
using epi_raw_t = std::conditional_t<EPI == BSCLIP_EPI_RESID_BF16, epi_u32x2, std::conditional_t<EPI == BSCLIP_EPI_DGELU_BF16, unsigned, f32x4>>;

template <int EPI>
__device__ __forceinline__ epi_raw_t<EPI> epi_fetch(const EpiArgs& e, int m, int n) {
    if constexpr (EPI == BSCLIP_EPI_RESID_F32) {
        return *reinterpret_cast<const f32x4*>(e.resid + (size_t)m * e.ld_resid + n);
    } else if constexpr (EPI == BSCLIP_EPI_RESID_BF16) {
        return *reinterpret_cast<const epi_u32x2*>(reinterpret_cast<const bf16_t*>(e.resid) + (size_t)m * e.ld_resid + n);
    } else if constexpr (EPI == BSCLIP_EPI_DGELU_BF16) {
        return *reinterpret_cast<const unsigned*>(e.aux + (size_t)m * e.ld_aux + n);
    } else if constexpr (epi_is_patch(EPI)) {   // position row of patch m % 196 (row 0 is the class token's)
        return *reinterpret_cast<const f32x4*>(e.resid + (size_t)(1 + m % 196) * e.ld_resid + n);
    } else {
        return f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
template <int EPI, bool F16 = false>
__device__ __forceinline__ f32x4 epi_cook(const epi_raw_t<EPI>& raw) {
    if constexpr (EPI == BSCLIP_EPI_RESID_BF16) return bf4_to_f32<F16>(uint2{raw[0], raw[1]});
    else if constexpr (EPI == BSCLIP_EPI_DGELU_BF16) return dg8_unpack4(raw);
    else return raw;
}

// v holds acc (+ bias), already through dropout; r is the cooked second operand; st(pointer, f32x4 or uint2) is the kernel's store
// (taken by reference: a copy per call changes the persistent kernel's diagnostic builds).
// Dropout is NOT in here: the line
//     if (e.drop.thr16) v = drop4(e.drop, (unsigned)m * (unsigned)e.n_total + (unsigned)n, v);
// stays at each call site under `if constexpr (epi_is_resid(EPI))`.  Inside any function (this one, one of its own, with EpiArgs
// or with DropCfg alone as the argument) it shifts the register allocation of the RESID kernels of the ping-pong and duo
// families; at the call site every kernel assembles to what it was (profiles/gemm_epilogue_refactor.jsonl).
// PTR_FIRST: the 16-bit RESID / PATCH outputs form the output address before the pack (ping-pong and duo kernels) or after it
// (the other two).  The same arithmetic either way; each kernel keeps the statement order it had when it was tuned, because
// the compiler's schedule follows it.
template <int EPI, bool F16, bool PTR_FIRST = false, class ST>
__device__ __forceinline__ void epi_finish_store(f32x4 v, const f32x4& r, int m, int n, void* C, int ldc, const ST& st) {
    [[maybe_unused]] int b = 0, p = 0;   // patch row m = 196 b + p -> token row 197 b + 1 + p
    if constexpr (epi_is_patch(EPI)) {
        b = m / 196;
        p = m - b * 196;
    }
    if constexpr (EPI == BSCLIP_EPI_DGELU_BF16) v *= r;
    else if constexpr (EPI != BSCLIP_EPI_F32) v += r;
    auto out = [&](auto* c) { return c + (size_t)(epi_is_patch(EPI) ? b * 197 + 1 + p : m) * ldc + n; };
    if constexpr (EPI == BSCLIP_EPI_F32 || EPI == BSCLIP_EPI_RESID_F32 || EPI == BSCLIP_EPI_PATCH_F32) {
        st(out(static_cast<float*>(C)), v);
    } else if constexpr (PTR_FIRST && EPI != BSCLIP_EPI_DGELU_BF16) {
        st(out(static_cast<bf16_t*>(C)), f32_to_bf4<F16>(v));
    } else {
        const uint2 o = f32_to_bf4<F16>(v);
        st(out(static_cast<bf16_t*>(C)), o);
    }
}

// gemm_nt_kernel: straight from the accumulator registers.  v already holds acc (+ bias).  No data-dependent branch guards a load.
template <int EPI, bool F16 = false>
__device__ __forceinline__ void epilogue_store(f32x4 v, int m, int n, void* C, int ldc, const EpiArgs& e) {
    if constexpr (EPI == BSCLIP_EPI_BF16) {
        uint2 o;
        o.x = pack_h2<F16>(v[0], v[1]);
        o.y = pack_h2<F16>(v[2], v[3]);
        *reinterpret_cast<uint2*>(static_cast<bf16_t*>(C) + (size_t)m * ldc + n) = o;
    } else if constexpr (EPI == BSCLIP_EPI_GELU_BF16) {
        // the same table-driven GELU as the 256x256 kernel (table read from global memory here: 8 KB, cache-resident), so a
        // row's result does not depend on which tile shape its batch size selects (tests/test_70_configs_gpu.py)
        f32x2 g0, d0, g1, d1;
        gelu_lut2(reinterpret_cast<const char*>(g_gelu_lut), f32x2{v[0], v[1]}, g0, d0);
        gelu_lut2(reinterpret_cast<const char*>(g_gelu_lut), f32x2{v[2], v[3]}, g1, d1);
        const float gl[4] = {g0[0], g0[1], g1[0], g1[1]}, dg[4] = {d0[0], d0[1], d1[0], d1[1]};
        if (e.aux)  // store only: gelu'(pre-activation) as 8-bit codes, all the backward pass needs
            *reinterpret_cast<unsigned*>(e.aux + (size_t)m * e.ld_aux + n) = dg8_pack4(dg[0], dg[1], dg[2], dg[3]);
        uint2 o;
        o.x = pack_h2<F16>(gl[0], gl[1]);
        o.y = pack_h2<F16>(gl[2], gl[3]);
        *reinterpret_cast<uint2*>(static_cast<bf16_t*>(C) + (size_t)m * ldc + n) = o;
    } else if constexpr (EPI == BSCLIP_EPI_DGELU_BF16) {
        // the multiply written per element: as the vector form of epi_finish_store these kernels assemble differently
        const f32x4 z = epi_cook<EPI>(epi_fetch<EPI>(e, m, n));
        uint2 o;
        o.x = pack_h2<F16>(v[0] * z[0], v[1] * z[1]);
        o.y = pack_h2<F16>(v[2] * z[2], v[3] * z[3]);
        *reinterpret_cast<uint2*>(static_cast<bf16_t*>(C) + (size_t)m * ldc + n) = o;
    } else if constexpr (epi_is_patch(EPI)) {
        // one quotient serves the position row and the output row: taken apart into epi_fetch's remainder and epi_finish_store's
        // quotient the division is expanded differently, so the remap is written out here
        const int b = m / 196, p = m - b * 196;
        const f32x4 pos = *reinterpret_cast<const f32x4*>(e.resid + (size_t)(1 + p) * e.ld_resid + n);
        v += pos;
        if constexpr (EPI == BSCLIP_EPI_PATCH_F32)
            *reinterpret_cast<f32x4*>(static_cast<float*>(C) + (size_t)(b * 197 + 1 + p) * ldc + n) = v;
        else
            *reinterpret_cast<uint2*>(static_cast<bf16_t*>(C) + (size_t)(b * 197 + 1 + p) * ldc + n) = f32_to_bf4<F16>(v);
    } else {
        auto plain = [](auto* p, auto w) { *reinterpret_cast<decltype(w)*>(p) = w; };
        const f32x4 r = epi_cook<EPI, F16>(epi_fetch<EPI>(e, m, n));
        if constexpr (epi_is_resid(EPI)) {
            if (e.drop.thr16) v = drop4(e.drop, (unsigned)m * (unsigned)e.n_total + (unsigned)n, v);
        }
        epi_finish_store<EPI, F16>(v, r, m, n, C, ldc, plain);
    }
}
