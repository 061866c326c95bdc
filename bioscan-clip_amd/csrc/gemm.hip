// bf16 MFMA GEMM family for gfx950:  C = epilogue(A[M,K] * B[N,K]^T)
//
// Takes over every torch.nn.Linear (and its dX autograd pass) on the contrastive-training path -- see
// include/bsclip.h for the reference call sites.  Design (MI355X_MICROARCH / cdna_hip_programming guides):
//   * BK = 64 K-tiles staged HBM -> LDS with global_load_lds_dwordx4 (no VGPR round trip), double buffered;
//   * LDS image is lane-linear per wave instruction (8 rows x 128 B); the 16-B chunk index is XOR-swizzled with
//     (row>>1)&7 on the SOURCE address and again on the ds_read_b128 address, which makes every 16-lane
//     ds_read_b128 group hit 16 distinct 16-B slots of the 256-B bank row (conflict-free);
//   * v_mfma_f32_16x16x32_bf16 with the operands swapped (weights as the MFMA "A" side) so each lane ends up
//     holding 4 consecutive output columns of one row -> 8-B (bf16) / 16-B (f32) epilogue stores;
//   * XCD-aware bijective blockIdx remap: the 8 XCDs each walk a contiguous range of tiles, N fastest, so the
//     A row-panel and the (small) weight matrix are re-used out of that XCD's private L2;
//   * epilogues fused in registers: bias, exact GELU (+ saved pre-activation), residual add in f32, GELU'
//     scaling for the backward pass (the forward saves gelu'(pre-activation), so the backward epilogue is one multiply),
//     and the ViT patch-embed row remap + position add.  Bias is loaded once per
//     thread before the stores and every epilogue is branch-free per element (a per-element "if (bias)" makes
//     hipcc wait vmcnt(0) around each load: 32 serial L2 round trips per tile).
//
// Which file holds what (the headers are parts of this one translation unit, included in this order):
//   gemm_epilogue.h  EpiArgs, the GELU table, and the ONE definition of what an epilogue does to a piece of an output row
//                    (second-operand fetch, + resid / * gelu', patch-row remap, pack, store); epilogue_store of gemm_nt_kernel
//   gemm_nt_body.h   the workgroup program of gemm_nt_kernel / gemm_nt_batched_kernel (below), as text
//   gemm_pp.h        gemm_nt_pp_kernel: 256x256 tile, 8 waves = two groups of four that run half a phase apart ("ping-pong"),
//                    fp8 / fp16 operand forms, the two fused InfoNCE epilogues; launch_pp
//   gemm_duo.h       gemm_nt_duo_kernel: 256x128 tile, two workgroups per CU; launch_duo
//   gemm_pers.h      gemm_nt_pers_kernel: the ping-pong kernel as a persistent workgroup that walks tiles; launch_pers
//   gemm_diag.h      -DBSCLIP_DIAG only: the phase-stamp / ablation entry points for tools/gemm_*phases.py, gemm_ablate.py
//   this file        gemm_nt_kernel (generic BMxBN tile, one barrier per K-tile: small / odd shapes, 128x128 and 256x128), tile
//                    selection (pick_tile), the launch ladder, and every product entry point (bf16 / fp16, split-K, InfoNCE,
//                    batched, fp8) with its argument checks
#include <type_traits>

#include "common.h"

namespace {

constexpr int BK = 64;            // K tile (bf16 elements) = 128 B per row
constexpr int ROW_BYTES = BK * 2;  // 128

__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// s_barrier that the compiler schedules nothing across: the K loops of the duo and persistent kernels (the ping-pong kernel's
// PP_BARRIER is this plus its ablation bit)
#define GEMM_BARRIER()                      \
    do {                                    \
        __builtin_amdgcn_sched_barrier(0);  \
        __builtin_amdgcn_s_barrier();       \
        __builtin_amdgcn_sched_barrier(0);  \
    } while (0)

#include "gemm_epilogue.h"

// ---------------------------------------------------------------------------------------------------------------
// generic tile, one barrier per K-tile
// ---------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, bool HAS_BIAS, bool F16 = false>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_nt_kernel(const bf16_t* __restrict__ A, int lda,
                                                                         const bf16_t* __restrict__ B, int ldb,
                                                                         void* __restrict__ C, int ldc, int M, int N,
                                                                         int K, int tiles_n, EpiArgs e) {
#include "gemm_nt_body.h"   // the workgroup program, shared with gemm_nt_batched_kernel
}

// Up to BSCLIP_GEMM_BATCH_MAX products of ONE shape in one launch (the small-N InfoNCE: 4 tiles per product, 6 products): problem
// blockIdx.z takes its operand pointers from the table, passed by value, and runs the same workgroup program -- the same text,
// gemm_nt_body.h, so gemm_nt_kernel itself compiles to what it was.  No bias, bf16 operands.  The RESID epilogue accumulates in
// place: resid is the problem's own C.
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_nt_batched_kernel(bsclip_gemm_batch t, int lda, int ldb, int ldc,
                                                                                 int M, int N, int K, int tiles_n, EpiArgs e) {
    constexpr bool HAS_BIAS = false, F16 = false;
    const bf16_t* __restrict__ A = static_cast<const bf16_t*>(t.A[blockIdx.z]);
    const bf16_t* __restrict__ B = static_cast<const bf16_t*>(t.B[blockIdx.z]);
    void* __restrict__ C = t.C[blockIdx.z];
    if constexpr (epi_is_resid(EPI)) {
        e.resid = static_cast<const float*>(C);
        e.ld_resid = ldc;
    }
#include "gemm_nt_body.h"
}

#include "gemm_pp.h"
#include "gemm_duo.h"
#include "gemm_pers.h"
#undef GEMM_BARRIER

int g_tile_override = 0;
// selection of the persistent kernel, tuned IN THE STEP (profiles/r03_m_pers_selection.log): per-shape microbenchmarks favour the
// duo kernel on the ViT's 768x768 GEMMs and tie on K >= 2304, but with two tower streams sharing the chip the step is fastest
// when every 256x256-tile GEMM with more tiles than CUs is persistent (39.24 -> 38.59 ms on one box)
const int g_pers_max_k = getenv("BSCLIP_PERS_MAX_K") ? atoi(getenv("BSCLIP_PERS_MAX_K")) : 4096;
const int g_pers_min_tiles = getenv("BSCLIP_PERS_MIN_TILES") ? atoi(getenv("BSCLIP_PERS_MIN_TILES")) : 256;
const bool g_duo_off = !(getenv("BSCLIP_GEMM_DUO") && atoi(getenv("BSCLIP_GEMM_DUO")) == 1);   // bsclip_gemm_set_tile(5) still selects it
const bool g_pers_off = getenv("BSCLIP_GEMM_PERSISTENT") && atoi(getenv("BSCLIP_GEMM_PERSISTENT")) == 0;   // A/B switch

// The kernels' argument block from the public one (nullable): operands of the epilogue, the row width, dropout OFF.  Each entry
// point checks what it requires of them itself, and bsclip_gemm_bf16 / bsclip_gemm_fp8 turn dropout on after their checks.
EpiArgs epi_from_public(const bsclip_epi_args* args, int N) {
    EpiArgs e{};
    if (args) {
        e.bias = args->bias;
        e.resid = static_cast<const float*>(args->resid);
        e.ld_resid = args->ld_resid;
        e.aux = static_cast<unsigned char*>(args->aux);
        e.ld_aux = args->ld_aux;
    }
    e.drop = make_drop(0.f, 0);
    e.n_total = N;
    return e;
}

template <int BM, int BN, int WM, int WN, int EPI, bool HB, bool F16>
void launch_cfg(const bf16_t* A, int lda, const bf16_t* B, int ldb, void* C, int ldc, int M, int N, int K,
                const EpiArgs& e, hipStream_t s) {
    const int tiles_m = ceil_div(M, BM), tiles_n = N / BN;
    hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, WM, WN, EPI, HB, F16>), dim3(tiles_m * tiles_n), dim3(WM * WN * 64), 0, s, A,
                       lda, B, ldb, C, ldc, M, N, K, tiles_n, e);
}

// which kernel launch_epi runs for a shape (the switch below): 1 = 128x128, 2 = 256x128, 3 = 256x256 plain, 4 = ping-pong, 5 = duo,
// 8 = persistent.  bsclip_gemm_bf16_batched asks too: it only has the 128x128 form and must agree with the single launch.
template <int EPI, bool F16>
int pick_tile(int M, int N, int K) {
    int tile = g_tile_override;
    if (tile == 0) {
        // 256x256 (8 waves, 1 block/CU) halves L2->LDS traffic per FLOP; fall back when N is not a multiple of
        // 256 or the grid would not fill the 256 CUs.
        // measured on MI355X (profiles/r01_b_gemm_tiles.log): the ping-pong 256x256 kernel wins on every encoder shape
        // once the grid covers the chip; 128x128 (2 workgroups/CU) is the better small-grid choice.
        const long t256 = (long)ceil_div(M, 256) * (N / 256);
        if (N % 256 == 0 && t256 >= 192) tile = 4;
        else tile = 1;
        // the two-workgroups-per-CU kernel (gemm_duo.h) ties the ping-pong kernel on most shapes and wins, per shape, where a tile
        // is short (12 K-tiles) and the grid is a few rounds deep: the ViT's N = K = 768 GEMMs (60 vs 67 us, 76 vs 79 us at
        // M = 50 432; profiles/r03_f_gemm_tiles.log).  Off by default since the end of round 3 (BSCLIP_GEMM_DUO=1): in the step,
        // beside the other tower's persistent kernels, it loses (profiles/r03_m_pers_selection.log).
        if (tile == 4 && N == 768 && K == 768 && t256 >= 500 && EPI != BSCLIP_EPI_GELU_BF16 && !g_duo_off) tile = 5;
        // the persistent form (gemm_pers.h) hides a tile's 2.5-3 us prologue under the previous tile.  Per shape it pays where
        // tiles are short (K <= 832) and ties at 36-48 K-tiles (profiles/r03_i_gemm_pers.log); in the step it pays everywhere a
        // workgroup has more than one tile to walk (g_pers_max_k / g_pers_min_tiles above)
        if (tile == 4 && pers_supported(EPI) && K <= g_pers_max_k && K >= 2 * BK && t256 >= g_pers_min_tiles && !g_pers_off) tile = 8;
    }
    if (F16 && tile == 5) tile = 4;
    if ((tile == 3 || tile == 4 || tile == 6 || tile == 7 || tile == 8) && N % 256 != 0) tile = 2;
    return tile;
}

// F16: fp16 operands (BSCLIP_OPERANDS_FP16).  The same tile selection as bf16, except that the duo kernel (bsclip_gemm_set_tile(5),
// BSCLIP_GEMM_DUO=1) has no fp16 form: the ping-pong kernel takes its shapes.
template <int EPI, bool HB, bool F16>
void launch_epi(const bf16_t* A, int lda, const bf16_t* B, int ldb, void* C, int ldc, int M, int N, int K,
                const EpiArgs& e, hipStream_t s) {
    if (EPI == BSCLIP_EPI_GELU_BF16) ensure_gelu_lut(s);
    const int tile = pick_tile<EPI, F16>(M, N, K);
    switch (tile) {
        case 4: launch_pp<EPI, HB, F16>(A, lda, B, ldb, C, ldc, M, N, K, e, s); break;
        case 5:
            if constexpr (!F16) launch_duo<EPI, HB>(A, lda, B, ldb, C, ldc, M, N, K, e, s);
            break;
        case 8:
            if constexpr (pers_supported(EPI)) {
                if (K >= 2 * BK && (size_t)M * lda * 2 < (1ull << 32) && (size_t)N * ldb * 2 < (1ull << 32)) {
                    launch_pers<EPI, HB, F16>(A, lda, B, ldb, C, ldc, M, N, K, e, s);
                    break;
                }
            }
            launch_pp<EPI, HB, F16>(A, lda, B, ldb, C, ldc, M, N, K, e, s);
            break;
#ifdef BSCLIP_DIAG
        case 6: launch_pp<EPI, HB, F16, 1>(A, lda, B, ldb, C, ldc, M, N, K, e, s); break;  // two-tiles-ahead DMA (comparison)
        case 7: launch_pp<EPI, HB, F16, 2>(A, lda, B, ldb, C, ldc, M, N, K, e, s); break;  // four barriers per K-tile (experimental)
#endif
        case 3: launch_cfg<256, 256, 2, 4, EPI, HB, F16>(A, lda, B, ldb, C, ldc, M, N, K, e, s); break;
        case 2: launch_cfg<256, 128, 4, 2, EPI, HB, F16>(A, lda, B, ldb, C, ldc, M, N, K, e, s); break;
        default: launch_cfg<128, 128, 2, 2, EPI, HB, F16>(A, lda, B, ldb, C, ldc, M, N, K, e, s); break;
    }
}

template <int EPI, int OP>
void launch_f8(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const EpiArgs& e,
               hipStream_t s) {
    if (EPI == BSCLIP_EPI_GELU_FP8) ensure_gelu_lut(s);
    const int tiles_m = ceil_div(M, 256), tiles_n = N / 256;
    hipLaunchKernelGGL((gemm_nt_pp_kernel<EPI, true, false, 0, 0, OP>), dim3(tiles_m * tiles_n), dim3(512), 0, s,
                       static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(B), ldb, C, ldc, M, N, K, tiles_n, e);
}

template <int EPI>
void launch_bias(const bf16_t* A, int lda, const bf16_t* B, int ldb, void* C, int ldc, int M, int N, int K,
                 const EpiArgs& e, hipStream_t s, bool f16) {
    if (f16) {
        if (e.bias) launch_epi<EPI, true, true>(A, lda, B, ldb, C, ldc, M, N, K, e, s);
        else launch_epi<EPI, false, true>(A, lda, B, ldb, C, ldc, M, N, K, e, s);
    } else {
        if (e.bias) launch_epi<EPI, true, false>(A, lda, B, ldb, C, ldc, M, N, K, e, s);
        else launch_epi<EPI, false, false>(A, lda, B, ldb, C, ldc, M, N, K, e, s);
    }
}

}  // namespace

#ifdef BSCLIP_DIAG
#include "gemm_diag.h"
#endif

// Fills the device-side GELU table.  Stream-ordered; the GEMM entry point also does this lazily on its own stream, so a
// single-stream caller never needs it -- callers that launch GEMMs on several streams call it once up front.
extern "C" int bsclip_init_tables(void* stream) {
    launch_gelu_lut(static_cast<hipStream_t>(stream));
    BSCLIP_LAUNCH_CHECK();
    g_lut_ready = true;
    return BSCLIP_OK;
}

extern "C" int bsclip_gemm_set_tile(int tile) {
#ifdef BSCLIP_DIAG
    BSCLIP_REQUIRE(tile >= 0 && tile <= 8, "bsclip_gemm_set_tile: tile %d not in 0..8", tile);
#else
    BSCLIP_REQUIRE((tile >= 0 && tile <= 5) || tile == 8, "bsclip_gemm_set_tile: tile %d not in 0..5, 8", tile);
#endif
    g_tile_override = tile;
    return BSCLIP_OK;
}

extern "C" int bsclip_gemm_set_persistent_grid(int workgroups) {
    BSCLIP_REQUIRE(workgroups >= 0 && workgroups <= 4096, "bsclip_gemm_set_persistent_grid: %d not in 0..4096", workgroups);
    g_pers_grid = workgroups;
    return BSCLIP_OK;
}

extern "C" int bsclip_epi_args_size(void) { return (int)sizeof(bsclip_epi_args); }

extern "C" int bsclip_gemm_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                                int epilogue, const bsclip_epi_args* args, void* stream) {
    BSCLIP_REQUIRE(A && B && C, "bsclip_gemm_bf16: null operand");
    const bool f16 = (epilogue & BSCLIP_OPERANDS_FP16) != 0;   // fp16 operands and 16-bit epilogue values (include/bsclip.h)
    epilogue &= ~BSCLIP_OPERANDS_FP16;
    BSCLIP_REQUIRE(M > 0 && N > 0 && K > 0, "bsclip_gemm_bf16: bad shape M=%d N=%d K=%d", M, N, K);
    BSCLIP_REQUIRE(K % 64 == 0, "bsclip_gemm_bf16: K=%d must be a multiple of 64", K);
    BSCLIP_REQUIRE(N % 128 == 0, "bsclip_gemm_bf16: N=%d must be a multiple of 128", N);
    BSCLIP_REQUIRE(lda >= K && ldb >= K && lda % 8 == 0 && ldb % 8 == 0, "bsclip_gemm_bf16: lda=%d ldb=%d (K=%d)", lda,
                   ldb, K);
    BSCLIP_REQUIRE(ldc >= N && ldc % 4 == 0, "bsclip_gemm_bf16: ldc=%d (N=%d)", ldc, N);
    BSCLIP_REQUIRE(aligned_to(16, A, B, C), "bsclip_gemm_bf16: 16-B alignment");
    BSCLIP_REQUIRE(!args || args->struct_size == sizeof(bsclip_epi_args),
                   "bsclip_gemm_bf16: args->struct_size=%u, this library's bsclip_epi_args is %zu bytes (binding out of date?)",
                   args->struct_size, sizeof(bsclip_epi_args));
    EpiArgs e = epi_from_public(args, N);
    if (args) {
        BSCLIP_REQUIRE(!e.aux || (e.ld_aux >= N && e.ld_aux % 16 == 0 && aligned_to(16, e.aux)),
                       "bsclip_gemm_bf16: aux (8-bit gelu' band) needs ld_aux >= N, ld_aux %% 16 == 0, 16-B alignment (ld_aux=%d)",
                       args->ld_aux);
        BSCLIP_REQUIRE(args->dropout_p >= 0.f && args->dropout_p < 1.f, "bsclip_gemm_bf16: dropout_p=%f", args->dropout_p);
        BSCLIP_REQUIRE(args->dropout_p == 0.f || epilogue == BSCLIP_EPI_RESID_F32 || epilogue == BSCLIP_EPI_RESID_BF16,
                       "bsclip_gemm_bf16: dropout is only defined for BSCLIP_EPI_RESID_F32 / _BF16");
        e.drop = make_drop(args->dropout_p, args->dropout_seed);
    }
    BSCLIP_REQUIRE(!e.bias || aligned_to(16, e.bias), "bsclip_gemm_bf16: bias must be 16-B aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf16_t* a = static_cast<const bf16_t*>(A);
    const bf16_t* b = static_cast<const bf16_t*>(B);
    switch (epilogue) {
        case BSCLIP_EPI_BF16: launch_bias<BSCLIP_EPI_BF16>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16); break;
        case BSCLIP_EPI_F32: launch_bias<BSCLIP_EPI_F32>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16); break;
        case BSCLIP_EPI_GELU_BF16: launch_bias<BSCLIP_EPI_GELU_BF16>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16); break;
        case BSCLIP_EPI_RESID_F32:
            BSCLIP_REQUIRE(e.resid && e.ld_resid >= N, "bsclip_gemm_bf16: RESID needs resid/ld_resid");
            launch_bias<BSCLIP_EPI_RESID_F32>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16);
            break;
        case BSCLIP_EPI_DGELU_BF16:
            BSCLIP_REQUIRE(e.aux && e.ld_aux >= N, "bsclip_gemm_bf16: DGELU needs aux/ld_aux");
            launch_bias<BSCLIP_EPI_DGELU_BF16>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16);
            break;
        case BSCLIP_EPI_PATCH_F32:
            BSCLIP_REQUIRE(e.resid && e.ld_resid >= N && M % 196 == 0, "bsclip_gemm_bf16: PATCH needs pos, M%%196==0");
            launch_bias<BSCLIP_EPI_PATCH_F32>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16);
            break;
        case BSCLIP_EPI_RESID_BF16:
            BSCLIP_REQUIRE(e.resid && e.ld_resid >= N && e.ld_resid % 4 == 0 && aligned_to(8, e.resid),
                           "bsclip_gemm_bf16: RESID_BF16 needs resid (bf16, 8-byte aligned rows) / ld_resid");
            launch_bias<BSCLIP_EPI_RESID_BF16>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16);
            break;
        case BSCLIP_EPI_PATCH_BF16:
            BSCLIP_REQUIRE(e.resid && e.ld_resid >= N && M % 196 == 0, "bsclip_gemm_bf16: PATCH needs pos, M%%196==0");
            launch_bias<BSCLIP_EPI_PATCH_BF16>(a, lda, b, ldb, C, ldc, M, N, K, e, s, f16);
            break;
        default: BSCLIP_REQUIRE(false, "bsclip_gemm_bf16: unknown epilogue %d", epilogue);
    }
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// split-K product with f32 accumulation into C: the weight-gradient GEMMs of full fine-tuning
// ---------------------------------------------------------------------------------------------------------------
// dW[N_out, K_in] = dY^T X has a small output (9 .. 36 tiles of 256 x 256) and a reduction over all tokens (50 432 for the ViT
// at batch 256): one workgroup per output tile would use 4 .. 14 % of the chip.  The reduction is cut into `splits` equal
// column ranges, every (tile, range) pair is one workgroup of the ping-pong kernel writing an f32 slab, and the slabs are
// summed in the fixed order z = 0 .. splits - 1 and added to C (no atomics: the result does not depend on the schedule).
__global__ __launch_bounds__(256) void splitk_reduce_add_kernel(const float* __restrict__ partial, int splits, int M, int N,
                                                                float* __restrict__ C, int ldc) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const size_t total = (size_t)M * N;
    if (i >= total) return;
    f32x4 acc = *reinterpret_cast<const f32x4*>(partial + i);
    for (int z = 1; z < splits; ++z) acc += *reinterpret_cast<const f32x4*>(partial + (size_t)z * total + i);
    const size_t m = i / N, n = i - m * N;
    f32x4* dst = reinterpret_cast<f32x4*>(C + m * ldc + n);
    *dst = *dst + acc;
}

extern "C" int bsclip_gemm_splitk_f32(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                                      int splits, float* partial, void* stream) {
    BSCLIP_REQUIRE(A && B && C && partial, "bsclip_gemm_splitk_f32: null operand");
    BSCLIP_REQUIRE(M > 0 && N > 0 && N % 256 == 0 && splits >= 1 && K > 0 && K % (64 * splits) == 0,
                   "bsclip_gemm_splitk_f32: M=%d N=%d (multiple of 256) K=%d (multiple of 64 * splits=%d)", M, N, K, splits);
    BSCLIP_REQUIRE(lda >= K && ldb >= K && lda % 8 == 0 && ldb % 8 == 0 && ldc >= N && ldc % 4 == 0,
                   "bsclip_gemm_splitk_f32: lda=%d ldb=%d ldc=%d", lda, ldb, ldc);
    BSCLIP_REQUIRE(aligned_to(16, A, B, C, partial), "bsclip_gemm_splitk_f32: 16-B alignment");
    EpiArgs e = epi_from_public(nullptr, N);
    e.split_stride = (long)M * N;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tiles_m = ceil_div(M, 256), tiles_n = N / 256;
    hipLaunchKernelGGL((gemm_nt_pp_kernel<BSCLIP_EPI_F32, false>), dim3(tiles_m * tiles_n, splits), dim3(512), 0, s,
                       static_cast<const bf16_t*>(A), lda, static_cast<const bf16_t*>(B), ldb, partial, N, M, N, K / splits, tiles_n, e);
    hipLaunchKernelGGL(splitk_reduce_add_kernel, dim3(ceil_div((int)((long)M * N / 4), 256)), dim3(256), 0, s, partial, splits, M, N, C, ldc);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fused InfoNCE products (called by loss.hip; not part of the public ABI)
// ---------------------------------------------------------------------------------------------------------------
// mode 0: pass 1 -- part[M, N/256, 4] from cosines A[M,K] . B[N,K]^T;  mode 1: pass 2 -- C = dL/dG in split form [M, 3*Np].
// scale_dev != nullptr (trainable temperature): the logit scale is scale_dev[1], read by the kernel; `logit_scale` is unused and
// `coef` holds the divisor P N.  Pass 1 then also fills part[..][3].
int bsclip_gemm_infonce(int mode, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                        const int64_t* labels, const float* cnt, const float* lse_row, const float* lse_col, float* part,
                        float logit_scale, float coef, int n_valid, int row_base, const float* scale_dev, void* stream) {
    BSCLIP_REQUIRE(A && B && labels && M > 0 && N % 256 == 0 && K % 64 == 0, "bsclip_gemm_infonce: bad shape M=%d N=%d K=%d", M, N, K);
    EpiArgs e = epi_from_public(nullptr, N);
    e.labels = labels;
    e.cnt = cnt;
    e.lse_row = lse_row;
    e.lse_col = lse_col;
    e.part = part;
    e.logit_scale = logit_scale;
    e.coef = coef;
    e.n_valid = n_valid;
    e.row_base = row_base;
    e.scale_dev = scale_dev;
    const int tiles_m = ceil_div(M, 256), tiles_n = N / 256;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf16_t* a = static_cast<const bf16_t*>(A);
    const bf16_t* b = static_cast<const bf16_t*>(B);
    if (mode == 0) {
        BSCLIP_REQUIRE(part, "bsclip_gemm_infonce: part is null");
        if (scale_dev)
            hipLaunchKernelGGL((gemm_nt_pp_kernel<EPI_LSE_PART_TS, false>), dim3(tiles_m * tiles_n), dim3(512), 0, s, a, lda, b, ldb,
                               C, ldc, M, N, K, tiles_n, e);
        else
            hipLaunchKernelGGL((gemm_nt_pp_kernel<EPI_LSE_PART, false>), dim3(tiles_m * tiles_n), dim3(512), 0, s, a, lda, b, ldb, C,
                               ldc, M, N, K, tiles_n, e);
    } else {
        BSCLIP_REQUIRE(C && cnt && lse_row && lse_col && ldc % 3 == 0, "bsclip_gemm_infonce: pass 2 operands");
        if (scale_dev)
            hipLaunchKernelGGL((gemm_nt_pp_kernel<EPI_LOSS_W_TS, false>), dim3(tiles_m * tiles_n), dim3(512), 0, s, a, lda, b, ldb, C,
                               ldc, M, N, K, tiles_n, e);
        else
            hipLaunchKernelGGL((gemm_nt_pp_kernel<EPI_LOSS_W, false>), dim3(tiles_m * tiles_n), dim3(512), 0, s, a, lda, b, ldb, C,
                               ldc, M, N, K, tiles_n, e);
    }
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// several small products of one shape in one launch (called by loss.hip; not part of the public ABI)
// ---------------------------------------------------------------------------------------------------------------
// true when bsclip_gemm_bf16 runs this shape on the 128x128 tile -- the only form the batched launch has.  The caller falls back
// to one bsclip_gemm_bf16 per product otherwise (bsclip_gemm_set_tile), so both ways always run the same workgroup program.
bool bsclip_gemm_batched_ok(int M, int N, int K, int epilogue) {
    if (M <= 0 || N <= 0 || N % 128 != 0 || K <= 0 || K % 64 != 0) return false;
    if (epilogue == BSCLIP_EPI_F32) return pick_tile<BSCLIP_EPI_F32, false>(M, N, K) == 1;
    if (epilogue == BSCLIP_EPI_RESID_F32) return pick_tile<BSCLIP_EPI_RESID_F32, false>(M, N, K) == 1;
    return false;
}

// C_i = A_i[M,K] . B_i[N,K]^T (BSCLIP_EPI_F32) or C_i += A_i . B_i^T (BSCLIP_EPI_RESID_F32, in place), i < nb
int bsclip_gemm_bf16_batched(const bsclip_gemm_batch& t, int nb, int lda, int ldb, int ldc, int M, int N, int K, int epilogue,
                             void* stream) {
    BSCLIP_REQUIRE(nb >= 1 && nb <= BSCLIP_GEMM_BATCH_MAX, "bsclip_gemm_bf16_batched: nb=%d", nb);
    BSCLIP_REQUIRE(bsclip_gemm_batched_ok(M, N, K, epilogue), "bsclip_gemm_bf16_batched: M=%d N=%d K=%d epilogue=%d is not a 128x128 shape",
                   M, N, K, epilogue);
    BSCLIP_REQUIRE(lda >= K && ldb >= K && lda % 8 == 0 && ldb % 8 == 0 && ldc >= N && ldc % 4 == 0,
                   "bsclip_gemm_bf16_batched: lda=%d ldb=%d ldc=%d", lda, ldb, ldc);
    for (int i = 0; i < nb; ++i)
        BSCLIP_REQUIRE(t.A[i] && t.B[i] && t.C[i] && aligned_to(16, t.A[i], t.B[i], t.C[i]),
                       "bsclip_gemm_bf16_batched: operand %d null or not 16-B aligned", i);
    const EpiArgs e = epi_from_public(nullptr, N);
    const int tiles_m = ceil_div(M, 128), tiles_n = N / 128;
    const dim3 grid(tiles_m * tiles_n, 1, nb);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (epilogue == BSCLIP_EPI_F32)
        hipLaunchKernelGGL((gemm_nt_batched_kernel<128, 128, 2, 2, BSCLIP_EPI_F32>), grid, dim3(256), 0, s, t, lda, ldb, ldc, M, N, K,
                           tiles_n, e);
    else
        hipLaunchKernelGGL((gemm_nt_batched_kernel<128, 128, 2, 2, BSCLIP_EPI_RESID_F32>), grid, dim3(256), 0, s, t, lda, ldb, ldc, M,
                           N, K, tiles_n, e);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fp8 entry points (BASELINE configs[4])
// ---------------------------------------------------------------------------------------------------------------
extern "C" int bsclip_gemm_fp8(const void* A8, int lda, const void* B8, int ldb, void* C, int ldc, int M, int N, int K,
                               int epilogue, const bsclip_epi_args* args, const bsclip_fp8_args* f8, void* stream) {
    BSCLIP_REQUIRE(A8 && B8 && C && args && f8, "bsclip_gemm_fp8: null pointer");
    BSCLIP_REQUIRE(args->struct_size == sizeof(bsclip_epi_args) && f8->struct_size == sizeof(bsclip_fp8_args),
                   "bsclip_gemm_fp8: struct_size mismatch (epi %u/%zu, fp8 %u/%zu)", args->struct_size,
                   sizeof(bsclip_epi_args), f8->struct_size, sizeof(bsclip_fp8_args));
    BSCLIP_REQUIRE(M > 0 && N > 0 && K > 0 && K % 128 == 0 && N % 256 == 0, "bsclip_gemm_fp8: M=%d N=%d K=%d (K %% 128, N %% 256)",
                   M, N, K);
    BSCLIP_REQUIRE(lda >= K && ldb >= K && lda % 16 == 0 && ldb % 16 == 0, "bsclip_gemm_fp8: lda=%d ldb=%d (K=%d)", lda, ldb, K);
    BSCLIP_REQUIRE(ldc >= N && ldc % 4 == 0 && (epilogue != BSCLIP_EPI_GELU_FP8 || ldc % 16 == 0), "bsclip_gemm_fp8: ldc=%d", ldc);
    BSCLIP_REQUIRE(aligned_to(16, A8, B8, C), "bsclip_gemm_fp8: 16-B alignment");
    BSCLIP_REQUIRE(args->bias && f8->alpha && aligned_to(16, args->bias, f8->alpha),
                   "bsclip_gemm_fp8: bias and alpha are required, 16-B aligned");
    BSCLIP_REQUIRE((f8->a_aug == nullptr) == (f8->b_aug == nullptr), "bsclip_gemm_fp8: a_aug and b_aug go together");
    BSCLIP_REQUIRE(!f8->a_aug || (f8->ld_a_aug >= 64 && f8->ld_b_aug >= 64 && f8->ld_a_aug % 8 == 0 && f8->ld_b_aug % 8 == 0 &&
                                  aligned_to(16, f8->a_aug, f8->b_aug)),
                   "bsclip_gemm_fp8: K-augmentation block needs ld >= 64, ld %% 8 == 0, 16-B alignment");
    BSCLIP_REQUIRE(f8->form == 1 || f8->form == 2, "bsclip_gemm_fp8: form %d (1 or 2)", f8->form);
    EpiArgs e = epi_from_public(args, N);
    BSCLIP_REQUIRE(!e.aux || (e.ld_aux >= N && e.ld_aux % 16 == 0 && aligned_to(16, e.aux)), "bsclip_gemm_fp8: aux band");
    BSCLIP_REQUIRE(args->dropout_p >= 0.f && args->dropout_p < 1.f && (args->dropout_p == 0.f || epilogue == BSCLIP_EPI_RESID_F32),
                   "bsclip_gemm_fp8: dropout_p=%f", args->dropout_p);
    e.drop = make_drop(args->dropout_p, args->dropout_seed);
    e.alpha = f8->alpha;
    e.a_aug = static_cast<const bf16_t*>(f8->a_aug);
    e.b_aug = static_cast<const bf16_t*>(f8->b_aug);
    e.ld_a_aug = f8->ld_a_aug;
    e.ld_b_aug = f8->ld_b_aug;
    hipStream_t s = static_cast<hipStream_t>(stream);
    BSCLIP_REQUIRE(epilogue != BSCLIP_EPI_RESID_F32 || (e.resid && e.ld_resid >= N), "bsclip_gemm_fp8: RESID needs resid/ld_resid");
    const bool available = pick_int<BSCLIP_EPI_BF16, BSCLIP_EPI_F32, BSCLIP_EPI_GELU_FP8, BSCLIP_EPI_RESID_F32>(epilogue, [&](auto epi) {
        pick_int<1, 2>(f8->form, [&](auto form) {
            launch_f8<decltype(epi)::value, decltype(form)::value>(A8, lda, B8, ldb, C, ldc, M, N, K, e, s);
        });
    });
    BSCLIP_REQUIRE(available, "bsclip_gemm_fp8: epilogue %d not available with fp8 operands", epilogue);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

namespace {
// one wave per row: amax -> scale = amax / 448, then e4m3 codes of src / scale
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const float* __restrict__ src, int R, int C,
                                                                unsigned char* __restrict__ dst, int ld, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (row >= R) return;
    const float* p = src + (size_t)row * C;
    float m = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    m = wave_max(m);
    const float sc = m > 0.f ? m * (1.0f / 448.0f) : 1.0f;
    const float inv = 1.0f / sc;
    if (lane == 0) scale[row] = sc;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
        *reinterpret_cast<unsigned*>(dst + (size_t)row * ld + c) = pack_fp8x4(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv);
    }
}

__global__ void lora_baug_set_kernel(bf16_t* __restrict__ b_aug, int ld, int H, const float* __restrict__ bq,
                                     const float* __restrict__ bv, const float* __restrict__ alpha) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over H * 4
    if (i >= H * 4) return;
    const int n = i >> 2, r = i & 3;
    b_aug[(size_t)n * ld + r] = f2bf(bq[i] / alpha[n]);
    b_aug[(size_t)(2 * H + n) * ld + 4 + r] = f2bf(bv[i] / alpha[2 * H + n]);
}
}  // namespace

extern "C" int bsclip_quantize_rows_fp8(const float* src, int R, int C, void* dst, int ld_dst, float* scale, void* stream) {
    BSCLIP_REQUIRE(src && dst && scale && R > 0 && C > 0 && C % 4 == 0 && ld_dst >= C && ld_dst % 4 == 0,
                   "bsclip_quantize_rows_fp8: R=%d C=%d ld_dst=%d", R, C, ld_dst);
    BSCLIP_REQUIRE(aligned_to(16, src, dst), "bsclip_quantize_rows_fp8: 16-B alignment");
    hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), src, R, C,
                       static_cast<unsigned char*>(dst), ld_dst, scale);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_lora_baug_set(void* b_aug, int ld_b, int H, const float* lora_bq, const float* lora_bv,
                                    const float* alpha, void* stream) {
    BSCLIP_REQUIRE(b_aug && lora_bq && lora_bv && alpha && H > 0 && ld_b >= 8, "bsclip_lora_baug_set: bad args");
    hipLaunchKernelGGL(lora_baug_set_kernel, dim3(ceil_div(H * 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<bf16_t*>(b_aug), ld_b, H, lora_bq, lora_bv, alpha);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}
