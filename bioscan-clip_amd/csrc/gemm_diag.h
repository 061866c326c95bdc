// Entry points of the diagnostic library (-DBSCLIP_DIAG, `make diag`): the 256-wide GEMM kernels with per-workgroup phase stamps,
// and the K-loop ablation mask of the ping-pong kernel.  Included by gemm.hip after its anonymous namespace; on no product path.

static int g_diag_ablate = 0;  // tools/gemm_ablate.py: which parts of the K loop the diagnostic EPI_BF16 build leaves out
// HAS_BIAS of the diagnostic build of each epilogue
constexpr bool diag_has_bias(int epi) { return epi == BSCLIP_EPI_GELU_BF16 || epi == BSCLIP_EPI_RESID_F32 || epi == BSCLIP_EPI_RESID_BF16; }

// Diagnostic: the ping-pong kernel with four phase stamps per workgroup and wave group (start, prologue done, K loop
// done, end) written to diag[grid*16] (8 per wave group: start, prologue, K loop, end, 4 epilogue sections) (100 MHz ticks).  Used by tools/gemm_phases.py; not on any product path.
extern "C" int bsclip_gemm_diag(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                                int epilogue, const bsclip_epi_args* args, unsigned long long* diag, void* stream) {
    BSCLIP_REQUIRE(A && B && C && diag && args, "bsclip_gemm_diag: null pointer");
    BSCLIP_REQUIRE(K % 64 == 0 && N % 256 == 0, "bsclip_gemm_diag: K %% 64, N %% 256");
    EpiArgs e = epi_from_public(args, N);
    e.diag = diag;
    const int tiles_m = ceil_div(M, 256), tiles_n = N / 256;
    const dim3 grid(tiles_m * tiles_n), block(512);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf16_t* a = static_cast<const bf16_t*>(A);
    const bf16_t* b = static_cast<const bf16_t*>(B);
    auto launch = [&](auto epi, auto abl) {
        constexpr int EPI = decltype(epi)::value;
        hipLaunchKernelGGL((gemm_nt_pp_kernel<EPI, diag_has_bias(EPI), true, decltype(abl)::value>), grid, block, 0, s, a, lda, b, ldb, C,
                           ldc, M, N, K, tiles_n, e);
    };
    if (epilogue == BSCLIP_EPI_BF16) {   // the only epilogue with ablated builds
        const bool built = pick_int<0, 1, 2, 4, 8, 6, 3, 5, 9>(
            g_diag_ablate, [&](auto abl) { launch(std::integral_constant<int, BSCLIP_EPI_BF16>{}, abl); });
        BSCLIP_REQUIRE(built, "bsclip_gemm_diag: ablation mask %d not instantiated", g_diag_ablate);
    } else {
        const bool built = pick_int<BSCLIP_EPI_GELU_BF16, BSCLIP_EPI_RESID_F32, BSCLIP_EPI_DGELU_BF16>(
            epilogue, [&](auto epi) { launch(epi, std::integral_constant<int, 0>{}); });
        BSCLIP_REQUIRE(built, "bsclip_gemm_diag: epilogue %d has no diagnostic build", epilogue);
    }
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// The duo kernel with per-workgroup stamps: diag[grid * 8] = {start, tile 0 landed, K loop done, end, HW_ID, XCC_ID, -, -}.
// tools/gemm_duo_phases.py reads co-residency (two workgroups with overlapping lifetimes on one CU) and section times from it.
extern "C" int bsclip_gemm_duo_diag(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                                    int epilogue, const bsclip_epi_args* args, unsigned long long* diag, void* stream) {
    BSCLIP_REQUIRE(A && B && C && diag && args, "bsclip_gemm_duo_diag: null pointer");
    BSCLIP_REQUIRE(K % 64 == 0 && N % 128 == 0, "bsclip_gemm_duo_diag: K %% 64, N %% 128");
    EpiArgs e = epi_from_public(args, N);
    e.diag = diag;
    const int tiles_m = ceil_div(M, 256), tiles_n = N / 128;
    const dim3 grid(tiles_m * tiles_n), block(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf16_t* a = static_cast<const bf16_t*>(A);
    const bf16_t* b = static_cast<const bf16_t*>(B);
    const bool built = pick_int<BSCLIP_EPI_BF16, BSCLIP_EPI_GELU_BF16, BSCLIP_EPI_RESID_F32, BSCLIP_EPI_DGELU_BF16>(epilogue, [&](auto epi) {
        constexpr int EPI = decltype(epi)::value;
        hipLaunchKernelGGL((gemm_nt_duo_kernel<EPI, diag_has_bias(EPI), true>), grid, block, 0, s, a, lda, b, ldb, C, ldc, M, N, K, tiles_n, e);
    });
    BSCLIP_REQUIRE(built, "bsclip_gemm_duo_diag: epilogue %d has no diagnostic build", epilogue);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

// The persistent kernel with per-workgroup stamps, diag[grid * 32] (layout: gemm_pers.h); tools/gemm_pers_phases.py.
extern "C" int bsclip_gemm_pers_diag(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                                     int epilogue, const bsclip_epi_args* args, unsigned long long* diag, int workgroups,
                                     void* stream) {
    BSCLIP_REQUIRE(A && B && C && diag && args, "bsclip_gemm_pers_diag: null pointer");
    BSCLIP_REQUIRE(K % 64 == 0 && K >= 128 && N % 256 == 0 && workgroups > 0, "bsclip_gemm_pers_diag: K %% 64, K >= 128, N %% 256");
    EpiArgs e = epi_from_public(args, N);
    e.diag = diag;
    const int tiles_m = ceil_div(M, 256), tiles_n = N / 256, nt = tiles_m * tiles_n;
    e.pers_gw = tiles_n | (getenv("BSCLIP_PERS_ABL") && atoi(getenv("BSCLIP_PERS_ABL")) == 1 ? 0x40000000 : 0);
    const dim3 grid(nt < workgroups ? nt : workgroups), block(512);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bf16_t* a = static_cast<const bf16_t*>(A);
    const bf16_t* b = static_cast<const bf16_t*>(B);
    const bool built = pick_int<BSCLIP_EPI_BF16, BSCLIP_EPI_GELU_BF16, BSCLIP_EPI_RESID_F32, BSCLIP_EPI_RESID_BF16, BSCLIP_EPI_DGELU_BF16>(
        epilogue, [&](auto epi) {
            constexpr int EPI = decltype(epi)::value;
            hipLaunchKernelGGL((gemm_nt_pers_kernel<EPI, diag_has_bias(EPI), true>), grid, block, 0, s, a, lda, b, ldb, C, ldc, M, N, K,
                               tiles_n, nt, e);
        });
    BSCLIP_REQUIRE(built, "bsclip_gemm_pers_diag: epilogue %d has no diagnostic build", epilogue);
    BSCLIP_LAUNCH_CHECK();
    return BSCLIP_OK;
}

extern "C" int bsclip_gemm_diag_ablate(int mask) {
    BSCLIP_REQUIRE(mask >= 0 && mask < 16, "bsclip_gemm_diag_ablate: mask %d", mask);
    g_diag_ablate = mask;
    return BSCLIP_OK;
}
