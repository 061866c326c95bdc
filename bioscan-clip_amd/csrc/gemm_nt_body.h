// The workgroup program of gemm_nt_kernel (gemm.hip), as text: included as the body of gemm_nt_kernel and of
// gemm_nt_batched_kernel, which differ only in where the operand pointers come from.  Expects in scope: the template constants BM, BN,
// WAVES_M, WAVES_N, EPI, HAS_BIAS, F16 and A, lda, B, ldb, C, ldc, M, N, K, tiles_n, e (EpiArgs, a modifiable copy).  It reads
// blockIdx.x / gridDim.x only, so a tile's arithmetic does not depend on which kernel runs it.
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;  // per-wave output tile
    if constexpr (epi_is_resid(EPI)) BSCLIP_DROP_RESOLVE(e.drop);
    constexpr int TM = WTM / 16, TN = WTN / 16;
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES;
    constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int A_PER_WAVE = BM / 8 / NW, B_PER_WAVE = BN / 8 / NW;
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "staging split");
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];

    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_n = wg % tiles_n, tile_m = wg / tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    // ---- staging sources: wave-instruction q covers tile rows [8q, 8q+8); lane -> (row, swizzled chunk) ----
    const bf16_t* a_src[A_PER_WAVE];
    const bf16_t* b_src[B_PER_WAVE];
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
        const int row = (wave + i * NW) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        const int grow = min(m0 + row, M - 1);
        a_src[i] = A + (size_t)grow * lda + c * 8;
    }
#pragma unroll
    for (int i = 0; i < B_PER_WAVE; ++i) {
        const int row = (wave + i * NW) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        const int grow = min(n0 + row, N - 1);
        b_src[i] = B + (size_t)grow * ldb + c * 8;
    }
    auto stage = [&](int buf, int k0) {
        char* sA = smem + buf * STAGE_BYTES;
        char* sB = sA + A_BYTES;
#pragma unroll
        for (int i = 0; i < A_PER_WAVE; ++i) glds16(a_src[i] + k0, sA + (wave + i * NW) * 1024);
#pragma unroll
        for (int i = 0; i < B_PER_WAVE; ++i) glds16(b_src[i] + k0, sB + (wave + i * NW) * 1024);
    };

    // ---- fragment read offsets (bytes) within a tile ----
    const int fr = lane & 15, fq = lane >> 4;
    const int sw = fr >> 1;  // (row>>1)&7 for rows that are 16-aligned + fr
    const int a_off0 = (wm * WTM + fr) * ROW_BYTES + ((fq ^ sw) << 4);        // ks = 0
    const int b_off0 = (wn * WTN + fr) * ROW_BYTES + ((fq ^ sw) << 4);
    // ks = 1 adds chunk 4: (4 + fq) ^ sw == (fq ^ sw) ^ 4  -> byte offset ^ 64

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BK;
    stage(0, 0);
    __syncthreads();  // drains the LDS-DMA (vmcnt(0)) and publishes the tile

    for (int t = 0; t < nk; ++t) {
        const int cur = t & 1;
        if (t + 1 < nk) stage(cur ^ 1, (t + 1) * BK);
        const char* sA = smem + cur * STAGE_BYTES;
        const char* sB = sA + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[TM], bfr[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = *reinterpret_cast<const bf16x8*>(sB + ((b_off0 ^ (ks << 6)) + j * 16 * ROW_BYTES));
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const bf16x8*>(sA + ((a_off0 ^ (ks << 6)) + i * 16 * ROW_BYTES));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = mfma16x16x32<F16>(bfr[j], af[i], acc[i][j]);
        }
        __syncthreads();
    }

    // ---- epilogue: lane holds C[m][n..n+3] with m = ... + (lane&15), n = ... + (lane>>4)*4 ----
    f32x4 bias[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        bias[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (HAS_BIAS) bias[j] = *reinterpret_cast<const f32x4*>(e.bias + n0 + wn * WTN + j * 16 + fq * 4);
    }
    // bias is consumed before the row guards: a loaded register live across a divergent branch makes hipcc wait
    // vmcnt(0) (which also drains the previous row's stores) at the top of every guarded block
    if constexpr (HAS_BIAS) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] += bias[j];
    }
    // Row guards only on the last (partial) M tile: per-row divergent branches make hipcc drain vmcnt(0) -- loads AND
    // the previous row's stores -- at the top of every guarded block.
    auto store_rows = [&](auto guard) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm * WTM + i * 16 + fr;
            if (!decltype(guard)::value || m < M) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn * WTN + j * 16 + fq * 4;
                    epilogue_store<EPI, F16>(acc[i][j], m, n, C, ldc, e);
                }
            }
        }
    };
    if (m0 + BM <= M) store_rows(std::false_type{});
    else store_rows(std::true_type{});
