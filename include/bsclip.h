/* libbsclip_hip.so -- C ABI of the MI355X (gfx950) BIOSCAN-CLIP contrastive-training-step kernels.
 *
 * The reference (bioscan-ml/bioscan-clip) has no FFI: its boundary for this path is the Python surface of
 * bioscanclip.model.* (SURVEY.md 8b).  Every arithmetic op that surface performs through torch/cuDNN/cuBLAS is
 * replaced by one entry point below; the comment on each names the reference site (file:line under
 * /root/reference) whose arithmetic it takes over.  bioscan-clip_amd/bioscanclip/hip/lib.py binds these with
 * ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory unless named host_*.
 *   - bf16 tensors are raw uint16 bit patterns; "f32" = float; ids/labels are int64.
 *   - row-major; ld* = leading dimension in ELEMENTS.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  No entry point allocates,
 *     synchronises or touches the host; all are capturable into a hipGraph.
 *   - return 0 on success, <0 on error; bsclip_last_error() describes the last failure of the calling thread.
 */
#ifndef BSCLIP_H
#define BSCLIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BSCLIP_OK 0
#define BSCLIP_ERR_INVALID (-1)
#define BSCLIP_ERR_LAUNCH (-2)

#define BSCLIP_LORA_COLS 8 /* r=4 for Q plus r=4 for V */
#define BSCLIP_KPAD 64     /* K-augmentation block appended to LN outputs: [t_q(4) t_v(4) 0...] */

const char* bsclip_last_error(void);
int bsclip_abi_version(void);

/* Clock counters sampled when `stream` reaches this node: for XCD x (HW_REG_XCC_ID, 0..15) out32[2x] = its shader-clock counter
 * (s_memtime), out32[2x + 1] = the 100 MHz real-time counter (s_memrealtime); entries of absent XCDs stay untouched (zero them
 * first).  Two probes around a region give the clock the chip actually ran at in it, per XCD: delta(s_memtime) /
 * delta(s_memrealtime) x 100 MHz.  bench.py reports the median, because the dense-MFMA peak a roofline is priced against
 * assumes the 2.4 GHz peak engine clock. */
int bsclip_clock_probe(unsigned long long* out32_dev, void* stream);
/* Dropout step word (hipGraph support).  Kernel arguments are frozen when a launch is captured into a graph, so a seed passed
 * by value would repeat its mask on every replay.  After bsclip_set_dropout_step(ptr) every dropout-carrying launch made BY
 * THE CALLING THREAD adds (*ptr * 0x9E3779B9) to its seed when the kernel runs (NULL: seeds are used as passed).  The word
 * is advanced once per training step with bsclip_counter_add (itself a capturable launch); forward and backward of a step read
 * the same value, so regenerated masks match. */
int bsclip_set_dropout_step(const uint32_t* step_dev);
int bsclip_counter_add(uint32_t* counter_dev, uint32_t inc, void* stream);
/* *counter_dev += the number of Inf / NaN elements among the n contiguous f32 (is_bf16 = 0) or bf16 (1) values at x.  The check behind
 * BSCLIP_DETECT_ANOMALY=1, this build's counterpart of torch.autograd.set_detect_anomaly(True) in the reference loop
 * (train_epoch.py:12): the engines probe their outputs, gradients and per-layer activations and name where non-finite values
 * first appear. */
int bsclip_count_nonfinite(const void* x, int64_t n, int is_bf16, uint32_t* counter_dev, void* stream);

/* ---- GEMM family: C = epilogue(A[M,K] * B[N,K]^T), bf16 operands, f32 accumulate (MFMA 16x16x32) -------------
 * Replaces every torch.nn.Linear on the path: timm Attention.qkv/proj, Mlp.fc1/fc2 (via
 * bioscanclip/model/image_encoder.py:108-109), HF BertSelfAttention q/k/v, BertSelfOutput.dense,
 * BertIntermediate.dense, BertOutput.dense, cls.predictions.{transform.dense,decoder}
 * (bioscanclip/model/dna_encoder.py:105), LoRA_bert.proj (language_encoder.py:89) and their autograd dX passes.
 * The LoRA side branch (image_encoder.py:42-48, dna_encoder.py:47-49) rides in the K dimension: A carries
 * BSCLIP_KPAD extra columns holding t = x A_lora^T and B carries the matching LoRA-B columns.
 * Requirements: K % 64 == 0, N % 128 == 0, lda/ldb % 8 == 0, 16-byte aligned bases. M is arbitrary. */
enum bsclip_epilogue {
    BSCLIP_EPI_BF16 = 0,       /* C bf16 = acc + bias                                               */
    BSCLIP_EPI_F32 = 1,        /* C f32  = acc + bias                                               */
    BSCLIP_EPI_GELU_BF16 = 2,  /* C bf16 = gelu(acc + bias); aux (uint8 codes, optional) = gelu'(acc + bias) */
    BSCLIP_EPI_RESID_F32 = 3,  /* C f32  = acc + bias + resid                                       */
    BSCLIP_EPI_DGELU_BF16 = 4, /* C bf16 = acc * aux          (aux = gelu' codes saved by the forward) */
    BSCLIP_EPI_PATCH_F32 = 5,  /* C f32 row (b*197+1+p) = acc + bias + pos[1+p], input row b*196+p  */
    BSCLIP_EPI_GELU_FP8 = 6,   /* bsclip_gemm_fp8 only: C fp8 e4m3 = gelu(..) (the next GEMM's operand); aux as GELU_BF16 */
    /* the residual stream stored as bf16 (the sum is formed in f32 and rounded once): 4 instead of 8 bytes per element moved */
    BSCLIP_EPI_RESID_BF16 = 7, /* C bf16 = acc + bias + resid, resid bf16 [M, ld_resid] (+ dropout as RESID_F32)  */
    BSCLIP_EPI_PATCH_BF16 = 8  /* as PATCH_F32 with a bf16 C (pos_embed stays f32)                         */
};
/* fp16 operands: bsclip_gemm_bf16 with (epilogue | BSCLIP_OPERANDS_FP16) takes A and B as IEEE fp16 (v_mfma_f32_16x16x32_f16,
 * the bf16 form's rate) and every 16-bit value of the epilogue -- the C of the *_BF16 epilogues, RESID_BF16's resid -- is fp16 as
 * well; f32 values and the 8-bit gelu' codes are unchanged.  Conversions round to nearest even, keep subnormals and overflow to
 * +-inf.  Same requirements as the bf16 form; the LoRA branch rides in K as there.  Library releases before this flag reject it
 * (unknown epilogue). */
#define BSCLIP_OPERANDS_FP16 0x100
/* The forward's other 16-bit entry points take the same flag or-ed into one integer argument (inference only: fp16 with dropout, keep
 * bits, the split-operand or the fp8 outputs is rejected, as are unknown bits; the low byte keeps the argument's own value):
 *   bsclip_attn_fwd        q_rows     qkv, ctx fp16; QK^T and PV on v_mfma_f32_32x32x16_f16, P rounded to fp16; lse f32
 *   bsclip_layernorm_fwd   x_bf16     a 16-bit x is fp16; y_bf16 and its LoRA t block fp16 (y_f32, stats unchanged)
 *   bsclip_layernorm_fwd_fp8  x_bf16  rejects the flag (no fp8 output form)
 *   bsclip_im2col_patch16  split      fp16 columns; split rows [hi | lo | hi] with lo = fp16(x - hi)
 *   bsclip_vit_cls_rows    x_bf16     the cls rows of an fp16 residual stream (x_bf16 must be set)
 *   bsclip_waug_set_lora_layers  layers  fp16 LoRA-B columns (the layer count must then be < 256)
 *   bsclip_count_nonfinite is_bf16    1 | BSCLIP_OPERANDS_FP16: the 16-bit elements are fp16
 * and bsclip_cast_f32_f16 is the fp16 form of bsclip_cast_f32_bf16 (its only integer argument is the 64-bit count).
 * The backward of the LoRA ViT on fp16 operands (training; no dropout anywhere, so the flag is rejected together with dropout or keep
 * bits) carries the same flag:
 *   bsclip_attn_bwd        q_rows     qkv, dctx, dqkv fp16; S, dP, dQ, dK, dV on v_mfma_f32_32x32x16_f16, P and dS rounded to fp16;
 *                                     lse, delta, softmax f32.  S = 197 only.
 *   bsclip_attn_bwd_lora   q_rows     the same, t_aug fp16; the dt / dB partials stay f32 up to accumulation order (B enters as hi + lo
 *                                     fp16 parts of 2^8 B, the 2^8 is taken off the f32 dt sums)
 *   bsclip_layernorm_bwd   x_bf16     x, g_resid / dx_f32 (resid_flags bits 0 / 1 required when given), g_gemm and dx_bf16 fp16;
 *                                     dx_bf16 = RNE of its f32 value.  H = 768, 16-bit x, resid_flags bits 2-4 rejected.
 *   bsclip_lora_grad_heads_f16  operands  BSCLIP_OPERANDS_FP16 | s (s <= 64 in the low byte, the flag is required): h fp16, the
 *                                     partials and dt in 2^s units; dA / dBq / dBv += 2^-s x the sums (exact)
 * Gradient scale of that backward: one static power of two 2^s per tower, put on where the head's f32 dL/dz becomes the fp16 dout
 * (bsclip_cast_f32_f16_scaled) and taken off, exactly, before each trainable gradient is added (bsclip_lora_grad_heads_f16,
 * bsclip_add_scaled_f32 for the head's dW); the bias gradient is summed from the unscaled f32 dL/dz. */
typedef struct bsclip_epi_args {
    uint32_t struct_size; /* = sizeof(bsclip_epi_args) = bsclip_epi_args_size(); a mismatch is rejected (ABI drift guard) */
    const float* bias;    /* [N] or NULL */
    const void* resid;  /* RESID_F32: f32 [M, ld_resid]; RESID_BF16: bf16 [M, ld_resid]; PATCH_*: pos_embed f32 [197, N] */
    int ld_resid;
    void* aux; /* gelu' side band, uint8 [M, ld_aux]: code = round((gelu' + 0.13) * 255 / 1.26); GELU: out (nullable), DGELU: in;
                * ld_aux % 16 == 0, 16-byte aligned */
    int ld_aux;
    float dropout_p;        /* RESID_* only: C = dropout(acc + bias) + resid (HF hidden_dropout_prob); 0 = off */
    uint32_t dropout_seed;  /* decision of element (m,n) = f(seed, m*N + n): see bsclip_layernorm_bwd */
} bsclip_epi_args;
int bsclip_gemm_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                     int epilogue, const bsclip_epi_args* args, void* stream);
/* sizeof(bsclip_epi_args) as this library was compiled; bindings assert their own struct against it */
int bsclip_epi_args_size(void);

/* ---- fp8 GEMM (BASELINE.json configs[4]: fp8 MFMA encoders, bf16 LoRA / loss) ------------------------------------
 * C = epilogue(alpha[n] * (A8[M,K] . B8[N,K]^T + A_aug[M,64] . B_aug[N,64]^T) + bias[n]) on the 256x256 ping-pong kernel.
 * A8 / B8: OCP fp8 e4m3 bytes, row-major, lda/ldb in elements (= bytes), K % 128 == 0, N % 256 == 0, lda/ldb % 16 == 0.
 * alpha f32 [N]: dequantisation scale per output column (activation scale x weight-row scale; bsclip_quantize_rows_fp8).
 * a_aug / b_aug (both or neither): bf16 K-augmentation block multiplied on the bf16 MFMA as the last K-tile -- the LoRA
 *   branch: a_aug = t columns written by bsclip_layernorm_fwd (y_fp8 mode), b_aug = LoRA-B columns / alpha[n]
 *   (bsclip_lora_baug_set).  ld_* in bf16 elements, % 8 == 0.
 * form: 1 = v_mfma_f32_16x16x32_fp8_fp8 (bf16 MFMA rate, half the operand bytes); 2 = v_mfma_scale_f32_16x16x128_f8f6f4 with
 *   unit block scales (2x the bf16 MFMA rate).  Identical results (exact products, f32 accumulation; summation order differs).
 * epilogue: BSCLIP_EPI_BF16, _F32, _RESID_F32 (+ dropout), _GELU_FP8.  args->bias is required.
 * Every e4m3 value this library writes (bsclip_layernorm_fwd_fp8, _GELU_FP8, bsclip_quantize_rows_fp8) is rounded to nearest even at
 *   scale 1 and saturated at +-448: a finite value beyond the bound and +-inf become 0x7e / 0xfe.  A NaN is NOT saturated: it is
 *   written as the NaN code (0x7f / 0xff) and stays NaN through the next GEMM, where a non-finite check can see it.  _GELU_FP8
 *   saturates on its pre-activation x (x >= 448, +inf included, -> 0x7e); x = -inf or NaN gives the NaN code. */
typedef struct bsclip_fp8_args {
    uint32_t struct_size; /* = sizeof(bsclip_fp8_args) */
    int form;
    const float* alpha;
    const void* a_aug;
    int ld_a_aug;
    const void* b_aug;
    int ld_b_aug;
} bsclip_fp8_args;
int bsclip_gemm_fp8(const void* A8, int lda, const void* B8, int ldb, void* C, int ldc, int M, int N, int K, int epilogue,
                    const bsclip_epi_args* args, const bsclip_fp8_args* f8, void* stream);
/* Row-wise quantisation of frozen weights: src f32 [R, C] -> dst fp8 e4m3 [R, ld_dst], scale[r] = amax(src[r,:]) / 448
 * (1 for an all-zero row), dst = round(src / scale[r]).  C % 4 == 0. */
int bsclip_quantize_rows_fp8(const float* src, int R, int C, void* dst, int ld_dst, float* scale, void* stream);
/* b_aug[3H, 64] bf16 (zero outside the LoRA columns): cols [0,4) of rows [0,H) = B_q / alpha, cols [4,8) of rows [2H,3H) =
 * B_v / alpha, refreshed every step from the f32 masters (the fp8 counterpart of bsclip_waug_set_lora_layers). */
int bsclip_lora_baug_set(void* b_aug, int ld_b, int H, const float* lora_bq, const float* lora_bv, const float* alpha,
                         void* stream);
/* one-time device tables (GELU Phi/phi table of the 256x256 kernel's epilogue).  bsclip_gemm_bf16 fills them lazily on
 * its own stream; call this once (and synchronise) before launching GEMMs from several streams. */
int bsclip_init_tables(void* stream);
/* tile override for benchmarking: 0 = auto, 1 = 128x128, 2 = 256x128, 3 = 256x256, 4 = 256x256 ping-pong,
 * 5 = the 256x128 kernel that runs two workgroups per CU (csrc/gemm_duo.h), 8 = the persistent form of 4 (one workgroup per CU
 * walks the tiles, the next tile's first K-tile staged under the current one's last; csrc/gemm_pers.h); the diagnostic
 * library (-DBSCLIP_DIAG, `make diag`) adds 6 = ping-pong with the LDS-DMA two K-tiles ahead (slower) and 7 = four instead of
 * eight barriers per K-tile (equal), kept for comparison only */
int bsclip_gemm_set_tile(int tile);
/* workgroups of the persistent kernel's launch: 0 = one per CU (the default); a small number makes every workgroup walk many
 * tiles of a small problem (tests) */
int bsclip_gemm_set_persistent_grid(int workgroups);
#ifdef BSCLIP_DIAG
/* ---- diagnostic builds: only in libbsclip_hip_diag.so (`make -C bioscan-clip_amd/csrc diag`), never in the product library.
 * bsclip_gemm_diag: the 256x256 kernel with per-workgroup phase stamps (start, prologue, K loop, end, epilogue sections) in
 * 100 MHz ticks, diag[grid * 16]; tools/gemm_phases.py.
 * bsclip_gemm_diag_ablate: which parts of the K loop the diagnostic EPI_BF16 build leaves out (1 MFMA, 2 LDS reads, 4 DMA,
 * 8 barriers; sums of two for the instantiated pairs): timing experiments only, results are garbage.  tools/gemm_ablate.py */
int bsclip_gemm_diag_ablate(int mask);
int bsclip_gemm_diag(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                     int epilogue, const bsclip_epi_args* args, unsigned long long* diag, void* stream);
/* the 256x128 two-workgroups-per-CU kernel (bsclip_gemm_set_tile(5)) with per-workgroup stamps, diag[grid * 8] = {start, tile 0
 * landed, K loop done, end, HW_ID, XCC_ID, -, -}: section times and co-residency; tools/gemm_duo_phases.py */
int bsclip_gemm_duo_diag(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                         int epilogue, const bsclip_epi_args* args, unsigned long long* diag, void* stream);
/* the persistent 256x256 kernel (bsclip_gemm_set_tile(8)) on `workgroups` workgroups with per-workgroup stamps, diag[grid * 32] =
 * {start, end, tiles done, -, second tile: K loop start, K loop end, after each of the 8 epilogue barriers, first tile: K loop
 * start, K loop end, second tile: end of K-tile 0..15}; tools/gemm_pers_phases.py */
int bsclip_gemm_pers_diag(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                          int epilogue, const bsclip_epi_args* args, unsigned long long* diag, int workgroups, void* stream);
/* the attention backward kernel (S = 197 or 133, no mask, no dropout) with per-wave section stamps in 100 MHz ticks,
 * diag[B*heads*4*8]; tools/attn_phases.py */
int bsclip_attn_bwd_diag(const void* qkv, int ld_qkv, const void* dctx, int ld_ctx, const float* lse, int B, int S,
                         int heads, float scale, void* dqkv, int ld_dqkv, unsigned long long* diag, void* stream);
/* Round 4 experiment, NOT a product kernel since ABI 9 (the pair is a wash against bsclip_attn_fwd / bsclip_attn_bwd, docs/HISTORY.md 6.0):
 * the same attention with a backward that forms every product once (csrc/attn_sweep.hip: key-owner waves sweep the query
 * blocks, a dQ wave follows; 20 MFMAs + 16 exp per 32x32 tile pair instead of 32 + 32).  delta = rowsum(P . dP) is taken from
 * the forward's OUTPUT, which therefore leaves O to 16 mantissa bits -- ctx = bf16(O) (the out-projection's operand, as before)
 * and ctx_lo = bf16(O - ctx), same layout -- and per query row stats[B, heads, S, 4] f32 = (nm2, inv, rZ, 0): e_k = exp2(s_k
 * scale log2e + nm2), inv = 1 / sum_k e_k, rZ = sum_k e_k / Z' where Z' sums the bf16-ROUNDED operands of the P.V product
 * (dropped keys: their e_k), so that sum_k dS_k = 0 holds to f32 rounding with delta = (dctx . O) rZ.  stats 16-byte aligned.
 * No q_rows form (every query row carries a gradient); argument meaning otherwise as bsclip_attn_fwd / bsclip_attn_bwd. */
int bsclip_attn_fwd2(const void* qkv, int ld_qkv, int B, int S, int heads, const float* key_bias, float scale, void* ctx,
                     void* ctx_lo, int ld_ctx, float* stats, float dropout_p, uint32_t dropout_seed, void* stream);
int bsclip_attn_bwd2(const void* qkv, int ld_qkv, const void* dctx, int ld_dctx, const void* ctx, const void* ctx_lo, int ld_ctx,
                     const float* stats, int B, int S, int heads, const float* key_bias, float scale, void* dqkv, int ld_dqkv,
                     float dropout_p, uint32_t dropout_seed, void* stream);
/* the key-owner-sweep backward (bsclip_attn_bwd2; S = 197 or 133, no mask, no dropout) with per-wave section stamps,
 * diag[B*heads*(NB+1)*8], NB = ceil(S / 32) key-owner waves + the dQ wave; tools/attn_sweep_phases.py */
int bsclip_attn_bwd2_diag(const void* qkv, int ld_qkv, const void* dctx, int ld_dctx, const void* ctx, const void* ctx_lo,
                          int ld_ctx, const float* stats, int B, int S, int heads, float scale, void* dqkv, int ld_dqkv,
                          unsigned long long* diag, void* stream);
/* the persistent form of the same (csrc/attn_pers.hip): per-wave stamps of each workgroup's second item, diag[grid * (NB+1) * 16];
 * tools/attn_pers_phases.py */
int bsclip_attn_bwd_pers_diag(const void* qkv, int ld_qkv, const void* dctx, int ld_dctx, const void* ctx, const void* ctx_lo,
                              int ld_ctx, const float* stats, int B, int S, int heads, float scale, void* dqkv, int ld_dqkv,
                              unsigned long long* diag, void* stream);
#endif

/* ---- LayerNorm (timm norm1/norm2/norm eps 1e-6; HF BertLayerNorm eps 1e-12) ------------------------------------
 * fwd: y = LN(x) * gamma + beta for f32 rows x[M,H] (H = 768 or 512).
 *   y_bf16 [M, ld_y]  (nullable): bf16(y) in cols [0,H); if lora_a != NULL cols [H,H+8) = bf16(y . lora_a^T) and
 *                     cols [H+8, H+BSCLIP_KPAD) = 0 (the K-augmentation block consumed by the QKV GEMM).
 *   y_f32  [M, H]     (nullable): f32 copy (post-LN residual stream of BERT).
 *   y_split3 [M, ld_y3 >= 3H] bf16 (nullable; exact mode, ABI 9): the output as the A operand of a split-bf16 GEMM, [hi | lo | hi] with
 *                     hi = bf16(y), lo = bf16(y - hi) -- what bsclip_split3_rows makes of y_f32 in a second pass.
 *   stats  [M, 2]     (nullable): (mean, rstd) saved for backward.
 *   x_bf16 != 0: x is bf16 [M, ld_x] instead of f32 (MLM transform LN after GELU).
 * bwd (gamma/beta frozen -> only dx): dy = g_resid(f32, nullable) + g_gemm(bf16, nullable) + dt[M,8] . lora_a
 *   mode 0 (pre-LN, ViT):  dx = g_resid + LNbwd(g_gemm + dt.lora_a)
 *   mode 1 (post-LN, BERT): dx = LNbwd(g_resid + g_gemm + dt.lora_a)
 *   Dropout (HF BERT, K15): fwd applies it to y (both copies; the embeddings LayerNorm); bwd applies it to dx_bf16 only --
 *   dx_bf16 is the operand of the dX GEMM of a Linear whose FORWARD output was dropped with the same (p, seed), and the
 *   mask of element (row, col) is a pure function of (seed, row*H + col), so it is regenerated, never stored.
 *   writes dx_f32 [M, ld_dx] (nullable) and dx_bf16 [M, ld_dxb] (nullable).  Row strides let the final ViT norm run on
 *   the token-0 rows only (x, g and dx all strided by 197*H).  stats is indexed by the compact row number.
 *   in_dropout_p > 0 (full fine-tuning, BertEmbeddings): the LN's own OUTPUT was dropped in forward with (p, seed); the
 *   assembled dy is masked the same way before it is differentiated. */
int bsclip_layernorm_fwd(const void* x, int ld_x, int x_bf16, int M, int H, const float* gamma, const float* beta,
                         float eps, void* y_bf16, int ld_y, float* y_f32, void* y_split3, int ld_y3, const float* lora_a, float* stats,
                         float dropout_p, uint32_t dropout_seed, void* stream);
/* fp8 operand variant (configs[4]): y_fp8 [M, ld_y bytes] = e4m3(LN(x)) (scale 1, saturated at +-448; a NaN row -- a NaN or an
 * infinity in x -- is written as NaN codes, see bsclip_gemm_fp8), t_aug bf16 [M, ld_t] = the LoRA
 * block (t in cols [0,8), zeros to col 64) when lora_a != NULL -- the operands of bsclip_gemm_fp8.  Other arguments as above. */
int bsclip_layernorm_fwd_fp8(const void* x, int ld_x, int x_bf16, int M, int H, const float* gamma, const float* beta,
                             float eps, void* y_fp8, int ld_y, void* t_aug, int ld_t, float* y_f32, const float* lora_a,
                             float* stats, float dropout_p, uint32_t dropout_seed, void* stream);
/* resid_flags: the residual-gradient stream (g_resid in, dx_f32 out) may be kept in bf16 -- bit 0: g_resid is bf16 [M, ld_gr],
 *   bit 1: dx_f32 points to a bf16 [M, ld_dx] buffer (the undropped gradient, rounded once); 0 = both f32.
 *   Exact mode: bit 2: g_gemm is f32; bit 3: the operand output dx_bf16 is f32 [M, ld_dxb]; bit 4 (ABI 9, excludes bit 3): the operand
 *   output is the split-bf16 GEMM operand [hi | lo | hi], bf16 [M, ld_dxb >= 3H]. */
int bsclip_layernorm_bwd(const void* x, int ld_x, int x_bf16, const float* stats, const float* gamma, int M, int H,
                         const void* g_resid, int ld_gr, const void* g_gemm, int ld_g, const float* dt,
                         const float* lora_a, int mode, void* dx_f32, int ld_dx, void* dx_bf16, int ld_dxb,
                         float dropout_p, uint32_t dropout_seed, float in_dropout_p, uint32_t in_dropout_seed,
                         int resid_flags, void* stream);

/* ---- self-attention (timm Attention.forward; HF BertSelfAttention) ---------------------------------------------
 * qkv bf16 [B*S, ld_qkv] with columns [q | k | v], each heads*64 wide; ctx bf16 [B*S, ld_ctx];
 * key_bias f32 [B,S] additive per key (HF extended attention mask, language_encoder.py:89) or NULL;
 * lse f32 [B, heads, S] = log-sum-exp of the scaled scores (saved for backward).  head_dim is 64.
 * dropout_p > 0: HF attention_probs_dropout_prob on the normalised probabilities (mask of (b,head,q,k) regenerated in bwd).
 * q_rows: 0 = every query; n > 0 = only the first n query rows of each sequence matter (rounded up to a block of 32):
 * fwd writes ctx/lse for those rows only, bwd takes dctx as zero on the others and writes zeros into their dq rows (the last
 * ViT block, whose output is read at token 0 only: image_encoder.py:108-109 -> timm global_pool='token').
 * S <= 224.  bwd recomputes P from qkv + lse, forms delta = rowsum(P . dP) in f32 from the same tiles (not from the
 * bf16-rounded ctx: that loses the softmax-backward cancellation), and writes dqkv in the same layout as qkv.
 * keep_bits (ABI 9, nullable; read / written only when dropout_p > 0): uint32 [B * heads, S, 2, 8], 16-byte aligned -- bit 8 g + i of word
 * kt of half h of row (b, head, q) = "key 32 kt + 8 g + 4 h + i of that query row was kept" (the key set one lane half of the kernels holds;
 * words kt >= ceil(S / 32) are unused).  The forward writes the words from the decisions it hashes; a
 * backward that is handed them reads the decisions instead of re-hashing (the same masks, hence the same gradients bit for bit;
 * the key-owner phase hashed once per element: a quarter of the S = 133 launch).  Without them the backward re-hashes, as before. */
int bsclip_attn_fwd(const void* qkv, int ld_qkv, int B, int S, int heads, const float* key_bias, float scale,
                    void* ctx, int ld_ctx, float* lse, int q_rows, void* keep_bits, float dropout_p, uint32_t dropout_seed,
                    void* stream);
int bsclip_attn_bwd(const void* qkv, int ld_qkv, const void* dctx, int ld_ctx, const float* lse, int B, int S,
                    int heads, const float* key_bias, float scale, void* dqkv, int ld_dqkv, int q_rows, const void* keep_bits,
                    float dropout_p, uint32_t dropout_seed, void* stream);
/* bsclip_attn_bwd that also leaves, from dq and dv while they are still in the accumulators, the partial sums of the rank-4 LoRA
 * gradients on q and v (ABI 10; the first pass of bsclip_lora_grad re-read dq and dv from HBM for them):
 *   dt_partial f32 [heads, 2, B*S, 4]:    [h][0][m][0:4] = dq[m, head h] . B_q[head h],  [h][1][m][0:4] = dv[m, head h] . B_v[head h]
 *   db_partial f32 [B*heads, 2, 4, 64]:   [b*heads+h][q|v][j][d] = sum over the tokens of sequence b of t[m][j (+4 for v)] * dq|dv[m][64 h + d]
 * t_aug: bf16 [B*S, ld_t], t = y A^T in columns 0..7 (the LayerNorm's block of the QKV operand), 16-byte aligned, ld_t % 8 == 0;
 * lora_b f32 [2, heads*64, 4] as bsclip_lora_grad.  With dropout the forward's keep_bits are required.  The products run on the matrix
 * pipe with B as hi + lo bf16 parts: f32 results up to accumulation order.  bsclip_lora_grad_heads reduces the partials.
 * q_rows | BSCLIP_OPERANDS_FP16 (both backward entry points): fp16 operands, S = 197, no dropout -- see BSCLIP_OPERANDS_FP16. */
int bsclip_attn_bwd_lora(const void* qkv, int ld_qkv, const void* dctx, int ld_ctx, const float* lse, int B, int S, int heads,
                         const float* key_bias, float scale, void* dqkv, int ld_dqkv, int q_rows, const void* keep_bits,
                         const void* t_aug, int ld_t, const float* lora_b, float* dt_partial, float* db_partial, float dropout_p,
                         uint32_t dropout_seed, void* stream);

/* ---- "exact" forward mode (BSCLIP_PARITY=2; csrc/exact.hip): every trunk GEMM on split-bf16 operands, f32 attention -----------
 * A bf16 MFMA GEMM is exact to ~2^-16 when both operands are carried as hi + lo (hi = bf16(x), lo = bf16(x - hi)) and the product is
 * formed as hi.hi + lo.hi + hi.lo: ONE bsclip_gemm_bf16 call with K tripled, A rows [hi | lo | hi] against W rows [hi | hi | lo].
 *   split3_rows:   src f32 [M, ld_src >= K] -> dst bf16 [M, ld_dst >= 3K] = [hi | lo | hi]   (K % 4 == 0)
 *   split3_weight: w f32 [N, K] -> dst bf16 [N, 3K] = [hi | hi | lo]; with lora_a f32 [8, K] (A_q rows 0..3, A_v rows 4..7) and lora_b
 *                  f32 [2, H, 4] the LoRA update is folded in f32 first (reference image_encoder.py:43-47, dna_encoder.py:47-49):
 *                  rows [0, H) += B_q A_q, rows [2H, 3H) += B_v A_v  (N = 3H, K = H)
 *   gelu_split3:   z f32 [M, N] -> exact (erf) GELU as bf16 [M, 3N] = [hi | lo | hi] (dst nullable) and / or as f32 [M, ld_g32] (g32
 *                  nullable; the MLM transform's GELU feeds a LayerNorm, not a GEMM); codes (nullable) u8 [M, ld_codes]: the 8-bit
 *                  gelu' side band the default backward reads
 *   meanpool_tokens_f32: x f32 [B*S, H] -> out f32 [B, H], the mean over each sequence's S tokens (language_encoder.py:89)
 *   attn_fwd_f32:  qkv f32 [B*S, ld_qkv] ([q | k | v], heads*64 each) -> ctx f32 [B*S, ld_ctx], lse f32 [B, heads, S]; f32 softmax
 *                  arithmetic, every product exact to ~2^-16 (bsclip_exact_attn_set_impl: split-bf16 operands by default, f32-operand
 *                  MFMA / vector ALU as second implementations; S <= 224), the bf16 kernels' dropout masks; argument meaning as
 *                  bsclip_attn_fwd.  ctx_split3 (nullable): ctx once more as bf16 [B*S, ld_c3 >= 3 heads 64] = [hi | lo | hi], the
 *                  out-projection GEMM's split operand (no stand-alone bsclip_split3_rows pass)
 * The exact backward (BSCLIP_PARITY=2) keeps every gradient in f32 and runs its dX / dW GEMMs on split operands as well:
 *   dgelu_split3:  dact f32 [M, N], z f32 [M, N] (fc1 pre-activation) -> dact * gelu'(z) as bf16 [M, 3N] = [hi | lo | hi] (dst nullable)
 *                  and / or f32 [M, ld_out32] (out32 nullable)
 *   split3_transpose: src f32 [R, C] -> dst bf16 [C, 3 Rp]: row c = the split of column c over Rp >= R positions (Rp % 64 == 0, zeros
 *                  beyond R), order 0 = [hi | lo | hi], 1 = [hi | hi | lo].  With order 0 / 1 on dY / X it builds the two operands of a
 *                  dW = dY^T X GEMM (the reduction runs over the R rows); with order 1 on a frozen weight [N, K] it builds W^T for the
 *                  dX GEMM; lora_a / lora_b (nullable, R = 3H, C = H) fold W + B A as in split3_weight
 *   softmax_meanpool_bwd_f32: bsclip_softmax_meanpool_bwd with f32 dlogits [B*S, ld_d]
 *   lora_grad_f32: dA [8, H] += (B^T dq | B^T dv) y^T, dB [2, H, 4] += (dq | dv)^T (A y) from dqkv f32 [M, ld_dqkv] ([dq | dk | dv]) and
 *                  the LayerNorm output y f32 [M, ld_y] (reference lora_layer.py:16-39); workspace:
 *                  bsclip_lora_grad_f32_workspace_floats(M, H) floats (t and dt [M, 8] + the per-workgroup slabs); sums in a fixed order
 *                  (round 5: t = A y by one pass, then bsclip_lora_grad's pipelined wave-per-row kernels on f32 rows)
 *   attn_bwd_f32:  dqkv f32 [B*S, ld_dqkv] from qkv f32, dctx f32, the forward's ctx f32 (delta = dctx . ctx) and lse; the forward's
 *                  implementation and dropout masks; argument meaning as bsclip_attn_bwd.  dqkv_split3 (nullable): [dq | dk | dv] once
 *                  more as bf16 [B*S, ld_d3 >= 9 heads 64] = [hi | lo | hi], the QKV dX GEMM's split operand
 * bsclip_layernorm_bwd takes the f32 GEMM gradient / writes the f32 or the split operand through resid_flags bits 2 / 3 / 4. */
int bsclip_split3_rows(const float* src, int ld_src, int M, int K, void* dst, int ld_dst, void* stream);
int bsclip_split3_weight(const float* w, int ld_w, int N, int K, const float* lora_a, const float* lora_b, int H, void* dst, int ld_dst,
                         void* stream);
int bsclip_gelu_split3(const float* z, int ld_z, int M, int N, void* dst, int ld_dst, void* codes, int ld_codes, float* g32, int ld_g32,
                       void* stream);
int bsclip_meanpool_tokens_f32(const float* x, int B, int S, int H, float* out, void* stream);
int bsclip_attn_fwd_f32(const float* qkv, int ld_qkv, int B, int S, int heads, const float* key_bias, float scale, float* ctx, int ld_ctx,
                        float* lse, void* ctx_split3, int ld_c3, float dropout_p, uint32_t dropout_seed, void* stream);
int bsclip_dgelu_split3(const float* dact, int ld_dact, const float* z, int ld_z, int M, int N, void* dst, int ld_dst, float* out32,
                        int ld_out32, void* stream);
int bsclip_split3_transpose(const float* src, int ld_src, int R, int C, int Rp, int order, const float* lora_a, const float* lora_b, int H,
                            void* dst, int ld_dst, void* stream);
int bsclip_softmax_meanpool_bwd_f32(const float* logits, const float* stats, const float* d_pooled, int B, int S, int C, float* dlogits,
                                    int ld_d, void* stream);
int64_t bsclip_lora_grad_f32_workspace_floats(int M, int H);
int bsclip_lora_grad_f32(const float* dqkv, int ld_dqkv, const float* y, int ld_y, int M, int H, const float* lora_a, const float* lora_b,
                         float* dA, float* dB, float* workspace, void* stream);
/* 0 (default, round 5) = split-bf16 operands on the bf16 matrix cores (csrc/attn_x3.hip: every product as hi.hi + lo.hi + hi.lo, f32 softmax
 * arithmetic; ~2^-16 per product, 16 x the f32 MFMA rate), 2 = f32 operands on the matrix pipe (v_mfma_f32_32x32x2_f32, round 4's default),
 * 1 = the one-row-per-thread vector-ALU kernels -- 1 and 2 are exact-f32 second implementations kept to test against */
int bsclip_exact_attn_set_impl(int impl);
int bsclip_attn_bwd_f32(const float* qkv, int ld_qkv, const float* dctx, int ld_dctx, const float* ctx, int ld_ctx, const float* lse, int B,
                        int S, int heads, const float* key_bias, float scale, float* dqkv, int ld_dqkv, void* dqkv_split3, int ld_d3,
                        float dropout_p, uint32_t dropout_seed, void* stream);

/* ---- embeddings ------------------------------------------------------------------------------------------------
 * im2col for timm PatchEmbed Conv2d(3,768,k=16,s=16): image f32 [B,3,224,224] -> bf16 [B*196, 768], column
 * order (c, ky, kx) = conv weight.flatten(1).  cls rows: x[b*197] = cls + pos[0].
 * bert_embed: word[id] + pos[t] + type[tt] -> f32 [B*S, H] (HF BertEmbeddings before LayerNorm). */
/* split != 0: each row is written as [hi | lo | hi] (3 x 768 columns, ld_cols >= 2304) for the split-bf16 patch-embed GEMM
 * against a weight stored as [hi | hi | lo] (K = 2304: hi.hi + lo.hi + hi.lo, ~2^-16 relative instead of 2^-8) */
int bsclip_im2col_patch16(const float* image, int B, void* cols_bf16, int ld_cols, int split, void* stream);
/* HF extended attention mask (BertModel, language_encoder.py:89): bias[i] = mask[i] ? 0 : finfo(f32).min */
int bsclip_mask_to_bias(const int64_t* mask, int n, float* bias, void* stream);
/* x[b*S, :] = cls_token + pos_embed[0] (x f32, or bf16 when x_bf16 != 0: the bf16 residual stream) */
int bsclip_vit_cls_rows(void* x, int x_bf16, const float* cls_token, const float* pos_embed, int B, int S, int H, void* stream);
int bsclip_bert_embed(const int64_t* ids, const int64_t* type_ids, int B, int S, int H, const float* word,
                      int vocab, const float* pos, const float* type, float* out, void* stream);

/* ---- heads -----------------------------------------------------------------------------------------------------
 * softmax_meanpool: LoRA_barcode_bert.forward `logits.softmax(-1).mean(1)` (dna_encoder.py:105):
 *   logits f32 [B*S, C] -> pooled f32 [B, C]; stats [B*S, 2] = (row max, sum exp) for backward.
 *   bwd: d_pooled f32 [B,C] -> dlogits bf16 [B*S, ld_d].
 * meanpool_tokens: LoRA_bert.forward `last_hidden_state.mean(1)` (language_encoder.py:89): f32 [B,S,H] -> bf16 [B,H].
 * l2norm: F.normalize(p=2, dim=-1, eps=1e-12) (simple_clip.py:34,47,49). */
int bsclip_softmax_meanpool_fwd(const float* logits, int B, int S, int C, float* pooled, float* stats, void* stream);
int bsclip_softmax_meanpool_bwd(const float* logits, const float* stats, const float* d_pooled, int B, int S, int C,
                                void* dlogits_bf16, int ld_d, void* stream);
int bsclip_meanpool_tokens_fwd(const float* x, int B, int S, int H, void* out_bf16, int ld_out, void* stream);
/* autograd of the mean: dx[b,t,:] = d_pooled[b,:] / S  (f32 [B*S, H]) */
int bsclip_meanpool_tokens_bwd(const float* d_pooled, int ld_d, int B, int S, int H, float* dx, void* stream);
/* out = g * z elementwise (g, out bf16 [M,N]; z uint8 codes), z = gelu'(pre-activation) as saved by BSCLIP_EPI_GELU_BF16: autograd of the
 * GELU inside cls.predictions.transform, where the producer of g is the LayerNorm backward rather than a GEMM. */
int bsclip_dgelu_mul(const void* g, int ld_g, const void* z, int ld_z, int M, int N, void* out, int ld_o, void* stream);
int bsclip_l2norm_fwd(const float* x, int M, int D, float* y, float* inv_norm, void* stream);
int bsclip_l2norm_bwd(const float* y, const float* inv_norm, const float* dy, int M, int D, float* dx, void* stream);

/* ---- contrastive loss ------------------------------------------------------------------------------------------
 * ContrastiveLoss.forward (bioscanclip/model/loss_func.py:29-54) with construct_label_metrix (:18-21) for
 * nmod = 2 or 3 modalities z[i] f32 [N, D] (D = 768).  The second F.normalize (:43-44) is applied inside
 * (forward and backward).  loss_out[0] = mean over all 2*nmod*(nmod-1) CE terms.
 * dz[i] f32 [n_local, D] receives dLoss/dz[i] for rows [row0, row0 + n_local) only (the rank's own slice of an
 * all-gathered batch); pass row0 = 0, n_local = N for the local-batch loss.
 * workspace: f32, at least bsclip_infonce_workspace_floats(N, nmod) elements. */
int64_t bsclip_infonce_workspace_floats(int N, int nmod);
/* implementation switch for benchmarking / cross-checking: 2 = fused -- the logits tile stays in the MFMA
 * accumulators, row max / log-sum-exp reduced with wave shuffles in the GEMM epilogue, pass 2 emits dL/dG from the
 * accumulators; 1 = logits formed in f32 row slabs in the workspace and reduced by separate kernels (round 1);
 * 0 (default) = by size: fused from 2 048 (padded) rows up, slabs below, where a product is too few 256 x 256 tiles to fill the chip */
int bsclip_infonce_set_impl(int impl);
int bsclip_infonce_fwd_bwd(const float* const* z, int nmod, const int64_t* labels, int N, int D, float scale,
                           int row0, int n_local, float* loss_out, float* const* dz, float* workspace,
                           void* stream);
/* Trainable temperature: bsclip_infonce_fwd_bwd with the scale in device memory as its logarithm.
 * log_scale_dev: one f32 t on the device, read when the kernels run and not at launch, so a replayed graph sees each step's value.
 * The scale used is s = exp(min(max(t, 0), ln 100)) (open_clip's clamp range; exactly 1 and 100 at and beyond the ends).
 * loss_out and dz are those of bsclip_infonce_fwd_bwd at that s, bit for bit: same layouts, same row0 / n_local meaning, the
 * same three forms chosen by the same rules, bsclip_infonce_set_impl honoured, the same workspace size.
 * scale_out f32 [2], required; it is also written early and read by the kernels of the call, so it must not alias anything else:
 *   scale_out[1] = s;
 *   scale_out[0] = the rank's share of dLoss/dt = s/(P N) * sum_{a != b} sum_{i in [row0, row0 + n_local)} sum_j
 *                  (cnt_i p^{ab}_ij - T_ij) G^{ab}_ij   (P = nmod (nmod - 1), G the cosines, p = softmax_j(s G), T_ij = [label_i ==
 *                  label_j], cnt_i = sum_j T_ij).  The shares of disjoint row slices add up to dLoss/dt, which is what a SUM
 *                  all-reduce needs.  0 when dz is NULL or n_local == 0, and 0 when t lies outside [0, ln 100] (the clamp's derivative).
 * No atomics: a repeated call returns the same bits.  All arguments are checked before the first launch; -1 names the bad one. */
int bsclip_infonce_fwd_bwd_ts(const float* const* z, int nmod, const int64_t* labels, int N, int D, const float* log_scale_dev,
                              int row0, int n_local, float* loss_out, float* const* dz, float* scale_out, float* workspace,
                              void* stream);
/* Sigmoid (SigLIP, Zhai et al. ICCV 2023) contrastive loss with a learnable scale and bias, forward + backward in one call.
 * z: nmod (2 or 3) f32 [N, 768]; zn = F.normalize(z) is applied inside, with its Jacobian in the backward; G^{ab} = zn^a (zn^b)^T.
 * log_scale_dev, bias_dev: one f32 each on the device (t and b), read when the kernels run and not at launch, so a replayed graph
 * sees each step's values.  s = exp(min(max(t, 0), ln 100)) as in bsclip_infonce_fwd_bwd_ts (exactly 1 and 100 at and beyond the ends).
 *   x_ij = s G_ij + b,  y_ij = +1 if label_i == label_j else -1,
 *   loss = 1/(P N) * sum_{a != b} sum_i sum_j softplus(-y_ij x^{ab}_ij),  P = nmod (nmod - 1)
 * (directed pairs, so the value compares with the InfoNCE mean; (a,b) and (b,a) hold the same terms, each unordered pair's logits
 * are formed once for the loss).  softplus and the sigmoid are the stable forms: exp is only taken of -|x|.
 * row0 / n_local as for bsclip_infonce_fwd_bwd: dz[m] f32 [n_local, 768] holds dLoss/dz^m of the rows [row0, row0 + n_local);
 * dz NULL or n_local == 0: loss only.  loss_out is the loss over all rows in either case.
 * aux_out f32 [4], required, written last (it must not alias log_scale_dev or bias_dev), with w_ij = -y_ij sigmoid(-y_ij x_ij):
 *   aux_out[0] = the own rows' share of dLoss/dt = 2 s/(P N) * sum_{a < b} sum_{i in [row0, row0 + n_local)} sum_j w^{ab}_ij G^{ab}_ij;
 *                0 when dz is NULL or n_local == 0, and 0 when t lies outside [0, ln 100] (the clamp's derivative)
 *   aux_out[1] = s
 *   aux_out[2] = the own rows' share of dLoss/db = 2/(P N) * sum_{a < b} sum_{i in own rows} sum_j w^{ab}_ij; 0 when dz is NULL or n_local == 0
 *   aux_out[3] = b
 * A row's share holds the cells (i, j) of G^{ab}, a < b, and their mirror cells (j, i) of G^{ba}; the shares of disjoint row slices
 * add up to the whole gradient, which is what a SUM all-reduce needs.
 * workspace: bsclip_infonce_workspace_floats(N, nmod) floats, 16-B aligned.  Of the InfoNCE layout the call uses the normalised
 * rows, the split operands, the logits (G) and dL/dG (W) regions and the gradient accumulator; the per-row sums of pass 1
 * (f64 [nmod (nmod - 1) / 2, Np, 3]) lie at the head of the gradient accumulator, which pass 2 writes after they were read.
 * Two forms by size, as for InfoNCE: up to 1024 padded rows one launch per stage over all pairs, above that 1024-row slabs launch
 * by launch.  There is no fused-epilogue form: bsclip_infonce_set_impl has no effect here.
 * No atomics, sums in f64 in a fixed order: a repeated call returns the same bits.  D = 768, N <= 16384; every argument is
 * checked before the first launch; -1 names the bad one. */
int bsclip_sigmoid_loss_fwd_bwd(const float* const* z, int nmod, const int64_t* labels, int N, int D, const float* log_scale_dev,
                                const float* bias_dev, int row0, int n_local, float* loss_out, float* const* dz, float* aux_out,
                                float* workspace, void* stream);
/* Cross-batch memory (XBM, Wang et al. CVPR 2020) for the InfoNCE: the normalised embeddings of the last steps stay on the GPU in
 * one ring buffer per modality and enter the loss as extra key columns that take no gradient.  One rank only.
 * bank[m]: f32, bsclip_xbm_bank_floats(Q) elements, 16-B aligned, one per modality.  Its first Q * 768 floats are the normalised
 * f32 rows by slot (row j at [768 j, 768 j + 768)); what follows belongs to the implementation (each row's split-bf16 operands,
 * row-major and transposed, written once at enqueue so that a step never re-splits the bank) and only these calls touch it.
 * bank_labels: int64 [Q], the label of each slot, shared by the modalities.
 * state_dev: int32 [2] on the device = (head, filled): head is the slot the next enqueue writes first, slot j is valid iff
 * j < filled.  Both words are read, and by bsclip_xbm_enqueue written, when the kernels run and not at launch, so a replayed graph
 * advances the ring.  An empty bank is state_dev = (0, 0); the contents of slots that are not valid never matter.
 * Limits of both calls: D = 768, nmod 2 or 3, 1 <= N <= 1024, Q a multiple of 256 in [256, 16384], N <= Q, 16-byte aligned z[m],
 * bank[m], dz[m] and workspace.  Every argument is checked before the first launch; -1 names the bad one.
 * workspace: f32, bsclip_xbm_workspace_floats(N, Q, nmod) elements; the two calls may share it. */
int64_t bsclip_xbm_bank_floats(int Q);
int64_t bsclip_xbm_workspace_floats(int N, int Q, int nmod);
/* Row i of every z[m] (f32 [N, 768]) is normalised (z / max(||z||, 1e-12)) and written to slot (head + i) % Q of bank[m], with
 * labels[i] to bank_labels; then head = (head + N) % Q and filled = min(filled + N, Q), from a launch of its own that is
 * stream-ordered after the row writes.  If any of the nmod * N input rows holds a non-finite value the whole call leaves the
 * banks, the labels and the state untouched: per-row flags, reduced by one workgroup in a fixed order, predicate the writers
 * (one overflowed step would otherwise poison the next Q / N steps).  5 launches. */
int bsclip_xbm_enqueue(const float* const* z, int nmod, const int64_t* labels, int N, int D, float* const* bank, int64_t* bank_labels,
                       int Q, int32_t* state_dev, float* workspace, void* stream);
/* InfoNCE with the valid bank slots as extra keys, forward + backward in one call.  For every ordered pair (a, b), a != b, the key
 * set C of b is its N own rows followed by the valid slots of bank[b]:
 *   x_ij = s <zn^a_i, k^b_j>,  T_ij = [labels_i == label of key j],  cnt_i = sum_{j in C} T_ij
 *   loss = 1/(P N) sum_{a != b} sum_i ( cnt_i logsumexp_{j in C} x_ij - sum_{j in C} T_ij x_ij ),  P = nmod (nmod - 1)
 * s = exp(min(max(t, 0), ln 100)) with t = *log_scale_dev read on the device, as in bsclip_infonce_fwd_bwd_ts (a fixed temperature
 * passes ln(scale) in a device word).  With filled = 0 this is bsclip_infonce_fwd_bwd_ts's loss.  Slots >= filled are selected out
 * of the log-sum-exp, of T and of cnt (their contents may be anything, NaN included); the call zeroes the implementation's
 * transposed operand of those slots in bank[m], the documented rows and bank_labels are only read.
 * dz[m] f32 [N, 768] (dz NULL: loss only): dLoss/dz^m -- the row role of m in every (m, b) through own and bank columns, the column
 * role in every (b, m) through its own N columns; bank rows take no gradient.
 * scale_out f32 [2]: scale_out[1] = s; scale_out[0] = dLoss/dt = s/(P N) sum_{a != b} sum_i sum_{j in C} (cnt_i p_ij - T_ij) G_ij
 * (G the cosines, p the softmax over C), 0 when dz is NULL or t lies outside [0, ln 100].
 * No atomics: row statistics in f64 partials per row, one workgroup sums them, the long key reduction of dz runs as a split over
 * the keys whose partial tiles are added in a fixed order; a repeated call returns the same bits.
 * Launches with gradients: 8 + nmod + 2 R with R runs of stacked queries in the split over the keys (R = 2 at nmod = 2, 4 at
 * nmod = 3): 14 and 19 wherever the products of one stage go as one batched launch over the pairs (every N <= 1024 except bank
 * logits of ceil(N / 256) * Q / 256 >= 192 tiles, which go pair by pair). */
int bsclip_infonce_xbm_fwd_bwd(const float* const* z, int nmod, const int64_t* labels, int N, int D, const float* log_scale_dev,
                               float* const* bank, const int64_t* bank_labels, int Q, const int32_t* state_dev, float* loss_out,
                               float* const* dz, float* scale_out, float* workspace, void* stream);

/* ---- retrieval --------------------------------------------------------------------------------
 * make_prediction (scripts/inference_and_eval.py:414-445): faiss IndexFlatIP over L2-normalised keys f32 [K, D], searched
 * with L2-normalised queries f32 [Q, D] (sklearn normalize, :416-417).  Outputs the top k (<= 16) inner products per query in
 * descending order (ties: lower key index first): scores_out f32 [Q, k], idx_out int64 [Q, k].  D % 64 == 0. */
int64_t bsclip_topk_ip_workspace_floats(int Q, int K, int D);
int bsclip_topk_ip(const float* queries, int Q, const float* keys, int K, int D, int k, float* scores_out,
                   int64_t* idx_out, float* workspace, void* stream);
/* faiss `index.add(keys)` once, many `.search`: bsclip_retrieval_index_build normalises and splits the keys f32 [K, D] into
 * `index`, a caller-owned 16-B aligned buffer of bsclip_retrieval_index_floats(K, D) floats (the key operand bsclip_topk_ip builds
 * on every call: bf16 [K padded to 256, 4 D], [lo|hi|lo|hi]).  bsclip_topk_ip_indexed is the query side of bsclip_topk_ip against
 * that buffer: same kernels, bit-identical outputs; it only reads the index.  workspace: f32, 16-B aligned, at least
 * bsclip_topk_ip_indexed_workspace_floats(Q, K, D) elements. */
int64_t bsclip_retrieval_index_floats(int K, int D);
int bsclip_retrieval_index_build(const float* keys, int K, int D, float* index, void* stream);
int64_t bsclip_topk_ip_indexed_workspace_floats(int Q, int K, int D);
int bsclip_topk_ip_indexed(const float* queries, int Q, const float* index, int K, int D, int k, float* scores_out,
                           int64_t* idx_out, float* workspace, void* stream);
/* The key side of bsclip_retrieval_index_build for rows [row0, row0 + n) of an index sized by
 * bsclip_retrieval_index_floats(K_capacity, D) that the caller has zero-filled: keys f32 [n, D] become those rows of the operand.
 * Any sequence of appends covering [0, K) leaves the buffer bit-identical to bsclip_retrieval_index_build of the whole [K, D] table
 * (the zero pad rows included); bsclip_topk_ip_indexed reads it unchanged.  D % 64 == 0, row0 + n <= K_capacity, 16-B aligned. */
int bsclip_retrieval_index_append(const float* keys, int n, int D, float* index, int K_capacity, int row0, void* stream);
/* Feature tables of one evaluation split (get_features_and_label, scripts/inference_and_eval.py:734-784), filled a batch at a time:
 * rows [row0, row0 + B) of each given table f32 [N, D] receive the rows of its input f32 [B, D] unchanged; t_avg [N, D] receives
 * (image + dna) * 0.5f (averaged_feature: the f32 rounding of numpy's float64 mean of two f32 values) and t_cat [N, 2 D] receives
 * [image | dna] (concatenated_feature).  image / dna / text are nullable, each together with its table; t_avg and t_cat are
 * nullable and need both image and dna.  D % 4 == 0, B >= 1, 0 <= row0, row0 + B <= N, every pointer 16-B aligned.  One launch. */
int bsclip_feature_rows(const float* image, const float* dna, const float* text, int B, int D, int64_t row0, int64_t N,
                        float* t_image, float* t_dna, float* t_text, float* t_avg, float* t_cat, void* stream);
/* Scoring on integer label ids (make_prediction's label lookup :424-437, top_k_micro_accuracy :448-464, top_k_macro_accuracy
 * :467-511); integers only, the caller forms the ratios.
 *   hit_ranks: idx int64 [Q, k] (k <= 16), key_labels int32 [K, L], query_labels int32 [Q, L], L <= 8 levels ->
 *     hit_rank int32 [Q, L] = the smallest r in [0, k) with key_labels[idx[q, r], l] == query_labels[q, l], or k without one;
 *     a hit at top-k' (k' <= k) is hit_rank < k'.
 *   class_counts: level_offsets int32 [L + 1] (HOST memory, level_offsets[0] = 0, non-decreasing) places the class ids of level l
 *     at [level_offsets[l], level_offsets[l + 1]) of one flat range of C = level_offsets[L] classes; k_list int32 [nk] (HOST
 *     memory, nk <= 8).  seen int32 [C] = queries per class, right int32 [nk, C] = those with hit_rank < k_list[j]; both are
 *     cleared by the entry point.  Integer atomics: the result does not depend on their order.
 * flag: one int32 device word the caller clears; the kernels only OR into it, so one word serves many calls.  Bit 0: an idx
 * entry outside [0, K) (never dereferenced, counted as no hit); bit 1: a query label outside its level's range (not counted). */
int bsclip_retrieval_hit_ranks(const int64_t* idx, int Q, int k, const int32_t* key_labels, int K, const int32_t* query_labels,
                               int L, int32_t* hit_rank, int32_t* flag, void* stream);
int bsclip_retrieval_class_counts(const int32_t* hit_rank, const int32_t* query_labels, int Q, int L,
                                  const int32_t* level_offsets, const int32_t* k_list, int nk, int32_t* seen, int32_t* right,
                                  int32_t* flag, void* stream);
/* Method-one evaluation (scripts/method_one_eval.py): an image query is searched against the seen keys and against the unseen
 * keys; rank slot r keeps the seen-key prediction when its similarity is above a threshold and takes the unseen-key one otherwise.
 * On label ids the two prediction lists of a query are two bit masks per level, and the merge is (A & s) | (B & ~s).
 *   match_bits: the label lookup of make_prediction and the `gt[level] in pred[level][:k]` of top_k_micro_accuracy, kept per
 *     rank.  idx int64 [Q, k] (k <= 16), key_labels int32 [K, L], query_labels int32 [Q, L], L <= 8 -> bits int32 [Q, L]: bit r
 *     is set exactly when key_labels[idx[q, r], l] == query_labels[q, l]; bits >= k are zero (ctz(bits), or k for 0, is the
 *     hit_rank of bsclip_retrieval_hit_ranks).  With member != NULL (int32 0/1 [C]) it is the `single_pred in species_list` of
 *     check_for_acc_about_correct_predict_seen_or_unseen (:264-278): bits int32 [Q], bit r set exactly when
 *     member[key_labels[idx[q, r], level]] != 0; query_labels is not read and may be NULL.  flag as above: bit 0 for an idx
 *     entry outside [0, K), bit 1 for a label outside [0, C); neither is dereferenced, its bit stays zero.
 *   merge_hit_ranks: decide_prediction_with_threshold (:59-84) followed by the hit test.  sim f32 [Q, k], A / B int32 [Q, L] the
 *     masks of the seen-key / unseen-key search.  s has bit r set exactly when (double)sim[q, r] > threshold -- strict, in
 *     float64 as Python compares `similarity.tolist()` with np.linspace values, so a NaN takes the unseen-key prediction; no order
 *     is assumed within a row.  hit_rank int32 [Q, L] = the lowest set bit below k of (A & s) | (B & ~s), or k: the contract of
 *     bsclip_retrieval_hit_ranks, so bsclip_retrieval_class_counts applies unchanged.
 *   threshold_sweep: the loop of search_threshold_with_harmonic_mean (:131-157) without the lists.  thresholds double [T] (DEVICE
 *     memory, any order); counts int32 [T] (zeroed by the caller, added to): counts[j] += the number of queries whose merged
 *     hit_rank at level `level` and threshold thresholds[j] is below k_prime (above k that is every query: clamp k_prime to k for
 *     the meaning of `pred[:k_prime]`, as for class_counts).  Brute force
 *     over (query, threshold); integer atomics only, so every run gives the same counts. */
int bsclip_retrieval_match_bits(const int64_t* idx, int Q, int k, const int32_t* key_labels, int K, const int32_t* query_labels,
                                int L, const int32_t* member, int C, int level, int32_t* bits, int32_t* flag, void* stream);
int bsclip_retrieval_merge_hit_ranks(const float* sim, int Q, int k, const int32_t* A, const int32_t* B, int L, double threshold,
                                     int32_t* hit_rank, void* stream);
int bsclip_retrieval_threshold_sweep(const float* sim, int Q, int k, const int32_t* A, const int32_t* B, int L, int level,
                                     int k_prime, const double* thresholds, int T, int32_t* counts, void* stream);

/* ---- supervised fine-tuning: species classifier on an encoder (util.EncoderWithExtraLayer) ----------------
 * The head `new_linear_layer` (bioscanclip/util/util.py:13-25) is logits [B, C] = z W^T + b for any C >= 1.  It runs on
 * bsclip_gemm_bf16 with split-bf16 operands (bsclip_split3_rows x bsclip_split3_weight, N = C padded to 128), so the logits
 * live in a padded buffer [B, ldc]; both entry points read columns [0, C) only: a padded column is absent, not a logit of 0.
 * ce_fwd_bwd: `criterion(output, target)` with nn.CrossEntropyLoss() (bioscanclip/epoch/fine_tuning_epoch.py:27,93) and its
 *   autograd.  logits f32 [B, ldc] (ldc >= C, ldc % 4 == 0, 16-byte aligned), targets int32 [B].  Per row, in f32: the maximum
 *   is subtracted first (logits of magnitude 1e4 are fine), row_loss[r] = log sum_c exp(x_c - max) + (max - x_target);
 *   loss_out[0] = sum_r row_loss[r] / B, summed in a fixed order (no float atomics: eager and graph replay agree bit for bit).
 *   dlogits = (softmax - onehot) / B goes out in the forms the backward products read, each nullable (both NULL: loss only):
 *     dlogits        f32 [B, ld_d] (ld_d >= C, % 4, 16-byte aligned): columns [0, C) are written, the rest is left alone --
 *                    bsclip_colsum makes db of it, bsclip_split3_transpose the operand of dW += dlogits^T z
 *     dlogits_split3 bf16 [B, ld_d3 >= 3 Cp], Cp = C rounded up to 64, 8-byte aligned: [hi | lo | hi], Cp columns each, zeros
 *                    in columns [C, Cp) -- the A operand of dz = dlogits W against bsclip_split3_transpose(W, order 1, Rp = Cp)
 *   A target outside [0, C) is never used as an index: it ORs bit 0 into *flag (one int32 device word the caller clears, as for
 *   bsclip_retrieval_hit_ranks) and its row gets loss 0 and a zero gradient; the divisor stays B.  row_loss f32 [B] is scratch
 *   the caller owns (the per-row losses stay readable in it).
 * class_topk: `torch.argsort(output, dim=1, descending=True)[:, :max(k_values)]` (fine_tuning_epoch.py:60): the k (<= 16,
 *   <= C) largest of each row's C logits in descending order, scores_out f32 [B, k], idx_out int64 [B, k].  Ties resolve to the
 *   lower class index.  Same layout requirements for logits as above. */
int bsclip_ce_fwd_bwd(const float* logits, int ldc, const int32_t* targets, int B, int C, float* loss_out, float* row_loss,
                      float* dlogits, int ld_d, void* dlogits_split3, int ld_d3, int32_t* flag, void* stream);
int bsclip_class_topk(const float* logits, int ldc, int B, int C, int k, float* scores_out, int64_t* idx_out, void* stream);

/* ---- method two: classifier confidences (reference scripts/method_two_fine_tuning_and_eval.py) --------------------------
 * class_softmax_topk: `F.softmax(output, dim=-1)` followed by `torch.topk(..., k=5, dim=1, largest=True, sorted=True)`
 *   (method_two_fine_tuning_and_eval.py:57-62) in one pass over the logits plus the selection's re-scan: the k (<= 16, <= C)
 *   highest softmax confidences of each row, conf_out f32 [B, k], and their class indices, idx_out int64 [B, k].  logits as for
 *   bsclip_class_topk: f32 [B, ldc], ldc >= C, ldc % 4 == 0, 16-byte aligned; columns >= C are absent, not logits of 0.
 *   conf = expf(x - M) / S in f32 with M the row maximum and S = sum_c expf(x_c - M) (logits of magnitude 1e4 are fine; a logit
 *   of -inf has confidence 0); S is summed in a fixed order (no float atomics: a repeated call gives the same bits).
 *   Tie rule: the order is by LOGIT descending, ties to the lower class index -- softmax is monotone, so this is torch.topk's
 *   order wherever that is defined, also where distinct logits round to equal confidences.  A row that holds a NaN logit gets
 *   NaN confidences; its indices stay inside [0, C) (a NaN ranks first, as in torch.topk).
 *   The confidences feed the method-one merge kernels (bsclip_retrieval_match_bits on a class table [C, L] built from
 *   idx_to_all_labels, bsclip_retrieval_threshold_sweep, bsclip_retrieval_merge_hit_ranks): decide_prediction_with_threshold
 *   (:88-114) compares them strictly against the threshold, search_threshold_with_harmonic_mean (:177-204) sweeps
 *   np.linspace(0, 1, num_intervals + 1). */
int bsclip_class_softmax_topk(const float* logits, int ldc, int B, int C, int k, float* conf_out, int64_t* idx_out, void* stream);

/* ---- silhouette coefficients (reference scripts/inference_and_eval.py:407-411) ------------------------------------------
 * silhouette_samples: sklearn's `silhouette_samples(image_features, gt_list)` with the euclidean metric, as
 *   calculate_silhouette_score (scripts/inference_and_eval.py:407-411) calls it once per taxonomic level.  The caller sorts the samples by class, so class c is the row
 *   range [seg_start[c], seg_start[c+1]) of x_sorted (f32 [N, ld], 16-byte aligned, ld >= D, ld % 4 == 0; what lies between D and
 *   ld is not read as features); seg_start is int32 [C + 1], on the device.  For row i of class A with n_A members:
 *   a = sum_{j in A} d(i,j) / (n_A - 1), b = min over the classes B != A of sum_{j in B} d(i,j) / n_B, out_sorted[i] =
 *   (b - a) / max(a, b), f32 [N]; 0 for a singleton class and where the quotient is no number (a = b = 0).  d(i,j) =
 *   sqrt(sum_k (x_ik - x_jk)^2) from the DIFFERENCES, f32 accumulation (never the Gram form, which cancels for near-duplicate
 *   rows); d(i,i) = 0 exactly.  The sums over a class are carried in double and added in column order: no float atomics, a
 *   repeated call gives the same bits.  Rows of out_sorted beyond N are not written.
 *   *flag is one int32 device word the caller clears (as for bsclip_retrieval_hit_ranks): bit 0 = a distance was no finite
 *   number (a NaN or inf feature, or an overflow of the squared distance in f32); bit 1 = seg_start is not a non-decreasing
 *   sequence from 0 to N -- checked on the device before any use, and then nothing is computed and out_sorted is left as it was.
 *   Refused on the host (-1, bsclip_last_error): null pointers, N < 3, C < 2 or C > N - 1, D < 1, ld < D or ld % 4 != 0, a
 *   misaligned pointer. */
int bsclip_silhouette_samples(const float* x_sorted, int ld, int N, int D, const int32_t* seg_start, int C, float* out_sorted,
                              int32_t* flag, void* stream);

/* ---- RCCL collectives of the global-batch step ---------------------------------------------------
 * One process per GPU.  bsclip_comm_unique_id on rank 0 -> the caller ships the bsclip_comm_unique_id_bytes() bytes to the
 * other ranks (any channel) -> bsclip_comm_init on every rank (ncclCommInitRank).  The collectives run on `comm_stream`;
 * `wait_event` (hipEvent_t as void*, nullable) is waited for on that stream first -- record it on the stream that produced
 * the payload -- and `done_event` (nullable) is recorded behind the collective for the consumer to wait on.  No host sync.
 *   allgather_embeddings: gather_features (bioscanclip/model/loss_func.py:58-91, :84-89): local f32 [count] (= B*D) ->
 *     gathered f32 [world*count], rank-major = row-major [world*B, D]; remote rows carry no gradient.
 *   allgather_labels: the label all-gather of ClipLoss (loss_func.py:122), int64.
 *   allreduce_grads: SUM over ranks of a flat f32 trainable-gradient buffer, in place (the gradient synchronisation
 *     scripts/train_cl.py lacks).
 * RCCL is bound with dlopen at first use; every call fails with a message when it cannot be found. */
int bsclip_comm_unique_id_bytes(void);
int bsclip_comm_unique_id(void* id_out);
int bsclip_comm_init(void** comm_out, const void* unique_id, int rank, int world);
int bsclip_comm_destroy(void* comm);
int bsclip_allgather_embeddings(void* comm, const float* local, float* gathered, int64_t count, void* comm_stream,
                                void* wait_event, void* done_event);
int bsclip_allgather_labels(void* comm, const int64_t* local, int64_t* gathered, int64_t count, void* comm_stream,
                            void* wait_event, void* done_event);
int bsclip_allreduce_grads(void* comm, float* grads, int64_t count, void* comm_stream, void* wait_event, void* done_event);

/* ---- input pipeline --------------------------------------------------------------------------------
 * kmer_tokenize: get_sequence_pipeline(k) (bioscanclip/model/dna_encoder.py:25-35; PadSequence / KmerTokenizer,
 *   bioscanclip/util/util.py:48-69).  seqs: the batch's nucleotide bytes back to back, offsets int64 [B+1]; each sequence is
 *   truncated to max_len or right-padded with 'N', cut into max_len/k non-overlapping k-mers, id = 3 + base-4 value over
 *   A,C,G,T (any other byte in the k-mer -> 2 = <UNK>), and a literal 0 (<MASK>) is put in front: ids int64 [B, max_len/k + 1].
 * augment_images: the image transforms of Dataset_for_CL (bioscanclip/util/dataset.py:171-200) for B decoded uint8 HWC images
 *   stored back to back in src_u8.  records int32 [B, 16] per image: {src offset lo, hi, H0, W0, H1, W1 (size after
 *   Resize(256)), crop top, left, height, width (in the resized image), hflip, vflip, rotate flag, cos(angle), sin(angle) as
 *   f32 bits, 0}.  mid: f32 scratch [B, 3, mid_capacity] (mid_capacity >= max H1*W1); out: f32 [B, 3, out_size, out_size].
 *   Arithmetic: ToTensor, antialiased bilinear resize (torch _upsample_bilinear2d_aa) twice, flips, nearest-neighbour
 *   rotation with zeros outside (torchvision functional_tensor.rotate).  The random draws are the caller's. */
int bsclip_kmer_tokenize(const void* seqs, const int64_t* offsets, int B, int max_len, int k, int64_t* ids, void* stream);
int bsclip_augment_images(const void* src_u8, const int32_t* records, int B, int64_t mid_capacity, float* mid, int out_size,
                          float* out, void* stream);

/* ---- JPEG shards: entropy decode on the host, pixels on the GPU -----------------------------------------
 * The reference stores JPEG bytes in its HDF5 file and decodes one per __getitem__ (bioscanclip/util/dataset.py:220-223,
 * Image.open(io.BytesIO(...)).convert("RGB")).  Here the serial part (markers + Huffman decoding) runs on loader threads and the
 * arithmetic (dequantise, 8x8 inverse DCT, chroma upsampling, YCbCr -> RGB; libjpeg's integer defaults) runs on the device.
 * Decoded: baseline SOF0, 8-bit, grey or YCbCr with luma sampling 1 or 2 per axis and chroma 1x1, one scan, restart intervals,
 * up to 4096 x 4096.  Anything else is refused with one of the codes below (never decoded in part); a truncated or corrupt
 * entropy stream is an error too (nothing is zero-filled).
 * jpeg_probe and jpeg_entropy_decode are HOST functions (host pointers, no device call, no allocation, no globals: callable
 *   from any number of threads at once; the error text is the calling thread's, like every bsclip_last_error).
 *   entropy_decode writes coef_out (int16, natural order, 64 per block; per component a block raster padded to whole MCUs:
 *   info.coef_count elements), qtab_out (uint16 [3][64], one table per component) and record_out (int32 [16]):
 *     {coef offset lo, hi (int16 elements, a multiple of 64), out offset lo, hi (bytes), W, H, components, luma h, luma v,
 *      table slot of component 0, 1, 2, blocks (= coefficients / 64), restart interval, 0, 0}
 *   with both offsets zero and slots 0, 1, 2: the caller places the image in its batch by setting them.
 * jpeg_pixels: B images in one launch sequence.  coef_dev int16 [coef_count], qtab_dev uint16 [qtab_slots][64], scratch
 *   >= bsclip_jpeg_pixels_workspace_bytes(coef_count) bytes, out_u8 [out_capacity]: image b's H x W x 3 bytes at its out offset.
 *   records_host: the B records in HOST memory (pinned for a copy that does not stall; they must stay unchanged until the stream
 *   has passed this call).  They are validated before anything is launched (sizes against the block count, every range against
 *   coef_count / out_capacity / qtab_slots); then the library copies them to records_dev (device int32 [B][16], the caller's
 *   scratch) on `stream` itself, so the kernels read exactly what was checked -- the one entry point that reads host memory.
 *   coef_dev, qtab_dev, scratch, out_u8 16-byte aligned.  Images must not overlap (not checked). */
#define BSCLIP_JPEG_ERR_TRUNCATED (-10)
#define BSCLIP_JPEG_ERR_CORRUPT (-11)
#define BSCLIP_JPEG_ERR_SOF (-12)           /* extended / progressive / lossless / arithmetic / 12-bit */
#define BSCLIP_JPEG_ERR_COMPONENTS (-13)    /* not 1 or 3 */
#define BSCLIP_JPEG_ERR_SAMPLING (-14)
#define BSCLIP_JPEG_ERR_MULTISCAN (-15)
#define BSCLIP_JPEG_ERR_MISSING_TABLE (-16)
#define BSCLIP_JPEG_ERR_SIZE (-17)
#define BSCLIP_JPEG_ERR_COLORSPACE (-18)    /* three components that are RGB */
typedef struct bsclip_jpeg_info {
    int32_t width, height, components, h_samp, v_samp, restart_interval;
    int64_t coef_count;   /* int16 coefficients = bytes of scratch */
    int64_t pixel_bytes;  /* width * height * 3 */
} bsclip_jpeg_info;
int bsclip_jpeg_probe(const void* host_bytes, int64_t n, bsclip_jpeg_info* info_out);
int bsclip_jpeg_entropy_decode(const void* host_bytes, int64_t n, int16_t* host_coef_out, int64_t coef_capacity,
                               uint16_t* host_qtab_out, int32_t* host_record_out);
int64_t bsclip_jpeg_pixels_workspace_bytes(int64_t coef_count);
int bsclip_jpeg_pixels(const int16_t* coef_dev, int64_t coef_count, const uint16_t* qtab_dev, int qtab_slots,
                       const int32_t* records_host, int32_t* records_dev, int B, void* scratch, int64_t scratch_bytes,
                       void* out_u8, int64_t out_capacity, void* stream);

/* ---- JPEG shards, entropy decode on the device (opt-in, the host decoder above stays the default) ------------
 * Huffman decoding is serial only while nobody knows where a code starts.  A SYNC INDEX, made once on the host when a shard is
 * written, cuts a scan into segments that decode independently: one entry at MCU 0, one at the first MCU of every restart
 * interval, and one every sync_mcus MCUs counted from the start of the current restart interval.  No segment crosses a restart
 * marker.  Which MCUs segment j covers, and how many segments there are, follows from the frame, the restart interval and
 * sync_mcus alone; a segment ends where the next begins, the last at the MCU count.
 * Index entry, int32[4]:
 *     [0] position of the segment's first entropy-coded bit, 8 * byte + bit from the start of the stream (bit 0 = the byte's most
 *         significant); the byte is always a data byte, never a stuffed 0x00 and never a marker
 *     [1] index of the segment's first MCU
 *     [2] DC predictor of Y at that point
 *     [3] DC predictors of Cb (low 16 bits) and Cr (high 16 bits), both two's-complement int16; 0 for a grey image
 * jpeg_sync_index (HOST: no device call, no allocation, no globals, thread-safe, its own error text): walks the scan with the
 *   segment decoder and writes the entries.  index_out == NULL: returns the entry count.  Otherwise returns the count written
 *   (<= capacity entries) or a negative code: the entropy decoder's own for whatever that refuses, BSCLIP_ERR_INVALID for a stream
 *   of 2^28 bytes or more, sync_mcus < 1 or a short buffer, BSCLIP_JPEG_ERR_CORRUPT for data bytes between the last MCU of a
 *   restart interval (or of the scan) and its marker, BSCLIP_JPEG_ERR_SOF for a scan that selects more than two DC or two AC tables.
 * jpeg_device_tables (HOST, same properties): parses a stream's headers once and writes what the device needs:
 *   huff_out  4 tables of BSCLIP_JPEG_HUFF_BYTES each (DC slot 0, DC slot 1, AC slot 0, AC slot 1; 4-byte aligned): the 9-bit
 *             look-up, the per-length largest codes and symbol offsets and the symbols, expanded here on the host
 *   qtab_out, record_out  as bsclip_jpeg_entropy_decode writes them, and record word 14 = the selector word: bit c = DC slot of
 *             component c, bit 4 + c = its AC slot (word 13, the restart interval, now matters too).
 * jpeg_entropy_device: the coefficients of B images, written exactly as bsclip_jpeg_entropy_decode writes them, one lane per
 *   segment.  bytes_dev: the streams, anywhere in [0, bytes_capacity < 2^31); sync_dev: int32 [sync_entries][4]; huff_dev:
 *   huff_slots groups of 4 tables; coef_dev int16 [coef_count].  records_host: the B 16-int records (coefficient offset, sizes,
 *   restart interval, selector word); segments_host int32 [B][8]:
 *     {byte offset, byte length (< 2^28), first index entry, index entries, sync_mcus, table-group slot, 0, 0}.
 *   Both stay in HOST memory and are validated before anything is launched (sizes against the block count, the entry count against
 *   frame, restart interval and sync_mcus, every range against bytes_capacity / sync_entries / huff_slots / coef_count); then the
 *   library copies them to records_dev [B][16] / segments_dev [B][8] (device scratch) and zeroes status_dev (int32 [B]) on
 *   `stream` itself.  After the launch every element of each image's coefficient range is defined, and status_dev[b] is 0 or an
 *   or of the BSCLIP_JPEG_SEG_* bits: the image's bytes or index are damaged and its coefficients must not be used.
 *   sync_dev, coef_dev 16-byte aligned; the others 4-byte.  Images must not overlap (not checked). */
#define BSCLIP_JPEG_HUFF_BYTES 1420
#define BSCLIP_JPEG_SEG_BAD_CODE 1    /* a code no table assigns */
#define BSCLIP_JPEG_SEG_BAD_RUN 2     /* a zero run that leaves its block */
#define BSCLIP_JPEG_SEG_OVERRUN 4     /* bits consumed past the byte range or a marker */
#define BSCLIP_JPEG_SEG_END_POS 8     /* a segment did not end where the next one starts */
#define BSCLIP_JPEG_SEG_END_PRED 16   /* DC predictors at a segment's end differ from the next entry's */
#define BSCLIP_JPEG_SEG_BAD_ENTRY 32  /* an entry's first MCU or bit position is not its segment's */
int64_t bsclip_jpeg_sync_index(const void* host_bytes, int64_t n, int sync_mcus, int32_t* host_index_out, int64_t capacity);
int bsclip_jpeg_device_tables(const void* host_bytes, int64_t n, void* host_huff_out, uint16_t* host_qtab_out,
                              int32_t* host_record_out);
int bsclip_jpeg_entropy_device(const void* bytes_dev, int64_t bytes_capacity, const int32_t* sync_dev, int64_t sync_entries,
                               const void* huff_dev, int huff_slots, const int32_t* records_host, const int32_t* segments_host,
                               int32_t* records_dev, int32_t* segments_dev, int B, int16_t* coef_dev, int64_t coef_count,
                               int32_t* status_dev, void* stream);

/* ---- LoRA / head gradients -------------------------------------------------------------------------------------
 * lora_grad: for one layer, from dqkv (bf16 [M, ld_dqkv], q cols [0,H), v cols [2H,3H)) and the augmented LN
 *   output h (bf16 [M, ld_h]: cols [0,H) = y, [H,H+4) = t_q, [H+4,H+8) = t_v):
 *     dt[M,8]   = [dq . B_q | dv . B_v]                     (f32 out, feeds layernorm_bwd)
 *     dA[8,H]  += dt^T h[:, :H]        (rows 0-3 = dA_q, 4-7 = dA_v)      (f32 accumulate)
 *     dBq[H,4] += dq^T t_q ; dBv[H,4] += dv^T t_v                         (f32 accumulate)
 *   lora_b f32 [2, H, 4] = (B_q, B_v).  Autograd of image_encoder.py:44-47 / dna_encoder.py:47-49.
 *   workspace: f32, bsclip_lora_grad_workspace_floats(H) elements (per-workgroup partial slabs; the final sum runs in a
 *   fixed order, so results are bitwise reproducible -- no float atomics).
 * colsum: db[N] += sum_m g[m, n] (bias gradients of the trainable heads), g bf16 or f32.
 * transpose_bf16: out[C,R] = in[R,C]^T (operands of the dW = dY^T X head GEMMs). */
int64_t bsclip_lora_grad_workspace_floats(int H);
int bsclip_lora_grad(const void* dqkv, int ld_dqkv, const void* h, int ld_h, int M, int H, const float* lora_b,
                     float* dt, float* dA, float* dBq, float* dBv, float* workspace, void* stream);
/* lora_grad from the partial sums of bsclip_attn_bwd_lora (B sequences, M = B*S tokens, heads = H / 64): dt[M,8] = sum over heads of
 * dt_partial, dBq / dBv += sum over sequences of db_partial, then dA += dt^T h[:, :H] as bsclip_lora_grad.  Same workspace; fixed
 * summation order (bitwise reproducible). */
int bsclip_lora_grad_heads(const void* h, int ld_h, int M, int H, int B, const float* dt_partial, const float* db_partial, float* dt,
                           float* dA, float* dBq, float* dBv, float* workspace, void* stream);
/* the same on fp16 operands with the static gradient scale 2^s (operands = BSCLIP_OPERANDS_FP16 | s; see BSCLIP_OPERANDS_FP16): h fp16
 * [M, ld_h], H = 768; dt stays in 2^s units, dA / dBq / dBv receive the true gradient.  h, dt_partial, dt, workspace 16-byte aligned. */
int bsclip_lora_grad_heads_f16(const void* h, int ld_h, int M, int H, int B, const float* dt_partial, const float* db_partial,
                               float* dt, float* dA, float* dBq, float* dBv, float* workspace, int operands, void* stream);
/* out[i] += 2^scale_log2 in[i], f32, |scale_log2| <= 64, 16-byte aligned (exact: a weight gradient formed from 2^s-scaled operands) */
int bsclip_add_scaled_f32(const float* in, int64_t n, int scale_log2, float* out, void* stream);
/* lora_grad with the fp8 operand layout: y_fp8 [M, ld_y bytes] (LN output, e4m3) and t_aug bf16 [M, ld_t] (t in cols [0,8)) */
int bsclip_lora_grad_fp8(const void* dqkv, int ld_dqkv, const void* y_fp8, int ld_y, const void* t_aug, int ld_t, int M,
                         int H, const float* lora_b, float* dt, float* dA, float* dBq, float* dBv, float* workspace,
                         void* stream);
int bsclip_colsum(const void* g, int ld_g, int g_is_bf16, int M, int N, float* out, void* stream);
int bsclip_transpose_bf16(const void* in, int ld_in, int R, int C, void* out, int ld_out, void* stream);
/* the same transpose, and colsum[c] += sum_r in[r, c] from the tiles while they are in registers (ordered sums): with in = dY
 * this is the operand of the weight-gradient GEMM and the bias gradient of a Linear in one pass over dY (full fine-tuning,
 * simple_clip.py:199-201).  workspace: bsclip_transpose_colsum_workspace_floats(R, C) floats; 16-byte aligned operands, ld % 8 == 0. */
int64_t bsclip_transpose_colsum_workspace_floats(int R, int C);
int bsclip_transpose_colsum_bf16(const void* in, int ld_in, int R, int C, void* out, int ld_out, float* colsum,
                                 float* workspace, void* stream);
int bsclip_cast_f32_bf16(const float* in, int64_t n, void* out, void* stream);
/* out fp16 [n] = in f32 [n]: round to nearest even, subnormals kept, overflow to +-inf (the head weight of an fp16-operand forward) */
int bsclip_cast_f32_f16(const float* in, int64_t n, void* out, void* stream);
/* out fp16 [n] = RNE(in [n] * 2^scale_log2), |scale_log2| <= 64, 16-byte aligned: the scaled dout of an fp16-operand backward */
int bsclip_cast_f32_f16_scaled(const float* in, int64_t n, int scale_log2, void* out, void* stream);
/* W_aug[3H, H+KPAD] bf16: cols [H,H+4) of rows [0,H) = B_q, cols [H+4,H+8) of rows [2H,3H) = B_v (refreshed
 * every step from the f32 masters; the frozen [3H,H] block is written once at pack time).
 * One launch for every LoRA layer of an encoder: table_dev[l] = {W_aug, B_q, B_v} as three 64-bit device addresses (the buffers live
 * as long as the encoder: the table is built once); all layers share ld_w and H.  (ABI 9: the one-layer form bsclip_waug_set_lora is
 * gone -- no engine called it.) */
int bsclip_waug_set_lora_layers(const int64_t* table_dev, int layers, int ld_w, int H, void* stream);

/* ---- full fine-tuning only (reference simple_clip.py:199-201 unfreezes every parameter) ----------------
 * ln_param_grad: d_gamma[c] += sum_r dy[r,c] xhat[r,c], d_beta[c] += sum_r dy[r,c] with dy assembled like
 *   bsclip_layernorm_bwd does (g_gemm bf16 + dt.lora_a + (mode 1: g_resid)), optionally masked by the dropout the LN's
 *   OUTPUT was subjected to in forward (BertEmbeddings).  workspace: bsclip_ln_param_grad_workspace_floats(H) floats.
 * embed_grad: autograd of HF BertEmbeddings' three lookups from d_emb f32 [B*S, H] (gradient at the input of its LayerNorm):
 *   d_pos[s] += sum_b (ordered), d_word[id] += rows in token order (one workgroup per vocabulary row scans the ids), d_type[tt] +=
 *   rows through ordered slabs -- no atomics; rows with id == pad_id get none (HF: nn.Embedding(padding_idx = config.pad_token_id
 *   = 0); pass -1 for "no padding row").  workspace: bsclip_embed_grad_workspace_floats(H) floats.
 * gather_cast_rows: dst bf16 [rows_out, H], dst[r] = src[(r / period_out) * period_in + offset + r % period_out] (f32): e.g. the
 *   196 patch rows of each image out of the 197-row residual gradient -> operand of the patch-embedding dW GEMM. */
int64_t bsclip_ln_param_grad_workspace_floats(int H);
int bsclip_ln_param_grad(const void* x, int ld_x, int x_bf16, const float* stats, int M, int H, const float* g_resid,
                         int ld_gr, const void* g_gemm, int ld_g, const float* dt, const float* lora_a, int mode,
                         float in_dropout_p, uint32_t in_dropout_seed, float* d_gamma, float* d_beta, float* workspace,
                         void* stream);
int64_t bsclip_embed_grad_workspace_floats(int H);
int bsclip_embed_grad(const int64_t* ids, const int64_t* type_ids, int B, int S, int H, int vocab, int pad_id,
                      const float* d_emb, float* d_word, float* d_pos, float* d_type, float* workspace, void* stream);
int bsclip_gather_cast_rows(const float* src, int ld_src, int rows_out, int period_in, int period_out, int offset, int H,
                            void* dst_bf16, int ld_dst, void* stream);
/* C[M, N] (f32) += A[M, K] . B[N, K]^T with the reduction cut into `splits` equal K ranges that run as separate workgroups
 * (the weight gradient dW = dY^T X of a Linear, simple_clip.py:199-201: a 768 x 3072 output reduced over 50 432 tokens would
 * otherwise occupy 36 of 256 CUs).  partial: f32 scratch of splits * M * N elements; the ranges are summed in a fixed order
 * (no atomics).  N % 256 == 0, K % (64 * splits) == 0; operands bf16 row-major, 16-byte aligned. */
int bsclip_gemm_splitk_f32(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K, int splits,
                           float* partial, void* stream);

/* ---- optimiser: torch.optim.AdamW defaults (scripts/train_cl.py:158), one launch over a flat f32 buffer ---------- */
int bsclip_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, float grad_scale, void* stream);
/* the same update with the two per-step quantities read from device memory when the kernel runs: hyper_dev[0] = lr (f32),
 * hyper_dev[1] = step count as a uint32 word (advance it with bsclip_counter_add, a capturable launch) -- the form a captured
 * hipGraph replays with a moving LR schedule; neither word is ever read from host memory by an in-flight node */
int bsclip_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, float beta1,
                          float beta2, float eps, float weight_decay, float grad_scale, void* stream);

/* ---- global gradient norm, clipping (torch.nn.utils.clip_grad_norm_) and overflow-safe steps (GradScaler.step), all on the device
 * and capturable.  Per optimizer step: one bsclip_grad_sumsq_partial per flat gradient buffer into consecutive slices
 * of one partials buffer, one bsclip_grad_clip_finish over all of them, then per buffer bsclip_counter_add_if on the step word and
 * bsclip_adamw_step_clip.
 * grad_norm_partials: how many partial sums grad_sumsq_partial writes for n floats: a pure function of n, >= 1, monotone, capped
 *   (-1 for n <= 0).
 * grad_sumsq_partial: partial[b] = sum of g[i]^2 over the elements workgroup b owns, squared and summed in f64 (the square of an f32
 *   is exact there, and a large finite gradient stays finite), in a fixed order without atomics: a repeated call gives the same bits.
 *   g 16-byte aligned, n arbitrary.
 * grad_clip_finish (one workgroup): total = partial[0] + ... + partial[n_partial - 1] in index order (f64); finite = isfinite(total)
 *   -- an Inf or NaN anywhere makes it false; norm = (float)sqrt(total); coef = finite ? (float)min(1, max_norm / (sqrt(total) + 1e-6))
 *   : 0 (torch's clip_coef_clamped).  max_norm = +inf: coef is exactly 1 (monitoring and skipping only); max_norm <= 0 or NaN is
 *   refused.  state: caller-owned, 16-byte aligned, twelve 4-byte words, zeroed once by the caller:
 *     0 apply (uint32: 1 = finite, 0 = skip)   1 coef (f32)   2 norm (f32; the non-finite value itself when skipped)
 *     3 clipped this step (uint32: finite and coef < 1)   4 steps seen   5 steps skipped   6 steps clipped (uint32, running)   7 zero
 *     8-9 f64 running sum of the finite steps' norms   10-11 f64 largest finite norm
 * counter_add_if: *counter += inc when *cond != 0 (bsclip_counter_add's conditional form: AdamW's step word counts applied steps).
 * adamw_step_clip: bsclip_adamw_step_dev's arithmetic with the gradient multiplied by state's coef; returns without a store when
 *   state's apply is 0.  With coef == 1 it leaves the bits bsclip_adamw_step_dev(..., grad_scale = 1) leaves. */
int64_t bsclip_grad_norm_partials(int64_t n);
int bsclip_grad_sumsq_partial(const float* g, int64_t n, double* partial, void* stream);
int bsclip_grad_clip_finish(const double* partial, int64_t n_partial, float max_norm, void* state, void* stream);
int bsclip_counter_add_if(uint32_t* counter, uint32_t inc, const uint32_t* cond, void* stream);
int bsclip_adamw_step_clip(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, const void* state,
                           float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- exponential moving average of the weights inside the AdamW update (timm ModelEmaV2 / V3), capturable.
 * adamw_step_ema: with clip_state == NULL bsclip_adamw_step_dev's arithmetic with grad_scale = 1, otherwise bsclip_adamw_step_clip's on
 *   that record (gradient times coef; no store at all, ema included, when the record's apply is 0); p, m, v receive the bits those
 *   entry points leave.  The thread that stored the new p[i] then does ema[i] += w * (p[i] - ema[i]) (torch's lerp_(p, w)), one f32 w
 *   per launch formed in f64 on the device: t = hyper_dev[1] (the uint32 step word: applied steps, this one included),
 *   d_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay, w = (float)(1 - d_t).  0 < ema_decay < 1; ema [n] f32 shares
 *   no byte with p, g, m, v; clip_state 16-byte aligned.  Same grid as the other AdamW entry points.
 * swap_f32: a[i] <-> b[i] for i < n (evaluating the averaged weights in place, then putting the raw ones back); a and b must not be
 *   the same or overlapping ranges. */
int bsclip_adamw_step_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* hyper_dev,
                          const void* clip_state, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                          int ema_warmup, void* stream);
int bsclip_swap_f32(float* a, float* b, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
