/*
 * qfx.h -- C ABI of libqfx.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * LoRA-training hot path of the Qwen-Image-Edit / FLUX-Kontext DiT.
 *
 * The reference (tsiendragon/qwen-image-finetune) has no native code and no FFI: its hot path is
 * Python calling torch/diffusers/peft ops.  Each entry point below names the
 * reference call sites whose device work it replaces (file:line relative to /root/reference).
 * Callers are the torch.autograd.Function wrappers in qwen-image-finetune_amd/qflux_amd/ops.py.
 *
 * Conventions
 *   - extern "C", plain device pointers + explicit sizes/strides (in ELEMENTS unless stated).
 *   - bf16 tensors are passed as `const uint16_t*` (raw bits), fp32 as `const float*`.
 *   - caller allocates every output and workspace; kernels are launched on `stream`
 *     (a hipStream_t passed as void*); no global state; thread-safe for distinct streams.
 *   - return 0 on success, a negative QFX_E* code on a rejected argument; HIP launch errors are
 *     returned as -(1000 + hipError_t).  No exceptions cross the ABI.
 */
#ifndef QFX_H
#define QFX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QFX_ABI_VERSION 7

#define QFX_OK 0
#define QFX_EINVAL (-1)   /* bad shape / alignment / null pointer */
#define QFX_EUNSUPPORTED (-2)

/* ---- GEMM with fused LoRA / epilogues ------------------------------------------------------
 * C[M,N] = A1[M,K1] * B1[N,K1]^T (+ A2[M,K2] * B2[N,K2]^T) (+ bias[N]) , then epilogue.
 * Replaces: nn.Linear + peft lora.Linear side branch + following elementwise ops
 *   (src/qflux/models/transformer_qwenimage.py:286-293,348,352 ; FeedForward at :479,485 ;
 *    gated residuals at :473-474,480,486 ; LoRA call site src/qflux/trainer/base_trainer.py:929-941)
 * and, with transposed weights, the dX GEMMs autograd runs for them.
 * K1, K2 multiples of 64; all row strides multiples of 8 elements; pointers 16-byte aligned.
 * Rounding points follow the reference's bf16 eager graph: if K2>0 the accumulator is rounded to
 * bf16 after (A1*B1^T + bias) -- the base nn.Linear output -- before the LoRA segment is added.
 */
enum {
  QFX_EPI_NONE = 0,      /* C = bf16(acc) */
  QFX_EPI_GELU = 1,      /* C = bf16(acc) (pre-activation), C2 = bf16(gelu_tanh(C)) */
  QFX_EPI_GATE_RES = 2,  /* C = bf16(aux + bf16(gate[b] * bf16(acc)))  (x + gate*y); if C2 != NULL also C2[m] = bf16(acc) (pre-gate y, rows unmapped, for d(gate)) */
  QFX_EPI_DGELU = 3      /* C = bf16(bf16(acc) * gelu_tanh'(aux))      (backward through GELU) */
};

typedef struct qfx_gemm_args {
  const uint16_t* A1; const uint16_t* B1; int64_t lda1; int64_t ldb1; int32_t K1;
  const uint16_t* A2; const uint16_t* B2; int64_t lda2; int64_t ldb2; int32_t K2;
  int32_t M; int32_t N;
  const uint16_t* bias;            /* [N] bf16 or NULL */
  uint16_t* C; int64_t ldc;
  uint16_t* C2; int64_t ldc2;      /* EPI_GELU second output */
  const uint16_t* aux; int64_t ldaux;   /* residual (GATE_RES) / pre-activation (DGELU); indexed like C */
  const uint16_t* gate; int64_t gate_bstride; /* gate[b*gate_bstride + n], b = m / rows_per_batch */
  int32_t rows_per_batch;          /* rows of A per batch sample (M if unused) */
  /* row remaps (joint [text|image] buffers): row(m) = (m / rows_per_batch) * X_batch_rows + X_row_off + m % rows_per_batch */
  int32_t a_batch_rows; int32_t a_row_off;   /* applied to A1 rows; a_batch_rows==0 => identity */
  int32_t c_batch_rows; int32_t c_row_off;   /* applied to C/C2/aux rows; c_batch_rows==0 => identity */
  int32_t epi;
  const float* row_mask;           /* optional [M] (compact row m): rows with mask 0 are written as exact zeros (multi-resolution
                                      padding, transformer_flux_custom.py:427-442,648-660,724-733); NULL = no masking */
  int32_t aux_unmapped;            /* 1: aux rows are indexed by m (compact) even when C uses the c_* row remap */
  int32_t seg2_plain;              /* 1: the second K segment is an ordinary continuation of the contraction (FLUX single block:
                                      [attn | mlp] @ W_out as two segments) -- no bf16 mid-rounding, bias added at the end */
} qfx_gemm_args;

int qfx_gemm_bf16(const qfx_gemm_args* args, void* stream);

/* Grouped launch: n <= QFX_MAX_GROUPS independent problems with the same epilogue kind in ONE grid
 * (image + text stream, q/k/v projections): the small text-stream GEMMs share the machine with the
 * image-stream ones instead of running latency-bound on a few dozen tiles. `groups` is a HOST array. */
#define QFX_MAX_GROUPS 6
int qfx_gemm_grouped(const qfx_gemm_args* groups, int32_t n, void* stream);

/* ---- low-precision trunk: MX-FP8 base GEMM (reference: src/qflux/models/quantize.py -- TE fp8 / bnb int8 / NF4 --
 * whose MI355X analogue is the block-scaled FP8 MFMA, v_mfma_scale_f32_16x16x128_f8f6f4, at twice the bf16 matrix rate).
 * OCP MX format: elements fp8 e4m3 (OCP e4m3fn), one shared E8M0 scale per 32 consecutive K elements,
 *   scale exponent = floor(log2(max|v|)) - 8 (e4m3 emax), elements = RNE(v / 2^e) saturated to +-448.
 * qfx_quant_mxfp8: X[M,K] bf16 (row stride ldx, optional joint-buffer row remap) -> Q[M,K] fp8 bytes (row stride ldq) and the
 *   E8M0 scale bytes S in TILE-MAJOR order [K/128][M][4]: the scale of row m, 32-element block kb sits at byte
 *   ((kb/4)*M + m)*4 + kb%4, so that the 16 rows of an MFMA fragment read one contiguous 64-byte line per K tile.  K % 128 == 0.
 *   (`lds` / `ldsa` / `ldsb` are unused, kept for ABI stability.)
 * qfx_gemm_mxfp8: same contract as qfx_gemm_bf16 (bias, bf16 mid-rounding of the base output, bf16 LoRA K-extension segment
 *   A2/B2, all four epilogues, row maps of C / aux) except that A1 / B1 are MX-FP8: g.A1 / g.B1 point at fp8 BYTES, lda1 / ldb1
 *   are byte strides, K1 % 128 == 0, A1 rows are NOT remapped; sa / sb are the tile-major scale arrays of A1 ([K1/128][M][4]) and
 *   B1 ([K1/128][N][4]).
 *   The product of two e4m3 values and a power-of-two scale is exact in fp32; accumulation is fp32 as in the bf16 kernel. */
typedef struct qfx_quant_args {
  const uint16_t* X; int64_t ldx; int32_t M; int32_t K;
  uint8_t* Q; int64_t ldq; uint8_t* S; int64_t lds;
  int32_t rows_per_batch; int32_t x_batch_rows; int32_t x_row_off;
} qfx_quant_args;
int qfx_quant_mxfp8(const qfx_quant_args* a, void* stream);
typedef struct qfx_gemm_fp8_args {
  qfx_gemm_args g;
  const uint8_t* sa; int64_t ldsa;
  const uint8_t* sb; int64_t ldsb;
  /* ABI 2: quantising epilogue (persistent kernel only: problems of >= 160 256x128 tiles, N % 128 == 0, not GATE_RES).  When
   * cq != NULL the output the NEXT GEMM contracts over -- C2 = gelu(h) for EPI_GELU, C otherwise -- also leaves the epilogue as
   * MX-FP8: bytes at cq + row*ldcq + n (rows indexed like C), E8M0 scales tile-major in cs ([N/128][cq_rows][4], cq_rows >= the
   * row extent of C); bit-identical to qfx_quant_mxfp8 of the bf16 tensor.  cq_only != 0: the bf16 copy of that output is not
   * written at all (the consumer is an MX-FP8 GEMM and nothing else reads it). */
  uint8_t* cq; uint8_t* cs; int64_t ldcq; int32_t cq_rows; int32_t cq_only;
} qfx_gemm_fp8_args;
int qfx_gemm_mxfp8(const qfx_gemm_fp8_args* a, void* stream);
/* n <= QFX_MAX_GROUPS problems with the same epilogue in ONE persistent grid (image + text stream, q/k/v), as qfx_gemm_grouped;
 * no seg2_plain.  qfx_gemm_mxfp8 routes large single problems here and keeps the 128x128 kernel for small ones. */
int qfx_gemm_mxfp8_grouped(const qfx_gemm_fp8_args* list, int32_t n, void* stream);

/* ---- LoRA rank-r down projection ("skinny" GEMM, HBM-bound) ----------------------------------
 * U[M,R] (fp32) = X[M,K] (bf16) * (W_hi + W_lo)[R,K]^T   (W = fp32 LoRA weight split in two bf16)
 * and its packed bf16 image EXT[M, 3R] = [U_hi | U_lo | U_hi] written at ext + m*ld_ext
 * (consumed as the A2 operand of qfx_gemm_bf16 against B2 = [V_hi | V_hi | V_lo]).
 * Replaces peft lora_A(x.float()) forward and the dY*B product of its backward. R in {16,32,48,64,96}.
 */
typedef struct qfx_lora_down_args {
  const uint16_t* X; int64_t ldx; int32_t M; int32_t K;
  const uint16_t* W_hi; const uint16_t* W_lo; int64_t ldw; int32_t R;
  float* U; int64_t ldu;                 /* may be NULL */
  uint16_t* ext; int64_t ld_ext;         /* may be NULL */
  uint16_t* Ut_hi; uint16_t* Ut_lo; int64_t ld_ut; /* may be NULL: transposed split image Ut[R][ld_ut] (column = row index m),
                                            the V operand of qfx_lora_grad; columns >= M must be pre-zeroed by the caller */
  int32_t group_R; int32_t group_stride; /* ext column of U column j: (j/group_R)*group_stride + j%group_R + {0,group_R,2*group_R}
                                            (several LoRA targets sharing X are fused in one call; group_R = R for one) */
  int32_t rows_per_batch; int32_t x_batch_rows; int32_t x_row_off; /* X row remap as in gemm */
  /* ABI 2, MX-FP8 trunk: xq != NULL -- the kernel reads every element of X anyway; it also writes X's MX-FP8 image for the GEMM that
   * contracts over it: bytes at xq + m*ldxq + k (m = compact row), E8M0 scales tile-major as qfx_quant_mxfp8 writes them, the
   * 32-column block ks of this call being block xq_kb0 + ks of an operand with xs_rows rows (several calls fill the column
   * sections of one operand: q / k / v sections of dqkv).  K % 128 == 0, xq_kb0 % 4 == 0. */
  uint8_t* xq; uint8_t* xs; int64_t ldxq; int32_t xs_rows; int32_t xq_kb0;
} qfx_lora_down_args;

int qfx_lora_down(const qfx_lora_down_args* args, void* stream);

/* ABI 6: second half of a down projection fused into an attention epilogue (qfx_head_lora): U[m, j] = sum_h part[h][row(m)][j] in
 * head order (deterministic), then exactly qfx_lora_down's outputs -- EXT[m, ...] = [U_hi | U_lo | U_hi] per group and the transposed
 * split image Ut -- for the M compact rows of one stream (row(m) = the joint row, X-remap fields as in qfx_lora_down).  R = total
 * columns (e.g. 3 * Rp for q | k | v with group_R = Rp).  Up to 2 problems (image + text stream) per launch. */
typedef struct qfx_lora_head_reduce_args {
  const float* part; int64_t part_hstride; int32_t ld_part; int32_t H;
  int32_t M; int32_t R;
  uint16_t* ext; int64_t ld_ext;
  uint16_t* Ut_hi; uint16_t* Ut_lo; int64_t ld_ut;
  int32_t group_R; int32_t group_stride;
  int32_t rows_per_batch; int32_t x_batch_rows; int32_t x_row_off; int32_t reserved;
} qfx_lora_head_reduce_args;
int qfx_lora_head_reduce(const qfx_lora_head_reduce_args* list, int32_t n, void* stream);
/* n <= QFX_MAX_BATCH independent problems of the same R in ONE launch (e.g. the q, k and v down projections of a block's
 * backward): every separate launch of these one-round-trip kernels costs a dispatch gap plus its own latency floor. */
#define QFX_MAX_BATCH 8
int qfx_lora_down_batch(const qfx_lora_down_args* list, int32_t n, void* stream);

/* ---- LoRA weight gradients (contraction over tokens, MFMA + LDS transpose reads) -------------
 * G[j,k] += out_scale * sum_m (Vt_hi+Vt_lo)[j,m] * X[m,k]   j<R, k<K ; Vt = transposed bf16 split of the fp32
 * rank-r activations written by qfx_lora_down (rows zero-padded to a multiple of 32 tokens), X bf16 [M,K];
 * G fp32, atomically accumulated at G[j*g_sr + k*g_sc] (dA [r,K] uses (K,1), dB [N,r] uses (1,r)).
 * Up to three fused targets: rank j belongs to group j/group_R and goes to G, G1 or G2 (rank j%group_R,
 * written only if < r_valid).  Replaces autograd's dW for lora_A / lora_B (frozen base weights never get a dW).
 */
typedef struct qfx_lora_grad_args {
  const uint16_t* Vt_hi; const uint16_t* Vt_lo; int64_t ldvt; int32_t R; int32_t r_valid; int32_t group_R;
  const uint16_t* X; int64_t ldx; int32_t M; int32_t K;
  float* G; float* G1; float* G2; int64_t g_sr; int64_t g_sc;
  int32_t rows_per_batch; int32_t x_batch_rows; int32_t x_row_off;
  float out_scale;                       /* lora_alpha/r for dB, 1 for dA */
  /* ABI 7 (optional; NULL = the round-1..5 behaviour: the partial sums of the token chunks meet in G by fp32 atomics, order-dependent
   * in the last bit).  ws: fp32 scratch of ws_floats >= qfx_lora_grad_ws_floats(M, K, R) elements, ws_count: int32[(K + 127) / 128], ZERO before the
   * first launch (every launch leaves it zero).  With both set the chunk partials go to ws and are added up in CHUNK ORDER before G is
   * updated with plain stores: same inputs -> same bits.  The library does that in a second launch on the same stream (the kernel
   * boundary is the hand-off).  ws_count is validated but no longer read: it held the tickets of an in-launch reduction that was
   * slower (profiles/r06_grad_handoff.json). */
  float* ws; int32_t* ws_count; int64_t ws_floats;      /* ws_floats = elements allocated behind ws: launches that need more are refused (QFX_EINVAL) */
} qfx_lora_grad_args;

int qfx_lora_grad(const qfx_lora_grad_args* args, void* stream);
int qfx_lora_grad_batch(const qfx_lora_grad_args* list, int32_t n, void* stream);   /* same R for all; see qfx_lora_down_batch */
int64_t qfx_lora_grad_ws_floats(int32_t M, int32_t K, int32_t R);   /* fp32 elements of qfx_lora_grad_args.ws for one problem (0: a single token chunk, no scratch needed) */

/* ---- LoRA operand packing (after every optimizer step) ---------------------------------------
 * From fp32 A[r,K], B[N,r] and scale s = lora_alpha/r build (Rp = r rounded up to 16):
 *   A_hi/A_lo [Rp,K] bf16, Bt_hi/Bt_lo [Rp,N] bf16 (= split of s*B^T),
 *   We  [N, Kext] = [sB_hi | sB_hi | sB_lo | 0]   (forward B2 operand)
 *   WeT [K, Kext] = [A_hi^T | A_hi^T | A_lo^T | 0] (dX B2 operand),  Kext = roundup(3*Rp, 64).
 */
typedef struct qfx_lora_pack_args {
  const float* A; const float* B; int32_t r; int32_t K; int32_t N; float scale;
  uint16_t* A_hi; uint16_t* A_lo; int64_t ld_a;      /* [Rp,K] rows at stride ld_a */
  uint16_t* Bt_hi; uint16_t* Bt_lo; int64_t ld_bt;   /* [Rp,N] rows at stride ld_bt */
  uint16_t* We; int64_t ld_we;                       /* [N,Kext] */
  uint16_t* WeT; int64_t ld_wet;                     /* [K,Kext] */
  int32_t Rp; int32_t Kext;
  /* ABI 6 (optional, NULL = off): head-fragment images for qfx_head_lora.  A_hl: (A_hi, A_lo) of an adapter whose INPUT is a
   * [*, H*hl_dh] attention output; Bt_hl: (Bt_hi, Bt_lo) of an adapter whose OUTPUT is a q / k / v row.  Element (row j, column
   * h*hl_dh + 32 ks + 16 db + 4 g + r) of the hi (sel = 0) / lo (sel = 1) split sits at
   *   ((((h * Rp/16 + j/16) * hl_dh/32 + ks) * 2 + sel) * 64 + 16 g + j%16) * 8 + 4 db + r        (bf16 elements). */
  uint16_t* A_hl; uint16_t* Bt_hl; int32_t hl_dh; int32_t reserved;
  /* ABI 6 (optional, NULL = off): the A rows of this adapter inside the MFMA-FRAGMENT image of a row group that a fused
   * LayerNorm + down projection reads (qfx_ln_down_args.W_fr): fr_nf = 16-row fragments of the whole group (q, k, v adapters
   * of one stream: 3 Rp / 16), fr_row0 = first group row of this adapter.  Element (group row j, column k) of the hi split sits at
   *   ((k/32 * fr_nf + j/16) * 64 + 16 * ((k%32)/8) + j%16) * 8 + k%8      (bf16 elements),
   * the lo split fr_nf * 16 * K elements further: a fragment of 16 rows x 32 columns is ONE lane-linear 1 KiB piece. */
  uint16_t* A_fr; int32_t fr_row0; int32_t fr_nf;
} qfx_lora_pack_args;

/* descs: DEVICE array of n descriptors (one per LoRA target); one launch packs them all. */
int qfx_lora_pack(const qfx_lora_pack_args* descs, int32_t n, int32_t max_dim, void* stream);

/* ---- LayerNorm (no affine, eps) + modulation ------------------------------------------------
 * y = bf16(bf16(bf16(LN(x)) * bf16(1+scale[b])) + shift[b])    (transformer_qwenimage.py:420-423,443-448,477-484;
 * AdaLayerNormContinuous at :662).  x,y [rows,D]; shift/scale [B,*] with batch stride mod_bstride.
 */
int qfx_ln_modulate_fwd(const uint16_t* x, const uint16_t* shift, const uint16_t* scale, int64_t mod_bstride,
                        uint16_t* y, int32_t rows, int32_t D, int32_t rows_per_batch, float eps, void* stream);
/* dx = bf16(dres + bf16(LN_bwd(dy * bf16(1+scale)))) ; optional dyg = bf16(gate[b] * dx) (input of the
 * previous gated-residual GEMM's backward). dres/gate/dyg may be NULL. */
int qfx_ln_modulate_bwd(const uint16_t* dy, const uint16_t* x, const uint16_t* scale, int64_t mod_bstride,
                        const uint16_t* dres, const uint16_t* gate, int64_t gate_bstride,
                        uint16_t* dx, uint16_t* dyg, int32_t rows, int32_t D, int32_t rows_per_batch,
                        float eps, const float* row_mask, void* stream);
/* row_mask (optional, [rows]): rows with mask 0 get dx = dyg = 0 (backward of the padded-token zeroing). */

/* Batched forms: n <= QFX_MAX_LN_BATCH problems in ONE launch (the image and the text stream of a block: the 384-row text
 * problem otherwise pays a dispatch gap and a memory round trip of its own).  Every problem but the last needs rows % 4 == 0. */
#define QFX_MAX_LN_BATCH 4
/* ABI 2, MX-FP8 trunk: yq / dygq != NULL -- the output (y resp. dyg) ALSO leaves the kernel as MX-FP8 (bytes at yq + row*ldyq,
 * E8M0 scales tile-major [D/128][ys_rows][4] as qfx_quant_mxfp8 writes them, bit-identical to quantising the bf16 output in a
 * separate pass; D % 128 == 0): the GEMM that consumes it skips its quantisation pass. */
typedef struct qfx_ln_fwd_args {
  const uint16_t* x; const uint16_t* shift; const uint16_t* scale; int64_t mod_bstride; uint16_t* y;
  int32_t rows; int32_t D; int32_t rows_per_batch; float eps;
  uint8_t* yq; uint8_t* ys; int64_t ldyq; int32_t ys_rows; int32_t pad_;
} qfx_ln_fwd_args;
typedef struct qfx_ln_bwd_args {
  const uint16_t* dy; const uint16_t* x; const uint16_t* scale; int64_t mod_bstride;
  const uint16_t* dres; const uint16_t* gate; int64_t gate_bstride; uint16_t* dx; uint16_t* dyg;
  const float* row_mask; int32_t rows; int32_t D; int32_t rows_per_batch; float eps;
  uint8_t* dygq; uint8_t* dygs; int64_t lddygq; int32_t dygs_rows; int32_t pad_;
} qfx_ln_bwd_args;
int qfx_ln_modulate_fwd_batch(const qfx_ln_fwd_args* list, int32_t n, void* stream);
int qfx_ln_modulate_bwd_batch(const qfx_ln_bwd_args* list, int32_t n, void* stream);
/* ---- fused LayerNorm+modulate forward AND the LoRA down projection of its output ("AdaLN fused into the projection
 * prologue", BASELINE north_star): y = bf16(LN(x) * bf16(1 + scale[b])) + shift[b] as qfx_ln_modulate_fwd, and in the same pass over
 * the row block u = y (W_hi + W_lo)^T with the K-extension image `ext` and the transposed split image `Ut` exactly as
 * qfx_lora_down writes them (same rounding points and MFMA order; the fp32 row statistics are summed in a different order than
 * in the one-wave-per-row kernel, so y may differ from it in the last bf16 ulp on rare elements).  Problems with
 * W_hi == NULL are plain LayerNorm+modulate rows (the un-adapted stream of a block rides in the same launch).
 * D % 256 == 0, D <= 3072, R in {16, 32, 48} and equal for all adapted problems of one call; n <= 2. */
typedef struct qfx_ln_down_args {
  qfx_ln_fwd_args ln;
  const uint16_t* W_hi; const uint16_t* W_lo; int64_t ldw; int32_t R;
  uint16_t* ext; int64_t ld_ext; uint16_t* Ut_hi; uint16_t* Ut_lo; int64_t ld_ut;
  int32_t group_R; int32_t group_stride;
  /* ABI 6 (optional): the same weights in MFMA-fragment order (qfx_lora_pack_args.A_fr: hi image, lo image R * D elements further).
   * Row-major weights are read as 16-byte pieces of 16 different rows per 16 lanes (64 line visits per wave load); the fragment image
   * as 8 whole lines: 37.4 -> 30.3 us per launch at the headline shape.  NULL: W_hi / W_lo are read. */
  const uint16_t* W_fr;
} qfx_ln_down_args;
int qfx_ln_down_fwd(const qfx_ln_down_args* list, int32_t n, void* stream);

/* ---- gradients of the AdaLN modulation vectors (needed only when the modulation linears carry adapters:
 * `img_mod.1` / `norm1.linear` ... in target_modules, configs/face_seg_flux_kontext_fp16.yaml:11, "all-linear").
 * For xm = bf16(LN(x) * bf16(1 + scale[b])) + shift[b]   (transformer_qwenimage.py:443-448; AdaLayerNormZero)
 * and  xo = x_res + bf16(gate[b] * y)                     (transformer_qwenimage.py:479-485)
 *   dshift[b] += sum_rows dy,   dscale[b] += sum_rows dy * bf16(LN(x)),   dgate[b] += sum_rows dxo * y
 * (fp32 accumulation, atomics into zero-initialised [B, out_bstride] buffers; rows of sample b = rows_per_batch consecutive
 * rows).  dxo / y / dgate may be NULL together (AdaLayerNormContinuous has no gate).  Row strides are explicit. */
typedef struct qfx_mod_grad_args {
  const uint16_t* dy; int64_t ld_dy; const uint16_t* x; int64_t ld_x;
  const uint16_t* dxo; int64_t ld_dxo; const uint16_t* y; int64_t ld_y;
  float* dshift; float* dscale; float* dgate; int64_t out_bstride;
  const float* row_mask; int32_t rows; int32_t D; int32_t rows_per_batch; float eps;
} qfx_mod_grad_args;
int qfx_mod_grad(const qfx_mod_grad_args* a, void* stream);
/* ABI 4: n <= QFX_MAX_LN_BATCH problems of one width class (ceil(D / 512) equal) in ONE launch -- the image and the text stream of a
 * block (the 384-row text problem otherwise pays a dispatch gap and a latency chain of its own for 48 blocks of work). */
int qfx_mod_grad_batch(const qfx_mod_grad_args* list, int32_t n, void* stream);

/* dyg = bf16(gate[b] * dx) only (used where no LayerNorm precedes). */
int qfx_gate_mul(const uint16_t* dx, const uint16_t* gate, int64_t gate_bstride, uint16_t* dyg,
                 int32_t rows, int32_t D, int32_t rows_per_batch, void* stream);

/* ---- RMSNorm over the last dim with learned weight (txt_norm, transformer_qwenimage.py:625) */
int qfx_rmsnorm_fwd(const uint16_t* x, const uint16_t* w, uint16_t* y, int32_t rows, int32_t D, float eps, void* stream);

/* ---- modulation GEMV: out[i][b][n] = bf16( sum_k bf16(silu(temb[b][k])) * W_i[n][k] + bias_i[n] )
 * for a list of nmat weight matrices (all [N,K]) -- every block's img_mod/txt_mod in one launch
 * (transformer_qwenimage.py:389-392,411-414,435-436; HBM-bound). */
int qfx_mod_gemv(const uint16_t* temb, int32_t B, int32_t K, const uint16_t* const* W, const uint16_t* const* bias,
                 int32_t nmat, int32_t N, int32_t apply_silu, uint16_t* out, void* stream);
/* W, bias: DEVICE arrays of nmat device pointers. apply_silu=0 gives a plain small-batch Linear
 * (timestep_embedder.linear_1). B <= 8. */
/* The same launch guarded by a device flag: every block returns before it touches anything when *skip != 0; with skip == NULL or
 * *skip == 0 it is qfx_mod_gemv bit for bit (one kernel).  The flag is the `hit` cell of qfx_mod_table_fetch. */
int qfx_mod_gemv_unless(const uint16_t* temb, int32_t B, int32_t K, const uint16_t* const* W, const uint16_t* const* bias,
                        int32_t nmat, int32_t N, int32_t apply_silu, uint16_t* out, const int32_t* skip, void* stream);
/* Modulation table of a frozen conditioning head: row i of tbl_mods ([n] rows of [nmat][N], ld_mods elements apart) and of tbl_out
 * ([n] rows of [N_out], ld_out apart) holds what the qfx_timestep_embed -> qfx_mod_gemv chain writes for the timestep keys[i].
 * Keys match as fp32 WORDS (NaN never hits, -0.0 is not 0.0).  Iff every one of the B timesteps t[b] is a key, sample b's rows are
 * copied to mods[mat][b][:] ([nmat][B][N]) and mod_out[b][:] ([B][N_out]) -- the layout of qfx_mod_gemv -- and *hit = 1; otherwise
 * *hit = 0 and neither destination is written.  Decided on the device: nothing reads the flag on the host.  B <= 8, n >= 1; the
 * four bf16 bases 16-byte aligned (rows that are not take the element-wise path). */
int qfx_mod_table_fetch(const float* t, int32_t B, const float* keys, int32_t n, const uint16_t* tbl_mods, int64_t ld_mods,
                        int32_t nmat, int32_t N, const uint16_t* tbl_out, int64_t ld_out, int32_t N_out, uint16_t* mods,
                        uint16_t* mod_out, int32_t* hit, void* stream);
/* Backward of the same frozen linears w.r.t. their (shared) input, needed when the conditioning head carries adapters
 * (target_modules "all-linear", configs/example_with_sampling.yaml:9): out[b, k] (fp32 [B, K], zeroed by the caller) +=
 * sum_mat sum_n dy[mat, b, n] * W_mat[n, k], dy bf16 [nmat, B, N] -- what autograd computes as dy @ W per module and sums.
 * One streaming pass over the weights (two passes per pair of samples beyond B = 2).  K <= 3072, K % 8 == 0. */
int qfx_mod_gemv_t(const uint16_t* dy, int32_t B, int32_t N, int32_t K, const uint16_t* const* W, int32_t nmat, float* out,
                   void* stream);

/* ---- adapters on the conditioning head (target_modules "all-linear", configs/example_with_sampling.yaml:9; the
 * (norm|norm1|norm1_context).linear alternatives of configs/face_seg_flux_kontext_fp16.yaml:11): the rank-r side terms of linears
 * that see M = batch rows -- timestep / guidance / pooled-text embedders (transformer_qwenimage.py:143-156,
 * transformer_flux.py:634-639), AdaLN modulation linears (:389-392,411-414 / transformer_flux.py:391,446-447), norm_out.linear
 * (:565) -- for a BANK of `na` adapters of one rank that share the input x [B,K] (bf16).  peft lora.Linear semantics
 * (call site base_trainer.py:929-941):
 *   qfx_cond_lora_fwd:  u_a = A_a act(x) (fp32, kept in `u`);  y_a[b][n] = bf16(float(y_a[b][n]) + scale_a * sum_j B_a[n][j] u_a[b][j])
 *                       in place on the base outputs qfx_mod_gemv wrote (y: device array of na row pointers, row b at + b*ldy).
 *   qfx_cond_lora_bwd:  g_a = bf16 gradient rows of the outputs (device array of na pointers, row b at + b*ldg);
 *                       dB_a += (scale_a g_a)^T u_a;  du_a = (scale_a g_a) B_a;  dA_a += du_a^T act(x);  dx[b][k] += sum_a du_a A_a
 *                       (dx fp32 [B,K] = gradient w.r.t. act(x), may be NULL; du [na,B,r] fp32 scratch ZEROED by the caller;
 *                       dA / dB: device arrays of pointers into the flat LoRA gradient buffer, accumulated).
 * act = bf16(silu(.)) when apply_silu (the eager graph's F.silu on bf16), identity otherwise.  A_a [r,K], B_a [N,r] fp32
 * (device arrays of pointers to the adapter weights), scale: device [na].  B <= 8, r <= 64. */
typedef struct qfx_cond_lora_args {
  const uint16_t* x; int32_t B; int32_t K; int32_t apply_silu; int32_t na; int32_t r; int32_t N;
  const float* const* A; const float* const* Bm; const float* scale;
  float* u;
  uint16_t* const* y; int64_t ldy;
  const uint16_t* const* g; int64_t ldg;
  float* const* dA; float* const* dB;
  float* du; float* dx;
} qfx_cond_lora_args;
int qfx_cond_lora_fwd(const qfx_cond_lora_args* a, void* stream);
int qfx_cond_lora_bwd(const qfx_cond_lora_args* a, void* stream);
/* out = bf16(in): the fp32 column sums of the HIP backward (qfx_mod_grad) handed to the head's backward as the bf16 gradients
 * autograd would see */
int qfx_cast_f32_bf16(const float* in, uint16_t* out, int64_t n, void* stream);
/* dx = bf16(bf16(ds) * silu'(x)): silu_backward of the eager graph on the conditioning vectors (temb, the embedders' hidden layers) */
int qfx_silu_bwd(const float* ds, const uint16_t* x, uint16_t* dx, int64_t n, void* stream);

/* ---- sinusoidal timestep projection (diffusers Timesteps(dim, flip_sin_to_cos=True, shift 0, scale);
 * transformer_qwenimage.py:147,151-152,623-624): t is first rounded to bf16 (timestep.to(bf16)),
 * out[b] = bf16([cos(t*scale*f_i) | sin(t*scale*f_i)]), f_i = exp(-ln(1e4) * i / (dim/2)). */
int qfx_timestep_embed(const float* t, int32_t B, int32_t dim, float scale, float pre_scale, uint16_t* out, void* stream);
/* pre_scale != 1: the value embedded is bf16(bf16(t) * pre_scale) (FLUX: `timestep.to(dtype) * 1000`, transformer_flux.py:729-730,
 * with scale = 1); Qwen passes pre_scale = 1, scale = 1000. */

/* out = bf16(bf16(a + b) + c)  (c may be NULL): sum of the time / guidance / pooled-text embeddings
 * (diffusers CombinedTimestepGuidanceTextProjEmbeddings, transformer_flux.py:731-735) */
int qfx_add3_bf16(const uint16_t* a, const uint16_t* b, const uint16_t* c, uint16_t* out, int64_t n, void* stream);

/* ---- QK RMSNorm + RoPE on the joint [text|image] qkv buffer ---------------------------------
 * qkv [B,S,3*H*dh] (q|k|v sections), in place on the q and k sections:
 *   t = bf16(bf16(x * rsqrt(mean(x^2)+eps)) * w) ; out = bf16(complex(t) * rope[s])   pairs (2j,2j+1)
 * w = w_txt_* for rows s < T, w_img_* otherwise. rope [S, dh/2, 2] fp32 (cos,sin), joint order.
 * (transformer_qwenimage.py:305-320, apply_rotary_emb_qwen :134-140). Pre-norm q,k are first copied to
 * `saved` [B,S,2*H*dh] (needed by the backward) when saved != NULL.
 */
/* rope_bstride: elements between consecutive samples' tables (per-sample RoPE of the multi-resolution path,
 * transformer_flux_custom.py:537-560); 0 = one table shared by the batch. */
int qfx_qk_norm_rope_fwd(uint16_t* qkv, uint16_t* saved, const float* rope,
                         const uint16_t* wq_txt, const uint16_t* wk_txt, const uint16_t* wq_img, const uint16_t* wk_img,
                         int32_t B, int32_t S, int32_t T, int32_t H, int32_t dh, float eps, int32_t flags, int64_t rope_bstride,
                         void* stream);
/* flags bit0: torch.nn.RMSNorm rounding (FLUX, transformer_flux.py:342-343: one rounding after x*rstd*w) instead of the
 * diffusers RMSNorm double rounding (Qwen).
 * flags bit1 (forward only): OUT OF PLACE -- the pre-norm q,k are read from `saved` ([B,S,2*H*dh], where the q/k projections
 * wrote them) and the normalised, rotated q,k go to the q,k sections of qkv: no copy pass (one 2*B*S*H*dh*2-byte write less). */
/* in place on the q,k sections of dqkv (v section untouched): un-rotate, RMSNorm backward. */
int qfx_qk_norm_rope_bwd(uint16_t* dqkv, const uint16_t* saved, const float* rope,
                         const uint16_t* wq_txt, const uint16_t* wk_txt, const uint16_t* wq_img, const uint16_t* wk_img,
                         int32_t B, int32_t S, int32_t T, int32_t H, int32_t dh, float eps, int32_t flags, int64_t rope_bstride,
                         void* stream);

/* ---- [B,S,H,dh] (row stride ld_in, column offset applied by caller) -> [B,H,dh,S_pad] with zero pad */
int qfx_transpose_heads(const uint16_t* in, int64_t ld_in, uint16_t* out, int32_t B, int32_t S, int32_t S_pad,
                        int32_t H, int32_t dh, void* stream);

/* ---- joint attention (non-causal flash attention, optional additive key mask) ---------------
 * Replaces torch.cat + F.scaled_dot_product_attention (transformer_qwenimage.py:324-337) and its backward.
 * Q,K,V: token-major [B,S,H,dh] views with row stride ld (elements).  Kt,Vt,Qt,dOt ([B,H,dh,S_pad]) are RESERVED: the
 * kernels take their transposed MFMA operands from the row-major LDS tiles with ds_read_b64_tr_b16, so no transposed
 * copy is read any more; the fields keep the struct layout stable and may be NULL.
 * O [B,S,H*dh] (row stride ldo). lse2 [B,H,S_pad] fp32 = log2-domain logsumexp. key_mask [B,S] fp32 additive or NULL.
 * At least one key of every sample must have a finite key_mask value.  The kernels write rows s < S and columns < H*dh only: the
 * pad columns [S, S_pad) of lse2 and dsum are never written (the backward reads but never uses them), and neither are the part
 * rows of a stream whose w_pk is NULL or the columns of a part row outside [c0, c0 + R).
 */
/* ABI 6: a rank-r LoRA down projection fused into an attention epilogue (north_star: "LoRA side branches ... inside the kernels").
 * The kernel that holds a row of X = O / d(pre-norm q) / d(pre-norm k) / dV in registers also emits, per head h,
 *     part[h * part_hstride + row * ld_part + c0 + j] = sum_{n < dh} X[row, h*dh + n] * (W_hi + W_lo)[j, h*dh + n]      (j < R, fp32)
 * with row = the JOINT row b*S + s; qfx_lora_head_reduce adds the H slabs in a fixed order and writes the bf16 images
 * qfx_lora_down would have written (peft: lora_A(x) in the forward, dY * B in the backward; base_trainer.py:929-941).
 * w_pk = the adapter weight in HEAD-FRAGMENT order (qfx_lora_pack's A_hl / Bt_hl images: the MFMA operand of lane l for head h, 16-row
 * group nf, 32-column step ks is 16 contiguous bytes, hi and lo split interleaved per step -- fully coalesced 1 KiB wave loads; the
 * row-major split images cost 7 us per launch in 8-byte pieces at row stride); index [0] applies to rows s >= T (image stream), [1]
 * to rows s < T (text stream); NULL = that stream has no adapter on this linear.  Needs T % 16 == 0, R in {16, 32}, part 16-byte
 * aligned with ld_part % 4 == 0 and c0 % 4 == 0.  part == NULL: off. */
typedef struct qfx_head_lora {
  const uint16_t* w_pk[2];
  float* part; int64_t part_hstride; int32_t ld_part; int32_t c0; int32_t R; int32_t reserved;
} qfx_head_lora;

typedef struct qfx_attn_args {
  const uint16_t* Q; const uint16_t* K; const uint16_t* V; int64_t ldq; int64_t ldk; int64_t ldv;
  const uint16_t* Qt; const uint16_t* Kt; const uint16_t* Vt;   /* reserved (unused), may be NULL */
  uint16_t* O; int64_t ldo;
  float* lse2; float* dsum;                                      /* [B,H,S_pad] */
  const uint16_t* dO; int64_t lddo; const uint16_t* dOt;         /* dOt reserved (unused) */
  uint16_t* dQ; uint16_t* dK; uint16_t* dV; int64_t lddq; int64_t lddk; int64_t lddv;
  const float* key_mask;
  int32_t B; int32_t S; int32_t S_pad; int32_t H; int32_t dh; float scale;
  /* ABI 3: backward of the QK RMSNorm + RoPE (transformer_qwenimage.py:305-320) fused into the EPILOGUES of qfx_attn_bwd_dq / _dkv
   * when qk_saved != NULL: the kernels then write d(pre-norm q) / d(pre-norm k) instead of d(q) / d(k) -- the arithmetic of
   * qfx_qk_norm_rope_bwd on the bf16-rounded attention gradient, same rounding points (norm_flags as there), without the extra
   * pass over dqkv.  qk_saved: the pre-norm q | k copy [B,S,2*H*dh] qfx_qk_norm_rope_fwd kept (row stride ld_saved, q at +0, k at
   * +H*dh); rope [S, dh/2, 2] fp32 (+ b * rope_bstride); weights [dh] bf16, *_txt for rows s < T. */
  const uint16_t* qk_saved; int64_t ld_saved; const float* rope; int64_t rope_bstride;
  const uint16_t* wq_txt; const uint16_t* wk_txt; const uint16_t* wq_img; const uint16_t* wk_img;
  int32_t T; int32_t norm_flags; float norm_eps;
  /* ABI 6 (zero = off): hl[0] X = O in qfx_attn_fwd; hl[1] X = d(pre-norm q) in qfx_attn_bwd_dq; hl[2] X = d(pre-norm k), hl[3] X = dV
   * in qfx_attn_bwd_dkv (the backward slots need qk_saved != NULL). */
  qfx_head_lora hl[4];
  /* ABI 7: workspace of the ONE-PASS backward qfx_attn_bwd_fused (sizes from qfx_attn_bwd_fused_workspace; ignored by every other entry
   * point): dq_acc = fp32 dQ tiles accumulated across the key blocks of a head, dq_turn = per-(batch, head, query tile) turn counters,
   * ZERO before the first launch (every launch leaves them zero again). */
  float* dq_acc; int32_t* dq_turn;
} qfx_attn_args;

int qfx_attn_fwd(const qfx_attn_args* a, void* stream);       /* needs Q,K,V -> O,lse2 */
int qfx_attn_bwd_prep(const qfx_attn_args* a, void* stream);  /* dsum = rowsum(dO*O); optional: qfx_attn_bwd_dq computes and writes it too */
int qfx_attn_bwd_dq(const qfx_attn_args* a, void* stream);    /* needs Q,K,V,O,dO,lse2 -> dQ and dsum (= rowsum(dO*O), consumed by qfx_attn_bwd_dkv: launch dq first) */
int qfx_attn_bwd_dkv(const qfx_attn_args* a, void* stream);   /* needs Q,K,V,dO,lse2,dsum -> dK,dV */
/* ABI 7: the whole backward of the joint SDPA (transformer_qwenimage.py:329-337 under autograd) in ONE pass over the score tiles
 * (csrc/qfx_attn_bwd1.hip): needs Q,K,V,O,dO,lse2 and the workspace dq_acc / dq_turn -> dQ,dK,dV (and dsum); every optional block of
 * qfx_attn_args (key_mask, qk_saved..., hl[1..3]) means what it means for qfx_attn_bwd_dq + qfx_attn_bwd_dkv, results agree with that
 * pair to fp32 summation order (dQ is summed over 256-key blocks in a fixed order: bit-reproducible).  dh = 128 only; the launch is a
 * persistent grid of whole heads (<= 256 blocks) whose blocks wait for each other: it must not share the device with another kernel
 * that never terminates.  qfx_attn_bwd_fused_workspace: bytes the two workspaces need for this shape; returns QFX_EUNSUPPORTED (sizes 0)
 * where the one-pass form does not exist (dh != 128, S < 64) -- the caller then launches the two-pass pair. */
int qfx_attn_bwd_fused(const qfx_attn_args* a, void* stream);
int qfx_attn_bwd_fused_workspace(const qfx_attn_args* a, int64_t* acc_bytes, int64_t* turn_bytes);
/* ABI 7: kernel-selection policy of the attention entry points (process-wide, read from the environment QFX_ATTN_FWD64 /
 * QFX_ATTN_DQ64 / QFX_ATTN_FWD_WAVES once, at the first launch; this call overrides it): comma list of key=value with
 * fwd64 = 0 | 1 | 1p | auto (32-query kernels | 64-query kernel | its pipelined form | by shape), dq64 = 0 | 1 | auto, fwd_waves = 0 | 4 | 8.
 * NULL / "" = keep.  Returns QFX_EINVAL (nothing changed) on an unknown key or value. */
int qfx_attn_tune(const char* spec);

/* ---- flow-matching MSE criterion (src/qflux/losses/mse_loss.py:66-83 with weighting=1;
 * caller math of src/qflux/trainer/qwen_image_edit_trainer.py:839-847) --------------------------
 * pred [B, S_all, C] bf16 (only rows < S_t per sample enter), target [B,S_t,C] bf16.
 * loss (fp32 scalar, must be zeroed by caller) += mean_b mean_{s,c} (pred-target)^2 ;
 * dpred [B,S_all,C] bf16 = bf16(2*(pred-target)/(B*S_t*C) * gscale), zero for rows >= S_t. */
int qfx_mse_loss_fwd_bwd(const uint16_t* pred, const uint16_t* target, float* loss, uint16_t* dpred,
                         int32_t B, int32_t S_all, int32_t S_t, int32_t C, float gscale, void* stream);

/* token-weighted variant (src/qflux/losses/attention_mask_loss.py:146-226, reduction="mean"): token_w [B,S_t] fp32 =
 * attention_mask * edit weight; loss += sum_{b,s} token_w * mean_c (pred-target)^2 * inv_denom, inv_denom = 1/(num_valid+eps)
 * (the caller knows the valid-token count on the host: no device sync). dpred as above with the same weights. */
int qfx_mse_token_weighted_fwd_bwd(const uint16_t* pred, const uint16_t* target, const float* token_w, float* loss, uint16_t* dpred,
                                   int32_t B, int32_t S_all, int32_t S_t, int32_t C, float inv_denom, float gscale, void* stream);

/* ---- flow-matching input preparation (qwen_image_edit_trainer.py:811-812,841), bf16 eager rounding:
 * packed[b] = cat(bf16(bf16(bf16(1-sigma)*x0) + bf16(sigma*noise)), ctrl) ; target = bf16(noise - x0) */
int qfx_flowmatch_prepare(const uint16_t* x0, const uint16_t* noise, const uint16_t* ctrl, const uint16_t* sigma,
                          uint16_t* packed, uint16_t* target, int32_t B, int32_t S_t, int32_t S_c, int32_t C, int32_t mode,
                          void* stream);
/* mode 0 (Qwen): everything bf16 as documented above. mode 1 (FLUX, flux_kontext_trainer.py:522-525,567-568): x0 holds FP16
 * bits (the cache dtype), packed = bf16(fp32(bf16(1-t))*x0 + fp32(bf16(t*noise))), target = bf16(noise - bf16(x0)). */

/* ---- fused global-norm clip + AdamW over the flat LoRA parameter buffer ----------------------
 * (base_trainer.py:449-455 clip_grad_norm_ ; optimizer.step :531 with torch.optim.AdamW semantics) */
/* qfx_sumsq ADDS the sum of squares into out[0] (one fp32 atomic per workgroup, in any order): the caller zeroes out, or keeps a
 * running total there.  Rejected with QFX_EINVAL: a NULL g or out, n <= 0. */
int qfx_sumsq(const float* g, int64_t n, float* out /* added into */, void* stream);
/* Deterministic form (ABI 3): block partial sums into `partials` (fp32[nslots], caller workspace, e.g. 1024), folded by one block in
 * a fixed order into out[0] (overwritten).  Same inputs -> same bits: data-parallel replicas (identical gradients after the
 * all-reduce) compute the SAME clip coefficient; qfx_sumsq's fp32 atomics let them drift apart by ~1e-10 per step.  Rejected with
 * QFX_EINVAL: a NULL g, out or partials, n <= 0, nslots <= 0. */
int qfx_sumsq_det(const float* g, int64_t n, float* out, float* partials, int32_t nslots, void* stream);
/* qfx_adamw_step rejects only a NULL p / g / m / v and n <= 0; its scalars are NOT validated (the grouped entry validates its rows):
 * bias_corr1 = 1 - beta1^t and bias_corr2 = 1 - beta2^t come from the caller, and the kernel forms lr / bias_corr1 and
 * 1 / sqrt(bias_corr2) once per launch.  gnorm_sq == NULL or max_norm <= 0: clip = grad_scale. */
int qfx_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, float bias_corr1, float bias_corr2,
                   const float* gnorm_sq /* may be NULL */, float max_norm, float grad_scale, void* stream);

/* ---- torch.optim.SGD, the fourth optimizer the reference documents (docs/guide/training.md:768-826, configuration.md:67,163-166:
 * momentum 0.9, weight_decay 1e-4; instantiated generically at base_trainer.py:884-909, stepped at :531 after clip_gradients
 * :449-455).  ONE launch over the flat fp32 LoRA buffers.  With clip exactly as qfx_adamw_step computes it from gnorm_sq / max_norm /
 * grad_scale (gnorm_sq == NULL or max_norm <= 0: clip = grad_scale), per element:
 *   gi = g * clip + weight_decay * p                            (L2 form; the clip comes first, as clip_grad_norm_ precedes step())
 *   momentum != 0:  buf = first ? gi : momentum * buf + (1 - dampening) * gi       (torch's first step applies no dampening)
 *                   gi  = nesterov ? gi + momentum * buf : buf
 *   p -= lr * gi
 * buf [n] may be NULL iff momentum == 0 (it is then neither read nor written); `first` != 0 on the step that creates buf (its
 * contents are then ignored).  No atomics: same inputs -> same bits.  Rejected with QFX_EINVAL before any launch: a NULL p or g,
 * n <= 0, a NULL buf with momentum != 0, nesterov with momentum <= 0 or dampening != 0 (torch's ValueError). ---- */
int qfx_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float dampening, float weight_decay,
                 int32_t nesterov, int32_t first, const float* gnorm_sq /* may be NULL */, float max_norm, float grad_scale,
                 void* stream);

/* ---- parameter groups (torch.optim's second axis: LoRA+ gives lora_B a higher lr than lora_A, peft's create_loraplus_optimizer /
 * kohya's loraplus_lr_ratio; no weight decay on lora_B; other rates per stream).  Every *_grouped entry below is its family's ONE
 * launch with the hyperparameters read per element from the row of the group the element's tensor belongs to; the arithmetic is the
 * ungrouped entry's, statement for statement (both kernels call one element function in one translation unit), so a grouped step
 * gives every tensor the bits an ungrouped step with its group's scalars gives it.  The clip stays global: ONE coefficient from
 * gnorm_sq / max_norm / grad_scale for all groups (clip_grad_norm_ runs over all parameters before step()).
 * groups: HOST array of n_groups rows, 1 <= n_groups <= QFX_MAX_PARAM_GROUPS, copied into the argument block (no device allocation, no
 * copy per step) and turned into per-group constants in LDS at workgroup start.
 * fp32 families: tile_group = device uint8[ceil(n / 64)], the group of every 64-element tile of the flat buffers -- every tensor
 * starts on a multiple of 64 elements (LoraStore), so a tile never holds two tensors; the padding behind a tensor carries the
 * tensor's group.  16-byte accesses when the buffers are 16-byte aligned.
 * blockwise 8-bit families: block_group = device uint8[n_blocks], the group of every block-table entry (an entry never leaves its
 * tensor); the scalar hyperparameters of the args struct are ignored, `step` is the one count of all groups.
 * A map entry >= n_groups cannot be seen from the host without a synchronisation: the builder of the maps checks the range before
 * upload (ops.tile_group_map / ops.block_group_map); the kernels clamp the index to the rows they were given: an entry >= n_groups
 * steps its tile (block) with the LAST row, groups[n_groups - 1].
 * Rejected with QFX_EINVAL before any launch: what the ungrouped entry rejects, a NULL map or groups pointer, n_groups outside
 * 1..QFX_MAX_PARAM_GROUPS, a row with a negative lr, a beta outside [0, 1), a negative weight_decay or eps (SGD: a negative momentum, a NULL
 * buf with a row whose momentum != 0, nesterov with momentum <= 0 or dampening != 0).  No atomics: same inputs -> same bits.
 * qfx_grouped_sweep_elems: the elements one grid sweep of a grouped launcher covers before its stride loop runs again -- blocksize
 * 0: the fp32 kernels (16-byte form), 256 / 2048: the blockwise kernels with full blocks; QFX_EINVAL otherwise. ---- */
#define QFX_MAX_PARAM_GROUPS 16
typedef struct qfx_adamw_group { float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2; } qfx_adamw_group;
typedef struct qfx_sgd_group { float lr, momentum, dampening, weight_decay; int32_t nesterov; } qfx_sgd_group;
typedef struct qfx_lion_group { float lr, beta1, beta2, weight_decay; } qfx_lion_group;
typedef struct qfx_adam8bit_group { float lr, beta1, beta2, eps, weight_decay; } qfx_adam8bit_group;
int64_t qfx_grouped_sweep_elems(int32_t blocksize);
int qfx_adamw_step_grouped(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* tile_group,
                           const qfx_adamw_group* groups, int32_t n_groups, const float* gnorm_sq /* may be NULL */, float max_norm,
                           float grad_scale, void* stream);
/* `first` as qfx_sgd_step's: the one step that creates buf, for every group */
int qfx_sgd_step_grouped(float* p, const float* g, float* buf, int64_t n, const uint8_t* tile_group, const qfx_sgd_group* groups,
                         int32_t n_groups, int32_t first, const float* gnorm_sq /* may be NULL */, float max_norm, float grad_scale,
                         void* stream);

/* ---- Prodigy, the reference's parameter-free optimizer choice (third party prodigyopt.Prodigy, requirements.txt:33; selected by
 * configs/face_seg_flux_kontext_fp16_prodigy.yaml:41-47 and the optimizer section of every tests/test_configs/test_example_*.yaml;
 * instantiated generically at base_trainer.py:884-898, stepped at :531 after clip_gradients :449-455).  One fused step over the
 * flat fp32 LoRA buffers: EMA update + the two global reductions (<g, p0 - p>, |s|_1) -> on-device update of the distance estimate
 * d -> parameter update.  The package's Python-float scalars live in `state` (device double[QFX_PRODIGY_STATE]: d, d_max,
 * d_numerator, d_denom, d_hat, k, then scratch), so nothing synchronises.  lr == 0 is the package's early return (nothing changes,
 * k does not advance).  beta3 <= 0 means sqrt(beta2).  Coupled weight decay (decouple = 0 with weight_decay != 0) is unsupported. */
#define QFX_PRODIGY_STATE 12
typedef struct qfx_prodigy_args {
  float* p;              /* [n] parameters, updated in place */
  const float* g;        /* [n] gradient (summed over ranks / micro-steps; scaled by grad_scale and the clip factor on the fly) */
  float* exp_avg;        /* [n] */
  float* exp_avg_sq;     /* [n] */
  float* s;              /* [n] */
  const float* p0;       /* [n] parameters at the first step() call */
  int64_t n;
  double* state;         /* device double[QFX_PRODIGY_STATE], initialised by qfx_prodigy_init_state */
  float lr, beta1, beta2, beta3, eps, weight_decay, d0, d_coef, growth_rate;
  int32_t use_bias_correction, safeguard_warmup, decouple;
  const float* gnorm_sq; /* may be NULL: sum of squares of g (qfx_sumsq) for the global-norm clip */
  float max_norm, grad_scale;
} qfx_prodigy_args;
/* d = d_max = d_hat = d0, everything else 0; synchronises.  d0 is the double the caller holds; the step's qfx_prodigy_args.d0 is a
 * float, and the package's `d == d0` (the first jump is not capped by growth_rate) is decided on their float images, so the two
 * spellings of one d0 (1e-6 and (float)1e-6) are equal. */
int qfx_prodigy_init_state(double* state, double d0, void* stream);
int qfx_prodigy_step(const qfx_prodigy_args* a, void* stream);

/* ---- blockwise 8-bit Adam / AdamW with bitsandbytes' state layout (third party bitsandbytes.optim.Adam8bit / AdamW8bit and their
 * Paged forms, selected by most of the reference's optimizer blocks, e.g. configs/face_seg_config.yaml:55-59; instantiated at
 * base_trainer.py:884-898, stepped at :531 after clip_gradients :449-455, resumed from optimizer.bin at :327-329).  ONE launch per
 * step over the flat LoRA buffers, driven by a block table the caller builds once per buffer layout.  Per element, with
 * g' = g * clip (clip exactly as qfx_adamw_step computes it from gnorm_sq / max_norm / grad_scale):
 *   8-bit block: m = qmap1[q1] * absmax1[blk], v = qmap2[q2] * absmax2[blk] (decoded), m = b1 m + (1-b1) g', v = b2 v + ((1-b2) g') g'
 *   fp32 block:  m = m32[..], v = v32[..],                                     m = b1 m + (1-b1) g', v = b2 v + (1-b2) (g' g')
 *   p += step_size * (m / (sqrt(v) + eps_hat)) with step_size = -lr sqrt(1-b2^t) / (1-b1^t), eps_hat = eps sqrt(1-b2^t) (both
 *   formed in double on the host, rounded to fp32), then p *= 1 - lr wd when wd > 0 (decoupled, after the update).  The update uses
 *   the fp32 moments, not their re-quantised images.  An element whose g' is not finite keeps p and its moments unchanged.
 * Per 8-bit block (`len` consecutive elements of ONE tensor): absmax = max |m| (resp. |v|) over the block; each moment is stored as
 * the nearest qmap code of m / absmax, the nearest being decided against the fp32 midpoints (q[k] + q[k+1]) / 2: x > midpoint -> the
 * upper code, x == midpoint -> the lower one.  state1 then keeps its sign (bnb's rule: a code whose value has the other sign bit than
 * m moves one index towards m).  A block whose absmax is 0 stores the code of 0.0 (it decodes to 0 whatever its codes).
 * No atomics: same inputs -> same bits.  qmap1 / qmap2: fp32[256] ascending code books (signed / unsigned dynamic maps; a checkpoint
 * carries its own).  Every pointer must be non-NULL (allocate one element for an unused buffer); p, g, q1, q2 are indexed by `off`,
 * m32 / v32 by `state` of the fp32 entries; `off` and `state` are multiples of 4.  Rejected with QFX_EINVAL before any launch: a NULL
 * pointer, blocksize outside {256, 2048}, n_blocks <= 0, step < 1, a negative lr. ---- */
#define QFX_ADAM8BIT_BLOCKWISE 0
#define QFX_ADAM8BIT_FP32 1
typedef struct qfx_adam8bit_block {
  int64_t off;           /* first element of the block in p / g / q1 / q2 */
  int64_t state;         /* QFX_ADAM8BIT_BLOCKWISE: index into absmax1 / absmax2; QFX_ADAM8BIT_FP32: first element in m32 / v32 */
  int32_t len;           /* 1 .. blocksize elements */
  int32_t mode;          /* QFX_ADAM8BIT_BLOCKWISE or QFX_ADAM8BIT_FP32 */
} qfx_adam8bit_block;
typedef struct qfx_adam8bit_args {
  float* p;              /* parameters, updated in place */
  const float* g;        /* gradient (summed over ranks / micro-steps; scaled by grad_scale and the clip factor on the fly) */
  uint8_t* q1;           /* state1 codes (signed map), same indexing as p */
  uint8_t* q2;           /* state2 codes (unsigned map) */
  float* absmax1;        /* per 8-bit block */
  float* absmax2;
  float* m32;            /* fp32 moments of the tensors below the 8-bit size */
  float* v32;
  const qfx_adam8bit_block* table;   /* device array of n_blocks entries */
  int32_t n_blocks;
  int32_t blocksize;     /* 256 or 2048: the largest `len` of the table */
  const float* qmap1;    /* fp32[256] */
  const float* qmap2;    /* fp32[256] */
  float lr, beta1, beta2, eps, weight_decay;
  int32_t step;          /* 1-based step count t (bias corrections) */
  const float* gnorm_sq; /* may be NULL: sum of squares of g (qfx_sumsq_det) for the global-norm clip */
  float max_norm, grad_scale;
} qfx_adam8bit_args;
int qfx_adam8bit_step(const qfx_adam8bit_args* a, void* stream);
/* parameter groups (see above): a->lr / beta1 / beta2 / eps / weight_decay are ignored, every table entry bi takes the row
 * groups[block_group[bi]]; step_size and eps_hat are formed per group, in double on the host, from the row and a->step */
int qfx_adam8bit_step_grouped(const qfx_adam8bit_args* a, const uint8_t* block_group, const qfx_adam8bit_group* groups,
                              int32_t n_groups, void* stream);

/* ---- Adafactor (third party transformers.optimization.Adafactor, the optimizer LoRA fine-tuning stacks offer next to the ones
 * above; in the reference one YAML line through the generic optimizer.class_path at base_trainer.py:884-909, stepped at :531 after
 * clip_gradients :449-455).  ONE launch steps every tensor of the flat fp32 LoRA buffers, one workgroup per tensor, driven by a device
 * table the caller builds once per buffer layout.  Per tensor of rows x cols elements, with g' = g * clip (clip exactly as
 * qfx_adamw_step computes it from gnorm_sq / max_norm / grad_scale), everything in fp32:
 *   RMS = |p|_2 / sqrt(numel) (before the update, stored in rms[]);  lr_t = lr * (scale_parameter ? max(eps2, RMS) : 1)
 *   u = g'^2 + eps1
 *   factored:    row = beta2t row + (1 - beta2t) mean(u, cols),  col = beta2t col + (1 - beta2t) mean(u, rows)
 *                upd = (rsqrt(row / mean(row)) [:, None] * rsqrt(col) [None, :]) * g'
 *   unfactored:  v = beta2t v + (1 - beta2t) u,  upd = rsqrt(v) * g'
 *   upd = upd / max(1, rms(upd) / clip_threshold) * lr_t;  use_beta1: m = beta1 m + (1 - beta1) upd, upd = m
 *   weight_decay != 0: p += p * (-weight_decay * lr_t);  p -= upd
 * `lr` is the relative step min(warmup_init ? 1e-6 t : 1e-2, 1 / sqrt(t)) or the external learning rate, beta2t = 1 - t^decay_rate;
 * the caller forms them (and 1 - beta2t, 1 - beta1) in double and rounds to fp32.  A tensor whose g' holds a non-finite value is
 * skipped whole: p, its statistics, m and rms[] stay as they were; the other tensors step.  Every reduction runs inside the tensor's
 * workgroup in an order fixed by its shape, no atomics: same inputs -> same bits.  p, g are indexed by `off`, m by `m`; row, col, v,
 * rms must be non-NULL (allocate one element for an unused buffer), m only with use_beta1.  Rejected with QFX_EINVAL before any
 * launch: n_tensors < 0, with n_tensors > 0 a NULL table or buffer, a negative lr, beta2t outside [0, 1), clip_threshold <= 0,
 * negative eps1 / eps2 / weight_decay, beta1 outside [0, 1).  n_tensors == 0 does nothing.  The table itself lives on the device
 * and cannot be checked here: its builder bounds rows * cols by 2^30 and every offset by its buffer. ---- */
typedef struct qfx_adafactor_tensor {
  int64_t off;           /* first element of the tensor in p / g */
  int64_t row;           /* factored: first of its `rows` elements in row */
  int64_t col;           /* factored: first of its `cols` elements in col */
  int64_t v;             /* unfactored: first of its `cols` elements in v */
  int64_t m;             /* first element in m (read only with use_beta1) */
  int32_t rows, cols;    /* the matrix; an unfactored tensor is 1 x numel */
  int32_t rms;           /* index into rms */
  int32_t factored;      /* 1: at least two dimensions */
} qfx_adafactor_tensor;
typedef struct qfx_adafactor_args {
  float* p;              /* parameters, updated in place */
  const float* g;        /* gradient (summed over ranks / micro-steps; scaled by grad_scale and the clip factor on the fly) */
  float* row;            /* exp_avg_sq_row of every factored tensor */
  float* col;            /* exp_avg_sq_col */
  float* v;              /* exp_avg_sq of every unfactored tensor */
  float* m;              /* exp_avg, may be NULL without use_beta1 */
  float* rms;            /* one RMS per tensor */
  const qfx_adafactor_tensor* table;   /* device array of n_tensors entries */
  int32_t n_tensors;
  int32_t scale_parameter, use_beta1;
  float lr, beta2t, one_minus_beta2t, eps1, eps2, clip_threshold, beta1, one_minus_beta1, weight_decay;
  const float* gnorm_sq; /* may be NULL: sum of squares of g (qfx_sumsq_det) for the global-norm clip */
  float max_norm, grad_scale;
} qfx_adafactor_args;
int qfx_adafactor_step(const qfx_adafactor_args* a, void* stream);

/* ---- CAME (Luo et al., "CAME: Confidence-guided Adaptive Memory Efficient Optimization", 2023; third party came_pytorch.CAME, the
 * optimizer LoRA fine-tuning stacks offer next to AdamW8bit, Adafactor and Prodigy; in the reference one YAML line through the generic
 * optimizer.class_path at base_trainer.py:884-909, stepped at :531 after clip_gradients :449-455).  Adafactor's factored second
 * moment, a full first moment, and a second factored pair over the instability (upd - m)^2 that rescales the momentum.  ONE launch
 * steps every tensor of the flat fp32 LoRA buffers, one workgroup per tensor, driven by a device table the caller builds once per
 * buffer layout.  Per tensor of rows x cols elements, with g' = g * clip (clip exactly as qfx_adamw_step computes it from gnorm_sq /
 * max_norm / grad_scale), everything in fp32, every operation rounded on its own (never contracted into an FMA):
 *   RMS = |p|_2 / sqrt(numel) (before the update, stored in rms[]; the package keeps it, the update does not read it)
 *   u = g'^2 + eps1
 *   factored:    row = beta2 row + (1 - beta2) mean(u, cols),  col = beta2 col + (1 - beta2) mean(u, rows)
 *                upd = (rsqrt(row / mean(row)) [:, None] * rsqrt(col) [None, :]) * g'
 *   unfactored:  v = beta2 v + (1 - beta2) u,  upd = rsqrt(v) * g'
 *   upd = upd / max(1, rms(upd) / clip_threshold);  m = beta1 m + (1 - beta1) upd
 *   factored:    res = (upd - m)^2 + eps2
 *                rrow = beta3 rrow + (1 - beta3) mean(res, cols),  rcol = beta3 rcol + (1 - beta3) mean(res, rows)
 *                out = (rsqrt(rrow / mean(rrow)) [:, None] * rsqrt(rcol) [None, :]) * m
 *   unfactored:  out = m
 *   weight_decay != 0: p += p * (-weight_decay * lr);  p -= lr * out
 * There is no relative step and no parameter scaling: lr is always external, beta2 is a constant, and lr multiplies `out` at the
 * end, not the update that enters m.  The caller forms 1 - beta1, 1 - beta2, 1 - beta3 in double and rounds to fp32.  A tensor whose
 * g' holds a non-finite value is skipped whole: p, its five statistics, m and rms[] stay as they were; the other tensors step.
 * Every reduction runs inside the tensor's workgroup in an order fixed by its shape (per-lane strided sums over groups of four
 * columns, xor-shuffle trees, fixed folds through LDS), no atomics: same inputs -> same bits.  16-byte accesses where the tensor
 * starts on a 16-byte boundary in p, g and m and cols is a multiple of 4; the order of every sum is the same without.  p, g and m
 * are indexed by `off`; every buffer must be non-NULL (allocate one element for an unused one).  Rejected with QFX_EINVAL before
 * any launch: n_tensors < 0, with n_tensors > 0 a NULL table or buffer, a negative lr, a beta or its complement outside [0, 1],
 * clip_threshold <= 0, negative eps1 / eps2 / weight_decay.  n_tensors == 0 does nothing.  The table itself lives on the device and
 * cannot be checked here: its builder bounds rows * cols by 2^30 and every offset by its buffer. ---- */
typedef struct qfx_came_tensor {
  int64_t off;           /* first element of the tensor in p / g / m */
  int64_t row;           /* factored: first of its `rows` elements in row */
  int64_t col;           /* factored: first of its `cols` elements in col */
  int64_t rrow;          /* factored: first of its `rows` elements in rrow */
  int64_t rcol;          /* factored: first of its `cols` elements in rcol */
  int64_t v;             /* unfactored: first of its `cols` elements in v */
  int32_t rows, cols;    /* the matrix; an unfactored tensor is 1 x numel */
  int32_t rms;           /* index into rms */
  int32_t factored;      /* 1: two dimensions */
} qfx_came_tensor;
typedef struct qfx_came_args {
  float* p;              /* parameters, updated in place */
  const float* g;        /* gradient (summed over ranks / micro-steps; scaled by grad_scale and the clip factor on the fly) */
  float* row;            /* exp_avg_sq_row of every factored tensor */
  float* col;            /* exp_avg_sq_col */
  float* rrow;           /* exp_avg_res_row */
  float* rcol;           /* exp_avg_res_col */
  float* v;              /* exp_avg_sq of every unfactored tensor */
  float* m;              /* exp_avg, indexed like p */
  float* rms;            /* one RMS per tensor */
  const qfx_came_tensor* table;   /* device array of n_tensors entries */
  int32_t n_tensors;
  float lr, beta1, one_minus_beta1, beta2, one_minus_beta2, beta3, one_minus_beta3, eps1, eps2, clip_threshold, weight_decay;
  const float* gnorm_sq; /* may be NULL: sum of squares of g (qfx_sumsq_det) for the global-norm clip */
  float max_norm, grad_scale;
} qfx_came_args;
int qfx_came_step(const qfx_came_args* a, void* stream);

/* ---- Lion (Chen et al., "Symbolic Discovery of Optimization Algorithms", 2023; third party lion_pytorch.Lion and
 * bitsandbytes.optim.Lion / Lion8bit / PagedLion8bit, the one-moment optimizer LoRA fine-tuning stacks offer next to the ones above;
 * in the reference one YAML line through the generic optimizer.class_path at base_trainer.py:884-909, stepped at :531 after
 * clip_gradients :449-455).  ONE launch over the flat LoRA buffers.  Per element, with g' = g * clip (clip exactly as qfx_adamw_step
 * computes it from gnorm_sq / max_norm / grad_scale), everything in fp32, 1 - b1, 1 - b2 and decay = 1 - lr wd formed in fp32:
 *   c = m b1 + (1 - b1) g'          (two products and one sum, each rounded: never contracted into an FMA, the sign of c decides)
 *   p = p decay                     (only when wd > 0: decoupled, BEFORE the update)
 *   p = p - lr sgn(c)               (sgn(0) = 0)
 *   m = m b2 + (1 - b2) g'          (the same un-contracted form)
 * An element whose g' is not finite keeps p and m unchanged.  The step count does not enter the arithmetic.
 * qfx_lion_step: m [n] in fp32, 16-byte accesses when p, g and m are 16-byte aligned.
 * qfx_lion8bit_step: bitsandbytes' blockwise 8-bit state of ONE moment, driven by the block table of qfx_adam8bit_step (same
 * struct, same builder).  8-bit block: m = qmap1[q1] * absmax1[blk] decoded, updated as above, then stored exactly as
 * qfx_adam8bit_step stores state1 -- absmax = max |m| over the block, the nearest code against the fp32 midpoints with a tie going
 * to the lower one, then the keep-the-sign rule; a block whose absmax is 0 stores the code of 0.0.  The parameter update uses the
 * fp32 m, not its re-quantised image.  fp32 entries keep their moment in m32.  Every pointer must be non-NULL (allocate one element
 * for an unused buffer); p, g, q1 are indexed by `off`, m32 by `state` of the fp32 entries; `off` and `state` are multiples of 4.
 * No atomics: same inputs -> same bits.  Rejected with QFX_EINVAL before any launch: a NULL p, g or m (8-bit: any NULL pointer but
 * gnorm_sq), n <= 0, a negative lr, a beta outside [0, 1), a negative weight_decay, and for the 8-bit entry n_blocks <= 0 or a
 * blocksize outside {256, 2048}. ---- */
int qfx_lion_step(float* p, const float* g, float* m, int64_t n, float lr, float beta1, float beta2, float weight_decay,
                  const float* gnorm_sq /* may be NULL */, float max_norm, float grad_scale, void* stream);
typedef struct qfx_lion8bit_args {
  float* p;              /* parameters, updated in place */
  const float* g;        /* gradient (summed over ranks / micro-steps; scaled by grad_scale and the clip factor on the fly) */
  uint8_t* q1;           /* state1 codes (signed map), same indexing as p */
  float* absmax1;        /* per 8-bit block */
  float* m32;            /* fp32 moment of the tensors below the 8-bit size */
  const qfx_adam8bit_block* table;   /* device array of n_blocks entries */
  int32_t n_blocks;
  int32_t blocksize;     /* 256 or 2048: the largest `len` of the table */
  const float* qmap1;    /* fp32[256] */
  float lr, beta1, beta2, weight_decay;
  const float* gnorm_sq; /* may be NULL: sum of squares of g (qfx_sumsq_det) for the global-norm clip */
  float max_norm, grad_scale;
} qfx_lion8bit_args;
int qfx_lion8bit_step(const qfx_lion8bit_args* a, void* stream);
/* parameter groups (see above); qfx_lion8bit_step_grouped ignores a->lr / beta1 / beta2 / weight_decay */
int qfx_lion_step_grouped(float* p, const float* g, float* m, int64_t n, const uint8_t* tile_group, const qfx_lion_group* groups,
                          int32_t n_groups, const float* gnorm_sq /* may be NULL */, float max_norm, float grad_scale, void* stream);
int qfx_lion8bit_step_grouped(const qfx_lion8bit_args* a, const uint8_t* block_group, const qfx_lion_group* groups, int32_t n_groups,
                              void* stream);

/* ---- Schedule-Free AdamW (Defazio et al., "The Road Less Scheduled", 2024; third party schedulefree.AdamWScheduleFree, the method
 * made for the constant learning rate the reference's configs run (lr_scheduler.scheduler_type: constant / constant_with_warmup);
 * in the reference one YAML line through the generic optimizer.class_path at base_trainer.py:884-909, stepped at :531 after
 * clip_gradients :449-455).  The parameters exist in two forms: y, where the gradient is taken (the parameter buffer in train
 * mode), and the averaged x that is sampled from and saved (the parameter buffer in eval mode); z is the base sequence.
 * qfx_sfadamw_step: ONE launch over the flat LoRA buffers.  The caller forms the group's scalars in double as the package does
 * (k counts steps from 0): lr_t = lr * min(1, (k + 1) / warmup_steps), bias_corr2 = 1 - beta2^(k + 1), lr_max = max(lr_t, lr_max),
 * weight = (k + 1)^r * lr_max^weight_lr_power, weight_sum += weight, ckp1 = weight / weight_sum (0 when weight_sum == 0).  Per
 * element, with g' = g * clip (clip exactly as qfx_adamw_step computes it from gnorm_sq / max_norm / grad_scale), everything in
 * fp32, every operation rounded on its own (never contracted into an FMA), 1 - beta2 and 1 - ckp1 formed in fp32, and
 * ylr = lr_t (beta1 (1 - ckp1) - 1) formed in double from the arguments and rounded once:
 *   v  = v beta2 + ((1 - beta2) g') g'
 *   gn = g' / (sqrt(v / bias_corr2) + eps)
 *   gn = gn + weight_decay y                  (only when weight_decay != 0)
 *   y  = lerp(y, z, ckp1)                      (torch.lerp: y + ckp1 (z - y) for |ckp1| < 0.5, else z - (z - y)(1 - ckp1))
 *   y  = y + ylr gn
 *   z  = z - lr_t gn
 * `first` != 0 on the step that creates the state: the kernel takes z = y (as it was before the step) and v = 0 instead of reading
 * them (their contents are then ignored), like qfx_sgd_step's `first`.  There is no non-finite guard: the package has none.
 * 16-byte accesses when p, g, z and v are 16-byte aligned, scalar ones otherwise and for the n % 4 tail.
 * qfx_sf_swap: p = lerp(p, z, weight), the same formula with both branches; weight = 1 - 1 / beta1 turns y into x (eval),
 * weight = 1 - beta1 turns x back into y (train).  The caller refuses beta1 == 0 (the first weight would divide by zero).
 * No atomics: same inputs -> same bits.  Rejected with QFX_EINVAL before any launch: a NULL p, g, z or v, n <= 0, a negative lr_t, a
 * beta outside [0, 1), a negative weight_decay or eps, bias_corr2 <= 0, ckp1 outside [0, 1]; for the swap a NULL p or z, n <= 0 or
 * a weight that is not finite. ---- */
int qfx_sfadamw_step(float* p, const float* g, float* z, float* v, int64_t n, float lr_t, float beta1, float beta2, float eps,
                     float weight_decay, float bias_corr2, float ckp1, int32_t first, const float* gnorm_sq /* may be NULL */,
                     float max_norm, float grad_scale, void* stream);
int qfx_sf_swap(float* p, const float* z, int64_t n, float weight, void* stream);

/* ---- Muon (Jordan et al., "Muon: An optimizer for hidden layers in neural networks", 2024; torch.optim.Muon, the one mainstream
 * optimizer defined per MATRIX; in the reference one YAML line through the generic optimizer.class_path at base_trainer.py:884-909,
 * stepped at :531 after clip_gradients :449-455).  ONE launch, one workgroup per adapter matrix, driven by a device table.  Per
 * matrix [rows, cols] (row-major at `off` in p / g / buf), with g' = g * clip (clip exactly as qfx_adamw_step computes it from
 * gnorm_sq / max_norm / grad_scale) and lerp(x, y, w) = w < 0.5 ? fma(w, y - x, x) : fma(w - 1, y - x, y) (ATen's lerp), the
 * rounding points of torch.optim.Muon:
 *   buf = lerp(buf, g', 1 - momentum)                                    fp32; 1 - momentum formed in double by the caller
 *   u   = nesterov ? lerp(g', buf, momentum) : buf                       fp32
 *   X   = bf16(u), transposed when rows > cols: X is [s, n], s = min(rows, cols) <= 96
 *   X   = bf16(X / max(bf16(sqrt(sum X^2)), bf16(eps)))                  the sum in fp32
 *   ns_steps times:  G = bf16(X X^T);  H = bf16(b G + c (G G));  X = bf16(a X + H X)
 *                    bf16 operands, fp32 accumulation (v_mfma_f32_16x16x32_bf16; s padded to a multiple of 16 and n to a multiple
 *                    of 32 by zeros, which change no sum)
 *   p   = fma(-(lr lr_ratio), O, p (1 - lr weight_decay))                fp32; O = X, transposed back
 * g' is rounded to fp32 before it is used (the file is compiled without FMA contraction): a clipped step equals a step on the
 * pre-scaled gradient bit for bit.
 * lr_ratio is torch's _adjust_lr per matrix: sqrt(max(1, rows / cols)) ("original" / None) or 0.2 sqrt(max(rows, cols))
 * ("match_rms_adamw").  An all-zero g' gives O = 0 exactly (only the decay moves p).  A matrix whose g' holds a non-finite value is
 * skipped whole: p and buf stay as they were; the other matrices step.  X lives in LDS when its padded image takes at most 96 KB
 * ([16, 3072] exactly) and otherwise in this workgroup's slot of the bf16 workspace `ws`, which the caller allocates with
 * qfx_muon_ws_bytes(host copy of the table, n_tensors) bytes (0 when every matrix fits LDS; QFX_EINVAL for a table with a matrix
 * whose short side exceeds 96, with rows * cols > 2^30 or with a negative offset).  A matrix that fits neither LDS nor the slot
 * ws_bytes provides, or that the builder would have refused, is left unchanged: the kernel never writes past a slot.  No atomics,
 * nothing crosses a workgroup, every sum runs in an order fixed by the shape: same inputs -> same bits.  Rejected with QFX_EINVAL
 * before any launch: n_tensors < 0, with n_tensors > 0 a NULL table, p, g or buf, a NULL or unaligned (16 B) ws with ws_bytes > 0,
 * a negative lr, weight_decay or momentum, ns_steps outside [0, 100), eps <= 0.  n_tensors == 0 does nothing. ---- */
typedef struct qfx_muon_tensor {
  int64_t off;           /* first element of the matrix in p / g / buf */
  int32_t rows, cols;
  float lr_ratio;        /* adjusted lr = lr * lr_ratio */
  int32_t reserved;      /* 0 */
} qfx_muon_tensor;
typedef struct qfx_muon_args {
  float* p;              /* parameters, updated in place */
  const float* g;        /* gradient (summed over ranks / micro-steps; scaled by grad_scale and the clip factor on the fly) */
  float* buf;            /* momentum buffer, indexed like p */
  uint16_t* ws;          /* bf16 workspace, may be NULL with ws_bytes == 0 */
  int64_t ws_bytes;      /* bytes allocated behind ws */
  const qfx_muon_tensor* table;   /* device array of n_tensors entries */
  int32_t n_tensors;
  int32_t nesterov, ns_steps;
  float lr, weight_decay, momentum, one_minus_momentum;
  float a, b, c;         /* ns_coefficients */
  float eps;
  const float* gnorm_sq; /* may be NULL: sum of squares of g (qfx_sumsq_det) for the global-norm clip */
  float max_norm, grad_scale;
} qfx_muon_args;
int64_t qfx_muon_ws_bytes(const qfx_muon_tensor* host_table, int32_t n_tensors);
int qfx_muon_step(const qfx_muon_args* a, void* stream);

/* ---- runtime: a HIP stream confined to the first `n_cus` bits of the driver's CU mask (consecutive bits walk the 8 XCDs first, so
 * 16 = two CUs per XCD).  The persistent GEMM grids occupy 240 of the 256 CUs; leaf work of the backward (the LoRA weight-gradient
 * launches, which the reference's autograd also schedules off the dX critical path) runs here without ever taking a CU a GEMM block
 * is waiting for.  Streams are plain hipStream_t handles; destroy with qfx_stream_destroy. ---- */
#define QFX_NUM_CU_TOTAL 256
int qfx_stream_create_cu_masked(int32_t n_cus, void** stream_out);
int qfx_stream_destroy(void* stream);
/* debug: out[2*b] = HW_ID register, out[2*b+1] = XCC_ID register of the CU block b ran on (blocks spin ~0.1 ms) */
int qfx_debug_where(uint32_t* out, int32_t n_blocks, void* stream);

/* ---- tuning: tile-geometry policy of the persistent GEMM (qfx_gemm_grouped / large qfx_gemm_bf16; ABI 5).  Every launch picks
 * its tile from rounds-over-256-CUs x relative tile time among the enabled geometries "256x128", "256x256" (rounds 1-3) and
 * "160x192" (round 4: M = 2048 image + 384 text rows tile into 13 + 3 M-tiles of 160 x 16 N-tiles = one whole round of 256 tiles).
 * tiles: NULL / "" = keep, "all", "legacy" (the two 256-row tiles), or a comma list of names; eff: NULL = keep, or three
 * comma-separated per-flop efficiencies relative to 256x128 in the order above.  Process-wide; the defaults come from the
 * environment (QFX_GEMM_TILES / QFX_GEMM_EFF) at the first launch.  Results do not depend on the geometry (same K order per
 * output element); only speed does.  Returns QFX_EINVAL for an unparsable argument.
 * Round 5: `tiles` also takes ONE policy token of the same-XCD split-K lever instead of a geometry list -- "splitk=0|1" (default 0),
 * "splitk_mink=<smallest base K taken, >= 2048>", "splitk_bias=<0..16 K tiles>" (environment: QFX_GEMM_SPLITK, _MINK, _BIAS).  With the
 * lever on, a launch whose problems all have N % 256 == 0 and K1 >= mink and whose 256x256 tiles make 218..256 work items in pairs
 * runs as two work items per tile (fp32 partial tiles through a per-stream workspace the library allocates on first use; never while the
 * stream is capturing a graph).  The fp32 summation order changes (results stay within the bf16 tolerance of the tests, run-to-run
 * bit-identical); measured slower than the unsplit launch on MI355X (profiles/r05_gemm_splitk.json): an A/B lever, not a default. ---- */
int qfx_gemm_tune(const char* tiles, const char* eff);

/* ---- debug: lane mapping of ds_read_b64_tr_b16 (64 lanes x 4 bf16 in, same out) ---- */
int qfx_debug_tr_read(const uint16_t* in, uint16_t* out, void* stream);

/* ---- misc ---- */
int qfx_abi_version(void);
const char* qfx_build_arch(void);

/* ---- EMA of the adapter weights (diffusers.training_utils.EMAModel, every diffusers training script's --use_ema): up to
 * QFX_EMA_MAX_SHADOWS fp32 shadow buffers over the flat LoRA buffer p, each with its own rate.  The caller forms the decay of the
 * step on the host (EMAModel.get_decay: qflux_amd.ema.get_decay) and passes one_minus_decay = float32(1 - decay).
 * qfx_ema_update: ONE launch, for k < n_shadows
 *   s_k[i] = s_k[i] - omd_k * (s_k[i] - p[i])      three separately rounded fp32 operations, in this order
 * (EMAModel.step's `s.sub_(one_minus_decay * (s - p))`; never contracted into an FMA); p is read once for all shadows and never
 * written.  omd == 1 is not special: the result is s - (s - p), what the package computes.  4 + 8 n_shadows bytes per element.
 * qfx_ema_swap: exchanges the contents of p and s bit for bit (NaN payloads and -0.0 included; the words move as integers),
 * 16 bytes per element.  16-byte accesses when every buffer of the call is 16-byte aligned, scalar ones otherwise and for the n % 4
 * tail.  The shadow pointers and rates travel by value in the kernel argument block: there is no device-side table.  No atomics:
 * same inputs -> same bits.  Rejected with QFX_EINVAL before any launch: a NULL p or a, n_shadows outside 1..4, n < 0, below
 * n_shadows a NULL shadow pointer, a shadow pointer equal to p or to an earlier shadow's, a one_minus_decay outside [0, 1] or NaN;
 * for the swap a NULL p or s, p == s, n < 0.  n == 0 returns QFX_OK without a launch. ---- */
#define QFX_EMA_MAX_SHADOWS 4
typedef struct qfx_ema_args {
  float*  shadow[QFX_EMA_MAX_SHADOWS];          /* n elements each, distinct from p and from each other */
  float   one_minus_decay[QFX_EMA_MAX_SHADOWS];
  int32_t n_shadows;                            /* 1..4 */
} qfx_ema_args;
int qfx_ema_update(const float* p, int64_t n, const qfx_ema_args* a, void* stream);
int qfx_ema_swap(float* p, float* s, int64_t n, void* stream);

/* ---- general flow-matching criterion: per-sample weights (diffusers' compute_loss_weighting_for_sd3), per-token weights (edit mask,
 * attention mask), L2 or kohya's pseudo-Huber / smooth-L1 with a per-sample threshold c, and the loss of every sample.  With
 * d = pred - target in fp32 (rows s < S_t of pred enter):
 *   loss_per_sample[b] = B * inv_denom * sum_{s<S_t} token_w[b,s] * (1/C) * sum_c rho_b(d[b,s,c])
 *   loss               = (1/B) * sum_b sample_w[b] * loss_per_sample[b]
 *   dpred[b,s,c]       = bf16( rho_b'(d) * sample_w[b] * token_w[b,s] * (1/C) * inv_denom * gscale ),  0 for rows s >= S_t
 *   QFX_LOSS_L2         rho = d^2                        rho' = 2 d
 *   QFX_LOSS_HUBER      rho = 2 c (sqrt(d^2 + c^2) - c)  rho' = 2 c d / sqrt(d^2 + c^2)
 *   QFX_LOSS_SMOOTH_L1  rho = 2 (sqrt(d^2 + c^2) - c)    rho' = 2 d / sqrt(d^2 + c^2)
 * inv_denom = 1/(B S_t): MseLoss with a [B,1,1] weighting (losses/mse_loss.py:66-83), and MaskEditLoss with token_w = the edit
 * weights; token_w = attention mask * edit weight and inv_denom = 1/(n_valid + eps): AttentionMaskMseLoss(reduction="mean") with
 * weighting.  sample_w [B] and token_w [B,S_t] fp32, NULL = ones; huber_c [B] fp32, required unless kind is L2, every value > 0 and
 * finite (the caller checks on the host).  loss (fp32 scalar) and loss_per_sample ([B] fp32, may be NULL) are WRITTEN, not
 * accumulated; dpred [B,S_all,C] bf16 may be NULL.
 * The gradient is fp32, each operation rounded, the factors multiplied from left to right as written above with 1/C =
 * float(1)/float(C); r = sqrt(d*d + c*c), rho' = (2c*d)/r resp. (2*d)/r, correctly rounded divide and square root, no FMA.
 * sqrt(d^2 + c^2) - c is formed as d^2 / (r + c).  The loss terms are those fp32 rho values, added in fp64: per (sample, chunk of
 * rows) into `workspace` (qfx_criterion_workspace_bytes(B, S_t, C) bytes, 8-byte aligned, need not be zeroed), then by a second
 * one-block launch in chunk order and in sample order -- no floating-point atomics, same inputs -> same bits.  16-byte accesses
 * when C % 8 == 0 and pred, target and dpred are 16-byte aligned, scalar ones otherwise; any C >= 1, 1 <= S_t <= S_all, B >= 1.
 * Rejected with QFX_EINVAL before any launch: a NULL args, pred, target, loss or workspace, a non-positive dimension, S_t > S_all,
 * an unknown kind, kind != L2 with a NULL huber_c, workspace_bytes below the query's answer.  The query returns 0 for a
 * non-positive dimension. ---- */
#define QFX_LOSS_L2 0
#define QFX_LOSS_HUBER 1
#define QFX_LOSS_SMOOTH_L1 2
typedef struct qfx_criterion_args {
  const uint16_t* pred;            /* [B, S_all, C] bf16 */
  const uint16_t* target;          /* [B, S_t, C] bf16 */
  const float*    sample_w;        /* [B] or NULL */
  const float*    token_w;         /* [B, S_t] or NULL */
  const float*    huber_c;         /* [B]; NULL allowed with QFX_LOSS_L2 only */
  float*          loss;            /* scalar, written */
  float*          loss_per_sample; /* [B] or NULL, written */
  uint16_t*       dpred;           /* [B, S_all, C] bf16 or NULL */
  void*           workspace;
  int64_t         workspace_bytes;
  int32_t         B, S_all, S_t, C;
  int32_t         kind;            /* QFX_LOSS_* */
  float           inv_denom, gscale;
} qfx_criterion_args;
int64_t qfx_criterion_workspace_bytes(int32_t B, int32_t S_t, int32_t C);
int qfx_criterion_fwd_bwd(const qfx_criterion_args* a, void* stream);

/* ---- max-norm regularisation of the adapters (kohya's --scale_weight_norms: LoRANetwork.apply_max_norm_regularization) over the
 * flat LoRA buffer p, behind the optimizer's launch.  Per adapter pair, A = lora_A.weight [r, in], B = lora_B.weight [out, r],
 * s = scale (lora_alpha / r, as fp32), m = max_norm:
 *   norm_raw    = float32(|s| * sqrt(sum_ij (A A^T)_ij (B^T B)_ij))   = ||s B A||_F; the product B A is never formed.  Both r x r
 *                 Gram matrices and their contraction are accumulated in fp64 from the widened fp32 weights (every product exact),
 *                 |s| * sqrt(.) is formed in fp64 and rounded ONCE to fp32; a sum that rounding left below 0 counts as 0
 *   ratio       = norm_raw > m ? m / norm_raw : 1                     one correctly rounded fp32 divide
 *                 (kohya's clamp(norm, min = m / 2), clamp(max = m) / norm: 1 when norm_raw <= m, else m / norm_raw)
 *   q           = sqrtf(ratio)                                        one correctly rounded fp32 square root
 *   A *= q, B *= q  when ratio != 1                                   one fp32 multiply per element; a pair with norm_raw <= m is
 *                                                                     not written at all
 *   norms[pair] = norm_raw * ratio                                    one fp32 multiply;  ratios[pair] = ratio
 *   summary     = { keys_scaled = the number of pairs with ratio != 1 (an integer count, written as fp32),
 *                   float32((fp64 sum of norms[] in pair order) / n_pairs),  the fp32 maximum of norms[] (a NaN is kept),  0 }
 * B = 0 (every adapter before the first step) gives norm_raw = 0, ratio = 1 and untouched weights.  A pair whose norm_raw is not
 * finite is left untouched and reported with ratio = 1 and its non-finite norm; the other pairs proceed (kohya multiplies by the
 * NaN; this is the Muon step's skip rule).  max_norm = +inf measures only: nothing is written to p, the statistics are produced.
 * ONE launch of one 256-lane workgroup per pair (any number of pairs), driven by the device table, then a second one-block launch
 * that writes summary from norms / ratios in pair order.  A and B stream through LDS tiles; each lane owns a fixed block of the
 * Gram matrices' upper triangle in fp64 registers; the workgroup folds in an order fixed by the shape.  No atomics, nothing crosses
 * a workgroup: same inputs -> same bits.  16-byte accesses where the addresses and lengths allow (the tiles: A 16-byte aligned and
 * in % 4 == 0, B 16-byte aligned and r % 4 == 0; the scaling: everything between the first and the last 16-byte boundary), scalar
 * ones otherwise.  1 <= r <= 128, 1 <= in, out <= 2^24, any offsets.
 * qfx_maxnorm_check_table runs on a HOST copy of the table: QFX_EINVAL for n_pairs < 0, n_elems < 0, a NULL table with n_pairs > 0,
 * r outside 1..128, in or out outside 1..2^24, a negative offset, a matrix that reaches past n_elems, two matrices of the table
 * that overlap, a non-finite scale.  The kernel skips a pair with such dimensions or offsets (norm 0, ratio 1), it does not check
 * extents: launch only tables that passed.  qfx_maxnorm_apply rejects with QFX_EINVAL before any launch: a NULL args, n_pairs < 0,
 * a max_norm that is NaN or <= 0, with n_pairs > 0 a NULL p, table, norms, ratios or summary.  n_pairs == 0 returns QFX_OK without
 * a launch. ---- */
typedef struct qfx_maxnorm_pair {     /* 32 bytes */
  int64_t off_a, off_b;               /* first element of A [r, in] / B [out, r], row-major, in p */
  int32_t r, in_features, out_features;
  float   scale;                      /* lora_alpha / r */
} qfx_maxnorm_pair;
typedef struct qfx_maxnorm_args {
  float* p;                           /* flat adapter weights, scaled in place */
  const qfx_maxnorm_pair* table;      /* device array */
  int32_t n_pairs;
  float   max_norm;                   /* > 0, +inf allowed */
  float*  norms;                      /* [n_pairs] scaled_norm, written */
  float*  ratios;                     /* [n_pairs] ratio, written */
  float*  summary;                    /* [4]: keys_scaled, mean, max, 0 -- written */
} qfx_maxnorm_args;
int qfx_maxnorm_check_table(const qfx_maxnorm_pair* host_table, int32_t n_pairs, int64_t n_elems);
int qfx_maxnorm_apply(const qfx_maxnorm_args* a, void* stream);

/* ---- Dropout on the rank-r activation of the adapters (kohya LoRAModule.forward: `dropout` = network_dropout, F.dropout on
 * lx = lora_down(x); `rank_dropout`, one keep / drop draw per sample and rank, broadcast over tokens, survivors scaled by
 * 1 / (1 - p)).  Appended under ABI 7: new structs and entry points only.
 * With u = x A^T [tokens, r] the adapted linear becomes y = base(x) + (f * u) (sB)^T and its backward v = f * (dy sB),
 * dB += dy^T (f * u), dA += v^T x, dX += v A, with the SAME factor f[token, rank] in both passes: 0 where the element or its rank is
 * dropped, `scale` where it is kept.  So the outputs of a rank-r producer (qfx_lora_down[_batch], qfx_ln_down_fwd,
 * qfx_lora_head_reduce) are multiplied by f in place, after the producer and before the first consumer, and every consumer (the
 * K-extension GEMMs, qfx_lora_grad) runs unchanged.  The mask is never stored: both passes regenerate it from the counters below.
 *
 * state: 8 device words  { seed_lo, seed_hi, step, active, thr_elem, thr_rank, scale (fp32 bits), sample0 }.
 *   thr = floor(p * 2^32), formed on the host; a draw is KEPT iff its 32-bit word >= thr (thr == 0: that option is off, nothing is
 *   drawn for it);  scale = float32(1 / ((1 - p_elem) (1 - p_rank))), formed in double on the host.
 * Generator: Philox4x32-10 (Random123: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85, 10 rounds),
 *   key = (seed_lo, seed_hi), counter (c0, c1, c2, c3):
 *     c3 = site    a 32-bit key of the adapter: zlib.crc32 of the adapted module's qualified name ("transformer_blocks.3.attn.to_q")
 *     c2 = step
 *     c1 = sample0 + m / rows_per_batch                    the global sample index (data-parallel rank k passes sample0 = k * B)
 *     element draw:  c0 = (m % rows_per_batch) * 32 + j' / 4      the four output words serve ranks 4q .. 4q+3 of the adapter
 *     rank draw:     c0 = 0xFFFFFFE0 + j' / 4                     (the same for every token of the sample)
 *   with m the row of the problem and j' = j % group_R the rank within its adapter (so group_R <= 128, rows_per_batch < 2^27 - 1).
 *   f = keep_elem && keep_rank ? scale : 0.
 * qfx_lora_dropout_apply: n <= QFX_MAX_BATCH problems in ONE launch; one problem = the outputs of one producer call, addressed by
 *   the fields of the same names in qfx_lora_down_args (Ut_hi / Ut_lo required, ext may be NULL); site[g] keys group g = j / group_R
 *   (the fused q | k | v call carries three adapters).  For row m < M and column j < R:
 *     u = float(Ut_hi[j][m]) + float(Ut_lo[j][m]);  u' = f == 0 ? +0 : u * f (one fp32 multiply);  hi' = bf16_rne(u'), lo' = bf16_rne(u' - hi')
 *   (the split of qfx_lora_down) written back to Ut_hi / Ut_lo and as [hi' | lo' | hi'] to the three ext images of the group.  A dropped
 *   element becomes exact zeros; padded ranks (zero) stay zero; Ut columns >= M are not touched.  The launch returns at once,
 *   uniformly, when active == 0 or both thresholds are 0, so a captured graph honours an eval() without being captured again.
 *   QFX_EINVAL before any launch: NULL list / state, n outside 1..QFX_MAX_BATCH, M <= 0, R <= 0 or R % 16 or R > 96, group_R <= 0 or
 *   group_R % 16 or R % group_R or group_R > 128 or more than 3 groups, rows_per_batch <= 0 or >= 2^27 - 1, NULL Ut_hi / Ut_lo,
 *   ld_ut < M, and with ext: ext not 8-byte aligned, ld_ext % 4, group_stride % 4 or < 0, ld_ext short of the last group's images.
 * qfx_lora_dropout_advance: state.step += 1 when state.active != 0, on the device (a one-lane launch): the first call of a forward
 *   program, so that eager and captured replays advance alike and an evaluation forward does not consume training masks.
 * qfx_lora_dropout_factors_host: HOST only, no GPU call -- out[0 .. r) = f of the token (local sample b, token t of the sample,
 *   ranks 0 .. r-1) of adapter `site` under a host copy of the state, through the same inline function the kernel calls (`active`
 *   is not consulted).  QFX_EINVAL for a NULL pointer, b < 0, t < 0 or t >= 2^27 - 1, r outside 1..128. ---- */
typedef struct qfx_lora_dropout_args {
  uint16_t* ext; int64_t ld_ext;
  uint16_t* Ut_hi; uint16_t* Ut_lo; int64_t ld_ut;
  int32_t M; int32_t R; int32_t group_R; int32_t group_stride; int32_t rows_per_batch;
  uint32_t site[3];
} qfx_lora_dropout_args;
int qfx_lora_dropout_apply(const qfx_lora_dropout_args* list, int32_t n, const uint32_t* state, void* stream);
int qfx_lora_dropout_advance(uint32_t* state, void* stream);
int qfx_lora_dropout_factors_host(const uint32_t* state, uint32_t site, int32_t b, int32_t t, int32_t r, float* out);

/* ---- torch.optim.RAdam / NAdam / Adamax over the flat fp32 LoRA buffers (csrc/qfx_adamx.hip): ONE entry, ONE launch, the variant
 * chosen per launch.  The specification is torch's single-tensor implementation (_single_tensor_radam, _single_tensor_nadam,
 * _single_tensor_adamax): its fp32 tensor operations in its order, one rounding each (the file is built without FMA contraction;
 * lerp_, add(alpha=) and addcmul_ are the fused multiply-adds torch's CPU kernels issue).  Every per-step scalar torch forms as a
 * Python float is formed by the CALLER in double and passed in the group's row as a float: nothing synchronises.  With
 * t = the step count (from 1), b1 = beta1, b2 = beta2, g' = g * clip (the clip prologue of qfx_adamw_step: gnorm_sq / max_norm /
 * grad_scale, applied before weight decay) and lerp(a, b, w) = a + w (b - a) for |w| < 0.5, b - (b - a)(1 - w) otherwise:
 *   all      weight_decay != 0:  decoupled (RAdam, NAdam only):  p *= decay          decay = 1 - lr weight_decay
 *                                 otherwise (L2):                 g' += weight_decay p
 *            exp_avg = lerp(exp_avg, g', one_minus_beta1)
 *   RAdam    state2 = exp_avg_sq = beta2 exp_avg_sq + (one_minus_beta2 g') g'
 *            u = (exp_avg / bias_corr1) lr                                             bias_corr1 = 1 - b1^t
 *            rectified:  u = (u ((1 / (sqrt(exp_avg_sq) + eps)) sqrt_bias_corr2)) rect   sqrt_bias_corr2 = sqrt(1 - b2^t)
 *            p -= u
 *              rho_inf = 2 / (1 - b2) - 1,  rho_t = rho_inf - 2 t b2^t / (1 - b2^t),  rectified = rho_t > 5,
 *              rect = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
 *   NAdam    state2 = exp_avg_sq as RAdam's;  den = sqrt(exp_avg_sq / bias_corr2) + eps      bias_corr2 = 1 - b2^t
 *            p += (c_grad g') / den;  p += (c_avg exp_avg) / den
 *              mu_t = b1 (1 - 0.5 * 0.96^(t momentum_decay)),  mu_product_t = mu_product_{t-1} mu_t (torch keeps it in fp32),
 *              c_grad = -lr (1 - mu_t) / (1 - mu_product_t),  c_avg = -lr mu_{t+1} / (1 - mu_product_t mu_{t+1})
 *   Adamax   state2 = exp_inf = max(beta2 exp_inf, |g'| + eps);  p += (neg_clr exp_avg) / exp_inf     neg_clr = -lr / (1 - b1^t)
 * A row holds every field; a variant reads its own (the others are ignored).  The entry is always grouped (parameter groups, see
 * qfx_adamw_step_grouped): groups = HOST array of 1..QFX_MAX_PARAM_GROUPS rows, tile_group = device uint8[ceil(n / 64)], which may be
 * NULL when n_groups == 1; a map entry >= n_groups steps its tile with the last row.  16-byte accesses when p, g, exp_avg and
 * state2 are 16-byte aligned, scalar ones otherwise; a grid-stride loop; no atomics: same inputs -> same bits, and every tensor gets
 * the bits a one-group launch with its row gives it.  maximize / differentiable / capturable are not implemented (the callers
 * refuse them).
 * QFX_EINVAL before any launch: NULL args / p / g / exp_avg / state2 / groups, n <= 0, an unknown variant, n_groups outside
 * 1..QFX_MAX_PARAM_GROUPS, a NULL tile_group with n_groups > 1, a row with a negative lr, eps or weight_decay or a beta outside
 * [0, 1), RAdam with bias_corr1 <= 0, NAdam with bias_corr2 <= 0. ---- */
enum { QFX_ADAMX_RADAM = 0, QFX_ADAMX_NADAM = 1, QFX_ADAMX_ADAMAX = 2 };
typedef struct qfx_adamx_group {
  float lr, beta1, beta2, eps, weight_decay;
  float one_minus_beta1, one_minus_beta2;      /* float(1 - b1), float(1 - b2): the weights torch hands lerp_ / addcmul_ */
  float decay;                                 /* float(1 - lr weight_decay); read with decoupled != 0 */
  float bias_corr1, bias_corr2;                /* RAdam: bias_corr1; NAdam: bias_corr2 */
  float sqrt_bias_corr2, rect;                 /* RAdam, read with rectified != 0 */
  float c_grad, c_avg;                         /* NAdam */
  float neg_clr;                               /* Adamax */
  int32_t decoupled;                           /* decoupled_weight_decay (RAdam, NAdam) */
  int32_t rectified;                           /* RAdam: rho_t > 5 */
  int32_t reserved;
} qfx_adamx_group;
typedef struct qfx_adamx_args {
  float* p; const float* g; float* exp_avg; float* state2;      /* state2: exp_avg_sq (RAdam, NAdam) or exp_inf (Adamax) */
  int64_t n;
  int32_t variant;                             /* QFX_ADAMX_* */
  int32_t n_groups;
  const qfx_adamx_group* groups;               /* HOST */
  const uint8_t* tile_group;                   /* device; may be NULL when n_groups == 1 */
  const float* gnorm_sq;                       /* may be NULL */
  float max_norm, grad_scale;
} qfx_adamx_args;
int qfx_adamx_step(const qfx_adamx_args* a, void* stream);

/* ---- AdEMAMix (Pagliardini et al., "The AdEMAMix Optimizer: Better, Faster, Older", 2024; third party bitsandbytes.optim.AdEMAMix /
 * AdEMAMix32bit / AdEMAMix8bit and their Paged forms, one YAML line through the generic optimizer.class_path of the reference) over
 * the flat LoRA buffers (csrc/qfx_ademamix.hip): Adam with a second, slow gradient average.  Three states -- the fast average m1,
 * the slow average m2, Adam's nu -- and two hyperparameters that move every step.  THE LISTING BELOW IS THE SPECIFICATION, not the
 * package: it restates what bitsandbytes' 32-bit AdEMAMix kernel is understood to compute (a decoupled multiplicative decay after
 * the update, eps outside the corrected root) and was written without a copy of bitsandbytes at hand; tests/ademamix_ref.py
 * restates it in numpy.  Per element, every operation rounding once in fp32, in this order (the file is built without FMA
 * contraction), with g' = g * clip (the clip prologue of qfx_adamw_step: gnorm_sq / max_norm / grad_scale):
 *   m1 = m1 beta1   + one_minus_beta1 g'
 *   m2 = m2 beta3_t + one_minus_beta3_t g'
 *   nu = nu beta2   + (one_minus_beta2 g') g'
 *   p  = p - lr ((m1 / bias_corr1 + alpha_t m2) / (sqrtf(nu) / sqrt_bias_corr2 + eps))
 *   p  = p decay                           only when weight_decay > 0;  decay = float(1 - lr weight_decay)
 * bias_corr1 = 1 - beta1^t, sqrt_bias_corr2 = sqrt(1 - beta2^t), t the step count from 1; the slow average gets no bias correction.
 * Every per-step scalar is formed by the CALLER in double and rounded to float in the group's row; nothing synchronises.  The two
 * schedules, per group and per step (t_alpha / t_beta3 absent: the constants alpha / beta3):
 *   alpha_t = min(t alpha / t_alpha, alpha)
 *   beta3_t = min(exp(ln(beta1) ln(beta3) / ((1 - s) ln(beta3) + s ln(beta1))), beta3),  s = t / t_beta3
 * An element whose g' is not finite keeps p and all three states (as in qfx_adam8bit_step).  No atomics: same inputs -> same bits,
 * and every tensor gets the bits a one-group launch with its row gives it.
 * qfx_ademamix_step: m1, m2, nu [n] in fp32; always grouped (parameter groups, see qfx_adamw_step_grouped): groups = HOST array of
 * 1..QFX_MAX_PARAM_GROUPS rows, tile_group = device uint8[ceil(n / 64)], which may be NULL when n_groups == 1; a map entry >=
 * n_groups steps its tile with the last row.  16-byte accesses when p, g, m1, m2 and nu are 16-byte aligned, scalar ones otherwise;
 * a grid-stride loop.
 * qfx_ademamix8bit_step / _grouped: bitsandbytes' blockwise 8-bit state, driven by the block table of qfx_adam8bit_step (same
 * struct, same builder, same grid policy).  state1 holds BOTH averages as two planes of signed-map codes: q1[2][q1_plane] (plane 0 =
 * m1, plane 1 = m2, each indexed like p) with absmax1[2][absmax1_plane]; nu is unsigned-map codes q2 with absmax2.  8-bit block:
 * the three states decoded (qmap[code] * absmax), updated as above, then stored exactly as qfx_adam8bit_step stores its states --
 * per plane absmax = max |state| over the block, the nearest code against the fp32 midpoints with a tie going to the lower one, the
 * keep-the-sign rule for the two planes of state1; a block whose absmax is 0 stores the code of 0.0.  The parameter update uses the
 * fp32 states, not their re-quantised images.  fp32 entries (tensors below min_8bit_size) keep m32[2][m32_plane] and v32.  Every
 * pointer must be non-NULL (allocate for an unused buffer); `off`, `state`, q1_plane and m32_plane are multiples of 4.  The
 * ungrouped entry reads the row a->hp; the grouped one ignores it and takes groups[block_group[bi]] for table entry bi.
 * QFX_EINVAL before any launch: a NULL args / buffer / groups pointer (gnorm_sq and, with one group, tile_group may be NULL), n <= 0,
 * n_groups outside 1..QFX_MAX_PARAM_GROUPS, a NULL tile_group with n_groups > 1, a row with a negative lr, eps, weight_decay or
 * alpha_t, with beta1, beta2 or beta3_t outside [0, 1), or with bias_corr1 <= 0; for the 8-bit entries also n_blocks <= 0, a
 * blocksize outside {256, 2048}, a NULL block_group (grouped) and a plane stride that is not positive or (q1, m32) no multiple of 4. ---- */
typedef struct qfx_ademamix_group {           /* 64 bytes */
  float lr, beta1, beta2, eps, weight_decay;
  float one_minus_beta1, one_minus_beta2;      /* float(1 - beta1), float(1 - beta2) */
  float beta3_t, one_minus_beta3_t;            /* the slow average's rate at this step and float(1 - beta3_t) */
  float alpha_t;                               /* the slow average's weight at this step */
  float bias_corr1, sqrt_bias_corr2;
  float decay;                                 /* float(1 - lr weight_decay); read with weight_decay > 0 */
  int32_t reserved[3];
} qfx_ademamix_group;
typedef struct qfx_ademamix_args {
  float* p; const float* g; float* m1; float* m2; float* nu;
  int64_t n;
  int32_t n_groups;
  int32_t reserved;
  const qfx_ademamix_group* groups;            /* HOST */
  const uint8_t* tile_group;                   /* device; may be NULL when n_groups == 1 */
  const float* gnorm_sq;                       /* may be NULL */
  float max_norm, grad_scale;
} qfx_ademamix_args;
int qfx_ademamix_step(const qfx_ademamix_args* a, void* stream);
typedef struct qfx_ademamix8bit_args {
  float* p;              /* parameters, updated in place */
  const float* g;        /* gradient (summed over ranks / micro-steps; scaled by grad_scale and the clip factor on the fly) */
  uint8_t* q1;           /* state1 codes (signed map), two planes: m1 at q1, m2 at q1 + q1_plane, each indexed like p */
  uint8_t* q2;           /* state2 codes (unsigned map): nu */
  float* absmax1;        /* per 8-bit block, two planes: absmax1 and absmax1 + absmax1_plane */
  float* absmax2;
  float* m32;            /* fp32 m1 / m2 of the tensors below the 8-bit size, two planes: m32 and m32 + m32_plane */
  float* v32;            /* fp32 nu of those tensors */
  int64_t q1_plane, absmax1_plane, m32_plane;      /* elements between the two planes */
  const qfx_adam8bit_block* table;   /* device array of n_blocks entries */
  int32_t n_blocks;
  int32_t blocksize;     /* 256 or 2048: the largest `len` of the table */
  const float* qmap1;    /* fp32[256] */
  const float* qmap2;    /* fp32[256] */
  qfx_ademamix_group hp; /* the one row of the ungrouped entry */
  const float* gnorm_sq; /* may be NULL: sum of squares of g (qfx_sumsq_det) for the global-norm clip */
  float max_norm, grad_scale;
} qfx_ademamix8bit_args;
int qfx_ademamix8bit_step(const qfx_ademamix8bit_args* a, void* stream);
int qfx_ademamix8bit_step_grouped(const qfx_ademamix8bit_args* a, const uint8_t* block_group, const qfx_ademamix_group* groups,
                                  int32_t n_groups, void* stream);

/* ---- Per-adapter training telemetry over the flat LoRA buffers (csrc/qfx_adapter_stats.hip): what a training log asks of every
 * adapter tensor -- its gradient norm, its weight norm, how far the last optimizer step moved it and whether anything in it is
 * not finite -- in two launches that bracket the optimizer's, instead of a host loop of .norm().item() over ~1400 views.
 * `table` (device) names the tensors: entry e covers elements off .. off + numel - 1 of p, g and prev; `out` (device) takes one
 * 32-byte row per entry.  One 256-lane workgroup per entry (blockIdx.x is the entry; more than 4096 entries are walked by stride).
 *   phase 0, before the optimizer's launch: with g' = g * clip, clip the prologue of qfx_adamw_step (gnorm_sq / max_norm /
 *     grad_scale: the reported gradient is the one the optimizer steps with; gnorm_sq NULL and grad_scale 1 give clip = 1 exactly),
 *       grad_sq = sum g'^2, grad_absmax = max |g'|, grad_nonfinite = the number of g' that are NaN or +-inf,
 *     and prev[off ..] = p[off ..] bit for bit, in the same sweep (elements of prev between the tensors are not written).  Phase 0
 *     writes the WHOLE row: weight_sq, update_sq, weight_nonfinite, r0 and r1 are set to 0.
 *   phase 1, behind the optimizer's launch: weight_sq = sum p^2, weight_nonfinite = the number of p that are NaN or +-inf,
 *     update_sq = sum (p - prev)^2 with the difference rounded to fp32; the other fields of the row are not written.
 * An element that is not finite (g' in phase 0; p, respectively p - prev, in phase 1) is counted, adds 0 to the sums and is passed
 * over by the maximum: one NaN leaves the rest of its row readable.  (A finite element whose square overflows makes the sum +inf.)
 * Order of every sum, whatever the alignment: lane L of the workgroup owns the elements i = L (mod 256) of the tensor and adds
 * their squares in index order -- one fp32 multiply and one fp32 add per element, the file is built without FMA contraction --
 * then the 64 lanes of each wave are folded by an xor-shuffle tree (offsets 32, 16, ... 1) and the four wave sums as
 * (w0 + w1) + (w2 + w3).  tests/adapter_stats_ref.py restates it.  No atomics, nothing crosses a workgroup: same inputs -> same
 * bits, and a tensor gets the same bits at any address.  16-byte accesses when p + off, prev + off and (phase 0) g + off are
 * 16-byte aligned (LoraStore starts every tensor on a multiple of 64 elements), scalar ones otherwise.
 * The kernel skips an entry with numel <= 0 or off < 0 (its row: all zeros in phase 0, the phase-1 fields zero in phase 1); it
 * does not check extents: every other entry must lie inside the three buffers.  Rejected with QFX_EINVAL before any launch: a NULL
 * p, prev, table or out, a NULL g in phase 0 (g is not read in phase 1 and may be NULL there), n_entries <= 0, a phase outside
 * {0, 1}, a max_norm that is negative or NaN, a grad_scale that is not finite. ---- */
typedef struct qfx_stats_entry {      /* 16 bytes */
  int64_t off;                        /* first element of the tensor in p / g / prev */
  int32_t numel;
  int32_t pad;
} qfx_stats_entry;
typedef struct qfx_stats_row {        /* 32 bytes */
  float   grad_sq, weight_sq, update_sq, grad_absmax;
  int32_t grad_nonfinite, weight_nonfinite;
  float   r0, r1;                     /* reserved: 0 */
} qfx_stats_row;
int qfx_adapter_stats(const float* p, const float* g, float* prev, const qfx_stats_entry* table, int32_t n_entries,
                      qfx_stats_row* out, int32_t phase, const float* gnorm_sq, float max_norm, float grad_scale, void* stream);

/* ---- Riemannian-preconditioned ("scaled") AdamW for LoRA pairs (Zhang & Pilanci, "Riemannian Preconditioned LoRA", ICML 2024)
 * over the flat LoRA buffers (csrc/qfx_scaled_adamw.hip).  Every trainable tensor here is half of a pair W = scaling * B A, and
 * for any invertible Q the tensors B Q and Q^-1 A are the same adapter, on which AdamW takes different steps; an r x r
 * preconditioner per pair, taken from the other half's Gram matrix, removes most of that dependence.  The authors' package was not
 * at hand: THIS LISTING IS THE SPECIFICATION (tests/scaled_adamw_ref.py restates it).  For one pair A [r, in], B [out, r]
 * (row-major fp32 at off_a / off_b of p, g, exp_avg, exp_avg_sq), step counter t from 1, c = the clip factor exactly as
 * qfx_adamw_step forms it from gnorm_sq, max_norm and grad_scale:
 *   gA = c * g_A                      gB = c * g_B                      fp32, as qfx_adamw_step scales g
 *   G_B = B^T B + reg I   [r, r]      G_A = A A^T + reg I   [r, r]      fp64 sums over fp32 inputs, fixed order; reg is the fp32
 *                                                                       argument widened
 *   P_B = G_B^-1                      P_A = G_A^-1                      fp64, Cholesky (reg > 0 makes both SPD), then L Y = I and
 *                                                                       L^T X = Y; one fp64 rounding per operation
 *   g^A = fp32(P_B gA)                g^B = fp32(gB P_A)                fp64 dot over the r terms in index order (each product and
 *                                                                       each sum rounded to fp64), rounded to fp32 once
 *   AdamW(A, g^A; lr_A, wd_A)         AdamW(B, g^B; lr_B, wd_B)         the operations of qfx_adamw_step in its order, with
 *                                                                       lr_X = lr * lr_ratio_X (one fp32 multiply), lr_X / bias_corr1
 *                                                                       and 1 / sqrt(bias_corr2) formed per tensor as it forms them
 * Both Gram matrices are taken from the weights before either tensor of the pair is written.  bias_corr1 = 1 - beta1^t and
 * bias_corr2 = 1 - beta2^t are formed on the host, as for qfx_adamw_step.  precondition = 0: no Gram matrix and no inverse is
 * formed, g^ = c * g, and p, exp_avg and exp_avg_sq of every pair get the bits qfx_adamw_step gives them with the tensor's lr and
 * weight decay.  Skip rule (the Muon step's): a pair with a non-finite element in its g (either mode), or with a Cholesky pivot
 * that is not positive and finite, keeps its p, exp_avg and exp_avg_sq unchanged; *skipped (device int32, set to 0 by a memset
 * node ahead of the launch) counts such pairs.
 * ONE launch, one 256-lane workgroup per pair, any number of pairs.  A, B and g stream through LDS tiles, both r x r fp64 matrices
 * live in LDS, the factorisation and the solves run inside the workgroup, a second sweep forms g^ and applies AdamW.  No value
 * crosses a workgroup but the skip counter (an integer atomic add, order-independent) and every sum runs in an order fixed by the
 * shape: same inputs -> same bits.  16-byte accesses for a tensor whose p, g, exp_avg and exp_avg_sq addresses are 16-byte
 * aligned and whose row length (in_features for A, r for B) is a multiple of 4; scalar accesses for any other tensor.
 * 1 <= r <= 64, 1 <= in, out <= 2^24, any offsets.
 * qfx_scaled_adamw_check_table runs on a HOST copy of the table: QFX_EINVAL for n_pairs < 0, n_elems < 0, a NULL table with
 * n_pairs > 0, r outside 1..64, in or out outside 1..2^24, a negative offset, a matrix that reaches past n_elems, two matrices of
 * the table that overlap, an lr_ratio or a weight decay that is negative or not finite.  The kernel skips a pair with such
 * dimensions or offsets without counting it; it does not check extents: launch only tables that passed.
 * qfx_scaled_adamw_step rejects with QFX_EINVAL before any launch: a NULL args, n_pairs < 0, lr or eps negative or NaN, a beta
 * outside [0, 1), a bias correction that is not > 0, precondition outside {0, 1}, with precondition = 1 a reg that is not finite
 * and > 0, a NaN max_norm, a grad_scale that is not finite, and with n_pairs > 0 a NULL p, g, exp_avg, exp_avg_sq, table or
 * skipped.  n_pairs == 0 returns QFX_OK without a launch. ---- */
typedef struct qfx_scaled_adamw_pair {    /* 48 bytes */
  int64_t off_a, off_b;                   /* first element of A [r, in] / B [out, r], row-major, in the flat buffers */
  int32_t r, in_features, out_features;
  float   lr_ratio_a, lr_ratio_b;         /* the tensor's learning rate over args.lr (LoRA+: 1 and the ratio) */
  float   wd_a, wd_b;                     /* the tensor's weight decay */
  int32_t reserved;
} qfx_scaled_adamw_pair;
typedef struct qfx_scaled_adamw_args {
  float* p;                               /* flat adapter weights, stepped in place */
  const float* g;                         /* flat gradient */
  float* exp_avg;
  float* exp_avg_sq;
  const qfx_scaled_adamw_pair* table;     /* device array */
  int32_t n_pairs;
  int32_t precondition;                   /* 1: the listing; 0: plain AdamW per tensor */
  float   lr, beta1, beta2, eps;
  float   reg;                            /* delta, > 0 (1e-6) */
  float   bias_corr1, bias_corr2;
  const float* gnorm_sq;                  /* the clip prologue of qfx_adamw_step */
  float   max_norm, grad_scale;
  int32_t* skipped;                       /* device counter, written */
} qfx_scaled_adamw_args;
int qfx_scaled_adamw_check_table(const qfx_scaled_adamw_pair* host_table, int32_t n_pairs, int64_t n_elems);
int qfx_scaled_adamw_step(const qfx_scaled_adamw_args* a, void* stream);

/* ---- The singular value decomposition of every adapter pair dW = B A over the flat LoRA buffer (csrc/qfx_lora_svd.hip): the
 * spectrum of each adapter, and kohya's resize_lora.py -- a trained pair re-expressed at a lower rank by truncated SVD -- without
 * ever forming the [out, in] product.  Appended under ABI 7: new structs and entry points only.  kohya's script was not at hand:
 * THIS LISTING IS THE SPECIFICATION (tests/lora_svd_ref.py restates it in numpy).  For one pair A [r, in], B [out, r] (row-major
 * fp32 at off_a / off_b of p), 1 <= r <= 64, 1 <= in, out <= 2^24, any offsets:
 *   G_A = A A^T,  G_B = B^T B               [r, r] fp64 sums over the widened fp32 inputs, fixed order (as qfx_maxnorm_apply forms them)
 *   G_A = V L V^T                           cyclic Jacobi in LDS, fp64 (below); negative l set to 0
 *   K   = L^1/2 V^T G_B                     [r, r] fp64: dots over the r terms in index order, then the one multiply by l_i^1/2
 *   H   = K V L^1/2                         [r, r] fp64, likewise; symmetrised: H_ij = H_ji = (H_ij + H_ji) / 2
 *   H   = W Th W^T                          cyclic Jacobi; th sorted descending (ties by index), negative th set to 0
 *   sv[i]  = sqrt(th_i)                     the singular values of B A (unscaled: the caller multiplies by |scaling|), written as
 *                                           fp64 sv [n_pairs, ld_sv]; entries r <= i < ld_sv are written 0
 *   rho    = #{ i : sv[i] > rank_tol sv[0] }    (0 when sv[0] == 0)
 *   T_B = V L^1/2 W             [r, r]      B T_B = U S;  columns i >= rho written as 0        ((V_ik l_k^1/2) W_kj summed over k in order)
 *   T_A = Th^-1 W^T K           [r, r]      T_A A = V^T (the right singular vectors as rows);  rows i >= rho written as 0
 *   info[pair] = { rho, sweeps of the first solve, sweeps of the second solve, converged (both) }    int32 x 4
 * No division occurs except by th_i for i < rho (and those of the rotations).  T_B and T_A go as fp64 to the caller's workspace
 * ws [n_pairs][2][64][64] (T_B first; row stride 64; everything outside the r x r corner written 0); ws == NULL: the spectrum
 * only, neither is formed.
 * The Jacobi solve of a symmetric M [n, n]: thr = 2^-52 ||M||_F / n; before each sweep off = max_{i<j} |M_ij|, the solve ends
 * converged when off <= thr and ends unconverged after max_sweeps sweeps (what it has is still written).  A sweep is n' - 1 rounds
 * (n' = n rounded up to even; index n is padding) of the round-robin ordering: round d pairs n' - 1 with d, and (d + k) mod (n' - 1)
 * with (d - k) mod (n' - 1) for k = 1 .. n'/2 - 1.  For each pair p < q of a round, from the matrix as the round finds it:
 *   M_pq == 0: c = 1, s = 0;  else tau = (M_qq - M_pp) / (2 M_pq), t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c
 * then every pair's columns (x, y) = (M_ip, M_iq) -> (c x - s y, s x + c y), the same on the accumulated vectors, then every pair's
 * rows likewise, with M_pq and M_qp set to 0.  Every trip count is fixed by r and max_sweeps: the kernel cannot spin (a NaN never
 * meets the criterion and runs to the cap).
 * Skip rule (Muon's, max-norm's): a pair with a non-finite Gram entry gets sv = 0, info = 0 (so converged = 0), a zero workspace,
 * and *skipped (device int32, set to 0 by a memset node ahead of the launch) counts it.
 * qfx_lora_spectrum: ONE launch, one 256-lane workgroup per pair, any number of pairs.  Both Gram matrices, both eigenproblems
 * and the transforms live in LDS (138 KB); no atomics but the integer skip counter, nothing else crosses a workgroup: same inputs
 * -> same bits at any address.  16-byte accesses for the tiles where A is 16-byte aligned and in % 4 == 0, resp. B 16-byte aligned
 * and r % 4 == 0; scalar ones otherwise.
 * qfx_lora_project: ONE launch, one workgroup per pair; reads p, ws and, per pair, dst = { dst_off_a, dst_off_b, k components
 * kept (1 <= k <= r), r_dst rows allocated (k <= r_dst <= 64) }; writes A' [r_dst, in] and B' [out, r_dst] into another buffer q:
 *   B'[:, j] = fp32(sum_i B[:, i] T_B[i, j])   j < k      fp64 products and sums in index order from +0, one rounding to fp32
 *   A'[j, :] = fp32(sum_i T_A[j, i] A[i, :])   j < k
 *   columns / rows k <= j < r_dst are written as +0.0
 * kohya's split: lora_up = U S, lora_down = V^T; the pair's scaling is unchanged, so the new lora_alpha is scaling * r_dst.
 * 16-byte stores of B' where its address is 16-byte aligned and r_dst % 4 == 0, 16-byte loads and stores for A' where A and A'
 * are 16-byte aligned and in % 4 == 0.
 * The two check functions run on HOST copies of the tables: QFX_EINVAL for n_pairs < 0, n_elems < 0, a NULL table with
 * n_pairs > 0, r outside 1..64, in or out outside 1..2^24, a negative offset, a matrix that reaches past n_elems, two matrices of
 * the table that overlap; qfx_lora_project_check_table (destination side, against the extent of q) also for k outside 1..r and
 * r_dst outside k..64.  The kernels skip a pair with such dimensions or offsets (spectrum: as a skipped pair, not counted;
 * project: nothing written); they do not check extents: launch only tables that passed.
 * qfx_lora_spectrum rejects with QFX_EINVAL before any launch: a NULL args, n_pairs < 0, a rank_tol that is not in (0, 1),
 * max_sweeps outside 1..64, ld_sv < 64, with n_pairs > 0 a NULL p, table, sv, info or skipped.  qfx_lora_project: a NULL args,
 * n_pairs < 0, q == p, with n_pairs > 0 a NULL p, q, table, dst or ws.  n_pairs == 0 returns QFX_OK without a launch. ---- */
typedef struct qfx_lora_svd_pair {        /* 32 bytes */
  int64_t off_a, off_b;                   /* first element of A [r, in] / B [out, r], row-major, in p */
  int32_t r, in_features, out_features;
  int32_t reserved;
} qfx_lora_svd_pair;
typedef struct qfx_lora_svd_dst {         /* 24 bytes */
  int64_t dst_off_a, dst_off_b;           /* first element of A' [r_dst, in] / B' [out, r_dst], row-major, in q */
  int32_t k, r_dst;
} qfx_lora_svd_dst;
typedef struct qfx_lora_spectrum_args {
  const float* p;                         /* flat adapter weights, read */
  const qfx_lora_svd_pair* table;         /* device array */
  int32_t n_pairs;
  int32_t max_sweeps;                     /* 1..64 (30) */
  double  rank_tol;                       /* in (0, 1) (1e-6) */
  double* sv;                             /* [n_pairs, ld_sv], written */
  int64_t ld_sv;                          /* >= 64 */
  int32_t* info;                          /* [n_pairs, 4], written */
  double* ws;                             /* [n_pairs][2][64][64], written; may be NULL */
  int32_t* skipped;                       /* device counter, written */
} qfx_lora_spectrum_args;
typedef struct qfx_lora_project_args {
  const float* p;                         /* the buffer qfx_lora_spectrum read */
  float* q;                               /* another flat buffer, written */
  const qfx_lora_svd_pair* table;         /* device array */
  const qfx_lora_svd_dst* dst;            /* device array */
  int32_t n_pairs;
  int32_t reserved;
  const double* ws;                       /* what qfx_lora_spectrum wrote */
} qfx_lora_project_args;
int qfx_lora_svd_check_table(const qfx_lora_svd_pair* host_table, int32_t n_pairs, int64_t n_elems);
int qfx_lora_project_check_table(const qfx_lora_svd_pair* host_table, const qfx_lora_svd_dst* host_dst, int32_t n_pairs, int64_t n_elems_dst);
int qfx_lora_spectrum(const qfx_lora_spectrum_args* a, void* stream);
int qfx_lora_project(const qfx_lora_project_args* a, void* stream);

/* ---- A rank-k factorisation D ~ Q C of every dense difference D = W1 - W0 of a device table (csrc/qfx_lora_extract.hip):
 * kohya's extract_lora_from_models.py by a randomized range finder (Halko, Martinsson, Tropp 2011, algorithms 4.4 / 5.1) instead
 * of a full SVD per layer.  Appended under ABI 7: new structs and entry points only.  kohya's script was not at hand:
 * THIS LISTING IS THE SPECIFICATION (tests/lora_extract_ref.py restates it in numpy).  For matrix m of the table, W1 and W0
 * [out, in] row-major with leading dimensions ld1 / ld0, both bf16 (dtype 0) or both fp32 (dtype 1), 1 <= k <= 64,
 * 1 <= in, out <= 2^24:
 *   D      = fp32(W1) - fp32(W0)            one fp32 subtraction per element; W0 == NULL: D = W1.  Formed before any product.
 *   Omega  [in, k] of +-1                   Philox4x32-10 (the generator of the dropout masks above), key = (seed_lo, seed_hi),
 *                                           counter = (row i, index, 0x4C524B58, 0) with `index` the field of the table row;
 *                                           Omega[i, j] = +1 if bit j & 31 of output word j >> 5 is clear, else -1
 *   Y = D Omega;  Q = orth(Y)
 *   q times:  Z = orth(D^T Q);  Q = orth(D Z)                0 <= q <= 4
 *   C = Q^T D                               [k, in]
 * Every product is over the fp32 values of D and of the other operand, one fp32 FMA per term in ascending order of the summed
 * index, the result an fp32 [out, k] resp. [in, k] matrix.  Nothing is rounded to bf16.
 * orth(Y) is o(o(Y)) with o(Y), for Y [n, k] fp32:
 *   G = Y^T Y                               [k, k] fp64 over the widened fp32 values (every product exact): per chunk of 64 rows
 *                                           in row order, the chunks' partials added in chunk order through the workspace
 *   G = V L V^T                             the cyclic Jacobi solve of the qfx_lora_spectrum listing above: the same ordering,
 *                                           threshold, sweep cap (max_sweeps) and fixed trip counts; l sorted descending, ties
 *                                           by index
 *   kept = #{ i : l_i > orth_tol l_0 }      (0 when l_0 <= 0)
 *   T_ij = V_ij / sqrt(l_j)  for j < kept,  0 otherwise
 *   o(Y) = fp32(Y T)                        fp64 products and sums in index order from +0, one rounding to fp32; the columns
 *                                           j >= kept come out as +0
 * The variant is rank-revealing on purpose: rank(D) < k (a model with a LoRA merged in) and k > min(out, in) leave the surplus
 * columns of Q and rows of C zero where a Cholesky QR would break down.
 * Output: Q as B [out, k] at off_b and C as A [k, in] at off_a of the flat fp32 buffer p, row-major: rows (off_a, off_b, k, in,
 * out) are a qfx_lora_svd_pair table with r = k for qfx_lora_spectrum / qfx_lora_project.  normsq[m] = ||D||_F^2 in fp64 (a
 * lane's elements in its order, the 256 lanes by a fixed tree, the chunks' partials in residue classes mod 256, then the tree).
 * info[m] = { kept of the last orth, the converged flags of every Jacobi solve of the matrix ANDed }.
 * Skip rule (Muon's, max-norm's): a matrix with a non-finite element of D gets A = 0, B = 0, normsq = 0, info = 0, and *skipped
 * (device int32, set to 0 by a memset node ahead of the launches) counts it.
 * qfx_lowrank_sketch enqueues 8 + 10 q launches and the memset on the stream, whatever the data; no host synchronisation, no
 * host -> device copy (host_table is read at enqueue time only: for the checks below and the grid sizes), so it can sit in a
 * captured graph.  The grids cover (chunk, matrix); a table may mix shapes and dtypes.  16-byte loads of W1 / W0 where both are
 * 16-byte aligned with leading dimensions that are multiples of 8 (bf16) resp. 4 (fp32) elements, scalar ones otherwise; the
 * edges of a 64 x 64 tile are handled in the kernel.  No floating-point atomics: same inputs -> same bits at any address.
 * ws: qfx_lowrank_sketch_workspace bytes (QFX_EINVAL, negative, for what the check below refuses in k / in / out / dtype / ld /
 * W1), 16-byte aligned; its contents need not survive between calls.
 * qfx_lowrank_check_table runs on a HOST copy of the table: QFX_EINVAL for n_mats < 0, n_elems < 0, a NULL table with
 * n_mats > 0, k outside 1..64, in or out outside 1..2^24, a leading dimension < in, a dtype other than 0 or 1, a NULL W1,
 * a negative offset, an output that reaches past n_elems, two outputs that overlap.
 * qfx_lowrank_sketch rejects with QFX_EINVAL before any launch: a NULL args, n_mats outside 0..65535, q outside 0..4, max_sweeps
 * outside 1..64, an orth_tol that is not in [0, 1), with n_mats > 0 a NULL table, host_table, p, normsq, info, skipped or ws, a
 * ws that is not 16-byte aligned or shorter than qfx_lowrank_sketch_workspace says, and whatever qfx_lowrank_check_table refuses
 * of host_table against n_elems.  n_mats == 0 returns QFX_OK without a launch. ---- */
typedef struct qfx_lowrank_mat {          /* 80 bytes */
  const void* w1;                         /* [out, in], device */
  const void* w0;                         /* [out, in], device; NULL: D = W1 */
  int64_t ld1, ld0;                       /* elements */
  int64_t off_a, off_b;                   /* first element of A = C [k, in] / B = Q [out, k] in p */
  int32_t k, in_features, out_features;
  int32_t dtype;                          /* 0: bf16, 1: fp32 */
  int32_t index;                          /* counter word 1 of Omega */
  int32_t reserved[3];
} qfx_lowrank_mat;
typedef struct qfx_lowrank_args {
  const qfx_lowrank_mat* table;           /* device array */
  const qfx_lowrank_mat* host_table;      /* the same rows on the host */
  int32_t n_mats;
  int32_t q;                              /* power iterations, 0..4 (2) */
  uint32_t seed_lo, seed_hi;
  double  orth_tol;                       /* in [0, 1) (1e-12) */
  int32_t max_sweeps;                     /* 1..64 (30) */
  int32_t reserved;
  float* p;                               /* flat output buffer, written */
  int64_t n_elems;                        /* its extent */
  double* normsq;                         /* [n_mats], written */
  int32_t* info;                          /* [n_mats, 2], written */
  int32_t* skipped;                       /* device counter, written */
  void* ws;
  int64_t ws_bytes;
} qfx_lowrank_args;
int qfx_lowrank_check_table(const qfx_lowrank_mat* host_table, int32_t n_mats, int64_t n_elems);
int64_t qfx_lowrank_sketch_workspace(const qfx_lowrank_mat* host_table, int32_t n_mats);
int qfx_lowrank_sketch(const qfx_lowrank_args* a, void* stream);

/* ---- W <- W + c B A over every dense matrix of a device table, in place (csrc/qfx_lora_fold.hip): the residual trunk of a PiSSA
 * initialisation (Meng et al. 2024; c = -lora_alpha / r) in one pass over the trunk, with bits that do not depend on a BLAS
 * library.  Appended under ABI 7: new structs and entry points only.  THIS LISTING IS THE SPECIFICATION (tests/pissa_ref.py
 * restates it in numpy).  For row m of the table: W [out, in] row-major with leading dimension ld, bf16 (dtype 0) or fp32
 * (dtype 1); A [r, in] and B [out, r] row-major fp32 at off_a / off_b of the flat buffer p, 1 <= r <= 64, 1 <= in, out <= 2^24;
 * c the row's fp32 coefficient.  For every o < out, i < in:
 *   s       = sum_{j<r} fp64(B[o,j]) fp64(A[j,i])     ascending j from +0; every product is exact in fp64, one rounding per
 *                                                     addition (an fp64 FMA gives the same bits; the kernel uses it)
 *   t       = fp64(c) s                               one rounding
 *   w'      = fp64(W[o,i]) + t                        one rounding
 *   W[o,i]  = fp32(w') (nearest even), and for a bf16 W that fp32 value rounded to bf16 (nearest even)
 * Every element is read and written by the same lane; no atomics, nothing crosses a workgroup: same inputs -> same bits at any
 * address and in any table order.  Columns in <= i < ld are never touched.  There is no skip rule: non-finite values propagate by
 * IEEE arithmetic into the elements they reach.  A and B are only read; several rows may name the same ones.
 * qfx_lora_fold enqueues a one-workgroup launch that writes tile_start [n_mats + 1] (the 64 x 64 tiles of the rows before each
 * row, int64) from the device table, and ONE launch over the flat grid of (tile, matrix), sized from host_table by the same count
 * (host_table is read at enqueue time only; no host synchronisation, no host -> device copy: it can sit in a captured graph).
 * The tile's B [64, r] and A [r, 64] are staged in LDS as fp32; 16-byte loads and stores of W where W is 16-byte aligned and
 * ld % 8 == 0 (bf16) resp. ld % 4 == 0 (fp32), scalar ones otherwise; tile edges are handled in the kernel.
 * qfx_lora_fold_check_table runs on a HOST copy of the table: QFX_EINVAL for n_mats outside 0..65535, n_elems < 0, a NULL table
 * with n_mats > 0, r outside 1..64, in or out outside 1..2^24, ld < in, a dtype other than 0 or 1, a NULL W, a negative offset,
 * A or B reaching past n_elems, two W of the table whose extents [W, W + (out - 1) ld + in) overlap, more than 2^24 - 1 tiles
 * in all (the flat grid of 256-lane workgroups stays below 2^32 lanes; 420 matrices of 12288 x 3072 are 3.9 million).
 * qfx_lora_fold rejects with QFX_EINVAL before any launch: a NULL args, n_mats outside 0..65535, with n_mats > 0 a NULL table,
 * host_table, p or tile_start, and whatever qfx_lora_fold_check_table refuses of host_table against n_elems.  n_mats == 0
 * returns QFX_OK without a launch. ---- */
typedef struct qfx_lora_fold_mat {        /* 64 bytes */
  void* w;                                /* [out, in], device; read and written */
  int64_t ld;                             /* elements */
  int64_t off_a, off_b;                   /* first element of A [r, in] / B [out, r] in p */
  int32_t r, in_features, out_features;
  int32_t dtype;                          /* 0: bf16, 1: fp32 */
  float   c;
  int32_t reserved[3];
} qfx_lora_fold_mat;
typedef struct qfx_lora_fold_args {
  const qfx_lora_fold_mat* table;         /* device array */
  const qfx_lora_fold_mat* host_table;    /* the same rows on the host */
  int32_t n_mats;
  int32_t reserved;
  const float* p;                         /* flat fp32 buffer that holds every A and B, read */
  int64_t n_elems;                        /* its extent */
  int64_t* tile_start;                    /* device, [n_mats + 1], written */
} qfx_lora_fold_args;
int qfx_lora_fold_check_table(const qfx_lora_fold_mat* host_table, int32_t n_mats, int64_t n_elems);
int qfx_lora_fold(const qfx_lora_fold_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QFX_H */
