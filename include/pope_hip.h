/* pope_hip.h — C ABI of the MI355X-native (gfx950) POPE hot path.
 *
 * The reference (karltan0328/POPE) is pure Python on PyTorch: it has no FFI, its "operator
 * interface" for this path is the call convention of two nn.Modules plus a namespace
 * (SURVEY.md §8b).  Each entry point below names the reference call site it replaces; the
 * Python mirror in pope_amd/ binds them with ctypes (see INTEGRATION.md for the stub a
 * reference maintainer would add).
 *
 * Conventions: every pointer is a DEVICE pointer unless the name ends in _host; tensors are
 * dense row-major fp32 in the reference's native layouts (torch Linear weight = [out, in]);
 * `stream` is a hipStream_t; no entry point allocates or synchronises — workspaces are
 * caller-provided (size query functions); return value 0 = OK, negative = error
 * (pope_error_string).  All work is enqueued asynchronously.
 * Devices: work is launched on the device that owns `stream`; for stream == NULL (the default
 * stream, which does not name a device) on the calling thread's current device, so a caller with
 * several GPUs makes the operands' device current first (pope_amd/_lib.py:on_device_of does).
 * State: the library keeps, per device and filled lazily, the CU count and one "large dynamic
 * LDS enabled" bit per kernel (atomics; idempotent) — nothing else, and nothing per call, so
 * entry points may be called concurrently from several threads and for several devices.
 *
 * f16x3 range guard: POPE_PREC_F16X3 keeps operands as f16 pairs after a power-of-two scale
 * (activations x8, weights and matcher features x256), i.e. it needs |activation| < 8190 and
 * |weight| < 255.9.  Every entry point that converts values takes `range_flag`, an optional
 * DEVICE word (NULL = no check) into which POPE_RANGE_* bits are ORed when a converted value
 * would not be finite in f16 (or is not finite to begin with); the caller zeroes it, reads it at
 * its next synchronisation point and re-runs the work with POPE_PREC_F32_MFMA, which has no range
 * contract (pope_amd/dinov2.py, pope_amd/pipeline.py do exactly that).
 */
#ifndef POPE_HIP_H
#define POPE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POPE_ABI_VERSION 10

enum {
    POPE_EPI_BIAS = 0,        /* C = A.W^T + bias                         nn.Linear                     */
    POPE_EPI_BIAS_GELU = 1,   /* C = gelu_erf(A.W^T + bias)               mlp.py:35-41 (fc1 + nn.GELU)  */
    POPE_EPI_BIAS_LS_RES = 2, /* C = res + gamma*(A.W^T + bias)           block.py:105-106 + layer_scale.py:28 */
    /* The w12 GEMM of the SwiGLU FFN with its activation (swiglu_ffn.py:29-33): A[M,K], W[N,K] with N = 2*hidden,
     * C[M, hidden] = silu(gate) * value — the [M, 2*hidden] product never reaches memory.  A 64 x 64 accumulator block has to
     * hold a hidden column's gate AND value, so the ROWS of W and bias are expected permuted: for every block t of 32 hidden
     * columns, rows 64t .. 64t+31 are w12 rows 32t .. 32t+31 (gates), rows 64t+32 .. 64t+63 are w12 rows
     * hidden+32t .. hidden+32t+31 (values).  N % 64 == 0.  silu(x) = x / (1 + exp(-x)) in fp32 (exp as exp2 of the pre-scaled
     * argument), finite for every finite gate.  pope_linear_planes_f32 (planes or fp32 out, range bit POPE_RANGE_GELU: it marks the
     * FC1 producer) and pope_linear_f32 with POPE_PREC_F32_MFMA take it; gamma and res are ignored. */
    POPE_EPI_BIAS_SWIGLU = 11,
    /* pope_linear_f16 only — the QKV projection of the POPE_PREC_F16 ViT blocks, whose output is the operand of
     * pope_attention_f16: C = (A.W^T + bias) * (col < N/3 ? 0.125 * log2 e : 1), rounded ONCE to f16 rows with no activation
     * scale (heads of 64: q carries head_dim^-0.5 * log2 e).  N % 192 == 0; range bit POPE_RANGE_QKV, checked after the scale. */
    POPE_EPI_QKV_F16 = 8
};

/* Arithmetic of the contractions.  Both take and return fp32 and accumulate in fp32:
 *  POPE_PREC_F32_MFMA  v_mfma_f32_32x32x2_f32, an exact k-ordered fp32 fma chain (157 TFLOP/s peak; on gfx950
 *                      this instruction runs on the VALU lanes);
 *  POPE_PREC_F16X3     operands split x = hi + lo (two f16, 22 significand bits), three f16 MFMAs
 *                      (v_mfma_f32_16x16x32_f16 in the GEMMs, v_mfma_f32_32x32x16_f16 in attention) per product
 *                      block on the matrix cores: same or smaller error than the fp32 chain inside the range
 *                      contract below (measured against fp64), 2.3x faster end to end. */
enum { POPE_PREC_F32_MFMA = 0, POPE_PREC_F16X3 = 1, POPE_PREC_F16 = 2 /* opt-in plain f16 operands, one MFMA per product: ViT / SAM encoders, LoFTR ResNet-FPN; see there */ };
/* bits of a range_flag word: which f16x3 producer saw a value out of range */
enum { POPE_RANGE_PATCH = 1, POPE_RANGE_LAYERNORM = 2, POPE_RANGE_QKV = 4, POPE_RANGE_GELU = 8, POPE_RANGE_MATCH = 16,
       POPE_RANGE_INPUT = 32 };

int pope_abi_version(void);
const char* pope_error_string(int code);

/* ---- op-level entry points (each is one kernel; used by the parity tests) ------------- */

/* nn.LayerNorm(dim, eps) over the last dim — vision_transformer.py:90,230; block.py:56,68. */
int pope_layernorm_f32(const float* x, const float* weight, const float* bias, float* y,
                       int rows, int dim, float eps, void* stream);

/* nn.Linear (+ fused epilogue) — attention.py:51,60; mlp.py:35-44.  A[M,K], W[N,K], C[M,N];
 * gamma[N] and res[M,N] only for POPE_EPI_BIAS_LS_RES (res may alias C).  precision: POPE_PREC_F32_MFMA or POPE_PREC_F16X3,
 * which splits A and W inside the kernel; with range_flag both operands are scanned first (POPE_RANGE_INPUT). */
int pope_linear_f32(const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                    int epilogue, const float* gamma, const float* res, int precision,
                    unsigned* range_flag, void* stream);

/* f16x3 "planes": a tensor X[rows, cols] (cols % 32 == 0) kept as f16 halves with X * scale = hi + lo
 * (scale a power of two: POPE_PLANES_ACT_SCALE for activations, POPE_PLANES_W_SCALE for weights), laid
 * out row-major with 2*cols halves per row and, per 32-column chunk, the 32 hi halves followed by the
 * 32 lo halves (one 128-byte cache line per row and GEMM K-step):
 *     half_offset(row, col, plane) = row*2*cols + (col/32)*64 + plane*32 + col%32.
 * Producers split once (LayerNorm, the GELU epilogue, the weight loader) so that the f16x3 GEMM
 * stages MFMA-ready operands with no conversion work in its K loop. */
#define POPE_PLANES_ACT_SCALE 8.0f
#define POPE_PLANES_W_SCALE 256.0f
int pope_split_planes_f32(const float* src, void* planes, int rows, int cols, float scale,
                          unsigned* range_flag, void* stream);
/* nn.Linear on planes: A planes [M,K], W planes [N,K]; output either fp32 C[M,N] (c_planes == NULL) or
 * activation planes [M,N] (C == NULL; not for POPE_EPI_BIAS_LS_RES).  K % 32 == 0, K >= 64.  POPE_EPI_BIAS_SWIGLU: the output
 * is [M, N/2]. */
int pope_linear_planes_f32(const void* a_planes, const void* w_planes, const float* bias, float* C,
                           void* c_planes, int M, int N, int K, int epilogue, const float* gamma,
                           const float* res, unsigned* range_flag, void* stream);

/* LayerNorm written as activation planes [rows, dim]. */
int pope_layernorm_planes_f32(const float* x, const float* weight, const float* bias, void* y_planes,
                              int rows, int dim, float eps, unsigned* range_flag, void* stream);

/* Test entry of the ViT's LayerNorm-fused residual GEMM (dim 384; the patch embed, proj and fc2 launches of
 * pope_vit_forward_f32 past its small-batch switch):
 *     x  = res + gamma * (A.W^T + bias)            A planes [M,K], W planes [384,K]; x [M,384] fp32, may alias res
 *     xn = LayerNorm(x) * ln_w + ln_b              eps inside the sqrt; exactly one of ln_planes (activation planes
 *                                                  [M,384], range-guarded: POPE_RANGE_LAYERNORM) and ln_out (fp32 [M,384])
 * res_mod == 0: res [M,384], gamma required; res_mod > 0: residual row = res[row % res_mod] of a [res_mod,384] table.
 * bias and gamma may be NULL (zero, one).  K % 32 == 0, K >= 64, M >= 1, (M + 192) * 1536 < 2^32 - 512; a call outside
 * this returns POPE_ERR_ARG before any HIP call. */
int pope_linear_rowln_f32(const void* a_planes, const void* w_planes, int M, int K, const float* bias, const float* gamma,
                          const float* res, int res_mod, float* x, const float* ln_w, const float* ln_b, float eps,
                          void* ln_planes, float* ln_out, unsigned* range_flag, void* stream);
/* Test entry of its small-batch twin, the stand-alone LayerNorm that pope_vit_forward_f32 runs after a
 * pope_linear_planes_f32(..., POPE_EPI_BIAS_LS_RES) below the switch: the fused epilogue's reduction order, bit for bit.
 * x [rows,384] -> exactly one of y_planes (activation planes, POPE_RANGE_LAYERNORM) and y_f32 (fp32; range_flag
 * untouched).  rows >= 1; a call outside this returns POPE_ERR_ARG before any HIP call. */
int pope_layernorm_rowln_order_f32(const float* x, const float* weight, const float* bias, void* y_planes, float* y_f32,
                                   int rows, float eps, unsigned* range_flag, void* stream);

/* Test entries of the remaining GEMM operand producers, one kernel each.  A call outside the stated shapes returns
 * POPE_ERR_ARG before any HIP call.
 * LayerNorm written as plain f16 rows y_f16[rows, dim] = f16(y * POPE_PLANES_ACT_SCALE), the A operand of the POPE_PREC_F16
 * GEMMs (range-guarded: POPE_RANGE_LAYERNORM).  dim as pope_layernorm_f32: 128..768 in steps of 128, 1024, 1280, 1536, 2048. */
int pope_layernorm_f16(const float* x, const float* weight, const float* bias, void* y_f16, int rows, int dim, float eps,
                       unsigned* range_flag, void* stream);
/* y_f16[i] = f16(x[i] * POPE_PLANES_ACT_SCALE), i < n; n % 4 == 0, x 16-byte and y_f16 8-byte aligned (POPE_RANGE_INPUT). */
int pope_to_f16(const float* x, void* y_f16, long long n, unsigned* range_flag, void* stream);
/* Test entry of the POPE_PREC_F16 Linears (single-product f16 MFMAs, fp32 accumulate): one call of the router that
 * pope_vit_forward_f32 and the SAM encoder use, which picks the 256-row LDS-direct mainloop from M >= 2048 (N >= 256) and the
 * 128 x 128 tile kernel below — bit-identical.  a_f16 [M,K] f16 = value * POPE_PLANES_ACT_SCALE, w_f16 [N,K] f16 = value *
 * POPE_PLANES_W_SCALE; M, N, K in real columns.  epilogue and output (the other output pointer NULL):
 *     POPE_EPI_BIAS          -> C [M,N] fp32
 *     POPE_EPI_BIAS_GELU     -> c_f16 [M,N] f16 = value * POPE_PLANES_ACT_SCALE        (POPE_RANGE_GELU)
 *     POPE_EPI_QKV_F16       -> c_f16 [M,N] f16, no scale; N % 192 == 0                (POPE_RANGE_QKV)
 *     POPE_EPI_BIAS_LS_RES   -> C [M,N] fp32 = res + gamma * (A.W^T + bias): res [M,N] (may alias C) with gamma, or with
 *                               res_mod > 0 residual row = res[row % res_mod] of a [res_mod,N] table (gamma may be NULL: one)
 * bias may be NULL.  K % 64 == 0, K >= 128; N % 4 == 0 (fp32 out) or N % 64 == 0 (f16 out); M >= 1.  A call outside this
 * returns POPE_ERR_ARG before any HIP call. */
int pope_linear_f16(const void* a_f16, const void* w_f16, const float* bias, float* C, void* c_f16, int M, int N, int K,
                    int epilogue, const float* gamma, const float* res, int res_mod, unsigned* range_flag, void* stream);
/* The matcher's feature planes: n blocks of [rows, cols] fp32, batch_stride floats apart (even, >= rows * cols), to compact
 * planes [n * rows, cols] of (src / divisor) * scale — the division first, in fp32, as coarse_matching.py:109 rounds it; scale a
 * power of two.  cols % 32 == 0 (POPE_RANGE_MATCH). */
int pope_div_planes_f32(const float* src, long long batch_stride, void* planes, int n, int rows, int cols, float divisor,
                        float scale, unsigned* range_flag, void* stream);

/* PatchEmbed.forward + prepare_tokens_with_masks — patch_embed.py:69-82,
 * vision_transformer.py:191-200.  img[B,3,H,W]; proj_w[dim, 3*patch*patch];
 * posb[ntok, dim] = {cls_token + pos[0]; conv_bias + pos[n]} with pos already interpolated to
 * the (H/patch, W/patch) grid; tokens[B, ntok, dim], ntok = 1 + (H/patch)*(W/patch). */
int pope_patch_embed_f32(const float* img, const float* proj_w, const float* posb, float* tokens,
                         int B, int H, int W, int patch, int dim, void* stream);
/* Same on the f16 matrix cores: the image patches are gathered into activation planes [B*ntok, kp] in
 * a_planes_scratch (>= B*ntok*kp*4 bytes; kp = 3*patch^2 rounded up to 32) and multiplied with proj_w_planes
 * [dim, kp] (weight planes, zero-padded columns); posb as above. */
int pope_patch_embed_planes_f32(const float* img, const void* proj_w_planes, const float* posb, float* tokens,
                                int B, int H, int W, int patch, int dim, void* a_planes_scratch,
                                size_t scratch_bytes, unsigned* range_flag, void* stream);

/* Attention.forward core — attention.py:51-59: qkv[B,N,3,heads,64] -> out[B,N,heads*64],
 * softmax((q*0.125) k^T) v.  precision: POPE_PREC_F32_MFMA or POPE_PREC_F16X3; with range_flag a POPE_PREC_F16X3
 * call scans qkv first (POPE_RANGE_INPUT). */
int pope_attention_f32(const float* qkv, float* out, int B, int N, int heads, int precision,
                       unsigned* range_flag, void* stream);
/* f16x3 attention on planes (layout and scale: POPE_PLANES_* above; the producer of the planes guards the range:
 * the output is a convex combination of v rows, so it fits whenever v did): qkv_planes [B*N, 3*heads*64] as written by
 * pope_linear_planes_f32(..., c_planes), out_planes [B*N, heads*64] as read by the proj GEMM.  heads*64 % 32 == 0. */
int pope_attention_planes_f32(const void* qkv_planes, void* out_planes, int B, int N, int heads, void* stream);

/* POPE_PREC_F16 attention core (BASELINE config 5's dtype; attention.py:51-59 in single-product f16 arithmetic with fp32 scores,
 * softmax and accumulators): qkv_f16 [B*N, 3*heads*64] f16 row-major holding q * (head_dim^-0.5 * log2 e), k, v — what the QKV
 * projection of the f16 ViT path writes — -> out_f16 [B*N, heads*64] f16, value * POPE_PLANES_ACT_SCALE (the f16 proj GEMM's
 * operand).  qkv_f16 and out_f16 16-byte aligned.  (ABI 9.) */
int pope_attention_f16(const void* qkv_f16, void* out_f16, int B, int N, int heads, void* stream);

/* Measurement only: pope_attention_planes_f32 through a diagnostic instantiation of the same kernel that counts the
 * (wave, 64-key tile) pairs whose softmax reference had to ADVANCE before the tile's exponentials (*exact_passes_host; of
 * B * heads * ceil(N / 32) * ceil(N / 64) pairs in all; until round 3 the count was of tiles redone after an overflow).
 * Same results; SYNCHRONISES the stream.  bench.py's `attention_ramp` leg. */
int pope_attention_planes_diag_f32(const void* qkv_planes, void* out_planes, int B, int N, int heads, long long* exact_passes_host,
                                   void* stream);

/* F.cosine_similarity(ref[1,D], fea[P,D], dim=1, eps) — eval_linemod_json.py:94. */
int pope_cls_cosine_f32(const float* ref, const float* fea, int P, int D, float eps, float* scores,
                        void* stream);

/* ---- whole-model entry point -------------------------------------------------------------- */

typedef struct pope_vit_block_weights {   /* state-dict keys blocks.{i}.*  (device pointers) */
    const float *norm1_w, *norm1_b;       /* norm1.weight/bias [dim]                          */
    const float *qkv_w, *qkv_b;           /* attn.qkv.weight [3dim,dim], bias [3dim]          */
    const float *proj_w, *proj_b;         /* attn.proj.weight [dim,dim], bias [dim]           */
    const float *ls1;                     /* ls1.gamma [dim]                                  */
    const float *norm2_w, *norm2_b;
    const float *fc1_w, *fc1_b;           /* mlp.fc1.weight [hidden,dim]                      */
    const float *fc2_w, *fc2_b;           /* mlp.fc2.weight [dim,hidden]                      */
    const float *ls2;
    /* optional (POPE_PREC_F16X3): weight planes [out][in] (layout above), scale POPE_PLANES_W_SCALE;
     * NULL -> the layer splits its fp32 weights on the fly */
    const void *qkv_wp, *fc1_wp, *fc2_wp, *proj_wp;
} pope_vit_block_weights;

typedef struct pope_vit_weights {
    int dim, depth, heads, patch, hidden;
    const float* patch_w;                 /* patch_embed.proj.weight flattened [dim, 3*patch^2] */
    const float *norm_w, *norm_b;         /* final norm                                         */
    const pope_vit_block_weights* blocks_host; /* HOST array [depth] of device-pointer structs  */
    int precision;                        /* POPE_PREC_* of the Linear layers and of attention; POPE_PREC_F16 (opt-in): the
                                             blocks' `*_wp` are plain f16 row-major matrices (value * 256), one MFMA per
                                             product; patch_wp stays weight planes (the patch embed is f16x3) */
    const void* patch_wp;                 /* optional: patch_w as weight planes [dim, kp], kp = 3*patch^2 rounded up to a
                                             multiple of 32 with zero columns; enables the f16x3 patch embed */
} pope_vit_weights;

size_t pope_vit_workspace_bytes(int B, int ntok, int dim, int hidden);

/* Feed-forward kind of the blocks.  POPE_FFN_MLP: fc2(gelu(fc1(x))), mlp.py:35-44.  POPE_FFN_SWIGLU: w3(silu(x1) * x2) with
 * x1, x2 = w12(x).chunk(2), swiglu_ffn.py:13-63 (ViT-g/14): fc1_w / fc1_b / fc1_wp hold w12 [2*hidden, dim] with its rows
 * permuted as POPE_EPI_BIAS_SWIGLU describes, fc2_* hold w3 [dim, hidden], pope_vit_weights::hidden = w3's in_features
 * (a multiple of 32); not with POPE_PREC_F16. */
enum { POPE_FFN_MLP = 0, POPE_FFN_SWIGLU = 1 };

/* DinoVisionTransformer.forward_features — vision_transformer.py:221-236.
 * Outputs: x_prenorm[B,ntok,dim] (also the residual stream, required) and x_norm[B,ntok,dim]
 * (final LayerNorm; row 0 = x_norm_clstoken, rows 1.. = x_norm_patchtokens; may be NULL).
 * n_taps/tap_blocks_host/tap_out_host: optional copies of the residual stream after the listed
 * blocks (get_intermediate_layers, vision_transformer.py:238-288).
 * ffn: POPE_FFN_* of the blocks.  An unknown kind, POPE_FFN_SWIGLU with POPE_PREC_F16, with hidden % 32 != 0 or with a NULL
 * fc1_w / fc1_b / fc2_w return POPE_ERR_ARG before any HIP call. */
int pope_vit_forward_f32(const pope_vit_weights* w_host, int ffn, const float* img, int B, int H, int W,
                         const float* posb, float* x_prenorm, float* x_norm,
                         int n_taps, const int* tap_blocks_host, float* const* tap_out_host,
                         void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream);

/* In-situ kernel timing of the product path (bench.py's roofline leg): identical launches, plus
 * events_host[i] (hipEvent_t made by pope_event_create) recorded on `stream` immediately before
 * launch i and one closing event, so consecutive events bracket exactly one kernel.  kinds_host[i]
 * receives the POPE_K_* id of launch i; *n_launches_host the number of launches (= pope_vit_launch_count). */
enum { POPE_K_PATCH_EMBED = 0, POPE_K_LAYERNORM = 1, POPE_K_GEMM_QKV = 2, POPE_K_ATTENTION = 3,
       POPE_K_GEMM_PROJ = 4, POPE_K_GEMM_FC1 = 5, POPE_K_GEMM_FC2 = 6, POPE_K_TAP_COPY = 7 };
int pope_vit_launch_count(int depth);
/* Only launches whose POPE_K_* bit is set in kind_mask are bracketed (an event before and one after each; ~0u =
 * all): timing one kernel kind leaves every other launch of the sequence back to back, as in the untimed path.  events_host[i] / kinds_host[i] then hold the recorded events in order; kinds_host[i] is the kind
 * of the launch that STARTS at event i, or -1 for an event that only closes the previous bracket;
 * *n_launches_host = number of recorded events - 1. */
int pope_vit_forward_profiled_f32(const pope_vit_weights* w_host, int ffn, const float* img, int B, int H, int W,
                                  const float* posb, float* x_prenorm, float* x_norm,
                                  void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream,
                                  void* const* events_host, int n_events, int* kinds_host,
                                  int* n_launches_host, unsigned kind_mask);
int pope_event_create(void** event_host);
int pope_event_destroy(void* event);
int pope_event_elapsed_ms(void* start, void* stop, float* ms_host);  /* both events must have completed */

/* ---- dense matcher --------------------------------------------------------------------------- */

/* CoarseMatching.forward + get_coarse_match (eval) — src/matcher/utils/coarse_matching.py:106-148,151-261, for both of
 * its matchers.  The caller fills one pope_dense_match_args, asks pope_dense_match_workspace_bytes for the size, sets
 * `workspace` / `workspace_bytes` and calls pope_dense_match_f32.
 * POPE_MATCH_DUAL_SOFTMAX (:106-119): conf = softmax_rows(sim) * softmax_cols(sim), sim = (feat0 / sqrt C) . (feat1 / sqrt C)^T /
 *   temperature.
 * POPE_MATCH_SINKHORN (:121-143): the dual softmax replaced by log-domain optimal transport.  sim carries no temperature
 *   (`temperature` is ignored: 1); Z [L+1, S+1] is sim (after the -1e9 fill) bordered by a dustbin row, column and corner that
 *   all hold *bin_score; norm = -log(L+S), log_mu = [norm]*L + [log(S)+norm], log_nu = [norm]*S + [log(L)+norm]; from u = v = 0,
 *   skh_iters times u_i = log_mu_i - logsumexp_j(Z_ij + v_j), v_j = log_nu_j - logsumexp_i(Z_ij + u_i);
 *   conf = exp(Z + u + v - norm)[:L, :S].
 * Threshold, border, mutual nearest neighbour, ordering and scaling then apply to conf in the same way for both.
 * POPE_ERR_ARG (null feat / output / workspace pointers, non-positive or inconsistent sizes, an unknown precision or match_type,
 * POPE_MATCH_SINKHORN without bin_score or with skh_iters < 1) and POPE_ERR_WORKSPACE are returned before any HIP call. */
enum { POPE_MATCH_DUAL_SOFTMAX = 0, POPE_MATCH_SINKHORN = 1 };
typedef struct pope_dense_match_args {
    /* feat0[n,L,C], feat1[n,S,C], 16-byte aligned, with `stride0` / `stride1` elements (multiples of 4) between consecutive
     * pairs: L*C / S*C when dense; larger when the features are the patch rows of an x_norm[B,1+L,C] buffer */
    const float* feat0; long long stride0;
    const float* feat1; long long stride1;
    int n, L, S, C;                /* C % 4 == 0, n <= 65535 */
    int h0, w0, h1, w1;            /* the grids: L == h0 * w0, S == h1 * w1 */
    float thr; int border_rm;
    float temperature;             /* POPE_MATCH_DUAL_SOFTMAX only */
    float scale;                   /* hw0_i[0] / hw0_c[0] */
    int match_type;                /* POPE_MATCH_* */
    /* POPE_MATCH_SINKHORN only.  bin_score: DEVICE pointer to one float, read by the kernels at run time (the learned parameter's
     * own storage; the host never reads it, an in-place update is seen by the next call).  skh_iters >= 1.  skh_prefilter != 0
     * zeroes the rows of conf whose largest assignment over the S+1 columns is the dustbin (strictly: a tie goes to the real
     * cell) and the columns likewise (:136-140). */
    const float* bin_score; int skh_iters, skh_prefilter;
    /* Padded batches and rescaling (coarse_matching.py:115-118,178-184,242-250): six optional inputs (NULL = absent; masks hold
     * 0 / 1 as fp32):
     *   fill_mask0[n,L], fill_mask1[n,S]: sim = -1e9 (finite, the reference's -INF) where fill_mask0[i] * fill_mask1[j] == 0,
     *     before both softmaxes (a missing one counts as ones);
     *   border_mask0[n,h0,w0], border_mask1[n,h1,w1]: when either is given, the bottom / right border of each pair lies at its
     *     valid extent (h = max column sum, w = max row sum, per image) instead of the grid's (mask_border_with_padding);
     *   scale0[n,2], scale1[n,2]: (x, y) factors, mkpts*_c = (idx % w, idx / w) * (scale * scale*[b]). */
    const float *fill_mask0, *fill_mask1, *border_mask0, *border_mask1, *scale0, *scale1;
    /* conf_matrix[n,L,S]: the published confidence matrix (the drop-in CoarseMatching publishes it, coarse_matching.py:145), or
     * NULL for callers that only consume the match lists: the matrix then lives in the workspace only. */
    float* conf_matrix;
    /* Outputs of capacity n*L: b_ids, i_ids, j_ids (int64), mconf, mkpts0_c / mkpts1_c [.,2] (x,y); counts[n+1] (int32): matches
     * per pair, then the total M (read it after synchronising). */
    long long *b_ids, *i_ids, *j_ids;
    float *mconf, *mkpts0_c, *mkpts1_c;
    int* counts;
    void* workspace; size_t workspace_bytes;
    /* POPE_PREC_* of the L x S x C contraction; POPE_PREC_F16X3 needs C % 32 == 0 (feat / sqrt(C) kept as hi/lo planes,
     * range-guarded: POPE_RANGE_MATCH); everything after the contraction is identical. */
    int precision;
    unsigned* range_flag;
} pope_dense_match_args;
/* Reads n, L, S, C, precision, match_type, and whether conf_matrix and either border mask are non-NULL; 0 for a NULL struct or
 * non-positive sizes. */
size_t pope_dense_match_workspace_bytes(const pope_dense_match_args* args_host);
int pope_dense_match_f32(const pope_dense_match_args* args_host, void* stream);

/* ---- LoFTR encoder layer (first slice) ---------------------------------------------------- */

/* LoFTREncoderLayer.forward — src/matcher/loftr_module/transformer.py:35-58: x[n,L,C] <- x + norm2(mlp(cat[x, norm1(merge(
 * attention(q(x), k(source), v(source))))])), in place; source[n,S,C] may be x itself ('self' layers).  C = 256 (coarse) or 128
 * (fine), nhead = 8.
 * The five bias-free Linears are given as f16x3 WEIGHT planes (layout above): q_wp [C,C], kv_wp [2C,C] (k_proj rows,
 * then v_proj rows), merge_wp [C,C], mlp0_wp [2C,2C], mlp1_wp [C,2C]; LayerNorm eps = ln_eps (nn.LayerNorm default
 * 1e-5).  LocalFeatureTransformer.forward (:85-106) is a sequence of these calls: 'self' = (f0,f0),(f1,f1); 'cross' =
 * (f0,f1) then (f1, NEW f0).
 * precision = POPE_PREC_F16X3, or POPE_PREC_F32_MFMA: the re-run of a range-guard event — the five `*_wp` are then plain fp32
 * [out, in] matrices and every contraction runs on the fp32 MFMA (no range contract; range_flag is not touched).
 * attention = POPE_LOFTR_ATTN_LINEAR: LinearAttention (linear_attention.py:20-47) with optional padding masks (:35-41; NULL = no
 * mask), 0 / 1 as fp32: x_mask[n,L] zeroes Q of padded query rows (their message is 0), source_mask[n,S] zeroes K and V of
 * padded source rows (V / S keeps the full length S).
 * attention = POPE_LOFTR_ATTN_FULL: FullAttention (linear_attention.py:50-81, the config's attention = 'full'): message =
 * softmax(Q K^T / sqrt(D), over the S source rows) V per head, D = C / nhead; everything around it, the weights struct and the
 * workspace are the same.  No masks (a padded query row is NaN in the reference): a non-NULL mask is POPE_ERR_ARG.  The softmax
 * runs in fp32 under both precisions (S > 64: flash-style on the fp32 MFMA, online softmax, nothing of size L x S is stored;
 * S <= 64: fp32 FMAs, one workgroup per 32 queries of a sequence); POPE_PREC_F16X3 writes the message as the merge GEMM's operand
 * planes and ORs POPE_RANGE_QKV into range_flag when a scaled value leaves the f16 range.  Every output row is bit-identical
 * whatever n.  POPE_ERR_ARG before any launch: null pointers, C not 128 / 256, nhead != 8, non-positive sizes, an unknown
 * precision.
 * An unknown `attention` is POPE_ERR_ARG. */
typedef struct pope_loftr_layer_weights {
    const void *q_wp, *kv_wp, *merge_wp, *mlp0_wp, *mlp1_wp;
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} pope_loftr_layer_weights;
enum { POPE_LOFTR_ATTN_LINEAR = 0, POPE_LOFTR_ATTN_FULL = 1 };
size_t pope_loftr_layer_workspace_bytes(int n, int L, int S, int C, int nhead);
int pope_loftr_encoder_layer_f32(const pope_loftr_layer_weights* w_host, float* x, const float* source,
                                 const float* x_mask, const float* source_mask,
                                 int n, int L, int S, int C, int nhead, float ln_eps, int attention, int precision,
                                 void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream);
/* The FULL attention core of that layer alone: q[n L, C], kv[n S, 2C] (k in columns 0..C-1, v in C..2C-1) fp32, 16-byte aligned
 * -> out[n L, C] fp32 rows.  precision is validated (F32_MFMA or F16X3; both run the fp32 kernels); range_flag is not
 * touched.  Same argument checks. */
int pope_loftr_full_attention_f32(const float* q, const float* kv, int n, int L, int S, int C, int nhead, int precision,
                                  float* out, unsigned* range_flag, void* stream);

/* The LINEAR attention core of pope_loftr_encoder_layer_f32 alone, by the layer's own launches: q[n L, C],
 * kv[n S, 2C] (k in columns 0..C-1, v in C..2C-1) fp32; x_mask[n,L] / source_mask[n,S] as in the layer, each may be
 * NULL.  Exactly one output: out_f32[n L, C] fp32 rows (what the layer computes under POPE_PREC_F32_MFMA), or out_planes
 * [n L, C] activation planes (scale 8; what it computes under POPE_PREC_F16X3), which ORs POPE_RANGE_INPUT into range_flag
 * (may be NULL) when a scaled value leaves the f16 range.  The per-head state is summed over the source rows in chunks of
 * `chunk_rows` rows, the partial sums in chunk order; a workgroup of the message kernel serves `rows_per_block` query rows
 * (pope_loftr_linear_attention_seams).  workspace: 256-byte aligned, pope_loftr_linear_attention_workspace_bytes (0 for
 * non-positive sizes, C not 128 / 256 or nhead != 8).  POPE_ERR_ARG before any HIP call: null q / kv / workspace,
 * non-positive sizes, C not 128 / 256, nhead != 8, both outputs or none, a misaligned workspace, n L or n S beyond the
 * layer's index range (2^31 / 2C rows); POPE_ERR_WORKSPACE for a short workspace. */
size_t pope_loftr_linear_attention_workspace_bytes(int n, int S, int C, int nhead);
void pope_loftr_linear_attention_seams(int* chunk_rows, int* rows_per_block);
int pope_loftr_linear_attention_f32(const float* q, const float* kv, const float* x_mask, const float* source_mask,
                                    int n, int L, int S, int C, int nhead, float* out_f32, void* out_planes,
                                    void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream);

/* ResNetFPN_8_2.forward — src/matcher/backbone/resnet_fpn.py:100-118 (BasicBlock :15-40), eval mode: the LoFTR
 * matcher's local-feature CNN.  gray[n,1,H,W] in [0,1], H and W multiples of 8.  Every convolution is an f16x3 planes
 * GEMM over zero-bordered NHWC activations (3x3 stride 1: implicit, no im2col; pope_amd/csrc/conv.hip); eval-mode
 * BatchNorm is folded into filter and bias by the caller.  Weights: planes (pope_split_planes_f32, scale 256) of
 * [Cout, K] matrices with K = taps x input channels rounded up to 32 (zero filled), tap-major (ky, kx, c):
 *   0 conv1+bn1 (K = 64: the 49 taps of the 7x7)            1..4  layer1: b0.conv1, b0.conv2, b1.conv1, b1.conv2
 *   5..9  layer2: b0.conv1, b0.conv2, b0.downsample (1x1), b1.conv1, b1.conv2        10..14 layer3: the same
 *   15 layer3_outconv  16 layer2_outconv  17 layer2_outconv2[0]+bn  18 layer2_outconv2[3]
 *   19 layer1_outconv  20 layer1_outconv2[0]+bn  21 layer1_outconv2[3]
 * b[i] = folded bias [Cout] or NULL (15, 16, 18, 19, 21).  Channel widths 128 / 196 / 256 (cvpr_ds_config.py).
 * Outputs are NHWC with a one-pixel border: out_c[n, H/8+2, W/8+2, 256] (x3_out; border zero) and
 * out_f[n, H/2+2, W/2+2, 128] (x1_out; border undefined) — the reference's NCHW maps are the interiors, permuted.
 * precision = POPE_PREC_F16X3, or POPE_PREC_F32_MFMA (the re-run of a range-guard event): w[i] are then the same [Cout, K]
 * matrices as plain fp32 and every convolution runs on the fp32 MFMA (gemm_f32.hip, implicit 3x3 loader).
 * POPE_PREC_F16 (opt-in): one f16 MFMA per product, fp32 accumulate.  w[i] are plain f16 row-major matrices, value *
 * POPE_PLANES_W_SCALE, [Cout, K] with the input channels of every tap rounded up to 64 (zero filled; matrix 0: K = 128, the 49
 * taps then zeros); activations travel between the layers as f16 rows, value * POPE_PLANES_ACT_SCALE, each rounded once in its
 * producer's epilogue.  Same workspace, same fp32 outputs; POPE_RANGE_INPUT when a scaled activation leaves the f16 range or is
 * not finite — the caller re-runs with POPE_PREC_F32_MFMA as for POPE_PREC_F16X3. */
typedef struct pope_resnetfpn_weights {
    const void* w[22];
    const float* b[22];
} pope_resnetfpn_weights;
size_t pope_resnetfpn_workspace_bytes(int n, int H, int W);
int pope_resnetfpn_forward_f32(const pope_resnetfpn_weights* w_host, const float* gray, int n, int H, int W, int precision,
                               float* out_c, float* out_f, void* workspace, size_t workspace_bytes,
                               unsigned* range_flag, void* stream);

/* Test entry of the convolution forms: ONE layer of the call above (or the SAM neck's 3x3), exactly its launch sequence, on
 * the caller's device buffers.  A pixel-row tensor [n, Hp, Wp, cch] is NHWC over the ZERO-BORDERED grid Hp = H + 2, Wp = W + 2,
 * one pixel = one row of cch chunks of 128 bytes: 32 planes columns (POPE_PREC_F16X3), 32 floats (POPE_PREC_F32_MFMA) or 64
 * plain f16 columns = value * 8 (POPE_PREC_F16).  Weights [N, K] as above (tap-major columns, channels padded to the chunk):
 * planes x 256, plain fp32, or f16 row-major x 256.  H, W: the interior of the INPUT grid (STEM: the image).
 *   form              operand a                       runs                                                    output grid
 *   POPE_CONV3        [n,H+2,W+2,cch]                 implicit 3x3 stride 1, K = 9 cch chunks                  H x W
 *   POPE_CONV_S2      [n,H+2,W+2,cch]                 taps = 9 (3x3 pad 1) or 1 (1x1), stride 2: straight from a where the
 *                                                     call fills a round of the CUs, else gather_s2 -> scratch + GEMM    H/2 x W/2
 *   POPE_CONV1_UP     [n,H+2,W+2,cch]                 1x1 + bilinear x2 (align_corners) of up_src [n,H/2+2,W/2+2,up_lds]
 *                                                     fp32 (zero-bordered), added before the activation        H x W
 *   POPE_CONV_STEM    gray image [n,H,W] fp32         7x7 stride 2 pad 3: stem_gather -> scratch [.., 64] + GEMM (K = 64)   H/2 x W/2
 * out = act(conv + bias [+ res]), act(v) = max(v, 0) + slope min(v, 0).  Exactly one of out_planes [rows, ldc] (planes x 8,
 * ldc = N rounded up to 32, the padding columns written as zeros; POPE_RANGE_INPUT when a value leaves the f16 range) and
 * out_f32 [rows, ldc] (ldc >= N, ldc % 4 == 0; columns >= N untouched; no range flag), rows = all pixels of the bordered output
 * grid.  POPE_PREC_F32_MFMA writes fp32 rows only (out_f32).  zero_border != 0 zeroes the border pixels' rows afterwards; a planes
 * output of CONV3 / CONV1_UP and every STEM call must ask for it (the next layer reads the border as the padding), CONV_S2 and the
 * fp32 outputs of CONV3 may leave them undefined.  res (CONV3 only): [rows, ldres] planes, or fp32 rows with POPE_PREC_F32_MFMA.
 * Served: CONV3 in all three precisions (POPE_PREC_F16: fp32 output, no res), STEM in F16X3 and F32_MFMA, the others F16X3.
 * Refused with POPE_ERR_ARG before any HIP call:
 *   - n, H, W < 1; N < 4, N % 4 != 0 or N > 256 (the widest tile of the 256-row routes); cch < 1, or a K of fewer than two
 *     chunks (CONV1_UP and CONV_S2 with taps = 1 need cch >= 2); STEM with cch != 0 or taps != 0
 *   - odd H or W for CONV_S2, CONV1_UP (whose epilogue needs Wp >= 4) and STEM
 *   - a_rows, the pixel rows the operand buffer holds, below n (H+2) (W+2): the loaders dereference every one of them (the
 *     fp32 loader through a raw pointer, M + 2 Wp + 2 rows)
 *   - out_planes with ldc != N rounded up to 32, or without zero_border where required; out_f32 with ldc < N or ldc % 4 != 0
 *   - res or up_src with a pitch below N, ldres % 32 != 0 (planes) / ldres % 4 != 0 (fp32), up_lds % 4 != 0
 *   - CONV_S2 / STEM without `scratch` (pope_conv_layer_scratch_bytes; a short one is POPE_ERR_WORKSPACE)
 *   - any buffer of 4 GiB or more (32-bit offsets), any pointer not 16-byte aligned. */
enum { POPE_CONV3 = 0, POPE_CONV_S2 = 1, POPE_CONV1_UP = 2, POPE_CONV_STEM = 3 };
typedef struct pope_conv_layer_args {
    int form, precision;
    int n, H, W;
    int cch, taps;                 /* taps: CONV_S2 only (9 or 1), else 0 */
    const void* a;
    size_t a_rows;                 /* pixel rows in a's buffer (STEM: ignored) */
    const void* w;
    const float* bias;             /* [N] or NULL */
    int N, ldc;
    float slope;
    void* out_planes;
    float* out_f32;
    int zero_border;
    const void* res;               /* CONV3: [rows, ldres] or NULL */
    int ldres;
    const float* up_src;           /* CONV1_UP */
    int up_lds;
    void* scratch;
    size_t scratch_bytes;
    unsigned* range_flag;
} pope_conv_layer_args;
size_t pope_conv_layer_scratch_bytes(int form, int n, int H, int W, int cch, int taps);
int pope_conv_layer_f32(const pope_conv_layer_args* args_host, void* stream);
/* The same struct and the same layer functions for the POPE_PREC_F16 ResNet-FPN (precision must be POPE_PREC_F16), all four
 * forms.  A chunk is 64 plain f16 columns (value * 8); weights are f16 row-major x 256, tap-major, channels padded to the chunk
 * (STEM: [N, 128], the 49 taps then zeros; its scratch row holds them the same way).  out_planes and res are F16 ROWS: ldc and
 * ldres count 4-byte units, i.e. column pairs — ldc = (N rounded up to 64) / 2, the padding columns written as zeros, every value
 * rounded once as f16(act(acc + bias [+ res]) * 8); 2 ldres >= N and ldres % 32 == 0.  out_f32 (CONV3 only) as in the entry above.
 * POPE_RANGE_INPUT is ORed into range_flag when a value written as f16 (or a STEM input) does not fit f16 at scale 8 or is not
 * finite.  Everything else — grids, zero_border, scratch, up_src, the 4 GiB and alignment rules — as above; the whole contract is
 * checked on the host before any HIP call (POPE_ERR_ARG, a short scratch POPE_ERR_WORKSPACE): res or up_src with the wrong form
 * (res with CONV1_UP included), out_f32 with another form than CONV3, a misaligned or short buffer. */
int pope_conv_layer_f16(const pope_conv_layer_args* args_host, void* stream);

/* FinePreprocess.forward — src/matcher/loftr_module/fine_preprocess.py:29-59 (fine_concat_coarse_feat = True), for
 * M > 0 matches: Wn x Wn windows (zero padded by Wn/2) of the 1/2-resolution maps centred on the matched coarse
 * cells (i_ids in map 0, j_ids in map 1; cell id = cy * wc + cx, centre pixel = cell * stride), concatenated with
 * down_proj(coarse feature of the cell) and passed through merge_feat.  Only the M matched windows are gathered (the
 * reference unfolds all of them first).  feat_f*: fp32 maps addressed through ELEMENT strides strides*_host[4] =
 * (n, c, h, w), so NCHW tensors and NHWC views both work; feat_c0[n,L,Cc], feat_c1[n,S,Cc]; b/i/j_ids: int64[M];
 * down_wp[Cf,Cc], merge_wp[Cf,2*Cf]: weight planes (scale 256) — plain fp32 matrices for precision = POPE_PREC_F32_MFMA, the
 * re-run of a range-guard event —, biases fp32; out[2*M, Wn*Wn, Cf] = windows of stream 0 then stream 1 (the reference's
 * torch.chunk(…, 2)).
 * ref0_of_pair = NULL: feat_f0 has one row per pair (n, n0 unused).  Otherwise SHARED map-0 rows (one reference image matched
 * against many crops): feat_f0 has n0 rows, and the windows of match m in map 0 are read at row ref0_of_pair[b_ids[m]].
 * ref0_of_pair: int64[n] (DEVICE), n = the number of pairs, n, n0 >= 1; feat_c0 stays [n, L, Cc] and indexed by b_ids[m] (it is
 * the per-pair transformer output), and so does everything of stream 1.  A pair outside [0, n) and a row outside [0, n0) are
 * clamped on the device (a wrong window, never a read outside the map).
 * n < 0, n0 < 0 and null feature / id / weight / out / workspace pointers return POPE_ERR_ARG before any HIP call. */
size_t pope_fine_preprocess_workspace_bytes(int M, int Wn, int Cc, int Cf);
int pope_fine_preprocess_f32(const float* feat_f0, const long long* strides0_host, int H0, int W0, int wc0,
                             const float* feat_f1, const long long* strides1_host, int H1, int W1, int wc1,
                             const float* feat_c0, const float* feat_c1, int L, int S, int Cc, int Cf,
                             const long long* b_ids, const long long* i_ids, const long long* j_ids, int M,
                             int Wn, int stride, const void* down_wp, const float* down_b, const void* merge_wp,
                             const float* merge_b, int precision, float* out, void* workspace, size_t workspace_bytes,
                             unsigned* range_flag, const long long* ref0_of_pair, int n, int n0, void* stream);
/* FineMatching.forward + get_fine_match — src/matcher/utils/fine_matching.py:15-74 for M > 0: correlation of the
 * centre of window 0 with window 1 (temperature 1/sqrt(C)), softmax, expectation over linspace(-1,1,Wn)^2 as (x, y)
 * and the summed standard deviation -> expec_f[M,3]; mkpts1_f[M,2] = mkpts1_c + expec_xy * (Wn/2) * scale_px
 * (scale_px = hw0_i[0] / hw0_f[0]).  win0, win1: [M, Wn*Wn, C] fp32 (the fine transformer's outputs).
 * Optional per-pair rescaling (fine_matching.py:68): scale1[n,2] (x, y) with b_ids int64[M] (the matches' pairs):
 * mkpts1_f[m] = mkpts1_c[m] + expec_xy * (Wn/2) * (scale_px * scale1[b_ids[m]]).  scale1 = NULL: none (b_ids unused). */
int pope_fine_match_f32(const float* win0, const float* win1, int M, int Wn, int C, const float* mkpts1_c,
                        float scale_px, const float* scale1, const long long* b_ids, float* expec_f,
                        float* mkpts1_f, void* stream);

/* ---- SAM image encoder (BASELINE config 5) --------------------------------------------------- */

/* ImageEncoderViT.forward — segment_anything/segment_anything/modeling/image_encoder.py:107-118 as build_sam.py:66-79
 * configures it (LayerNorm eps 1e-6, qkv bias, absolute + decomposed relative position terms, window attention with
 * `window` x `window` windows except in the blocks marked global, MLP ratio = hidden / dim, neck 1x1 conv ->
 * LayerNorm2d -> 3x3 conv -> LayerNorm2d).  image[B,3,img,img] fp32 (already normalised and padded by the caller,
 * sam.py preprocess) -> out[B,out_chans,g,g] fp32, g = img / patch.  head_dim = dim / heads must be 64 (ViT-B/L) or
 * 80 (ViT-H); dim % 128 == 0; out_chans % 256 == 0; patch % 8 == 0.  precision POPE_PREC_F16X3: fp32 operands as
 * hi + lo f16 planes, three MFMAs per product; POPE_PREC_F16: plain f16 operands, one MFMA per product (see the field);
 * fp32 accumulation, softmax, LayerNorm, GELU and residual stream in both.
 * Weights: `*_wp` = weight planes (pope_split_planes_f32, scale 256; POPE_PREC_F16: f16 row-major, value * 256) of the
 * torch [out, in] matrices —
 * patch_wp[dim, 3 patch^2] = proj.weight.reshape(dim, -1); neck0_wp[out_chans, dim]; neck2_wp[out_chans, 9 out_chans]
 * with the taps in (ky, kx, channel) order = weight.permute(0, 2, 3, 1).reshape(out_chans, -1).  pos[g*g, dim] or NULL.
 * rel_h / rel_w: the tables get_rel_pos returns (image_encoder.py:288-316), R[q][k][head_dim] fp32 with q, k < window
 * (window blocks) or < g (global blocks); the bias q.Rh + q.Rw is folded into the score product (sam_attention.hip).
 * ones[dim] = 1.0f.  blocks_host: HOST array [depth] of device pointers.  Optional taps as pope_vit_forward_f32
 * (tap_out_host[t][B*g*g, dim] fp32 = output of block tap_blocks_host[t]). */
typedef struct pope_sam_block_weights {
    const float *norm1_w, *norm1_b;
    const void* qkv_wp; const float* qkv_b;
    const void* proj_wp; const float* proj_b;
    const float *rel_h, *rel_w;
    const float *norm2_w, *norm2_b;
    const void* fc1_wp; const float* fc1_b;
    const void* fc2_wp; const float* fc2_b;
    int global_attn;
} pope_sam_block_weights;
typedef struct pope_sam_encoder_weights {
    int img, patch, dim, depth, heads, hidden, out_chans, window;
    int precision;   /* POPE_PREC_F16X3, or POPE_PREC_F16: BASELINE config 5's "fp16" — every `*_wp` is then a plain f16
                      * row-major matrix (value * 256) and every contraction ONE f16 MFMA per product with fp32
                      * accumulation; residual stream, softmax, LayerNorm statistics and GELU stay fp32 —, or
                      * POPE_PREC_F32_MFMA: every `*_wp` is a plain fp32 matrix and every contraction runs on the fp32 MFMA (the
                      * reference's arithmetic, no range contract: what a range-guard event is re-run in; ~10x slower) */
    const void* patch_wp; const float* patch_b;
    const float* pos;
    const float* ones;
    const pope_sam_block_weights* blocks_host;
    const void* neck0_wp;
    const float *neck1_w, *neck1_b;
    const void* neck2_wp;
    const float *neck3_w, *neck3_b;
    float block_eps, neck_eps;   /* LayerNorm eps of the blocks' norm1 / norm2 (build_sam.py:71: 1e-6; nn.LayerNorm's default: 1e-5)
                                  * and of the neck's two LayerNorm2d (common.py:28: 1e-6); <= 0 selects 1e-6 */
} pope_sam_encoder_weights;
size_t pope_sam_encoder_workspace_bytes(const pope_sam_encoder_weights* w_host, int B);
int pope_sam_encoder_forward_f32(const pope_sam_encoder_weights* w_host, const float* image, int B, float* out,
                                 int n_taps, const int* tap_blocks_host, float* const* tap_out_host,
                                 void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream);

/* ---- SAM mask decoder (point, box and mask prompts) ------------------------------------------------------------ */

/* MaskDecoder.forward with TwoWayTransformer — segment_anything/segment_anything/modeling/{mask_decoder,transformer}.py as
 * build_sam.py configures them (dim 256, 8 heads, attention_downsample_rate 2, mlp_dim 2048, depth 2, a 64 x 64 embedding,
 * 4 mask tokens, IoU head depth 3 / hidden 256).  image[256, 64, 64] and image_pe[256, 64, 64] fp32 (one image);
 * sparse[P, n_sparse, 256] (0 <= n_sparse <= 11; NULL when 0); dense[P, 256, 64, 64] with dense_stride floats between
 * prompts: 0 (a broadcast, what PromptEncoder returns without a mask: layer 0's image-only projections then run once per
 * call) or 256 * 4096 (an embedding per prompt, what pope_sam_mask_embed_f32 writes for mask prompts).  multimask != 0:
 * masks[P, 3, 256, 256] = mask tokens 1..3 and iou[P, 3]; else masks[P, 1, 256, 256] = mask token 0 and iou[P, 1]
 * (predict_masks' slices).  Optional hs_out[P, 5 + n_sparse, 256] (final tokens) and
 * keys_out[P, 4096, 256] (final image tokens).  The prompts run in chunks: the workspace is bounded by 16 prompts, and a
 * prompt's outputs are bit-identical whatever P and wherever it falls.
 * precision POPE_PREC_F16X3: the image-side Linears (`*_wp`) on weight planes (scale 256), their activations as planes
 * (range-guarded: POPE_RANGE_LAYERNORM, POPE_RANGE_QKV); POPE_PREC_F32_MFMA: every `*_wp` a plain fp32 matrix on the fp32
 * GEMM.  Token-side Linears, attention, LayerNorms and the upscaling tail are fp32 in both.
 * Layouts (torch [out, in] unless stated): sa_qkv_w[768, 256] = q | k | v of self_attn; img_qk_wp[256, 256] =
 * cross_attn_token_to_image.k_proj | cross_attn_image_to_token.q_proj (both read keys + pe); img_v_wp[128, 256] =
 * cross_attn_token_to_image.v_proj; i2t_kv_w[256, 256] = cross_attn_image_to_token.k_proj | v_proj; tokens[5, 256] = iou
 * token, mask tokens; up1_wp[256, 256]: row tap * 64 + co (tap = 2 dy + dx) = output_upscaling[0].weight[:, co, dy, dx],
 * up1_b[256] its bias per row; up2_w[128, 64]: row tap * 32 + c = output_upscaling[3].weight[:, c, dy, dx] (fp32);
 * hyper_w / hyper_b[3 i + j] = output_hypernetworks_mlps[i].layers[j]; iou_w / iou_b[j] = iou_prediction_head.layers[j]. */
typedef struct pope_sam_decoder_layer_weights {
    const float *sa_qkv_w, *sa_qkv_b, *sa_o_w, *sa_o_b, *norm1_w, *norm1_b;
    const float *t2i_q_w, *t2i_q_b, *t2i_o_w, *t2i_o_b, *norm2_w, *norm2_b;
    const float *mlp1_w, *mlp1_b, *mlp2_w, *mlp2_b, *norm3_w, *norm3_b;
    const float *i2t_kv_w, *i2t_kv_b;
    const void* img_qk_wp; const float* img_qk_b;
    const void* img_v_wp; const float* img_v_b;
    const void* i2t_o_wp; const float* i2t_o_b;
    const float *norm4_w, *norm4_b;
} pope_sam_decoder_layer_weights;
typedef struct pope_sam_decoder_weights {
    int dim, heads, mlp_dim, depth, grid, num_mask_tokens, iou_hidden, iou_depth;
    int precision;                /* POPE_PREC_F16X3 or POPE_PREC_F32_MFMA */
    float token_eps, up_eps;      /* nn.LayerNorm of the tokens / image tokens (1e-5); LayerNorm2d of the upscaling (1e-6) */
    const float* tokens;
    const pope_sam_decoder_layer_weights* layers_host;   /* HOST array [depth] */
    const float *fin_q_w, *fin_q_b;
    const void* fin_k_wp; const float* fin_k_b;
    const void* fin_v_wp; const float* fin_v_b;
    const float *fin_o_w, *fin_o_b, *norm_final_w, *norm_final_b;
    const void* up1_wp; const float* up1_b;
    const float *up_ln_w, *up_ln_b, *up2_w, *up2_b;
    const float* hyper_w[12];
    const float* hyper_b[12];
    const float* iou_w[3];
    const float* iou_b[3];
} pope_sam_decoder_weights;
/* 0 for an unsupported geometry or argument; shared != 0: the dense embedding is a broadcast (dense_stride 0). */
size_t pope_sam_decoder_workspace_bytes(const pope_sam_decoder_weights* w_host, int P, int n_sparse, int shared);
int pope_sam_decoder_forward_f32(const pope_sam_decoder_weights* w_host, const float* image, const float* image_pe,
                                 const float* sparse, int P, int n_sparse, const float* dense, long long dense_stride,
                                 int multimask, float* masks, float* iou, float* hs_out, float* keys_out,
                                 void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream);
/* The same decoder over the prompts of N images in one call (Sam.forward's workload: a few prompts on each of several
 * images).  images[N, 256, 64, 64] fp32; prompt_image_host[P]: a HOST int array in any order, entry p the image of prompt p
 * (0 <= entry < N is checked on the host: a bad index is POPE_ERR_ARG before any launch); dense[256, 64, 64] with
 * dense_stride 0, the broadcast PromptEncoder returns without a mask (any other stride is POPE_ERR_ARG); the other arguments
 * as above, without hs_out / keys_out.  Layer 0's image-only projections run once per image (GEMMs over up to 16 x 4 096
 * rows), the 16-prompt chunks fill across images (a chunk's image indices travel as a kernel argument: no device copy, no
 * synchronisation, no allocation), and range_flag covers the whole call.  masks / iou of prompt p are bit-identical to
 * pope_sam_decoder_forward_f32 on prompt p with images[prompt_image_host[p]] alone, whatever N, P, the order of the prompts
 * and the chunk a prompt falls in, in both precisions.  The workspace holds the layer-0 buffers once per image (18 MB each)
 * on top of the 16-prompt chunk; the query returns 0 for an unsupported geometry or argument (N <= 0, a NULL or
 * out-of-range prompt_image_host, dense_stride != 0). */
size_t pope_sam_decoder_images_workspace_bytes(const pope_sam_decoder_weights* w_host, int N, const int* prompt_image_host,
                                               int P, int n_sparse, long long dense_stride);
int pope_sam_decoder_forward_images_f32(const pope_sam_decoder_weights* w_host, const float* images, int N,
                                        const float* image_pe, const float* sparse, const int* prompt_image_host, int P,
                                        int n_sparse, const float* dense, long long dense_stride, int multimask, float* masks,
                                        float* iou, void* workspace, size_t workspace_bytes, unsigned* range_flag,
                                        void* stream);
/* The decoder's kernels one at a time, as the decoder launches them (for tests that compare one kernel with a reference).  All
 * pointers are DEVICE pointers except slot_host (HOST [P]: entry p selects which block of a strided buffer prompt p reads; every
 * entry >= 0).  T = tokens per prompt, 1 .. max_tokens; P = prompts of the launch, 1 .. chunk (self-attention, linear: no such
 * limit).  The image side is always 4 096 tokens.  Each entry returns POPE_ERR_ARG before any launch for a NULL pointer, a size
 * out of range, a buffer read as float4 that is not 16-byte aligned or a stride that is no multiple of 4 floats.
 *   seams: chunk = prompts per pass over the image side, lin_rows = rows per workgroup of the token linear, max_tokens,
 *     base_tokens = iou token + mask tokens (T = base_tokens + n_sparse).
 *   token_linear: Y[m, n] = act(sum_k X'[m, k] W[n, k] + bias[n]) (+ res[m, n]); X' = X + add for the columns n < add_cols (add
 *     may be NULL), X otherwise; rows of X and add have pitch ldx >= K, rows of Y and res pitch ldy >= N; K % 4 == 0, W 16-byte
 *     aligned; the staged rows (lin_rows x K floats, twice with add) must fit 64 KiB of LDS.
 *   self_attention: qkv[P T, 768] = q | k | v (8 heads of 32) -> out[P T, 256].
 *   t2i_attention: q[P T, 128] against the 4 096 keys K + slot[p] * kps (rows of pitch ldk >= 128) and values V + slot[p] * vps
 *     (rows of 128), 8 heads of 16 -> out[P T, 128].
 *   i2t_attention: the 4 096 queries Q + slot[p] * qps (rows of 256, the first 128 columns read) against kv[P T, 256] = k | v ->
 *     [P 4096, 128] as fp32 rows or activation planes (exactly one; planes: POPE_RANGE_QKV).
 *   residual_norm: keys[p, n] = LayerNorm(res[slot[p] * rps + n] + y[p, n]) * w + b over 256 columns; f32 != 0: opB = fp32
 *     keys + pe_t[n]; else opA = planes(keys), opB = planes(keys + pe_t[n]) (POPE_RANGE_LAYERNORM).
 *   prepare_keys: keys[z] = (image + z * image_stride + dense + z * dense_stride)^T for z < nz <= chunk ([256, 4096] ->
 *     [4096, 256]), pe_t = image_pe^T, and the operands as above.
 *   upscale_tail: y[P 4096, 256] (the first ConvTranspose's output, column tap * 64 + channel) -> LayerNorm2d(eps), GELU, second
 *     ConvTranspose w2[128, 64] + b2[32], GELU, dot with hyper[P, 4, 32] -> masks[P, 3 or 1, 256, 256] (multimask: masks 1..3). */
void pope_sam_decoder_seams(int* chunk, int* lin_rows, int* max_tokens, int* base_tokens);
int pope_sam_decoder_token_linear_f32(const float* X, int ldx, const float* add, int add_cols, const float* W, const float* bias,
                                      const float* res, float* Y, int ldy, int M, int N, int K, int relu, void* stream);
int pope_sam_decoder_self_attention_f32(const float* qkv, float* out, int P, int T, void* stream);
int pope_sam_decoder_t2i_attention_f32(const float* q, const float* K, int ldk, long long kps, const float* V, long long vps,
                                       const int* slot_host, float* out, int T, int P, void* stream);
int pope_sam_decoder_i2t_attention_f32(const float* Q, long long qps, const int* slot_host, const float* kv, int T, int P,
                                       float* out_f32, void* out_planes, unsigned* range_flag, void* stream);
int pope_sam_decoder_residual_norm_f32(const float* res, long long rps, const int* slot_host, const float* y, const float* w,
                                       const float* b, float eps, const float* pe_t, float* keys, void* opA, void* opB, int f32,
                                       int P, unsigned* range_flag, void* stream);
int pope_sam_decoder_prepare_keys_f32(const float* image, long long image_stride, const float* image_pe, const float* dense,
                                      long long dense_stride, int nz, float* keys, void* opA, void* opB, int f32, float* pe_t,
                                      unsigned* range_flag, void* stream);
int pope_sam_decoder_upscale_tail_f32(const float* y, const float* ln_w, const float* ln_b, float eps, const float* w2,
                                      const float* b2, const float* hyper, int multimask, int P, float* masks, void* stream);

/* ---- SAM prompt encoder: mask prompts --------------------------------------------------------------------------- */

/* PromptEncoder._embed_masks — segment_anything/segment_anything/modeling/prompt_encoder.py:51-59, 102-105: mask_downscaling =
 * Conv2d(1 -> 4, k2, s2), LayerNorm2d(4), GELU (erf), Conv2d(4 -> 16, k2, s2), LayerNorm2d(16), GELU, Conv2d(16 -> 256, k1), in
 * ONE kernel without an intermediate in memory: an output pixel depends on one 4 x 4 patch of its mask.
 * masks[P, 1, 256, 256] fp32 (16-byte aligned) -> dense[P, 256, 64, 64] fp32 (16-byte aligned), channel-major: the per-prompt
 * dense embedding pope_sam_decoder_forward_f32 takes with dense_stride = 256 * 4096.  The weights are DEVICE pointers in
 * torch's native layouts; LayerNorm2d is common.py's: mean and biased variance over the channels, (x - u) / sqrt(s + eps),
 * then weight and bias per channel.  Every output element is computed by one thread in a fixed order (taps in (dy, dx, c_in)
 * order from the bias, hidden channels 0..15 in order, each step one fused multiply-add), so a prompt's embedding is
 * bit-identical whatever P and wherever it stands in the batch.  Non-finite input gives non-finite output (no check).
 * No workspace.  P <= 0, a NULL pointer (the struct, any weight, masks, dense) or another geometry than
 * (mask_in_chans, embed_dim, grid) = (16, 256, 64) returns POPE_ERR_ARG before any HIP call. */
typedef struct pope_sam_mask_embed_weights {
    int mask_in_chans, embed_dim, grid;        /* 16, 256, 64 */
    float ln1_eps, ln2_eps;                    /* LayerNorm2d eps (1e-6) */
    const float *conv1_w /* [4, 1, 2, 2] */, *conv1_b, *ln1_w, *ln1_b;
    const float *conv2_w /* [16, 4, 2, 2] */, *conv2_b, *ln2_w, *ln2_b;
    const float *conv3_w /* [256, 16] */, *conv3_b;
} pope_sam_mask_embed_weights;
int pope_sam_mask_embed_f32(const pope_sam_mask_embed_weights* w_host, const float* masks, int P, float* dense, void* stream);

/* ---- SAM automatic mask generator: post-processing of one decoder call ------------------------------------------ */

/* Sam.postprocess_masks (modeling/sam.py) and the tail of SamAutomaticMaskGenerator._process_batch in one pass over the
 * low-res logits.  low_res[M, h, w] fp32 (the decoder's masks, flattened over prompts x masks); selection[n_sel] = DEVICE
 * int32 indices into M in the order the results are wanted (NULL: the first n_sel masks; an index outside [0, M) yields an
 * empty mask); the frame: img_size (the 1024 square), (ih, iw) = the resized frame inside it, (H, W) = the original frame.
 * Per selected mask the logit of every frame pixel is the reference's two bilinear resamplings (low-res -> img_size x
 * img_size, crop to [:ih, :iw], -> H x W; align_corners=False), bit-equal to torch's CPU kernels: per axis
 * scale = (float)n_in / n_out, src = max(fmaf(scale, dst + 0.5f, -0.5f), 0), i0 = (int)src, i1 = min(i0 + 1, n_in - 1),
 * l1 = src - i0, value = fmaf(1 - l1, in[i0], l1 * in[i1]), x axis first.  Outputs:
 *   stats[n_sel, 8] int32: #(logit > thr + offset), #(logit > thr - offset), #(logit > thr), the box x0, y0, x1, y1 of
 *     logit > thr (inclusive maxima, 0 0 0 0 for an empty mask: amg.py batched_mask_to_box) and the fp32 bits of the
 *     stability score (float)n_hi / (float)n_lo; the thresholds are (float)(mask_threshold +- stability_offset);
 *   packed[n_sel, H, ceil(W / 32)] uint32 (optional): logit > thr, bit (x & 31) of word (x >> 5), pad bits zero;
 *   logits[n_sel, H, W] fp32 (optional): the dense logits (what postprocess_masks returns).
 * A mask's results do not depend on M, n_sel or the other masks of the call.  workspace: 4-byte aligned. */
size_t pope_sam_postprocess_workspace_bytes(int img_size, int H, int W);   /* 0 for an unsupported geometry */
int pope_sam_postprocess_f32(const float* low_res, int M, int h, int w, const int* selection, int n_sel, int img_size,
                             int ih, int iw, int H, int W, double mask_threshold, double stability_offset, int* stats,
                             unsigned* packed, float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* Greedy box NMS for one category as torchvision.ops.nms defines it: boxes[n, 4] fp32 XYXY, scores[n] fp32, n <= 2048;
 * order by score descending, stable; a box is dropped when its IoU with a kept box is > iou_threshold
 * (area = (x1 - x0) * (y1 - y0), iou = inter / (area_i + area_j - inter), fp32).  keep[n] int32 receives the kept indices
 * in score order, count[1] their number (both DEVICE). */
int pope_sam_nms_f32(const float* boxes, const float* scores, int n, float iou_threshold, int* keep, int* count, void* stream);
/* pope_sam_nms_f32 for S independent segments in ONE launch (one workgroup per segment; the same device function, so a segment's
 * result is bit for bit that of pope_sam_nms_f32 on its boxes).  boxes[n, 4], scores[n]; seg_offsets[S + 1] int32 (DEVICE,
 * non-decreasing, within [0, n]): segment s owns boxes seg_offsets[s] .. seg_offsets[s + 1] - 1, at most 2048 of them.
 * keep[n] int32: the kept boxes of segment s start at keep[seg_offsets[s]], in score order, as GLOBAL indices into n;
 * count[S] their numbers (0 for an empty segment).  The offsets are clamped to [0, n] on the device; a segment longer than 2048
 * is not run and gets count -1 (callers that know the offsets on the host refuse it before the call).  S == 0 is a no-op. */
int pope_sam_nms_segments_f32(const float* boxes, const float* scores, const int* seg_offsets, int S, int n, float iou_threshold,
                              int* keep, int* count, void* stream);
/* segment_anything/utils/amg.py:remove_small_regions, as automatic_mask_generator.py:postprocess_small_regions calls it
 * twice per mask (mode "holes", then "islands"), for a whole batch of bit-packed masks in ONE launch and without OpenCV.
 * packed[n, H, ceil(W / 32)] uint32 in the layout pope_sam_postprocess_f32 writes (bit (x & 31) of word (x >> 5); pad bits
 * are not pixels and are ignored).  Per mask, with 8-connected components inside the H x W image:
 *   holes: every component of the COMPLEMENT with fewer than min_area pixels is filled (the outer background is a component
 *     like any other: a mask with fewer than min_area background pixels becomes all foreground);
 *   islands, on the filled mask: every component with fewer than min_area pixels is removed; if all are that small, the
 *     largest stays, on an exact tie the one whose first pixel comes first in raster order.
 * Outputs: packed_out[n, H, ceil(W / 32)] (pad bits zero; packed_out == packed cleans in place, any other overlap is refused);
 * unchanged[n] int32 = 1 unless one of the two steps met a component below min_area (0 even if the mask comes out identical,
 * as for a single small island); boxes[n, 4] int32 XYXY of the cleaned mask (inclusive maxima, 0 0 0 0 for an empty mask:
 * batched_mask_to_box); area[n] int32.  H * W < 2^24, min_area >= 0; n == 0 is a no-op.  One workgroup cleans one mask and at
 * most 32 masks are in flight, so the workspace stops growing at n = 32; a mask's outputs depend neither on n nor on its
 * place in the batch, and integer atomics only make them independent of the launch order.  workspace: 4-byte aligned. */
size_t pope_sam_small_regions_workspace_bytes(int n, int H, int W);   /* 0 for an unsupported geometry or n <= 0 */
int pope_sam_small_regions_u32(const unsigned* packed, int n, int H, int W, int min_area,
                               unsigned* packed_out, int* unchanged, int* boxes, int* area,
                               void* workspace, size_t workspace_bytes, void* stream);
/* segment_anything/utils/amg.py:mask_to_rle_pytorch for a batch of bit-packed masks.  packed[n, H, ceil(W / 32)] uint32 in the
 * layout pope_sam_postprocess_f32 and pope_sam_small_regions_u32 write (bit (x & 31) of word (x >> 5); pad bits are not pixels
 * and are ignored).  Per mask, flattened COLUMN-major (i = x * H + y) with a clear virtual pixel before i = 0: with
 * t_0 < .. < t_k the indices where a pixel differs from its predecessor (a column's first pixel from the previous column's
 * last), counts = [t_0, t_1 - t_0, .., H * W - t_k]: k + 2 entries, a leading 0 when pixel (0, 0) is set, [H * W] for a mask
 * without a transition.  The output is ragged, so the entry is called twice:
 *   counts == NULL: lengths[n] int32 receives the number of entries of every mask (at most H * W + 1);
 *   counts != NULL: offsets[n + 1] int64 (DEVICE; the exclusive scan of the lengths, offsets[n] = their sum) and
 *     capacity = the number of uint32 entries `counts` holds; mask i's counts are written at [offsets[i], offsets[i + 1]).
 *     offsets[n] is read back first (one stream synchronisation): offsets[n] > capacity returns POPE_ERR_WORKSPACE and writes
 *     nothing (no clipping); no mask writes outside [offsets[i], min(offsets[i + 1], capacity)) whatever the offsets say.
 * H, W <= 2^14; n == 0 is a no-op.  One workgroup encodes one mask, without workspace and without atomics (integer arithmetic
 * only): a mask's output depends neither on n nor on its place in the batch. */
int pope_sam_rle_u32(const unsigned* packed, int n, int H, int W, int* lengths, const long long* offsets, unsigned* counts,
                     long long capacity, void* stream);

/* ---- caller-side preprocessing, batched ------------------------------------------------- */

/* set_torch_image for P crops at once — segment_anything/segment_anything/dinov2_utils.py:55-78: Resize (Pillow's
 * 8-bit bilinear resample, bit-identical) -> CenterCrop -> ToTensor -> Normalize.  img_hwc[P,Hin,Win,3] uint8 (channel
 * order as given: the drivers pass BGR); the window / weight tables of the two resample passes are DEVICE int32 arrays
 * built by the host exactly as Pillow builds them (pope_amd/preprocess.py:resize_tables): hstart/hcount[OW],
 * hk[OW,kh], vstart/vcount[OH], vk[OH,kv] with 22 fractional bits; (top,left,ch,cw) = crop window in the resized
 * image; [row0, row0+nrows) = input rows those output rows read; mean_host/std_host[3] = HOST floats;
 * out[P,3,ch,cw] fp32; scratch >= P*nrows*cw*3 bytes. */
int pope_preprocess_u8_f32(const unsigned char* img_hwc, int P, int Hin, int Win,
                           const int* hstart, const int* hcount, const int* hk, int kh,
                           const int* vstart, const int* vcount, const int* vk, int kv,
                           int top, int left, int ch, int cw, int row0, int nrows,
                           const float* mean_host, const float* std_host, float* out,
                           unsigned char* scratch, size_t scratch_bytes, void* stream);
/* SAM's input transform for P frames of one size.  The tables are those of pope_preprocess_u8_f32 (DEVICE int32, built by
 * pope_amd/preprocess.py:resize_tables for Win -> OW and Hin -> OH); the whole resized image is computed.
 * scratch >= P*Hin*OW*3 bytes (the horizontal pass of every input row).  Null pointers, non-positive sizes and (fp32 entry)
 * S % 4 != 0, OH > S, OW > S or an `out` that is not 16-byte aligned return POPE_ERR_ARG, a short scratch POPE_ERR_WORKSPACE,
 * both before any HIP call.
 *   pope_resize_u8 — ResizeLongestSide.apply_image (segment_anything/utils/transforms.py: Pillow's 8-bit bilinear resample,
 *     bit-identical): img_hwc[P,Hin,Win,3] uint8 -> out[P,OH,OW,3] uint8.
 *   pope_sam_preprocess_u8_f32 — the resample, Sam.preprocess (segment_anything/modeling/sam.py) and its pad as one result:
 *     out[P,3,S,S] fp32, out[p,c,y,x] = ((float)u8 - mean[c]) / std[c] (IEEE subtraction and division, on the 0..255 values)
 *     for y < OH, x < OW, where u8 is the resampled byte of source channel (flip ? 2 - c : c); every other element of the
 *     S x S square is +0.0, written by the same launch.  mean_host / std_host[3] = HOST floats per OUTPUT channel. */
int pope_resize_u8(const unsigned char* img_hwc, int P, int Hin, int Win,
                   const int* hstart, const int* hcount, const int* hk, int kh,
                   const int* vstart, const int* vcount, const int* vk, int kv,
                   int OH, int OW, unsigned char* out, unsigned char* scratch, size_t scratch_bytes, void* stream);
int pope_sam_preprocess_u8_f32(const unsigned char* img_hwc, int P, int Hin, int Win,
                               const int* hstart, const int* hcount, const int* hk, int kh,
                               const int* vstart, const int* vcount, const int* vk, int kv,
                               int OH, int OW, int S, int flip, const float* mean_host, const float* std_host, float* out,
                               unsigned char* scratch, size_t scratch_bytes, void* stream);
/* ToTensor + Normalize of a crop window without resizing (torchvision semantics: x / 255, then (x - mean) / std in
 * fp32) — the dense pair path's 476 x 630 centre crop of a 640 x 480 frame: img_hwc[P,Hin,Win,3] uint8 ->
 * out[P,3,ch,cw] fp32 (16-byte aligned); mean_host / std_host[3] = HOST floats in the channel order of img. */
int pope_crop_normalize_u8_f32(const unsigned char* img_hwc, int P, int Hin, int Win, int top, int left, int ch, int cw,
                               const float* mean_host, const float* std_host, float* out, void* stream);
/* cv2.cvtColor(BGR2GRAY) (8-bit fixed point) followed by / 255. — eval_linemod_json.py:103-111:
 * bgr_hwc[P,H,W,3] uint8 -> out[P,1,H,W] fp32 in [0,1] (the Matcher's input). */
int pope_gray_u8_f32(const unsigned char* bgr_hwc, int P, int H, int W, float* out, void* stream);
/* The image pair of the image-conditioned pose heads (pose/model_cnn.py, pose/model0604.py), built on the device —
 * linemod.py:107,129-130 and pose/dataset.py:102-106 (`cv2.resize(img, (224, 224))`, INTER_LINEAR on uint8), then
 * train0604.py:148-151 (`.float()`, `.permute(0, 3, 2, 1)`): src_hwc[P, Hin, Win, 3] uint8 ->
 *   transposed != 0: out[Q, 3, OW, OH] fp32, out[q, c, x, y] = (float)resized[q][y][x][c]   (the reference's layout)
 *   transposed == 0: out[Q, 3, OH, OW] fp32, out[q, c, y, x]
 * raw 0..255 values, channels in the stored order.  Output image q is the resize of src[rows[q]]: rows[Q] is a DEVICE int32
 * array, or NULL for the identity (which needs Q == P); a row outside [0, P) gives an all-zero image and is never read.
 * The resize is OpenCV's generic 8-bit INTER_LINEAR path, restated from its public algorithm and unpinned against cv2 (absent):
 * per axis DEVICE int32 tables built on the host (pope_amd/preprocess.py:resize_linear_cv_tables): xstart[OW] / ystart[OH] the
 * first tap (the second is min(first + 1, n_in - 1)), xcoef[OW, 2] / ycoef[OH, 2] the two coefficients with 11 fractional bits.
 * With h(y) = src[y][sx] * ax0 + src[y][sx1] * ax1 in int32, a pixel is
 *   (((ay0 * (h(sy) >> 4)) >> 16) + ((ay1 * (h(sy1) >> 4)) >> 16) + 2) >> 2.
 * Equal sizes are thereby a copy; when BOTH axes shrink exactly 2 x (Hin == 2 OH and Win == 2 OW) the tables are not read and a
 * pixel is (a + b + c + d + 2) >> 2 over its 2 x 2 block, as OpenCV's area path gives for that case.  Taps are clamped to the
 * image whatever the tables say.  Integer arithmetic only: a pixel depends on nothing but its source image and the tables, so an
 * image's result does not depend on Q or on its place in the batch.  One launch covers all Q; Q == 0 is a no-op.  Null pointers
 * (other than rows), non-positive sizes, Q < 0, rows == NULL with Q != P and an `out` that is not 4-byte aligned return
 * POPE_ERR_ARG before any HIP call. */
int pope_pose_images_u8_f32(const unsigned char* src_hwc, int P, int Hin, int Win, const int* rows, int Q,
                            const int* xstart, const int* xcoef, const int* ystart, const int* ycoef,
                            int OH, int OW, int transposed, float* out, void* stream);

/* Proposal crops — get_image_crop_resize (utils/data_utils.py:239-255 = cv2.warpAffine(image, M, (w, h), INTER_LINEAR), border
 * constant 0) as the drivers use it twice per SAM proposal (eval_linemod_json.py:83-90: crop at the expanded box's own size,
 * an integer translation, then a uniform resize of that crop to 256 x 256), for P proposals of one frame in one launch.
 * img_hwc[H, W, C] uint8 (C <= 4); minv[P, 6] fp64 (DEVICE): the INVERSE 2 x 3 map of each output (destination pixel ->
 * source position in window coordinates; what cv::warpAffine derives from the forward matrix); win[P, 4] int32 (DEVICE) =
 * (x0, y0, w, h): the source of output p is the w x h window of the frame at (x0, y0), everything outside the window or the
 * frame reads 0 — i.e. the reference's intermediate zero-padded crop, never materialised; (0, 0, W, H) warps the frame itself.
 * out[P, oh, ow, C] uint8.  Arithmetic: OpenCV's 8-bit bilinear convention (1/32 px positions, integer weights summing to
 * 1024, round to nearest) — restated, unpinned against cv2 (absent); integer translations are exact copies. */
int pope_crop_warp_u8(const unsigned char* img_hwc, int H, int W, int C, const double* minv, const int* win, int P,
                      int oh, int ow, unsigned char* out, void* stream);

/* ---- relative pose from the matches ----------------------------------------------------------- */

/* estimate_pose for B pairs in one launch — src/utils/metrics.py:69-94 (call site eval_linemod_json.py:160): K-normalise
 * both point sets (:72-75), threshold = thresh / mean(fx0, fy1, fx0, fy1) (:78), essential matrix by RANSAC over five-point
 * minimal samples (what cv2.findEssentialMat(..., cv2.RANSAC) does: Sampson error <= threshold^2, a model is kept when it has
 * MORE inliers than the best so far and at least five, budget log(1 - conf) / log(1 - w^5) re-evaluated after every round of
 * 256 hypotheses, at most max_iters <= 2^27 — OpenCV's default is 1000), then recoverPose for every returned E (:86-94): the
 * (R, t) of the four decompositions with the most inliers in front of both cameras.  A pair with exactly five matches is
 * the minimal problem itself: all of its solutions go through recoverPose.  All arithmetic fp64.
 * Inputs are the dense matcher's compacted outputs as they lie in HBM: kpts0 / kpts1 [M, 2] fp32 pixel coordinates with
 * the matches of pair b contiguous and pairs in order (mkpts0_c / mkpts1_c or mkpts0_f / mkpts1_f), counts [B] int32
 * (DEVICE: matches per pair, sum <= M), K0 / K1 [B, 9] fp64 row-major intrinsics of image 0 / image 1 of each pair.
 * Outputs: R [B, 9], t [B, 3] (unit norm), E [B, 9] fp64; inliers [M] bytes (RANSAC inlier AND in front of both cameras,
 * the mask recoverPose leaves behind); info [B, 8] int32 = {n_inliers of the returned pose — 0 means `None` (fewer than five
 * matches, no model with five inliers, or no point in front of both cameras) —, RANSAC inliers, hypotheses tried, rounds,
 * winning hypothesis, winning root, matches of the pair, status (-1: refused — the counts up to and including this pair exceed
 * M, or one of them is negative)}.  Rows of `inliers` past sum(counts) are not written.
 * The minimal samples of hypothesis h come from a counter-based hash of (seed, h): results do not depend on the batch a
 * pair rides in.  cv2's own random stream is not reproducible without cv2 (absent here): parity with OpenCV is unpinned,
 * the checker is oracle/pose_ref.py (same algorithm, same samples, numpy fp64).
 * Workspace (>= pope_estimate_pose_workspace_bytes(B, M), 32-byte aligned): normalised points and two masks per match, and per
 * pair the list of one round's models (256 hypotheses x <= 10 roots x 9 fp64) that spreads the scoring evenly over the threads. */
size_t pope_estimate_pose_workspace_bytes(int B, long long M);
int pope_estimate_pose_f64(const float* kpts0, const float* kpts1, const int* counts, const double* K0, const double* K1,
                           int B, long long M, double thresh, double conf, int max_iters, unsigned long long seed,
                           double* R, double* t, double* E, unsigned char* inliers, int* info,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The minimal solver alone (parity tests): S problems of five correspondences in normalised coordinates,
 * x0 / x1 [S, 5, 2] fp64 -> E_out [S, 10, 9] (unit Frobenius norm, ascending root order, zero filled), n_out [S]. */
int pope_five_point_f64(const double* x0, const double* x1, int S, double* E_out, int* n_out, void* stream);

/* ---- batched driver step: device-side vote and slot tally (vote.hip) ------------------------------------------------ */

/* CLS cosine + streaming top-3 vote for Q queries in one launch (one workgroup per query, any P; eval_linemod_json.py:93-101).
 * cls_ref [Q, D], cls_prop [N, D] fp32; seg [Q + 1] int32 (DEVICE): query q owns proposal rows seg[q] .. seg[q + 1] (P_q = 0
 * allowed; rows are clamped to [0, N]).  scores [N]: the arithmetic of pope_cls_cosine_f32, bit-equal to it called per query.
 * slot_scores [Q, 3] fp32 / slot_index [Q, 3] int64 (local to the query, -1 = slot never filled): exactly
 * pope_streaming_top3_host over the query's scores in proposal order.  pair_row [3 Q] int32: global proposal row of slot s of
 * query q (0 for a dead slot); pair_live [3 Q] bytes: 1 when the slot was filled.  Q = 0: POPE_OK, nothing launched. */
int pope_vote_top3_batch_f32(const float* cls_ref, const float* cls_prop, const int* seg, int Q, int N, int D, float eps,
                             float* scores, float* slot_scores, long long* slot_index, int* pair_row, unsigned char* pair_live,
                             void* stream);

/* The same vote for Q queries that SHARE proposal segments (several queries asked of one frame): cls_prop [N, D] holds every
 * segment once and is read in place, no gathered copy is made.  seg [S + 1] int32 (DEVICE): segment s owns rows seg[s] ..
 * seg[s + 1], clamped to [0, N] as above.  query_seg [Q] int32 (DEVICE): query q votes over segment query_seg[q]; a value
 * outside [0, S) is an empty segment.  score_begin [Q + 1] int32 (DEVICE): query q's scores go to scores[score_begin[q] ..),
 * in proposal order; at most score_begin[q + 1] - score_begin[q] of them are written and voted on (none when score_begin[q]
 * is negative), so `scores` holds score_begin[Q] floats.  slot_scores / slot_index as above, slot_index local to the segment;
 * pair_row [3 Q] is the GLOBAL row in N (two queries may name the same row), 0 for a dead slot.  A query with an empty
 * segment still gets its three slots written as dead.  pope_vote_top3_batch_f32 is this entry with query_seg[q] = q and
 * score_begin = seg: one device body serves both, bit for bit.  Q = 0: POPE_OK, nothing launched. */
int pope_vote_top3_shared_f32(const float* cls_ref, const float* cls_prop, const int* seg, int S, const int* query_seg,
                              const int* score_begin, int Q, int N, int D, float eps, float* scores, float* slot_scores,
                              long long* slot_index, int* pair_row, unsigned char* pair_live, void* stream);

/* The published matches of a Matcher call over 3 Q pairs (pair 3 q + s = slot s of query q) -> the pose solver's inputs.
 * m_bids [M] int64 sorted (matches pair-contiguous, pairs in order), mconf [M], mkpts0_f / mkpts1_f [M, 2] fp32, pair_live
 * [3 Q] bytes.  pair_begin / pair_count [3 Q] int32: each pair's rows in the match list; matching_score [Q, 3] int64 =
 * #(mconf > conf_thr) per slot (fp32, strict; eval_linemod_json.py:121-122), 0 for a dead slot; best_slot [Q] int32 = first
 * maximum of the three (np.argmax, :150); best_count [Q] int32 = matches of the best slot (0 when it is dead); best_kpts0 /
 * best_kpts1 [M, 2]: each query's best-slot matches, in order, at the exclusive scan of best_count — the layout
 * pope_estimate_pose_f64 takes with counts = best_count (rows past sum(best_count) are not written).
 * Two launches, integer arithmetic only, no atomics.  M = 0 or Q = 0: POPE_OK, nothing launched, nothing written. */
int pope_slot_tally_f32(const long long* m_bids, const float* mconf, const float* mkpts0_f, const float* mkpts1_f,
                        const unsigned char* pair_live, int Q, long long M, float conf_thr, int* pair_begin, int* pair_count,
                        long long* matching_score, int* best_slot, int* best_count, float* best_kpts0, float* best_kpts1,
                        void* stream);

/* ---- learned pose regressor (pose/model.py:Mkpts_Reg_Model) ------------------------------------------------------ */

/* One nn.TransformerEncoderLayer(d_model=76, nhead=2) in torch's own layouts (device pointers, fp32): in_proj [228, 76] /
 * [228], out_proj [76, 76] / [76], linear1 [2048, 76] / [2048], linear2 [76, 2048] / [76], norm1 / norm2 [76] each. */
typedef struct pope_pose_regressor_layer {
    const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b;
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} pope_pose_regressor_layer;

/* mode: POPE_ROT_MATRIX (rotation_head 32 -> 9, view(3, 3)), POPE_ROT_QUAT (32 -> 4, qua2mat, w x y z) or POPE_ROT_6D
 * (32 -> 6, o6d2mat, x y z as columns).  mlp_w[i] / mlp_b[i] = mlp.{0,3,6,9,12,15,18}: [19S, 76S], [S, 19S], [256, S],
 * [128, 256], [64, 128], [32, 64], [32, 32].  The pointers are read on every call: no derived copy exists. */
#define POPE_ROT_MATRIX 0
#define POPE_ROT_QUAT 1
#define POPE_ROT_6D 2
typedef struct pope_pose_regressor_weights {
    int num_sample, mode;
    pope_pose_regressor_layer layers[4];
    const float* mlp_w[7];
    const float* mlp_b[7];
    const float *trans_w, *trans_b, *rot_w, *rot_b;
} pope_pose_regressor_weights;

/* Mkpts_Reg_Model.forward (pose/model.py:106-114) for B pairs of S = num_sample sample slots, fp32 throughout:
 * embedding [x, sin(f x), cos(f x)] with f = linspace(1, 256, 9) and the fp32-rounded product f * x as the argument ->
 * four post-norm encoder layers (ReLU, eps 1e-5) -> mlp -> translation / rotation heads -> convert2matrix.
 * The B pairs form B / G attention groups of G consecutive pairs (1 <= G <= 64, B % G == 0): attention runs across the G
 * members of a group, separately per sample slot — the reference's batch_first=False reading of [B, S, 76] is G = B; every
 * pair on its own (the notebooks' unsqueeze(0)) is G = 1.
 * Input, one of:  dense0 / dense1 [B, S, 2] (kpts0 / kpts1 / counts NULL), or the matcher's compacted buffers kpts0 / kpts1
 * [M, 2] with pairs contiguous and counts [B] int32 on the DEVICE (dense0 / dense1 NULL; the contract of
 * pope_estimate_pose_f64).  A pair with count <= S is zero-padded to S rows; with count > S it is sampled: by sample_index
 * [B, S] int32 when given (an entry outside [0, count) sets status -2 for that pair and is not read), else by the device
 * sampler: key(i) = splitmix64(seed_b ^ (i + 1) * 0xD1B54A32D192ED03) (splitmix64 as in pose_math.h), slot j takes the match
 * with the j-th smallest (key, i).  seeds [B] uint64 on the device (NULL: all 0).
 * Outputs (device): trans [B, 3], rot [B, 9] row-major, status [B] int32 (0 ok; -1 refused: negative count here or before,
 * or counts exceed M; -2 sample_index out of range) — a pair whose status is not 0 gets zeros.
 * The *_embedding / *_encoder entries stop early for tests: x_out [B, S, 76] after the embedding / after layer 4, index_out
 * [B, S] int32 the chosen match per slot (-1: padding).  Workspace >= pope_pose_regressor_workspace_bytes(B, S), 256-byte
 * aligned.  Bad arguments (null pointers, S != weights->num_sample, G, B, workspace) return a negative code before any launch. */
size_t pope_pose_regressor_workspace_bytes(int B, int S);
int pope_pose_regressor_forward_f32(const pope_pose_regressor_weights* w, const float* dense0, const float* dense1,
                                    const float* kpts0, const float* kpts1, const int* counts, const int* sample_index,
                                    const unsigned long long* seeds, int B, int S, int G, long long M, float* trans, float* rot,
                                    int* status, void* workspace, size_t workspace_bytes, void* stream);
int pope_pose_regressor_embedding_f32(const float* dense0, const float* dense1, const float* kpts0, const float* kpts1,
                                      const int* counts, const int* sample_index, const unsigned long long* seeds, int B, int S,
                                      long long M, float* x_out, int* index_out, int* status, void* stream);
int pope_pose_regressor_encoder_f32(const pope_pose_regressor_weights* w, const float* dense0, const float* dense1,
                                    const float* kpts0, const float* kpts1, const int* counts, const int* sample_index,
                                    const unsigned long long* seeds, int B, int S, int G, long long M, float* x_out,
                                    int* index_out, int* status, void* stream);
/* The launches of the forward one by one (tests).  Each refuses null pointers and sizes <= 0 with POPE_ERR_ARG.
 * layer: one encoder layer in place on X [B, S, 76], groups as above (1 <= G <= 64, B % G == 0; weights 16-byte aligned).
 * stream_linear: Y [B, N] = leaky_relu(A [B, K] . W [N, K]^T + bias, 0.01); 16-byte loads when K % 4 == 0 and A and W are
 * 16-byte aligned, single floats otherwise; a row's summation order depends on K and on that route alone.
 * tail: mlp.6 .. 18, the heads and convert2matrix over Y2 [B, num_sample]: reads num_sample, mode, mlp_w / mlp_b [2 .. 6]
 * and the heads of w; a pair whose status is not 0 gets zeros. */
int pope_pose_regressor_layer_f32(const pope_pose_regressor_layer* w, float* X, int B, int S, int G, void* stream);
int pope_pose_regressor_stream_linear_f32(const float* A, const float* W, const float* bias, float* Y, int B, long long K, int N,
                                          void* stream);
int pope_pose_regressor_tail_f32(const pope_pose_regressor_weights* w, const float* Y2, const int* status, int B, float* trans,
                                 float* rot, void* stream);

/* ---- ConvNeXtV2 image backbone and the image pose head (pose/convnextv2/convnextv2.py, pose/model_cnn.py) -------- */

/* One Block: dwconv 7 x 7 (groups = C) -> LayerNorm(C, 1e-6) -> pwconv1 + GELU -> GRN(4C) -> pwconv2 -> + input.
 * dw_w is the depthwise weight [C, 1, 7, 7] RE-LAID [49, C] (tap-major, channel fastest); grn_gamma / grn_beta [4C];
 * pw1_w [4C, C], pw2_w [C, 4C] fp32 in nn.Linear's layout; pw1_wp / pw2_wp the same matrices as weight planes
 * (pope_split_planes_f32, scale POPE_PLANES_W_SCALE), read by POPE_PREC_F16X3 only and only where K % 32 == 0 (pw1_wp may be
 * NULL when C % 32 != 0, both may be NULL for POPE_PREC_F32_MFMA). */
typedef struct pope_convnext_block_weights {
    const float *dw_w, *dw_b, *norm_w, *norm_b;
    const float *pw1_w, *pw1_b, *grn_gamma, *grn_beta, *pw2_w, *pw2_b;
    const void *pw1_wp, *pw2_wp;
} pope_convnext_block_weights;

/* stem_w: Conv2d(3, C0, 4, 4) weight flattened [C0, 48] (columns (channel, kh, kw), its own memory order); ds_w[i]: the
 * downsample Conv2d(C_i, C_{i+1}, 2, 2) weight RE-LAID [C_{i+1}, (kh, kw, C_i)], ds_wp[i] its weight planes (POPE_PREC_F16X3);
 * ds_ln_*: the channels-first LayerNorm(C_i) in front of it.  blocks_host: HOST array of depths[0] + .. + depths[3] blocks in
 * stage order.  ones: max(dims) floats of 1.0f (the LayerScale slot of the residual epilogue).  dims[i] % 8 == 0.
 * head_w [num_classes, C3]; num_classes % 4 == 0 when logits are asked for. */
typedef struct pope_convnext_weights {
    int depths[4], dims[4];
    int num_classes;
    const float *stem_w, *stem_b, *stem_ln_w, *stem_ln_b;
    const float *ds_ln_w[3], *ds_ln_b[3], *ds_w[3], *ds_b[3];
    const void* ds_wp[3];
    const pope_convnext_block_weights* blocks_host;
    const float *norm_w, *norm_b, *head_w, *head_b, *ones;
} pope_convnext_weights;

/* ConvNeXtV2.forward_features / forward for image [B, 3, H, W] fp32 (H % 32 == 0, W % 32 == 0: the reference would silently
 * truncate other sizes; here they are POPE_ERR_ARG).  Activations are channels-last [B, h, w, C] fp32 between launches.
 * precision: POPE_PREC_F32_MFMA, or POPE_PREC_F16X3: every Linear / 2 x 2 convolution whose K is a multiple of 32 runs on
 * f16x3 planes (its operand written as planes by the producer in front of it: the block LayerNorm, the GRN apply step, the
 * downsample LayerNorm), the others (stem K = 48, C = 40 / 48 / 80 ..) on the fp32 MFMA; the head Linear splits its operands
 * in its K loop.  range_flag (device word, may be NULL) collects POPE_RANGE_LAYERNORM (LayerNorm producers), POPE_RANGE_GELU
 * (GRN apply) and POPE_RANGE_INPUT (head operands); the caller re-runs the call with POPE_PREC_F32_MFMA when it is set.
 * GRN statistics: a fixed-order column reduction per image (64-row chunks in row order, then the chunks in order), no
 * atomics — an image's result does not depend on the other images of the call.
 * features_out [B, C3] (the pooled, normalised features) and logits_out [B, num_classes] are each optional; taps: NULL or a
 * HOST array of 5 device pointers (each may be NULL): the stem output and the four stage outputs, channels-last
 * [B, H / 4 >> i, W / 4 >> i, dims[i]].  Workspace >= pope_convnext_workspace_bytes(w, B, H, W) (0: bad arguments), 256-byte
 * aligned.  Every bad argument — null pointers, sizes, an unknown precision, a short workspace — is POPE_ERR_ARG, returned
 * before the device is touched. */
size_t pope_convnext_workspace_bytes(const pope_convnext_weights* w, int B, int H, int W);
int pope_convnext_forward_f32(const pope_convnext_weights* w, const float* image, int B, int H, int W, int precision,
                              float* features_out, float* logits_out, float* const* taps, void* workspace,
                              size_t workspace_bytes, unsigned* range_flag, void* stream);
/* Depthwise Conv2d(C, C, 7, padding = 3, groups = C) + bias on channels-last x [B, H, W, C] -> y (y != x); w49 [49, C].
 * Any H, W >= 1 (maps smaller than the kernel included), C >= 1. */
int pope_convnext_dwconv_f32(const float* x, const float* w49, const float* bias, float* y, int B, int H, int W, int C,
                             void* stream);
/* GRN over x [B, HW, C] (C % 32 == 0): y = gamma * (x * Nx) + beta + x, Nx = Gx / (mean_c Gx + 1e-6), Gx = the L2 norm of a
 * column over the HW rows of its image.  Exactly one of y_f32 (may be x itself) and y_planes (activation planes [B HW, C],
 * POPE_RANGE_GELU into range_flag).  Workspace >= pope_convnext_grn_workspace_bytes(B, HW, C). */
size_t pope_convnext_grn_workspace_bytes(int B, int HW, int C);
int pope_convnext_grn_f32(const float* x, const float* gamma, const float* beta, int B, int HW, int C, float* y_f32,
                          void* y_planes, void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream);
/* The image pose head (pose/model_cnn.py:179-180): trans [B, 3] = translation_head_rot(feat), rot [B, 9] =
 * convert2matrix(rotation_head_rot(feat)) for feat [B, inner] (inner <= 256), mode POPE_ROT_*: the conversion code of the
 * key-point regressor. */
int pope_convnext_pose_heads_f32(const float* feat, const float* trans_w, const float* trans_b, const float* rot_w,
                                 const float* rot_b, int mode, int B, int inner, float* trans, float* rot, void* stream);

/* ---- MoCoPE fusion pose model (pose/model0604.py:MoCoPE) --------------------------------------------------------- */

/* One layer of nn.TransformerEncoder / nn.TransformerDecoder (post-norm, ReLU, 2048 hidden, nhead = 1, eps 1e-5) in torch's own
 * layouts (device pointers, fp32, 16-byte aligned): in_proj [3d, d] / [3d], out_proj [d, d] / [d], linear1 [2048, d] / [2048],
 * linear2 [d, 2048] / [d], norms [d].  The decoder layer's cross_* are its multihead_attn (q from the target rows, k | v from
 * the memory rows); its norm2 follows the cross-attention, norm3 the FFN. */
typedef struct pope_mocope_encoder_layer {
    const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b;
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} pope_mocope_encoder_layer;
typedef struct pope_mocope_decoder_layer {
    const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *cross_in_proj_w, *cross_in_proj_b, *cross_out_proj_w,
        *cross_out_proj_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b;
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *norm3_w, *norm3_b;
} pope_mocope_decoder_layer;
/* nn.Transformer(d_model, nhead = 1): 6 encoder layers + encoder.norm, 6 decoder layers + decoder.norm */
typedef struct pope_mocope_transformer {
    pope_mocope_encoder_layer enc[6];
    const float *enc_norm_w, *enc_norm_b;
    pope_mocope_decoder_layer dec[6];
    const float *dec_norm_w, *dec_norm_b;
} pope_mocope_transformer;
/* mode: POPE_ROT_*.  transformer_mkpts has d_model 76, mkpts_as_q / cnn_as_q 512.  mlp1_w[i] = mlp1.{0,3}: [38S, 76S],
 * [1024, 38S]; mlp_img: [512, 1000]; mlp2_w[i] = mlp2.{0,3,..,18}: [1024, 2048], [512, 1024], [256, 512], [128, 256], [64, 128],
 * [32, 64], [32, 32]; heads [3, 32] and [9 | 4 | 6, 32].  The pointers are read on every call: no derived copy exists. */
typedef struct pope_mocope_weights {
    int num_sample, mode;
    pope_mocope_transformer transformer_mkpts, mkpts_as_q, cnn_as_q;
    const float* mlp1_w[2];
    const float* mlp1_b[2];
    const float *mlp_img_w, *mlp_img_b;
    const float* mlp2_w[7];
    const float* mlp2_b[7];
    const float *trans_w, *trans_b, *rot_w, *rot_b;
} pope_mocope_weights;

/* train_type of MoCoPE: the full fusion, or the reference's own reduced routes (mkpts_as_q(x_mkpts, x_mkpts) / cnn_as_q(x_img,
 * x_img), each concatenated with itself) */
#define POPE_MOCOPE_FUSION 0
#define POPE_MOCOPE_MKPTS 1
#define POPE_MOCOPE_CNN 2
/* stages pope_mocope_tap_f32 stops after; tap_out is [B, S, 76] for the first three, [B, 2, 512] for the others */
#define POPE_MOCOPE_TAP_EMBEDDING 0   /* Embedding(2, 9, logscale=False) of cat(mkpts0, mkpts1) */
#define POPE_MOCOPE_TAP_MEMORY 1      /* transformer_mkpts: the encoder output after encoder.norm */
#define POPE_MOCOPE_TAP_MKPTS_T 2     /* transformer_mkpts(x, x) */
#define POPE_MOCOPE_TAP_X_MKPTS 3     /* mlp1 output */
#define POPE_MOCOPE_TAP_X_IMG 4       /* stacked mlp_img outputs */
#define POPE_MOCOPE_TAP_QMKPTS 5      /* mkpts_as_q output */
#define POPE_MOCOPE_TAP_QIMG 6        /* cnn_as_q output */

/* MoCoPE.forward (pose/model0604.py:248-300) after the backbone, fp32 throughout, for B pairs of S = num_sample sample slots.
 * Key-point input, sampling, padding, seeds, status codes and the group size G are those of pope_pose_regressor_forward_f32:
 * the B pairs form B / G attention groups of G consecutive pairs (1 <= G <= 64, B % G == 0) — torch reads [B, S, 76] and
 * [B, 2, 512] with batch_first=False, so all three transformers attend ACROSS the pairs of a call (G = B); G = 1 is every pair
 * on its own.  feat0 / feat1 [B, 1000]: the backbone's logits of the two images (not read by POPE_MOCOPE_MKPTS; the key points
 * still give the status of a pair under POPE_MOCOPE_CNN).
 * Launch sequence: select, embed | per transformer layer: in_proj (q | k | v of one streamed Linear, or v alone for G = 1),
 * attention over the group, out_proj, residual + LayerNorm, (decoder: the same again against the memory rows), then the FFN: at
 * d = 76 one launch on the fp32 MFMA (linear1 + ReLU + linear2 + residual + LayerNorm, hidden activation in registers), at d = 512
 * linear1 + ReLU, linear2, residual + LayerNorm (the closing encoder.norm / decoder.norm ride the last layer's launch) | streamed Linears +
 * LeakyReLU for mlp1, mlp_img, mlp2.0, mlp2.3 | one tail launch per call for mlp2.6 .. 18, the heads and convert2matrix.
 * Every Linear output element is a lane-strided sum over K (lane l takes the 16-byte groups l, l + 64, ..) followed by a xor
 * butterfly: its order depends on K alone, not on B, G, the row or the CU.  Plain launches only.
 * Outputs (device): trans [B, 3], rot [B, 9] row-major, status [B] int32; a pair whose status is not 0 gets zeros.
 * Workspace >= pope_mocope_workspace_bytes(B, S), 256-byte aligned.  Bad arguments (null pointers, S != weights->num_sample, B,
 * G, train_type, stage, workspace) return a negative code before any HIP call. */
size_t pope_mocope_workspace_bytes(int B, int S);
int pope_mocope_forward_f32(const pope_mocope_weights* w, const float* dense0, const float* dense1, const float* kpts0,
                            const float* kpts1, const int* counts, const int* sample_index, const unsigned long long* seeds,
                            const float* feat0, const float* feat1, int B, int S, int G, long long M, int train_type,
                            float* trans, float* rot, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* The same call stopped after `stage` (POPE_MOCOPE_TAP_*, tests): tap_out receives that stage's tensor; a stage the
 * train_type does not compute is POPE_ERR_ARG. */
int pope_mocope_tap_f32(const pope_mocope_weights* w, const float* dense0, const float* dense1, const float* kpts0,
                        const float* kpts1, const int* counts, const int* sample_index, const unsigned long long* seeds,
                        const float* feat0, const float* feat1, int B, int S, int G, long long M, int train_type, int stage,
                        float* tap_out, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* The launches of the transformers one by one (tests).  Each refuses null pointers and sizes <= 0 with POPE_ERR_ARG.
 * linear: Y [R, N] = act(A [R, K] . W [N, K]^T + bias), act 0 (none) or 1 (ReLU); K % 4 == 0, A and W 16-byte aligned.
 * attention: rows r = b * S + s; row r attends over the G rows (b / G * G + g) * S + s, g < G, softmax(q . k / sqrt(d)) v, one
 * head; q / k / v rows at pitches ldq / ldk / ldv >= d floats, O [R, d] dense.  d is 76 or 512, 1 <= G <= 64, R % (S G) == 0.
 * add_ln: X [R, d] = LayerNorm(X + Y; w1, b1), then LayerNorm(.; w2, b2) when w2 / b2 are given (both or neither); eps 1e-5.
 * ffn76: X [R, 76] = LayerNorm(X + linear2(relu(linear1(X))); nw, nb), then LayerNorm(.; fw, fb) when given; linear1
 * [2048, 76], linear2 [76, 2048], 16-byte aligned. */
int pope_mocope_linear_f32(const float* A, const float* W, const float* bias, float* Y, int R, int K, int N, int act, void* stream);
int pope_mocope_attention_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int R, int S, int G,
                              int d, void* stream);
int pope_mocope_add_ln_f32(float* X, const float* Y, const float* w1, const float* b1, const float* w2, const float* b2, int R, int d,
                           void* stream);
int pope_mocope_ffn76_f32(float* X, const float* l1w, const float* l1b, const float* l2w, const float* l2b, const float* nw,
                          const float* nb, const float* fw, const float* fb, int R, void* stream);

/* ---- Vision Mamba backbone (pose/vim/models_mamba.py:VisionMamba; mixer after the Mamba and Vim papers) -------- */

/* One direction of a bidirectional ("v2") mixer, device pointers, fp32: conv_w [E, 4] (Conv1d(E, E, 4, groups = E) weight
 * [E, 1, 4] as it lies), conv_b [E], x_proj_w [R + 32, E] (rows dt | B | C), dt_w [E, R], dt_b [E], A_log [E, 16], D [E]. */
typedef struct pope_vim_dir_weights {
    const float *conv_w, *conv_b, *x_proj_w, *dt_w, *dt_b, *A_log, *D;
} pope_vim_dir_weights;

/* One Block: norm_w [D] (RMSNorm, no bias), in_proj_w [2E, D], out_proj_w [D, E] (nn.Linear layout, no bias); in_proj_wp /
 * out_proj_wp the same matrices as weight planes (POPE_PREC_F16X3 only); dir[0] the forward, dir[1] the backward (`_b`) set. */
typedef struct pope_vim_layer_weights {
    const float *norm_w, *in_proj_w, *out_proj_w;
    const void *in_proj_wp, *out_proj_wp;
    pope_vim_dir_weights dir[2];
} pope_vim_layer_weights;

/* img: side of the square image (a multiple of 8); patch 16; stride 8 or 16; dim D (a multiple of 64, <= 512); E = 2 D,
 * d_state 16, d_conv 4, dt_rank R = ceil(D / 16).  patch_w [D, 768] (the Conv2d weight as it lies), patch_wp its weight planes
 * (POPE_PREC_F16X3), patch_b [D], cls [D], pos [L, D] with L = g g + 1, g = (img - 16) / stride + 1: the class token sits at
 * row (g g) / 2.  layers_host: HOST array of `depth` layers.  norm_f_w [D]; head_w [num_classes, D], head_b: read when logits
 * are asked for (num_classes % 4 == 0). */
typedef struct pope_vim_weights {
    int img, stride, dim, depth, num_classes;
    float eps;
    const float *patch_w, *patch_b, *cls, *pos;
    const void* patch_wp;
    const pope_vim_layer_weights* layers_host;
    const float *norm_f_w, *head_w, *head_b;
} pope_vim_weights;

/* VisionMamba.forward_features / forward (eval mode) for image [B, 3, img, img] fp32.  precision POPE_PREC_F32_MFMA, or
 * POPE_PREC_F16X3: patch embedding, in_proj and out_proj on f16x3 planes (operands written as planes by the gather, the
 * add + RMSNorm and the scan), x_proj and the head split their fp32 operands in the K loop where the shape allows it and run
 * on the fp32 MFMA where not; conv1d, dt_proj, the scan and the norms are fp32 in both.  range_flag (device word, may be NULL)
 * collects POPE_RANGE_PATCH, POPE_RANGE_LAYERNORM (norm output), POPE_RANGE_GELU (scan output) and POPE_RANGE_INPUT; the
 * caller re-runs with POPE_PREC_F32_MFMA when it is set.  Nothing in the call depends on B: an image's result is the same
 * bits alone or in a batch.  features [B, D] and logits [B, num_classes] are each optional; taps: NULL or a HOST array of 4
 * device pointers (each may be NULL), [B, L, D] each: the token matrix, and hidden + residual after layers 0,
 * depth / 2 - 1 and depth - 1.  Workspace >= pope_vim_workspace_bytes(w, B) (0: bad arguments), 256-byte aligned.  Every bad
 * argument is POPE_ERR_ARG (a short workspace POPE_ERR_WORKSPACE), returned before the device is touched. */
size_t pope_vim_workspace_bytes(const pope_vim_weights* w, int B);
int pope_vim_forward_f32(const pope_vim_weights* w, const float* image, int B, int precision, void* workspace,
                         size_t workspace_bytes, float* features, float* logits, float* const* taps, unsigned* range_flag,
                         void* stream);
/* The launches one by one (tests).  Null pointers and sizes <= 0 are POPE_ERR_ARG, a short workspace POPE_ERR_WORKSPACE.
 * scan: both directions of one layer.  xc [2, B L, E] (the conv1d outputs of the two directions), z [B L] rows of pitch ldz,
 * xdbl [2, B L, R + 32] (x_proj outputs), dirs: HOST array of 2 (dt_w, dt_b, A_log, D are read); exactly one of out_f32
 * [B L, E] and out_planes (activation planes, POPE_RANGE_GELU): (o_fwd + o_bwd) / 2.  E % 16 == 0, R % 4 == 0, R <= 32.
 * The sequence is cut into chunks of pope_vim_scan_chunk() steps whose states are carried in chunk order. */
int pope_vim_scan_chunk(void);
size_t pope_vim_scan_workspace_bytes(int B, int L, int E);
int pope_vim_scan_f32(const float* xc, const float* z, int ldz, const float* xdbl, const pope_vim_dir_weights* dirs, int B, int L,
                      int E, int R, float* out_f32, void* out_planes, void* workspace, size_t workspace_bytes,
                      unsigned* range_flag, void* stream);
/* xc [2, B L, E]: xc[0] = silu(causal conv1d of x; dirs[0]), xc[1] = silu(anti-causal conv1d; dirs[1]): the backward
 * direction's convolution in un-reversed time.  x [B L] rows of pitch ldx (the first E columns of xz).  Any L >= 1. */
int pope_vim_conv1d_silu_f32(const float* x, int ldx, const pope_vim_dir_weights* dirs, int B, int L, int E, float* xc,
                             void* stream);
/* r = hidden [+ res_in]; res_out = r (optional); y = r * rsqrt(mean(r^2) + eps) * w as fp32 rows or activation planes (exactly
 * one; planes: D % 32 == 0, POPE_RANGE_LAYERNORM).  Input row i is row i * row_stride + row_offset of hidden / res_in /
 * res_out, output row i is row i of y.  D % 4 == 0, D <= 2048. */
int pope_vim_add_rmsnorm_f32(const float* hidden, const float* res_in, float* res_out, const float* w, float* y_f32,
                             void* y_planes, long long rows, int D, float eps, long long row_stride, long long row_offset,
                             unsigned* range_flag, void* stream);

/* ---- host-side helper ------------------------------------------------------------------------ */

/* Streaming top-3 proposal vote — eval_linemod_json.py:71,95-101 (HOST pointers): slots start at
 * 0; a proposal enters iff score > min(slots), replacing the first minimal slot. */
int pope_streaming_top3_host(const float* scores_host, int P, float* slot_scores_host,
                             long long* slot_index_host);

#ifdef __cplusplus
}
#endif
#endif /* POPE_HIP_H */
