// Internal launcher interface between the kernel translation units and the C ABI (capi.hip, vit_forward.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>
#include <utility>
#include "../../include/pope_hip.h"  // POPE_RANGE_* bits of the f16x3 range-guard word

enum GemmEpilogue {
    EPI_BIAS = 0,         // C = A.W^T + bias
    EPI_BIAS_GELU = 1,    // C = gelu_erf(A.W^T + bias)
    EPI_BIAS_LS_RES = 2,  // C = res + gamma * (A.W^T + bias)      (LayerScale + residual)
    EPI_POSB = 3,         // patch embed: C = im2col(img).W^T + posb[token]   (A = image)
    EPI_BIAS_RELU = 5,    // C = max(A.W^T + bias, 0)                (LoFTR encoder MLP, transformer.py:24-28; gemm_planes.hip only)
    EPI_SIM = 4,          // batched similarity (planes kernel): C[b] = (A[b].W[b]^T * alpha) / divisor, no bias
    EPI_SIM_MASK = 10,    // kernel-side instantiation of EPI_SIM with GemmParams::sim_mask0 / sim_mask1 (callers pass EPI_SIM)
    EPI_SAM_QKV = 7,      // SAM block's QKV projection written straight into the attention operand planes (sam_attention.hip; gemm_planes.hip only)
    EPI_QKV_F16 = 8,      // plain f16 only (POPE_PREC_F16 ViT blocks): C = (A.W^T + bias) * (col < sam_dim ? sam_qscale : 1) -> f16 row-major
                          // [M, N] with NO activation scale: the operand of attention_f16.hip (q carries head_dim^-0.5 * log2 e before its ONE rounding)
    EPI_CONV_UP = 9,      // kernel-side instantiation of EPI_CONV with GemmParams::up_src (callers pass EPI_CONV)
    EPI_BIAS_SWIGLU = 11, // C[M, N / 2] = silu(gate + b_gate) * (value + b_value), the w12 GEMM of the SwiGLU FFN (swiglu_ffn.py:29-33) with
                          // the rows of W / bias PERMUTED (pope_hip.h POPE_EPI_BIAS_SWIGLU): output columns 64 t .. 64 t + 31 are the
                          // gates of hidden columns 32 t .. 32 t + 31, columns 64 t + 32 .. 64 t + 63 their values; N = 2 hidden is a
                          // multiple of 64, ldc is the pitch of the HIDDEN rows; planes -> planes / fp32 and the fp32 GEMM
    EPI_CONV = 6,         // C = act(A.W^T + bias [+ res_pl]), act(v) = max(v, 0) + act_slope * min(v, 0): ReLU (0), LeakyReLU
                          // (0.01) or identity (1); the ResNet-FPN convolutions (conv.hip; gemm_planes.hip only)
};

struct GemmParams {
    const float* A;     // [M, lda] row-major activations (EPI_POSB: image [B,3,H,W])
    const float* W;     // [N, ldw] row-major weights (torch Linear layout, out x in)
    const float* bias;  // [N] or null
    float* C;           // [M, ldc]
    int lda, ldw, ldc;
    int M, N, K;
    int epilogue;
    const float* gamma;  // [N]      (EPI_BIAS_LS_RES)
    const float* res;    // [M,ldres](EPI_BIAS_LS_RES; may alias C)
    int ldres;
    // EPI_SIM: nbatch problems of [rows_a x rows_w x K]; A planes [nbatch*rows_a, lda], W planes [nbatch*rows_w, ldw],
    // C [nbatch, rows_a, rows_w] fp32 (ldc = rows_w); M = rows_a, N = rows_w
    int nbatch;
    float alpha, divisor;
    // EPI_SIM fused softmax statistics (dense matcher, match.hip): every wave writes, for its 64-column block, the
    // (max, sum exp(. - max)) of each of its rows, and for each of its two 32-row blocks the same per column:
    //   row_part  [nbatch][M][ncb]      float2, ncb = 2 * ceil(N / 128)
    //   col_pmax / col_psum [nbatch][nrb][ldp] floats, nrb = 4 * ceil(M / 128), ldp = N rounded up to 4
    // divisor_eff = divisor / alpha and rdiv = 1 / divisor_eff (host, correctly rounded): sim = acc / divisor_eff
    float* row_part;
    float* col_pmax;
    float* col_psum;
    int ncb, nrb, ldp;
    float divisor_eff, rdiv;
    int res_mod;         // > 0: the residual row is (row % res_mod) of a [res_mod, ldres] table (patch embed: pos + bias)
    // f16x3 "planes" operands (gemm_planes.hip): a tensor X[rows, ld] kept as two f16
    // planes with X = (hi + lo) / scale (power-of-two scale: activations 8, weights 256).  The planes
    // kernel needs a_pl and w_pl; when c_pl is set its epilogue writes planes (scale 8) instead of fp32 C.
    // Layout of a planes tensor [rows, ld]: row-major, 2*ld halves per row, per 32-column chunk the
    // 32 hi halves then the 32 lo halves (128 contiguous bytes = one cache line per row and K-step):
    //   offset(row, col, plane) = row*2*ld + pope_planes_col(col) + plane*32   (common.h, with the producers' pope_planes_store).
    const void* a_pl;
    const void* w_pl;
    void* c_pl;
    // f16x3 range guard: a planes-writing epilogue ORs range_bit into *range_flag (may be null) when a value does
    // not fit f16 after scaling; the on-the-fly f16x3 kernel checks its operands before the split
    unsigned* range_flag;
    unsigned range_bit;
    // fused following LayerNorm (gemm_rowln.hip, N = 384): x = res + gamma * (A.W^T + bias) -> C, and
    // LayerNorm(x) * ln_w + ln_b -> ln_planes (activation planes) or ln_f32 (exactly one of the two)
    const float* ln_w; const float* ln_b;
    float ln_eps;
    void* ln_planes;
    float* ln_f32;
    int rl_prefetch;     // gemm_rowln.hip: touch the tile's residual lines during its K loop (set by the launcher)
    // EPI_CONV (gemm_planes.hip): optional residual as activation planes [M, ldres_pl] (BasicBlock shortcut), activation
    // slope, and — conv_cch > 0 — the implicit 3x3 stride-1 convolution over a zero-bordered NHWC planes tensor
    // [n, Hp, Wp = conv_wp, 32 * conv_cch channels]: output row R = pixel R + Wp + 1, and the A row of K-step
    // (tap (dy, dx), chunk c) is row R + dy * Wp + dx, chunk c — a row-uniform shift, i.e. a scalar offset per K-step
    // (K = 9 * 32 * conv_cch; W rows hold the taps in (dy, dx, channel) order); a_pl may be read up to 2 Wp + 2 rows
    // past M (the caller's buffer has them, or the range check returns zeros)
    const void* res_pl;
    int ldres_pl;
    float act_slope;
    int conv_cch, conv_wp;
    // gemm_plain.hip CONV = 2 (conv_s2_taps > 0): stride-2 convolution read straight from the zero-bordered INPUT tensor
    // [n, conv_s2_hpi, conv_wp, 32 * conv_cch] (conv_s2_in_rows pixel rows) for the output grid [n, conv_s2_hpo, conv_s2_wpo];
    // conv_s2_taps = 9 (3 x 3, pad 1) or 1 (the 1 x 1 shortcut)
    int conv_s2_taps, conv_s2_hpi, conv_s2_hpo, conv_s2_wpo, conv_s2_in_rows;
    // EPI_CONV with up_src (gemm_planes.hip; round 4): the FPN merge of resnet_fpn.py:109-115 in the lateral 1 x 1 convolution's
    // epilogue — output row R is pixel R of this level's zero-bordered grid [up_n, up_hp, up_wp]; the bilinear x2
    // (align_corners) sample of the half-resolution fp32 map up_src [up_n, (up_hp - 2) / 2 + 2, (up_wp - 2) / 2 + 2, up_lds] at
    // that pixel is added before the activation.  The arithmetic of conv.hip's upsample_add_f32_kernel (the fp32 mode's two-step
    // form), term for term, without the fp32 round trip of the lateral map.  Not together with res_pl; up_wp >= 4.
    const float* up_src;
    int up_lds, up_hp, up_wp, up_n;
    float up_sh, up_sw;          // bilinear scales (Hs - 1) / (H - 1), (Ws - 1) / (W - 1) (0 for a single output row / column)
    unsigned up_m_hw, up_m_w;    // floor(2^32 / (up_hp * up_wp)), floor(2^32 / up_wp)
    // plain != 0 (gemm_planes.hip only): single-product f16 arithmetic.  a_pl / w_pl (and c_pl) are f16 ROW-MAJOR tensors
    // (value * scale); K, lda, ldw and a planes output's ldc are given in 64-bit column PAIRS (= real columns / 2, so
    // that a row's pitch is still ld * 4 bytes); N, ldc of an fp32 output, bias, gamma and res stay in real columns.
    int plain;
    // EPI_SAM_QKV: C[t, which * dim + head * hd + c] (+ bias, q additionally * sam_qscale) goes to row
    // sam_rowmap[t] + head * sam_npad, column c of sam_q / sam_k / sam_v (f16 hi/lo rows [DQ | DQ], [DQ | hd], [DV | DV];
    // plain: the hi parts only) — the window partition of image_encoder.py:238-259 is that row map
    void *sam_q, *sam_k, *sam_v;
    unsigned sam_bytes[3];
    const int* sam_rowmap;
    int sam_hd, sam_dim, sam_npad, sam_dq, sam_dv;
    float sam_qscale;
    // patch-embed gather (EPI_POSB)
    const float* posb;   // [ntok, N]: row 0 = cls_token + pos[0]; row n = conv bias + pos[n]
    int ntok, img_h, img_w, patch, grid_w;
    // EPI_SIM padding masks (coarse_matching.py:115-118), 0 / 1 fp32, each optional: sim_mask0 [nbatch, M], sim_mask1 [nbatch, N];
    // sim = -1e9 where sim_mask0[b][row] * sim_mask1[b][col] == 0 (a missing mask counts as ones)
    const float* sim_mask0;
    const float* sim_mask1;
};

int pope_launch_gemm_nt_f32(const GemmParams& g, hipStream_t stream);

// Same contract on the f16 matrix cores with error-compensated operands (gemm_f16x3.hip).
bool pope_gemm_f16x3_supported(const GemmParams& g);
// Every GEMM on pre-split f16x3 planes or (GemmParams::plain) plain f16 operands: Linears (BIAS, BIAS_GELU, BIAS_RELU,
// BIAS_SWIGLU, BIAS_LS_RES, QKV_F16, SAM_QKV), the batched similarity (SIM) and the convolutions (CONV: implicit 3 x 3, up_src, and —
// conv_s2_taps > 0 — the stride-2 implicit form).  Checks the arguments and picks the mainloop (gemm_planes.hip).
int pope_launch_gemm_planes(const GemmParams& g, hipStream_t stream);
// whether pope_launch_gemm_planes takes a stride-2 convolution without the gathered tap tensor (conv.hip gathers otherwise)
bool pope_wide_conv_s2_supported(const GemmParams& g);
// residual GEMM + the following LayerNorm in one kernel (gemm_rowln.hip; N = 384 only: `supported` says)
bool pope_gemm_rowln_supported(const GemmParams& g);
// the whole argument contract of pope_launch_gemm_rowln (host only: no HIP call)
bool pope_gemm_rowln_args_ok(const GemmParams& g);
int pope_launch_gemm_rowln(const GemmParams& g, hipStream_t stream);
constexpr float K_PLANES_ACT_SCALE = 8.0f, K_PLANES_W_SCALE = 256.0f;  // == POPE_PLANES_*_SCALE of pope_hip.h

// The row widths the wave-per-row LayerNorm kernels are instantiated for, in units of 128 columns (5, 10: the SAM ViT-H width
// 1280 and its test twin 640).  pope_ln_dispatch calls f(std::integral_constant<int, NV>) for dim == 128 NV and returns
// false, without a call, for every other dim; pope_ln_width_ok asks the same list without a call.
template <typename F, int... NV>
inline bool pope_ln_dispatch(int dim, F&& f, std::integer_sequence<int, NV...>) {
    return ((dim == 128 * NV && (f(std::integral_constant<int, NV>{}), true)) || ...);
}
template <typename F>
inline bool pope_ln_dispatch(int dim, F&& f) {
    return pope_ln_dispatch(dim, f, std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 8, 10, 12, 16>{});
}
inline bool pope_ln_width_ok(int dim) { return pope_ln_dispatch(dim, [](auto) {}); }

// y = LayerNorm(x) written as f16 planes (scale POPE_PLANES_ACT_SCALE), [rows, dim] halves each.
int pope_launch_layernorm_planes(const float* x, int ldx, const float* w, const float* b, void* y_pl,
                                 int rows, int dim, float eps, unsigned* range_flag, hipStream_t stream);
// LayerNorm(384) in the exact arithmetic of gemm_rowln.hip's fused epilogue (bit-identical results): the small-batch twin
int pope_launch_layernorm_rowln_order(const float* x, const float* w, const float* b, void* y_planes, float* y_f32, int rows, float eps,
                                      unsigned* flag, hipStream_t stream);
// Generic fp32 [rows, ld] -> planes converter (ld % 32 == 0).
// patch embed, f16x3: image [B,3,H,W] -> A planes [B*ntok, kp] (kp = 3*patch^2 rounded up to 32; row b*ntok is the
// all-zero CLS row, row b*ntok + 1 + n the flattened patch n; zero K padding)
int pope_launch_im2col_planes(const float* img, void* a_planes, int B, int H, int W, int patch, int kp, unsigned* range_flag,
                              hipStream_t stream);
// the whole patch embed (vit_forward.hip), tokens [B * ntok, dim] fp32: the arguments of pope_patch_embed_f32 / _planes_f32
int pope_launch_patch_embed_f32(const float* img, const float* proj_w, const float* posb, float* tokens, int B, int H, int W,
                                int patch, int dim, hipStream_t stream);
int pope_launch_patch_embed_planes(const float* img, const void* proj_w_planes, const float* posb, float* tokens, int B, int H, int W,
                                   int patch, int dim, void* a_planes_scratch, size_t scratch_bytes, unsigned* range_flag,
                                   hipStream_t stream);
// matcher operand: planes of feat / divisor (a true fp32 division, coarse_matching.py:109) for n blocks of `rows` rows
// with `bs` elements between blocks; output compact [n*rows, cols]
int pope_launch_div_planes(const float* src, long long bs, void* planes, int n, int rows, int cols, float divisor, float scale,
                           unsigned* range_flag, hipStream_t stream);
int pope_launch_split_planes(const float* src, void* pl, int rows, int ld, float scale, unsigned* range_flag, hipStream_t stream);
// HBM-bound scan: ORs `bit` into *flag when any |x[i]| * scale >= 65520 or x[i] is not finite (operand check of the
// op-level f16x3 entry points, which split fp32 operands inside their K loops)
int pope_launch_range_check(const float* x, size_t n, float scale, unsigned* flag, unsigned bit, hipStream_t stream);
int pope_launch_gemm_nt_f16x3(const GemmParams& g, hipStream_t stream);

// y[r,:] = LayerNorm(x[r,:]) * w + b over `dim` (multiple of 128, <= 2048), eps inside the sqrt.
int pope_launch_layernorm_f32(const float* x, int ldx, const float* w, const float* b, float* y, int ldy,
                              int rows, int dim, float eps, hipStream_t stream);

// POPE_PREC_F16 pieces of the DINOv2 and SAM paths (layernorm.hip, attention_f16.hip): LayerNorm -> f16 row-major (value * 8), the
// plain conversion fp32 -> f16 (value * 8) of n4 quads; attention on the f16 operands of the QKV epilogue, f16 row-major output (value * 8)
int pope_launch_layernorm_f16(const float* x, const float* w, const float* b, void* y_f16, int rows, int dim, float eps, unsigned* flag,
                              hipStream_t stream);
int pope_launch_to_f16(const float* x, void* y_f16, long long n4, unsigned* flag, hipStream_t stream);
// round 4: f16 qkv in (EPI_QKV_F16), LDS-direct K / V staging, four stages, software-pipelined (attention_f16.hip)
int pope_launch_attention_f16_dma(const void* qkv_f16, void* out_f16, int B, int N, int heads, hipStream_t stream);
// Multi-head softmax attention over qkv[B, N, 3, heads, 64] -> out[B, N, heads*64].
int pope_launch_attention_f32(const float* qkv, float* out, int B, int N, int heads, hipStream_t stream);
int pope_launch_attention_f16x3(const float* qkv, float* out, int B, int N, int heads, hipStream_t stream);
// qkv given as planes (the QKV GEMM epilogue's output), output planes: the whole-model f16x3 dataflow
int pope_launch_attention_f16x3_planes_io_diag(const void* qkv_planes, void* out_planes, int B, int N, int heads, long long* exact_passes_host,
                                               hipStream_t stream);   // diagnostic twin: counts exact passes, synchronises
int pope_launch_attention_f16x3_planes_io(const void* qkv_planes, void* out_planes, int B, int N, int heads, hipStream_t stream);

struct MatchParams {
    const float* feat0;  // [n, L, C]
    const float* feat1;  // [n, S, C]
    int n, L, S, C;
    long long bs0, bs1;  // elements between consecutive pairs in feat0 / feat1 (>= L*C, S*C)
    int h0, w0, h1, w1;  // coarse grids (L = h0*w0, S = h1*w1)
    float thr, temperature;
    int border;
    float scale;         // hw0_i[0] / hw0_c[0]
    float* sim;          // [n, L, S]: sim; conf in place when publish_conf (then it is the caller's conf_matrix)
    int publish_conf;
    void* planes0; void* planes1;  // optional scratch [n*L*C] / [n*S*C] floats-worth: similarity on the f16 matrix cores
    // pieces of the softmax statistics written by the f16x3 contraction's epilogue (GemmParams: row_part, col_pmax, col_psum)
    float* row_part; float* col_pmax; float* col_psum;
    int ncb, nrb, ldp;               // 2 * ceil(S/128), 4 * ceil(L/128), S rounded up to 4
    float* row_max; float* row_sum;  // [n, L]   softmax(sim, dim=2) statistics
    float* col_max; float* col_sum;  // [n, S]   softmax(sim, dim=1) statistics
    float* colmax_part;              // [n, nrb2, ldp] column maxima of conf per 32-row block
    int nrb2;                        // pope_match_nrb2(L)
    float* conf_colmax;              // [n, S]
    float* conf_rowmax;              // [n, L]
    int* row_arg; int* row_cnt;      // [n, L]  first argmax column of conf, number of columns attaining the maximum
    int* row_j;                      // [n, L]  matched column or -1
    float* row_conf;                 // [n, L]
    unsigned* range_flag;            // optional f16x3 range-guard word (POPE_RANGE_MATCH)
    int* counts;                     // [n + 1] per-pair match counts, then total
    // compacted outputs (capacity n * L)
    long long* b_ids; long long* i_ids; long long* j_ids;
    float* mconf; float* mkpts0; float* mkpts1;
    // padding masks and rescaling (all optional, 0 / 1 fp32 masks): fill0 [n, L] / fill1 [n, S] set sim = -1e9 where
    // fill0[i] * fill1[j] == 0 (coarse_matching.py:115-118); border0 [n, h0, w0] / border1 [n, h1, w1] move the bottom and
    // right border to the valid extent of each pair (mask_border_with_padding, :28-43), extent [n, 4] ints of scratch
    // (h0, w0, h1, w1 valid); scale0 / scale1 [n, 2] (x, y) factors of mkpts0_c / mkpts1_c (:242-250)
    const float* fill0; const float* fill1;
    const float* border0; const float* border1;
    int* extent;
    const float* scale0; const float* scale1;
    // Sinkhorn matcher only (match_type='sinkhorn', sinkhorn.hip): the dustbin score is read on the device, from the
    // parameter's own storage; u [n, L + 1] / v [n, S + 1] the dual potentials (last entry: the dustbin), skh_cmax [n, S] the
    // column maxima of Z + u over the real rows after the last column step (the column prefilter's left-hand side)
    const float* bin_score;
    int skh_iters, skh_prefilter;
    float* skh_u; float* skh_v; float* skh_cmax;
    float skh_norm, skh_log_mu_bin, skh_log_nu_bin;   // -log(L + S), log(S) + norm, log(L) + norm (fp32, set by the launcher)
};
int pope_match_nrb2(int L);
int pope_match_params_check(const MatchParams& p);   // host only (no HIP call); both launchers run it first
int pope_launch_dense_match_f32(const MatchParams& p, hipStream_t stream);
// match_type='sinkhorn': same contraction (temperature 1), then the passes of sinkhorn.hip in place of the dual softmax, then
// the same selection / compaction kernels.  The matrix always ends up holding conf (in the workspace when not published).
int pope_launch_dense_match_sinkhorn_f32(MatchParams p, hipStream_t stream);
// sinkhorn.hip: p.sim holds Z's L x S block and p.row_max / p.row_sum its row softmax statistics; runs the iterations and the
// confidence pass (conf in place; conf_rowmax / row_arg / row_cnt / colmax_part as conf_pass_kernel of match.hip leaves them)
int pope_launch_sinkhorn_passes(const MatchParams& p, hipStream_t stream);

#ifdef __HIPCC__
struct RowBest {   // running (max, first argmax, number of argmax ties) of a row
    float v;
    int idx, cnt;
    __device__ __forceinline__ void take(float c, int col) {
        const bool gt = c > v, eq = c == v;
        cnt = gt ? 1 : cnt + (eq ? 1 : 0);
        idx = gt ? col : idx;   // columns arrive in ascending order per lane: a tie keeps the earlier column
        v = gt ? c : v;
    }
    __device__ __forceinline__ void merge(float ov, int oidx, int ocnt) {
        const bool gt = ov > v, eq = ov == v;
        cnt = gt ? ocnt : cnt + (eq ? ocnt : 0);
        idx = gt ? oidx : (eq && oidx < idx ? oidx : idx);
        v = gt ? ov : v;
    }
};
#endif

// Batched PIL-exact preprocessing (preprocess.hip): resize (window / fixed-point weight tables from the host) ->
// centre crop -> /255 -> normalise, uint8 HWC [P, Hin, Win, 3] -> fp32 NCHW [P, 3, ch, cw]
struct PreprocParams {
    const unsigned char* img;
    int P, Hin, Win;
    const int *hstart, *hcount, *hk; int kh;   // horizontal tables, indexed by OUTPUT column of the full resized image
    const int *vstart, *vcount, *vk; int kv;   // vertical tables, indexed by output row
    int top, left, ch, cw;                     // crop window in the resized image
    int row0, nrows;                           // input rows the cropped output rows read: [row0, row0 + nrows)
    float mean[3], std[3];
    unsigned char* tmp;                        // [P, nrows, cw, 3]
    float* out;
};
int pope_launch_preprocess(const PreprocParams& p, hipStream_t stream);
// The same resample of whole frames (preprocess.hip), SAM's input transform: uint8 HWC [P, Hin, Win, 3] -> the resized uint8
// HWC [P, OH, OW, 3] (f32 = false), or -> fp32 NCHW [P, 3, S, S] with (v - mean) / std inside OH x OW and zeros elsewhere
struct ResizeParams {
    const unsigned char* img;
    int P, Hin, Win;
    const int *hstart, *hcount, *hk; int kh;   // horizontal tables [OW], [OW], [OW, kh]
    const int *vstart, *vcount, *vk; int kv;   // vertical tables [OH], [OH], [OH, kv]
    int OH, OW;
    bool f32;
    int S, flip;                               // f32: side of the padded square; channel c reads source channel 2 - c
    float mean[3], std[3];                     // f32: per OUTPUT channel, on the 0..255 scale
    void* out;
    unsigned char* tmp; size_t tmp_bytes;      // [P, Hin, OW, 3]
};
int pope_resize_check(const ResizeParams& p);   // no HIP call
int pope_launch_resize(const ResizeParams& p, hipStream_t stream);
int pope_launch_gray(const unsigned char* bgr, size_t npix, float* out, hipStream_t stream);
int pope_launch_crop_warp(const unsigned char* img, int H, int W, int C, const double* minv, const int* win, int P, int oh, int ow,
                          unsigned char* out, hipStream_t stream);
int pope_launch_crop_norm(const unsigned char* img, int P, int Hin, int Win, int top, int left, int ch, int cw, const float* mean,
                          const float* std, float* out, hipStream_t stream);
// The image pair of the image-conditioned pose heads (preprocess.hip): OpenCV's 8-bit INTER_LINEAR resize of src[rows[q]] as
// fp32 planes, uint8 HWC [P, Hin, Win, 3] -> [Q, 3, OW, OH] (transposed) or [Q, 3, OH, OW]
struct PoseImagesParams {
    const unsigned char* src;
    int P, Hin, Win;
    const int* rows; int Q;                    // device; NULL: the identity (Q == P)
    const int *xstart, *xcoef;                 // [OW], [OW, 2]: first tap and the two 11-bit coefficients of every output column
    const int *ystart, *ycoef;                 // [OH], [OH, 2]
    int OH, OW, transposed;
    float* out;
};
int pope_pose_images_check(const PoseImagesParams& p);   // no HIP call
int pope_launch_pose_images(const PoseImagesParams& p, hipStream_t stream);

// One LoFTR encoder layer update (loftr.hip): x <- layer(x, source); weights as f16x3 planes (bias-free Linears)
struct LoftrLayerParams {
    float* x;              // [n, L, C] in / out
    const float* source;   // [n, S, C] (may be x itself: 'self' layers)
    int n, L, S, C, H;
    const void *q_wp, *kv_wp, *merge_wp, *mlp0_wp, *mlp1_wp;   // [C,C], [2C,C] (k rows then v rows), [C,C], [2C,2C], [C,2C]
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
    const float *q_w, *kv_w, *merge_w, *mlp0_w, *mlp1_w;       // POPE_PREC_F32_MFMA: the same matrices as fp32
    int precision;                                             // POPE_PREC_F16X3 | POPE_PREC_F32_MFMA
    float ln_eps;
    void* ws; size_t ws_bytes;
    unsigned* range_flag;
    // optional padding masks (linear_attention.py:35-41), 0 / 1 fp32: x_mask [n, L] zeroes padded query rows' Q,
    // source_mask [n, S] padded source rows' K and V; null = no mask (the unmasked kernels)
    const float* x_mask;
    const float* source_mask;
    int attention;         // POPE_LOFTR_ATTN_LINEAR (0: a zeroed struct is the linear layer) | POPE_LOFTR_ATTN_FULL (softmax; no masks)
};
// Full softmax attention of the layer (loftr_attention.hip): q [n L, C], kv [n S, 2C] (k | v) fp32 -> the message [n L, C] as fp32
// rows, or (planes) as activation planes with POPE_RANGE_QKV on a value outside the f16 range.  C = 256 / 128, H = 8.
int pope_loftr_full_attention_check(const void* q, const void* kv, int n, int L, int S, int C, int H, const void* out);   // no HIP call
int pope_launch_loftr_full_attention(const float* q, const float* kv, int n, int L, int S, int C, int H, bool planes, float* msg,
                                     unsigned* range_flag, hipStream_t stream);
// ResNet-FPN local-feature CNN of the LoFTR matcher (conv.hip; resnet_fpn.py:43-118)
struct ResnetFpnParams {
    const float* img;          // [n, 1, H, W] gray in [0, 1]
    int n, H, W;               // H, W multiples of 8
    const void* w[22];         // weight planes (scale 256), BatchNorm folded: order in pope_hip.h
    const float* b[22];        // folded biases (null where the reference has neither bias nor BatchNorm)
    const float* wf[22];       // POPE_PREC_F32_MFMA: the same [Cout, K] matrices as fp32 (w may then be null)
    int precision;             // POPE_PREC_F16X3 | POPE_PREC_F32_MFMA
    float* out_c;              // [n, H/8 + 2, W/8 + 2, 256] fp32, zero border
    float* out_f;              // [n, H/2 + 2, W/2 + 2, 128] fp32, border undefined
    void* ws; size_t ws_bytes;
    unsigned* range_flag;
};
size_t pope_resnetfpn_workspace(int n, int H, int W);
int pope_launch_resnetfpn(const ResnetFpnParams& q, hipStream_t stream);
// LoFTR fine stage (fine.hip; fine_preprocess.py:29-59, fine_matching.py:15-74)
struct FinePreParams {
    const float *f0, *f1;          // 1/2-resolution maps, addressed through element strides (n, c, h, w)
    long long s0[4], s1[4];
    int H0, W0, H1, W1;            // map sizes
    int wc0, wc1;                  // coarse grid widths (cell id = cy * wc + cx)
    const float *fc0, *fc1;        // [n, L, Cc], [n, S, Cc] coarse features after the coarse transformer
    int L, S, Cc, Cf;
    const long long *b_ids, *i_ids, *j_ids;   // [M] matches (device)
    int M, Wn, stride;             // window size (5), fine pixels per coarse cell
    const void *down_wp, *merge_wp;   // [Cf, Cc], [Cf, 2 Cf] weight planes
    const float *down_b, *merge_b;
    const float *down_w, *merge_w;    // POPE_PREC_F32_MFMA: the same matrices as fp32
    int precision;                    // POPE_PREC_F16X3 | POPE_PREC_F32_MFMA
    float* out;                    // [2 M, Wn * Wn, Cf]: windows of stream 0, then of stream 1
    void* ws; size_t ws_bytes;
    unsigned* range_flag;
    const long long* ref0_of_pair; // [n_pairs] (device) or nullptr: map 0 has n0 rows and pair b reads row ref0_of_pair[b]; fc0 stays per pair
    int n_pairs, n0;
};
size_t pope_fine_preprocess_workspace(int M, int WW, int Cc, int Cf);
int pope_launch_fine_preprocess(const FinePreParams& q, hipStream_t stream);
int pope_launch_fine_match(const float* win0, const float* win1, int M, int Wn, int C, const float* mkpts1_c, float scale_px,
                           float* expec, float* mkpts1_f, hipStream_t stream);
// per-pair rescaling (fine_matching.py:68): the offset of match m is scaled by scale_px * scale1[b_ids[m]] (x, y)
int pope_launch_fine_match_scaled(const float* win0, const float* win1, int M, int Wn, int C, const float* mkpts1_c, float scale_px,
                                  const float* scale1, const long long* b_ids, float* expec, float* mkpts1_f, hipStream_t stream);
size_t pope_loftr_layer_workspace(int n, int L, int S, int C, int H);
int pope_launch_loftr_layer(const LoftrLayerParams& p, hipStream_t stream);
// The layer's linear attention alone (the same launches): q [n L, C], kv [n S, 2C] (k | v) fp32 -> the message as fp32 rows
// (out_f32) or as activation planes (out_planes; POPE_RANGE_INPUT on a value outside the f16 range); exactly one of the two.
// ws: 256-byte aligned, pope_loftr_linear_attention_workspace bytes (0 for bad sizes).  The check makes no HIP call.
void pope_loftr_linattn_seams(int* chunk_rows, int* rows_per_block);
size_t pope_loftr_linear_attention_workspace(int n, int S, int C, int H);
int pope_loftr_linear_attention_check(const void* q, const void* kv, int n, int L, int S, int C, int H, const void* out_f32,
                                      const void* out_planes, const void* ws, size_t ws_bytes);
int pope_launch_loftr_linear_attention(const float* q, const float* kv, const float* x_mask, const float* source_mask, int n, int L, int S,
                                       int C, int H, float* out_f32, void* out_planes, void* ws, size_t ws_bytes, unsigned* range_flag,
                                       hipStream_t stream);

// SAM image encoder (sam.hip; segment_anything/segment_anything/modeling/image_encoder.py:17-118): the arguments of
// pope_sam_encoder_forward_f32.  The weights are read from the ABI's struct as it is (pope_hip.h: what every `*_wp` holds per precision).
struct SamEncArgs {
    const pope_sam_encoder_weights* w;
    const float* image;   // [B, 3, img, img] fp32
    float* out;           // [B, out_chans, g, g] fp32, g = img / patch
    int B;
    int n_taps; const int* tap_blocks; float* const* tap_out;   // optional block outputs [B g g, dim] fp32 (host arrays)
    void* ws; size_t ws_bytes;
    unsigned* range_flag;
};
size_t pope_sam_encoder_workspace(const pope_sam_encoder_weights* w, int B);
// every POPE_ERR_ARG / POPE_ERR_WORKSPACE is returned before the first HIP call
int pope_launch_sam_encoder(const SamEncArgs& a, hipStream_t stream);

// Attention of one SAM encoder block on the f16 matrix cores (sam_attention.hip), POPE_PREC_F16X3 or (plain) POPE_PREC_F16:
// the plan of a geometry (window side ws; ws = g: a global block), its operand regions in the caller's workspace, the
// once-per-pass preparation and one block.
struct SamAttnPlan {
    int B = 0, g = 0, ws = 0, heads = 0, hd = 0;   // images, token grid g x g, window side, heads, head dim
    int nstep = 0;                                 // score depth / 16
    bool bias = false;               // relative-position terms as a bias table (sam_attn_kernel<.., BIAS>), not as columns of Q' / K'
    size_t qp = 0, kp = 0, vp = 0, tab = 0, map = 0;   // bytes: operand planes Q', K', V, the bias table (0 without one), the row map
    int hpg = 0, n_tasks = 0;        // the relative-position kernel's heads per wave and task count
    bool launchable = false;         // false: an operand reaches 4 GiB or the task count 2^31 (the caller splits the batch)
};
struct SamAttnOperands { void *q, *k, *v, *tab; int* map; };   // 256-byte aligned regions of qp, kp, vp, tab, map bytes
bool pope_sam_attn_plan(int B, int g, int ws, int heads, int hd, SamAttnPlan& p);   // false: no kernel holds hd + 2 ws score columns; no HIP call
// prepare and block take a plan that pope_sam_attn_plan accepted; block returns POPE_ERR_ARG, before any launch, for one that is
// not `launchable` or whose bias table has no region
int pope_sam_attn_prepare(const SamAttnPlan& p, const SamAttnOperands& o, bool plain, hipStream_t stream);
// xn = norm1(x) as the precision's GEMM operand [B g g, dim] -> att_out, the proj GEMM's operand; reads k.qkv_wp, qkv_b, rel_h, rel_w
int pope_sam_attn_block(const SamAttnPlan& p, const SamAttnOperands& o, bool plain, const void* xn, const pope_sam_block_weights& k,
                        void* att_out, unsigned* flag, hipStream_t stream);

// POPE_PREC_F32_MFMA pieces of the SAM encoder (sam_f32.hip): every operand fp32
int pope_launch_sam32_im2col(const float* img, float* out, int B, int S, int P, hipStream_t stream);   // -> rows [B g g, 3 P P]; P % 4 == 0
int pope_sam32_attention_check(int B, int g, int ws, int heads, int hd);   // head dim, grid size and LDS size of the launch below; no HIP call
// qkv [B g g, 3 dim] -> out [B g g, dim]; rel_h / rel_w [ws, ws, hd].  The caller has passed pope_sam32_attention_check.
int pope_launch_sam32_attention(const float* qkv, const float* qkv_bias, const float* rel_h, const float* rel_w, float* out, int B, int g,
                                int ws, int heads, int hd, hipStream_t stream);
// LayerNorm2d: bordered_out: in [B g g, C] -> out [B, g + 2, g + 2, C] with a zero border; else in bordered -> out NCHW [B, C, g, g]
int pope_launch_sam32_ln2d(const float* in, const float* w, const float* b, float* out, int B, int g, int C, float eps, bool bordered_out,
                           hipStream_t stream);

// Batched relative pose (pose.hip; src/utils/metrics.py:69-94): one workgroup per pair
struct PoseParams {
    const float* kpts0; const float* kpts1;   // [M, 2] fp32 pixel coordinates, the matches of pair b contiguous, pairs in order
    const int* counts;                        // [B] matches per pair (device; the matcher's counts)
    const double* K0; const double* K1;       // [B, 9] intrinsics, row-major
    int B; long long M;                       // M = rows of kpts0 / kpts1 (capacity; sum(counts) <= M)
    double thresh, conf;                      // pixels; RANSAC confidence
    int max_iters;
    unsigned long long seed;
    double* R; double* t; double* E;          // [B, 9], [B, 3], [B, 9]
    unsigned char* inliers;                   // [M]
    int* info;                                // [B, 8]: n_good (0 = None), RANSAC inliers, hypotheses, rounds, best hypothesis, best root, N, status
    void* xn; unsigned char* mask_ws; unsigned char* cheir_ws;   // filled in by the launcher from the workspace
    double* cand_ws; int* cmeta_ws;
};
size_t pope_pose_workspace(int B, long long M);
int pope_launch_estimate_pose(PoseParams q, void* ws, size_t ws_bytes, hipStream_t stream);
int pope_launch_five_point(const double* x0, const double* x1, int S, double* E_out, int* n_out, hipStream_t stream);

// Device-side glue of the batched driver step (vote.hip): the arguments of pope_vote_top3_batch_f32 / pope_slot_tally_f32
int pope_launch_vote_top3_batch(const float* cls_ref, const float* cls_prop, const int* seg, int Q, int N, int D, float eps,
                                float* scores, float* slot_scores, long long* slot_index, int* pair_row, unsigned char* pair_live,
                                hipStream_t stream);
int pope_launch_vote_top3_shared(const float* cls_ref, const float* cls_prop, const int* seg, int S, const int* query_seg,
                                 const int* score_begin, int Q, int N, int D, float eps, float* scores, float* slot_scores,
                                 long long* slot_index, int* pair_row, unsigned char* pair_live, hipStream_t stream);
int pope_launch_slot_tally(const long long* m_bids, const float* mconf, const float* mkpts0, const float* mkpts1,
                           const unsigned char* pair_live, int Q, long long M, float conf_thr, int* pair_begin, int* pair_count,
                           long long* matching_score, int* best_slot, int* best_count, float* best_kpts0, float* best_kpts1,
                           hipStream_t stream);

// SAM mask decoder (sam_decoder.hip): the arguments of pope_sam_decoder_forward_f32 and, with prompt_image (HOST [P]: the image
// of each prompt) and image = n_images embeddings, of pope_sam_decoder_forward_images_f32
struct SamDecArgs {
    const pope_sam_decoder_weights* w;
    const float *image, *image_pe, *sparse, *dense;
    int P, n_sparse, multimask;
    int n_images;
    const int* prompt_image;
    long long dense_stride;
    float *masks, *iou, *hs_out, *keys_out;
    void* ws;
    size_t ws_bytes;
    unsigned* range_flag;
};
size_t pope_sam_decoder_workspace(const pope_sam_decoder_weights* w, int P, int n_sparse, int shared);
size_t pope_sam_decoder_images_workspace(const pope_sam_decoder_weights* w, int n_images, const int* prompt_image, int P, int n_sparse,
                                         long long dense_stride);
int pope_launch_sam_decoder(const SamDecArgs& a, hipStream_t stream);
// its kernels one at a time (pope_sam_decoder_*_f32): POPE_ERR_ARG on the host before the launch; slot_host: HOST [P]
void pope_sam_decoder_seam_values(int* chunk, int* lin_rows, int* max_tokens, int* base_tokens);
int pope_launch_sam_decoder_token_linear(const float* X, int ldx, const float* add, int add_cols, const float* W, const float* bias,
                                         const float* res, float* Y, int ldy, int M, int N, int K, int relu, hipStream_t stream);
int pope_launch_sam_decoder_self_attention(const float* qkv, float* out, int P, int T, hipStream_t stream);
int pope_launch_sam_decoder_t2i_attention(const float* q, const float* K, int ldk, long long kps, const float* V, long long vps,
                                          const int* slot_host, float* out, int T, int P, hipStream_t stream);
int pope_launch_sam_decoder_i2t_attention(const float* Q, long long qps, const int* slot_host, const float* kv, int T, int P,
                                          float* out_f32, void* out_planes, unsigned* range_flag, hipStream_t stream);
int pope_launch_sam_decoder_residual_norm(const float* res, long long rps, const int* slot_host, const float* y, const float* w,
                                          const float* b, float eps, const float* pe_t, float* keys, void* opA, void* opB, int f32,
                                          int P, unsigned* range_flag, hipStream_t stream);
int pope_launch_sam_decoder_prepare_keys(const float* image, long long image_stride, const float* image_pe, const float* dense,
                                         long long dense_stride, int nz, float* keys, void* opA, void* opB, int f32, float* pe_t,
                                         unsigned* range_flag, hipStream_t stream);
int pope_launch_sam_decoder_upscale_tail(const float* y, const float* ln_w, const float* ln_b, float eps, const float* w2,
                                         const float* b2, const float* hyper, int multimask, int P, float* masks, hipStream_t stream);

// SAM prompt encoder, mask prompts (sam_prompt.hip): pope_sam_mask_embed_f32
int pope_sam_mask_embed_check(const pope_sam_mask_embed_weights* w, const float* masks, int P, const float* dense);   // no HIP call
int pope_launch_sam_mask_embed(const pope_sam_mask_embed_weights* w, const float* masks, int P, float* dense, hipStream_t stream);

// SAM generator post-processing (sam_postprocess.hip): the arguments of pope_sam_postprocess_f32
struct SamPostArgs {
    const float* low;
    int M, h, w;
    const int* sel;
    int n_sel, img, ih, iw, H, W;
    double mask_threshold, stability_offset;
    int* stats;
    unsigned* packed;
    float* logits;
    void* ws;
    size_t ws_bytes;
};
size_t pope_sam_postprocess_workspace(int img, int H, int W);
int pope_launch_sam_postprocess(const SamPostArgs& a, hipStream_t stream);
int pope_launch_sam_nms(const float* boxes, const float* scores, int n, float thresh, int* keep, int* count, hipStream_t stream);
int pope_launch_sam_nms_segments(const float* boxes, const float* scores, const int* seg_offsets, int S, int n, float thresh,
                                 int* keep, int* count, hipStream_t stream);

// SAM generator small-region clean-up (sam_regions.hip): the arguments of pope_sam_small_regions_u32
struct SamRegionsArgs {
    const unsigned* packed;
    int n, H, W, min_area;
    unsigned* packed_out;
    int *unchanged, *boxes, *area;
    void* ws;
    size_t ws_bytes;
};
int pope_sam_small_regions_chunk();   // masks in flight: the workspace does not grow beyond that many
size_t pope_sam_small_regions_workspace(int n, int H, int W);
int pope_sam_small_regions_check(const SamRegionsArgs& a);   // no HIP call
int pope_launch_sam_small_regions(const SamRegionsArgs& a, hipStream_t stream);

// SAM generator run-length encoding (sam_rle.hip): the arguments of pope_sam_rle_u32
struct SamRleArgs {
    const unsigned* packed;
    int n, H, W;
    int* lengths;               // counts == nullptr: the lengths are written
    const long long* offsets;   // counts != nullptr: [n + 1], device
    unsigned* counts;
    long long capacity;
};
int pope_sam_rle_check(const SamRleArgs& a);   // no HIP call
int pope_launch_sam_rle(const SamRleArgs& a, hipStream_t stream);

// Learned pose regressor (pose_regressor.hip; pose/model.py:Mkpts_Reg_Model): the inputs of pope_pose_regressor_forward_f32
struct PoseRegInput {
    const float *dense0, *dense1;             // [B, S, 2], or
    const float *kpts0, *kpts1;               // [M, 2] compacted, with
    const int* counts;                        // [B] (device)
    const int* sample_index;                  // [B, S] or null
    const unsigned long long* seeds;          // [B] or null
    int B, S;
    long long M;
};
int pope_posereg_input_check(const PoseRegInput& in);   // no HIP call
int pope_launch_posereg_embed(const PoseRegInput& in, float* X, int* index, int* status, hipStream_t stream);
int pope_launch_posereg_layer(const pope_pose_regressor_layer& w, float* X, int B, int S, int G, hipStream_t stream);
// Y[B, N] = leaky_relu(A[B, K] . W[N, K]^T + bias, 0.01), W read once per chunk of pairs (mlp.0 and mlp.3)
int pope_launch_posereg_stream_linear(const float* A, const float* W, const float* bias, float* Y, int B, long long K, int N,
                                      hipStream_t stream);
int pope_launch_posereg_tail(const pope_pose_regressor_weights& w, const float* Y2, const int* status, int B, float* trans,
                             float* rot, hipStream_t stream);

// MoCoPE fusion pose model (mocope.hip; pose/model0604.py:MoCoPE): the arguments of pope_mocope_forward_f32 / pope_mocope_tap_f32
struct MocopeArgs {
    const pope_mocope_weights* w;
    PoseRegInput in;
    const float *feat0, *feat1;     // [B, 1000]
    int G, train_type;
    int stage;                      // POPE_MOCOPE_TAP_*, or MOCOPE_STAGE_FULL: trans / rot are written
    float *trans, *rot, *tap_out;
    int* status;
    void* ws; size_t ws_bytes;
};
constexpr int MOCOPE_STAGE_FULL = -1;
size_t pope_mocope_workspace(int B, int S);
int pope_mocope_check(const MocopeArgs& a);   // no HIP call
int pope_launch_mocope(const MocopeArgs& a, hipStream_t stream);
// the launches of mocope.hip one by one (the op-level entries pope_mocope_*_f32; the argument checks are theirs)
int pope_launch_mocope_linear(const float* A, const float* W, const float* bias, float* Y, int R, int K, int N, int act, hipStream_t stream);
int pope_launch_mocope_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int R, int S, int G,
                                 int d, hipStream_t stream);
int pope_launch_mocope_add_ln(float* X, const float* Y, const float* w1, const float* b1, const float* w2, const float* b2, int R, int d,
                              hipStream_t stream);
int pope_launch_mocope_ffn76(float* X, const float* l1w, const float* l1b, const float* l2w, const float* l2b, const float* nw,
                             const float* nb, const float* fw, const float* fb, int R, hipStream_t stream);

// ConvNeXtV2 backbone and the image pose head (convnext.hip; pose/convnextv2/convnextv2.py, pose/model_cnn.py): the arguments of
// pope_convnext_forward_f32 and of the op-level entries.  The *_check functions make no HIP call.
struct ConvNextArgs {
    const pope_convnext_weights* w;
    const float* image;
    int B, H, W, precision;
    float *features, *logits;
    float* const* taps;
    void* ws; size_t ws_bytes;
    unsigned* range_flag;
};
size_t pope_convnext_workspace(const pope_convnext_weights* w, int B, int H, int W);   // 0: bad weights or geometry
int pope_convnext_check(const ConvNextArgs& a);
int pope_launch_convnext(const ConvNextArgs& a, hipStream_t stream);
int pope_launch_convnext_dwconv(const float* x, const float* w49, const float* bias, float* y, int B, int H, int W, int C,
                                hipStream_t stream);
size_t pope_convnext_grn_workspace(int B, int HW, int C);
int pope_convnext_grn_check(const float* x, const float* gamma, const float* beta, int B, int HW, int C, const float* y_f32,
                            const void* y_planes, const void* ws, size_t ws_bytes);
int pope_launch_convnext_grn(const float* x, const float* gamma, const float* beta, int B, int HW, int C, float* y_f32, void* y_planes,
                             void* ws, unsigned* range_flag, hipStream_t stream);
int pope_launch_convnext_pose_heads(const float* feat, const float* trans_w, const float* trans_b, const float* rot_w,
                                    const float* rot_b, int mode, int B, int inner, float* trans, float* rot, hipStream_t stream);

// Vision Mamba backbone (vim.hip; pose/vim/models_mamba.py:VisionMamba): the arguments of pope_vim_forward_f32 and of the
// op-level entries.  The *_check functions make no HIP call.
struct VimArgs {
    const pope_vim_weights* w;
    const float* image;
    int B, precision;
    float *features, *logits;
    float* const* taps;
    void* ws; size_t ws_bytes;
    unsigned* range_flag;
};
size_t pope_vim_workspace(const pope_vim_weights* w, int B);   // 0: bad weights or geometry
int pope_vim_check(const VimArgs& a);
int pope_launch_vim(const VimArgs& a, hipStream_t stream);
int pope_vim_scan_chunk_len();
size_t pope_vim_scan_workspace(int B, int L, int E);
int pope_vim_scan_check(const float* xc, const float* z, int ldz, const float* xdbl, const pope_vim_dir_weights* dirs, int B, int L, int E,
                        int R, const float* out_f32, const void* out_planes, const void* ws, size_t ws_bytes);
int pope_launch_vim_scan(const float* xc, const float* z, int ldz, const float* xdbl, const pope_vim_dir_weights* dirs, int B, int L, int E,
                         int R, float* out_f32, void* out_planes, void* ws, unsigned* range_flag, hipStream_t stream);
int pope_vim_conv1d_check(const float* x, int ldx, const pope_vim_dir_weights* dirs, int B, int L, int E, const float* xc);
int pope_launch_vim_conv1d(const float* x, int ldx, const pope_vim_dir_weights* dirs, int B, int L, int E, float* xc, hipStream_t stream);
int pope_vim_add_rmsnorm_check(const float* hidden, const float* w, const float* y_f32, const void* y_planes, long long rows, int D, float eps,
                               long long row_stride, long long row_offset);
int pope_launch_vim_add_rmsnorm(const float* hidden, const float* res_in, float* res_out, const float* w, float* y_f32, void* y_planes,
                                long long rows, int D, float eps, long long row_stride, long long row_offset, unsigned* range_flag,
                                hipStream_t stream);
