// C ABI (include/pope_hip.h) over the kernel launchers: the device scope of the stream, argument checks and the translation
// of the public structs into the launchers' parameters.  No allocation, no synchronisation.  (The ViT forward: vit_forward.hip.)
#include "../../include/pope_hip.h"
#include "common.h"
#include "conv_layer.h"
#include "kernels.h"
#include "linear.h"
#include "stream_device.h"
#include <cstdlib>

namespace {

__global__ __launch_bounds__(256) void cls_cosine_kernel(const float* __restrict__ ref, const float* __restrict__ fea,
                                                          int P, int D, float eps, float* __restrict__ scores) {
    // x.y / (max(|x|, eps) * max(|y|, eps)) — torch semantics, each norm clamped separately
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const float* f = fea + size_t(p) * D;
    float dot = 0.f, nr = 0.f, nf = 0.f;
    for (int i = lane; i < D; i += 64) {
        const float a = ref[i], b = f[i];
        dot += a * b;
        nr += a * a;
        nf += b * b;
    }
    dot = wave_sum(dot);
    nr = wave_sum(nr);
    nf = wave_sum(nf);
    if (lane == 0) scores[p] = dot / (fmaxf(sqrtf(nr), eps) * fmaxf(sqrtf(nf), eps));
}

}  // namespace

extern "C" {

int pope_abi_version(void) { return POPE_ABI_VERSION; }

const char* pope_error_string(int code) {
    switch (code) {
        case POPE_OK: return "ok";
        case POPE_ERR_ARG: return "invalid argument (shape, alignment or null pointer)";
        case POPE_ERR_LAUNCH: return "HIP launch failed";
        case POPE_ERR_WORKSPACE: return "workspace too small";
    }
    return "unknown error";
}

int pope_layernorm_f32(const float* x, const float* weight, const float* bias, float* y, int rows, int dim,
                       float eps, void* stream) {
    StreamDevice on_device(stream);
    if (!x || !weight || !bias || !y) return POPE_ERR_ARG;
    return pope_launch_layernorm_f32(x, dim, weight, bias, y, dim, rows, dim, eps, static_cast<hipStream_t>(stream));
}

int pope_linear_f32(const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                    int epilogue, const float* gamma, const float* res, int precision, unsigned* range_flag,
                    void* stream) {
    const bool swiglu = epilogue == POPE_EPI_BIAS_SWIGLU;
    if (!A || !W || !C || epilogue < 0 || (epilogue > POPE_EPI_BIAS_LS_RES && !swiglu)) return POPE_ERR_ARG;
    if (precision != POPE_PREC_F32_MFMA && precision != POPE_PREC_F16X3) return POPE_ERR_ARG;
    // SwiGLU: fp32 MFMA only here (the f16x3 form is the planes entry below); N = 2 hidden columns in, [M, N / 2] out
    if (swiglu && (precision != POPE_PREC_F32_MFMA || N <= 0 || (N & 63))) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    const GemmParams g = pope_linear_params(LINEAR_F32, A, W, bias, C, nullptr, M, N, K, epilogue, gamma, res, 0, range_flag);
    // shapes the f16x3 kernel does not take (K % 32 != 0) run on the fp32 MFMA: same contract, same results
    if (precision == POPE_PREC_F16X3 && pope_gemm_f16x3_supported(g))
        return pope_launch_gemm_nt_f16x3(g, static_cast<hipStream_t>(stream));
    return pope_launch_gemm_nt_f32(g, static_cast<hipStream_t>(stream));
}

int pope_split_planes_f32(const float* src, void* planes, int rows, int cols, float scale, unsigned* range_flag, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_split_planes(src, planes, rows, cols, scale, range_flag, static_cast<hipStream_t>(stream));
}

int pope_linear_planes_f32(const void* a_planes, const void* w_planes, const float* bias, float* C, void* c_planes,
                           int M, int N, int K, int epilogue, const float* gamma, const float* res, unsigned* range_flag,
                           void* stream) {
    const bool swiglu = epilogue == POPE_EPI_BIAS_SWIGLU;
    if (epilogue < 0 || (epilogue > POPE_EPI_BIAS_LS_RES && !swiglu)) return POPE_ERR_ARG;
    if (swiglu && (!a_planes || !w_planes || (!C) == (!c_planes) || N <= 0 || (N & 63))) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_gemm_planes(pope_linear_params(LINEAR_PLANES, a_planes, w_planes, bias, C, c_planes, M, N, K, epilogue, gamma, res,
                                                      0, range_flag), static_cast<hipStream_t>(stream));
}

int pope_layernorm_planes_f32(const float* x, const float* weight, const float* bias, void* y_planes, int rows, int dim,
                              float eps, unsigned* range_flag, void* stream) {
    StreamDevice on_device(stream);
    if (!x || !weight || !bias) return POPE_ERR_ARG;
    return pope_launch_layernorm_planes(x, dim, weight, bias, y_planes, rows, dim, eps, range_flag, static_cast<hipStream_t>(stream));
}

// the `rowln` launch of vit_forward.hip with every operand from the caller; checked before the stream's device is touched
int pope_linear_rowln_f32(const void* a_planes, const void* w_planes, int M, int K, const float* bias, const float* gamma,
                          const float* res, int res_mod, float* x, const float* ln_w, const float* ln_b, float eps,
                          void* ln_planes, float* ln_out, unsigned* range_flag, void* stream) {
    const GemmParams g = pope_linear_rowln_params(a_planes, w_planes, M, 384, K, bias, gamma, res, res_mod, x, ln_w, ln_b, eps, ln_planes,
                                                  ln_out, range_flag);
    if (!pope_gemm_rowln_args_ok(g)) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_gemm_rowln(g, static_cast<hipStream_t>(stream));
}

int pope_layernorm_rowln_order_f32(const float* x, const float* weight, const float* bias, void* y_planes, float* y_f32,
                                   int rows, float eps, unsigned* range_flag, void* stream) {
    if (!x || !weight || !bias || (!y_planes) == (!y_f32) || rows <= 0) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_layernorm_rowln_order(x, weight, bias, y_planes, y_f32, rows, eps, range_flag, static_cast<hipStream_t>(stream));
}

// the operand producers of the plain-f16 GEMMs and of the matcher, one launch each; checked before the stream's device is touched
int pope_layernorm_f16(const float* x, const float* weight, const float* bias, void* y_f16, int rows, int dim, float eps,
                       unsigned* range_flag, void* stream) {
    if (!x || !weight || !bias || !y_f16 || rows <= 0 || !pope_ln_width_ok(dim)) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_layernorm_f16(x, weight, bias, y_f16, rows, dim, eps, range_flag, static_cast<hipStream_t>(stream));
}

int pope_to_f16(const float* x, void* y_f16, long long n, unsigned* range_flag, void* stream) {
    if (!x || !y_f16 || n <= 0 || (n & 3)) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_to_f16(x, y_f16, n / 4, range_flag, static_cast<hipStream_t>(stream));
}

// a Linear of the plain-f16 GEMM family through the router the models use (vit_forward.hip's `linear` with LINEAR_PLAIN, sam.hip);
// checked before the stream's device is touched
int pope_linear_f16(const void* a_f16, const void* w_f16, const float* bias, float* C, void* c_f16, int M, int N, int K, int epilogue,
                    const float* gamma, const float* res, int res_mod, unsigned* range_flag, void* stream) {
    static_assert(int(POPE_EPI_QKV_F16) == int(EPI_QKV_F16), "the public value is the router's");
    const bool out_f16 = epilogue == POPE_EPI_BIAS_GELU || epilogue == POPE_EPI_QKV_F16;
    if (!out_f16 && epilogue != POPE_EPI_BIAS && epilogue != POPE_EPI_BIAS_LS_RES) return POPE_ERR_ARG;
    if (!a_f16 || !w_f16 || (out_f16 ? !c_f16 || C : !C || c_f16)) return POPE_ERR_ARG;
    if (M <= 0 || N <= 0 || K < 128 || (K & 63) || (N & (out_f16 ? 63 : 3))) return POPE_ERR_ARG;
    if (epilogue == POPE_EPI_QKV_F16 && N % 192) return POPE_ERR_ARG;
    if (epilogue == POPE_EPI_BIAS_LS_RES && (!res || (!gamma && res_mod <= 0))) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    GemmParams g = pope_linear_params(LINEAR_PLAIN, a_f16, w_f16, bias, C, c_f16, M, N, K, epilogue, gamma, res, res_mod, range_flag);
    if (epilogue == EPI_QKV_F16) { g.sam_dim = N / 3; g.sam_qscale = 0.125f * 1.44269504088896340736f; }   // vit_forward.hip's QKV launch
    return pope_launch_gemm_planes(g, static_cast<hipStream_t>(stream));
}

int pope_div_planes_f32(const float* src, long long batch_stride, void* planes, int n, int rows, int cols, float divisor, float scale,
                        unsigned* range_flag, void* stream) {
    if (!src || !planes || n <= 0 || rows <= 0 || cols <= 0 || (cols & 31) || (batch_stride & 1) ||
        batch_stride < (long long)rows * cols)
        return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_div_planes(src, batch_stride, planes, n, rows, cols, divisor, scale, range_flag, static_cast<hipStream_t>(stream));
}

int pope_patch_embed_f32(const float* img, const float* proj_w, const float* posb, float* tokens, int B, int H,
                         int W, int patch, int dim, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_patch_embed_f32(img, proj_w, posb, tokens, B, H, W, patch, dim, static_cast<hipStream_t>(stream));
}

int pope_patch_embed_planes_f32(const float* img, const void* proj_w_planes, const float* posb, float* tokens, int B, int H,
                                int W, int patch, int dim, void* a_planes_scratch, size_t scratch_bytes, unsigned* range_flag,
                                void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_patch_embed_planes(img, proj_w_planes, posb, tokens, B, H, W, patch, dim, a_planes_scratch, scratch_bytes,
                                          range_flag, static_cast<hipStream_t>(stream));
}

int pope_attention_planes_f32(const void* qkv_planes, void* out_planes, int B, int N, int heads, void* stream) {
    StreamDevice on_device(stream);
    if (!qkv_planes || !out_planes) return POPE_ERR_ARG;
    return pope_launch_attention_f16x3_planes_io(qkv_planes, out_planes, B, N, heads, static_cast<hipStream_t>(stream));
}

int pope_attention_f16(const void* qkv_f16, void* out_f16, int B, int N, int heads, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_attention_f16_dma(qkv_f16, out_f16, B, N, heads, static_cast<hipStream_t>(stream));
}

int pope_attention_planes_diag_f32(const void* qkv_planes, void* out_planes, int B, int N, int heads, long long* exact_passes_host,
                                   void* stream) {
    StreamDevice on_device(stream);
    if (!qkv_planes || !out_planes) return POPE_ERR_ARG;
    return pope_launch_attention_f16x3_planes_io_diag(qkv_planes, out_planes, B, N, heads, exact_passes_host, static_cast<hipStream_t>(stream));
}

int pope_attention_f32(const float* qkv, float* out, int B, int N, int heads, int precision, unsigned* range_flag,
                       void* stream) {
    StreamDevice on_device(stream);
    if (!qkv || !out) return POPE_ERR_ARG;
    if (precision == POPE_PREC_F16X3 && range_flag) {  // q, k, v are split inside the kernel: check them in a scan
        if (B <= 0 || N <= 0 || heads <= 0) return POPE_ERR_ARG;
        const int rc = pope_launch_range_check(qkv, size_t(B) * N * 3 * heads * 64, 1.0f, range_flag, POPE_RANGE_INPUT,
                                               static_cast<hipStream_t>(stream));
        if (rc) return rc;
    }
    if (precision == POPE_PREC_F16X3) return pope_launch_attention_f16x3(qkv, out, B, N, heads, static_cast<hipStream_t>(stream));
    if (precision != POPE_PREC_F32_MFMA) return POPE_ERR_ARG;
    return pope_launch_attention_f32(qkv, out, B, N, heads, static_cast<hipStream_t>(stream));
}

int pope_cls_cosine_f32(const float* ref, const float* fea, int P, int D, float eps, float* scores, void* stream) {
    StreamDevice on_device(stream);
    if (!ref || !fea || !scores || P <= 0 || D <= 0) return POPE_ERR_ARG;
    hipLaunchKernelGGL(cls_cosine_kernel, dim3((P + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), ref, fea,
                       P, D, eps, scores);
    return pope_check_launch();
}

int pope_event_create(void** event_host) {
    if (!event_host) return POPE_ERR_ARG;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return POPE_ERR_LAUNCH;
    *event_host = e;
    return POPE_OK;
}
int pope_event_destroy(void* event) {
    return hipEventDestroy(static_cast<hipEvent_t>(event)) == hipSuccess ? POPE_OK : POPE_ERR_LAUNCH;
}
int pope_event_elapsed_ms(void* start, void* stop, float* ms_host) {
    if (!ms_host) return POPE_ERR_ARG;
    return hipEventElapsedTime(ms_host, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)) == hipSuccess
               ? POPE_OK : POPE_ERR_LAUNCH;
}

namespace {
// workspace carving of the dense matcher, shared by the size query and the entry: the dual-softmax pieces, the pair extents of
// the padded border rule, then the Sinkhorn scratch (u [n, L + 1], v [n, S + 1], the last column step's maxima [n, S])
struct MatchLayout {
    size_t nl, ns, part, rowp, colp, pl0, pl1, simb, extent, skh_u, skh_v, skh_cmax, total;
    int ncb, nrb, nrb2, ldp;
    explicit MatchLayout(const pope_dense_match_args& a) {
        const size_t n = size_t(a.n);
        const int L = a.L, S = a.S;
        nl = pope_align256(n * L * 4);
        ns = pope_align256(n * S * 4);
        ncb = 2 * ((S + 127) / 128);
        nrb = 4 * ((L + 127) / 128);
        nrb2 = pope_match_nrb2(L);
        ldp = (S + 3) & ~3;
        part = pope_align256(n * nrb2 * ldp * 4);
        const bool x3 = a.precision == POPE_PREC_F16X3;
        rowp = x3 ? pope_align256(n * L * ncb * 8) : 0;
        colp = x3 ? pope_align256(n * nrb * ldp * 4) : 0;
        pl0 = x3 ? pope_align256(n * L * a.C * 4) : 0;
        pl1 = x3 ? pope_align256(n * S * a.C * 4) : 0;
        // (Sinkhorn: the matrix holds conf after the confidence pass even when it is not published; it lives here then)
        simb = a.conf_matrix ? 0 : pope_align256(n * L * S * 4);
        extent = a.border_mask0 || a.border_mask1 ? pope_align256(n * 4 * 4) : 0;
        const bool skh = a.match_type == POPE_MATCH_SINKHORN;
        skh_u = skh ? pope_align256(n * (L + 1) * 4) : 0;
        skh_v = skh ? pope_align256(n * (S + 1) * 4) : 0;
        skh_cmax = skh ? ns : 0;
        total = 7 * nl + 3 * ns + part + rowp + 2 * colp + pl0 + pl1 + simb + extent + skh_u + skh_v + skh_cmax;
    }
};
}  // namespace

size_t pope_dense_match_workspace_bytes(const pope_dense_match_args* a) {
    if (!a || a->n <= 0 || a->L <= 0 || a->S <= 0 || a->C <= 0) return 0;
    return MatchLayout(*a).total;
}

// One body for both matchers; every check comes before the stream's device is touched: a refused call makes no HIP call
int pope_dense_match_f32(const pope_dense_match_args* args, void* stream) {
    if (!args) return POPE_ERR_ARG;
    const pope_dense_match_args& a = *args;
    if (!a.feat0 || !a.feat1 || !a.b_ids || !a.i_ids || !a.j_ids || !a.mconf || !a.mkpts0_c || !a.mkpts1_c || !a.counts || !a.workspace)
        return POPE_ERR_ARG;
    if (a.n <= 0 || a.L <= 0 || a.S <= 0 || a.C <= 0) return POPE_ERR_ARG;
    if (a.precision != POPE_PREC_F32_MFMA && a.precision != POPE_PREC_F16X3) return POPE_ERR_ARG;
    const bool sinkhorn = a.match_type == POPE_MATCH_SINKHORN;
    if (!sinkhorn && a.match_type != POPE_MATCH_DUAL_SOFTMAX) return POPE_ERR_ARG;
    if (sinkhorn && (!a.bin_score || a.skh_iters < 1)) return POPE_ERR_ARG;
    const MatchLayout lay(a);
    if (a.workspace_bytes < lay.total) return POPE_ERR_WORKSPACE;
    pope_carver ws{static_cast<char*>(a.workspace)};   // (every piece of the layout is a multiple of 256 bytes)
    MatchParams p = {};
    p.feat0 = a.feat0; p.feat1 = a.feat1;
    p.n = a.n; p.L = a.L; p.S = a.S; p.C = a.C;
    p.bs0 = a.stride0; p.bs1 = a.stride1;
    p.h0 = a.h0; p.w0 = a.w0; p.h1 = a.h1; p.w1 = a.w1;
    p.thr = a.thr; p.temperature = sinkhorn ? 1.0f : a.temperature; p.border = a.border_rm; p.scale = a.scale;
    p.publish_conf = a.conf_matrix != nullptr;
    p.ncb = lay.ncb; p.nrb = lay.nrb; p.nrb2 = lay.nrb2; p.ldp = lay.ldp;
    p.row_max = ws.take<float>(lay.nl);
    p.row_sum = ws.take<float>(lay.nl);
    p.conf_rowmax = ws.take<float>(lay.nl);
    p.row_j = ws.take<int>(lay.nl);
    p.row_conf = ws.take<float>(lay.nl);
    p.row_arg = ws.take<int>(lay.nl);
    p.row_cnt = ws.take<int>(lay.nl);
    p.col_max = ws.take<float>(lay.ns);
    p.col_sum = ws.take<float>(lay.ns);
    p.conf_colmax = ws.take<float>(lay.ns);
    p.colmax_part = ws.take<float>(lay.part);
    if (a.precision == POPE_PREC_F16X3) {
        p.row_part = ws.take<float>(lay.rowp);
        p.col_pmax = ws.take<float>(lay.colp);
        p.col_psum = ws.take<float>(lay.colp);
        p.planes0 = ws.take(lay.pl0);
        p.planes1 = ws.take(lay.pl1);
    }
    p.sim = a.conf_matrix ? a.conf_matrix : ws.take<float>(lay.simb);
    if (lay.extent) p.extent = ws.take<int>(lay.extent);
    if (sinkhorn) {
        p.bin_score = a.bin_score; p.skh_iters = a.skh_iters; p.skh_prefilter = a.skh_prefilter;
        p.skh_u = ws.take<float>(lay.skh_u);
        p.skh_v = ws.take<float>(lay.skh_v);
        p.skh_cmax = ws.take<float>(lay.skh_cmax);
    }
    p.counts = a.counts;
    p.range_flag = a.range_flag;
    p.b_ids = a.b_ids; p.i_ids = a.i_ids; p.j_ids = a.j_ids;
    p.mconf = a.mconf; p.mkpts0 = a.mkpts0_c; p.mkpts1 = a.mkpts1_c;
    p.fill0 = a.fill_mask0; p.fill1 = a.fill_mask1;
    p.border0 = a.border_mask0; p.border1 = a.border_mask1;
    p.scale0 = a.scale0; p.scale1 = a.scale1;
    POPE_TRY(pope_match_params_check(p));
    StreamDevice on_device(stream);
    if (sinkhorn) return pope_launch_dense_match_sinkhorn_f32(p, static_cast<hipStream_t>(stream));
    return pope_launch_dense_match_f32(p, static_cast<hipStream_t>(stream));
}

size_t pope_loftr_layer_workspace_bytes(int n, int L, int S, int C, int nhead) {
    if (n <= 0 || L <= 0 || S <= 0 || C <= 0 || nhead <= 0) return 0;
    return pope_loftr_layer_workspace(n, L, S, C, nhead);
}

int pope_loftr_encoder_layer_f32(const pope_loftr_layer_weights* w, float* x, const float* source, const float* x_mask,
                                 const float* source_mask, int n, int L, int S, int C, int nhead, float ln_eps, int attention,
                                 int precision, void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream) {
    if (attention != POPE_LOFTR_ATTN_LINEAR && attention != POPE_LOFTR_ATTN_FULL) return POPE_ERR_ARG;
    if (attention == POPE_LOFTR_ATTN_FULL &&
        (x_mask || source_mask || (C != 256 && C != 128) || nhead != 8 || (precision != POPE_PREC_F32_MFMA && precision != POPE_PREC_F16X3)))
        return POPE_ERR_ARG;
    if (!w || !x || !source || !workspace || n <= 0 || L <= 0 || S <= 0) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    LoftrLayerParams p = {};
    p.x = x; p.source = source; p.n = n; p.L = L; p.S = S; p.C = C; p.H = nhead;
    p.precision = precision;
    if (precision == POPE_PREC_F32_MFMA) {   // the five `*_wp` are then plain fp32 [out, in] matrices
        p.q_w = static_cast<const float*>(w->q_wp); p.kv_w = static_cast<const float*>(w->kv_wp);
        p.merge_w = static_cast<const float*>(w->merge_wp); p.mlp0_w = static_cast<const float*>(w->mlp0_wp);
        p.mlp1_w = static_cast<const float*>(w->mlp1_wp);
    }
    p.q_wp = w->q_wp; p.kv_wp = w->kv_wp; p.merge_wp = w->merge_wp; p.mlp0_wp = w->mlp0_wp; p.mlp1_wp = w->mlp1_wp;
    p.norm1_w = w->norm1_w; p.norm1_b = w->norm1_b; p.norm2_w = w->norm2_w; p.norm2_b = w->norm2_b;
    p.ln_eps = ln_eps; p.ws = workspace; p.ws_bytes = workspace_bytes; p.range_flag = range_flag;
    p.x_mask = x_mask; p.source_mask = source_mask;
    p.attention = attention;
    return pope_launch_loftr_layer(p, static_cast<hipStream_t>(stream));
}

int pope_loftr_full_attention_f32(const float* q, const float* kv, int n, int L, int S, int C, int nhead, int precision, float* out,
                                  unsigned* range_flag, void* stream) {
    if (precision != POPE_PREC_F32_MFMA && precision != POPE_PREC_F16X3) return POPE_ERR_ARG;
    POPE_TRY(pope_loftr_full_attention_check(q, kv, n, L, S, C, nhead, out));
    StreamDevice on_device(stream);
    // both precisions run the fp32-MFMA kernel (small sequences: fp32 FMAs); range_flag is not touched with fp32 rows out
    return pope_launch_loftr_full_attention(q, kv, n, L, S, C, nhead, false, out, range_flag, static_cast<hipStream_t>(stream));
}

size_t pope_loftr_linear_attention_workspace_bytes(int n, int S, int C, int nhead) {
    return pope_loftr_linear_attention_workspace(n, S, C, nhead);
}

void pope_loftr_linear_attention_seams(int* chunk_rows, int* rows_per_block) { pope_loftr_linattn_seams(chunk_rows, rows_per_block); }

int pope_loftr_linear_attention_f32(const float* q, const float* kv, const float* x_mask, const float* source_mask, int n, int L, int S,
                                    int C, int nhead, float* out_f32, void* out_planes, void* workspace, size_t workspace_bytes,
                                    unsigned* range_flag, void* stream) {
    // checked before the stream's device is touched: a refused call makes no HIP call
    POPE_TRY(pope_loftr_linear_attention_check(q, kv, n, L, S, C, nhead, out_f32, out_planes, workspace, workspace_bytes));
    StreamDevice on_device(stream);
    return pope_launch_loftr_linear_attention(q, kv, x_mask, source_mask, n, L, S, C, nhead, out_f32, out_planes, workspace, workspace_bytes,
                                              range_flag, static_cast<hipStream_t>(stream));
}

// one layer of the ResNet-FPN forward (or the SAM neck's 3 x 3) through the layer functions the models call (conv_layer.h);
// checked before the stream's device is touched
size_t pope_conv_layer_scratch_bytes(int form, int n, int H, int W, int cch, int taps) {
    return pope_conv_layer_scratch(form, n, H, W, cch, taps);
}

int pope_conv_layer_f32(const pope_conv_layer_args* args, void* stream) {
    if (!args) return POPE_ERR_ARG;
    if (const int rc = pope_conv_layer_check(*args)) return rc;
    StreamDevice on_device(stream);
    return pope_launch_conv_layer(*args, false, static_cast<hipStream_t>(stream));
}

int pope_conv_layer_f16(const pope_conv_layer_args* args, void* stream) {
    if (!args) return POPE_ERR_ARG;
    if (const int rc = pope_conv_layer_f16_check(*args)) return rc;
    StreamDevice on_device(stream);
    return pope_launch_conv_layer(*args, true, static_cast<hipStream_t>(stream));
}

size_t pope_resnetfpn_workspace_bytes(int n, int H, int W) {
    if (n <= 0 || H < 16 || W < 16 || (H & 7) || (W & 7)) return 0;
    return pope_resnetfpn_workspace(n, H, W);
}

int pope_resnetfpn_forward_f32(const pope_resnetfpn_weights* w, const float* gray, int n, int H, int W, int precision, float* out_c,
                               float* out_f, void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream) {
    StreamDevice on_device(stream);
    if (!w) return POPE_ERR_ARG;
    ResnetFpnParams q = {};
    q.img = gray; q.n = n; q.H = H; q.W = W;
    q.precision = precision;
    for (int i = 0; i < 22; ++i) { q.w[i] = w->w[i]; q.b[i] = w->b[i]; q.wf[i] = static_cast<const float*>(w->w[i]); }
    q.out_c = out_c; q.out_f = out_f; q.ws = workspace; q.ws_bytes = workspace_bytes; q.range_flag = range_flag;
    return pope_launch_resnetfpn(q, static_cast<hipStream_t>(stream));
}

size_t pope_fine_preprocess_workspace_bytes(int M, int Wn, int Cc, int Cf) {
    if (M <= 0 || Wn <= 0 || Cc <= 0 || Cf <= 0) return 0;
    return pope_fine_preprocess_workspace(M, Wn * Wn, Cc, Cf);
}

int pope_fine_preprocess_f32(const float* feat_f0, const long long* strides0, int H0, int W0, int wc0, const float* feat_f1,
                             const long long* strides1, int H1, int W1, int wc1, const float* feat_c0, const float* feat_c1, int L,
                             int S, int Cc, int Cf, const long long* b_ids, const long long* i_ids, const long long* j_ids, int M,
                             int Wn, int stride, const void* down_wp, const float* down_b, const void* merge_wp,
                             const float* merge_b, int precision, float* out, void* workspace, size_t workspace_bytes,
                             unsigned* range_flag, const long long* ref0_of_pair, int n, int n0, void* stream) {
    // the checks that need no device come first: a bad call returns before any HIP call
    if (n < 0 || n0 < 0 || (ref0_of_pair && (n == 0 || n0 == 0))) return POPE_ERR_ARG;
    if (!feat_f0 || !feat_f1 || !feat_c0 || !feat_c1 || !b_ids || !i_ids || !j_ids || !down_wp || !merge_wp || !out || !workspace)
        return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    if (!strides0 || !strides1 || H0 <= 0 || W0 <= 0 || H1 <= 0 || W1 <= 0 || wc0 <= 0 || wc1 <= 0 || L <= 0 || S <= 0) return POPE_ERR_ARG;
    FinePreParams q = {};
    q.ref0_of_pair = ref0_of_pair; q.n_pairs = n; q.n0 = n0;
    q.f0 = feat_f0; q.f1 = feat_f1;
    for (int i = 0; i < 4; ++i) { q.s0[i] = strides0[i]; q.s1[i] = strides1[i]; }
    q.H0 = H0; q.W0 = W0; q.H1 = H1; q.W1 = W1; q.wc0 = wc0; q.wc1 = wc1;
    q.fc0 = feat_c0; q.fc1 = feat_c1; q.L = L; q.S = S; q.Cc = Cc; q.Cf = Cf;
    q.b_ids = b_ids; q.i_ids = i_ids; q.j_ids = j_ids; q.M = M; q.Wn = Wn; q.stride = stride;
    q.down_wp = down_wp; q.down_b = down_b; q.merge_wp = merge_wp; q.merge_b = merge_b;
    q.precision = precision;
    q.down_w = static_cast<const float*>(down_wp); q.merge_w = static_cast<const float*>(merge_wp);
    q.out = out; q.ws = workspace; q.ws_bytes = workspace_bytes; q.range_flag = range_flag;
    return pope_launch_fine_preprocess(q, static_cast<hipStream_t>(stream));
}

int pope_fine_match_f32(const float* win0, const float* win1, int M, int Wn, int C, const float* mkpts1_c, float scale_px,
                        const float* scale1, const long long* b_ids, float* expec_f, float* mkpts1_f, void* stream) {
    if (!win0 || !win1 || !mkpts1_c || !expec_f || !mkpts1_f || (scale1 && !b_ids) || M <= 0 || Wn <= 0 || Wn * Wn > 64 || C <= 0)
        return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_fine_match_scaled(win0, win1, M, Wn, C, mkpts1_c, scale_px, scale1, b_ids, expec_f, mkpts1_f,
                                         static_cast<hipStream_t>(stream));
}

size_t pope_sam_encoder_workspace_bytes(const pope_sam_encoder_weights* w, int B) { return pope_sam_encoder_workspace(w, B); }

int pope_sam_encoder_forward_f32(const pope_sam_encoder_weights* w, const float* image, int B, float* out, int n_taps,
                                 const int* tap_blocks_host, float* const* tap_out_host, void* workspace, size_t workspace_bytes,
                                 unsigned* range_flag, void* stream) {
    StreamDevice on_device(stream);
    SamEncArgs a{};
    a.w = w; a.image = image; a.out = out; a.B = B;
    a.n_taps = n_taps; a.tap_blocks = tap_blocks_host; a.tap_out = tap_out_host;
    a.ws = workspace; a.ws_bytes = workspace_bytes; a.range_flag = range_flag;
    return pope_launch_sam_encoder(a, static_cast<hipStream_t>(stream));
}

size_t pope_sam_decoder_workspace_bytes(const pope_sam_decoder_weights* w, int P, int n_sparse, int shared) {
    return pope_sam_decoder_workspace(w, P, n_sparse, shared);
}

int pope_sam_decoder_forward_f32(const pope_sam_decoder_weights* w, const float* image, const float* image_pe, const float* sparse,
                                 int P, int n_sparse, const float* dense, long long dense_stride, int multimask, float* masks,
                                 float* iou, float* hs_out, float* keys_out, void* workspace, size_t workspace_bytes,
                                 unsigned* range_flag, void* stream) {
    SamDecArgs a{};
    a.w = w; a.image = image; a.image_pe = image_pe; a.sparse = sparse; a.dense = dense;
    a.P = P; a.n_sparse = n_sparse; a.multimask = multimask; a.dense_stride = dense_stride;
    a.masks = masks; a.iou = iou; a.hs_out = hs_out; a.keys_out = keys_out;
    a.ws = workspace; a.ws_bytes = workspace_bytes; a.range_flag = range_flag;
    if (pope_sam_decoder_workspace(w, P, n_sparse, dense_stride == 0) == 0) return POPE_ERR_ARG;   // before any HIP call
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder(a, static_cast<hipStream_t>(stream));
}

size_t pope_sam_decoder_images_workspace_bytes(const pope_sam_decoder_weights* w, int N, const int* prompt_image_host, int P,
                                               int n_sparse, long long dense_stride) {
    return pope_sam_decoder_images_workspace(w, N, prompt_image_host, P, n_sparse, dense_stride);
}

int pope_sam_decoder_forward_images_f32(const pope_sam_decoder_weights* w, const float* images, int N, const float* image_pe,
                                        const float* sparse, const int* prompt_image_host, int P, int n_sparse, const float* dense,
                                        long long dense_stride, int multimask, float* masks, float* iou, void* workspace,
                                        size_t workspace_bytes, unsigned* range_flag, void* stream) {
    SamDecArgs a{};
    a.w = w; a.image = images; a.image_pe = image_pe; a.sparse = sparse; a.dense = dense;
    a.P = P; a.n_sparse = n_sparse; a.multimask = multimask; a.dense_stride = dense_stride;
    a.n_images = N; a.prompt_image = prompt_image_host;
    a.masks = masks; a.iou = iou;
    a.ws = workspace; a.ws_bytes = workspace_bytes; a.range_flag = range_flag;
    // before any HIP call: the images, their count, every prompt's image index and the broadcast
    if (!images || pope_sam_decoder_images_workspace(w, N, prompt_image_host, P, n_sparse, dense_stride) == 0) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder(a, static_cast<hipStream_t>(stream));
}

// the decoder's kernels one at a time: the launchers check every argument before their launch
void pope_sam_decoder_seams(int* chunk, int* lin_rows, int* max_tokens, int* base_tokens) {
    pope_sam_decoder_seam_values(chunk, lin_rows, max_tokens, base_tokens);
}

int pope_sam_decoder_token_linear_f32(const float* X, int ldx, const float* add, int add_cols, const float* W, const float* bias,
                                      const float* res, float* Y, int ldy, int M, int N, int K, int relu, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder_token_linear(X, ldx, add, add_cols, W, bias, res, Y, ldy, M, N, K, relu, static_cast<hipStream_t>(stream));
}

int pope_sam_decoder_self_attention_f32(const float* qkv, float* out, int P, int T, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder_self_attention(qkv, out, P, T, static_cast<hipStream_t>(stream));
}

int pope_sam_decoder_t2i_attention_f32(const float* q, const float* K, int ldk, long long kps, const float* V, long long vps,
                                       const int* slot_host, float* out, int T, int P, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder_t2i_attention(q, K, ldk, kps, V, vps, slot_host, out, T, P, static_cast<hipStream_t>(stream));
}

int pope_sam_decoder_i2t_attention_f32(const float* Q, long long qps, const int* slot_host, const float* kv, int T, int P,
                                       float* out_f32, void* out_planes, unsigned* range_flag, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder_i2t_attention(Q, qps, slot_host, kv, T, P, out_f32, out_planes, range_flag,
                                                 static_cast<hipStream_t>(stream));
}

int pope_sam_decoder_residual_norm_f32(const float* res, long long rps, const int* slot_host, const float* y, const float* w,
                                       const float* b, float eps, const float* pe_t, float* keys, void* opA, void* opB, int f32, int P,
                                       unsigned* range_flag, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder_residual_norm(res, rps, slot_host, y, w, b, eps, pe_t, keys, opA, opB, f32, P, range_flag,
                                                 static_cast<hipStream_t>(stream));
}

int pope_sam_decoder_prepare_keys_f32(const float* image, long long image_stride, const float* image_pe, const float* dense,
                                      long long dense_stride, int nz, float* keys, void* opA, void* opB, int f32, float* pe_t,
                                      unsigned* range_flag, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder_prepare_keys(image, image_stride, image_pe, dense, dense_stride, nz, keys, opA, opB, f32, pe_t,
                                                range_flag, static_cast<hipStream_t>(stream));
}

int pope_sam_decoder_upscale_tail_f32(const float* y, const float* ln_w, const float* ln_b, float eps, const float* w2, const float* b2,
                                      const float* hyper, int multimask, int P, float* masks, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_decoder_upscale_tail(y, ln_w, ln_b, eps, w2, b2, hyper, multimask, P, masks, static_cast<hipStream_t>(stream));
}

int pope_sam_mask_embed_f32(const pope_sam_mask_embed_weights* w, const float* masks, int P, float* dense, void* stream) {
    if (const int rc = pope_sam_mask_embed_check(w, masks, P, dense)) return rc;   // before any HIP call
    StreamDevice on_device(stream);
    return pope_launch_sam_mask_embed(w, masks, P, dense, static_cast<hipStream_t>(stream));
}

size_t pope_sam_postprocess_workspace_bytes(int img_size, int H, int W) { return pope_sam_postprocess_workspace(img_size, H, W); }

int pope_sam_postprocess_f32(const float* low_res, int M, int h, int w, const int* selection, int n_sel, int img_size, int ih, int iw,
                             int H, int W, double mask_threshold, double stability_offset, int* stats, unsigned* packed,
                             float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    SamPostArgs a{};
    a.low = low_res; a.M = M; a.h = h; a.w = w; a.sel = selection; a.n_sel = n_sel;
    a.img = img_size; a.ih = ih; a.iw = iw; a.H = H; a.W = W;
    a.mask_threshold = mask_threshold; a.stability_offset = stability_offset;
    a.stats = stats; a.packed = packed; a.logits = logits; a.ws = workspace; a.ws_bytes = workspace_bytes;
    StreamDevice on_device(stream);
    return pope_launch_sam_postprocess(a, static_cast<hipStream_t>(stream));
}

int pope_sam_nms_f32(const float* boxes, const float* scores, int n, float iou_threshold, int* keep, int* count, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_sam_nms(boxes, scores, n, iou_threshold, keep, count, static_cast<hipStream_t>(stream));
}

int pope_sam_nms_segments_f32(const float* boxes, const float* scores, const int* seg_offsets, int S, int n, float iou_threshold,
                              int* keep, int* count, void* stream) {
    if (S < 0 || n < 0 || (S > 0 && (!seg_offsets || !count)) || (S > 0 && n > 0 && (!boxes || !scores || !keep))) return POPE_ERR_ARG;
    if (S == 0) return POPE_OK;      // before any HIP call
    StreamDevice on_device(stream);
    return pope_launch_sam_nms_segments(boxes, scores, seg_offsets, S, n, iou_threshold, keep, count, static_cast<hipStream_t>(stream));
}

size_t pope_sam_small_regions_workspace_bytes(int n, int H, int W) { return pope_sam_small_regions_workspace(n, H, W); }

int pope_sam_small_regions_u32(const unsigned* packed, int n, int H, int W, int min_area, unsigned* packed_out, int* unchanged,
                               int* boxes, int* area, void* workspace, size_t workspace_bytes, void* stream) {
    SamRegionsArgs a{};
    a.packed = packed; a.n = n; a.H = H; a.W = W; a.min_area = min_area;
    a.packed_out = packed_out; a.unchanged = unchanged; a.boxes = boxes; a.area = area; a.ws = workspace; a.ws_bytes = workspace_bytes;
    if (const int rc = pope_sam_small_regions_check(a)) return rc;   // before any HIP call
    if (n == 0) return POPE_OK;
    StreamDevice on_device(stream);
    return pope_launch_sam_small_regions(a, static_cast<hipStream_t>(stream));
}

int pope_sam_rle_u32(const unsigned* packed, int n, int H, int W, int* lengths, const long long* offsets, unsigned* counts,
                     long long capacity, void* stream) {
    SamRleArgs a{};
    a.packed = packed; a.n = n; a.H = H; a.W = W; a.lengths = lengths; a.offsets = offsets; a.counts = counts; a.capacity = capacity;
    if (const int rc = pope_sam_rle_check(a)) return rc;   // before any HIP call
    if (n == 0) return POPE_OK;
    StreamDevice on_device(stream);
    return pope_launch_sam_rle(a, static_cast<hipStream_t>(stream));
}

int pope_preprocess_u8_f32(const unsigned char* img_hwc, int P, int Hin, int Win, const int* hstart, const int* hcount,
                           const int* hk, int kh, const int* vstart, const int* vcount, const int* vk, int kv, int top, int left,
                           int ch, int cw, int row0, int nrows, const float* mean_host, const float* std_host, float* out,
                           unsigned char* scratch, size_t scratch_bytes, void* stream) {
    StreamDevice on_device(stream);
    if (!mean_host || !std_host || P <= 0 || nrows <= 0 || cw <= 0) return POPE_ERR_ARG;
    if (scratch_bytes < size_t(P) * nrows * cw * 3) return POPE_ERR_WORKSPACE;
    PreprocParams p = {};
    p.img = img_hwc; p.P = P; p.Hin = Hin; p.Win = Win;
    p.hstart = hstart; p.hcount = hcount; p.hk = hk; p.kh = kh;
    p.vstart = vstart; p.vcount = vcount; p.vk = vk; p.kv = kv;
    p.top = top; p.left = left; p.ch = ch; p.cw = cw; p.row0 = row0; p.nrows = nrows;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean_host[c]; p.std[c] = std_host[c]; }
    p.tmp = scratch; p.out = out;
    return pope_launch_preprocess(p, static_cast<hipStream_t>(stream));
}

namespace {
// the arguments both whole-frame resample entries share
ResizeParams resize_params(const unsigned char* img_hwc, int P, int Hin, int Win, const int* hstart, const int* hcount, const int* hk,
                           int kh, const int* vstart, const int* vcount, const int* vk, int kv, int OH, int OW, void* out,
                           unsigned char* scratch, size_t scratch_bytes) {
    ResizeParams p = {};
    p.img = img_hwc; p.P = P; p.Hin = Hin; p.Win = Win;
    p.hstart = hstart; p.hcount = hcount; p.hk = hk; p.kh = kh;
    p.vstart = vstart; p.vcount = vcount; p.vk = vk; p.kv = kv;
    p.OH = OH; p.OW = OW; p.out = out; p.tmp = scratch; p.tmp_bytes = scratch_bytes;
    return p;
}
}  // namespace

int pope_resize_u8(const unsigned char* img_hwc, int P, int Hin, int Win, const int* hstart, const int* hcount, const int* hk, int kh,
                   const int* vstart, const int* vcount, const int* vk, int kv, int OH, int OW, unsigned char* out,
                   unsigned char* scratch, size_t scratch_bytes, void* stream) {
    const ResizeParams p = resize_params(img_hwc, P, Hin, Win, hstart, hcount, hk, kh, vstart, vcount, vk, kv, OH, OW, out, scratch,
                                         scratch_bytes);
    if (const int rc = pope_resize_check(p)) return rc;   // before any HIP call
    StreamDevice on_device(stream);
    return pope_launch_resize(p, static_cast<hipStream_t>(stream));
}

int pope_sam_preprocess_u8_f32(const unsigned char* img_hwc, int P, int Hin, int Win, const int* hstart, const int* hcount,
                               const int* hk, int kh, const int* vstart, const int* vcount, const int* vk, int kv, int OH, int OW,
                               int S, int flip, const float* mean_host, const float* std_host, float* out, unsigned char* scratch,
                               size_t scratch_bytes, void* stream) {
    if (!mean_host || !std_host) return POPE_ERR_ARG;
    ResizeParams p = resize_params(img_hwc, P, Hin, Win, hstart, hcount, hk, kh, vstart, vcount, vk, kv, OH, OW, out, scratch,
                                   scratch_bytes);
    p.f32 = true; p.S = S; p.flip = flip;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean_host[c]; p.std[c] = std_host[c]; }
    if (const int rc = pope_resize_check(p)) return rc;   // before any HIP call
    StreamDevice on_device(stream);
    return pope_launch_resize(p, static_cast<hipStream_t>(stream));
}

int pope_crop_normalize_u8_f32(const unsigned char* img_hwc, int P, int Hin, int Win, int top, int left, int ch, int cw,
                               const float* mean_host, const float* std_host, float* out, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_crop_norm(img_hwc, P, Hin, Win, top, left, ch, cw, mean_host, std_host, out, static_cast<hipStream_t>(stream));
}

int pope_gray_u8_f32(const unsigned char* bgr_hwc, int P, int H, int W, float* out, void* stream) {
    StreamDevice on_device(stream);
    if (P <= 0 || H <= 0 || W <= 0) return POPE_ERR_ARG;
    return pope_launch_gray(bgr_hwc, size_t(P) * H * W, out, static_cast<hipStream_t>(stream));
}

int pope_pose_images_u8_f32(const unsigned char* src_hwc, int P, int Hin, int Win, const int* rows, int Q, const int* xstart,
                            const int* xcoef, const int* ystart, const int* ycoef, int OH, int OW, int transposed, float* out,
                            void* stream) {
    PoseImagesParams p = {};
    p.src = src_hwc; p.P = P; p.Hin = Hin; p.Win = Win; p.rows = rows; p.Q = Q;
    p.xstart = xstart; p.xcoef = xcoef; p.ystart = ystart; p.ycoef = ycoef;
    p.OH = OH; p.OW = OW; p.transposed = transposed; p.out = out;
    if (const int rc = pope_pose_images_check(p)) return rc;   // before any HIP call
    if (Q == 0) return POPE_OK;
    StreamDevice on_device(stream);
    return pope_launch_pose_images(p, static_cast<hipStream_t>(stream));
}

int pope_crop_warp_u8(const unsigned char* img_hwc, int H, int W, int C, const double* minv, const int* win, int P, int oh, int ow,
                      unsigned char* out, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_crop_warp(img_hwc, H, W, C, minv, win, P, oh, ow, out, static_cast<hipStream_t>(stream));
}

int pope_streaming_top3_host(const float* scores, int P, float* slot_scores, long long* slot_index) {
    if (!scores || !slot_scores || !slot_index || P < 0) return POPE_ERR_ARG;
    for (int k = 0; k < 3; ++k) { slot_scores[k] = 0.f; slot_index[k] = -1; }
    for (int p = 0; p < P; ++p) {
        const float s = scores[p];
        if (s > slot_scores[0] || s > slot_scores[1] || s > slot_scores[2]) {
            int k = 0;  // np.argmin: first minimum
            if (slot_scores[1] < slot_scores[k]) k = 1;
            if (slot_scores[2] < slot_scores[k]) k = 2;
            slot_scores[k] = s;
            slot_index[k] = p;
        }
    }
    return POPE_OK;
}

int pope_vote_top3_batch_f32(const float* cls_ref, const float* cls_prop, const int* seg, int Q, int N, int D, float eps,
                             float* scores, float* slot_scores, long long* slot_index, int* pair_row, unsigned char* pair_live,
                             void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_vote_top3_batch(cls_ref, cls_prop, seg, Q, N, D, eps, scores, slot_scores, slot_index, pair_row, pair_live,
                                       static_cast<hipStream_t>(stream));
}

int pope_vote_top3_shared_f32(const float* cls_ref, const float* cls_prop, const int* seg, int S, const int* query_seg,
                              const int* score_begin, int Q, int N, int D, float eps, float* scores, float* slot_scores,
                              long long* slot_index, int* pair_row, unsigned char* pair_live, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_vote_top3_shared(cls_ref, cls_prop, seg, S, query_seg, score_begin, Q, N, D, eps, scores, slot_scores,
                                        slot_index, pair_row, pair_live, static_cast<hipStream_t>(stream));
}

int pope_slot_tally_f32(const long long* m_bids, const float* mconf, const float* mkpts0_f, const float* mkpts1_f,
                        const unsigned char* pair_live, int Q, long long M, float conf_thr, int* pair_begin, int* pair_count,
                        long long* matching_score, int* best_slot, int* best_count, float* best_kpts0, float* best_kpts1,
                        void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_slot_tally(m_bids, mconf, mkpts0_f, mkpts1_f, pair_live, Q, M, conf_thr, pair_begin, pair_count,
                                  matching_score, best_slot, best_count, best_kpts0, best_kpts1, static_cast<hipStream_t>(stream));
}

}  // extern "C"

size_t pope_estimate_pose_workspace_bytes(int B, long long M) { return pope_pose_workspace(B, M); }

int pope_estimate_pose_f64(const float* kpts0, const float* kpts1, const int* counts, const double* K0, const double* K1, int B,
                           long long M, double thresh, double conf, int max_iters, unsigned long long seed, double* R, double* t,
                           double* E, unsigned char* inliers, int* info, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_device(stream);
    PoseParams q = {};
    q.kpts0 = kpts0; q.kpts1 = kpts1; q.counts = counts; q.K0 = K0; q.K1 = K1; q.B = B; q.M = M;
    q.thresh = thresh; q.conf = conf; q.max_iters = max_iters; q.seed = seed;
    q.R = R; q.t = t; q.E = E; q.inliers = inliers; q.info = info;
    return pope_launch_estimate_pose(q, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

// ---- learned pose regressor (pose_regressor.hip) ---------------------------------------------------------------------------

namespace {

struct PoseRegWorkspace { size_t x, index, y1, y2, total; };
PoseRegWorkspace posereg_layout(int B, int S) {
    PoseRegWorkspace l;
    const size_t b = size_t(B), s = size_t(S);
    l.x = pope_align256(b * s * 76 * sizeof(float));
    l.index = pope_align256(b * s * sizeof(int));
    l.y1 = pope_align256(b * s * 19 * sizeof(float));
    l.y2 = pope_align256(b * s * sizeof(float));
    l.total = l.x + l.index + l.y1 + l.y2;
    return l;
}

bool posereg_weights_ok(const pope_pose_regressor_weights* w, int S) {
    if (!w || w->num_sample != S || w->mode < POPE_ROT_MATRIX || w->mode > POPE_ROT_6D) return false;
    uintptr_t bits = 0;
    bool all = true;
    auto see = [&](const float* p) { all = all && p; bits |= reinterpret_cast<uintptr_t>(p); };
    for (const pope_pose_regressor_layer& l : w->layers)
        for (const float* p : {l.in_proj_w, l.in_proj_b, l.out_proj_w, l.out_proj_b, l.linear1_w, l.linear1_b, l.linear2_w, l.linear2_b,
                               l.norm1_w, l.norm1_b, l.norm2_w, l.norm2_b}) see(p);
    for (int i = 0; i < 7; ++i) { see(w->mlp_w[i]); see(w->mlp_b[i]); }
    for (const float* p : {w->trans_w, w->trans_b, w->rot_w, w->rot_b}) see(p);
    return all && !(bits & 15);
}

PoseRegInput posereg_input(const float* dense0, const float* dense1, const float* kpts0, const float* kpts1, const int* counts,
                           const int* sample_index, const unsigned long long* seeds, int B, int S, long long M) {
    PoseRegInput in = {};
    in.dense0 = dense0; in.dense1 = dense1; in.kpts0 = kpts0; in.kpts1 = kpts1; in.counts = counts; in.sample_index = sample_index;
    in.seeds = seeds; in.B = B; in.S = S; in.M = M;
    return in;
}

int posereg_encoder(const pope_pose_regressor_weights* w, const PoseRegInput& in, int G, float* X, int* index, int* status,
                    hipStream_t stream) {
    POPE_TRY(pope_launch_posereg_embed(in, X, index, status, stream));
    for (const pope_pose_regressor_layer& l : w->layers) POPE_TRY(pope_launch_posereg_layer(l, X, in.B, in.S, G, stream));
    return POPE_OK;
}

}  // namespace

size_t pope_pose_regressor_workspace_bytes(int B, int S) { return B > 0 && S > 0 ? posereg_layout(B, S).total : 0; }

int pope_pose_regressor_embedding_f32(const float* dense0, const float* dense1, const float* kpts0, const float* kpts1,
                                      const int* counts, const int* sample_index, const unsigned long long* seeds, int B, int S,
                                      long long M, float* x_out, int* index_out, int* status, void* stream) {
    const PoseRegInput in = posereg_input(dense0, dense1, kpts0, kpts1, counts, sample_index, seeds, B, S, M);
    POPE_TRY(pope_posereg_input_check(in));
    if (!x_out || !index_out || !status) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_posereg_embed(in, x_out, index_out, status, static_cast<hipStream_t>(stream));
}

int pope_pose_regressor_encoder_f32(const pope_pose_regressor_weights* w, const float* dense0, const float* dense1,
                                    const float* kpts0, const float* kpts1, const int* counts, const int* sample_index,
                                    const unsigned long long* seeds, int B, int S, int G, long long M, float* x_out,
                                    int* index_out, int* status, void* stream) {
    const PoseRegInput in = posereg_input(dense0, dense1, kpts0, kpts1, counts, sample_index, seeds, B, S, M);
    POPE_TRY(pope_posereg_input_check(in));
    if (!posereg_weights_ok(w, S) || !x_out || !index_out || !status || G < 1 || G > 64 || B % G) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return posereg_encoder(w, in, G, x_out, index_out, status, static_cast<hipStream_t>(stream));
}

int pope_pose_regressor_forward_f32(const pope_pose_regressor_weights* w, const float* dense0, const float* dense1,
                                    const float* kpts0, const float* kpts1, const int* counts, const int* sample_index,
                                    const unsigned long long* seeds, int B, int S, int G, long long M, float* trans, float* rot,
                                    int* status, void* workspace, size_t workspace_bytes, void* stream) {
    const PoseRegInput in = posereg_input(dense0, dense1, kpts0, kpts1, counts, sample_index, seeds, B, S, M);
    POPE_TRY(pope_posereg_input_check(in));
    if (!posereg_weights_ok(w, S) || !trans || !rot || !status || G < 1 || G > 64 || B % G) return POPE_ERR_ARG;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) return POPE_ERR_ARG;
    const PoseRegWorkspace lay = posereg_layout(B, S);
    if (workspace_bytes < lay.total) return POPE_ERR_WORKSPACE;
    StreamDevice on_device(stream);
    hipStream_t st = static_cast<hipStream_t>(stream);
    pope_carver ws{static_cast<char*>(workspace)};
    float* X = ws.take<float>(lay.x);
    int* index = ws.take<int>(lay.index);
    float* y1 = ws.take<float>(lay.y1);
    float* y2 = ws.take<float>(lay.y2);
    POPE_TRY(posereg_encoder(w, in, G, X, index, status, st));
    POPE_TRY(pope_launch_posereg_stream_linear(X, w->mlp_w[0], w->mlp_b[0], y1, B, 76ll * S, 19 * S, st));
    POPE_TRY(pope_launch_posereg_stream_linear(y1, w->mlp_w[1], w->mlp_b[1], y2, B, 19ll * S, S, st));
    return pope_launch_posereg_tail(*w, y2, status, B, trans, rot, st);
}

// the launches of the forward one by one (tests)
int pope_pose_regressor_layer_f32(const pope_pose_regressor_layer* w, float* X, int B, int S, int G, void* stream) {
    if (!w || !X || B <= 0 || S <= 0 || G < 1 || G > 64 || B % G) return POPE_ERR_ARG;
    if (size_t(B) * S * 76 >= (size_t(1) << 31)) return POPE_ERR_ARG;
    uintptr_t bits = 0;
    for (const float* p : {w->in_proj_w, w->in_proj_b, w->out_proj_w, w->out_proj_b, w->linear1_w, w->linear1_b, w->linear2_w, w->linear2_b,
                           w->norm1_w, w->norm1_b, w->norm2_w, w->norm2_b}) {
        if (!p) return POPE_ERR_ARG;
        bits |= reinterpret_cast<uintptr_t>(p);
    }
    if (bits & 15) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_posereg_layer(*w, X, B, S, G, static_cast<hipStream_t>(stream));
}

int pope_pose_regressor_stream_linear_f32(const float* A, const float* W, const float* bias, float* Y, int B, long long K, int N,
                                          void* stream) {
    if (!A || !W || !bias || !Y || B <= 0 || K <= 0 || N <= 0) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_posereg_stream_linear(A, W, bias, Y, B, K, N, static_cast<hipStream_t>(stream));
}

int pope_pose_regressor_tail_f32(const pope_pose_regressor_weights* w, const float* Y2, const int* status, int B, float* trans,
                                 float* rot, void* stream) {
    if (!w || !Y2 || !status || !trans || !rot || B <= 0 || w->num_sample <= 0) return POPE_ERR_ARG;
    if (w->mode < POPE_ROT_MATRIX || w->mode > POPE_ROT_6D) return POPE_ERR_ARG;
    for (int i = 2; i < 7; ++i)
        if (!w->mlp_w[i] || !w->mlp_b[i]) return POPE_ERR_ARG;
    if (!w->trans_w || !w->trans_b || !w->rot_w || !w->rot_b) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_posereg_tail(*w, Y2, status, B, trans, rot, static_cast<hipStream_t>(stream));
}

// ---- ConvNeXtV2 backbone and the image pose head (convnext.hip) ------------------------------------------------------------

size_t pope_convnext_workspace_bytes(const pope_convnext_weights* w, int B, int H, int W) { return pope_convnext_workspace(w, B, H, W); }

int pope_convnext_forward_f32(const pope_convnext_weights* w, const float* image, int B, int H, int W, int precision,
                              float* features_out, float* logits_out, float* const* taps, void* workspace,
                              size_t workspace_bytes, unsigned* range_flag, void* stream) {
    ConvNextArgs a = {};
    a.w = w; a.image = image; a.B = B; a.H = H; a.W = W; a.precision = precision; a.features = features_out; a.logits = logits_out;
    a.taps = taps; a.ws = workspace; a.ws_bytes = workspace_bytes; a.range_flag = range_flag;
    POPE_TRY(pope_convnext_check(a));
    StreamDevice on_device(stream);
    return pope_launch_convnext(a, static_cast<hipStream_t>(stream));
}

int pope_convnext_dwconv_f32(const float* x, const float* w49, const float* bias, float* y, int B, int H, int W, int C,
                             void* stream) {
    if (!x || !w49 || !bias || !y || x == y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_convnext_dwconv(x, w49, bias, y, B, H, W, C, static_cast<hipStream_t>(stream));
}

size_t pope_convnext_grn_workspace_bytes(int B, int HW, int C) { return pope_convnext_grn_workspace(B, HW, C); }

int pope_convnext_grn_f32(const float* x, const float* gamma, const float* beta, int B, int HW, int C, float* y_f32,
                          void* y_planes, void* workspace, size_t workspace_bytes, unsigned* range_flag, void* stream) {
    POPE_TRY(pope_convnext_grn_check(x, gamma, beta, B, HW, C, y_f32, y_planes, workspace, workspace_bytes));
    StreamDevice on_device(stream);
    return pope_launch_convnext_grn(x, gamma, beta, B, HW, C, y_f32, y_planes, workspace, range_flag, static_cast<hipStream_t>(stream));
}

int pope_convnext_pose_heads_f32(const float* feat, const float* trans_w, const float* trans_b, const float* rot_w,
                                 const float* rot_b, int mode, int B, int inner, float* trans, float* rot, void* stream) {
    if (!feat || !trans_w || !trans_b || !rot_w || !rot_b || !trans || !rot || B <= 0 || inner <= 0 || inner > 256 ||
        mode < POPE_ROT_MATRIX || mode > POPE_ROT_6D)
        return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_convnext_pose_heads(feat, trans_w, trans_b, rot_w, rot_b, mode, B, inner, trans, rot, static_cast<hipStream_t>(stream));
}

int pope_five_point_f64(const double* x0, const double* x1, int S, double* E_out, int* n_out, void* stream) {
    StreamDevice on_device(stream);
    return pope_launch_five_point(x0, x1, S, E_out, n_out, static_cast<hipStream_t>(stream));
}

// ---- Vision Mamba backbone (vim.hip) ------------------------------------------------------------------------------------------

size_t pope_vim_workspace_bytes(const pope_vim_weights* w, int B) { return pope_vim_workspace(w, B); }

int pope_vim_forward_f32(const pope_vim_weights* w, const float* image, int B, int precision, void* workspace, size_t workspace_bytes,
                         float* features, float* logits, float* const* taps, unsigned* range_flag, void* stream) {
    VimArgs a = {};
    a.w = w; a.image = image; a.B = B; a.precision = precision; a.features = features; a.logits = logits; a.taps = taps;
    a.ws = workspace; a.ws_bytes = workspace_bytes; a.range_flag = range_flag;
    POPE_TRY(pope_vim_check(a));
    StreamDevice on_device(stream);
    return pope_launch_vim(a, static_cast<hipStream_t>(stream));
}

int pope_vim_scan_chunk(void) { return pope_vim_scan_chunk_len(); }

size_t pope_vim_scan_workspace_bytes(int B, int L, int E) { return pope_vim_scan_workspace(B, L, E); }

int pope_vim_scan_f32(const float* xc, const float* z, int ldz, const float* xdbl, const pope_vim_dir_weights* dirs, int B, int L, int E,
                      int R, float* out_f32, void* out_planes, void* workspace, size_t workspace_bytes, unsigned* range_flag,
                      void* stream) {
    POPE_TRY(pope_vim_scan_check(xc, z, ldz, xdbl, dirs, B, L, E, R, out_f32, out_planes, workspace, workspace_bytes));
    StreamDevice on_device(stream);
    return pope_launch_vim_scan(xc, z, ldz, xdbl, dirs, B, L, E, R, out_f32, out_planes, workspace, range_flag, static_cast<hipStream_t>(stream));
}

int pope_vim_conv1d_silu_f32(const float* x, int ldx, const pope_vim_dir_weights* dirs, int B, int L, int E, float* xc, void* stream) {
    POPE_TRY(pope_vim_conv1d_check(x, ldx, dirs, B, L, E, xc));
    StreamDevice on_device(stream);
    return pope_launch_vim_conv1d(x, ldx, dirs, B, L, E, xc, static_cast<hipStream_t>(stream));
}

int pope_vim_add_rmsnorm_f32(const float* hidden, const float* res_in, float* res_out, const float* w, float* y_f32, void* y_planes,
                             long long rows, int D, float eps, long long row_stride, long long row_offset, unsigned* range_flag,
                             void* stream) {
    POPE_TRY(pope_vim_add_rmsnorm_check(hidden, w, y_f32, y_planes, rows, D, eps, row_stride, row_offset));
    StreamDevice on_device(stream);
    return pope_launch_vim_add_rmsnorm(hidden, res_in, res_out, w, y_f32, y_planes, rows, D, eps, row_stride, row_offset, range_flag,
                                       static_cast<hipStream_t>(stream));
}

// ---- MoCoPE fusion pose model (mocope.hip) ------------------------------------------------------------------------------------

size_t pope_mocope_workspace_bytes(int B, int S) { return pope_mocope_workspace(B, S); }

int pope_mocope_forward_f32(const pope_mocope_weights* w, const float* dense0, const float* dense1, const float* kpts0,
                            const float* kpts1, const int* counts, const int* sample_index, const unsigned long long* seeds,
                            const float* feat0, const float* feat1, int B, int S, int G, long long M, int train_type,
                            float* trans, float* rot, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    MocopeArgs a = {};
    a.w = w; a.in = posereg_input(dense0, dense1, kpts0, kpts1, counts, sample_index, seeds, B, S, M);
    a.feat0 = feat0; a.feat1 = feat1; a.G = G; a.train_type = train_type; a.stage = MOCOPE_STAGE_FULL;
    a.trans = trans; a.rot = rot; a.status = status; a.ws = workspace; a.ws_bytes = workspace_bytes;
    POPE_TRY(pope_mocope_check(a));
    StreamDevice on_device(stream);
    return pope_launch_mocope(a, static_cast<hipStream_t>(stream));
}

int pope_mocope_tap_f32(const pope_mocope_weights* w, const float* dense0, const float* dense1, const float* kpts0,
                        const float* kpts1, const int* counts, const int* sample_index, const unsigned long long* seeds,
                        const float* feat0, const float* feat1, int B, int S, int G, long long M, int train_type, int stage,
                        float* tap_out, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (stage == MOCOPE_STAGE_FULL) return POPE_ERR_ARG;
    MocopeArgs a = {};
    a.w = w; a.in = posereg_input(dense0, dense1, kpts0, kpts1, counts, sample_index, seeds, B, S, M);
    a.feat0 = feat0; a.feat1 = feat1; a.G = G; a.train_type = train_type; a.stage = stage;
    a.tap_out = tap_out; a.status = status; a.ws = workspace; a.ws_bytes = workspace_bytes;
    POPE_TRY(pope_mocope_check(a));
    StreamDevice on_device(stream);
    return pope_launch_mocope(a, static_cast<hipStream_t>(stream));
}

// the launches of the transformers one by one (tests)
int pope_mocope_linear_f32(const float* A, const float* W, const float* bias, float* Y, int R, int K, int N, int act, void* stream) {
    if (!A || !W || !bias || !Y || R <= 0 || K <= 0 || (K & 3) || N <= 0 || act < 0 || act > 1) return POPE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15) return POPE_ERR_ARG;    // 16-byte loads
    StreamDevice on_device(stream);
    return pope_launch_mocope_linear(A, W, bias, Y, R, K, N, act, static_cast<hipStream_t>(stream));
}

int pope_mocope_attention_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int R, int S, int G,
                              int d, void* stream) {
    if (!Q || !K || !V || !O || (d != 76 && d != 512) || G < 1 || G > 64 || R <= 0 || S <= 0) return POPE_ERR_ARG;
    if (ldq < d || ldk < d || ldv < d || (long long)R % ((long long)S * G)) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_mocope_attention(Q, ldq, K, ldk, V, ldv, O, R, S, G, d, static_cast<hipStream_t>(stream));
}

int pope_mocope_add_ln_f32(float* X, const float* Y, const float* w1, const float* b1, const float* w2, const float* b2, int R, int d,
                           void* stream) {
    if (!X || !Y || !w1 || !b1 || !w2 != !b2 || (d != 76 && d != 512) || R <= 0) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_mocope_add_ln(X, Y, w1, b1, w2, b2, R, d, static_cast<hipStream_t>(stream));
}

int pope_mocope_ffn76_f32(float* X, const float* l1w, const float* l1b, const float* l2w, const float* l2b, const float* nw,
                          const float* nb, const float* fw, const float* fb, int R, void* stream) {
    if (!X || !l1w || !l1b || !l2w || !l2b || !nw || !nb || !fw != !fb || R <= 0) return POPE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(l1w) | reinterpret_cast<uintptr_t>(l1b) | reinterpret_cast<uintptr_t>(l2w)) & 15) return POPE_ERR_ARG;
    StreamDevice on_device(stream);
    return pope_launch_mocope_ffn76(X, l1w, l1b, l2w, l2b, nw, nb, fw, fb, R, static_cast<hipStream_t>(stream));
}
