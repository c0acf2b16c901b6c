// The launch sequence of one DinoVisionTransformer forward (pope_vit_forward*_f32 of include/pope_hip.h) and its patch embed:
// argument checks, workspace carving, the route, the launches.  No allocation, no synchronisation.
#include "../../include/pope_hip.h"
#include "common.h"
#include "kernels.h"
#include "linear.h"
#include "stream_device.h"

namespace {

// Optional in-situ timing: events[i] is recorded on the stream right before launch i and one more
// after the last launch, so events[i]..events[i+1] bracket exactly one kernel of the product path.
// With a kind mask only the selected launches are bracketed: an event is recorded when the coming launch is
// selected (it starts a bracket) or the previous one was (it closes one); kinds[i] = -1 marks close-only events.
struct Recorder {
    void* const* events;
    int capacity;
    int* kinds;
    int n;
    unsigned mask = ~0u;
    bool open = false;
    bool mark(int kind, hipStream_t stream) {
        if (!events) return true;
        const bool sel = kind >= 0 && ((mask >> kind) & 1u);
        if (!sel && !open) return true;
        if (n >= capacity) return false;
        if (hipEventRecord(static_cast<hipEvent_t>(events[n]), stream) != hipSuccess) return false;
        if (kinds) kinds[n] = sel ? kind : -1;
        open = sel;
        ++n;
        return true;
    }
};

}  // namespace

int pope_launch_patch_embed_f32(const float* img, const float* proj_w, const float* posb, float* tokens, int B, int H, int W,
                                int patch, int dim, hipStream_t stream) {
    if (!img || !proj_w || !posb || !tokens || B <= 0 || patch <= 0 || H % patch || W % patch) return POPE_ERR_ARG;
    GemmParams g = {};
    g.A = img; g.W = proj_w; g.C = tokens;
    g.K = 3 * patch * patch;
    g.ldw = g.K; g.ldc = dim;
    g.ntok = 1 + (H / patch) * (W / patch);
    g.M = B * g.ntok; g.N = dim;
    g.epilogue = EPI_POSB;
    g.posb = posb;
    g.img_h = H; g.img_w = W; g.patch = patch; g.grid_w = W / patch;
    return pope_launch_gemm_nt_f32(g, stream);
}

int pope_launch_patch_embed_planes(const float* img, const void* proj_w_planes, const float* posb, float* tokens, int B, int H, int W,
                                   int patch, int dim, void* a_planes_scratch, size_t scratch_bytes, unsigned* range_flag,
                                   hipStream_t stream) {
    if (!img || !proj_w_planes || !posb || !tokens || !a_planes_scratch || B <= 0 || patch <= 0 || H % patch || W % patch)
        return POPE_ERR_ARG;
    const int kp = (3 * patch * patch + 31) & ~31, ntok = 1 + (H / patch) * (W / patch);
    if (scratch_bytes < size_t(B) * ntok * kp * 4) return POPE_ERR_WORKSPACE;
    POPE_TRY(pope_launch_im2col_planes(img, a_planes_scratch, B, H, W, patch, kp, range_flag, stream));
    // tokens[b, n] = posb[n] + 1 * (A[b, n] . W^T): rows n = 0 are all-zero A rows (cls_token + pos_embed[0] from the table)
    GemmParams g = pope_linear_params(LINEAR_PLANES, a_planes_scratch, proj_w_planes, nullptr, tokens, nullptr, B * ntok, dim, kp,
                                      EPI_BIAS_LS_RES, nullptr, posb, ntok);
    g.range_bit = 0;   // fp32 tokens: nothing to report
    return pope_launch_gemm_planes(g, stream);
}

static int vit_forward_impl(const pope_vit_weights* w, int ffn, const float* img, int B, int H, int W, const float* posb,
                            float* x_prenorm, float* x_norm, int n_taps, const int* tap_blocks_host,
                            float* const* tap_out_host, void* workspace, size_t workspace_bytes, unsigned* range_flag,
                            void* stream_, Recorder& rec) {
    if (!w || !img || !posb || !x_prenorm || !workspace || !w->blocks_host) return POPE_ERR_ARG;
    if (w->dim != w->heads * 64 || w->patch <= 0 || H % w->patch || W % w->patch || B <= 0) return POPE_ERR_ARG;
    if (n_taps < 0 || (n_taps > 0 && (!tap_blocks_host || !tap_out_host))) return POPE_ERR_ARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int dim = w->dim, hidden = w->hidden, prec = w->precision;
    if (prec != POPE_PREC_F32_MFMA && prec != POPE_PREC_F16X3 && prec != POPE_PREC_F16) return POPE_ERR_ARG;
    // SwiGLU FFN (pope_hip.h POPE_FFN_SWIGLU): fc1 = the permuted w12 [2 hidden, dim], fc2 = w3 [dim, hidden]; the w12 GEMM's
    // 64-column blocks need hidden % 32 == 0; no plain-f16 form
    if (ffn != POPE_FFN_MLP && ffn != POPE_FFN_SWIGLU) return POPE_ERR_ARG;
    const bool swiglu = ffn == POPE_FFN_SWIGLU;
    if (swiglu && (prec == POPE_PREC_F16 || hidden <= 0 || (hidden & 31))) return POPE_ERR_ARG;
    for (int i = 0; swiglu && i < w->depth; ++i)
        if (!w->blocks_host[i].fc1_w || !w->blocks_host[i].fc1_b || !w->blocks_host[i].fc2_w) return POPE_ERR_ARG;
    StreamDevice on_device(stream_);   // the only device query of the forward: every launch below is a launcher call
    const int fc1_n = swiglu ? 2 * hidden : hidden, fc1_epi = swiglu ? int(EPI_BIAS_SWIGLU) : int(EPI_BIAS_GELU);
    const int ntok = 1 + (H / w->patch) * (W / w->patch);
    const int rows = B * ntok;
    if (workspace_bytes < pope_vit_workspace_bytes(B, ntok, dim, hidden)) return POPE_ERR_WORKSPACE;

    // workspace: xn [rows,dim] | big [rows, max(4dim, hidden)] = {qkv [rows,3dim], attn [rows,dim]} or fc1 out.  The packed
    // forms (planes, f16 rows) alias the same buffers: 2 x f16 per element = the fp32 footprint
    pope_carver ws{static_cast<char*>(workspace)};
    float* xn = ws.take<float>(size_t(rows) * dim * sizeof(float));
    float* big = reinterpret_cast<float*>(ws.at);
    const size_t big_bytes = workspace_bytes - size_t(ws.at - static_cast<char*>(workspace));
    float* qkv = big;
    float* att = big + size_t(rows) * 3 * dim;
    float* hid = big;
    float* x = x_prenorm;
    const float eps = 1e-6f;  // vision_transformer.py:90

    // f16x3 = the planes dataflow end to end (every operand is split ONCE by its producer, which also guards the f16
    // range: range_flag).  It needs the weight planes of all four Linear layers of every block; without them (or with
    // a width the planes layout does not take) the model runs on the fp32 MFMA, which has no range contract.
    bool planes = (prec == POPE_PREC_F16X3 || prec == POPE_PREC_F16) && dim % 32 == 0 && dim >= 64 && hidden % 32 == 0;
    for (int i = 0; planes && i < w->depth; ++i) {
        const pope_vit_block_weights& k = w->blocks_host[i];
        planes = k.qkv_wp && k.proj_wp && k.fc1_wp && k.fc2_wp;
    }
    // POPE_PREC_F16: the blocks' Linear layers and attention in plain f16 (one MFMA per product; `*_wp` of the blocks
    // are f16 row-major matrices, value * 256); the patch embed stays f16x3 (`patch_wp` = planes) and the residual
    // stream, LayerNorm statistics, softmax and GELU fp32.  Needs the weights and widths the plain GEMM takes.
    const bool plain = prec == POPE_PREC_F16;
    if (plain && (!planes || !w->patch_wp || (dim & 63) || (hidden & 63))) return POPE_ERR_ARG;
    // Fused form (dim 384): every residual GEMM (patch embed, proj, fc2) also emits the LayerNorm that follows it —
    // as planes for the next GEMM, or as fp32 x_norm after the last block — so no stand-alone LayerNorm launch is left
    // (gemm_rowln.hip).
    const GemmParams probe = pope_linear_params(LINEAR_PLANES, nullptr, nullptr, nullptr, nullptr, nullptr, rows, dim, dim, EPI_BIAS_LS_RES);
    const bool fusable = planes && !plain && w->patch_wp && pope_gemm_rowln_supported(probe);
    // Small batches: the full-row-tile kernel has one tile per 128 rows, each a serial chain of K / 32 K-steps + a 23 us
    // epilogue; while the 128 x 128 residual GEMM still fits ONE round of its 2 x CUs workgroup slots (3 column tiles per row
    // tile) it finishes sooner, and `layernorm_rowln_order` reproduces the fused epilogue's LayerNorm bit for bit — an image
    // gives the same tokens alone (this path) and inside a 64-image chunk (fused path).  Driver step (9 images of 196 x
    // 196): proj 38 -> ~25 us, FC2 105 -> ~70 us per launch.
    const bool small = fusable && 3 * ((rows + 127) / 128) <= 2 * pope_cu_count();
    const bool fused = fusable && !small;
    const LinearForm form = plain ? LINEAR_PLAIN : planes ? LINEAR_PLANES : LINEAR_F32;

    // ---- the route's operations; the block loop below is the same for every route ----
    // LayerNorm(x) -> xn as the route's GEMM operand (fused: the residual GEMM before it has written it already)
    auto norm = [&](const float* nw, const float* nb) {
        if (plain) return pope_launch_layernorm_f16(x, nw, nb, xn, rows, dim, eps, range_flag, stream);
        if (small) return pope_launch_layernorm_rowln_order(x, nw, nb, xn, nullptr, rows, eps, range_flag, stream);
        if (planes) return pope_launch_layernorm_planes(x, dim, nw, nb, xn, rows, dim, eps, range_flag, stream);
        return pope_launch_layernorm_f32(x, dim, nw, nb, xn, dim, rows, dim, eps, stream);
    };
    // one Linear over the token rows: fp32 `Cf` or packed `c_pk` (planes; plain: f16 rows) = epi(a . W^T + bias [, gamma, res]);
    // `wf` is the fp32 route's weight, `wp` the packed routes'.  Only a packed output (and every plain launch) reports its range.
    auto linear = [&](const void* a, const float* wf, const void* wp, const float* bias, float* Cf, void* c_pk, int N, int K, int epi,
                      const float* gamma, const float* res) {
        if (form == LINEAR_F32) {
            if (!wf) return POPE_ERR_ARG;
            float* C = Cf ? Cf : static_cast<float*>(c_pk);
            return pope_launch_gemm_nt_f32(pope_linear_params(form, a, wf, bias, C, nullptr, rows, N, K, epi, gamma, res), stream);
        }
        GemmParams g = pope_linear_params(form, a, wp, bias, Cf, c_pk, rows, N, K, epi, gamma, res, 0, plain || c_pk ? range_flag : nullptr);
        if (epi == EPI_QKV_F16) { g.sam_dim = N / 3; g.sam_qscale = 0.125f * 1.44269504088896340736f; }   // heads of 64: head_dim^-0.5 * log2 e
        return pope_launch_gemm_planes(g, stream);
    };
    // residual GEMM + following LayerNorm: x = res + gamma * (a . W^T + bias); LN(x; ln_w, ln_b) -> planes or fp32
    auto rowln = [&](const void* a_pl, const void* w_pl, int K, const float* bias, const float* gamma, const float* res, int res_mod,
                     const float* ln_w, const float* ln_b, void* ln_planes, float* ln_f32) {
        return pope_launch_gemm_rowln(pope_linear_rowln_params(a_pl, w_pl, rows, dim, K, bias, gamma, res, res_mod, x, ln_w, ln_b, eps,
                                                               ln_planes, ln_f32, range_flag), stream);
    };
    auto attention = [&] {
        // plain: q (pre-scaled by head_dim^-0.5 log2 e), k, v leave the QKV epilogue as f16 rows: the attention kernel stages K / V
        // memory -> LDS directly (attention_f16.hip)
        if (plain) return pope_launch_attention_f16_dma(qkv, att, B, ntok, w->heads, stream);
        // q, k, v stay planes from the QKV epilogue to the attention kernel's LDS
        if (planes) return pope_launch_attention_f16x3_planes_io(qkv, att, B, ntok, w->heads, stream);
        return pope_launch_attention_f32(qkv, att, B, ntok, w->heads, stream);
    };

#define POPE_MARK(kind) do { if (!rec.mark(kind, stream)) return POPE_ERR_ARG; } while (0)
    POPE_MARK(POPE_K_PATCH_EMBED);
    if (fused) {   // `big` is free here: it holds the im2col planes
        const int kp = (3 * w->patch * w->patch + 31) & ~31;
        if (big_bytes < size_t(rows) * kp * 4) return POPE_ERR_WORKSPACE;
        POPE_TRY(pope_launch_im2col_planes(img, big, B, H, W, w->patch, kp, range_flag, stream));
        const pope_vit_block_weights& k0 = w->blocks_host[0];
        POPE_TRY(rowln(big, w->patch_wp, kp, nullptr, nullptr, posb, ntok, k0.norm1_w, k0.norm1_b, xn, nullptr));
    } else if (planes && w->patch_wp) {
        POPE_TRY(pope_launch_patch_embed_planes(img, w->patch_wp, posb, x, B, H, W, w->patch, dim, big, big_bytes, range_flag, stream));
    } else {
        POPE_TRY(pope_launch_patch_embed_f32(img, w->patch_w, posb, x, B, H, W, w->patch, dim, stream));
    }
    for (int i = 0; i < w->depth; ++i) {
        const pope_vit_block_weights& k = w->blocks_host[i];
        // x = x + ls1(attn(norm1(x)))                                      block.py:105
        if (!fused) {
            POPE_MARK(POPE_K_LAYERNORM);
            POPE_TRY(norm(k.norm1_w, k.norm1_b));
        }
        POPE_MARK(POPE_K_GEMM_QKV);
        POPE_TRY(linear(xn, k.qkv_w, k.qkv_wp, k.qkv_b, nullptr, qkv, 3 * dim, dim, plain ? EPI_QKV_F16 : EPI_BIAS, nullptr, nullptr));
        POPE_MARK(POPE_K_ATTENTION);
        POPE_TRY(attention());
        POPE_MARK(POPE_K_GEMM_PROJ);
        if (fused) POPE_TRY(rowln(att, k.proj_wp, dim, k.proj_b, k.ls1, x, 0, k.norm2_w, k.norm2_b, xn, nullptr));
        else POPE_TRY(linear(att, k.proj_w, k.proj_wp, k.proj_b, x, nullptr, dim, dim, EPI_BIAS_LS_RES, k.ls1, x));
        // x = x + ls2(mlp(norm2(x)))                                       block.py:106
        if (!fused) {
            POPE_MARK(POPE_K_LAYERNORM);
            POPE_TRY(norm(k.norm2_w, k.norm2_b));
        }
        POPE_MARK(POPE_K_GEMM_FC1);
        POPE_TRY(linear(xn, k.fc1_w, k.fc1_wp, k.fc1_b, nullptr, hid, fc1_n, dim, fc1_epi, nullptr, nullptr));   // -> hid [rows, hidden] either way
        POPE_MARK(POPE_K_GEMM_FC2);
        if (fused && i + 1 < w->depth) {
            const pope_vit_block_weights& kn = w->blocks_host[i + 1];
            POPE_TRY(rowln(hid, k.fc2_wp, hidden, k.fc2_b, k.ls2, x, 0, kn.norm1_w, kn.norm1_b, xn, nullptr));
        } else if (fused && x_norm) {   // last block: the final norm (vision_transformer.py:230) as fp32
            POPE_TRY(rowln(hid, k.fc2_wp, hidden, k.fc2_b, k.ls2, x, 0, w->norm_w, w->norm_b, nullptr, x_norm));
        } else {
            POPE_TRY(linear(hid, k.fc2_w, k.fc2_wp, k.fc2_b, x, nullptr, dim, hidden, EPI_BIAS_LS_RES, k.ls2, x));
        }
        for (int t = 0; t < n_taps; ++t)
            if (tap_blocks_host[t] == i && tap_out_host[t]) {
                POPE_MARK(POPE_K_TAP_COPY);
                if (hipMemcpyAsync(tap_out_host[t], x, size_t(rows) * dim * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
                    return POPE_ERR_LAUNCH;
            }
    }
    if (x_norm && !fused) {
        POPE_MARK(POPE_K_LAYERNORM);
        if (small) POPE_TRY(pope_launch_layernorm_rowln_order(x, w->norm_w, w->norm_b, nullptr, x_norm, rows, eps, nullptr, stream));
        else POPE_TRY(pope_launch_layernorm_f32(x, dim, w->norm_w, w->norm_b, x_norm, dim, rows, dim, eps, stream));
    }
    POPE_MARK(-1);  // closing event
#undef POPE_MARK
    return POPE_OK;
}

extern "C" {

size_t pope_vit_workspace_bytes(int B, int ntok, int dim, int hidden) {
    if (B <= 0 || ntok <= 0 || dim <= 0 || hidden <= 0) return 0;
    const size_t rows = size_t(B) * ntok;
    const size_t big = size_t(hidden) > size_t(4) * dim ? size_t(hidden) : size_t(4) * dim;
    return pope_align256(rows * dim * sizeof(float)) + pope_align256(rows * big * sizeof(float));
}

int pope_vit_forward_f32(const pope_vit_weights* w, int ffn, const float* img, int B, int H, int W, const float* posb,
                         float* x_prenorm, float* x_norm, int n_taps, const int* tap_blocks_host,
                         float* const* tap_out_host, void* workspace, size_t workspace_bytes, unsigned* range_flag,
                         void* stream) {
    Recorder rec{nullptr, 0, nullptr, 0};
    return vit_forward_impl(w, ffn, img, B, H, W, posb, x_prenorm, x_norm, n_taps, tap_blocks_host, tap_out_host, workspace,
                            workspace_bytes, range_flag, stream, rec);
}

int pope_vit_forward_profiled_f32(const pope_vit_weights* w, int ffn, const float* img, int B, int H, int W,
                                  const float* posb, float* x_prenorm, float* x_norm, void* workspace,
                                  size_t workspace_bytes, unsigned* range_flag, void* stream,
                                  void* const* events_host, int n_events, int* kinds_host, int* n_launches_host,
                                  unsigned kind_mask) {
    if (!events_host || n_events < 2 || !kinds_host || !n_launches_host) return POPE_ERR_ARG;
    Recorder rec{events_host, n_events, kinds_host, 0};
    rec.mask = kind_mask;
    const int rc = vit_forward_impl(w, ffn, img, B, H, W, posb, x_prenorm, x_norm, 0, nullptr, nullptr, workspace,
                                    workspace_bytes, range_flag, stream, rec);
    *n_launches_host = rec.n > 0 ? rec.n - 1 : 0;
    return rc;
}

int pope_vit_launch_count(int depth) { return depth > 0 ? 7 * depth + 2 : 0; }

}  // extern "C"
