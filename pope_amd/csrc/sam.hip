// SAM image encoder (segment_anything/segment_anything/modeling/image_encoder.py:17-118: ViT-B/L/H with 14x14 window
// attention, four global blocks, decomposed relative position terms, and the 1x1 / 3x3 convolution neck) on the f16x3
// planes GEMMs of the DINOv2 path.  BASELINE config 5 / SURVEY.md §8 f-3.
//
// This file: the encoder's own small kernels (patch-embed operand, the neck's LayerNorm2d), its workspace layout
// (`SamEncLayout`, shared by the size query and the launcher), its argument check and its ONE launch sequence for the three
// precisions (pope_hip.h): POPE_PREC_F16X3 = f16 hi / lo operand planes, three MFMAs per product; POPE_PREC_F16 = plain f16
// operands, one MFMA per product (template flag PLAIN here and in gemm_planes.hip), fp32 accumulators / softmax / LayerNorm /
// residual stream in both; POPE_PREC_F32_MFMA = fp32 operands everywhere (kernels: sam_f32.hip), the range guard's re-run.
// What is new in this encoder is the attention: sam_attention.hip.
#include "attention_common.h"
#include "conv_layer.h"
#include "kernels.h"
#include "linear.h"
#include <algorithm>

namespace {

using pope_attn::f16x4;
using pope_attn::f16x8;

constexpr float A_SCALE = K_PLANES_ACT_SCALE;

using pope_attn::cat;

// ---- patch embed operand: image [B, 3, S, S] -> activation planes [B * g * g, 3 * P * P], k = (c, ky, kx) as
// Conv2d's weight.reshape(dim, -1) (image_encoder.py:385-393); P % 8 == 0
template <bool PLAIN>
__global__ __launch_bounds__(256) void sam_im2col_kernel(const float* __restrict__ img, _Float16* __restrict__ out, int B, int S,
                                                         int P, unsigned* range_flag) {
    const int g = S / P, K = 3 * P * P, pieces = K / 8;
    const long long total = (long long)B * g * g * pieces;
    float amax = 0.f;
    for (long long id = blockIdx.x * 256ll + threadIdx.x; id < total; id += 256ll * gridDim.x) {
        const int pc = int(id % pieces);
        const long long row = id / pieces;
        const int px = int(row % g), py = int((row / g) % g), b = int(row / ((long long)g * g));
        const int k = pc * 8, c = k / (P * P), ky = (k - c * P * P) / P, kx = k - c * P * P - ky * P;
        const float* src = img + (((size_t)b * 3 + c) * S + (py * P + ky)) * S + px * P + kx;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
        amax = pope_amax4(pope_amax4(amax, v0), v1);
        const float s8 = ((v0[0] + v0[1]) + (v0[2] + v0[3])) + ((v1[0] + v1[1]) + (v1[2] + v1[3]));
        if (!(s8 == s8)) amax = INFINITY;   // NaN (fmax drops it)
        if constexpr (PLAIN) {   // f16 row-major
            *reinterpret_cast<f16x8*>(out + (size_t)row * K + k) =
                cat(__builtin_convertvector(v0 * A_SCALE, f16x4), __builtin_convertvector(v1 * A_SCALE, f16x4));
        } else {
            pope_planes_store(out + (size_t)row * 2 * K, k, v0 * A_SCALE, v1 * A_SCALE);
        }
    }
    pope_range_flag(range_flag, POPE_RANGE_INPUT, !(amax * A_SCALE < POPE_F16_OVERFLOW));
}

// ---- neck LayerNorm2d (common.py:27-43: per pixel over the channels, eps inside the sqrt, a true division) -----------
// in: fp32 [pixels, C] (C % 256 == 0, <= 1024); one wave per pixel, four channels per lane and 256-column group
template <bool TO_BORDERED_PLANES, bool PLAIN = false>
__global__ __launch_bounds__(256) void sam_ln2d_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                       const float* __restrict__ bvec, void* __restrict__ out, int B, int g, int C,
                                                       float eps, unsigned* range_flag) {
    // TO_BORDERED_PLANES: in = [B g g, C] rows, out = activation planes [B, g + 2, g + 2, C] with a zero border (the
    //   3x3 convolution's operand, conv.hip layout); the wave index walks the BORDERED pixels
    // else: in = fp32 [B, g + 2, g + 2, C] (the convolution's bordered output), out = fp32 NCHW [B, C, g, g]; the wave
    //   index walks the interior pixels
    const int gp = g + 2, nv = C / 256;
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * 4, total = (long long)B * (TO_BORDERED_PLANES ? gp * gp : g * g);
    float amax = 0.f;
    for (long long pix = blockIdx.x * 4ll + (threadIdx.x >> 6); pix < total; pix += waves) {
        int b, y, x;   // interior coordinates
        if (TO_BORDERED_PLANES) {
            b = int(pix / (gp * gp));
            const int rem = int(pix - (long long)b * gp * gp);
            y = rem / gp - 1;
            x = rem % gp - 1;
        } else {
            b = int(pix / (g * g));
            const int rem = int(pix - (long long)b * g * g);
            y = rem / g;
            x = rem % g;
        }
        const bool interior = y >= 0 && y < g && x >= 0 && x < g;
        f32x4 v[4] = {};
        float sum = 0.f;
        const float* src = TO_BORDERED_PLANES ? in + ((size_t)b * g * g + (size_t)y * g + x) * C
                                              : in + ((size_t)b * gp * gp + (size_t)(y + 1) * gp + (x + 1)) * C;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (interior && k < nv) {
                v[k] = *reinterpret_cast<const f32x4*>(src + k * 256 + lane * 4);
                sum += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
            }
        const float u = wave_sum(sum) / float(C);
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (interior && k < nv) {
                v[k] = v[k] - u;
                sq += (v[k][0] * v[k][0] + v[k][1] * v[k][1]) + (v[k][2] * v[k][2] + v[k][3] * v[k][3]);
            }
        const float den = sqrtf(wave_sum(sq) / float(C) + eps);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= nv) continue;
            const int col = k * 256 + lane * 4;
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            if (interior) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + col), b4 = *reinterpret_cast<const f32x4*>(bvec + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = w4[e] * (v[k][e] / den) + b4[e];
            }
            if (TO_BORDERED_PLANES) {
                amax = pope_amax4(amax, r);
                if (!((r[0] + r[1]) + (r[2] + r[3]) == (r[0] + r[1]) + (r[2] + r[3]))) amax = INFINITY;
                if constexpr (PLAIN) {
                    *reinterpret_cast<f16x4*>(static_cast<_Float16*>(out) + (size_t)pix * C + col) = __builtin_convertvector(r * A_SCALE, f16x4);
                } else {
                    pope_planes_store(static_cast<_Float16*>(out) + (size_t)pix * 2 * C, col, r * A_SCALE);
                }
            } else {
                float* dst = static_cast<float*>(out) + (((size_t)b * C + col) * g + y) * g + x;
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[(size_t)e * g * g] = r[e];
            }
        }
    }
    if (TO_BORDERED_PLANES) pope_range_flag(range_flag, POPE_RANGE_INPUT, !(amax * A_SCALE < POPE_F16_OVERFLOW));
}

// ---- host ---------------------------------------------------------------------------------------------------------
// The workspace of one forward pass over B images: byte offsets from its start, every region 256-byte aligned.  The size
// query returns `total`; the launcher adds the offsets to the caller's pointer.
struct SamEncLayout {
    int g = 0, hd = 0;
    size_t rows = 0, brows = 0, kp = 0;   // tokens B g g, pixels of the neck's bordered maps B (g + 2)^2, patch-embed depth 3 patch^2
    SamAttnPlan plan[2];      // [0] the window blocks' geometry (window 0: the grid's), [1] the global blocks'
    // x: residual stream fp32 [rows, dim] | xn: the LayerNorm output as the precision's GEMM operand | big: im2col operand, then
    // per block the attention output (the proj GEMM's operand; room for 4 dim: mlp_ratio 4) and fc1's output | one operand set per
    // geometry: their constant parts are written once per forward pass | t1: neck 1x1 output fp32 [rows, oc] | t1_pl: its
    // LayerNorm2d as the 3x3 convolution's bordered operand | t2: the convolution's bordered output fp32
    size_t x = 0, xn = 0, big = 0, t1 = 0, t1_pl = 0, t2 = 0, total = 0;   // total 0: no layout for this geometry
    struct { size_t q, k, v, tab, map; } op[2] = {};
    // POPE_PREC_F32_MFMA reads the same bytes as fp32 scratch: qkv [rows, 3 dim] in `big`, the attention output [rows, dim] at
    // the start of the operand sets, LayerNorm2d's bordered fp32 output on `t1_pl` (the same brows oc 4 bytes)
    size_t qkv32 = 0, att32 = 0, t1b32 = 0;
    bool att32_fits = false;

    SamEncLayout(const pope_sam_encoder_weights& w, int B) {
        if (B <= 0 || w.img <= 0 || w.patch <= 0 || w.img % w.patch || w.heads <= 0 || w.dim % w.heads) return;
        g = w.img / w.patch; hd = w.dim / w.heads;
        rows = size_t(B) * g * g; brows = size_t(B) * (g + 2) * (g + 2); kp = size_t(3) * w.patch * w.patch;
        if (!pope_sam_attn_plan(B, g, w.window > 0 ? w.window : g, w.heads, hd, plan[0]) || !pope_sam_attn_plan(B, g, g, w.heads, hd, plan[1]))
            return;
        size_t at = 0;
        auto take = [&at](size_t bytes) { const size_t off = at; at += pope_align256(bytes); return off; };
        x = take(rows * w.dim * 4);
        xn = take(rows * w.dim * 4);
        big = take(std::max({rows * 4 * w.dim * 4, rows * w.hidden * 4, rows * kp * 4}));
        for (int s = 0; s < 2; ++s) {
            op[s].q = take(plan[s].qp); op[s].k = take(plan[s].kp); op[s].v = take(plan[s].vp);
            op[s].tab = take(plan[s].tab); op[s].map = take(plan[s].map);
        }
        t1 = take(rows * w.out_chans * 4);
        t1_pl = take(brows * w.out_chans * 4);
        t2 = take(brows * w.out_chans * 4);
        total = at;
        qkv32 = big; att32 = op[0].q; t1b32 = t1_pl;
        // Q' of the window geometry alone is G Npad 2 DQ 2 bytes with G Npad >= rows heads and DQ >= hd whenever hd is a multiple
        // of 16: at least rows dim 4.  So this holds for the head dims sam_encoder_check admits (64, 80) and never refuses one of
        // them; it is false only for a head dim the check refuses anyway, and is computed rather than assumed so that a new
        // head dim or score depth cannot silently overlap the regions.
        att32_fits = plan[0].qp >= rows * w.dim * 4;
    }
    SamAttnOperands operands(char* base, int s) const {
        return {base + op[s].q, base + op[s].k, base + op[s].v, base + op[s].tab, reinterpret_cast<int*>(base + op[s].map)};
    }
};

// Everything pope_launch_sam_encoder can refuse, without a HIP call.  use[s]: some block runs on geometry s.
int sam_encoder_check(const SamEncArgs& q, const SamEncLayout& L, bool use[2]) {
    if (!q.w || !q.w->blocks_host) return POPE_ERR_ARG;
    const pope_sam_encoder_weights& w = *q.w;
    if (!q.image || !q.out || !q.ws || !w.patch_wp || !w.patch_b || !w.ones || !w.neck0_wp || !w.neck2_wp || !w.neck1_w || !w.neck1_b ||
        !w.neck3_w || !w.neck3_b)
        return POPE_ERR_ARG;
    if (q.n_taps < 0 || (q.n_taps > 0 && (!q.tap_blocks || !q.tap_out))) return POPE_ERR_ARG;
    if (q.B <= 0 || w.depth <= 0 || w.patch <= 0 || (w.patch & 7) || w.img % w.patch || w.heads <= 0 || w.dim % w.heads) return POPE_ERR_ARG;
    const int hd = w.dim / w.heads, dim = w.dim, hidden = w.hidden, oc = w.out_chans, kp = 3 * w.patch * w.patch;
    if ((hd != 64 && hd != 80) || (dim & 127) || dim > 2048 || (hidden & 31) || (oc & 255) || oc > 1024 || w.window < 0 || (kp & 31))
        return POPE_ERR_ARG;
    if (!L.total || !L.att32_fits) return POPE_ERR_ARG;
    if ((L.rows + 256) * (hidden > 3 * dim ? hidden : 3 * dim) * 4 >= (1ull << 32) - 512 || L.brows * oc * 4 >= (1ull << 32) - 512)
        return POPE_ERR_ARG;   // 32-bit buffer offsets in the GEMMs: the caller splits larger batches
    if (w.precision != POPE_PREC_F16X3 && w.precision != POPE_PREC_F16 && w.precision != POPE_PREC_F32_MFMA) return POPE_ERR_ARG;
    if (w.precision == POPE_PREC_F16 && ((dim & 63) || (hidden & 63) || (kp & 63))) return POPE_ERR_ARG;
    use[0] = use[1] = false;
    for (int i = 0; i < w.depth; ++i) {
        const pope_sam_block_weights& k = w.blocks_host[i];
        if (!k.norm1_w || !k.norm1_b || !k.qkv_wp || !k.qkv_b || !k.proj_wp || !k.proj_b || !k.norm2_w || !k.norm2_b || !k.fc1_wp ||
            !k.fc1_b || !k.fc2_wp || !k.fc2_b || !k.rel_h || !k.rel_w)
            return POPE_ERR_ARG;
        use[(k.global_attn || w.window <= 0) ? 1 : 0] = true;
    }
    for (int s = 0; s < 2; ++s) {
        if (!use[s]) continue;
        if (w.precision == POPE_PREC_F32_MFMA) POPE_TRY(pope_sam32_attention_check(q.B, L.g, L.plan[s].ws, w.heads, hd));
        else if (!L.plan[s].launchable) return POPE_ERR_ARG;
    }
    return q.ws_bytes < L.total ? POPE_ERR_WORKSPACE : POPE_OK;
}

}  // namespace

size_t pope_sam_encoder_workspace(const pope_sam_encoder_weights* w, int B) {
    return w && w->blocks_host && w->depth > 0 ? SamEncLayout(*w, B).total : 0;
}

int pope_launch_sam_encoder(const SamEncArgs& q, hipStream_t stream) {
    if (!q.w) return POPE_ERR_ARG;
    const SamEncLayout L(*q.w, q.B);
    bool use[2];
    POPE_TRY(sam_encoder_check(q, L, use));

    const pope_sam_encoder_weights& w = *q.w;
    const int B = q.B, g = L.g, dim = w.dim, hidden = w.hidden, oc = w.out_chans, kp = int(L.kp), rows = int(L.rows);
    char* const base = static_cast<char*>(q.ws);
    float* x = reinterpret_cast<float*>(base + L.x);
    void* xn = base + L.xn;
    void* big = base + L.big;   // attention output (the proj GEMM's operand); fc1's output reuses the buffer
    float* t1 = reinterpret_cast<float*>(base + L.t1);
    void* t1_pl = base + L.t1_pl;
    float* t2 = reinterpret_cast<float*>(base + L.t2);
    const SamAttnOperands ops[2] = {L.operands(base, 0), L.operands(base, 1)};
    // LayerNorm eps of the blocks (build_sam.py:71 passes 1e-6; the constructor's default norm_layer has 1e-5) and of the
    // neck's LayerNorm2d (common.py:28: 1e-6)
    const float eps = w.block_eps > 0.f ? w.block_eps : 1e-6f, neck_eps = w.neck_eps > 0.f ? w.neck_eps : 1e-6f;
    unsigned* flag = q.range_flag;

    // ---- the route's operations; the sequence below is the same for every route ----
    // precision "f16" (POPE_PREC_F16): every operand is a plain f16 tensor (activations * 8, weights * 256), one MFMA per
    // product, fp32 accumulation, fp32 residual stream / softmax / LayerNorm statistics — BASELINE config 5's dtype.
    // POPE_PREC_F32_MFMA: `*_wp` are fp32 matrices, every operand fp32, no range flag
    const bool f32 = w.precision == POPE_PREC_F32_MFMA, plain = w.precision == POPE_PREC_F16;
    const LinearForm form = f32 ? LINEAR_F32 : plain ? LINEAR_PLAIN : LINEAR_PLANES;
    void* att = f32 ? base + L.att32 : big;
    // LN(x) -> xn as the route's GEMM operand
    auto norm = [&](const float* nw, const float* nb) {
        if (f32) return pope_launch_layernorm_f32(x, dim, nw, nb, static_cast<float*>(xn), dim, rows, dim, eps, stream);
        if (plain) return pope_launch_layernorm_f16(x, nw, nb, xn, rows, dim, eps, flag, stream);
        return pope_launch_layernorm_planes(x, dim, nw, nb, xn, rows, dim, eps, flag, stream);
    };
    // one Linear over the token rows: fp32 `Cf` or the route's operand `c_op` = epi(a . W^T + bias [, gamma, res])
    auto linear = [&](const void* a, const void* wp, const float* bias, float* Cf, void* c_op, int N, int K, int epi, const float* gamma,
                      const float* res, int res_mod) {
        if (f32)
            return pope_launch_gemm_nt_f32(pope_linear_params(form, a, wp, bias, Cf ? Cf : static_cast<float*>(c_op), nullptr, rows, N, K, epi,
                                                              gamma, res), stream);
        return pope_launch_gemm_planes(pope_linear_params(form, a, wp, bias, Cf, c_op, rows, N, K, epi, gamma, res, res_mod, flag), stream);
    };
    // xn = norm1(x) -> att, the proj GEMM's operand
    auto attention = [&](const pope_sam_block_weights& k, int s) {
        if (!f32) return pope_sam_attn_block(L.plan[s], ops[s], plain, xn, k, att, flag, stream);
        float* qkv = reinterpret_cast<float*>(base + L.qkv32);
        POPE_TRY(linear(xn, k.qkv_wp, k.qkv_b, qkv, nullptr, 3 * dim, dim, EPI_BIAS, nullptr, nullptr, 0));
        return pope_launch_sam32_attention(qkv, k.qkv_b, k.rel_h, k.rel_w, static_cast<float*>(att), B, g, L.plan[s].ws, w.heads, L.hd, stream);
    };
    // the residual stream x -> xn as the neck's first operand (the fp32 GEMM reads x itself)
    auto to_operand = [&] {
        if (f32) return int(POPE_OK);
        if (plain) return pope_launch_to_f16(x, xn, (long long)rows * dim / 4, flag, stream);
        return pope_launch_split_planes(x, xn, rows, dim, A_SCALE, flag, stream);
    };
    // LayerNorm2d of the neck: t1 -> the 3x3 convolution's bordered operand, and the convolution's bordered output -> out
    auto norm2d_operand = [&] {
        const dim3 grid(pope_grid_for((long long)L.brows, 4));
        if (f32) return pope_launch_sam32_ln2d(t1, w.neck1_w, w.neck1_b, reinterpret_cast<float*>(base + L.t1b32), B, g, oc, neck_eps, true, stream);
        if (plain) hipLaunchKernelGGL((sam_ln2d_kernel<true, true>), grid, dim3(256), 0, stream, t1, w.neck1_w, w.neck1_b, t1_pl, B, g, oc, neck_eps, flag);
        else hipLaunchKernelGGL((sam_ln2d_kernel<true, false>), grid, dim3(256), 0, stream, t1, w.neck1_w, w.neck1_b, t1_pl, B, g, oc, neck_eps, flag);
        return pope_check_launch();
    };
    // the 3x3 convolution as a GEMM over the bordered pixels (conv.hip): LayerNorm2d's bordered operand -> t2
    auto conv3x3 = [&] {
        const int occ = plain ? oc / 2 : oc;   // plain: column pairs
        const void* a = f32 ? static_cast<const void*>(base + L.t1b32) : t1_pl;
        return pope_conv3_layer(w.precision, a, occ, w.neck2_wp, nullptr, oc, ConvGrid{B, g + 2, g + 2}, nullptr, t2, oc, 1.0f /* identity */,
                                nullptr, 0, false, flag, stream);
    };
    auto norm2d_out = [&] {
        if (f32) return pope_launch_sam32_ln2d(t2, w.neck3_w, w.neck3_b, q.out, B, g, oc, neck_eps, false, stream);
        hipLaunchKernelGGL((sam_ln2d_kernel<false, false>), dim3(pope_grid_for((long long)rows, 4)), dim3(256), 0, stream, t2, w.neck3_w, w.neck3_b,
                           static_cast<void*>(q.out), B, g, oc, neck_eps, static_cast<unsigned*>(nullptr));
        return pope_check_launch();
    };

    // patch embed + absolute position table (image_encoder.py:108-110): x = conv(img) + bias + pos[token]
    const int pe_epi = w.pos ? EPI_BIAS_LS_RES : EPI_BIAS;
    const float* pe_gamma = w.pos ? w.ones : nullptr;
    if (f32) {
        float* cols = static_cast<float*>(big);
        POPE_TRY(pope_launch_sam32_im2col(q.image, cols, B, w.img, w.patch, stream));
        for (int b = 0; b < B; ++b) {   // the position table is per token, the same for every image: one GEMM per image (gemm_f32.hip has no res_mod)
            const size_t r0 = size_t(b) * g * g;
            POPE_TRY(pope_launch_gemm_nt_f32(pope_linear_params(form, cols + r0 * kp, w.patch_wp, w.patch_b, x + r0 * dim, nullptr, g * g, dim, kp,
                                                                pe_epi, pe_gamma, w.pos), stream));
        }
    } else {
        const dim3 grid(pope_grid_for((long long)rows * (kp / 8)));
        if (plain) hipLaunchKernelGGL(sam_im2col_kernel<true>, grid, dim3(256), 0, stream, q.image, static_cast<_Float16*>(big), B, w.img, w.patch, flag);
        else hipLaunchKernelGGL(sam_im2col_kernel<false>, grid, dim3(256), 0, stream, q.image, static_cast<_Float16*>(big), B, w.img, w.patch, flag);
        POPE_TRY(pope_check_launch());
        POPE_TRY(linear(big, w.patch_wp, w.patch_b, x, nullptr, dim, kp, pe_epi, pe_gamma, w.pos, w.pos ? g * g : 0));
        // the attention operands' block-independent parts, once per pass and geometry in use
        for (int s = 0; s < 2; ++s)
            if (use[s]) POPE_TRY(pope_sam_attn_prepare(L.plan[s], ops[s], plain, stream));
    }
    for (int i = 0; i < w.depth; ++i) {
        const pope_sam_block_weights& k = w.blocks_host[i];
        // x = x + attn(norm1(x))                                         image_encoder.py:166-179
        POPE_TRY(norm(k.norm1_w, k.norm1_b));
        POPE_TRY(attention(k, (k.global_attn || w.window <= 0) ? 1 : 0));
        POPE_TRY(linear(att, k.proj_wp, k.proj_b, x, nullptr, dim, dim, EPI_BIAS_LS_RES, w.ones, x, 0));
        // x = x + mlp(norm2(x))                                          image_encoder.py:181; common.py:13-25
        POPE_TRY(norm(k.norm2_w, k.norm2_b));
        POPE_TRY(linear(xn, k.fc1_wp, k.fc1_b, nullptr, big, hidden, dim, EPI_BIAS_GELU, nullptr, nullptr, 0));
        POPE_TRY(linear(big, k.fc2_wp, k.fc2_b, x, nullptr, dim, hidden, EPI_BIAS_LS_RES, w.ones, x, 0));
        for (int t = 0; t < q.n_taps; ++t)
            if (q.tap_blocks[t] == i && q.tap_out[t] &&
                hipMemcpyAsync(q.tap_out[t], x, size_t(rows) * dim * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess)
                return POPE_ERR_LAUNCH;
    }
    // neck (image_encoder.py:89-105): 1x1 conv (no bias) -> LayerNorm2d -> 3x3 conv pad 1 (no bias) -> LayerNorm2d
    POPE_TRY(to_operand());
    POPE_TRY(linear(f32 ? static_cast<const void*>(x) : xn, w.neck0_wp, nullptr, t1, nullptr, oc, dim, EPI_BIAS, nullptr, nullptr, 0));
    POPE_TRY(norm2d_operand());
    POPE_TRY(conv3x3());
    return norm2d_out();
}
