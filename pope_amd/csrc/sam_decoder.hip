// SAM mask decoder (segment_anything/modeling/{mask_decoder,transformer}.py) for point and box prompts on gfx950.
//
// Image side (4 096 tokens per prompt): every Linear is a planes GEMM (pope_launch_gemm_planes; POPE_PREC_F32_MFMA: the fp32
// GEMM), fed by the planes this file's kernels emit.  Token side (<= 16 tokens per prompt): fp32 vector kernels.  The
// residual stream, softmax and LayerNorm statistics are fp32 everywhere.  Per layer and prompt:
//   keys (fp32 [4096, 256]) -> planes(keys), planes(keys + pe)                       (sd_prep / sd_res_ln emit)
//   [t2i.k | i2t.q] = planes(keys + pe) . W^T   (one GEMM, N = 256: both read keys + pe)
//   t2i.v           = planes(keys) . W^T          (N = 128)
//   tokens: self-attention, token->image attention (sd_t2i_attn), MLP (ReLU), i2t k / v
//   image->token attention (sd_i2t_attn) -> planes -> out_proj GEMM -> + keys, norm4     (sd_res_ln)
// Layer 0 with a broadcast dense embedding (batch stride 0): keys = image + dense depends on the image alone, so its two
// projections run once per image and call, and the per-prompt kernels read them at the image of their prompt (SdImageOf: a
// chunk's image indices, a kernel argument by value).  pope_sam_decoder_forward_images_f32 is that path over several images:
// the chunks fill across images, and a prompt's arithmetic does not know which other images the call holds.
// Upscaling: ConvTranspose 2x2/2 (256 -> 64) as a GEMM with N = 4 taps x 64 (row = pixel of the 64 x 64 grid, column =
// tap * 64 + channel), then sd_tail: LayerNorm2d + GELU, the second ConvTranspose (64 -> 32) + GELU and the dot with the 4
// hypernetwork vectors per prompt, written straight into low_res_masks.
// Every per-prompt result is computed by the same threads in the same order whatever the batch and chunk: prompts are
// batch-invariant bit for bit.
#include "common.h"
#include "kernels.h"
#include "linear.h"

namespace {

constexpr int D = 256;          // transformer_dim
constexpr int NPIX = 4096;      // 64 x 64 image tokens
constexpr int GRID = 64;
constexpr int DI = 128;         // internal dim of the cross attentions (downsample 2): 8 heads x 16
constexpr int MLP = 2048;
constexpr int NMASK = 4;
constexpr int NBASE = 1 + NMASK;   // iou token + mask tokens
constexpr int MAX_SPARSE = 11;
constexpr int MAX_T = NBASE + MAX_SPARSE;
constexpr int CHUNK = 16;        // prompts per pass over the image side (workspace ~ 24 MB per prompt)
constexpr int HDC = 16;          // head dim of the cross attentions
constexpr int HDS = 32;          // head dim of the self attention
constexpr int HEADS = 8;

// one value into an activation planes tensor [rows, ld] (layout: kernels.h GemmParams::a_pl), scale 8
__device__ __forceinline__ void sd_put_planes(_Float16* pl, int ld, size_t row, int c, float v, bool& bad) {
    const float y = v * K_PLANES_ACT_SCALE;
    bad |= !(__builtin_fabsf(y) < POPE_F16_OVERFLOW);
    pope_planes_store(pl + row * 2 * ld, c, y);
}

// the GEMM operands of a keys row: A = keys (planes; f32: the fp32 keys themselves, nothing to write), B = keys + pe
__device__ __forceinline__ void sd_emit(void* opA, void* opB, bool f32, size_t row, int c, float x, float pe, bool& bad) {
    const float xp = x + pe;
    if (f32) {
        static_cast<float*>(opB)[row * D + c] = xp;
    } else {
        sd_put_planes(static_cast<_Float16*>(opA), D, row, c, x, bad);
        sd_put_planes(static_cast<_Float16*>(opB), D, row, c, xp, bad);
    }
}

// the layer-0 tensors a chunk's prompts read: slot i[p] of the per-image (or, past layer 0, per-prompt: i[p] = p) buffers
struct SdImageOf {
    int i[CHUNK];
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o));
    return v;
}

// src = image + dense (image_embeddings / image_pe / dense are channel-major [256, 4096]; block z reads the image at z * is
// and the dense embedding at z * ds: prompts of one image (is 0) or images under a broadcast (ds 0)) ->
// keys [nz, 4096, 256] fp32 + operands; pe_t [4096, 256] = image_pe transposed (block z == 0 writes it)
__global__ __launch_bounds__(256) void sd_prep_kernel(const float* __restrict__ img, long long is, const float* __restrict__ pe,
                                                      const float* __restrict__ dense, long long ds, float* __restrict__ keys,
                                                      void* opA, void* opB, int f32, float* __restrict__ pe_t, unsigned* flag) {
    __shared__ float ti[32][33], tp[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32, p = blockIdx.z;
    const float* dp = dense + p * ds;
    const float* ip = img + p * is;
    for (int i = ty; i < 32; i += 8) {
        const size_t e = size_t(c0 + i) * NPIX + n0 + tx;
        ti[i][tx] = ip[e] + dp[e];
        tp[i][tx] = pe[e];
    }
    __syncthreads();
    bool bad = false;
    for (int i = ty; i < 32; i += 8) {
        const int n = n0 + i, c = c0 + tx;
        const float x = ti[tx][i], q = tp[tx][i];
        const size_t row = size_t(p) * NPIX + n;
        keys[row * D + c] = x;
        if (p == 0) pe_t[size_t(n) * D + c] = q;
        sd_emit(opA, opB, f32, row, c, x, q, bad);
    }
    pope_range_flag(flag, POPE_RANGE_LAYERNORM, bad);
}

// keys[p, n] = LayerNorm(res[im.i[p] * rps + n] + y[p, n]) (norm4, eps) and its operands; one wave per row, 4 columns per
// lane; a block's 4 rows are of one prompt (4 | 4 096)
__global__ __launch_bounds__(256) void sd_res_ln_kernel(const float* res, long long rps, SdImageOf im, const float* __restrict__ y,
                                                        const float* __restrict__ w, const float* __restrict__ b, float eps,
                                                        const float* __restrict__ pe_t, float* keys, void* opA, void* opB, int f32,
                                                        int rows, unsigned* flag) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int p = blockIdx.x / (NPIX / 4), n = row - p * NPIX;
    const int c = lane * 4;
    const f32x4 r = *reinterpret_cast<const f32x4*>(res + im.i[p] * rps + size_t(n) * D + c);
    const f32x4 a = *reinterpret_cast<const f32x4*>(y + size_t(row) * D + c);
    const f32x4 x = r + a;
    const float mean = wave_sum((x[0] + x[1]) + (x[2] + x[3])) * (1.f / D);
    const f32x4 d = x - mean;
    const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.f / D);
    const float rstd = 1.f / __builtin_sqrtf(var + eps);
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c), bv = *reinterpret_cast<const f32x4*>(b + c);
    const f32x4 pv = *reinterpret_cast<const f32x4*>(pe_t + size_t(n) * D + c);
    f32x4 o;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[i] = (d[i] * rstd) * wv[i] + bv[i];
        sd_emit(opA, opB, f32 != 0, row, c + i, o[i], pv[i], bad);
    }
    *reinterpret_cast<f32x4*>(keys + size_t(row) * D + c) = o;
    pope_range_flag(flag, POPE_RANGE_LAYERNORM, bad);
}

// token rows: out = LayerNorm(x) * w + b, eps; one wave per row
__global__ __launch_bounds__(256) void sd_ln_tok_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ w,
                                                        const float* __restrict__ b, float eps, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int c = lane * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + size_t(row) * D + c);
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.f / D);
    const f32x4 d = v - mean;
    const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.f / D);
    const float rstd = 1.f / __builtin_sqrtf(var + eps);
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c), bv = *reinterpret_cast<const f32x4*>(b + c);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (d[i] * rstd) * wv[i] + bv[i];
    *reinterpret_cast<f32x4*>(out + size_t(row) * D + c) = o;
}

// token-side Linear: Y[m, n] = act(sum_k X'[m, k] W[n, k] + bias[n]) (+ res[m, n]), X' = X + ADD for the columns n < add_cols
// (q / k read tokens + pe, v the tokens).  4 rows per block, one column per thread, k in order.
constexpr int LIN_ROWS = 4;
__global__ __launch_bounds__(256) void sd_lin_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ ADD, int ldadd,
                                                     int add_cols, const float* __restrict__ W, const float* __restrict__ bias,
                                                     const float* __restrict__ res, int ldres, float* __restrict__ Y, int ldy, int M,
                                                     int N, int K, int relu) {
    extern __shared__ float xs[];   // [LIN_ROWS][K] X, then [LIN_ROWS][K] X + ADD
    const int m0 = blockIdx.y * LIN_ROWS, n = blockIdx.x * 256 + threadIdx.x;
    const int nr = M - m0 < LIN_ROWS ? M - m0 : LIN_ROWS;
    for (int i = threadIdx.x; i < nr * K; i += 256) {
        const int r = i / K, k = i - r * K;
        const float v = X[size_t(m0 + r) * ldx + k];
        xs[i] = v;
        if (ADD) xs[LIN_ROWS * K + i] = v + ADD[size_t(m0 + r) * ldadd + k];
    }
    __syncthreads();
    if (n >= N) return;
    const float* xr = (ADD && n < add_cols) ? xs + LIN_ROWS * K : xs;
    const float* wr = W + size_t(n) * K;
    float acc[LIN_ROWS] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k += 4) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
#pragma unroll
        for (int r = 0; r < LIN_ROWS; ++r) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[r] = __builtin_fmaf(xr[r * K + k + j], wv[j], acc[r]);
        }
    }
    for (int r = 0; r < nr; ++r) {
        float v = acc[r] + bias[n];
        if (relu) v = __builtin_fmaxf(v, 0.f);
        if (res) v = res[size_t(m0 + r) * ldres + n] + v;
        Y[size_t(m0 + r) * ldy + n] = v;
    }
}

// token self-attention (8 heads of 32) of one (head, prompt): qkv [R, 768] = q | k | v, out [R, 256]
__global__ __launch_bounds__(64) void sd_self_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, float scale) {
    const int h = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    if (t >= T) return;
    const float* base = qkv + size_t(p) * T * 3 * D;
    const float* q = base + size_t(t) * 3 * D + h * HDS;
    float s[MAX_T];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < MAX_T; ++j) {
        if (j < T) {
            const float* k = base + size_t(j) * 3 * D + D + h * HDS;
            float a = 0.f;
            for (int d = 0; d < HDS; ++d) a = __builtin_fmaf(q[d], k[d], a);
            s[j] = a / scale;
            m = __builtin_fmaxf(m, s[j]);
        }
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_T; ++j) {
        if (j < T) {
            s[j] = __expf(s[j] - m);
            l += s[j];
        }
    }
    float o[HDS];
#pragma unroll
    for (int d = 0; d < HDS; ++d) o[d] = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_T; ++j) {
        if (j < T) {
            const float* v = base + size_t(j) * 3 * D + 2 * D + h * HDS;
#pragma unroll
            for (int d = 0; d < HDS; ++d) o[d] = __builtin_fmaf(s[j], v[d], o[d]);
        }
    }
    float* op = out + (size_t(p) * T + t) * D + h * HDS;
#pragma unroll
    for (int d = 0; d < HDS; ++d) op[d] = o[d] / l;
}

// token -> image attention of one (head, prompt): q [R, 128] (tokens), K rows of ld ldk at K + im.i[p] * kps, V rows of ld
// 128 at V + im.i[p] * vps (layer 0 under a broadcast: the projections of the prompt's image), out [R, 128].  Each thread owns
// keys tid + 256 i.
__global__ __launch_bounds__(256) void sd_t2i_attn_kernel(const float* __restrict__ q, const float* __restrict__ K, int ldk, long long kps,
                                                          const float* __restrict__ V, long long vps, SdImageOf im,
                                                          float* __restrict__ out, int T) {
    __shared__ float qs[MAX_T][HDC];
    __shared__ float sc[NPIX];
    __shared__ float red[4][HDC + 1];
    __shared__ float bc;
    const int h = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    for (int i = tid; i < T * HDC; i += 256) qs[i / HDC][i % HDC] = q[(size_t(p) * T + i / HDC) * DI + h * HDC + i % HDC];
    __syncthreads();
    const float* kb = K + im.i[p] * kps + h * HDC;
    const float* vb = V + im.i[p] * vps + h * HDC;
    for (int t = 0; t < T; ++t) {
        float m = -INFINITY;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const float* kr = kb + size_t(tid + 256 * i) * ldk;
            float a = 0.f;
#pragma unroll
            for (int d4 = 0; d4 < HDC; d4 += 4) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + d4);
#pragma unroll
                for (int j = 0; j < 4; ++j) a = __builtin_fmaf(qs[t][d4 + j], kv[j], a);
            }
            sc[tid + 256 * i] = a * 0.25f;   // / sqrt(16); each thread reads back only its own scores
            m = __builtin_fmaxf(m, sc[tid + 256 * i]);
        }
        m = wave_max(m);
        if (lane == 0) red[wv][0] = m;
        __syncthreads();
        if (tid == 0) bc = __builtin_fmaxf(__builtin_fmaxf(red[0][0], red[1][0]), __builtin_fmaxf(red[2][0], red[3][0]));
        __syncthreads();
        m = bc;
        float l = 0.f, acc[HDC];
#pragma unroll
        for (int d = 0; d < HDC; ++d) acc[d] = 0.f;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const float e = __expf(sc[tid + 256 * i] - m);
            l += e;
            const float* vr = vb + size_t(tid + 256 * i) * DI;
#pragma unroll
            for (int d4 = 0; d4 < HDC; d4 += 4) {
                const f32x4 vv = *reinterpret_cast<const f32x4*>(vr + d4);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[d4 + j] = __builtin_fmaf(e, vv[j], acc[d4 + j]);
            }
        }
        l = wave_sum(l);
#pragma unroll
        for (int d = 0; d < HDC; ++d) acc[d] = wave_sum(acc[d]);
        if (lane == 0) {
            red[wv][HDC] = l;
#pragma unroll
            for (int d = 0; d < HDC; ++d) red[wv][d] = acc[d];
        }
        __syncthreads();
        if (tid < HDC) {
            const float lt = (red[0][HDC] + red[1][HDC]) + (red[2][HDC] + red[3][HDC]);
            const float at = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
            out[(size_t(p) * T + t) * DI + h * HDC + tid] = at / lt;
        }
        __syncthreads();
    }
}

// image -> token attention: 4 096 queries of a prompt (Q rows of ld 256 at Q + im.i[p] * qps) against its T tokens
// (kv [R, 256] = k | v); thread = (pixel, head); out [np * 4096, 128] as planes, or fp32 (f32)
__global__ __launch_bounds__(256) void sd_i2t_attn_kernel(const float* __restrict__ Q, long long qps, SdImageOf im,
                                                          const float* __restrict__ kv, int T,
                                                          void* out, int f32, unsigned* flag) {
    __shared__ float ks[MAX_T * D];
    const int p = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < T * D; i += 256) ks[i] = kv[size_t(p) * T * D + i];
    __syncthreads();
    const int n = blockIdx.x * 32 + (tid >> 3), h = tid & 7;
    const float* qr = Q + im.i[p] * qps + size_t(n) * D + h * HDC;
    float qv[HDC];
#pragma unroll
    for (int d4 = 0; d4 < HDC; d4 += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(qr + d4);
#pragma unroll
        for (int j = 0; j < 4; ++j) qv[d4 + j] = v[j];
    }
    float s[MAX_T];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < MAX_T; ++t) {
        if (t < T) {
            const float* kr = ks + t * D + h * HDC;
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < HDC; ++d) a = __builtin_fmaf(qv[d], kr[d], a);
            s[t] = a * 0.25f;   // / sqrt(16)
            m = __builtin_fmaxf(m, s[t]);
        }
    }
    float l = 0.f, o[HDC];
#pragma unroll
    for (int d = 0; d < HDC; ++d) o[d] = 0.f;
#pragma unroll
    for (int t = 0; t < MAX_T; ++t) {
        if (t < T) {
            const float e = __expf(s[t] - m);
            l += e;
            const float* vr = ks + t * D + DI + h * HDC;
#pragma unroll
            for (int d = 0; d < HDC; ++d) o[d] = __builtin_fmaf(e, vr[d], o[d]);
        }
    }
    const size_t row = size_t(p) * NPIX + n;
    bool bad = false;
    if (f32) {
        float* orow = static_cast<float*>(out) + row * DI + h * HDC;
#pragma unroll
        for (int d = 0; d < HDC; ++d) orow[d] = o[d] / l;
    } else {
#pragma unroll
        for (int d = 0; d < HDC; ++d) sd_put_planes(static_cast<_Float16*>(out), DI, row, h * HDC + d, o[d] / l, bad);
    }
    pope_range_flag(flag, POPE_RANGE_QKV, bad);
}

// iou token + mask tokens, then the prompt's sparse embeddings: queries = point_embedding = tokens [R, 256]
__global__ __launch_bounds__(256) void sd_tokens_kernel(const float* __restrict__ base, const float* __restrict__ sparse, int ns, int T,
                                                        int R, float* __restrict__ qry, float* __restrict__ tpe) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * D) return;
    const int r = i / D, c = i - r * D, p = r / T, t = r - p * T;
    const float v = t < NBASE ? base[t * D + c] : sparse[(size_t(p) * ns + (t - NBASE)) * D + c];
    qry[i] = v;
    tpe[i] = v;
}

// the upscaling tail of one intermediate pixel (64-grid pixel n, first-ConvTranspose tap): y [np * 4096, 256] = first
// ConvTranspose + bias (column tap * 64 + channel) -> LayerNorm2d(64, eps) -> GELU -> second ConvTranspose (w2 [4 * 32][64]:
// row tap2 * 32 + c, column = input channel) + b2 -> GELU -> dot with hyper [np][4][32] for masks m0 .. m0 + C - 1 -> masks [np][C][256][256]
__global__ __launch_bounds__(256) void sd_tail_kernel(const float* __restrict__ y, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                      float eps, const float* __restrict__ w2, const float* __restrict__ b2,
                                                      const float* __restrict__ hyper, int m0, int C, float* __restrict__ masks) {
    __shared__ __attribute__((aligned(16))) float ws[128 * 64];
    __shared__ float hs[NMASK * 32];
    __shared__ float bs[32], lw[64], lb[64];
    const int p = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 64 * 128; i += 256) ws[i] = w2[i];
    if (tid < NMASK * 32) hs[tid] = hyper[size_t(p) * NMASK * 32 + tid];
    if (tid < 32) bs[tid] = b2[tid];
    if (tid < 64) {
        lw[tid] = lnw[tid];
        lb[tid] = lnb[tid];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + tid, n = i >> 2, tap1 = i & 3;
    const float* src = y + (size_t(p) * NPIX + n) * D + tap1 * 64;
    float u[64];
#pragma unroll
    for (int c4 = 0; c4 < 64; c4 += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + c4);
#pragma unroll
        for (int j = 0; j < 4; ++j) u[c4 + j] = v[j];
    }
    float mean = 0.f;
#pragma unroll
    for (int c = 0; c < 64; ++c) mean += u[c];
    mean *= (1.f / 64);
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < 64; ++c) var = __builtin_fmaf(u[c] - mean, u[c] - mean, var);
    var *= (1.f / 64);
    const float rstd = 1.f / __builtin_sqrtf(var + eps);
#pragma unroll
    for (int c = 0; c < 64; ++c) u[c] = pope_gelu_erf(lw[c] * ((u[c] - mean) * rstd) + lb[c]);
    const int gy = n / GRID, gx = n - gy * GRID;
    const int Y = 2 * gy + (tap1 >> 1), X = 2 * gx + (tap1 & 1);
    for (int tap2 = 0; tap2 < 4; ++tap2) {
        float mk[NMASK] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < 32; ++c) {
            const float* wc = ws + (tap2 * 32 + c) * 64;
            float a = 0.f;
#pragma unroll
            for (int ci = 0; ci < 64; ci += 4) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wc + ci);
#pragma unroll
                for (int j = 0; j < 4; ++j) a = __builtin_fmaf(u[ci + j], wv[j], a);
            }
            const float g = pope_gelu_erf(a + bs[c]);
#pragma unroll
            for (int m = 0; m < NMASK; ++m) mk[m] = __builtin_fmaf(hs[m * 32 + c], g, mk[m]);
        }
        const int oy = 2 * Y + (tap2 >> 1), ox = 2 * X + (tap2 & 1);
        for (int m = 0; m < C; ++m) masks[(size_t(p) * C + m) * (4 * GRID * 4 * GRID) + oy * (4 * GRID) + ox] = mk[m0 + m];
    }
}

struct Ws {
    char* p;
    size_t off = 0;
    template <typename T>
    T* take(size_t elems) {
        T* r = reinterpret_cast<T*>(p ? p + off : nullptr);
        off += pope_align256(elems * sizeof(T));
        return r;
    }
};

struct Buffers {
    float *pe_t, *keys0, *qk0, *v0;
    void *opA0, *opB0;
    float *keys, *qk, *v, *y;
    void *opA, *opB, *att;
    float *qry, *tpe, *tmp, *tatt, *tqkv, *th, *tq, *tkv, *h1, *h2, *hyper;
};

// n_img > 0: the layer-0 buffers of n_img images (a broadcast dense embedding)
Buffers carve(char* base, int cp, int T, int n_img, size_t* total) {
    Ws w{base};
    Buffers b{};
    const size_t img = size_t(NPIX) * D;
    b.pe_t = w.take<float>(img);
    if (n_img > 0) {
        b.keys0 = w.take<float>(img * n_img);
        b.opA0 = w.take<float>(img * n_img);
        b.opB0 = w.take<float>(img * n_img);
        b.qk0 = w.take<float>(img * n_img);
        b.v0 = w.take<float>(size_t(NPIX) * DI * n_img);
    }
    b.keys = w.take<float>(img * cp);
    b.opA = w.take<float>(img * cp);   // planes of [rows, 256]: 4 bytes per element, like fp32
    b.opB = w.take<float>(img * cp);
    b.qk = w.take<float>(img * cp);
    b.v = w.take<float>(size_t(NPIX) * DI * cp);
    b.att = w.take<float>(size_t(NPIX) * DI * cp);
    b.y = w.take<float>(img * cp);
    const size_t R = size_t(T) * cp;
    b.qry = w.take<float>(R * D);
    b.tpe = w.take<float>(R * D);
    b.tmp = w.take<float>(R * D);
    b.tatt = w.take<float>(R * D);
    b.tqkv = w.take<float>(R * 3 * D);
    b.th = w.take<float>(R * MLP);
    b.tq = w.take<float>(R * DI);
    b.tkv = w.take<float>(R * D);
    b.h1 = w.take<float>(size_t(cp) * D);
    b.h2 = w.take<float>(size_t(cp) * D);
    b.hyper = w.take<float>(size_t(cp) * NMASK * 32);
    *total = w.off;
    return b;
}

struct Ctx {
    bool f32;
    unsigned* flag;
    hipStream_t s;
};

// C[M, N] = A . W^T + bias over K: planes GEMM (A activation planes, W weight planes) or, f32, the fp32 GEMM
int gemm(const Ctx& c, const void* A, const void* W, const float* bias, float* C, int M, int N, int K) {
    GemmParams g = pope_linear_params(c.f32 ? LINEAR_F32 : LINEAR_PLANES, A, W, bias, C, nullptr, M, N, K, EPI_BIAS, nullptr, nullptr, 0,
                                      c.f32 ? nullptr : c.flag);
    g.ldres = 0; g.range_bit = 0;   // no residual; an fp32 output reports no range
    return c.f32 ? pope_launch_gemm_nt_f32(g, c.s) : pope_launch_gemm_planes(g, c.s);
}

int lin(const Ctx& c, const float* X, int ldx, const float* add, int add_cols, const float* W, const float* b, const float* res,
        float* Y, int ldy, int M, int N, int K, bool relu) {
    return pope_launch_sam_decoder_token_linear(X, ldx, add, add_cols, W, b, res, Y, ldy, M, N, K, relu ? 1 : 0, c.s);
}

int ln_tok(const Ctx& c, const float* x, float* out, const float* w, const float* b, float eps, int rows) {
    hipLaunchKernelGGL(sd_ln_tok_kernel, dim3((rows + 3) / 4), dim3(256), 0, c.s, x, out, w, b, eps, rows);
    return pope_check_launch();
}

int t2i(const Ctx& c, const float* q, const float* K, int ldk, long long kps, const float* V, long long vps, const SdImageOf& im,
        float* out, int T, int np) {
    hipLaunchKernelGGL(sd_t2i_attn_kernel, dim3(HEADS, np), dim3(256), 0, c.s, q, K, ldk, kps, V, vps, im, out, T);
    return pope_check_launch();
}

int self_attn(const Ctx& c, const float* qkv, float* out, int T, int np) {
    hipLaunchKernelGGL(sd_self_attn_kernel, dim3(HEADS, np), dim3(64), 0, c.s, qkv, out, T, __builtin_sqrtf(float(HDS)));
    return pope_check_launch();
}

// out: planes [np * 4096, 128], or fp32 (c.f32)
int i2t(const Ctx& c, const float* Q, long long qps, const SdImageOf& im, const float* kv, int T, void* out, int np) {
    hipLaunchKernelGGL(sd_i2t_attn_kernel, dim3(NPIX / 32, np), dim3(256), 0, c.s, Q, qps, im, kv, T, out, c.f32 ? 1 : 0, c.flag);
    return pope_check_launch();
}

int res_ln(const Ctx& c, const float* res, long long rps, const SdImageOf& im, const float* y, const float* w, const float* b, float eps,
           const float* pe_t, float* keys, void* opA, void* opB, int np) {
    const int rows = np * NPIX;
    hipLaunchKernelGGL(sd_res_ln_kernel, dim3(rows / 4), dim3(256), 0, c.s, res, rps, im, y, w, b, eps, pe_t, keys, opA, opB,
                       c.f32 ? 1 : 0, rows, c.flag);
    return pope_check_launch();
}

int prep(const Ctx& c, const float* img, long long is, const float* pe, const float* dense, long long ds, float* keys, void* opA,
         void* opB, float* pe_t, int nz) {
    hipLaunchKernelGGL(sd_prep_kernel, dim3(NPIX / 32, D / 32, nz), dim3(256), 0, c.s, img, is, pe, dense, ds, keys, opA, opB,
                       c.f32 ? 1 : 0, pe_t, c.flag);
    return pope_check_launch();
}

int tail(const Ctx& c, const float* y, const float* lnw, const float* lnb, float eps, const float* w2, const float* b2,
         const float* hyper, bool multimask, int np, float* masks) {
    const int C = multimask ? NMASK - 1 : 1, m0 = multimask ? 1 : 0;
    hipLaunchKernelGGL(sd_tail_kernel, dim3(NPIX * 4 / 256, np), dim3(256), 0, c.s, y, lnw, lnb, eps, w2, b2, hyper, m0, C, masks);
    return pope_check_launch();
}

bool geometry_ok(const pope_sam_decoder_weights* w) {
    return w && w->dim == D && w->heads == HEADS && w->mlp_dim == MLP && w->depth == 2 && w->grid == GRID &&
           w->num_mask_tokens == NMASK && w->iou_hidden == D && w->iou_depth == 3 && w->layers_host &&
           (w->precision == POPE_PREC_F16X3 || w->precision == POPE_PREC_F32_MFMA);
}

bool weights_ok(const pope_sam_decoder_weights* w) {
    const void* top[] = {w->tokens, w->fin_q_w, w->fin_q_b, w->fin_k_wp, w->fin_k_b, w->fin_v_wp, w->fin_v_b, w->fin_o_w,
                         w->fin_o_b, w->norm_final_w, w->norm_final_b, w->up1_wp, w->up1_b, w->up_ln_w, w->up_ln_b, w->up2_w,
                         w->up2_b};
    for (const void* p : top)
        if (!p) return false;
    for (int i = 0; i < 3 * NMASK; ++i)
        if (!w->hyper_w[i] || !w->hyper_b[i]) return false;
    for (int i = 0; i < 3; ++i)
        if (!w->iou_w[i] || !w->iou_b[i]) return false;
    for (int l = 0; l < 2; ++l) {
        const pope_sam_decoder_layer_weights& L = w->layers_host[l];
        const void* lp[] = {L.sa_qkv_w, L.sa_qkv_b, L.sa_o_w, L.sa_o_b, L.norm1_w, L.norm1_b, L.t2i_q_w, L.t2i_q_b, L.t2i_o_w,
                            L.t2i_o_b, L.norm2_w, L.norm2_b, L.mlp1_w, L.mlp1_b, L.mlp2_w, L.mlp2_b, L.norm3_w, L.norm3_b,
                            L.i2t_kv_w, L.i2t_kv_b, L.img_qk_wp, L.img_qk_b, L.img_v_wp, L.img_v_b, L.i2t_o_wp, L.i2t_o_b,
                            L.norm4_w, L.norm4_b};
        for (const void* p : lp)
            if (!p) return false;
    }
    return true;
}

}  // namespace

size_t pope_sam_decoder_workspace(const pope_sam_decoder_weights* w, int P, int n_sparse, int shared) {
    if (!geometry_ok(w) || P <= 0 || n_sparse < 0 || n_sparse > MAX_SPARSE) return 0;
    size_t total = 0;
    carve(nullptr, P < CHUNK ? P : CHUNK, NBASE + n_sparse, shared ? 1 : 0, &total);
    return total;
}

size_t pope_sam_decoder_images_workspace(const pope_sam_decoder_weights* w, int n_images, const int* prompt_image, int P, int n_sparse,
                                         long long dense_stride) {
    if (!geometry_ok(w) || n_images <= 0 || !prompt_image || P <= 0 || n_sparse < 0 || n_sparse > MAX_SPARSE) return 0;
    if (dense_stride != 0) return 0;   // the broadcast only
    for (int p = 0; p < P; ++p)
        if (prompt_image[p] < 0 || prompt_image[p] >= n_images) return 0;
    size_t total = 0;
    carve(nullptr, P < CHUNK ? P : CHUNK, NBASE + n_sparse, n_images, &total);
    return total;
}

int pope_launch_sam_decoder(const SamDecArgs& a, hipStream_t stream) {
    const pope_sam_decoder_weights* w = a.w;
    if (!geometry_ok(w) || !weights_ok(w)) return POPE_ERR_ARG;
    if (a.P <= 0 || a.n_sparse < 0 || a.n_sparse > MAX_SPARSE || (a.n_sparse > 0 && !a.sparse)) return POPE_ERR_ARG;
    if (!a.image || !a.image_pe || !a.dense || !a.masks || !a.iou || !a.ws) return POPE_ERR_ARG;
    if (a.dense_stride != 0 && a.dense_stride != (long long)D * NPIX) return POPE_ERR_ARG;
    const bool shared = a.dense_stride == 0;
    // several images (prompt_image: prompt -> image): the broadcast only, and before any launch no index outside the images
    const int NI = a.prompt_image ? a.n_images : 1;
    if (a.prompt_image && (a.hs_out || a.keys_out ||
                           pope_sam_decoder_images_workspace(w, NI, a.prompt_image, a.P, a.n_sparse, a.dense_stride) == 0))
        return POPE_ERR_ARG;
    const int T = NBASE + a.n_sparse, cp_max = a.P < CHUNK ? a.P : CHUNK;
    size_t need = 0;
    const Buffers B = carve(static_cast<char*>(a.ws), cp_max, T, shared ? NI : 0, &need);
    if (a.ws_bytes < need) return POPE_ERR_WORKSPACE;
    const Ctx c{w->precision == POPE_PREC_F32_MFMA, a.range_flag, stream};
    const float teps = w->token_eps, ueps = w->up_eps;
    const int C = a.multimask ? NMASK - 1 : 1, m0 = a.multimask ? 1 : 0;
    const size_t img = size_t(NPIX) * D;

    SdImageOf own{}, im0{};   // a prompt's own slot of the per-prompt buffers; layer 0 under a broadcast: its image (0: the one image)
    for (int p = 0; p < CHUNK; ++p) own.i[p] = p;
    // layer 0's image-only projections, once per image and call; at most CHUNK images per GEMM: the row counts of the
    // per-prompt GEMMs below, whose rows do not depend on the rows beside them
    for (int i0 = 0; shared && i0 < NI; i0 += CHUNK) {
        const int ni = NI - i0 < CHUNK ? NI - i0 : CHUNK;
        const size_t o = size_t(i0) * img, ov = size_t(i0) * NPIX * DI;
        float* keys0 = B.keys0 + o;
        void* opA0 = static_cast<float*>(B.opA0) + o;   // planes of [rows, 256]: 4 bytes per element, like fp32
        void* opB0 = static_cast<float*>(B.opB0) + o;
        POPE_TRY(prep(c, a.image + o, (long long)img, a.image_pe, a.dense, 0LL, keys0, opA0, opB0, B.pe_t, ni));
        const void* A0 = c.f32 ? static_cast<const void*>(keys0) : opA0;
        POPE_TRY(gemm(c, opB0, w->layers_host[0].img_qk_wp, w->layers_host[0].img_qk_b, B.qk0 + o, ni * NPIX, D, D));
        POPE_TRY(gemm(c, A0, w->layers_host[0].img_v_wp, w->layers_host[0].img_v_b, B.v0 + ov, ni * NPIX, DI, D));
    }
    const void* opA = c.f32 ? static_cast<const void*>(B.keys) : B.opA;
    for (int pg0 = 0; pg0 < a.P; pg0 += CHUNK) {
        const int cp = a.P - pg0 < CHUNK ? a.P - pg0 : CHUNK, R = T * cp, rows = cp * NPIX;
        if (a.prompt_image)
            for (int p = 0; p < cp; ++p) im0.i[p] = a.prompt_image[pg0 + p];
        hipLaunchKernelGGL(sd_tokens_kernel, dim3((R * D + 255) / 256), dim3(256), 0, stream, w->tokens,
                           a.n_sparse ? a.sparse + size_t(pg0) * a.n_sparse * D : nullptr, a.n_sparse, T, R, B.qry, B.tpe);
        POPE_TRY(pope_check_launch());
        if (!shared)
            POPE_TRY(prep(c, a.image, 0LL, a.image_pe, a.dense + pg0 * a.dense_stride, a.dense_stride, B.keys, B.opA, B.opB, B.pe_t, cp));
        for (int l = 0; l < 2; ++l) {
            const pope_sam_decoder_layer_weights& L = w->layers_host[l];
            const float *qk = B.qk, *v = B.v, *res = B.keys;
            const long long qps = (long long)img, vps = (long long)NPIX * DI, rps = (long long)img;
            const bool first = l == 0 && shared;
            const SdImageOf& im = first ? im0 : own;
            if (first) {
                qk = B.qk0; v = B.v0; res = B.keys0;
            } else {
                POPE_TRY(gemm(c, B.opB, L.img_qk_wp, L.img_qk_b, B.qk, rows, D, D));
                POPE_TRY(gemm(c, opA, L.img_v_wp, L.img_v_b, B.v, rows, DI, D));
            }
            // self-attention; layer 0 (skip_first_layer_pe): no pe, and its output replaces the queries
            POPE_TRY(lin(c, B.qry, D, l ? B.tpe : nullptr, 2 * D, L.sa_qkv_w, L.sa_qkv_b, nullptr, B.tqkv, 3 * D, R, 3 * D, D, false));
            POPE_TRY(self_attn(c, B.tqkv, B.tatt, T, cp));
            POPE_TRY(lin(c, B.tatt, D, nullptr, 0, L.sa_o_w, L.sa_o_b, l ? B.qry : nullptr, B.tmp, D, R, D, D, false));
            POPE_TRY(ln_tok(c, B.tmp, B.qry, L.norm1_w, L.norm1_b, teps, R));
            // tokens -> image
            POPE_TRY(lin(c, B.qry, D, B.tpe, DI, L.t2i_q_w, L.t2i_q_b, nullptr, B.tq, DI, R, DI, D, false));
            POPE_TRY(t2i(c, B.tq, qk, D, qps, v, vps, im, B.tatt, T, cp));
            POPE_TRY(lin(c, B.tatt, DI, nullptr, 0, L.t2i_o_w, L.t2i_o_b, B.qry, B.tmp, D, R, D, DI, false));
            POPE_TRY(ln_tok(c, B.tmp, B.qry, L.norm2_w, L.norm2_b, teps, R));
            // MLP (ReLU)
            POPE_TRY(lin(c, B.qry, D, nullptr, 0, L.mlp1_w, L.mlp1_b, nullptr, B.th, MLP, R, MLP, D, true));
            POPE_TRY(lin(c, B.th, MLP, nullptr, 0, L.mlp2_w, L.mlp2_b, B.qry, B.tmp, D, R, D, MLP, false));
            POPE_TRY(ln_tok(c, B.tmp, B.qry, L.norm3_w, L.norm3_b, teps, R));
            // image -> tokens: k from tokens + pe, v from tokens
            POPE_TRY(lin(c, B.qry, D, B.tpe, DI, L.i2t_kv_w, L.i2t_kv_b, nullptr, B.tkv, D, R, D, D, false));
            POPE_TRY(i2t(c, qk + DI, qps, im, B.tkv, T, B.att, cp));
            POPE_TRY(gemm(c, B.att, L.i2t_o_wp, L.i2t_o_b, B.y, rows, D, DI));
            POPE_TRY(res_ln(c, res, rps, im, B.y, L.norm4_w, L.norm4_b, teps, B.pe_t, B.keys, B.opA, B.opB, cp));
        }
        // final token -> image attention: k into qk (ld 128), v into v
        POPE_TRY(gemm(c, B.opB, w->fin_k_wp, w->fin_k_b, B.qk, rows, DI, D));
        POPE_TRY(gemm(c, opA, w->fin_v_wp, w->fin_v_b, B.v, rows, DI, D));
        POPE_TRY(lin(c, B.qry, D, B.tpe, DI, w->fin_q_w, w->fin_q_b, nullptr, B.tq, DI, R, DI, D, false));
        POPE_TRY(t2i(c, B.tq, B.qk, DI, (long long)NPIX * DI, B.v, (long long)NPIX * DI, own, B.tatt, T, cp));
        POPE_TRY(lin(c, B.tatt, DI, nullptr, 0, w->fin_o_w, w->fin_o_b, B.qry, B.tmp, D, R, D, DI, false));
        POPE_TRY(ln_tok(c, B.tmp, B.qry, w->norm_final_w, w->norm_final_b, teps, R));
        if (a.hs_out && hipMemcpyAsync(a.hs_out + size_t(pg0) * T * D, B.qry, size_t(R) * D * sizeof(float), hipMemcpyDeviceToDevice,
                                       stream) != hipSuccess)
            return POPE_ERR_LAUNCH;
        if (a.keys_out && hipMemcpyAsync(a.keys_out + size_t(pg0) * img, B.keys, size_t(rows) * D * sizeof(float),
                                         hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return POPE_ERR_LAUNCH;
        // hypernetwork MLPs (mask token i -> hyper[:, i]) and the IoU head (iou token -> the C columns the output keeps)
        for (int i = 0; i < NMASK; ++i) {
            POPE_TRY(lin(c, B.qry + (1 + i) * D, T * D, nullptr, 0, w->hyper_w[3 * i], w->hyper_b[3 * i], nullptr, B.h1, D, cp, D, D, true));
            POPE_TRY(lin(c, B.h1, D, nullptr, 0, w->hyper_w[3 * i + 1], w->hyper_b[3 * i + 1], nullptr, B.h2, D, cp, D, D, true));
            POPE_TRY(lin(c, B.h2, D, nullptr, 0, w->hyper_w[3 * i + 2], w->hyper_b[3 * i + 2], nullptr, B.hyper + i * 32, NMASK * 32, cp,
                       32, D, false));
        }
        POPE_TRY(lin(c, B.qry, T * D, nullptr, 0, w->iou_w[0], w->iou_b[0], nullptr, B.h1, D, cp, D, D, true));
        POPE_TRY(lin(c, B.h1, D, nullptr, 0, w->iou_w[1], w->iou_b[1], nullptr, B.h2, D, cp, D, D, true));
        POPE_TRY(lin(c, B.h2, D, nullptr, 0, w->iou_w[2] + size_t(m0) * D, w->iou_b[2] + m0, nullptr, a.iou + size_t(pg0) * C, C, cp, C,
                   D, false));
        // upscaling: first ConvTranspose as a GEMM (N = 4 taps x 64), then the fused tail
        POPE_TRY(gemm(c, opA, w->up1_wp, w->up1_b, B.y, rows, D, D));
        POPE_TRY(tail(c, B.y, w->up_ln_w, w->up_ln_b, ueps, w->up2_w, w->up2_b, B.hyper, a.multimask != 0, cp,
                      a.masks + size_t(pg0) * C * (16 * NPIX)));
    }
    return POPE_OK;
}

// ---- the kernels one at a time (pope_sam_decoder_*_f32): every argument is checked on the host before the launch ----------
namespace {

bool al16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool stride_ok(long long s) { return s >= 0 && s % 4 == 0; }   // rows read as f32x4
bool tokens_ok(int T, int P) { return T >= 1 && T <= MAX_T && P >= 1 && P <= CHUNK; }

// slot_host [P] -> the kernel argument; false: null or a negative slot
bool slots(const int* slot_host, int P, SdImageOf* im) {
    if (!slot_host) return false;
    *im = SdImageOf{};
    for (int p = 0; p < P; ++p) {
        if (slot_host[p] < 0) return false;
        im->i[p] = slot_host[p];
    }
    return true;
}

constexpr size_t LIN_LDS_LIMIT = 64 * 1024;   // dynamic LDS of a launch without an opt-in attribute

}  // namespace

void pope_sam_decoder_seam_values(int* chunk, int* lin_rows, int* max_tokens, int* base_tokens) {
    if (chunk) *chunk = CHUNK;
    if (lin_rows) *lin_rows = LIN_ROWS;
    if (max_tokens) *max_tokens = MAX_T;
    if (base_tokens) *base_tokens = NBASE;
}

// lin()'s convention: ADD rows have the pitch of X, residual rows the pitch of Y
int pope_launch_sam_decoder_token_linear(const float* X, int ldx, const float* add, int add_cols, const float* W, const float* bias,
                                         const float* res, float* Y, int ldy, int M, int N, int K, int relu, hipStream_t stream) {
    if (!X || !al16(W) || !bias || !Y || M <= 0 || N <= 0 || K <= 0 || K % 4 != 0 || ldx < K || ldy < N || add_cols < 0)
        return POPE_ERR_ARG;
    if ((M + LIN_ROWS - 1) / LIN_ROWS > 65535) return POPE_ERR_ARG;
    const size_t lds = size_t(LIN_ROWS) * K * (add ? 2 : 1) * sizeof(float);
    if (lds > LIN_LDS_LIMIT) return POPE_ERR_ARG;
    hipLaunchKernelGGL(sd_lin_kernel, dim3((N + 255) / 256, (M + LIN_ROWS - 1) / LIN_ROWS), dim3(256), lds, stream, X, ldx, add, ldx,
                       add_cols, W, bias, res, ldy, Y, ldy, M, N, K, relu ? 1 : 0);
    return pope_check_launch();
}

int pope_launch_sam_decoder_self_attention(const float* qkv, float* out, int P, int T, hipStream_t stream) {
    if (!qkv || !out || T < 1 || T > MAX_T || P < 1 || P > 65535) return POPE_ERR_ARG;
    return self_attn(Ctx{true, nullptr, stream}, qkv, out, T, P);
}

int pope_launch_sam_decoder_t2i_attention(const float* q, const float* K, int ldk, long long kps, const float* V, long long vps,
                                          const int* slot_host, float* out, int T, int P, hipStream_t stream) {
    SdImageOf im;
    if (!q || !al16(K) || !al16(V) || !out || !tokens_ok(T, P) || ldk < DI || ldk % 4 != 0 || !stride_ok(kps) || !stride_ok(vps) ||
        !slots(slot_host, P, &im))
        return POPE_ERR_ARG;
    return t2i(Ctx{true, nullptr, stream}, q, K, ldk, kps, V, vps, im, out, T, P);
}

int pope_launch_sam_decoder_i2t_attention(const float* Q, long long qps, const int* slot_host, const float* kv, int T, int P,
                                          float* out_f32, void* out_planes, unsigned* range_flag, hipStream_t stream) {
    SdImageOf im;
    if (!al16(Q) || !kv || !tokens_ok(T, P) || !stride_ok(qps) || (out_f32 != nullptr) == (out_planes != nullptr) ||
        !slots(slot_host, P, &im))
        return POPE_ERR_ARG;
    return i2t(Ctx{out_f32 != nullptr, range_flag, stream}, Q, qps, im, kv, T, out_f32 ? static_cast<void*>(out_f32) : out_planes, P);
}

int pope_launch_sam_decoder_residual_norm(const float* res, long long rps, const int* slot_host, const float* y, const float* w,
                                          const float* b, float eps, const float* pe_t, float* keys, void* opA, void* opB, int f32,
                                          int P, unsigned* range_flag, hipStream_t stream) {
    SdImageOf im;
    if (!al16(res) || !al16(y) || !al16(w) || !al16(b) || !al16(pe_t) || !al16(keys) || !opB || (!f32 && !opA) || !(eps >= 0.f) ||
        !stride_ok(rps) || P < 1 || P > CHUNK || !slots(slot_host, P, &im))
        return POPE_ERR_ARG;
    return res_ln(Ctx{f32 != 0, range_flag, stream}, res, rps, im, y, w, b, eps, pe_t, keys, opA, opB, P);
}

int pope_launch_sam_decoder_prepare_keys(const float* image, long long image_stride, const float* image_pe, const float* dense,
                                         long long dense_stride, int nz, float* keys, void* opA, void* opB, int f32, float* pe_t,
                                         unsigned* range_flag, hipStream_t stream) {
    if (!image || !image_pe || !dense || !keys || !pe_t || !opB || (!f32 && !opA) || image_stride < 0 || dense_stride < 0 || nz < 1 ||
        nz > CHUNK)
        return POPE_ERR_ARG;
    return prep(Ctx{f32 != 0, range_flag, stream}, image, image_stride, image_pe, dense, dense_stride, keys, opA, opB, pe_t, nz);
}

int pope_launch_sam_decoder_upscale_tail(const float* y, const float* ln_w, const float* ln_b, float eps, const float* w2,
                                         const float* b2, const float* hyper, int multimask, int P, float* masks, hipStream_t stream) {
    if (!al16(y) || !ln_w || !ln_b || !al16(w2) || !b2 || !hyper || !masks || !(eps >= 0.f) || P < 1 || P > CHUNK) return POPE_ERR_ARG;
    return tail(Ctx{true, nullptr, stream}, y, ln_w, ln_b, eps, w2, b2, hyper, multimask != 0, P, masks);
}
