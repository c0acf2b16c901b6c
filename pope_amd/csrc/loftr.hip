// LoFTR encoder layer (first slice: the coarse and fine `LocalFeatureTransformer`s of the reference
// Matcher) on HIP kernels.  One layer update, src/matcher/loftr_module/transformer.py:35-58 with the linear attention
// of linear_attention.py:20-47:
//     q = x Wq^T ; k = s Wk^T ; v = s Wv^T                       (bias-free, 8 heads x D, D = C / 8)
//     Q = elu(q) + 1 ; K = elu(k) + 1 ; V = v / S                (the reference's /S ... *S is kept: it rounds)
//     KV[h] = K[h]^T V[h]  (D x D per head and image) ; Ksum[h] = sum_s K[s, h]
//     msg = (Q . KV) * 1 / (Q . Ksum + 1e-6) * S
//     msg = LayerNorm(msg Wm^T)  (eps 1e-5)
//     x  <- x + LayerNorm(relu(cat[x, msg] W0^T) W1^T)
// With LoftrLayerParams::attention = POPE_LOFTR_ATTN_FULL the second and third line are the softmax attention of
// linear_attention.py:50-81 instead, msg = softmax(q k^T / sqrt(D)) v per head: one launch (loftr_attention.hip), no masks.
// The five projections run on the f16x3 planes GEMM (gemm_planes.hip: fp32-equivalent arithmetic, bias-free, the MLP's
// ReLU in the epilogue, its output straight to planes); everything around them is small and HBM / launch bound:
// attention is O(L) — the per-head D x D state is reduced over the source rows in chunks (fixed order: deterministic),
// then applied row by row.  The launch sequence lives behind ONE C-ABI call per layer update (capi.hip), so a
// 4 x (self, cross) transformer is 16 calls instead of ~200 torch ops.
#include "common.h"
#include "kernels.h"
#include "linear.h"

namespace {

constexpr int LA_CHUNK = 64;   // source rows per workgroup of the KV reduction
constexpr int LA_ROWS_PER_BLOCK = 16;   // query rows per workgroup of the apply kernel

// elu(x) + 1 as torch evaluates it in fp32: x > 0 ? x : exp(x) - 1, then + 1 (two roundings on the negative side)
__device__ __forceinline__ float elu1(float x) { return (x > 0.f ? x : expf(x) - 1.0f) + 1.0f; }

// Partial KV / Ksum of one (image, head) over one chunk of source rows.  kv: [n, S, 2C] fp32 (k | v).
// part: [n * H, chunks, D * D + D].
// MASKED: kv_mask [n, S] (0 / 1) multiplies K and V before the reduction — K = (elu(k) + 1) * m, V = (v * m) / S with S
// the full length (linear_attention.py:35-41): a padded source row adds nothing to KV and Ksum.
template <int D, bool MASKED>
__global__ __launch_bounds__(256) void linattn_reduce_kernel(const float* __restrict__ kv, int S, int C, int H, float inv_len_unused,
                                                              float* __restrict__ part, int chunks, const float* __restrict__ kv_mask) {
    __shared__ float Kt[LA_CHUNK][D + 1];
    __shared__ float Vt[LA_CHUNK][D];
    constexpr int VPT = D * D / 256 > 0 ? D * D / 256 : 1;   // outputs per thread: 4 (D = 32) or 1 (D = 16)
    const int c = blockIdx.y, nh = blockIdx.x, n = nh / H, h = nh - n * H;
    const int s0 = c * LA_CHUNK, ns = S - s0 < LA_CHUNK ? S - s0 : LA_CHUNK;
    const float* base = kv + (size_t(n) * S + s0) * 2 * C + h * D;
    const float len = float(S);
    for (int i = threadIdx.x; i < LA_CHUNK * D; i += 256) {
        const int s = i / D, d = i - s * D;
        float kk = 0.f, vv = 0.f;
        if (s < ns) {
            if constexpr (MASKED) {
                const float mk = kv_mask[size_t(n) * S + s0 + s];
                kk = elu1(base[size_t(s) * 2 * C + d]) * mk;
                vv = base[size_t(s) * 2 * C + C + d] * mk / len;
            } else {
                kk = elu1(base[size_t(s) * 2 * C + d]);
                vv = base[size_t(s) * 2 * C + C + d] / len;   // values / v_length (linear_attention.py:41)
            }
        }
        Kt[s][d] = kk;
        Vt[s][d] = vv;
    }
    __syncthreads();
    float* out = part + (size_t(nh) * chunks + c) * (D * D + D);
    if (threadIdx.x < D * D / VPT) {
        const int d = threadIdx.x / (D / VPT), v0 = (threadIdx.x % (D / VPT)) * VPT;
        float acc[VPT];
#pragma unroll
        for (int e = 0; e < VPT; ++e) acc[e] = 0.f;
        float ks = 0.f;
        for (int s = 0; s < ns; ++s) {
            const float kd = Kt[s][d];
            ks += kd;
#pragma unroll
            for (int e = 0; e < VPT; ++e) acc[e] += kd * Vt[s][v0 + e];
        }
#pragma unroll
        for (int e = 0; e < VPT; ++e) out[d * D + v0 + e] = acc[e];
        if (v0 == 0) out[D * D + d] = ks;
    }
}

// KV / Ksum = sum of the chunk partials, in chunk order.  kvf: [n * H, D * D + D]
__global__ __launch_bounds__(256) void linattn_finish_kernel(const float* __restrict__ part, int chunks, int per, float* __restrict__ kvf) {
    const int nh = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;   // one value per thread: (n H) x ceil(per / 256) blocks
    if (i >= per) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t(nh) * chunks + c) * per + i];
    kvf[size_t(nh) * per + i] = s;
}

// msg[l, h, v] = (sum_d Q[l,h,d] KV[h][d][v]) * (1 / (sum_d Q[l,h,d] Ksum[h][d] + eps)) * S,  Q = elu(q) + 1.
// Block: 256 threads = 256 / C rows at a time; a thread owns one output column and keeps its KV column and its head's
// Ksum in registers across the block's rows.
// PLANES (round 4): the message leaves as activation planes — the merge GEMM's operand — instead of fp32 + a split_planes pass
// (the same hi / lo arithmetic: bit-identical planes, one launch and two passes over the tensor less per layer)
// MASKED: Q = (elu(q) + 1) * q_mask[n, l] (linear_attention.py:36-37): a padded query row gets the message 0 and still goes
// through merge, LayerNorm and MLP like any other row.
template <int D, bool PLANES, bool MASKED>
__global__ __launch_bounds__(256) void linattn_apply_kernel(const float* __restrict__ q, const float* __restrict__ kvf, int L, int C, int H,
                                                             int S, float eps, float* __restrict__ msg, int rows_per_block,
                                                             unsigned* range_flag, const float* __restrict__ q_mask) {
    __shared__ float Qs[2][256];
    const int rpp = 256 / C;                          // rows per pass (C = 256: 1, C = 128: 2)
    const int sub = threadIdx.x / C, col = threadIdx.x - sub * C;
    const int h = col / D, v = col - h * D;
    const int n = blockIdx.x, l0 = blockIdx.y * rows_per_block;
    const float* kvh = kvf + (size_t(n) * H + h) * (D * D + D);
    float kvc[D], ksum[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        kvc[d] = kvh[d * D + v];
        ksum[d] = kvh[D * D + d];
    }
    const float len = float(S);
    float amax = 0.f;
    for (int r = 0; r < rows_per_block; r += rpp) {
        const int l = l0 + r + sub;
        const bool ok = l < L && r + sub < rows_per_block;
        __syncthreads();
        if constexpr (MASKED) Qs[0][threadIdx.x] = ok ? elu1(q[(size_t(n) * L + l) * C + col]) * q_mask[size_t(n) * L + l] : 0.f;
        else Qs[0][threadIdx.x] = ok ? elu1(q[(size_t(n) * L + l) * C + col]) : 0.f;
        __syncthreads();
        const float* qh = &Qs[0][sub * C + h * D];
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            num += qh[d] * kvc[d];
            den += qh[d] * ksum[d];
        }
        const float m = num * (1.0f / (den + eps)) * len;
        if constexpr (PLANES) {
            if (ok) {
                const float sv = m * K_PLANES_ACT_SCALE;
                amax = fmaxf(amax, fabsf(sv));
                if (!(sv == sv)) amax = INFINITY;
                pope_planes_store(reinterpret_cast<_Float16*>(msg) + (size_t(n) * L + l) * 2 * C, col, sv);
            }
        } else {
            if (ok) msg[(size_t(n) * L + l) * C + col] = m;
        }
    }
    if constexpr (PLANES) pope_range_flag(range_flag, POPE_RANGE_INPUT, !(amax < POPE_F16_OVERFLOW));
}

// planes row [x | LayerNorm(m) * w + b] of width 2C (the MLP's input cat[x, message], transformer.py:54), one wave per
// row, NV = C / 64 consecutive columns per lane
template <int NV, bool PLANES>   // PLANES = false: the fp32 twin writes [x | LN(m)] as floats [rows, 2C]
__global__ __launch_bounds__(256) void ln_cat_planes_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                             const float* __restrict__ w, const float* __restrict__ b,
                                                             _Float16* __restrict__ pl, int rows, float eps, float scale, unsigned* flag) {
    constexpr int C = NV * 64;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int c0 = lane * NV;
    float mv[NV], xv[NV];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        mv[e] = m[size_t(row) * C + c0 + e];
        xv[e] = x[size_t(row) * C + c0 + e];
        s += mv[e];
    }
    const float mean = wave_sum(s) * (1.0f / float(C));
    float qv = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const float d = mv[e] - mean;
        qv += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(qv) * (1.0f / float(C)) + eps);
    _Float16* pr = pl + size_t(row) * 4 * C;   // 2 * (2C) halves per row
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int c = c0 + e;
        const float vals[2] = {xv[e] * scale, ((mv[e] - mean) * rstd * w[c] + b[c]) * scale};
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const int cc = part * C + c;
            const float val = vals[part];
            if constexpr (PLANES) {
                amax = fmaxf(amax, fabsf(val));
                pope_planes_store(pr, cc, val);
            } else {
                reinterpret_cast<float*>(pl)[size_t(row) * 2 * C + cc] = val;   // scale = 1
            }
        }
    }
    if constexpr (PLANES) pope_range_flag(flag, POPE_RANGE_LAYERNORM, !(amax < POPE_F16_OVERFLOW) || !(fabsf(mean) + rstd < INFINITY));
}

// x <- x + LayerNorm(y) * w + b   (transformer.py:56-58), one wave per row
template <int NV>
__global__ __launch_bounds__(256) void ln_add_kernel(float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w,
                                                      const float* __restrict__ b, int rows, float eps) {
    constexpr int C = NV * 64;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int c0 = lane * NV;
    float yv[NV];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        yv[e] = y[size_t(row) * C + c0 + e];
        s += yv[e];
    }
    const float mean = wave_sum(s) * (1.0f / float(C));
    float qv = 0.f;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const float d = yv[e] - mean;
        qv += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(qv) * (1.0f / float(C)) + eps);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int c = c0 + e;
        x[size_t(row) * C + c] += (yv[e] - mean) * rstd * w[c] + b[c];
    }
}

}  // namespace

// The linear attention of one layer update (steps 3 and 4 of pope_launch_loftr_layer) and of the op-level entry: the chunk
// partials of KV / Ksum, their sum in chunk order, then the message row by row.  part: [n H, chunks, D D + D], kvf: [n H, D D + D].
// planes: the message leaves as activation planes (and range_flag is raised on a value outside the f16 range), else as fp32 rows.
static void linattn_launch(const float* q, const float* kv, const float* x_mask, const float* source_mask, int n, int L, int S, int C, int H,
                           bool planes, float* dst, float* part, float* kvf, unsigned* range_flag, hipStream_t stream) {
    const int D = C / H, chunks = (S + LA_CHUNK - 1) / LA_CHUNK, per = D * D + D;
    // (padding masks, LoFTREncoderLayer's x_mask / source_mask: separate instantiations, the unmasked ones are unchanged)
#define LA_REDUCE(DD, MK) hipLaunchKernelGGL((linattn_reduce_kernel<DD, MK>), dim3(n * H, chunks), dim3(256), 0, stream, kv, S, C, H, 0.f, \
                                             part, chunks, source_mask)
    if (source_mask) { if (D == 32) LA_REDUCE(32, true); else LA_REDUCE(16, true); }
    else { if (D == 32) LA_REDUCE(32, false); else LA_REDUCE(16, false); }
#undef LA_REDUCE
    hipLaunchKernelGGL(linattn_finish_kernel, dim3(n * H, (per + 255) / 256), dim3(256), 0, stream, part, chunks, per, kvf);
    const int rpb = LA_ROWS_PER_BLOCK;
#define LA_APPLY(DD, PL, MK, DST) hipLaunchKernelGGL((linattn_apply_kernel<DD, PL, MK>), dim3(n, (L + rpb - 1) / rpb), dim3(256), 0, stream, q, \
                                                     kvf, L, C, H, S, 1e-6f, DST, rpb, range_flag, x_mask)
#define LA_APPLY_D(PL, MK, DST) do { if (D == 32) LA_APPLY(32, PL, MK, DST); else LA_APPLY(16, PL, MK, DST); } while (0)
    if (!planes) {
        if (x_mask) LA_APPLY_D(false, true, dst); else LA_APPLY_D(false, false, dst);
    } else {
        if (x_mask) LA_APPLY_D(true, true, dst); else LA_APPLY_D(true, false, dst);
    }
#undef LA_APPLY_D
#undef LA_APPLY
}

void pope_loftr_linattn_seams(int* chunk_rows, int* rows_per_block) {
    if (chunk_rows) *chunk_rows = LA_CHUNK;
    if (rows_per_block) *rows_per_block = LA_ROWS_PER_BLOCK;
}

size_t pope_loftr_linear_attention_workspace(int n, int S, int C, int H) {
    if (n <= 0 || S <= 0 || (C != 256 && C != 128) || H != 8) return 0;
    const size_t D = C / H, chunks = (S + LA_CHUNK - 1) / LA_CHUNK;
    return pope_align256(size_t(n) * H * chunks * (D * D + D) * 4) + pope_align256(size_t(n) * H * (D * D + D) * 4);
}

int pope_loftr_linear_attention_check(const void* q, const void* kv, int n, int L, int S, int C, int H, const void* out_f32,
                                      const void* out_planes, const void* ws, size_t ws_bytes) {
    if (!q || !kv || !ws || n <= 0 || L <= 0 || S <= 0 || (C != 256 && C != 128) || H != 8) return POPE_ERR_ARG;
    if ((out_f32 != nullptr) == (out_planes != nullptr)) return POPE_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(ws) & 255) return POPE_ERR_ARG;
    const size_t rx = size_t(n) * L, rs = size_t(n) * S;
    if (rx > 0x7fffffffull / (2 * C) || rs > 0x7fffffffull / (2 * C)) return POPE_ERR_ARG;   // the layer's index range
    if (ws_bytes < pope_loftr_linear_attention_workspace(n, S, C, H)) return POPE_ERR_WORKSPACE;
    return POPE_OK;
}

int pope_launch_loftr_linear_attention(const float* q, const float* kv, const float* x_mask, const float* source_mask, int n, int L, int S,
                                       int C, int H, float* out_f32, void* out_planes, void* ws, size_t ws_bytes, unsigned* range_flag,
                                       hipStream_t stream) {
    POPE_TRY(pope_loftr_linear_attention_check(q, kv, n, L, S, C, H, out_f32, out_planes, ws, ws_bytes));
    const int D = C / H, chunks = (S + LA_CHUNK - 1) / LA_CHUNK, per = D * D + D;
    pope_carver carve{static_cast<char*>(ws)};
    float* part = carve.take<float>(size_t(n) * H * chunks * per * 4);
    float* kvf = carve.take<float>(size_t(n) * H * per * 4);
    linattn_launch(q, kv, x_mask, source_mask, n, L, S, C, H, out_planes != nullptr, out_planes ? static_cast<float*>(out_planes) : out_f32, part,
                   kvf, range_flag, stream);
    return pope_check_launch();
}

size_t pope_loftr_layer_workspace(int n, int L, int S, int C, int H) {
    const size_t rx = size_t(n) * L, rs = size_t(n) * S, D = C / H, chunks = (S + LA_CHUNK - 1) / LA_CHUNK;
    return pope_align256(rx * C * 4) /*xp*/ + pope_align256(rs * C * 4) /*sp*/ + pope_align256(rx * C * 4) /*q, later merge out*/ + pope_align256(rs * 2 * C * 4) /*kv*/ +
           pope_align256(size_t(n) * H * chunks * (D * D + D) * 4) + pope_align256(size_t(n) * H * (D * D + D) * 4) + pope_align256(rx * C * 4) /*msg, later mlp out*/ +
           pope_align256(rx * C * 4) /*msg planes*/ + pope_align256(rx * 2 * C * 4) /*cat planes*/ + pope_align256(rx * 2 * C * 4) /*hidden planes*/;
}

int pope_launch_loftr_layer(const LoftrLayerParams& p, hipStream_t stream) {
    const int C = p.C, H = p.H, D = C / H;
    if (!p.x || !p.source || !p.ws || p.n <= 0 || p.L <= 0 || p.S <= 0 || (C != 256 && C != 128) || H != 8) return POPE_ERR_ARG;
    const bool f32 = p.precision == POPE_PREC_F32_MFMA;
    if (!f32 && p.precision != POPE_PREC_F16X3) return POPE_ERR_ARG;
    if (!p.norm1_w || !p.norm1_b || !p.norm2_w || !p.norm2_b) return POPE_ERR_ARG;
    if (f32 ? (!p.q_w || !p.kv_w || !p.merge_w || !p.mlp0_w || !p.mlp1_w) : (!p.q_wp || !p.kv_wp || !p.merge_wp || !p.mlp0_wp || !p.mlp1_wp))
        return POPE_ERR_ARG;
    const bool full = p.attention == POPE_LOFTR_ATTN_FULL;
    if (!full && p.attention != POPE_LOFTR_ATTN_LINEAR) return POPE_ERR_ARG;
    if (full && (p.x_mask || p.source_mask)) return POPE_ERR_ARG;   // a padded query row is NaN in the reference's FullAttention
    if (p.ws_bytes < pope_loftr_layer_workspace(p.n, p.L, p.S, C, H)) return POPE_ERR_WORKSPACE;
    const size_t rx = size_t(p.n) * p.L, rs = size_t(p.n) * p.S;
    if (rx > 0x7fffffffull / (2 * C) || rs > 0x7fffffffull / (2 * C)) return POPE_ERR_ARG;
    const int chunks = (p.S + LA_CHUNK - 1) / LA_CHUNK, per = D * D + D;
    pope_carver ws{static_cast<char*>(p.ws)};
    void* xp = ws.take(rx * C * 4);
    void* sp = ws.take(rs * C * 4);
    float* q = ws.take<float>(rx * C * 4);
    float* kv = ws.take<float>(rs * 2 * C * 4);
    float* part = ws.take<float>(size_t(p.n) * H * chunks * per * 4);
    float* kvf = ws.take<float>(size_t(p.n) * H * per * 4);
    float* msg = ws.take<float>(rx * C * 4);
    void* msgp = ws.take(rx * C * 4);
    void* catp = ws.take(rx * 2 * C * 4);
    void* hidp = ws.take(rx * 2 * C * 4);
    const bool self = p.source == p.x && p.S == p.L;
    // POPE_PREC_F32_MFMA (the range guard's re-run): the same sequence with fp32 operands on gemm_f32.hip — "planes" buffers
    // hold plain fp32 rows (same bytes), no operand split, no range contract
    auto gemm = [&](const void* a_pl, const void* w_pl, float* Cf, void* Cp, int M, int N, int K, int epi) {
        if (f32) {   // gemm_f32.hip has BIAS_RELU as EPI_CONV's activation: slope 0 = ReLU, 1 = identity
            GemmParams g = pope_linear_params(LINEAR_F32, a_pl, w_pl, nullptr, Cf ? Cf : static_cast<float*>(Cp), nullptr, M, N, K, EPI_CONV);
            g.act_slope = epi == EPI_BIAS_RELU ? 0.f : 1.f;
            g.ldres = 0;
            return pope_launch_gemm_nt_f32(g, stream);
        }
        GemmParams g = pope_linear_params(LINEAR_PLANES, a_pl, w_pl, nullptr, Cf, Cp, M, N, K, epi, nullptr, nullptr, 0, p.range_flag);
        g.ldres = 0;
        g.range_bit = POPE_RANGE_GELU;   // the hidden planes of the MLP are this layer's only packed output
        return pope_launch_gemm_planes(g, stream);
    };
    // 1. operands of the projections
    if (f32) {
        xp = p.x;
        sp = const_cast<float*>(p.source);
    } else {
        POPE_TRY(pope_launch_split_planes(p.x, xp, int(rx), C, K_PLANES_ACT_SCALE, p.range_flag, stream));
        if (!self) POPE_TRY(pope_launch_split_planes(p.source, sp, int(rs), C, K_PLANES_ACT_SCALE, p.range_flag, stream));
    }
    const void* Wq = f32 ? static_cast<const void*>(p.q_w) : p.q_wp;
    const void* Wkv = f32 ? static_cast<const void*>(p.kv_w) : p.kv_wp;
    const void* Wm = f32 ? static_cast<const void*>(p.merge_w) : p.merge_wp;
    const void* W0 = f32 ? static_cast<const void*>(p.mlp0_w) : p.mlp0_wp;
    const void* W1 = f32 ? static_cast<const void*>(p.mlp1_w) : p.mlp1_wp;
    // 2. q = x Wq^T ; [k | v] = source [Wk ; Wv]^T
    POPE_TRY(gemm(xp, Wq, q, nullptr, int(rx), C, C, EPI_BIAS));
    POPE_TRY(gemm(self ? xp : sp, Wkv, kv, nullptr, int(rs), 2 * C, C, EPI_BIAS));
    // 3.-4. full attention: softmax(q k^T / sqrt(D)) v in one launch (loftr_attention.hip), the message where step 4 writes it
    if (full) {
        if (f32) msgp = msg;
        POPE_TRY(pope_launch_loftr_full_attention(q, kv, p.n, p.L, p.S, C, H, !f32, static_cast<float*>(msgp), p.range_flag, stream));
    } else {
        // 3. per-head state, 4. message (f16x3: the message is written as planes straight away; fp32 mode: plain rows)
        if (f32) msgp = msg;
        linattn_launch(q, kv, p.x_mask, p.source_mask, p.n, p.L, p.S, C, H, !f32, static_cast<float*>(msgp), part, kvf, p.range_flag, stream);
    }
    // 5. merge (-> q buffer), 6. cat[x, LN1(merge)] as planes
    POPE_TRY(gemm(msgp, Wm, q, nullptr, int(rx), C, C, EPI_BIAS));
    const dim3 rows4(unsigned((rx + 3) / 4));
    const float cat_scale = f32 ? 1.0f : K_PLANES_ACT_SCALE;
#define LN_CAT(NV, PL) hipLaunchKernelGGL((ln_cat_planes_kernel<NV, PL>), rows4, dim3(256), 0, stream, p.x, q, p.norm1_w, p.norm1_b, \
                                          static_cast<_Float16*>(catp), int(rx), p.ln_eps, cat_scale, p.range_flag)
    if (C == 256) { if (f32) LN_CAT(4, false); else LN_CAT(4, true); }
    else { if (f32) LN_CAT(2, false); else LN_CAT(2, true); }
#undef LN_CAT
    // 7. MLP: relu(cat W0^T) -> planes ; W1 -> fp32 (msg buffer) ; 8. x += LN2(.)
    POPE_TRY(gemm(catp, W0, nullptr, hidp, int(rx), 2 * C, 2 * C, EPI_BIAS_RELU));
    POPE_TRY(gemm(hidp, W1, msg, nullptr, int(rx), C, 2 * C, EPI_BIAS));
    if (C == 256) hipLaunchKernelGGL(ln_add_kernel<4>, rows4, dim3(256), 0, stream, p.x, msg, p.norm2_w, p.norm2_b, int(rx), p.ln_eps);
    else hipLaunchKernelGGL(ln_add_kernel<2>, rows4, dim3(256), 0, stream, p.x, msg, p.norm2_w, p.norm2_b, int(rx), p.ln_eps);
    return pope_check_launch();
}
