// ConvNeXtV2 backbone (pose/convnextv2/convnextv2.py: Block + GRN) and the image pose head (pose/model_cnn.py) for gfx950, wave64.
//
// Layout: channels-last [B, h, w, C] fp32 between launches, so every 1 x 1 / 2 x 2 / 4 x 4 convolution and every Linear is a
// row-major GEMM [pixels, K] . [N, K]^T on the existing kernels, and a channels-first LayerNorm is a LayerNorm of a pixel row.
// The kernels of this file are the memory-bound rest (bytes against the algorithmic minimum: DESIGN.md "ConvNeXtV2"):
//   stem_gather      NCHW image -> [M, 48] rows (columns (channel, kh, kw): the conv weight's own order)
//   ln_rows          LayerNorm of a pixel row -> fp32 rows or f16x3 planes, optionally scattered as the 2 x 2 patch row of the
//                    downsample convolution (one producer for the stem, the blocks, the downsample layers)
//   dwconv7          depthwise 7 x 7 + bias: a lane is a channel, an 8 x 8 pixel tile with its halo (14 x 14) in LDS
//   grn_partial / grn_colnorm / grn_finish / grn_apply   Global Response Normalization, fixed summation order, no atomics
//   tail             mean over h w in row order, then nn.LayerNorm(C3)
//   pose_heads       the two 32 -> 3 / 9 | 4 | 6 Linears and convert2matrix (rot_convert.h)
// The block LayerNorm is NOT fused into dwconv7: a fused form needs all C channels of a pixel in one workgroup, and the
// halo of an 8 x 8 tile at C = 1536 is 1.2 MB; the separate producer costs one extra read and write of [M, C], 2 of the
// ~26 M C floats a block moves.
#include "common.h"
#include "kernels.h"
#include "linear.h"
#include "rot_convert.h"

namespace {

constexpr float LN_EPS = 1e-6f, GRN_EPS = 1e-6f;
constexpr int GRN_ROWS = 64;     // rows per chunk of the GRN column reduction: depends on nothing but this constant
constexpr int DW_T = 8, DW_HALO = DW_T + 6;

__device__ __forceinline__ float block_sum(float v, float* red) {   // 256 threads; the same order for every caller
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

// image [B, 3, H, W] -> rows [B (H / 4) (W / 4), 48]; one thread per 16-byte quad of the image, in image order
__global__ __launch_bounds__(256) void stem_gather_kernel(const float* __restrict__ img, float* __restrict__ out, int H, int W, long long quads) {
    const int wq = W >> 2;
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < quads; q += 256ll * gridDim.x) {
        const int ow = int(q % wq);
        const long long t = q / wq;
        const int h = int(t % H);
        const int c = int((t / H) % 3);
        const long long n = t / (3ll * H);
        const f32x4 v = *reinterpret_cast<const f32x4*>(img + 4 * q);
        const long long row = (n * (H >> 2) + (h >> 2)) * wq + ow;
        *reinterpret_cast<f32x4*>(out + row * 48 + c * 16 + (h & 3) * 4) = v;
    }
}

// LayerNorm over the C channels of a pixel row (a wave per row, two-pass variance), eps inside the sqrt.
// PATCH: pixel (n, h, w) of the [H, W] map goes to row (n, h / 2, w / 2), columns ((h & 1) 2 + (w & 1)) C .. of a [M / 4, 4 C]
// matrix: the operand of the 2 x 2 stride-2 convolution.  PLANES: activation planes (scale 8) instead of fp32.  y may be x
// when neither is set (every lane re-reads only what it wrote).
template <bool PLANES, bool PATCH>
__global__ __launch_bounds__(256) void ln_rows_kernel(const float* x, const float* __restrict__ w, const float* __restrict__ b, void* y,
                                                      long long M, int C, int H, int W, unsigned* flag) {
    const int lane = threadIdx.x & 63;
    const long long r = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (r >= M) return;
    const float* xr = x + r * C;
    float s = 0.f;
    for (int c = 4 * lane; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wave_sum(s) / float(C);
    float q = 0.f;
    for (int c = 4 * lane; c < C; c += 256) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(xr + c) - mean;
        q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / float(C) + LN_EPS);
    long long orow = r;
    int col0 = 0, ld = C;
    if constexpr (PATCH) {
        const int px = int(r % W), py = int((r / W) % H);
        const long long n = r / (1ll * W * H);
        orow = (n * (H >> 1) + (py >> 1)) * (W >> 1) + (px >> 1);
        col0 = ((py & 1) * 2 + (px & 1)) * C;
        ld = 4 * C;
    }
    pope_range_acc acc;
    for (int c = 4 * lane; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
        const f32x4 o = ((v - mean) * rstd) * *reinterpret_cast<const f32x4*>(w + c) + *reinterpret_cast<const f32x4*>(b + c);
        if constexpr (PLANES) {
            const f32x4 sc = o * K_PLANES_ACT_SCALE;
            acc.add(sc);
            pope_planes_store(static_cast<_Float16*>(y) + orow * 2 * ld, col0 + c, sc);
        } else {
            *reinterpret_cast<f32x4*>(static_cast<float*>(y) + orow * ld + col0 + c) = o;
        }
    }
    if constexpr (PLANES) pope_range_flag(flag, POPE_RANGE_LAYERNORM, acc.bad());
}

// Depthwise 7 x 7, padding 3, + bias.  Workgroup = an 8 x 8 pixel tile x 64 channels of one image; lane = channel, so every
// global and LDS row access of a wave is 256 contiguous bytes.  Wave v computes tile rows 2 v and 2 v + 1, eight pixels at a
// time from a sliding window of 14 LDS values per kernel row.  Taps are summed in (ky, kx) order, then the bias.
__global__ __launch_bounds__(256) void dwconv7_kernel(const float* __restrict__ x, const float* __restrict__ w49, const float* __restrict__ bias,
                                                      float* __restrict__ y, int H, int W, int C, int tiles_x) {
    __shared__ float tile[DW_HALO * DW_HALO * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < C;
    const int ty0 = (blockIdx.x / tiles_x) * DW_T, tx0 = (blockIdx.x % tiles_x) * DW_T;
    const size_t img = size_t(blockIdx.z) * H * W;
    // the channel's 49 weights first: their loads are in flight while the halo is staged
    float wk[49];
#pragma unroll
    for (int k = 0; k < 49; ++k) wk[k] = live ? w49[size_t(k) * C + c] : 0.f;
    // 196 halo positions = 4 waves x 7 rounds x 7 positions: the seven loads of a round are issued before their LDS writes
    static_assert(DW_HALO * DW_HALO == 4 * 7 * 7, "staging rounds");
    for (int p0 = wave; p0 < DW_HALO * DW_HALO; p0 += 28) {
        float v[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int p = p0 + 4 * j, hy = ty0 + p / DW_HALO - 3, hx = tx0 + p % DW_HALO - 3;
            v[j] = 0.f;
            if (live && hy >= 0 && hy < H && hx >= 0 && hx < W) v[j] = x[(img + size_t(hy) * W + hx) * C + c];
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) tile[(p0 + 4 * j) * 64 + lane] = v[j];
    }
    __syncthreads();
    if (!live) return;
    const float bc = bias[c];
    for (int r = 0; r < 2; ++r) {
        const int oy = wave * 2 + r;
        if (ty0 + oy >= H) break;
        float acc[DW_T];
#pragma unroll
        for (int i = 0; i < DW_T; ++i) acc[i] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const float* row = tile + (oy + ky) * DW_HALO * 64 + lane;
            float in[DW_HALO];
#pragma unroll
            for (int i = 0; i < DW_HALO; ++i) in[i] = row[i * 64];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx)
#pragma unroll
                for (int ox = 0; ox < DW_T; ++ox) acc[ox] = fmaf(in[ox + kx], wk[ky * 7 + kx], acc[ox]);
        }
#pragma unroll
        for (int ox = 0; ox < DW_T; ++ox)
            if (tx0 + ox < W) y[(img + size_t(ty0 + oy) * W + tx0 + ox) * C + c] = acc[ox] + bc;
    }
}

// GRN statistics, pass 1: sums of squares of 256 columns over one chunk of GRN_ROWS rows of one image.  Wave v takes rows
// v, v + 4, .. of the chunk in order; the four waves are added as (0 + 1) + (2 + 3).  part [B, chunks, C].
__global__ __launch_bounds__(256) void grn_partial_kernel(const float* __restrict__ x, float* __restrict__ part, int HW, int C, int chunks) {
    __shared__ f32x4 red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 256 + 4 * lane, chunk = blockIdx.y, n = blockIdx.z;
    const int r0 = chunk * GRN_ROWS, r1 = min(r0 + GRN_ROWS, HW);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (c < C)
        for (int r = r0 + wave; r < r1; r += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t(n) * HW + r) * C + c);
            s += v * v;
        }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < C)
        *reinterpret_cast<f32x4*>(part + (size_t(n) * chunks + chunk) * C + c) = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// pass 2, a thread per column: Gx[n, c] = sqrt(the chunks' sums added in chunk order) -> nx [B, C]
__global__ __launch_bounds__(256) void grn_colnorm_kernel(const float* __restrict__ part, float* __restrict__ nx, int C, int chunks) {
    const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (c >= C) return;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < chunks; ++k) s += part[(size_t(n) * chunks + k) * C + c];
    nx[size_t(n) * C + c] = sqrtf(s);
}

// pass 3, one workgroup per image: Nx[c] = Gx[c] / (mean_c Gx + 1e-6) in place; the mean in a fixed order (a thread's columns
// c, c + 256, .. in order, then the butterfly and the four waves)
__global__ __launch_bounds__(256) void grn_finish_kernel(float* __restrict__ nx, int C) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    float local = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) local += nx[size_t(n) * C + c];
    const float denom = block_sum(local, red) / float(C) + GRN_EPS;
    for (int c = threadIdx.x; c < C; c += 256) nx[size_t(n) * C + c] = nx[size_t(n) * C + c] / denom;   // the thread's own columns
}

// y = gamma (x Nx) + beta + x, in the reference's order of operations; one read and one write of [M, C]
template <bool PLANES>
__global__ __launch_bounds__(256) void grn_apply_kernel(const float* x, const float* __restrict__ nx, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, void* y, long long quads, int HW, int C, unsigned* flag) {
    const int cq = C >> 2;
    pope_range_acc acc;
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < quads; q += 256ll * gridDim.x) {
        const long long row = q / cq;
        const int c = int(q % cq) * 4;
        const long long n = row / HW;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * q);
        const f32x4 o = (*reinterpret_cast<const f32x4*>(gamma + c) * (v * *reinterpret_cast<const f32x4*>(nx + n * C + c)) +
                         *reinterpret_cast<const f32x4*>(beta + c)) + v;
        if constexpr (PLANES) {
            const f32x4 sc = o * K_PLANES_ACT_SCALE;
            acc.add(sc);
            pope_planes_store(static_cast<_Float16*>(y) + row * 2 * C, c, sc);
        } else {
            *reinterpret_cast<f32x4*>(static_cast<float*>(y) + 4 * q) = o;
        }
    }
    if constexpr (PLANES) pope_range_flag(flag, POPE_RANGE_GELU, acc.bad());
}

// x [B, HW, C] -> feat [B, C] = LayerNorm(mean over the HW rows in row order); one workgroup per image, C floats of LDS
__global__ __launch_bounds__(256) void tail_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                   float* __restrict__ feat, int HW, int C) {
    extern __shared__ float pooled[];
    __shared__ float red[4];
    const int n = blockIdx.x;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f;
#pragma unroll 8
        for (int r = 0; r < HW; ++r) a += x[(size_t(n) * HW + r) * C + c];
        a /= float(HW);
        pooled[c] = a;
        s += a;
    }
    const float mean = block_sum(s, red) / float(C);
    float q = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) q += (pooled[c] - mean) * (pooled[c] - mean);
    const float rstd = 1.0f / sqrtf(block_sum(q, red) / float(C) + LN_EPS);
    for (int c = threadIdx.x; c < C; c += 256) feat[size_t(n) * C + c] = ((pooled[c] - mean) * rstd) * w[c] + b[c];
}

// one wave per pair: lane j < 3 the translation, lanes 3 .. 3 + rdim the rotation head, lane 0 converts
__global__ __launch_bounds__(64) void pose_heads_kernel(const float* __restrict__ feat, const float* __restrict__ tw, const float* __restrict__ tb,
                                                        const float* __restrict__ rw, const float* __restrict__ rb, int mode, int inner,
                                                        float* __restrict__ trans, float* __restrict__ rot) {
    __shared__ float head[12];
    const int b = blockIdx.x, j = threadIdx.x;
    const int rdim = mode == POPE_ROT_MATRIX ? 9 : mode == POPE_ROT_QUAT ? 4 : 6;
    if (j < 3 + rdim) {
        const float* wrow = j < 3 ? tw + size_t(j) * inner : rw + size_t(j - 3) * inner;
        float s = 0.f;
        for (int k = 0; k < inner; ++k) s = fmaf(wrow[k], feat[size_t(b) * inner + k], s);
        head[j] = s + (j < 3 ? tb[j] : rb[j - 3]);
    }
    __syncthreads();
    if (j != 0) return;
    for (int i = 0; i < 3; ++i) trans[3 * b + i] = head[i];
    pope_rot_to_matrix(mode, head + 3, rot + 9 * b);
}

// ---- host -----------------------------------------------------------------------------------------------------------------

bool planes_k(int precision, int K) { return precision == POPE_PREC_F16X3 && K >= 64 && (K & 31) == 0; }

int launch_ln(bool planes, bool patch, const float* x, const float* w, const float* b, void* y, long long M, int C, int H, int W, unsigned* flag,
              hipStream_t st) {
    const dim3 grid((unsigned)((M + 3) / 4)), block(256);
    if (planes && patch) hipLaunchKernelGGL((ln_rows_kernel<true, true>), grid, block, 0, st, x, w, b, y, M, C, H, W, flag);
    else if (planes) hipLaunchKernelGGL((ln_rows_kernel<true, false>), grid, block, 0, st, x, w, b, y, M, C, H, W, flag);
    else if (patch) hipLaunchKernelGGL((ln_rows_kernel<false, true>), grid, block, 0, st, x, w, b, y, M, C, H, W, flag);
    else hipLaunchKernelGGL((ln_rows_kernel<false, false>), grid, block, 0, st, x, w, b, y, M, C, H, W, flag);
    return pope_check_launch();
}

// a [M, K] (fp32 rows, or planes when `planes`) . w^T + bias with the epilogue -> fp32 C
int linear(bool planes, const void* a, const float* wf, const void* wp, const float* bias, float* C, long long M, int N, int K, int epi,
           const float* gamma, const float* res, unsigned* flag, hipStream_t st) {
    if (planes)
        return pope_launch_gemm_planes(pope_linear_params(LINEAR_PLANES, a, wp, bias, C, nullptr, int(M), N, K, epi, gamma, res, 0, flag), st);
    return pope_launch_gemm_nt_f32(pope_linear_params(LINEAR_F32, a, wf, bias, C, nullptr, int(M), N, K, epi, gamma, res), st);
}

struct Layout { size_t x, x2, t, a, h, hp, grn, feat, total; };

bool geometry_ok(const pope_convnext_weights* w, int B, int H, int W) {
    if (!w || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (H & 31) || (W & 31)) return false;
    for (int i = 0; i < 4; ++i)
        if (w->depths[i] < 0 || w->dims[i] < 8 || (w->dims[i] & 7) || w->dims[i] > 8192) return false;   // tail: C3 floats of LDS
    // the GEMMs address their rows through 32-bit byte offsets (gemm_planes.hip args_ok: (M + 256) ld 4 < 2^32 - 512)
    size_t m = size_t(B) * (H / 4) * (W / 4);
    for (int i = 0; i < 4; ++i, m /= 4)
        if ((m + 256) * size_t(4 * w->dims[i]) * 4 >= (size_t(1) << 32) - 512) return false;
    return size_t(B) * H * W * 3 < (size_t(1) << 40);
}

Layout layout(const pope_convnext_weights* w, int B, int H, int W, bool x3) {
    size_t m = size_t(B) * (H / 4) * (W / 4), act = 0, hid = 0, grn = 0;
    int hw = (H / 4) * (W / 4), cmax = 0;
    for (int i = 0; i < 4; ++i, m /= 4, hw /= 4) {
        const size_t c = size_t(w->dims[i]);
        act = act > m * c ? act : m * c;
        hid = hid > 4 * m * c ? hid : 4 * m * c;
        const size_t g = pope_convnext_grn_workspace(B, hw, 4 * int(c));
        grn = grn > g ? grn : g;
        cmax = cmax > int(c) ? cmax : int(c);
    }
    const size_t m0 = size_t(B) * (H / 4) * (W / 4);
    Layout l;
    l.x = l.x2 = l.t = pope_align256(act * 4);
    l.a = pope_align256((act > m0 * 48 ? act : m0 * 48) * 4);
    l.h = pope_align256(hid * 4);
    l.hp = x3 ? l.h : 0;
    l.grn = grn;
    l.feat = pope_align256(size_t(B) * w->dims[3] * 4);
    l.total = l.x + l.x2 + l.t + l.a + l.h + l.hp + l.grn + l.feat;
    return l;
}

}  // namespace

int pope_launch_convnext_dwconv(const float* x, const float* w49, const float* bias, float* y, int B, int H, int W, int C, hipStream_t stream) {
    if (!x || !w49 || !bias || !y || x == y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || B > 65535 || (C + 63) / 64 > 65535) return POPE_ERR_ARG;
    const int tx = (W + DW_T - 1) / DW_T, ty = (H + DW_T - 1) / DW_T;
    if (size_t(tx) * ty > 0x7fffffffu) return POPE_ERR_ARG;
    hipLaunchKernelGGL(dwconv7_kernel, dim3(tx * ty, (C + 63) / 64, B), dim3(256), 0, stream, x, w49, bias, y, H, W, C, tx);
    return pope_check_launch();
}

size_t pope_convnext_grn_workspace(int B, int HW, int C) {
    if (B <= 0 || HW <= 0 || C <= 0) return 0;
    const size_t chunks = (size_t(HW) + GRN_ROWS - 1) / GRN_ROWS;
    return pope_align256(size_t(B) * chunks * C * 4) + pope_align256(size_t(B) * C * 4);
}

int pope_convnext_grn_check(const float* x, const float* gamma, const float* beta, int B, int HW, int C, const float* y_f32,
                            const void* y_planes, const void* ws, size_t ws_bytes) {
    if (!x || !gamma || !beta || B <= 0 || HW <= 0 || C <= 0 || (C & 31) || B > 65535 || (!y_f32) == (!y_planes)) return POPE_ERR_ARG;
    if ((HW + GRN_ROWS - 1) / GRN_ROWS > 65535) return POPE_ERR_ARG;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return POPE_ERR_ARG;
    return ws_bytes < pope_convnext_grn_workspace(B, HW, C) ? POPE_ERR_ARG : POPE_OK;
}

int pope_launch_convnext_grn(const float* x, const float* gamma, const float* beta, int B, int HW, int C, float* y_f32, void* y_planes,
                             void* ws, unsigned* range_flag, hipStream_t stream) {
    const int chunks = (HW + GRN_ROWS - 1) / GRN_ROWS;
    pope_carver cv{static_cast<char*>(ws)};
    float* part = cv.take<float>(size_t(B) * chunks * C * 4);
    float* nx = cv.take<float>(size_t(B) * C * 4);
    hipLaunchKernelGGL(grn_partial_kernel, dim3((C + 255) / 256, chunks, B), dim3(256), 0, stream, x, part, HW, C, chunks);
    POPE_TRY(pope_check_launch());
    hipLaunchKernelGGL(grn_colnorm_kernel, dim3((C + 255) / 256, B), dim3(256), 0, stream, part, nx, C, chunks);
    POPE_TRY(pope_check_launch());
    hipLaunchKernelGGL(grn_finish_kernel, dim3(B), dim3(256), 0, stream, nx, C);
    POPE_TRY(pope_check_launch());
    const long long quads = 1ll * B * HW * (C / 4);
    if (y_planes)
        hipLaunchKernelGGL((grn_apply_kernel<true>), dim3(pope_grid_for(quads)), dim3(256), 0, stream, x, nx, gamma, beta, y_planes, quads, HW, C,
                           range_flag);
    else
        hipLaunchKernelGGL((grn_apply_kernel<false>), dim3(pope_grid_for(quads)), dim3(256), 0, stream, x, nx, gamma, beta, static_cast<void*>(y_f32),
                           quads, HW, C, range_flag);
    return pope_check_launch();
}

int pope_launch_convnext_pose_heads(const float* feat, const float* trans_w, const float* trans_b, const float* rot_w, const float* rot_b,
                                    int mode, int B, int inner, float* trans, float* rot, hipStream_t stream) {
    if (!feat || !trans_w || !trans_b || !rot_w || !rot_b || !trans || !rot || B <= 0 || inner <= 0 || inner > 256) return POPE_ERR_ARG;
    if (mode < POPE_ROT_MATRIX || mode > POPE_ROT_6D) return POPE_ERR_ARG;
    hipLaunchKernelGGL(pose_heads_kernel, dim3(B), dim3(64), 0, stream, feat, trans_w, trans_b, rot_w, rot_b, mode, inner, trans, rot);
    return pope_check_launch();
}

size_t pope_convnext_workspace(const pope_convnext_weights* w, int B, int H, int W) {
    return geometry_ok(w, B, H, W) ? layout(w, B, H, W, true).total : 0;
}

int pope_convnext_check(const ConvNextArgs& a) {
    if (a.precision != POPE_PREC_F32_MFMA && a.precision != POPE_PREC_F16X3) return POPE_ERR_ARG;
    if (!geometry_ok(a.w, a.B, a.H, a.W) || !a.image || (reinterpret_cast<uintptr_t>(a.image) & 15)) return POPE_ERR_ARG;
    const pope_convnext_weights& w = *a.w;
    bool all = w.blocks_host && w.stem_w && w.stem_b && w.stem_ln_w && w.stem_ln_b && w.norm_w && w.norm_b && w.ones;
    for (int i = 0; i < 3 && all; ++i)
        all = w.ds_ln_w[i] && w.ds_ln_b[i] && w.ds_w[i] && w.ds_b[i] && (a.precision != POPE_PREC_F16X3 || w.ds_wp[i]);
    if (!all) return POPE_ERR_ARG;
    int nb = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < w.depths[i]; ++j, ++nb) {
            const pope_convnext_block_weights& k = w.blocks_host[nb];
            if (!k.dw_w || !k.dw_b || !k.norm_w || !k.norm_b || !k.pw1_w || !k.pw1_b || !k.grn_gamma || !k.grn_beta || !k.pw2_w || !k.pw2_b)
                return POPE_ERR_ARG;
            if (a.precision == POPE_PREC_F16X3 && (!k.pw2_wp || (planes_k(a.precision, w.dims[i]) && !k.pw1_wp))) return POPE_ERR_ARG;
        }
    if (a.logits && (!w.head_w || !w.head_b || w.num_classes <= 0 || (w.num_classes & 3))) return POPE_ERR_ARG;
    if (!a.ws || (reinterpret_cast<uintptr_t>(a.ws) & 255)) return POPE_ERR_ARG;
    return a.ws_bytes < pope_convnext_workspace(a.w, a.B, a.H, a.W) ? POPE_ERR_ARG : POPE_OK;
}

int pope_launch_convnext(const ConvNextArgs& a, hipStream_t st) {
    POPE_TRY(pope_convnext_check(a));
    const pope_convnext_weights& w = *a.w;
    const int prec = a.precision, B = a.B;
    const Layout lay = layout(a.w, B, a.H, a.W, true);
    pope_carver cv{static_cast<char*>(a.ws)};
    float* x = cv.take<float>(lay.x);
    float* x2 = cv.take<float>(lay.x2);
    float* t = cv.take<float>(lay.t);
    void* op = cv.take<void>(lay.a);
    float* h = cv.take<float>(lay.h);
    void* hp = cv.take<void>(lay.hp);
    void* grn = cv.take<void>(lay.grn);
    float* feat_ws = cv.take<float>(lay.feat);
    unsigned* flag = prec == POPE_PREC_F16X3 ? a.range_flag : nullptr;

    int hh = a.H / 4, ww = a.W / 4;
    long long M = 1ll * B * hh * ww;
    auto tap = [&](int i, const float* src, int C) {
        if (!a.taps || !a.taps[i]) return POPE_OK;
        return hipMemcpyAsync(a.taps[i], src, size_t(M) * C * 4, hipMemcpyDeviceToDevice, st) == hipSuccess ? POPE_OK : POPE_ERR_LAUNCH;
    };
    // stem: K = 48 is no multiple of 32, so the fp32 MFMA in both precisions
    {
        const long long quads = 1ll * B * 3 * a.H * (a.W / 4);
        hipLaunchKernelGGL(stem_gather_kernel, dim3(pope_grid_for(quads)), dim3(256), 0, st, a.image, static_cast<float*>(op), a.H, a.W, quads);
        POPE_TRY(pope_check_launch());
        POPE_TRY(linear(false, op, w.stem_w, nullptr, w.stem_b, x, M, w.dims[0], 48, EPI_BIAS, nullptr, nullptr, nullptr, st));
        POPE_TRY(launch_ln(false, false, x, w.stem_ln_w, w.stem_ln_b, x, M, w.dims[0], hh, ww, nullptr, st));
        POPE_TRY(tap(0, x, w.dims[0]));
    }
    int nb = 0;
    for (int i = 0; i < 4; ++i) {
        const int C = w.dims[i];
        if (i > 0) {   // LayerNorm(C_{i-1}) per pixel -> 2 x 2 patch rows -> GEMM
            const int Cp = w.dims[i - 1];
            const bool pl = planes_k(prec, 4 * Cp);
            POPE_TRY(launch_ln(pl, true, x, w.ds_ln_w[i - 1], w.ds_ln_b[i - 1], op, M, Cp, hh, ww, flag, st));
            hh /= 2; ww /= 2; M /= 4;
            POPE_TRY(linear(pl, op, w.ds_w[i - 1], w.ds_wp[i - 1], w.ds_b[i - 1], x2, M, C, 4 * Cp, EPI_BIAS, nullptr, nullptr, flag, st));
            float* s = x; x = x2; x2 = s;
        }
        for (int j = 0; j < w.depths[i]; ++j, ++nb) {
            const pope_convnext_block_weights& k = w.blocks_host[nb];
            const bool pl1 = planes_k(prec, C), pl2 = planes_k(prec, 4 * C);
            POPE_TRY(pope_launch_convnext_dwconv(x, k.dw_w, k.dw_b, t, B, hh, ww, C, st));
            POPE_TRY(launch_ln(pl1, false, t, k.norm_w, k.norm_b, op, M, C, hh, ww, flag, st));
            POPE_TRY(linear(pl1, op, k.pw1_w, k.pw1_wp, k.pw1_b, h, M, 4 * C, C, EPI_BIAS_GELU, nullptr, nullptr, flag, st));
            POPE_TRY(pope_launch_convnext_grn(h, k.grn_gamma, k.grn_beta, B, hh * ww, 4 * C, pl2 ? nullptr : h, pl2 ? hp : nullptr, grn, flag, st));
            POPE_TRY(linear(pl2, pl2 ? hp : static_cast<void*>(h), k.pw2_w, k.pw2_wp, k.pw2_b, x, M, C, 4 * C, EPI_BIAS_LS_RES, w.ones, x, flag, st));
        }
        POPE_TRY(tap(i + 1, x, C));
    }
    const int C3 = w.dims[3];
    float* feat = a.features ? a.features : feat_ws;
    if (a.features || a.logits) {
        hipLaunchKernelGGL(tail_kernel, dim3(B), dim3(256), size_t(C3) * 4, st, x, w.norm_w, w.norm_b, feat, hh * ww, C3);
        POPE_TRY(pope_check_launch());
    }
    if (a.logits) {
        GemmParams g = pope_linear_params(LINEAR_F32, feat, w.head_w, w.head_b, a.logits, nullptr, B, w.num_classes, C3, EPI_BIAS, nullptr, nullptr, 0, flag);
        if (prec == POPE_PREC_F16X3 && pope_gemm_f16x3_supported(g)) return pope_launch_gemm_nt_f16x3(g, st);
        g.range_flag = nullptr;
        return pope_launch_gemm_nt_f32(g, st);
    }
    return POPE_OK;
}
