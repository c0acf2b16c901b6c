// SAM prompt encoder, mask prompts (segment_anything/modeling/prompt_encoder.py:51-59, 102-105): mask_downscaling =
// Conv2d(1 -> 4, k2, s2), LayerNorm2d(4), GELU, Conv2d(4 -> 16, k2, s2), LayerNorm2d(16), GELU, Conv2d(16 -> 256, k1) in one
// kernel, masks [P, 1, 256, 256] -> dense [P, 256, 64, 64] (channel-major, what sd_prep_kernel of sam_decoder.hip reads).
//
// Both strided convolutions have kernel = stride, so the chain is local: an output pixel reads one 4 x 4 patch of its mask,
// i.e. four 2 x 2 positions x 4 channels after the first convolution, 16 channels after the second, and 256 dot products of
// length 16 after that.  Nothing between the mask and the embedding touches memory.
//
// Threads lie along the pixel index and a lane owns 4 consecutive pixels (every value below is an f32x4 over them): it loads
// 4 patch rows of 16 floats (a wave: whole 1 KiB mask rows), keeps the 16 hidden values of its pixels in registers, and for
// every output channel stores 16 bytes, so a wave's store is a 1 KiB run of dense[p, c, :].  The kernel is store-bound (4 MiB
// written, 256 KiB read, ~33 MFLOP per prompt), and the hidden values cost about as many instructions as 50 output channels:
// a block owns 1024 pixels x 64 channels (gridDim.y = 4 channel groups recompute the hidden values; profiles/sam_mask_prompt.md).
// All weights are indexed by compile-time or wave-uniform values and come through scalar loads (const __restrict__ arguments).
//
// Arithmetic, fixed per output element: a convolution starts from its bias and adds its taps in (dy, dx, c_in) order, the last
// layer its hidden channels 0..15 in order, each step one fused multiply-add; LayerNorm2d sums its channels as a balanced
// tree; 1 / sqrt and the GELU are the library's (common.h).  No value depends on P, on the prompt's place in the batch or on
// the launch geometry.
#include "common.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int SIDE = 256, GRID = 64, NPIX = GRID * GRID, C1 = 4, C2 = 16, C3 = 256;
constexpr int THREADS = 256, LANE_PIX = 4, BLOCK_PIX = THREADS * LANE_PIX, BLOCK_CH = 64;
constexpr int TILES = NPIX / BLOCK_PIX;   // pixel tiles of a prompt
constexpr int MAX_P = 1 << 28;            // gridDim.x = TILES * P

__device__ __forceinline__ f32x4 splat(float v) { return f32x4{v, v, v, v}; }
__device__ __forceinline__ f32x4 fma4(float w, f32x4 x, f32x4 acc) { return __builtin_elementwise_fma(splat(w), x, acc); }

// common.py LayerNorm2d over the N channels of x (per pixel), then GELU, in place
template <int N>
__device__ __forceinline__ void ln2d_gelu(f32x4 (&x)[N], const float* __restrict__ w, const float* __restrict__ b, float eps) {
    f32x4 t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = x[i];
#pragma unroll
    for (int n = N / 2; n > 0; n /= 2)
#pragma unroll
        for (int i = 0; i < n; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    const f32x4 mean = t[0] * (1.f / N);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x[i] = x[i] - mean;
        t[i] = x[i] * x[i];
    }
#pragma unroll
    for (int n = N / 2; n > 0; n /= 2)
#pragma unroll
        for (int i = 0; i < n; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    const f32x4 var = t[0] * (1.f / N) + eps;
    f32x4 rstd;
#pragma unroll
    for (int j = 0; j < LANE_PIX; ++j) rstd[j] = 1.f / __builtin_sqrtf(var[j]);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const f32x4 y = (x[i] * rstd) * w[i] + b[i];
#pragma unroll
        for (int j = 0; j < LANE_PIX; ++j) x[i][j] = pope_gelu_erf(y[j]);
    }
}

// The 16 hidden values (after the second LayerNorm2d + GELU) of the 4 pixels whose patches start at `in`
__device__ __forceinline__ void mask_hidden(const float* __restrict__ in, const float* __restrict__ w1, const float* __restrict__ b1,
                                            const float* __restrict__ g1, const float* __restrict__ s1, float eps1,
                                            const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ g2,
                                            const float* __restrict__ s2, float eps2, f32x4 (&h2)[C2]) {
    f32x4 patch[4][LANE_PIX];   // [patch row][pixel] = the 4 mask columns of that pixel
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < LANE_PIX; ++j) patch[r][j] = *reinterpret_cast<const f32x4*>(in + r * SIDE + 4 * j);

    // Conv2d(1 -> 4, k2, s2) + LayerNorm2d + GELU at the four positions (py, px) of the patch
    f32x4 h1[4][C1];
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px) {
            f32x4(&h)[C1] = h1[2 * py + px];
#pragma unroll
            for (int c = 0; c < C1; ++c) {
                f32x4 acc = splat(b1[c]);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int r = 2 * py + dy, cx = 2 * px + dx;
                        const f32x4 v = {patch[r][0][cx], patch[r][1][cx], patch[r][2][cx], patch[r][3][cx]};
                        acc = fma4(w1[c * 4 + dy * 2 + dx], v, acc);
                    }
                h[c] = acc;
            }
            ln2d_gelu<C1>(h, g1, s1, eps1);
        }

    // Conv2d(4 -> 16, k2, s2) + LayerNorm2d + GELU: weight [k, c_in, dy, dx], position dy * 2 + dx of h1
#pragma unroll
    for (int k = 0; k < C2; ++k) {
        f32x4 acc = splat(b2[k]);
#pragma unroll
        for (int pos = 0; pos < 4; ++pos)
#pragma unroll
            for (int ci = 0; ci < C1; ++ci) acc = fma4(w2[k * (C1 * 4) + ci * 4 + pos], h1[pos][ci], acc);
        h2[k] = acc;
    }
    ln2d_gelu<C2>(h2, g2, s2, eps2);
}

__global__ __launch_bounds__(THREADS) void sam_mask_embed_kernel(
    const float* __restrict__ masks, float* __restrict__ dense, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ g1, const float* __restrict__ s1, float eps1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ g2, const float* __restrict__ s2, float eps2,
    const float* __restrict__ w3, const float* __restrict__ b3) {
    const int p = blockIdx.x / TILES, tile = blockIdx.x % TILES;
    const int c0 = blockIdx.y * BLOCK_CH;
    const int pix = tile * BLOCK_PIX + threadIdx.x * LANE_PIX;   // the first of this lane's pixels: row y, columns x .. x + 3
    const int y = pix / GRID, x = pix % GRID;
    f32x4 h2[C2];
    mask_hidden(masks + size_t(p) * (SIDE * SIDE) + size_t(4 * y) * SIDE + 4 * x, w1, b1, g1, s1, eps1, w2, b2, g2, s2, eps2, h2);

    // Conv2d(16 -> 256, k1): this block's channels, one 16-byte store per lane and channel
    float* out = dense + (size_t(p) * C3 + c0) * NPIX + pix;
#pragma unroll 4
    for (int c = 0; c < BLOCK_CH; ++c) {
        const float* wc = w3 + (c0 + c) * C2;
        f32x4 acc = splat(b3[c0 + c]);
#pragma unroll
        for (int k = 0; k < C2; ++k) acc = fma4(wc[k], h2[k], acc);
        *reinterpret_cast<f32x4*>(out + size_t(c) * NPIX) = acc;
    }
}

}  // namespace

int pope_sam_mask_embed_check(const pope_sam_mask_embed_weights* w, const float* masks, int P, const float* dense) {
    if (!w || !masks || !dense || P <= 0 || P > MAX_P) return POPE_ERR_ARG;
    if (w->mask_in_chans != C2 || w->embed_dim != C3 || w->grid != GRID) return POPE_ERR_ARG;
    const void* ptrs[] = {w->conv1_w, w->conv1_b, w->ln1_w, w->ln1_b, w->conv2_w, w->conv2_b, w->ln2_w, w->ln2_b, w->conv3_w, w->conv3_b};
    for (const void* q : ptrs)
        if (!q) return POPE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(masks) | reinterpret_cast<uintptr_t>(dense)) & 15) return POPE_ERR_ARG;   // 16-byte loads and stores
    return POPE_OK;
}

int pope_launch_sam_mask_embed(const pope_sam_mask_embed_weights* w, const float* masks, int P, float* dense, hipStream_t stream) {
    POPE_TRY(pope_sam_mask_embed_check(w, masks, P, dense));
    static_assert(NPIX % BLOCK_PIX == 0 && C3 % BLOCK_CH == 0 && GRID % LANE_PIX == 0, "a block owns whole tiles");
    hipLaunchKernelGGL(sam_mask_embed_kernel, dim3(TILES * P, C3 / BLOCK_CH), dim3(THREADS), 0, stream, masks, dense, w->conv1_w,
                       w->conv1_b, w->ln1_w, w->ln1_b, w->ln1_eps, w->conv2_w, w->conv2_b, w->ln2_w, w->ln2_b, w->ln2_eps, w->conv3_w,
                       w->conv3_b);
    return pope_check_launch();
}
