// Row-tile pieces of the d_model = 76 transformer layers, shared by pose_regressor.hip (nhead = 2 encoder layer) and mocope.hip
// (the FFN of the nhead = 1 encoder / decoder layers): products on the exact fp32 MFMA in TRANSPOSED form,
// D^T[n][row] = W[n][:] . X[row][:]^T (see pose_regressor.hip).  Workgroups of 256 threads, rows in LDS at pitch XP.
#pragma once
#include "common.h"

namespace posereg_tile {

constexpr int D = 76, HID = 2048, HD = 38;
constexpr int XP = 77;     // LDS pitch of a 76-wide row

// a lane's B operands of a K = 76 product: x[row = rb * 32 + lane % 32][coff + 38 * (lane / 32) + s]
template <int RB>
__device__ __forceinline__ void load_rows(const float* buf, int pitch, int coff, float (&xb)[RB][HD]) {
    const int lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int s = 0; s < HD; ++s) xb[rb][s] = buf[(rb * 32 + l32) * pitch + coff + h * HD + s];
}

// the lane's half of a weight row (38 floats at wrow, 8-byte aligned; null: a row past the matrix, zeros)
__device__ __forceinline__ void load_wrow(const float* wrow, f32x2 (&wv)[19]) {
#pragma unroll
    for (int i = 0; i < 19; ++i) wv[i] = wrow ? *reinterpret_cast<const f32x2*>(wrow + 2 * i) : f32x2{0.f, 0.f};
}

// acc[rb][v] += sum_k W[n0 + lane % 32][k] * x[rb * 32 + lane % 32][k]: D^T fragment, register v = row n0 + mfma32_row(v, half) of
// W, lane % 32 = the activation row
template <int RB>
__device__ __forceinline__ void mm76(const f32x2 (&wv)[19], const float (&xb)[RB][HD], f32x16 (&acc)[RB]) {
#pragma unroll
    for (int s = 0; s < HD; ++s)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[rb] = mfma_32x32x2(wv[s >> 1][s & 1], xb[rb][s], acc[rb]);
}

__device__ __forceinline__ void layernorm_row(const float* src, float* dst, const float* w, const float* b) {
    float mean = 0.f;
    for (int c = 0; c < D; ++c) mean += src[c];
    mean *= (1.0f / D);
    float var = 0.f;
    for (int c = 0; c < D; ++c) { const float d = src[c] - mean; var += d * d; }
    const float rstd = 1.0f / sqrtf(var * (1.0f / D) + 1e-5f);
    for (int c = 0; c < D; ++c) dst[c] = (src[c] - mean) * rstd * w[c] + b[c];
}

// ys[row] = xs[row] + linear2(relu(linear1(xs[row]))) for the RT = 32 RB rows of the tile (pre-LayerNorm sums); red: [2][96][RT]
// floats of LDS for the partial sums.  Every thread of the workgroup calls it; ends behind a barrier.
template <int RB>
__device__ __forceinline__ void ffn76_tile(const float* __restrict__ l1w, const float* __restrict__ l1b, const float* __restrict__ l2w,
                                           const float* __restrict__ l2b, const float* xs, float* ys, float* red) {
    constexpr int RT = 32 * RB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
    float xb[RB][HD];
    // FFN: this wave's chunks of 32 hidden columns; H^T = relu(W1 x^T + b1) stays in the accumulators and feeds W2 H^T directly
    load_rows<RB>(xs, XP, 0, xb);
    f32x16 accY[RB][3] = {};
    f32x2 wv[19];
    load_wrow(l1w + size_t(wave * 32 + l32) * D + h * HD, wv);
    for (int ci = 0; ci < HID / 128; ++ci) {
        const int hid0 = (wave + 4 * ci) * 32;
        f32x2 wn[19];
        if (ci + 1 < HID / 128) load_wrow(l1w + size_t(hid0 + 128 + l32) * D + h * HD, wn);
        f32x4 w2[3][4], b1[4];
#pragma unroll
        for (int nb = 0; nb < 3; ++nb) {
            const int n = nb * 32 + l32;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                w2[nb][g] = n < D ? *reinterpret_cast<const f32x4*>(l2w + size_t(n) * HID + hid0 + 8 * g + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) b1[g] = *reinterpret_cast<const f32x4*>(l1b + hid0 + 8 * g + 4 * h);
        f32x16 accH[RB] = {};
        mm76<RB>(wv, xb, accH);
#pragma unroll
        for (int s = 0; s < 16; ++s) {     // register s = hidden column hid0 + 8 (s / 4) + 4 half + s % 4: the K index of this step
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const float hv = fmaxf(accH[rb][s] + b1[s >> 2][s & 3], 0.f);
#pragma unroll
                for (int nb = 0; nb < 3; ++nb) accY[rb][nb] = mfma_32x32x2(w2[nb][s >> 2][s & 3], hv, accY[rb][nb]);
            }
        }
        if (ci + 1 < HID / 128) {
#pragma unroll
            for (int i = 0; i < 19; ++i) wv[i] = wn[i];
        }
    }
    // (wave 0 + wave 2) + (wave 1 + wave 3), through LDS as [n][row]
    auto red_at = [&](int buf, int rb, int nb, int v) { return red + (size_t(buf) * 96 + nb * 32 + mfma32_row(v, h)) * RT + rb * 32 + l32; };
    if (wave >= 2) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int nb = 0; nb < 3; ++nb)
#pragma unroll
                for (int v = 0; v < 16; ++v) *red_at(wave - 2, rb, nb, v) = accY[rb][nb][v];
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int nb = 0; nb < 3; ++nb)
#pragma unroll
                for (int v = 0; v < 16; ++v) accY[rb][nb][v] += *red_at(wave, rb, nb, v);
    }
    __syncthreads();
    if (wave == 1) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int nb = 0; nb < 3; ++nb)
#pragma unroll
                for (int v = 0; v < 16; ++v) *red_at(0, rb, nb, v) = accY[rb][nb][v];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int nb = 0; nb < 3; ++nb)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int nn = nb * 32 + mfma32_row(v, h);
                if (nn < D) {
                    const float bias = l2b[nn];
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        const int row = rb * 32 + l32;
                        ys[row * XP + nn] = xs[row * XP + nn] + ((accY[rb][nb][v] + *red_at(0, rb, nb, v)) + bias);
                    }
                }
            }
    }
    __syncthreads();
}

}  // namespace posereg_tile
