// MoCoPE fusion pose model: pose/model0604.py:MoCoPE.forward after the backbone, from the matcher's matches and the two images'
// logits to (t, R), fp32 throughout.  What it adds to pose_regressor.hip is a full nn.Transformer (6 post-norm encoder layers +
// encoder.norm, 6 decoder layers with cross-attention to the encoder memory + decoder.norm, nhead = 1) at d_model 76
// (transformer_mkpts, rows = B S) and 512 (mkpts_as_q / cnn_as_q, rows = 2 B <= 128 in a group call).  Select / embed, the
// streamed Linear + LeakyReLU (mlp1, mlp_img, mlp2.0, mlp2.3) and the tail (mlp2.6 .. 18, heads, convert2matrix) are
// pose_regressor.hip's own launches.
//
//   linear     Y[r][n] = act(A[r][:] . W[n][:] + bias[n]): weight streaming.  A wave owns RW output rows n (2 for N <= 1024, else
//              4: N / RW one-wave workgroups, so a [512, 512] matrix still spreads over 256 of them) and a chunk of 8 activation
//              rows, reads its weight rows once in coalesced 16-byte loads and applies them to the 8 rows, which stay in
//              registers as accumulators.  Lane l sums the 16-byte groups l, l + 64, .. of K in order, then a xor butterfly: the
//              order of an output element depends on K alone.  Epilogues: bias, bias + ReLU.  q | k | v are one launch over
//              in_proj (N = 3 d); for a group of one both attentions are out_proj(v_proj(.)) and only the v third is read;
//              the cross-attention reads the q third on the target rows and the k | v thirds on the memory rows.
//   attention  one wave per query row: the G <= 64 scores of its group (lane g keeps score g), softmax, sum of p_g v_g.
//   ffn76      d = 76 only: linear1 + ReLU + linear2 + residual + LayerNorm (+ the closing norm) of a 32-row tile in one launch on the
//              fp32 MFMA, the hidden activation in the accumulators (posereg_tile.h).  d = 512 runs its FFN as two linear launches.
//   add_ln     x = LayerNorm(x + y) per row by one wave (two-pass mean / variance), optionally followed by the closing
//              encoder.norm / decoder.norm in the same launch.
//
// LDS: only ffn76 uses any (44 KB, worked out at the kernel) — elsewhere a row lives in the registers of one wave (at most 8
// floats per lane at d = 512) and the memory rows of the cross-attention are read from global memory (L2: 76 or 512 floats per
// key), so no memory tile has to fit next to the other buffers.  The hidden activation of the d = 512 FFN goes through a
// [<= 4096, 2048] workspace buffer in row blocks.  Plain launches only, no cross-workgroup waiting.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "posereg_tile.h"

namespace {

constexpr int HID = 2048, NB = 8, FFN_ROWS = 4096, D1 = 76, D2 = 512, NIMG = 1000, MAX_GRID_Y = 65535;
enum { ACT_NONE = 0, ACT_RELU = 1 };

template <int RW>
__global__ __launch_bounds__(64) void mocope_linear_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ Y, int R, int K, int N,
                                                           int act) {
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * RW, r0 = blockIdx.y * NB;     // n0 < N and r0 < R by the grid
    const f32x4* w[RW];
    const f32x4* a[NB];
#pragma unroll
    for (int r = 0; r < RW; ++r) w[r] = reinterpret_cast<const f32x4*>(W + size_t(min(n0 + r, N - 1)) * K);   // past N: read again, dropped
#pragma unroll
    for (int b = 0; b < NB; ++b) a[b] = reinterpret_cast<const f32x4*>(A + size_t(min(r0 + b, R - 1)) * K);   // past R: likewise
    float acc[RW][NB];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
    const int steps = K >> 2;
    for (int i = lane; i < steps; i += 64) {
        f32x4 wv[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) wv[r] = w[r][i];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const f32x4 x = a[b][i];
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r][b] = fmaf(wv[r][e], x[e], acc[r][b]);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const float sum = wave_sum(acc[r][b]);
            if (lane == 0 && n0 + r < N && r0 + b < R) {
                float v = sum + bias[n0 + r];
                if (act == ACT_RELU) v = fmaxf(v, 0.f);
                Y[size_t(r0 + b) * N + n0 + r] = v;
            }
        }
}

// rows r = b * S + s of [B, S, d]; the group of row r: pairs (b / G) * G + g, g < G, at the same s.  NJ = ceil(d / 64).
template <int NJ>
__global__ __launch_bounds__(256) void mocope_attention_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kp, int ldk,
                                                              const float* __restrict__ V, int ldv, float* __restrict__ O, int R, int S,
                                                              int G, int d, float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= R) return;     // the whole wave
    const int b = row / S, s = row - b * S, b0 = (b / G) * G;
    float q[NJ], o[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        q[j] = c < d ? Q[size_t(row) * ldq + c] : 0.f;
        o[j] = 0.f;
    }
    float mine = -INFINITY;
    for (int g = 0; g < G; ++g) {
        const float* k = Kp + (size_t(b0 + g) * S + s) * ldk;
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            if (c < d) part = fmaf(q[j], k[c], part);
        }
        const float sc = wave_sum(part) * scale;
        if (lane == g) mine = sc;
    }
    const float m = wave_max(mine);
    const float e = lane < G ? expf(mine - m) : 0.f;
    const float p = e / wave_sum(e);
    for (int g = 0; g < G; ++g) {
        const float* v = V + (size_t(b0 + g) * S + s) * ldv;
        const float pg = __shfl(p, g);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            if (c < d) o[j] = fmaf(pg, v[c], o[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        if (c < d) O[size_t(row) * d + c] = o[j];
    }
}

template <int NJ>
__device__ __forceinline__ void layernorm_wave(float (&v)[NJ], const float* __restrict__ w, const float* __restrict__ b, int d) {
    const int lane = threadIdx.x & 63;
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) part += v[j];      // entries past d are 0
    const float mean = wave_sum(part) / float(d);
    part = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float c = v[j] - mean;
        if (lane + 64 * j < d) part += c * c;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(part) / float(d) + 1e-5f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < d ? (v[j] - mean) * rstd * w[c] + b[c] : 0.f;
    }
}

// X[row] = LayerNorm(X[row] + Y[row]; w1, b1), then LayerNorm(.; w2, b2) when w2 is given
template <int NJ>
__global__ __launch_bounds__(256) void mocope_add_ln_kernel(float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, int R, int d) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= R) return;
    float v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < d ? X[size_t(row) * d + c] + Y[size_t(row) * d + c] : 0.f;
    }
    layernorm_wave<NJ>(v, w1, b1, d);
    if (w2) layernorm_wave<NJ>(v, w2, b2, d);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        if (c < d) X[size_t(row) * d + c] = v[j];
    }
}

// d = 76: the FFN of a tile of 32 rows on the exact fp32 MFMA (posereg_tile.h, the key-point regressor's: transposed products, the
// [2048, rows] hidden activation never leaves the accumulators), then residual + LayerNorm and, in a stack's last layer, the closing
// norm.  LDS: xs and ys 2 x 32 x 77 floats, the partial sums of the four waves 2 x 96 x 32 floats: 44 288 bytes of the 160 KB.
__global__ __launch_bounds__(256) void mocope_ffn76_kernel(float* __restrict__ X, const float* l1w, const float* l1b, const float* l2w,
                                                          const float* l2b, const float* nw, const float* nb, const float* fw,
                                                          const float* fb, int R) {
    using namespace posereg_tile;
    __shared__ float xs[32 * XP], ys[32 * XP], red[2 * 96 * 32];
    const int tid = threadIdx.x, r0 = blockIdx.x * 32, nrows = min(32, R - r0);
    for (int i = tid; i < 32 * D; i += 256) {
        const int r = i / D, c = i - r * D;
        xs[r * XP + c] = r < nrows ? X[size_t(r0 + r) * D + c] : 0.f;     // rows past the tile are masked, not read
    }
    __syncthreads();
    ffn76_tile<1>(l1w, l1b, l2w, l2b, xs, ys, red);
    if (tid < 32) {
        layernorm_row(ys + tid * XP, xs + tid * XP, nw, nb);
        if (fw) layernorm_row(xs + tid * XP, ys + tid * XP, fw, fb);
    }
    __syncthreads();
    const float* out = fw ? ys : xs;
    for (int i = tid; i < nrows * D; i += 256) {
        const int r = i / D, c = i - r * D;
        X[size_t(r0 + r) * D + c] = out[r * XP + c];
    }
}

// dst[r][c] = src[r][c] for r < rows, c < cols, with row pitches lds / ldd
__global__ __launch_bounds__(256) void mocope_copy_kernel(const float* __restrict__ src, long long lds, float* __restrict__ dst, long long ldd,
                                                         long long rows, int cols) {
    const long long total = rows * cols;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += 256ll * gridDim.x) {
        const long long r = i / cols;
        const int c = int(i - r * cols);
        dst[r * ldd + c] = src[r * lds + c];
    }
}

int launch_copy(const float* src, long long lds, float* dst, long long ldd, long long rows, int cols, hipStream_t st) {
    hipLaunchKernelGGL(mocope_copy_kernel, dim3(pope_grid_for(rows * cols)), dim3(256), 0, st, src, lds, dst, ldd, rows, cols);
    return pope_check_launch();
}

int launch_linear(const float* A, const float* W, const float* bias, float* Y, int R, int K, int N, int act, hipStream_t st) {
    if (R <= 0 || N <= 0 || K <= 0 || (K & 3)) return POPE_ERR_ARG;
    const int chunks = (R + NB - 1) / NB;
    for (int c0 = 0; c0 < chunks; c0 += MAX_GRID_Y) {
        const int cy = std::min(MAX_GRID_Y, chunks - c0), rows = std::min(R - c0 * NB, cy * NB);
        const float* a = A + size_t(c0) * NB * K;
        float* y = Y + size_t(c0) * NB * N;
        if (N <= 1024)
            hipLaunchKernelGGL(mocope_linear_kernel<2>, dim3((N + 1) / 2, cy), dim3(64), 0, st, a, W, bias, y, rows, K, N, act);
        else
            hipLaunchKernelGGL(mocope_linear_kernel<4>, dim3((N + 3) / 4, cy), dim3(64), 0, st, a, W, bias, y, rows, K, N, act);
        POPE_TRY(pope_check_launch());
    }
    return POPE_OK;
}

int launch_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int R, int S, int G, int d,
                     hipStream_t st) {
    const float scale = 1.0f / sqrtf(float(d));
    const dim3 grid((R + 3) / 4), block(256);
    if (d == D1)
        hipLaunchKernelGGL(mocope_attention_kernel<2>, grid, block, 0, st, Q, ldq, K, ldk, V, ldv, O, R, S, G, d, scale);
    else
        hipLaunchKernelGGL(mocope_attention_kernel<8>, grid, block, 0, st, Q, ldq, K, ldk, V, ldv, O, R, S, G, d, scale);
    return pope_check_launch();
}

int launch_add_ln(float* X, const float* Y, const float* w1, const float* b1, const float* w2, const float* b2, int R, int d,
                  hipStream_t st) {
    const dim3 grid((R + 3) / 4), block(256);
    if (d == D1)
        hipLaunchKernelGGL(mocope_add_ln_kernel<2>, grid, block, 0, st, X, Y, w1, b1, w2, b2, R, d);
    else
        hipLaunchKernelGGL(mocope_add_ln_kernel<8>, grid, block, 0, st, X, Y, w1, b1, w2, b2, R, d);
    return pope_check_launch();
}

int launch_ffn76(float* X, const float* l1w, const float* l1b, const float* l2w, const float* l2b, const float* nw, const float* nb,
                 const float* fw, const float* fb, int R, hipStream_t st) {
    hipLaunchKernelGGL(mocope_ffn76_kernel, dim3((R + 31) / 32), dim3(256), 0, st, X, l1w, l1b, l2w, l2b, nw, nb, fw, fb, R);
    return pope_check_launch();
}

// scratch of a transformer over R rows of width d: qkv [R, 3 d], att [R, d], proj [R, d], hid [min(R, FFN_ROWS), 2048]
struct Scratch { float *qkv, *att, *proj, *hid; };
struct Dims { int R, S, G, d; };     // rows r = b * S + s, attention groups of G consecutive b

// x += attention(x as q; kv as k, v) through in_proj / out_proj, then LayerNorm: kv == x is the self-attention
int attention_block(float* x, const float* kv, const float* in_w, const float* in_b, const float* out_w, const float* out_b,
                    const float* nw, const float* nb, const Dims& m, const Scratch& s, hipStream_t st) {
    const int d = m.d, R = m.R;
    const size_t dd = size_t(d) * d;
    if (m.G == 1) {     // the softmax of one score is 1: out_proj(v_proj(kv row))
        POPE_TRY(launch_linear(kv, in_w + 2 * dd, in_b + 2 * d, s.att, R, d, d, ACT_NONE, st));
    } else if (kv == x) {
        POPE_TRY(launch_linear(x, in_w, in_b, s.qkv, R, d, 3 * d, ACT_NONE, st));
        POPE_TRY(launch_attention(s.qkv, 3 * d, s.qkv + d, 3 * d, s.qkv + 2 * d, 3 * d, s.att, R, m.S, m.G, d, st));
    } else {
        float* q = s.qkv;
        float* k = s.qkv + size_t(R) * d;      // [R, 2 d]: k | v
        POPE_TRY(launch_linear(x, in_w, in_b, q, R, d, d, ACT_NONE, st));
        POPE_TRY(launch_linear(kv, in_w + dd, in_b + d, k, R, d, 2 * d, ACT_NONE, st));
        POPE_TRY(launch_attention(q, d, k, 2 * d, k + d, 2 * d, s.att, R, m.S, m.G, d, st));
    }
    POPE_TRY(launch_linear(s.att, out_w, out_b, s.proj, R, d, d, ACT_NONE, st));
    return launch_add_ln(x, s.proj, nw, nb, nullptr, nullptr, R, d, st);
}

// x = LayerNorm(x + linear2(relu(linear1(x)))), then the closing norm when given
int ffn_block(float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* nw, const float* nb,
              const float* fw, const float* fb, const Dims& m, const Scratch& s, hipStream_t st) {
    if (m.d == D1) return launch_ffn76(x, w1, b1, w2, b2, nw, nb, fw, fb, m.R, st);
    for (int r0 = 0; r0 < m.R; r0 += FFN_ROWS) {
        const int rows = std::min(FFN_ROWS, m.R - r0);
        POPE_TRY(launch_linear(x + size_t(r0) * m.d, w1, b1, s.hid, rows, m.d, HID, ACT_RELU, st));
        POPE_TRY(launch_linear(s.hid, w2, b2, s.proj + size_t(r0) * m.d, rows, HID, m.d, ACT_NONE, st));
    }
    return launch_add_ln(x, s.proj, nw, nb, fw, fb, m.R, m.d, st);
}

int encoder(const pope_mocope_transformer& t, float* src, const Dims& m, const Scratch& s, hipStream_t st) {
    for (int i = 0; i < 6; ++i) {
        const pope_mocope_encoder_layer& l = t.enc[i];
        const bool last = i == 5;
        POPE_TRY(attention_block(src, src, l.in_proj_w, l.in_proj_b, l.out_proj_w, l.out_proj_b, l.norm1_w, l.norm1_b, m, s, st));
        POPE_TRY(ffn_block(src, l.linear1_w, l.linear1_b, l.linear2_w, l.linear2_b, l.norm2_w, l.norm2_b, last ? t.enc_norm_w : nullptr,
                           last ? t.enc_norm_b : nullptr, m, s, st));
    }
    return POPE_OK;
}

int decoder(const pope_mocope_transformer& t, const float* memory, float* tgt, const Dims& m, const Scratch& s, hipStream_t st) {
    for (int i = 0; i < 6; ++i) {
        const pope_mocope_decoder_layer& l = t.dec[i];
        const bool last = i == 5;
        POPE_TRY(attention_block(tgt, tgt, l.in_proj_w, l.in_proj_b, l.out_proj_w, l.out_proj_b, l.norm1_w, l.norm1_b, m, s, st));
        POPE_TRY(attention_block(tgt, memory, l.cross_in_proj_w, l.cross_in_proj_b, l.cross_out_proj_w, l.cross_out_proj_b, l.norm2_w,
                                 l.norm2_b, m, s, st));
        POPE_TRY(ffn_block(tgt, l.linear1_w, l.linear1_b, l.linear2_w, l.linear2_b, l.norm3_w, l.norm3_b, last ? t.dec_norm_w : nullptr,
                           last ? t.dec_norm_b : nullptr, m, s, st));
    }
    return POPE_OK;
}

// nn.Transformer(src, tgt): src becomes the memory, tgt the result (both in place; src != tgt)
int transformer(const pope_mocope_transformer& t, float* src, float* tgt, const Dims& m, const Scratch& s, hipStream_t st) {
    POPE_TRY(encoder(t, src, m, s, st));
    return decoder(t, src, tgt, m, s, st);
}

struct Layout { size_t x, y, index, qkv, att, proj, hid, y1, xm, f0, f1, xi, s1, t1, cat, z1, z2, total; };
Layout layout(int B, int S) {
    Layout l;
    const size_t b = size_t(B), r1 = b * size_t(S), r2 = 2 * b, f = sizeof(float);
    l.x = l.y = pope_align256(r1 * D1 * f);
    l.index = pope_align256(r1 * sizeof(int));
    l.qkv = pope_align256(std::max(r1 * 3 * D1, r2 * 3 * D2) * f);
    l.att = l.proj = pope_align256(std::max(r1 * D1, r2 * D2) * f);
    l.hid = pope_align256(std::min(std::max(r1, r2), size_t(FFN_ROWS)) * HID * f);
    l.y1 = pope_align256(r1 * 38 * f);
    l.xm = l.xi = l.s1 = l.t1 = l.z1 = pope_align256(b * 1024 * f);
    l.f0 = l.f1 = l.z2 = pope_align256(b * 512 * f);
    l.cat = pope_align256(b * 2048 * f);
    l.total = l.x + l.y + l.index + l.qkv + l.att + l.proj + l.hid + l.y1 + l.xm + l.f0 + l.f1 + l.xi + l.s1 + l.t1 + l.cat + l.z1 + l.z2;
    return l;
}

bool transformer_ok(const pope_mocope_transformer& t, uintptr_t& bits) {
    bool all = true;
    auto see = [&](const float* p) { all = all && p; bits |= reinterpret_cast<uintptr_t>(p); };
    for (const pope_mocope_encoder_layer& l : t.enc)
        for (const float* p : {l.in_proj_w, l.in_proj_b, l.out_proj_w, l.out_proj_b, l.linear1_w, l.linear1_b, l.linear2_w, l.linear2_b,
                               l.norm1_w, l.norm1_b, l.norm2_w, l.norm2_b}) see(p);
    for (const pope_mocope_decoder_layer& l : t.dec)
        for (const float* p : {l.in_proj_w, l.in_proj_b, l.out_proj_w, l.out_proj_b, l.cross_in_proj_w, l.cross_in_proj_b, l.cross_out_proj_w,
                               l.cross_out_proj_b, l.linear1_w, l.linear1_b, l.linear2_w, l.linear2_b, l.norm1_w, l.norm1_b, l.norm2_w,
                               l.norm2_b, l.norm3_w, l.norm3_b}) see(p);
    for (const float* p : {t.enc_norm_w, t.enc_norm_b, t.dec_norm_w, t.dec_norm_b}) see(p);
    return all;
}

bool weights_ok(const pope_mocope_weights* w, int S) {
    if (!w || w->num_sample != S || w->mode < POPE_ROT_MATRIX || w->mode > POPE_ROT_6D) return false;
    uintptr_t bits = 0;
    bool all = transformer_ok(w->transformer_mkpts, bits) && transformer_ok(w->mkpts_as_q, bits) && transformer_ok(w->cnn_as_q, bits);
    auto see = [&](const float* p) { all = all && p; bits |= reinterpret_cast<uintptr_t>(p); };
    for (int i = 0; i < 2; ++i) { see(w->mlp1_w[i]); see(w->mlp1_b[i]); }
    for (int i = 0; i < 7; ++i) { see(w->mlp2_w[i]); see(w->mlp2_b[i]); }
    for (const float* p : {w->mlp_img_w, w->mlp_img_b, w->trans_w, w->trans_b, w->rot_w, w->rot_b}) see(p);
    return all && !(bits & 15);
}

bool stage_ok(int stage, int train_type) {
    if (stage == MOCOPE_STAGE_FULL) return true;
    if (stage < POPE_MOCOPE_TAP_EMBEDDING || stage > POPE_MOCOPE_TAP_QIMG) return false;
    if (train_type == POPE_MOCOPE_MKPTS) return stage != POPE_MOCOPE_TAP_X_IMG && stage != POPE_MOCOPE_TAP_QIMG;
    if (train_type == POPE_MOCOPE_CNN) return stage == POPE_MOCOPE_TAP_X_IMG || stage == POPE_MOCOPE_TAP_QIMG;
    return true;
}

}  // namespace

int pope_launch_mocope_linear(const float* A, const float* W, const float* bias, float* Y, int R, int K, int N, int act, hipStream_t st) {
    return launch_linear(A, W, bias, Y, R, K, N, act, st);
}

int pope_launch_mocope_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int R, int S, int G,
                                 int d, hipStream_t st) {
    return launch_attention(Q, ldq, K, ldk, V, ldv, O, R, S, G, d, st);
}

int pope_launch_mocope_add_ln(float* X, const float* Y, const float* w1, const float* b1, const float* w2, const float* b2, int R, int d,
                              hipStream_t st) {
    return launch_add_ln(X, Y, w1, b1, w2, b2, R, d, st);
}

int pope_launch_mocope_ffn76(float* X, const float* l1w, const float* l1b, const float* l2w, const float* l2b, const float* nw,
                             const float* nb, const float* fw, const float* fb, int R, hipStream_t st) {
    return launch_ffn76(X, l1w, l1b, l2w, l2b, nw, nb, fw, fb, R, st);
}

size_t pope_mocope_workspace(int B, int S) { return B > 0 && S > 0 ? layout(B, S).total : 0; }

int pope_mocope_check(const MocopeArgs& a) {
    POPE_TRY(pope_posereg_input_check(a.in));
    if (!weights_ok(a.w, a.in.S) || !a.status || a.G < 1 || a.G > 64 || a.in.B % a.G) return POPE_ERR_ARG;
    if (a.train_type < POPE_MOCOPE_FUSION || a.train_type > POPE_MOCOPE_CNN || !stage_ok(a.stage, a.train_type)) return POPE_ERR_ARG;
    if (a.train_type != POPE_MOCOPE_MKPTS && (!a.feat0 || !a.feat1)) return POPE_ERR_ARG;
    if (a.stage == MOCOPE_STAGE_FULL ? (!a.trans || !a.rot) : !a.tap_out) return POPE_ERR_ARG;
    if (size_t(a.in.B) * a.in.S * 3 * D1 >= (size_t(1) << 31) || a.in.B >= (1 << 19)) return POPE_ERR_ARG;
    if (!a.ws || (reinterpret_cast<uintptr_t>(a.ws) & 255)) return POPE_ERR_ARG;
    if (a.ws_bytes < layout(a.in.B, a.in.S).total) return POPE_ERR_WORKSPACE;
    return POPE_OK;
}

int pope_launch_mocope(const MocopeArgs& a, hipStream_t st) {
    POPE_TRY(pope_mocope_check(a));
    const pope_mocope_weights& w = *a.w;
    const int B = a.in.B, S = a.in.S, G = a.G;
    const Layout lay = layout(B, S);
    pope_carver ws{static_cast<char*>(a.ws)};
    float* X = ws.take<float>(lay.x);
    float* Y = ws.take<float>(lay.y);
    int* index = ws.take<int>(lay.index);
    Scratch s;
    s.qkv = ws.take<float>(lay.qkv);
    s.att = ws.take<float>(lay.att);
    s.proj = ws.take<float>(lay.proj);
    s.hid = ws.take<float>(lay.hid);
    float* y1 = ws.take<float>(lay.y1);
    float* xm = ws.take<float>(lay.xm);
    float* f0 = ws.take<float>(lay.f0);
    float* f1 = ws.take<float>(lay.f1);
    float* xi = ws.take<float>(lay.xi);
    float* s1 = ws.take<float>(lay.s1);
    float* t1 = ws.take<float>(lay.t1);
    float* cat = ws.take<float>(lay.cat);
    float* z1 = ws.take<float>(lay.z1);
    float* z2 = ws.take<float>(lay.z2);
    const long long n76 = (long long)B * S * D1, n1024 = (long long)B * 1024;
    auto tap = [&](const float* src, long long n) { return launch_copy(src, n, a.tap_out, n, 1, int(n), st); };

    // status of every pair, and the embedding where the route reads key points
    POPE_TRY(pope_launch_posereg_embed(a.in, X, index, a.status, st));
    if (a.stage == POPE_MOCOPE_TAP_EMBEDDING) return tap(X, n76);
    const bool mk = a.train_type != POPE_MOCOPE_CNN, im = a.train_type != POPE_MOCOPE_MKPTS;
    if (mk) {
        const Dims m = {B * S, S, G, D1};
        POPE_TRY(launch_copy(X, n76, Y, n76, 1, int(n76), st));       // transformer_mkpts(x, x): src and tgt start equal
        POPE_TRY(encoder(w.transformer_mkpts, X, m, s, st));
        if (a.stage == POPE_MOCOPE_TAP_MEMORY) return tap(X, n76);
        POPE_TRY(decoder(w.transformer_mkpts, X, Y, m, s, st));
        if (a.stage == POPE_MOCOPE_TAP_MKPTS_T) return tap(Y, n76);
        POPE_TRY(pope_launch_posereg_stream_linear(Y, w.mlp1_w[0], w.mlp1_b[0], y1, B, 76ll * S, 38 * S, st));
        POPE_TRY(pope_launch_posereg_stream_linear(y1, w.mlp1_w[1], w.mlp1_b[1], xm, B, 38ll * S, 1024, st));
        if (a.stage == POPE_MOCOPE_TAP_X_MKPTS) return tap(xm, n1024);
    }
    if (im) {   // x_img[b] = (mlp_img(feat0[b]), mlp_img(feat1[b]))
        POPE_TRY(pope_launch_posereg_stream_linear(a.feat0, w.mlp_img_w, w.mlp_img_b, f0, B, NIMG, D2, st));
        POPE_TRY(pope_launch_posereg_stream_linear(a.feat1, w.mlp_img_w, w.mlp_img_b, f1, B, NIMG, D2, st));
        POPE_TRY(launch_copy(f0, D2, xi, 2 * D2, B, D2, st));
        POPE_TRY(launch_copy(f1, D2, xi + D2, 2 * D2, B, D2, st));
        if (a.stage == POPE_MOCOPE_TAP_X_IMG) return tap(xi, n1024);
    }
    // fusion: rows r = b * 2 + j of [B, 2, 512], groups across the pairs.  qm / qi: where the two results end up
    const Dims m2 = {2 * B, 2, G, D2};
    const float *qm = nullptr, *qi = nullptr;
    if (a.train_type == POPE_MOCOPE_FUSION) {
        POPE_TRY(launch_copy(xi, n1024, s1, n1024, 1, int(n1024), st));
        POPE_TRY(launch_copy(xm, n1024, t1, n1024, 1, int(n1024), st));
        POPE_TRY(transformer(w.mkpts_as_q, s1, t1, m2, s, st));        // mkpts_as_q(src = x_img, tgt = x_mkpts)
        if (a.stage == POPE_MOCOPE_TAP_QMKPTS) return tap(t1, n1024);
        POPE_TRY(transformer(w.cnn_as_q, xm, xi, m2, s, st));          // cnn_as_q(src = x_mkpts, tgt = x_img)
        if (a.stage == POPE_MOCOPE_TAP_QIMG) return tap(xi, n1024);
        qm = t1; qi = xi;
    } else if (a.train_type == POPE_MOCOPE_MKPTS) {
        POPE_TRY(launch_copy(xm, n1024, t1, n1024, 1, int(n1024), st));
        POPE_TRY(transformer(w.mkpts_as_q, xm, t1, m2, s, st));
        if (a.stage == POPE_MOCOPE_TAP_QMKPTS) return tap(t1, n1024);
        qm = qi = t1;
    } else {
        POPE_TRY(launch_copy(xi, n1024, t1, n1024, 1, int(n1024), st));
        POPE_TRY(transformer(w.cnn_as_q, xi, t1, m2, s, st));
        if (a.stage == POPE_MOCOPE_TAP_QIMG) return tap(t1, n1024);
        qm = qi = t1;
    }
    // cat(qmkpts, qimg, dim=-1) of [B, 2, 512] each -> [B, 2, 1024] -> [B, 2048]
    POPE_TRY(launch_copy(qm, D2, cat, 2 * D2, 2ll * B, D2, st));
    POPE_TRY(launch_copy(qi, D2, cat + D2, 2 * D2, 2ll * B, D2, st));
    POPE_TRY(pope_launch_posereg_stream_linear(cat, w.mlp2_w[0], w.mlp2_b[0], z1, B, 2048, 1024, st));
    POPE_TRY(pope_launch_posereg_stream_linear(z1, w.mlp2_w[1], w.mlp2_b[1], z2, B, 1024, 512, st));
    // mlp2.6 .. 18 and the heads are the key-point regressor's tail over a 512-wide input
    pope_pose_regressor_weights tw = {};
    tw.num_sample = D2;
    tw.mode = w.mode;
    for (int i = 2; i < 7; ++i) { tw.mlp_w[i] = w.mlp2_w[i]; tw.mlp_b[i] = w.mlp2_b[i]; }
    tw.trans_w = w.trans_w; tw.trans_b = w.trans_b; tw.rot_w = w.rot_w; tw.rot_b = w.rot_b;
    return pope_launch_posereg_tail(tw, z2, a.status, B, a.trans, a.rot, st);
}
