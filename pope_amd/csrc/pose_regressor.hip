// Learned pose regressor: pose/model.py:Mkpts_Reg_Model.forward (the fork's head on top of upstream POPE) from the matcher's
// compacted matches to (t, R), fp32 throughout.
//
//   select   one workgroup per pair: offset of the pair's matches from the counts, refusal of corrupt counts (as pose.hip),
//            and the S sample slots -> match indices (identity + zero padding, a host-supplied index, or the device sampler:
//            the S smallest (splitmix64 key, i), a uniform ordered sample without replacement like random.sample)
//   embed    [x, sin(f x), cos(f x), ...] of the 4-vector (kpts0, kpts1), f = 1 + 31.875 k (torch.linspace(1, 256, 9), exact in
//            fp32); the ARGUMENT is the fp32-rounded product (the reference multiplies in fp32 at up to 1.6e5 rad), then
//            full-range sinf / cosf
//   layer    one nn.TransformerEncoderLayer(76, nhead=2) per launch (post-norm, ReLU, 2048 hidden).  A workgroup owns a tile of
//            sample slots and all G members of their attention group: QKV -> 2-head attention over the G members (G = 1: the
//            softmax of one score is 1, only V is projected) -> out_proj + residual + LayerNorm1 -> FFN -> residual +
//            LayerNorm2.  Every product runs on the exact fp32 MFMA in TRANSPOSED form, D^T[n][row] = W[n][:] . X[row][:]^T:
//            the weights are the A operand straight from global memory (L2), a lane's 38 x values per row block stay in
//            registers, and the [2048, rows] hidden activation of the FFN never leaves the accumulators — the C fragment of the
//            first product (lane = row, register = hidden column) IS the B fragment of the second, with the K order of that
//            product permuted to match (both operands alike, so the same products are summed).  Each wave owns every fourth
//            32-column chunk of the hidden width; the four partial sums meet in a fixed tree through LDS.
//   stream   mlp.0 ([19 S, 76 S]: 1.44 GB at S = 500) and mlp.3: every weight element is read once per chunk of 8 pairs in
//            coalesced 16-byte loads (a wave streams four weight rows at once) and applied to all rows of the chunk; a row's
//            summation order (lane-strided partial sums, xor butterfly) does not depend on B or on the chunk.  64-bit indexing.
//   tail     mlp.6 .. mlp.18, both heads and convert2matrix by one workgroup per pair.
#include "common.h"
#include "kernels.h"
#include "pose_math.h"
#include "posereg_tile.h"
#include "rot_convert.h"

namespace {

using namespace posereg_tile;
constexpr int NQKV = 228;
constexpr int QP = 229;    // LDS pitch of a q | k | v row
constexpr int CH = 8;      // pairs per weight read of the streamed Linear (pose_regressor.py ROW_CHUNK)
constexpr int KEY_TILE = 1024;

__device__ __forceinline__ unsigned long long sample_key(unsigned long long seed, int i) {
    return pose::splitmix64(seed ^ ((unsigned long long)(i + 1) * 0xD1B54A32D192ED03ull));
}

// offset of pair b's matches = sum of the (non-negative) counts before it; bad = a negative count before it
__device__ __forceinline__ void pair_offset(const int* counts, int b, int tid, int nt, int* s_off, int* s_bad) {
    if (tid == 0) { *s_off = 0; *s_bad = 0; }
    __syncthreads();
    int part = 0, bad = 0;
    for (int k = tid; k < b; k += nt) {
        const int c = counts[k];
        bad |= c < 0;
        part += c > 0 ? c : 0;
    }
    if (part) atomicAdd(s_off, part);
    if (bad) *s_bad = 1;
    __syncthreads();
}

__global__ __launch_bounds__(256) void posereg_select_kernel(PoseRegInput in, int* __restrict__ index, int* __restrict__ status) {
    __shared__ unsigned long long s_keys[KEY_TILE];
    __shared__ int s_off, s_bad, s_badidx;
    const int b = blockIdx.x, tid = threadIdx.x, S = in.S;
    int* idx = index + size_t(b) * S;
    if (!in.counts) {   // dense input: slot s is row s
        for (int s = tid; s < S; s += 256) idx[s] = s;
        if (tid == 0) status[b] = 0;
        return;
    }
    if (tid == 0) s_badidx = 0;
    pair_offset(in.counts, b, tid, 256, &s_off, &s_bad);
    const long long off = s_off;
    const int N = in.counts[b];
    if (N < 0 || s_bad || off + N > in.M) {
        for (int s = tid; s < S; s += 256) idx[s] = -1;
        if (tid == 0) status[b] = -1;
        return;
    }
    if (N <= S) {       // collate_fn: not sampled (N == S included), zero-padded
        for (int s = tid; s < S; s += 256) idx[s] = s < N ? s : -1;
        if (tid == 0) status[b] = 0;
        return;
    }
    if (in.sample_index) {
        int bad = 0;
        for (int s = tid; s < S; s += 256) {
            const int v = in.sample_index[size_t(b) * S + s];
            const bool ok = v >= 0 && v < N;
            bad |= !ok;
            idx[s] = ok ? v : -1;
        }
        if (bad) s_badidx = 1;
        __syncthreads();
        if (tid == 0) status[b] = s_badidx ? -2 : 0;
        return;
    }
    const unsigned long long seed = in.seeds ? in.seeds[b] : 0ull;
    for (int base = 0; base < N; base += 256) {
        const int i = base + tid;
        const bool live = i < N;
        const unsigned long long ki = sample_key(seed, i);
        int rank = 0;
        for (int jb = 0; jb < N; jb += KEY_TILE) {
            __syncthreads();
            const int m = min(KEY_TILE, N - jb);
            for (int j = tid; j < m; j += 256) s_keys[j] = sample_key(seed, jb + j);
            __syncthreads();
            if (live)
                for (int j = 0; j < m; ++j) {
                    const unsigned long long kj = s_keys[j];
                    rank += (kj < ki || (kj == ki && jb + j < i)) ? 1 : 0;
                }
        }
        if (live && rank < S) idx[rank] = i;
    }
    if (tid == 0) status[b] = 0;
}

__global__ __launch_bounds__(256) void posereg_embed_kernel(PoseRegInput in, const int* __restrict__ index, const int* __restrict__ status,
                                                            float* __restrict__ X) {
    __shared__ int s_off, s_bad;
    const int b = blockIdx.y, tid = threadIdx.x, S = in.S;
    if (in.counts) pair_offset(in.counts, b, tid, 256, &s_off, &s_bad);
    const int e = blockIdx.x * 256 + tid;
    if (e >= 4 * S) return;
    const int s = e >> 2, c = e & 3;
    float v = 0.f;
    if (!in.counts) {
        v = (c < 2 ? in.dense0 : in.dense1)[(size_t(b) * S + s) * 2 + (c & 1)];
    } else {
        const int i = index[size_t(b) * S + s];
        if (status[b] == 0 && i >= 0) v = (c < 2 ? in.kpts0 : in.kpts1)[(size_t(s_off) + i) * 2 + (c & 1)];
    }
    float* row = X + (size_t(b) * S + s) * D;
    row[c] = v;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float f = 1.0f + 31.875f * float(k);
        const float p = __fmul_rn(f, v);     // the fp32 product is the argument (parity-critical), never contracted
        row[4 + 8 * k + c] = sinf(p);
        row[8 + 8 * k + c] = cosf(p);
    }
}

// ---- encoder layer ----------------------------------------------------------------------------------------------------------

// X: [B, S, 76]; attention groups of G consecutive pairs; slot universe u in [0, NU), NU = (B / G) * S: u = q * S + s, member g
// of it is pair q * G + g.  A workgroup takes T slots = T * G <= 32 * RB rows, row r = t * G + g.
template <int RB>
__global__ __launch_bounds__(256) void posereg_layer_kernel(pope_pose_regressor_layer w, float* __restrict__ X, int NU, int S, int G, int T) {
    constexpr int RT = 32 * RB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                // [RT][XP] layer input, then LayerNorm1 output, then the layer's output
    float* ys = xs + RT * XP;        // [RT][XP] pre-LayerNorm sums
    float* qkv = ys + RT * XP;       // [RT][QP]; after the attention: [2][96][RT] partial FFN sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
    const int u0 = blockIdx.x * T;
    const int nrows = min(T, NU - u0) * G;
    auto row_ptr = [&](int r) {
        const int t = r / G, g = r - t * G, u = u0 + t, q = u / S, s = u - q * S;
        return X + (size_t(q) * G + g) * S * D + size_t(s) * D;
    };
    for (int i = tid; i < RT * D; i += 256) {
        const int r = i / D, c = i - r * D;
        xs[r * XP + c] = r < nrows ? row_ptr(r)[c] : 0.f;     // rows past the tile are masked, not read
    }
    __syncthreads();

    float xb[RB][HD];
    load_rows<RB>(xs, XP, 0, xb);
    {   // q | k | v = in_proj; a group of one needs v alone
        const int nb0 = G == 1 ? 2 * D : 0, nblocks = G == 1 ? 3 : 8;
        for (int blk = wave; blk < nblocks; blk += 4) {
            const int n = nb0 + blk * 32 + l32;
            f32x2 wv[19];
            load_wrow(n < NQKV ? w.in_proj_w + size_t(n) * D + h * HD : nullptr, wv);
            f32x16 acc[RB] = {};
            mm76<RB>(wv, xb, acc);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int nn = nb0 + blk * 32 + mfma32_row(v, h);
                if (nn < NQKV) {
                    const float bias = w.in_proj_b[nn];
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) qkv[(rb * 32 + l32) * QP + nn] = acc[rb][v] + bias;
                }
            }
        }
    }
    __syncthreads();
    if (G > 1) {    // softmax(q k^T / sqrt(38)) v over the G members of the row's slot, per head; the result replaces the row's own q
        const float scale = 1.0f / sqrtf(float(HD));
        for (int item = tid; item < nrows * 2; item += 256) {
            const int r = item >> 1, hd = item & 1, t = r / G;
            float* q = qkv + r * QP + hd * HD;
            float qr[HD], o[HD];
#pragma unroll
            for (int d = 0; d < HD; ++d) { qr[d] = q[d]; o[d] = 0.f; }
            float m = -INFINITY;
            for (int g = 0; g < G; ++g) {
                const float* k = qkv + (t * G + g) * QP + D + hd * HD;
                float dot = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) dot = fmaf(qr[d], k[d], dot);
                m = fmaxf(m, dot * scale);
            }
            float sum = 0.f;
            for (int g = 0; g < G; ++g) {
                const float* k = qkv + (t * G + g) * QP + D + hd * HD;
                float dot = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) dot = fmaf(qr[d], k[d], dot);
                const float e = expf(dot * scale - m);
                sum += e;
                const float* vv = k + D;
#pragma unroll
                for (int d = 0; d < HD; ++d) o[d] = fmaf(e, vv[d], o[d]);
            }
            const float inv = 1.0f / sum;
#pragma unroll
            for (int d = 0; d < HD; ++d) q[d] = o[d] * inv;
        }
        __syncthreads();
    }
    load_rows<RB>(qkv, QP, G == 1 ? 2 * D : 0, xb);
    if (wave < 3) {   // out_proj + residual
        const int n = wave * 32 + l32;
        f32x2 wv[19];
        load_wrow(n < D ? w.out_proj_w + size_t(n) * D + h * HD : nullptr, wv);
        f32x16 acc[RB] = {};
        mm76<RB>(wv, xb, acc);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int nn = wave * 32 + mfma32_row(v, h);
            if (nn < D) {
                const float bias = w.out_proj_b[nn];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    const int row = rb * 32 + l32;
                    ys[row * XP + nn] = xs[row * XP + nn] + (acc[rb][v] + bias);
                }
            }
        }
    }
    __syncthreads();
    if (tid < RT) layernorm_row(ys + tid * XP, xs + tid * XP, w.norm1_w, w.norm1_b);
    __syncthreads();

    ffn76_tile<RB>(w.linear1_w, w.linear1_b, w.linear2_w, w.linear2_b, xs, ys, qkv);
    if (tid < RT) layernorm_row(ys + tid * XP, xs + tid * XP, w.norm2_w, w.norm2_b);
    __syncthreads();
    for (int i = tid; i < nrows * D; i += 256) {
        const int r = i / D, c = i - r * D;
        row_ptr(r)[c] = xs[r * XP + c];
    }
}

// ---- streamed Linear + LeakyReLU ------------------------------------------------------------------------------------------

__device__ __forceinline__ float leaky(float v) { return v >= 0.f ? v : 0.01f * v; }

// a wave owns RW consecutive output rows; NB pairs (rows of A) per weight read; V = 4: 16-byte loads (K % 4 == 0), V = 1: any K
constexpr int RW = 4;
template <int V, int NB>
__global__ __launch_bounds__(256) void posereg_stream_linear_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                                    const float* __restrict__ bias, float* __restrict__ Y,
                                                                    long long K, int N) {
    typedef typename std::conditional<V == 4, f32x4, float>::type vec;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n0 = (long long)(blockIdx.x * 4 + wave) * RW;
    if (n0 >= N) return;
    const vec* w[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) w[r] = reinterpret_cast<const vec*>(W + (n0 + r < N ? n0 + r : n0) * K);   // rows past N: row n0 again, dropped
    float acc[RW][NB];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
    const int steps = int(K / V);
#pragma unroll 2
    for (int i = lane; i < steps; i += 64) {
        vec a[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) a[r] = __builtin_nontemporal_load(w[r] + i);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const vec x = *(reinterpret_cast<const vec*>(A + b * K) + i);
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                if constexpr (V == 4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[r][b] = fmaf(a[r][e], x[e], acc[r][b]);
                } else {
                    acc[r][b] = fmaf(a[r], x, acc[r][b]);
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const float sum = wave_sum(acc[r][b]);
            if (lane == 0 && n0 + r < N) Y[(long long)b * N + n0 + r] = leaky(sum + bias[n0 + r]);
        }
}

template <int V, int NB>
int launch_stream(const float* A, const float* W, const float* bias, float* Y, long long K, int N, int chunks, hipStream_t stream) {
    // blockIdx.y = chunk: A and Y advance by NB rows per chunk
    for (int c = 0; c < chunks; ++c) {
        hipLaunchKernelGGL((posereg_stream_linear_kernel<V, NB>), dim3((N + 4 * RW - 1) / (4 * RW)), dim3(256), 0, stream, A + (long long)c * NB * K, W, bias,
                           Y + (long long)c * NB * N, K, N);
        POPE_TRY(pope_check_launch());
    }
    return POPE_OK;
}

template <int V>
int launch_stream_rem(int nb, const float* A, const float* W, const float* bias, float* Y, long long K, int N, hipStream_t stream) {
    switch (nb) {
        case 1: return launch_stream<V, 1>(A, W, bias, Y, K, N, 1, stream);
        case 2: return launch_stream<V, 2>(A, W, bias, Y, K, N, 1, stream);
        case 3: return launch_stream<V, 3>(A, W, bias, Y, K, N, 1, stream);
        case 4: return launch_stream<V, 4>(A, W, bias, Y, K, N, 1, stream);
        case 5: return launch_stream<V, 5>(A, W, bias, Y, K, N, 1, stream);
        case 6: return launch_stream<V, 6>(A, W, bias, Y, K, N, 1, stream);
        case 7: return launch_stream<V, 7>(A, W, bias, Y, K, N, 1, stream);
    }
    return POPE_OK;
}

// ---- tail -----------------------------------------------------------------------------------------------------------------

// out[n] = act(in . W[n, :] + bias[n]) for n < N by the four waves of the workgroup (lane-strided partial sums, xor butterfly)
__device__ __forceinline__ void dense_layer(const float* in, int K, const float* __restrict__ W, const float* __restrict__ bias, int N,
                                            float* out, bool act) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int TN = 8;     // outputs in flight per wave: their loads and butterflies overlap (one at a time is a latency chain)
    for (int n0 = wave * TN; n0 < N; n0 += 4 * TN) {
        float part[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) part[j] = 0.f;
        for (int k = lane; k < K; k += 64) {
            const float x = in[k];
#pragma unroll
            for (int j = 0; j < TN; ++j) part[j] = fmaf(W[size_t(min(n0 + j, N - 1)) * K + k], x, part[j]);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float s = wave_sum(part[j]);
            if (lane == 0 && n0 + j < N) out[n0 + j] = act ? leaky(s + bias[n0 + j]) : s + bias[n0 + j];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void posereg_tail_kernel(pope_pose_regressor_weights w, const float* __restrict__ Y2,
                                                           const int* __restrict__ status, float* __restrict__ trans, float* __restrict__ rot) {
    __shared__ float a[256], c[128], head[12];
    const int b = blockIdx.x, tid = threadIdx.x, S = w.num_sample;
    float* t_out = trans + 3 * b;
    float* r_out = rot + 9 * b;
    if (status[b] != 0) {
        if (tid < 3) t_out[tid] = 0.f;
        if (tid < 9) r_out[tid] = 0.f;
        return;
    }
    dense_layer(Y2 + size_t(b) * S, S, w.mlp_w[2], w.mlp_b[2], 256, a, true);
    dense_layer(a, 256, w.mlp_w[3], w.mlp_b[3], 128, c, true);
    dense_layer(c, 128, w.mlp_w[4], w.mlp_b[4], 64, a, true);
    dense_layer(a, 64, w.mlp_w[5], w.mlp_b[5], 32, c, true);
    dense_layer(c, 32, w.mlp_w[6], w.mlp_b[6], 32, a, true);
    const int rdim = w.mode == POPE_ROT_MATRIX ? 9 : w.mode == POPE_ROT_QUAT ? 4 : 6;
    dense_layer(a, 32, w.trans_w, w.trans_b, 3, head, false);
    dense_layer(a, 32, w.rot_w, w.rot_b, rdim, head + 3, false);
    if (tid != 0) return;
    for (int i = 0; i < 3; ++i) t_out[i] = head[i];
    pope_rot_to_matrix(w.mode, head + 3, r_out);
}

}  // namespace

int pope_posereg_input_check(const PoseRegInput& in) {
    if (in.B <= 0 || in.S <= 0 || in.M < 0) return POPE_ERR_ARG;
    const bool dense = in.dense0 && in.dense1, compact = in.counts != nullptr;
    if (dense == compact) return POPE_ERR_ARG;
    if (dense && (in.kpts0 || in.kpts1 || in.sample_index)) return POPE_ERR_ARG;
    if (compact && (in.dense0 || in.dense1 || ((!in.kpts0 || !in.kpts1) && in.M > 0))) return POPE_ERR_ARG;
    if (size_t(in.B) * in.S * D >= (size_t(1) << 31)) return POPE_ERR_ARG;
    return POPE_OK;
}

int pope_launch_posereg_embed(const PoseRegInput& in, float* X, int* index, int* status, hipStream_t stream) {
    POPE_TRY(pope_posereg_input_check(in));
    if (!X || !index || !status) return POPE_ERR_ARG;
    hipLaunchKernelGGL(posereg_select_kernel, dim3(in.B), dim3(256), 0, stream, in, index, status);
    POPE_TRY(pope_check_launch());
    hipLaunchKernelGGL(posereg_embed_kernel, dim3((4 * in.S + 255) / 256, in.B), dim3(256), 0, stream, in, index, status, X);
    return pope_check_launch();
}

int pope_launch_posereg_layer(const pope_pose_regressor_layer& w, float* X, int B, int S, int G, hipStream_t stream) {
    if (!X || B <= 0 || S <= 0 || G < 1 || G > 64 || B % G) return POPE_ERR_ARG;
    const int NU = (B / G) * S;
    if (G > 32) {
        const size_t lds = size_t(2 * 64 * XP + 64 * QP) * sizeof(float);
        return pope_launch_lds<posereg_layer_kernel<2>>(dim3(NU), dim3(256), lds, stream, w, X, NU, S, G, 1);
    }
    const int T = 32 / G;
    const size_t lds = size_t(2 * 32 * XP + 32 * QP) * sizeof(float);
    return pope_launch_lds<posereg_layer_kernel<1>>(dim3((NU + T - 1) / T), dim3(256), lds, stream, w, X, NU, S, G, T);
}

int pope_launch_posereg_stream_linear(const float* A, const float* W, const float* bias, float* Y, int B, long long K, int N,
                                      hipStream_t stream) {
    if (!A || !W || !bias || !Y || B <= 0 || K <= 0 || N <= 0) return POPE_ERR_ARG;
    const bool vec = (K & 3) == 0 && !((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15);
    const int full = B / CH, rem = B - full * CH;
    if (vec) {
        if (full) POPE_TRY((launch_stream<4, CH>(A, W, bias, Y, K, N, full, stream)));
        return launch_stream_rem<4>(rem, A + (long long)full * CH * K, W, bias, Y + (long long)full * CH * N, K, N, stream);
    }
    if (full) POPE_TRY((launch_stream<1, CH>(A, W, bias, Y, K, N, full, stream)));
    return launch_stream_rem<1>(rem, A + (long long)full * CH * K, W, bias, Y + (long long)full * CH * N, K, N, stream);
}

int pope_launch_posereg_tail(const pope_pose_regressor_weights& w, const float* Y2, const int* status, int B, float* trans, float* rot,
                             hipStream_t stream) {
    if (!Y2 || !status || !trans || !rot || B <= 0) return POPE_ERR_ARG;
    hipLaunchKernelGGL(posereg_tail_kernel, dim3(B), dim3(256), 0, stream, w, Y2, status, trans, rot);
    return pope_check_launch();
}
