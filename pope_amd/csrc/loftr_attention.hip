// Full (softmax) attention of the LoFTR encoder layer — loftr_module/linear_attention.py:50-81 without masks:
//     A = softmax(Q K^T / sqrt(D), over the S source rows) ; message = A V      per head, D = C / 8 = 32 (coarse) or 16 (fine)
// on the buffers of the layer's launch sequence (loftr.hip): q [n L, C] fp32, kv [n S, 2C] fp32 (k | v), head h = columns
// h D .. h D + D - 1.  The message leaves as fp32 rows [n L, C] or as the merge GEMM's activation planes (scale 8, range flag).
//
// Two routes, both exact fp32 arithmetic in a fixed order per output row (a row's bits depend on its position in its
// sequence and on S only: not on n, not on its neighbours):
//   S >  64: flash-style, v_mfma_f32_32x32x2_f32.  128 queries of one (sequence, head) per workgroup, 64-key K/V tiles
//            through LDS, online softmax in the log2 domain.  Orientation of attention_f32.hip: S^T = K . Q^T (lane
//            (r, h) = (lane & 31, lane >> 5) holds 16 keys of query r per 32-key sub-tile), O^T += V^T . P^T with the
//            score registers as the B operand.  Nothing proportional to L x S is ever stored.
//   S <= 64: the fine transformer's 25-token windows.  K/V of all 8 heads of one sequence in LDS, one thread per
//            (query, head), two passes over the keys in plain fp32 FMAs.
// Padding masks do not exist here: a padded query row is an all -inf softmax row, NaN in the reference (and from the second
// layer on in every row), so the callers refuse masks with full attention.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int FQB = 128;        // flash: queries per workgroup (4 waves x 32)
constexpr int FKT = 64;         // flash: keys per LDS tile
constexpr int SMALL_S = 64;     // longest source the small-sequence route takes
constexpr int SMALL_QB = 32;    // small route: queries per workgroup (x 8 heads = 256 threads)
constexpr float LOG2E = 1.44269504088896340736f;

// four consecutive message columns of one row: fp32, or split into the merge GEMM's operand planes
template <bool PLANES>
__device__ __forceinline__ void store_msg4(float* __restrict__ msg, size_t row, int C, int col, f32x4 v, pope_range_acc& acc) {
    if constexpr (PLANES) {
        const f32x4 sv = v * K_PLANES_ACT_SCALE;
        acc.add(sv);
        pope_planes_store(reinterpret_cast<_Float16*>(msg) + row * 2 * C, col, sv);
    } else {
        *reinterpret_cast<f32x4*>(msg + row * C + col) = v;
    }
}

// LDS row of D + 4 floats: an odd number of 16-byte pieces, so the ds_read_b128 of 32 consecutive rows is conflict-free
template <int D, bool PLANES>
__global__ __launch_bounds__(256) void loftr_flash_f32_kernel(const float* __restrict__ q, const float* __restrict__ kv, int L, int S,
                                                               int C, int H, float qscale, float* __restrict__ msg,
                                                               unsigned* range_flag) {
    constexpr int ST = D + 4, NJ = D / 8, PPT = D / 16;   // PPT: 16-byte pieces of a K (and a V) tile per thread
    __shared__ __attribute__((aligned(16))) float Ks[FKT * ST];
    __shared__ __attribute__((aligned(16))) float Vs[FKT * ST];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nqb = (L + FQB - 1) / FQB;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);   // the query blocks of one (sequence, head) share an XCD's L2
    const int bh = logical / nqb, head = bh % H, b = bh / H, q0 = (logical - bh * nqb) * FQB;
    const float* qb = q + size_t(b) * L * C + head * D;
    const float* kb = kv + size_t(b) * S * 2 * C + head * D;   // v: + C

    // Q^T fragments of all k-steps, pre-scaled by D^-0.5 * log2(e): scores come out of the MFMA in the log2 domain
    const int qrow = q0 + wave * 32 + r;
    f32x4 qf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qrow < L) v = *reinterpret_cast<const f32x4*>(qb + size_t(qrow) * C + 8 * j + 4 * h);
        qf[j] = v * qscale;
    }

    // K/V staging through registers: the next tile's loads are in flight under this tile's MFMAs; rows >= S read as zeros
    f32x4 rk[PPT], rv[PPT];
    auto load_kv = [&](int kt) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = tid + 256 * i, row = p / (D / 4), c4 = (p - row * (D / 4)) * 4, key = kt * FKT + row;
            f32x4 k4 = {0.f, 0.f, 0.f, 0.f}, v4 = {0.f, 0.f, 0.f, 0.f};
            if (key < S) {
                const float* src = kb + size_t(key) * 2 * C + c4;
                k4 = *reinterpret_cast<const f32x4*>(src);
                v4 = *reinterpret_cast<const f32x4*>(src + C);
            }
            rk[i] = k4;
            rv[i] = v4;
        }
    };
    auto store_kv = [&]() {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = tid + 256 * i, row = p / (D / 4), c4 = (p - row * (D / 4)) * 4;
            *reinterpret_cast<f32x4*>(&Ks[row * ST + c4]) = rk[i];
            *reinterpret_cast<f32x4*>(&Vs[row * ST + c4]) = rv[i];
        }
    };

    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;   // running max (log2 domain), this lane's share of the running sum
    // V^T is the A operand: lane r supplies row d = r.  D = 16: rows 16..31 of the 32 x 32 block are zeros
    const int vcol = r < D ? r : 0;
    const float vkeep = r < D ? 1.0f : 0.0f;

    const int nkt = (S + FKT - 1) / FKT;
    load_kv(0);
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt) __syncthreads();   // every wave is done with the previous stage
        store_kv();
        __syncthreads();
        if (kt + 1 < nkt) load_kv(kt + 1);

        f32x16 s0, s1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s0[i] = 0.f; s1[i] = 0.f; }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f32x4 k0 = *reinterpret_cast<const f32x4*>(&Ks[r * ST + 8 * j + 4 * h]);
            const f32x4 k1 = *reinterpret_cast<const f32x4*>(&Ks[(32 + r) * ST + 8 * j + 4 * h]);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                s0 = mfma_32x32x2(k0[s], qf[j][s], s0);
                s1 = mfma_32x32x2(k1[s], qf[j][s], s1);
            }
        }
        if (kt == nkt - 1) {   // the padded keys of the last tile leave the softmax
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kt * FKT + mfma32_row(i, h);
                if (key >= S) s0[i] = -INFINITY;
                if (key + 32 >= S) s1[i] = -INFINITY;
            }
        }
        float mt = __builtin_fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int i = 1; i < 16; ++i) mt = __builtin_fmaxf(mt, __builtin_fmaxf(s0[i], s1[i]));
        mt = __builtin_fmaxf(mt, __shfl_xor(mt, 32));   // key 0 of every tile is real: finite
        const float m_new = __builtin_fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: exp2(-inf) = 0
        m_run = m_new;
        float ls = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            s0[i] = __builtin_amdgcn_exp2f(s0[i] - m_new);
            s1[i] = __builtin_amdgcn_exp2f(s1[i] - m_new);
            ls += s0[i] + s1[i];
        }
        l_run = l_run * alpha + ls;
        o *= alpha;
#pragma unroll
        for (int t = 0; t < 16; ++t) o = mfma_32x32x2(Vs[mfma32_row(t, h) * ST + vcol] * vkeep, s0[t], o);
#pragma unroll
        for (int t = 0; t < 16; ++t) o = mfma_32x32x2(Vs[(32 + mfma32_row(t, h)) * ST + vcol] * vkeep, s1[t], o);
    }

    // O^T: register i of lane (r, h) is d = mfma32_row(i, h) of query r: four consecutive d per register quad
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
    pope_range_acc acc;
    if (qrow < L) {
#pragma unroll
        for (int g = 0; g < D / 8; ++g) {
            const f32x4 v = {o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv};
            store_msg4<PLANES>(msg, size_t(b) * L + qrow, C, head * D + 8 * g + 4 * h, v, acc);
        }
    }
    if constexpr (PLANES) pope_range_flag(range_flag, POPE_RANGE_QKV, acc.bad());
}

// S <= 64.  Workgroup = 32 queries x 8 heads of one sequence; LDS: the sequence's kv rows [S][2C] as they lie in memory.
// A wave holds two heads: its K / V reads are two broadcast addresses.  Pass 1: the row maximum; pass 2 recomputes each
// score with the same fma chain (same bits), so exp2(score - max) <= 1 exactly as in a stored-score softmax.
template <int D, bool PLANES>
__global__ __launch_bounds__(256) void loftr_small_attn_kernel(const float* __restrict__ q, const float* __restrict__ kv, int L, int S,
                                                                int C, float qscale, float* __restrict__ msg, unsigned* range_flag) {
    extern __shared__ __attribute__((aligned(16))) float kvs[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const f32x4* src = reinterpret_cast<const f32x4*>(kv + size_t(b) * S * 2 * C);
    for (int i = tid; i < S * 2 * C / 4; i += 256) reinterpret_cast<f32x4*>(kvs)[i] = src[i];
    __syncthreads();
    const int head = tid >> 5, l = blockIdx.y * SMALL_QB + (tid & 31);
    pope_range_acc acc;
    if (l < L) {
        const size_t row = size_t(b) * L + l;
        float qv[D];
#pragma unroll
        for (int d4 = 0; d4 < D; d4 += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(q + row * C + head * D + d4) * qscale;
            qv[d4] = v[0]; qv[d4 + 1] = v[1]; qv[d4 + 2] = v[2]; qv[d4 + 3] = v[3];
        }
        const float* kh = kvs + head * D;
        auto score = [&](int s) {
            const float* kr = kh + s * 2 * C;
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) a = __builtin_fmaf(qv[d], kr[d], a);
            return a;
        };
        float m = -INFINITY;
        for (int s = 0; s < S; ++s) m = __builtin_fmaxf(m, score(s));
        float ov[D];
#pragma unroll
        for (int d = 0; d < D; ++d) ov[d] = 0.f;
        float sum = 0.f;
        for (int s = 0; s < S; ++s) {
            const float p = __builtin_amdgcn_exp2f(score(s) - m);
            const float* vr = kh + s * 2 * C + C;
            sum += p;
#pragma unroll
            for (int d = 0; d < D; ++d) ov[d] = __builtin_fmaf(p, vr[d], ov[d]);
        }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int d4 = 0; d4 < D; d4 += 4) {
            const f32x4 v = {ov[d4] * inv, ov[d4 + 1] * inv, ov[d4 + 2] * inv, ov[d4 + 3] * inv};
            store_msg4<PLANES>(msg, row, C, head * D + d4, v, acc);
        }
    }
    if constexpr (PLANES) pope_range_flag(range_flag, POPE_RANGE_QKV, acc.bad());
}

template <int D, bool PLANES>
int launch_small(const float* q, const float* kv, int n, int L, int S, int C, float qscale, float* msg, unsigned* range_flag,
                 hipStream_t stream) {
    // opt in once for the largest stage (S = 64 of C = 256: 128 KiB of the CU's 160), launch with the sequence's own size
    static pope_dev_mask lds_ok{0};
    constexpr size_t max_bytes = size_t(SMALL_S) * 2 * 8 * D * sizeof(float);
    if (!pope_opt_in_lds(loftr_small_attn_kernel<D, PLANES>, max_bytes, lds_ok)) return POPE_ERR_LAUNCH;
    hipLaunchKernelGGL((loftr_small_attn_kernel<D, PLANES>), dim3(n, (L + SMALL_QB - 1) / SMALL_QB), dim3(256),
                       size_t(S) * 2 * C * sizeof(float), stream, q, kv, L, S, C, qscale, msg, range_flag);
    return pope_check_launch();
}

template <int D, bool PLANES>
int launch_flash(const float* q, const float* kv, int n, int L, int S, int C, int H, float qscale, float* msg, unsigned* range_flag,
                 hipStream_t stream) {
    const size_t blocks = size_t(n) * H * ((L + FQB - 1) / FQB);
    if (blocks > 0x7fffffffull) return POPE_ERR_ARG;
    hipLaunchKernelGGL((loftr_flash_f32_kernel<D, PLANES>), dim3(unsigned(blocks)), dim3(256), 0, stream, q, kv, L, S, C, H, qscale, msg,
                       range_flag);
    return pope_check_launch();
}

}  // namespace

int pope_loftr_full_attention_check(const void* q, const void* kv, int n, int L, int S, int C, int H, const void* out) {
    if (!q || !kv || !out || n <= 0 || L <= 0 || S <= 0 || (C != 256 && C != 128) || H != 8) return POPE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(q) & 15) || (reinterpret_cast<uintptr_t>(kv) & 15) || (reinterpret_cast<uintptr_t>(out) & 15))
        return POPE_ERR_ARG;
    if (S <= SMALL_S && (L + SMALL_QB - 1) / SMALL_QB > 65535) return POPE_ERR_ARG;   // the small route's grid.y
    if (size_t(n) * L > 0x7fffffffull / (2 * C) || size_t(n) * S > 0x7fffffffull / (2 * C)) return POPE_ERR_ARG;
    return POPE_OK;
}

int pope_launch_loftr_full_attention(const float* q, const float* kv, int n, int L, int S, int C, int H, bool planes, float* msg,
                                     unsigned* range_flag, hipStream_t stream) {
    POPE_TRY(pope_loftr_full_attention_check(q, kv, n, L, S, C, H, msg));
    const int D = C / H;
    const float qscale = (1.0f / sqrtf(float(D))) * LOG2E;
#define LOFTR_FULL(FN, ...) \
    (D == 32 ? (planes ? FN<32, true>(__VA_ARGS__) : FN<32, false>(__VA_ARGS__)) : (planes ? FN<16, true>(__VA_ARGS__) : FN<16, false>(__VA_ARGS__)))
    if (S <= SMALL_S) return LOFTR_FULL(launch_small, q, kv, n, L, S, C, qscale, msg, range_flag, stream);
    return LOFTR_FULL(launch_flash, q, kv, n, L, S, C, H, qscale, msg, range_flag, stream);
#undef LOFTR_FULL
}
