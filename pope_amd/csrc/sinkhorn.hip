// Sinkhorn coarse matching (match_type='sinkhorn'): log-domain optimal transport with a dustbin row and column.
//
// Semantics follow the reference CoarseMatching (src/matcher/utils/coarse_matching.py:121-143) around the published SuperGlue
// recursion (the reference imports it from a file it does not ship; pope_amd/sinkhorn_cpu.py states it):
//   Z [L+1, S+1]: the L x S block is sim (no temperature, -1e9 fill), the last row, column and corner are alpha = bin_score
//   norm = -log(L + S);  log_mu = [norm] * L + [log(S) + norm];  log_nu = [norm] * S + [log(L) + norm]
//   u = v = 0; skh_iters times:  u_i = log_mu_i - logsumexp_j(Z_ij + v_j);  v_j = log_nu_j - logsumexp_i(Z_ij + u_i)
//   conf = exp(Z + u + v - norm)[:L, :S]
//   skh_prefilter: conf rows whose argmax over the S + 1 columns is the dustbin are zeroed, and columns likewise (:136-140)
//
// The dustbin row, column and corner are never stored: a pass adds alpha + (a vector entry) where the index runs past the
// block.  alpha is read from the parameter's storage by every kernel: no host copy exists.
//
// Passes over the L x S matrix, skh_iters = 3: iteration 1's row step costs none (with v = 0 it is the row softmax statistics
// the contraction left behind), then column, (row, column) x 2, and the confidence pass, which sweeps a row twice (the row
// prefilter needs the whole row before any of its confidences is final; the second sweep hits the cache) and writes it once.
#include "common.h"
#include "kernels.h"

namespace {

constexpr float L2E = 1.44269504088896340736f;
constexpr float LN2 = 0.69314718055994530942f;

// (m, s): max and sum of exp(. - m) of the values seen so far.  The empty state is (-inf, 0).
struct Lse {
    float m, s;
    __device__ __forceinline__ void add(float t) {   // t finite
        const float mn = fmaxf(m, t);
        s = s * __builtin_amdgcn_exp2f((m - mn) * L2E) + __builtin_amdgcn_exp2f((t - mn) * L2E);
        m = mn;
    }
    __device__ __forceinline__ void merge(float om, float os) {   // either side may be empty
        const float mn = fmaxf(m, om);
        const float a = m == mn ? 1.f : __builtin_amdgcn_exp2f((m - mn) * L2E);
        const float b = om == mn ? 1.f : __builtin_amdgcn_exp2f((om - mn) * L2E);
        s = s * a + os * b;
        m = mn;
    }
    __device__ __forceinline__ float value() const { return m + __builtin_amdgcn_logf(s) * LN2; }   // v_log_f32 is log2
};

// Iteration 1, row step: v = 0, so logsumexp_j(Z_ij) over the real columns is row_max + log(row_sum) of the contraction's
// statistics; the dustbin column adds alpha.  The dustbin row is S + 1 times alpha.
__global__ __launch_bounds__(256) void skh_first_rows_kernel(const MatchParams p) {
    const int row = blockIdx.x * 256 + threadIdx.x, pair = blockIdx.y;
    if (row > p.L) return;
    const float alpha = *p.bin_score;
    float* u = p.skh_u + size_t(pair) * (p.L + 1);
    if (row == p.L) {
        u[row] = p.skh_log_mu_bin - (alpha + __builtin_amdgcn_logf(float(p.S + 1)) * LN2);
        return;
    }
    Lse a{p.row_max[size_t(pair) * p.L + row], p.row_sum[size_t(pair) * p.L + row]};
    a.merge(alpha, 1.f);
    u[row] = p.skh_norm - a.value();
}

// Row step: one wave per row of the (L + 1) x (S + 1) problem; row L is the dustbin row (alpha everywhere).
__global__ __launch_bounds__(256) void skh_rows_kernel(const MatchParams p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), pair = blockIdx.y;
    if (row > p.L) return;
    const float alpha = *p.bin_score;
    const float* v = p.skh_v + size_t(pair) * (p.S + 1);
    const bool real = row < p.L;
    const float* x = p.sim + (size_t(pair) * p.L + (real ? row : 0)) * p.S;
    Lse a{-INFINITY, 0.f};
    for (int s = lane; s <= p.S; s += 64) a.add((real && s < p.S ? x[s] : alpha) + v[s]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a.merge(__shfl_xor(a.m, o), __shfl_xor(a.s, o));
    if (lane == 0) p.skh_u[size_t(pair) * (p.L + 1) + row] = (real ? p.skh_norm : p.skh_log_mu_bin) - a.value();
}

// Column step: 64 columns per block, 16 waves stride over the real rows and meet in LDS in a fixed order; the dustbin row
// joins last.  Column S is the dustbin column.  LAST: keep the maximum over the real rows of Z_ij + u_i (the column prefilter).
constexpr int SC_WAVES = 16;
template <bool LAST>
__global__ __launch_bounds__(64 * SC_WAVES) void skh_cols_kernel(const MatchParams p) {
    __shared__ float red_m[SC_WAVES][64], red_s[SC_WAVES][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c, pair = blockIdx.y;
    const bool ok = col <= p.S, real = col < p.S;
    const float alpha = *p.bin_score;
    const float* u = p.skh_u + size_t(pair) * (p.L + 1);
    const float* x = p.sim + size_t(pair) * p.L * p.S + (real ? col : 0);
    Lse a{-INFINITY, 0.f};
    if (ok)
        for (int l = g; l < p.L; l += SC_WAVES) a.add((real ? x[size_t(l) * p.S] : alpha) + u[l]);
    red_m[g][c] = a.m;
    red_s[g][c] = a.s;
    __syncthreads();
    if (g || !ok) return;
    for (int w = 1; w < SC_WAVES; ++w) a.merge(red_m[w][c], red_s[w][c]);
    if (LAST && real) p.skh_cmax[size_t(pair) * p.S + col] = a.m;
    a.merge(alpha + u[p.L], 1.f);
    p.skh_v[size_t(pair) * (p.S + 1) + col] = (real ? p.skh_norm : p.skh_log_nu_bin) - a.value();
}

// conf(i, j) = exp(Z_ij + u_i + v_j - norm), in the reference's order of operations
__device__ __forceinline__ float skh_conf(float z, float u, float v, float norm) {
    return __builtin_amdgcn_exp2f((((z + u) + v) - norm) * L2E);
}

constexpr int CP_ROWS = 32;   // rows per workgroup, 8 per wave: the row blocks of colmax_part (pope_match_nrb2)
constexpr int SK_K = 16;      // columns per lane and chunk: a chunk is 1024 columns

// Workgroup = 32 rows of one pair x all columns, as conf_pass_kernel of match.hip: lane l owns columns c0 + 64 k + l and keeps
// their v, prefilter verdict and running maximum in registers while its wave walks 8 rows.  Before that, each wave sweeps its
// rows once for max_j(Z_ij + v_j): row i is filtered iff alpha + v_S is strictly greater (u_i cancels; a tie goes to the real
// cell, as torch.max returns the first maximum).  Column j is filtered iff alpha + u_L > skh_cmax[j].
__global__ __launch_bounds__(256) void skh_conf_kernel(const MatchParams p) {
    __shared__ float cmax_s[4][64 * SK_K];
    constexpr int RPW = CP_ROWS / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.y, blk = blockIdx.x;
    const int row0 = blk * CP_ROWS + wave * RPW;
    const size_t prow = size_t(pair) * p.L;
    const float alpha = *p.bin_score;
    const float* ug = p.skh_u + size_t(pair) * (p.L + 1);
    const float* vg = p.skh_v + size_t(pair) * (p.S + 1);
    const float* cmg = p.skh_cmax + size_t(pair) * p.S;
    const float row_bin = alpha + vg[p.S], col_bin = alpha + ug[p.L];
    const bool pre = p.skh_prefilter != 0;

    bool keep[RPW];
    RowBest best[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        best[r] = RowBest{-1.f, 0, 0};   // conf >= 0
        keep[r] = true;
        const int row = row0 + r;
        if (!pre || row >= p.L) continue;   // wave-uniform
        const float* x = p.sim + (prow + row) * p.S;
        float m = -INFINITY;
        for (int s = lane; s < p.S; s += 64) m = fmaxf(m, x[s] + vg[s]);
        keep[r] = !(row_bin > wave_max(m));
    }

    for (int c0 = 0; c0 < p.S; c0 += 64 * SK_K) {
        float v[SK_K], cbest[SK_K];
        bool ckeep[SK_K];
#pragma unroll
        for (int k = 0; k < SK_K; ++k) {
            const int col = c0 + 64 * k + lane;
            const bool ok = col < p.S;
            v[k] = ok ? vg[col] : 0.f;
            ckeep[k] = ok && !(pre && col_bin > cmg[col]);
            cbest[k] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int row = row0 + r;
            if (row >= p.L) break;   // wave-uniform
            const float u = ug[row];
            float* x = p.sim + (prow + row) * p.S;
#pragma unroll
            for (int k = 0; k < SK_K; ++k) {
                const int col = c0 + 64 * k + lane;
                if (c0 + 64 * k >= p.S) break;   // wave-uniform
                if (col < p.S) {
                    const float c = keep[r] && ckeep[k] ? skh_conf(x[col], u, v[k], p.skh_norm) : 0.f;
                    x[col] = c;
                    best[r].take(c, col);
                    cbest[k] = fmaxf(cbest[k], c);
                }
            }
        }
        // column maxima of this 32-row block: the four waves' registers meet in LDS
        if (c0) __syncthreads();
#pragma unroll
        for (int k = 0; k < SK_K; ++k) cmax_s[wave][64 * k + lane] = cbest[k];
        __syncthreads();
        float* out = p.colmax_part + (size_t(pair) * p.nrb2 + blk) * p.ldp;
        for (int c = threadIdx.x; c < 64 * SK_K && c0 + c < p.S; c += 256)
            out[c0 + c] = fmaxf(fmaxf(cmax_s[0][c], cmax_s[1][c]), fmaxf(cmax_s[2][c], cmax_s[3][c]));
    }
    // per row: reduce the lanes' candidates (first argmax = smallest column among the maxima)
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int row = row0 + r;
        if (row >= p.L) break;
        RowBest b = best[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b.merge(__shfl_xor(b.v, o), __shfl_xor(b.idx, o), __shfl_xor(b.cnt, o));
        if (lane == 0) {
            p.conf_rowmax[prow + row] = b.v;
            p.row_arg[prow + row] = b.idx;
            p.row_cnt[prow + row] = b.cnt;
        }
    }
}

}  // namespace

int pope_launch_sinkhorn_passes(const MatchParams& p, hipStream_t stream) {
    if (p.nrb2 != (p.L + CP_ROWS - 1) / CP_ROWS) return POPE_ERR_ARG;
    const dim3 rows((p.L + 1 + 3) / 4, p.n), cols((p.S + 1 + 63) / 64, p.n);
    for (int it = 0; it < p.skh_iters; ++it) {
        if (it == 0) hipLaunchKernelGGL(skh_first_rows_kernel, dim3((p.L + 1 + 255) / 256, p.n), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(skh_rows_kernel, rows, dim3(256), 0, stream, p);
        if (it == p.skh_iters - 1) hipLaunchKernelGGL(skh_cols_kernel<true>, cols, dim3(64 * SC_WAVES), 0, stream, p);
        else hipLaunchKernelGGL(skh_cols_kernel<false>, cols, dim3(64 * SC_WAVES), 0, stream, p);
    }
    hipLaunchKernelGGL(skh_conf_kernel, dim3((p.L + CP_ROWS - 1) / CP_ROWS, p.n), dim3(256), 0, stream, p);
    return pope_check_launch();
}
