// Device-side glue of the batched driver step (pope_amd/driver.py:locate_match_pose_batch_u8): the proposal vote of Q queries
// in one launch, and the per-slot tally of the 3Q-pair Matcher call that hands each query's best slot to the pose solver.
// What the single-query step does on the host between two downloads (eval_linemod_json.py:93-101, :118-125, :150) stays
// on the card.  Integer arithmetic everywhere an order could show; no float atomics.
#include "common.h"
#include "kernels.h"

namespace {

// The vote of one query, run by one workgroup: reference row `ref` against proposal rows begin .. begin + count of cls_prop,
// scores to out[0 .. count) in proposal order, the three slots to entry q of the slot arrays.
// Scores: the arithmetic of cls_cosine_kernel (capi.hip) — one wave per proposal, lane-strided accumulation, wave_sum, each
// norm clamped by eps separately — so out[] is bit-equal to pope_cls_cosine_f32 over those rows.
// Vote: pope_streaming_top3_host's loop, run by one lane over the query's scores in proposal order (it is order-dependent
// by definition: a score enters only if strictly greater than some slot and replaces the FIRST minimum).
__device__ __forceinline__ void vote_top3_body(const float* __restrict__ ref, const float* __restrict__ cls_prop, int begin, int count,
                                               int D, float eps, float* out, int q, float* __restrict__ slot_scores,
                                               long long* __restrict__ slot_index, int* __restrict__ pair_row,
                                               unsigned char* __restrict__ pair_live) {
    const int lane = threadIdx.x & 63;
    for (int p = threadIdx.x >> 6; p < count; p += 4) {
        const float* f = cls_prop + size_t(begin + p) * D;
        float dot = 0.f, nr = 0.f, nf = 0.f;
        for (int i = lane; i < D; i += 64) {
            const float a = ref[i], b = f[i];
            dot += a * b;
            nr += a * a;
            nf += b * b;
        }
        dot = wave_sum(dot);
        nr = wave_sum(nr);
        nf = wave_sum(nf);
        if (lane == 0) out[p] = dot / (fmaxf(sqrtf(nr), eps) * fmaxf(sqrtf(nf), eps));
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    float s3[3] = {0.f, 0.f, 0.f};
    int i3[3] = {-1, -1, -1};
    for (int p = 0; p < count; ++p) {
        const float s = out[p];
        if (s > s3[0] || s > s3[1] || s > s3[2]) {
            int k = 0;  // np.argmin: first minimum
            if (s3[1] < s3[k]) k = 1;
            if (s3[2] < s3[k]) k = 2;
            s3[k] = s;
            i3[k] = p;
        }
    }
    for (int k = 0; k < 3; ++k) {
        slot_scores[3 * q + k] = s3[k];
        slot_index[3 * q + k] = i3[k];
        pair_row[3 * q + k] = i3[k] >= 0 ? begin + i3[k] : 0;
        pair_live[3 * q + k] = i3[k] >= 0;
    }
}

// One workgroup per query; query q owns segment q and its scores lie at the segment's own rows.
__global__ __launch_bounds__(256) void vote_top3_batch_kernel(const float* __restrict__ cls_ref, const float* __restrict__ cls_prop,
                                                               const int* __restrict__ seg, int N, int D, float eps,
                                                               float* scores, float* __restrict__ slot_scores,
                                                               long long* __restrict__ slot_index, int* __restrict__ pair_row,
                                                               unsigned char* __restrict__ pair_live) {
    const int q = blockIdx.x;
    const int begin = min(max(seg[q], 0), N);
    const int end = min(max(seg[q + 1], begin), N);
    vote_top3_body(cls_ref + size_t(q) * D, cls_prop, begin, end - begin, D, eps, scores + begin, q, slot_scores, slot_index,
                   pair_row, pair_live);
}

// One workgroup per query; query q votes over segment query_seg[q] of the shared proposals, read in place (two queries may
// name one segment), and its scores go to scores[score_begin[q] ..): as many as that range holds, the vote sees no more.
__global__ __launch_bounds__(256) void vote_top3_shared_kernel(const float* __restrict__ cls_ref, const float* __restrict__ cls_prop,
                                                                const int* __restrict__ seg, int S, const int* __restrict__ query_seg,
                                                                const int* __restrict__ score_begin, int N, int D, float eps,
                                                                float* scores, float* __restrict__ slot_scores,
                                                                long long* __restrict__ slot_index, int* __restrict__ pair_row,
                                                                unsigned char* __restrict__ pair_live) {
    const int q = blockIdx.x;
    const int s = query_seg[q];
    int begin = 0, count = 0;
    if (s >= 0 && s < S) {
        begin = min(max(seg[s], 0), N);
        count = min(max(seg[s + 1], begin), N) - begin;
    }
    const int first = score_begin[q];
    count = first < 0 ? 0 : min(count, max(score_begin[q + 1] - first, 0));
    vote_top3_body(cls_ref + size_t(q) * D, cls_prop, begin, count, D, eps, scores + max(first, 0), q, slot_scores, slot_index,
                   pair_row, pair_live);
}

// Matches a slot hands on: a dead slot's are dropped whatever the Matcher found in its all-zero image.
__device__ __forceinline__ int slot_count(const int* pair_count, const unsigned char* pair_live, int b) {
    return pair_live[b] ? pair_count[b] : 0;
}

// np.argmax of a query's three matching scores (first maximum)
__device__ __forceinline__ int first_argmax3(const long long* s) {
    int k = 0;
    if (s[1] > s[k]) k = 1;
    if (s[2] > s[k]) k = 2;
    return k;
}

__device__ __forceinline__ int block_sum_int(int v, int* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    v = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return v;
}

// One workgroup per pair: its rows in the pair-contiguous match list by binary search on m_bids (an empty pair gets
// begin = where it would lie, count 0), then #(mconf > conf_thr) over those rows — fp32, strict.
__global__ __launch_bounds__(256) void slot_bounds_kernel(const long long* __restrict__ m_bids, const float* __restrict__ mconf,
                                                           const unsigned char* __restrict__ pair_live, long long M, float conf_thr,
                                                           int* __restrict__ pair_begin, int* __restrict__ pair_count,
                                                           long long* __restrict__ matching_score) {
    __shared__ int lds[4];
    const int b = blockIdx.x;
    long long lo = 0, hi = M;          // first row with m_bids >= b
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (m_bids[mid] < b) lo = mid + 1; else hi = mid;
    }
    const long long first = lo;
    hi = M;                            // first row with m_bids > b
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (m_bids[mid] <= b) lo = mid + 1; else hi = mid;
    }
    const int count = int(lo - first);
    int above = 0;
    if (pair_live[b])
        for (int i = threadIdx.x; i < count; i += 256) above += mconf[first + i] > conf_thr ? 1 : 0;
    above = block_sum_int(above, lds);
    if (threadIdx.x == 0) {
        pair_begin[b] = int(first);
        pair_count[b] = count;
        matching_score[b] = above;
    }
}

// One workgroup per query: best slot, its match count, the exclusive scan of the best counts of the queries before it (an
// integer sum, recomputed per workgroup from the per-pair results) and the in-order copy of the best slot's matches there.
__global__ __launch_bounds__(256) void slot_compact_kernel(const float2* __restrict__ mk0, const float2* __restrict__ mk1,
                                                            const unsigned char* __restrict__ pair_live,
                                                            const int* __restrict__ pair_begin, const int* __restrict__ pair_count,
                                                            const long long* __restrict__ matching_score, long long M,
                                                            int* __restrict__ best_slot, int* __restrict__ best_count,
                                                            float2* __restrict__ best0, float2* __restrict__ best1) {
    __shared__ int lds[4];
    const int q = blockIdx.x;
    int before = 0;
    for (int j = threadIdx.x; j < q; j += 256)
        before += slot_count(pair_count, pair_live, 3 * j + first_argmax3(matching_score + 3 * j));
    const long long off = block_sum_int(before, lds);
    const int s = first_argmax3(matching_score + 3 * q);
    const int n = slot_count(pair_count, pair_live, 3 * q + s);
    const long long src = pair_begin[3 * q + s];
    if (threadIdx.x == 0) {
        best_slot[q] = s;
        best_count[q] = n;
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        if (off + i >= M || src + i >= M) break;   // only an unsorted m_bids can get here
        best0[off + i] = mk0[src + i];
        best1[off + i] = mk1[src + i];
    }
}

}  // namespace

int pope_launch_vote_top3_batch(const float* cls_ref, const float* cls_prop, const int* seg, int Q, int N, int D, float eps,
                                float* scores, float* slot_scores, long long* slot_index, int* pair_row, unsigned char* pair_live,
                                hipStream_t stream) {
    if (Q < 0 || N < 0 || D <= 0) return POPE_ERR_ARG;
    if (Q == 0) return POPE_OK;
    if (!cls_ref || !seg || !slot_scores || !slot_index || !pair_row || !pair_live || (N > 0 && (!cls_prop || !scores)))
        return POPE_ERR_ARG;
    hipLaunchKernelGGL(vote_top3_batch_kernel, dim3(Q), dim3(256), 0, stream, cls_ref, cls_prop, seg, N, D, eps, scores,
                       slot_scores, slot_index, pair_row, pair_live);
    return pope_check_launch();
}

int pope_launch_vote_top3_shared(const float* cls_ref, const float* cls_prop, const int* seg, int S, const int* query_seg,
                                 const int* score_begin, int Q, int N, int D, float eps, float* scores, float* slot_scores,
                                 long long* slot_index, int* pair_row, unsigned char* pair_live, hipStream_t stream) {
    if (Q < 0 || N < 0 || S < 0 || D <= 0) return POPE_ERR_ARG;
    if (Q == 0) return POPE_OK;
    if (!cls_ref || !seg || !query_seg || !score_begin || !slot_scores || !slot_index || !pair_row || !pair_live ||
        (N > 0 && (!cls_prop || !scores)))
        return POPE_ERR_ARG;
    hipLaunchKernelGGL(vote_top3_shared_kernel, dim3(Q), dim3(256), 0, stream, cls_ref, cls_prop, seg, S, query_seg, score_begin, N,
                       D, eps, scores, slot_scores, slot_index, pair_row, pair_live);
    return pope_check_launch();
}

int pope_launch_slot_tally(const long long* m_bids, const float* mconf, const float* mkpts0, const float* mkpts1,
                           const unsigned char* pair_live, int Q, long long M, float conf_thr, int* pair_begin, int* pair_count,
                           long long* matching_score, int* best_slot, int* best_count, float* best_kpts0, float* best_kpts1,
                           hipStream_t stream) {
    if (Q < 0 || M < 0 || M > 0x7fffffffLL || Q > 0x7fffffff / 3) return POPE_ERR_ARG;
    if (Q == 0 || M == 0) return POPE_OK;
    if (!m_bids || !mconf || !mkpts0 || !mkpts1 || !pair_live || !pair_begin || !pair_count || !matching_score || !best_slot ||
        !best_count || !best_kpts0 || !best_kpts1)
        return POPE_ERR_ARG;
    hipLaunchKernelGGL(slot_bounds_kernel, dim3(3 * Q), dim3(256), 0, stream, m_bids, mconf, pair_live, M, conf_thr, pair_begin,
                       pair_count, matching_score);
    if (int rc = pope_check_launch()) return rc;
    hipLaunchKernelGGL(slot_compact_kernel, dim3(Q), dim3(256), 0, stream, reinterpret_cast<const float2*>(mkpts0),
                       reinterpret_cast<const float2*>(mkpts1), pair_live, pair_begin, pair_count, matching_score, M, best_slot,
                       best_count, reinterpret_cast<float2*>(best_kpts0), reinterpret_cast<float2*>(best_kpts1));
    return pope_check_launch();
}
