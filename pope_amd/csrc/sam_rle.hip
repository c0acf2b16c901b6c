// SAM automatic mask generator, run-length encoding of a batch of bit-packed masks (segment_anything/utils/amg.py:
// mask_to_rle_pytorch): the mask flattened COLUMN-major (i = x * H + y), the virtual pixel before i = 0 clear, transitions
// t_0 < t_1 < .. < t_k where a pixel differs from its predecessor (a column's first pixel from the previous column's last),
// counts = [t_0, t_1 - t_0, .., H * W - t_k], i.e. k + 2 entries, [H * W] without a transition.
//
// Masks are packed along x, runs go along y.  A wave owns 64 consecutive columns (two words of a row) and walks them in blocks
// of 64 rows: lane l loads the two words of row 64 r + l, and 64 ballots of one bit each transpose the 64 x 64 block, so lane l
// ends up with the 64 rows of column 64 wp + l in one 64-bit register.  Transitions of that segment are
// seg ^ ((seg << 1) | carry) with carry = the row above the block, or, at the top of a column, the last row of the column to
// the left (the last row shifted by one pixel).  One workgroup of 16 waves encodes one mask in strips of 1024 columns (thread =
// column): pass A counts a column's transitions and keeps its last one, an exclusive scan over the strip (sum of the counts,
// maximum of the last indices) plus the running totals of the strips before gives every column its place in the output and the
// transition it continues from, pass B walks the column again and writes t_j - t_(j-1).  No workspace, no atomics, integer
// arithmetic only: a mask's output depends neither on n nor on its place in the batch nor on any arrival order.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 1024;          // one column of a strip per thread
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSide = 1 << 14;

struct RleK {
    const unsigned* packed;   // [n, H, Wp]
    int* lengths;             // [n], lengths mode
    const long long* offsets; // [n + 1], write mode
    unsigned* counts;         // [capacity], write mode
    long long capacity;
    int n, H, W, Wp;
    unsigned last_valid;      // valid bits of the last word of a row
};

// word i of row y with the pad bits cleared; zero outside the mask
__device__ inline unsigned rle_word(const RleK& k, const unsigned* mask, int y, int i) {
    if (y < 0 || y >= k.H || i < 0 || i >= k.Wp) return 0u;
    const unsigned w = mask[size_t(y) * k.Wp + i];
    return i == k.Wp - 1 ? w & k.last_valid : w;
}

// Rows 64 r .. 64 r + 63 of column 64 wp + lane as one 64-bit word (bit p = row 64 r + p, rows past H clear) and the pixel the
// first of them follows.  Every lane of the wave takes part: the ballots are the transposition.
__device__ inline unsigned long long rle_segment(const RleK& k, const unsigned* mask, int wp, int r, int lane, unsigned& carry) {
    const int y = r * 64 + lane;
    const unsigned w0 = rle_word(k, mask, y, 2 * wp), w1 = rle_word(k, mask, y, 2 * wp + 1);
    unsigned long long seg = 0ull;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        const unsigned long long s0 = __ballot((w0 >> b) & 1u), s1 = __ballot((w1 >> b) & 1u);
        if (lane == b) seg = s0;
        if (lane == 32 + b) seg = s1;
    }
    // the row above the block; at the top of a column the last row, one pixel to the left (wave-uniform words)
    unsigned a0, a1;
    if (r > 0) {
        a0 = rle_word(k, mask, r * 64 - 1, 2 * wp);
        a1 = rle_word(k, mask, r * 64 - 1, 2 * wp + 1);
    } else {
        const unsigned l0 = rle_word(k, mask, k.H - 1, 2 * wp), l1 = rle_word(k, mask, k.H - 1, 2 * wp + 1);
        a0 = (l0 << 1) | (rle_word(k, mask, k.H - 1, 2 * wp - 1) >> 31);
        a1 = (l1 << 1) | (l0 >> 31);
    }
    carry = lane < 32 ? (a0 >> lane) & 1u : (a1 >> (lane - 32)) & 1u;
    return seg;
}

__device__ inline unsigned long long rle_transitions(unsigned long long seg, unsigned carry, int rows) {
    const unsigned long long valid = rows >= 64 ? ~0ull : (1ull << rows) - 1ull;
    return (seg ^ ((seg << 1) | carry)) & valid;
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void sam_rle_kernel(RleK k) {
    __shared__ int wave_count[kWaves], wave_last[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.x;
    const unsigned* mask = k.packed + size_t(m) * k.H * k.Wp;
    const int blocks = (k.H + 63) / 64;
    // this mask's part of the output: nothing is written outside it, whatever the offsets say
    long long begin = 0, end = 0;
    if (WRITE) {
        begin = k.offsets[m];
        end = k.offsets[m + 1];
        end = end < k.capacity ? end : k.capacity;
        if (begin < 0) end = begin;
    }
    int total = 0, last_all = 0;     // transitions and the last transition of the strips before (0: the virtual start)
    for (int x0 = 0; x0 < k.W; x0 += kThreads) {     // workgroup-uniform: every barrier and ballot below is met by all threads
        const int x = x0 + tid, wp = x >> 6;
        const bool live = wp * 64 < k.W;             // wave-uniform
        int cnt = 0, last = -1;
        if (live) {
            for (int r = 0; r < blocks; ++r) {
                unsigned carry;
                const unsigned long long seg = rle_segment(k, mask, wp, r, lane, carry);
                const unsigned long long t = rle_transitions(seg, carry, k.H - r * 64);
                if (x < k.W && t) {
                    cnt += __popcll(t);
                    last = x * k.H + r * 64 + 63 - __clzll(t);
                }
            }
        }
        // exclusive scan over the strip's columns: sum of the counts, maximum of the last transitions
        int inc_c = cnt, inc_l = last;
        for (int d = 1; d < 64; d <<= 1) {
            const int c = __shfl_up(inc_c, d), l = __shfl_up(inc_l, d);
            if (lane >= d) { inc_c += c; inc_l = l > inc_l ? l : inc_l; }
        }
        if (lane == 63) { wave_count[wave] = inc_c; wave_last[wave] = inc_l; }
        const int left_l = __shfl_up(inc_l, 1);
        __syncthreads();
        int pre_c = total, pre_l = last_all;
        for (int w = 0; w < kWaves; ++w) {
            const int c = wave_count[w], l = wave_last[w];
            if (w < wave) { pre_c += c; pre_l = l > pre_l ? l : pre_l; }
            total += c;
            last_all = l > last_all ? l : last_all;
        }
        __syncthreads();     // the wave totals are rewritten by the next strip
        if (WRITE && live && __any(cnt > 0)) {
            long long pos = begin + pre_c + (inc_c - cnt);
            int prev = lane > 0 && left_l > pre_l ? left_l : pre_l;
            for (int r = 0; r < blocks; ++r) {
                unsigned carry;
                const unsigned long long seg = rle_segment(k, mask, wp, r, lane, carry);
                unsigned long long t = x < k.W ? rle_transitions(seg, carry, k.H - r * 64) : 0ull;
                for (; t; t &= t - 1) {
                    const int at = x * k.H + r * 64 + __builtin_ctzll(t);
                    if (pos >= begin && pos < end) k.counts[pos] = unsigned(at - prev);
                    prev = at;
                    ++pos;
                }
            }
        }
    }
    if (tid == 0) {
        if (WRITE) {
            const long long pos = begin + total;
            if (pos >= begin && pos < end) k.counts[pos] = unsigned(k.H * k.W - last_all);
        } else {
            k.lengths[m] = total + 1;
        }
    }
}

}  // namespace

int pope_sam_rle_check(const SamRleArgs& a) {
    if (a.n < 0 || a.H <= 0 || a.W <= 0 || a.H > kMaxSide || a.W > kMaxSide) return POPE_ERR_ARG;
    if (a.n == 0) return POPE_OK;
    if (!a.packed) return POPE_ERR_ARG;
    if (a.counts ? (!a.offsets || a.capacity < 0) : !a.lengths) return POPE_ERR_ARG;
    return POPE_OK;
}

int pope_launch_sam_rle(const SamRleArgs& a, hipStream_t stream) {
    POPE_TRY(pope_sam_rle_check(a));
    if (a.n == 0) return POPE_OK;
    RleK k = {};
    k.packed = a.packed; k.lengths = a.lengths; k.offsets = a.offsets; k.counts = a.counts; k.capacity = a.capacity;
    k.n = a.n; k.H = a.H; k.W = a.W; k.Wp = (a.W + 31) / 32;
    k.last_valid = (a.W & 31) ? (1u << (a.W & 31)) - 1u : ~0u;
    if (a.counts) {
        // the total the caller allocated for, read back before anything is written: too small a buffer is refused, not clipped
        long long total = -1;
        if (hipMemcpyAsync(&total, a.offsets + a.n, sizeof(total), hipMemcpyDeviceToHost, stream) != hipSuccess
            || hipStreamSynchronize(stream) != hipSuccess) return POPE_ERR_LAUNCH;
        if (total < 0) return POPE_ERR_ARG;
        if (total > a.capacity) return POPE_ERR_WORKSPACE;
        hipLaunchKernelGGL(sam_rle_kernel<true>, dim3(a.n), dim3(kThreads), 0, stream, k);
    } else {
        hipLaunchKernelGGL(sam_rle_kernel<false>, dim3(a.n), dim3(kThreads), 0, stream, k);
    }
    return pope_check_launch();
}
