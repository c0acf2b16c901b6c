// SAM automatic mask generator, post-processing of one decoder call (segment_anything/modeling/sam.py:postprocess_masks +
// the tail of automatic_mask_generator.py:_process_batch) in one pass over the low-res logits: per selected mask the
// frame-resolution logit of every pixel is recomputed from the 256 x 256 logits (two bilinear resamplings, bit-equal to torch's
// CPU kernels), thresholded three times, counted, boxed and bit-packed.  Neither the 1024 x 1024 nor the H x W fp32 tensor is
// ever written (except on request: the dense store behind Sam.postprocess_masks).
//
// Arithmetic of one axis (n_in -> n_out samples, align_corners=False), every step one fp32 rounding:
//   scale = (float)n_in / (float)n_out;  src = max(fmaf(scale, dst + 0.5f, -0.5f), 0);  i0 = (int)src;  i1 = min(i0 + 1, n_in - 1)
//   l1 = src - i0;  l0 = 1 - l1;  out = fmaf(l0, in[i0], l1 * in[i1])      (x axis first, then y)
// The build has -ffp-contract=off; the fused and the rounded operations are spelled out.
//
// One workgroup = (selected mask, band of output rows).  Stage 1: the x pass of the FIRST resampling for the few low-res rows
// the band touches, T[q][c] for c < iw, into LDS (shared by every output row of the band).  Stage 2: one wave per output row,
// 64 pixels per step: 4 mid-grid values from 8 LDS reads, the second resampling, three ballots.  Counts and box extrema are
// wave-uniform integers; they meet in LDS and leave as one vector atomic each per band (integer add / min / max: the result
// does not depend on the launch order).  Mask bits leave as one 32-bit word per lane, a whole row per store.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNmsMax = 2048;
constexpr size_t kLdsBudget = 40 * 1024;   // per workgroup in stage 1: four workgroups per CU
constexpr size_t kLdsMax = 64 * 1024;

struct Tap { int i0, i1; float l1; };

__host__ __device__ inline Tap axis_tap(int n_in, int n_out, int dst) {
#ifdef __HIP_DEVICE_COMPILE__
    const float scale = __fdiv_rn((float)n_in, (float)n_out);
    const float src = fmaxf(__fmaf_rn(scale, (float)dst + 0.5f, -0.5f), 0.0f);
#else
    const float scale = (float)n_in / (float)n_out;
    const float src = fmaxf(__builtin_fmaf(scale, (float)dst + 0.5f, -0.5f), 0.0f);
#endif
    Tap t;
    t.i0 = (int)src;
    if (t.i0 > n_in - 1) t.i0 = n_in - 1;   // never taken for a finite scale; keeps every index in range regardless
    t.i1 = t.i0 + 1 < n_in - 1 ? t.i0 + 1 : n_in - 1;
    t.l1 = src - (float)t.i0;
    return t;
}

// Tables in the workspace: three arrays (i0, i1, l1) per axis.
struct Tables {
    int *my0, *my1; float* myl;     // low rows  -> img rows      [img]
    int *mx0, *mx1; float* mxl;     // low cols  -> img cols      [img]
    int *oy0, *oy1; float* oyl;     // img rows (cropped to ih) -> H   [H]
    int *ox0, *ox1; float* oxl;     // img cols (cropped to iw) -> W   [W]
};

inline size_t table_words(int img, int H, int W) { return 3 * (2 * size_t(img) + size_t(H) + size_t(W)); }

inline Tables carve(void* ws, int img, int H, int W) {
    int* p = static_cast<int*>(ws);
    Tables t;
    auto take = [&](int n) { int* r = p; p += n; return r; };
    t.my0 = take(img); t.my1 = take(img); t.myl = reinterpret_cast<float*>(take(img));
    t.mx0 = take(img); t.mx1 = take(img); t.mxl = reinterpret_cast<float*>(take(img));
    t.oy0 = take(H); t.oy1 = take(H); t.oyl = reinterpret_cast<float*>(take(H));
    t.ox0 = take(W); t.ox1 = take(W); t.oxl = reinterpret_cast<float*>(take(W));
    return t;
}

struct PostK {
    const float* low; int M, h, w;
    const int* sel; int n_sel;
    int img, ih, iw, H, W;
    float thr_hi, thr_lo, thr;
    int* stats; unsigned* packed; float* logits;
    Tables t;
    int band_rows, nbands, max_rows, pitch;
};

// stats rows while the bands accumulate: n_hi, n_lo, area, min x, min y, max x, max y, -
__global__ __launch_bounds__(256) void sam_post_setup_kernel(PostK k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < k.img) {
        Tap a = axis_tap(k.h, k.img, i);
        k.t.my0[i] = a.i0; k.t.my1[i] = a.i1; k.t.myl[i] = a.l1;
        a = axis_tap(k.w, k.img, i);
        k.t.mx0[i] = a.i0; k.t.mx1[i] = a.i1; k.t.mxl[i] = a.l1;
    }
    if (i < k.H) { const Tap a = axis_tap(k.ih, k.H, i); k.t.oy0[i] = a.i0; k.t.oy1[i] = a.i1; k.t.oyl[i] = a.l1; }
    if (i < k.W) { const Tap a = axis_tap(k.iw, k.W, i); k.t.ox0[i] = a.i0; k.t.ox1[i] = a.i1; k.t.oxl[i] = a.l1; }
    if (i < k.n_sel) {
        int* s = k.stats + size_t(i) * 8;
        s[0] = s[1] = s[2] = 0; s[3] = s[4] = 0x7fffffff; s[5] = s[6] = -1; s[7] = 0;
    }
}

// stats rows as the caller reads them: n_hi, n_lo, area, x0, y0, x1, y1 (batched_mask_to_box), stability score (fp32 bits)
__global__ __launch_bounds__(256) void sam_post_finish_kernel(int* stats, int n_sel) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sel) return;
    int* s = stats + size_t(i) * 8;
    if (s[5] < s[3] || s[6] < s[4]) s[3] = s[4] = s[5] = s[6] = 0;
    s[7] = __float_as_int(__fdiv_rn((float)s[0], (float)s[1]));   // calculate_stability_score: int / int in fp32, 0 / 0 = nan
}

template <bool DENSE>
__global__ __launch_bounds__(kThreads) void sam_post_kernel(PostK k) {
    extern __shared__ float T[];   // [rows of this band][iw]
    __shared__ int red[7];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band = blockIdx.x % k.nbands, j = blockIdx.x / k.nbands;
    const int Y0 = band * k.band_rows, Y1 = min(Y0 + k.band_rows, k.H) - 1;
    const int m = k.sel ? k.sel[j] : j;
    const int low_lo = k.t.my0[k.t.oy0[Y0]], low_hi = k.t.my1[k.t.oy1[Y1]];
    const int rows = low_hi - low_lo + 1;
    if ((unsigned)m >= (unsigned)k.M || rows > k.max_rows || rows <= 0) {
        // an index outside the batch selects nothing: an empty mask (workgroup-uniform exit, before any barrier)
        if (k.packed)
            for (int i = tid; i < (Y1 - Y0 + 1) * k.pitch; i += kThreads) k.packed[(size_t(j) * k.H + Y0) * k.pitch + i] = 0u;
        return;
    }
    if (tid < 7) red[tid] = tid < 3 ? 0 : (tid < 5 ? 0x7fffffff : -1);

    // stage 1: x pass of the first resampling
    const float* src = k.low + (size_t(m) * k.h + low_lo) * k.w;
    for (int q = 0; q < rows; ++q) {
        const float* row = src + size_t(q) * k.w;
        for (int c = tid; c < k.iw; c += kThreads) {
            const float l1 = k.t.mxl[c];
            T[q * k.iw + c] = __fmaf_rn(1.0f - l1, row[k.t.mx0[c]], __fmul_rn(l1, row[k.t.mx1[c]]));
        }
    }
    __syncthreads();

    // stage 2
    int n_hi = 0, n_lo = 0, area = 0, xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    const int steps = (k.W + 63) / 64;
    for (int Y = Y0 + wave; Y <= Y1; Y += kWaves) {
        const int r0 = k.t.oy0[Y], r1 = k.t.oy1[Y];
        const float wy1 = k.t.oyl[Y], wy0 = 1.0f - wy1;
        const float a1 = k.t.myl[r0], a0 = 1.0f - a1, b1 = k.t.myl[r1], b0 = 1.0f - b1;
        const float* Ta0 = T + (k.t.my0[r0] - low_lo) * k.iw;
        const float* Ta1 = T + (k.t.my1[r0] - low_lo) * k.iw;
        const float* Tb0 = T + (k.t.my0[r1] - low_lo) * k.iw;
        const float* Tb1 = T + (k.t.my1[r1] - low_lo) * k.iw;
        unsigned word = 0u;
        for (int s = 0; s < steps; ++s) {
            const int X = s * 64 + lane;
            const bool in = X < k.W;
            const int Xc = in ? X : k.W - 1;
            const int c0 = k.t.ox0[Xc], c1 = k.t.ox1[Xc];
            const float wx1 = k.t.oxl[Xc], wx0 = 1.0f - wx1;
            const float ma0 = __fmaf_rn(a0, Ta0[c0], __fmul_rn(a1, Ta1[c0]));
            const float ma1 = __fmaf_rn(a0, Ta0[c1], __fmul_rn(a1, Ta1[c1]));
            const float mb0 = __fmaf_rn(b0, Tb0[c0], __fmul_rn(b1, Tb1[c0]));
            const float mb1 = __fmaf_rn(b0, Tb0[c1], __fmul_rn(b1, Tb1[c1]));
            const float ta = __fmaf_rn(wx0, ma0, __fmul_rn(wx1, ma1));
            const float tb = __fmaf_rn(wx0, mb0, __fmul_rn(wx1, mb1));
            const float v = __fmaf_rn(wy0, ta, __fmul_rn(wy1, tb));
            if (DENSE && in) k.logits[(size_t(j) * k.H + Y) * k.W + X] = v;
            const unsigned long long bm = __ballot(in && v > k.thr);
            n_hi += __popcll(__ballot(in && v > k.thr_hi));
            n_lo += __popcll(__ballot(in && v > k.thr_lo));
            area += __popcll(bm);
            if (bm) {
                xmin = min(xmin, s * 64 + (__ffsll(bm) - 1));
                xmax = max(xmax, s * 64 + 63 - __clzll(bm));
                ymin = min(ymin, Y);
                ymax = max(ymax, Y);
            }
            // lane 2 s' + p of each group of 32 steps keeps half p of step s' (the ballot is wave-uniform: no shuffle)
            if ((lane >> 1) == (s & 31)) word = (lane & 1) ? unsigned(bm >> 32) : unsigned(bm);
            if (k.packed && ((s & 31) == 31 || s == steps - 1)) {
                const int wi = (s & ~31) * 2 + lane;
                if (wi < k.pitch) k.packed[(size_t(j) * k.H + Y) * k.pitch + wi] = word;
                word = 0u;
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&red[0], n_hi); atomicAdd(&red[1], n_lo); atomicAdd(&red[2], area);
        atomicMin(&red[3], xmin); atomicMin(&red[4], ymin); atomicMax(&red[5], xmax); atomicMax(&red[6], ymax);
    }
    __syncthreads();
    int* out = k.stats + size_t(j) * 8;
    if (tid < 3) { if (red[tid]) atomicAdd(out + tid, red[tid]); }
    else if (tid < 5) atomicMin(out + tid, red[tid]);
    else if (tid < 7) atomicMax(out + tid, red[tid]);
}

// Greedy NMS of n <= kNmsMax boxes in one workgroup: stable rank by score (descending), then a serial walk over the ranked
// boxes; each kept box marks what it suppresses in parallel.  IoU exactly as torchvision's nms kernel computes it in fp32.
// `boxes`, `scores` and `keep` point at the workgroup's own boxes; the kept indices are written as `base` + local index.
struct NmsShared {
    float4 sb[kNmsMax];
    float sarea[kNmsMax];
    float sscore[kNmsMax];
    int sorder[kNmsMax];
    unsigned char dead[kNmsMax];
};

__device__ inline void sam_nms_workgroup(NmsShared& sh, const float* boxes, const float* scores, int n, float thresh, int base,
                                         int* keep, int* count) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 1024) {
        const float s = scores[i];
        sh.sscore[i] = s == s ? s : -INFINITY;   // a nan score ranks last (keeps the ranks a permutation)
        sh.dead[i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const float s = sh.sscore[i];
        int rank = 0;
        for (int q = 0; q < n; ++q) {
            const float sq = sh.sscore[q];
            rank += (sq > s) || (sq == s && q < i);
        }
        sh.sorder[rank] = i;
    }
    __syncthreads();
    for (int r = tid; r < n; r += 1024) {
        const float* b = boxes + size_t(sh.sorder[r]) * 4;
        sh.sb[r] = make_float4(b[0], b[1], b[2], b[3]);
        sh.sarea[r] = __fmul_rn(b[2] - b[0], b[3] - b[1]);
    }
    __syncthreads();
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        if (sh.dead[i]) continue;   // workgroup-uniform: dead[] only changes between barriers
        if (tid == 0) keep[kept] = base + sh.sorder[i];
        ++kept;
        const float4 bi = sh.sb[i];
        const float ai = sh.sarea[i];
        for (int q = i + 1 + tid; q < n; q += 1024) {
            const float4 bq = sh.sb[q];
            const float w = fmaxf(0.0f, fminf(bi.z, bq.z) - fmaxf(bi.x, bq.x));
            const float h = fmaxf(0.0f, fminf(bi.w, bq.w) - fmaxf(bi.y, bq.y));
            const float inter = __fmul_rn(w, h);
            const float ovr = __fdiv_rn(inter, (ai + sh.sarea[q]) - inter);
            if (ovr > thresh) sh.dead[q] = 1;
        }
        __syncthreads();
    }
    if (tid == 0) *count = kept;
}

__global__ __launch_bounds__(1024) void sam_nms_kernel(const float* boxes, const float* scores, int n, float thresh, int* keep,
                                                       int* count) {
    __shared__ NmsShared sh;
    sam_nms_workgroup(sh, boxes, scores, n, thresh, 0, keep, count);
}

// S independent segments, one workgroup each: segment s owns boxes seg_offsets[s] .. seg_offsets[s + 1] - 1 of the n.  The
// offsets are device data, so they are clamped to [0, n] here; a segment that does not fit the LDS arrays is not run at all.
__global__ __launch_bounds__(1024) void sam_nms_segments_kernel(const float* boxes, const float* scores, const int* seg_offsets,
                                                                int n, float thresh, int* keep, int* count) {
    __shared__ NmsShared sh;
    const int s = blockIdx.x;
    int b = seg_offsets[s], e = seg_offsets[s + 1];
    b = b < 0 ? 0 : (b > n ? n : b);
    e = e < b ? b : (e > n ? n : e);
    if (e - b > kNmsMax) {           // workgroup-uniform
        if (threadIdx.x == 0) count[s] = -1;
        return;
    }
    sam_nms_workgroup(sh, boxes + size_t(b) * 4, scores + b, e - b, thresh, b, keep + b, count + s);
}

// Largest band (16, 8, .. 1 output rows) whose stage-1 rows fit the LDS budget; the tables are recomputed on the host with the
// same fp32 operations the setup kernel uses.
bool plan_bands(const SamPostArgs& a, int& band_rows, int& max_rows) {
    for (int br = 16; br >= 1; br >>= 1) {
        int worst = 0;
        for (int Y0 = 0; Y0 < a.H; Y0 += br) {
            const int Y1 = (Y0 + br < a.H ? Y0 + br : a.H) - 1;
            const int lo = axis_tap(a.h, a.img, axis_tap(a.ih, a.H, Y0).i0).i0;
            const int hi = axis_tap(a.h, a.img, axis_tap(a.ih, a.H, Y1).i1).i1;
            worst = hi - lo + 1 > worst ? hi - lo + 1 : worst;
        }
        const size_t bytes = size_t(worst) * a.iw * sizeof(float);
        if (bytes <= kLdsBudget || (br == 1 && bytes <= kLdsMax)) { band_rows = br; max_rows = worst; return true; }
    }
    return false;
}

bool post_args_ok(const SamPostArgs& a) {
    return a.M > 0 && a.h > 0 && a.w > 0 && a.img > 0 && a.ih > 0 && a.iw > 0 && a.ih <= a.img && a.iw <= a.img && a.H > 0 && a.W > 0
           && a.n_sel >= 0 && a.img <= (1 << 14) && a.H <= (1 << 14) && a.W <= (1 << 14) && a.h <= (1 << 14) && a.w <= (1 << 14);
}

}  // namespace

size_t pope_sam_postprocess_workspace(int img, int H, int W) {
    if (img <= 0 || H <= 0 || W <= 0 || img > (1 << 14) || H > (1 << 14) || W > (1 << 14)) return 0;
    return table_words(img, H, W) * sizeof(int);
}

int pope_launch_sam_postprocess(const SamPostArgs& a, hipStream_t stream) {
    if (!post_args_ok(a) || !a.low || !a.stats || !a.ws) return POPE_ERR_ARG;
    if (a.ws_bytes < pope_sam_postprocess_workspace(a.img, a.H, a.W)) return POPE_ERR_WORKSPACE;
    if (a.n_sel == 0) return POPE_OK;
    PostK k = {};
    k.low = a.low; k.M = a.M; k.h = a.h; k.w = a.w; k.sel = a.sel; k.n_sel = a.n_sel;
    k.img = a.img; k.ih = a.ih; k.iw = a.iw; k.H = a.H; k.W = a.W;
    // torch compares an fp32 tensor with a Python float in fp32: the sums in double, rounded once
    k.thr_hi = float(a.mask_threshold + a.stability_offset);
    k.thr_lo = float(a.mask_threshold - a.stability_offset);
    k.thr = float(a.mask_threshold);
    k.stats = a.stats; k.packed = a.packed; k.logits = a.logits;
    k.t = carve(a.ws, a.img, a.H, a.W);
    k.pitch = (a.W + 31) / 32;
    if (!plan_bands(a, k.band_rows, k.max_rows)) return POPE_ERR_ARG;
    k.nbands = (a.H + k.band_rows - 1) / k.band_rows;
    if (size_t(k.nbands) * a.n_sel > 0x7fffffffull) return POPE_ERR_ARG;
    int most = a.img > a.H ? a.img : a.H;
    most = most > a.W ? most : a.W;
    most = most > a.n_sel ? most : a.n_sel;
    hipLaunchKernelGGL(sam_post_setup_kernel, dim3((most + 255) / 256), dim3(256), 0, stream, k);
    const size_t lds = size_t(k.max_rows) * a.iw * sizeof(float);
    const dim3 grid(unsigned(k.nbands) * unsigned(a.n_sel));
    if (a.logits) hipLaunchKernelGGL(sam_post_kernel<true>, grid, dim3(kThreads), lds, stream, k);
    else hipLaunchKernelGGL(sam_post_kernel<false>, grid, dim3(kThreads), lds, stream, k);
    hipLaunchKernelGGL(sam_post_finish_kernel, dim3((a.n_sel + 255) / 256), dim3(256), 0, stream, a.stats, a.n_sel);
    return pope_check_launch();
}

int pope_launch_sam_nms(const float* boxes, const float* scores, int n, float thresh, int* keep, int* count, hipStream_t stream) {
    if (n < 0 || n > kNmsMax || !count || (n > 0 && (!boxes || !scores || !keep))) return POPE_ERR_ARG;
    hipLaunchKernelGGL(sam_nms_kernel, dim3(1), dim3(1024), 0, stream, boxes, scores, n, thresh, keep, count);
    return pope_check_launch();
}

int pope_launch_sam_nms_segments(const float* boxes, const float* scores, const int* seg_offsets, int S, int n, float thresh,
                                 int* keep, int* count, hipStream_t stream) {
    if (S < 0 || n < 0 || (S > 0 && (!seg_offsets || !count)) || (S > 0 && n > 0 && (!boxes || !scores || !keep))) return POPE_ERR_ARG;
    if (S == 0) return POPE_OK;
    hipLaunchKernelGGL(sam_nms_segments_kernel, dim3(S), dim3(1024), 0, stream, boxes, scores, seg_offsets, n, thresh, keep, count);
    return pope_check_launch();
}
