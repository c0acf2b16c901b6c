// Batched image preprocessing on the GPU: what the reference does per proposal on the host with
// PIL + torchvision (segment_anything/segment_anything/dinov2_utils.py:55-78: ToPILImage -> Resize((256,256)) ->
// CenterCrop((196,196)) | Resize((224,224)) -> ToTensor -> Normalize) for P uint8 HWC crops at once, bit-identical to
// that host path: the resize is Pillow's 8-bit bilinear resample — two separable passes (horizontal, then vertical),
// per-output-pixel windows with 22-bit fixed-point weights, int32 accumulation from 2^21, each pass rounded to uint8 —
// with the window / weight tables built on the host in double precision exactly as Pillow builds them
// (pope_amd/preprocess.py:resize_tables); ToTensor and Normalize are one fp32 division and one fp32 subtract + division.
// Only the centre-crop window is computed.  Channel order is taken as given (the drivers pass cv2 BGR frames as RGB).
// HBM-bound streaming kernels: a thread per output pixel, the three channels of a pixel together, coalesced along x.
//
// SAM's input transform (segment_anything utils/transforms.py ResizeLongestSide.apply_image, modeling/sam.py preprocess) is
// the same resample of the WHOLE frame: the horizontal pass above over every input row, then `resize_v_kernel`, the vertical
// pass with two epilogues — the resized uint8 HWC image itself (pope_resize_u8), or (v - mean) / std on the 0..255 values
// into the top-left corner of a zero S x S square, NCHW fp32 (pope_sam_preprocess_u8_f32: resample, normalisation and pad in
// one result, the pad written by the same launch).  A thread of it owns four consecutive pixels of a row.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PIL_BITS = 22;   // Pillow: PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= PIL_BITS;
    return static_cast<unsigned char>(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass over the input rows the vertical pass will need, for the cropped output columns only:
// tmp[p][r][x][c], r = input row - row0, x = output column - left
__global__ __launch_bounds__(256) void resize_h_kernel(const unsigned char* __restrict__ img, int P, int Hin, int Win,
                                                        const int* __restrict__ hstart, const int* __restrict__ hcount,
                                                        const int* __restrict__ hk, int kh, int row0, int nrows, int left, int cw,
                                                        unsigned char* __restrict__ tmp) {
    const size_t total = size_t(P) * nrows * cw;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += size_t(gridDim.x) * 256) {
        const int x = int(i % cw);
        const size_t pr = i / cw;
        const int r = int(pr % nrows), p = int(pr / nrows);
        const int ox = left + x, s = hstart[ox], n = hcount[ox];
        const unsigned char* src = img + ((size_t(p) * Hin + row0 + r) * Win + s) * 3;
        const int* k = hk + size_t(ox) * kh;
        int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int w = k[t];
            a0 += int(src[3 * t]) * w;
            a1 += int(src[3 * t + 1]) * w;
            a2 += int(src[3 * t + 2]) * w;
        }
        unsigned char* o = tmp + i * 3;
        o[0] = clip8(a0); o[1] = clip8(a1); o[2] = clip8(a2);
    }
}

// vertical pass + centre crop + ToTensor (/255) + Normalize ((v - mean) / std), NCHW fp32
__global__ __launch_bounds__(256) void resize_v_norm_kernel(const unsigned char* __restrict__ tmp, int P, int row0, int nrows,
                                                             const int* __restrict__ vstart, const int* __restrict__ vcount,
                                                             const int* __restrict__ vk, int kv, int top, int ch, int cw,
                                                             float m0, float m1, float m2, float s0, float s1, float s2,
                                                             float* __restrict__ out) {
    const size_t total = size_t(P) * ch * cw;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += size_t(gridDim.x) * 256) {
        const int x = int(i % cw);
        const size_t py = i / cw;
        const int y = int(py % ch), p = int(py / ch);
        const int oy = top + y, s = vstart[oy], n = vcount[oy];
        const unsigned char* src = tmp + ((size_t(p) * nrows + (s - row0)) * cw + x) * 3;
        const int* k = vk + size_t(oy) * kv;
        int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int w = k[t];
            const unsigned char* q = src + size_t(t) * cw * 3;
            a0 += int(q[0]) * w;
            a1 += int(q[1]) * w;
            a2 += int(q[2]) * w;
        }
        const size_t plane = size_t(ch) * cw, o = size_t(p) * 3 * plane + size_t(y) * cw + x;
        out[o] = (float(clip8(a0)) / 255.0f - m0) / s0;
        out[o + plane] = (float(clip8(a1)) / 255.0f - m1) / s1;
        out[o + 2 * plane] = (float(clip8(a2)) / 255.0f - m2) / s2;
    }
}

// vertical pass over tmp[p][Hin][OW][3] (the horizontal pass of every input row of a frame) for the whole resized image.  A
// thread owns the four pixels x0 .. x0 + 3 of one row of the output grid, which is OH x OW for the uint8 epilogue and S x S for
// the fp32 one; pixels of the grid outside OH x OW are the pad.
// `vec` (OW % 4 == 0, `tmp` and a uint8 `out` 4-byte aligned): the 12 bytes of a quad are three aligned words, in `tmp` and in `out`.
//   F32 = false: out[p][y][x][c] uint8, the resample alone (three 4-byte stores when `vec`).
//   F32 = true:  out[p][c][y][x] fp32 = (float(v[flip ? 2 - c : c]) - mean[c]) / std[c] inside OH x OW and +0.0 outside; one
//                16-byte store per channel plane (S % 4 == 0, `out` 16-byte aligned), the quad that straddles OW selects per element.
// The windows are clipped to [0, Hin) and to kv weights whatever the tables say.
template <bool F32>
__global__ __launch_bounds__(256) void resize_v_kernel(const unsigned char* __restrict__ tmp, int P, int Hin,
                                                        const int* __restrict__ vstart, const int* __restrict__ vcount,
                                                        const int* __restrict__ vk, int kv, int OH, int OW, int S, int flip, int vec,
                                                        float m0, float m1, float m2, float s0, float s1, float s2,
                                                        void* __restrict__ out) {
    const int gh = F32 ? S : OH, gw = F32 ? S : OW, qw = (gw + 3) / 4;
    const size_t total = size_t(P) * gh * qw;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += size_t(gridDim.x) * 256) {
        const int x0 = 4 * int(i % qw);
        const size_t py = i / qw;
        const int y = int(py % gh), p = int(py / gh);
        const int nx = y < OH ? (OW - x0 < 4 ? OW - x0 : 4) : 0;   // pixels of this quad inside the image (<= 0: all pad)
        unsigned char v[12] = {};
        if (nx > 0) {
            int s = vstart[y], n = vcount[y];
            if (s < 0) s = 0;
            if (n > kv) n = kv;
            if (n > Hin - s) n = Hin - s;
            const unsigned char* src = tmp + ((size_t(p) * Hin + s) * OW + x0) * 3;
            const int* k = vk + size_t(y) * kv;
            int a[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) a[j] = 1 << (PIL_BITS - 1);
            if (vec) {   // nx == 4 in every quad and the 12 bytes of a tap are three aligned words
                for (int t = 0; t < n; ++t) {
                    const int w = k[t];
                    const unsigned* q = reinterpret_cast<const unsigned*>(src + size_t(t) * OW * 3);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const unsigned u = q[d];
#pragma unroll
                        for (int b = 0; b < 4; ++b) a[4 * d + b] += int((u >> (8 * b)) & 255u) * w;
                    }
                }
            } else {
                for (int t = 0; t < n; ++t) {
                    const int w = k[t];
                    const unsigned char* q = src + size_t(t) * OW * 3;
#pragma unroll
                    for (int j = 0; j < 12; ++j)
                        if (j < 3 * nx) a[j] += int(q[j]) * w;
                }
            }
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if (j < 3 * nx) v[j] = clip8(a[j]);
        }
        if constexpr (F32) {
            const size_t plane = size_t(S) * S;
            float* o = static_cast<float*>(out) + size_t(p) * 3 * plane + size_t(y) * S + x0;
            const float m[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned char u = flip ? v[3 * e + 2 - c] : v[3 * e + c];
                    r[e] = e < nx ? __fdiv_rn(__fsub_rn(float(u), m[c]), sd[c]) : 0.0f;
                }
                *reinterpret_cast<f32x4*>(o + c * plane) = r;
            }
        } else {
            unsigned char* o = static_cast<unsigned char*>(out) + ((size_t(p) * OH + y) * OW + x0) * 3;
            if (vec) {   // nx == 4 in every quad
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    reinterpret_cast<unsigned*>(o)[d] = unsigned(v[4 * d]) | unsigned(v[4 * d + 1]) << 8 | unsigned(v[4 * d + 2]) << 16
                                                        | unsigned(v[4 * d + 3]) << 24;
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < 3 * nx) o[j] = v[j];
            }
        }
    }
}

// cv2.cvtColor(BGR2GRAY) for 8-bit images (OpenCV's fixed-point form: B 1868, G 9617, R 4899, 14 fractional bits,
// round to nearest) followed by `/ 255.` (eval_linemod_json.py:103-111): [P,H,W,3] uint8 BGR -> [P,1,H,W] fp32
__global__ __launch_bounds__(256) void gray_kernel(const unsigned char* __restrict__ bgr, size_t npix, float* __restrict__ out) {
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < npix; i += size_t(gridDim.x) * 256) {
        const unsigned char* q = bgr + i * 3;
        const int g = (int(q[0]) * 1868 + int(q[1]) * 9617 + int(q[2]) * 4899 + (1 << 13)) >> 14;
        out[i] = float(g) / 255.0f;
    }
}

// ToTensor + Normalize of a crop window, no resize (torchvision: x / 255, then (x - mean) / std, fp32): the dense
// pair path feeds 476 x 630 centre crops of 640 x 480 frames.  [P, Hin, Win, 3] uint8 -> [P, 3, ch, cw] fp32; a thread
// converts four pixels of a row (12 input bytes, three 16-byte stores when cw % 4 == 0)
__global__ __launch_bounds__(256) void crop_norm_kernel(const unsigned char* __restrict__ img, int P, int Hin, int Win, int top,
                                                        int left, int ch, int cw, float m0, float m1, float m2, float s0, float s1,
                                                        float s2, float* __restrict__ out) {
    const int qw = (cw + 3) / 4;
    const size_t total = size_t(P) * ch * qw, plane = size_t(ch) * cw;
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += size_t(gridDim.x) * 256) {
        const int xq = int(i % qw);
        const size_t py = i / qw;
        const int y = int(py % ch), p = int(py / ch);
        const unsigned char* q = img + ((size_t(p) * Hin + top + y) * Win + left + 4 * xq) * 3;
        float* o = out + size_t(p) * 3 * plane + size_t(y) * cw + 4 * xq;
        const int nx = cw - 4 * xq < 4 ? cw - 4 * xq : 4;
        float r[3][4];
        for (int e = 0; e < nx; ++e) {
            r[0][e] = (float(q[3 * e]) / 255.0f - m0) / s0;
            r[1][e] = (float(q[3 * e + 1]) / 255.0f - m1) / s1;
            r[2][e] = (float(q[3 * e + 2]) / 255.0f - m2) / s2;
        }
        for (int c = 0; c < 3; ++c) {
            if (nx == 4 && !(cw & 3)) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{r[c][0], r[c][1], r[c][2], r[c][3]};
            else for (int e = 0; e < nx; ++e) o[c * plane + e] = r[c][e];
        }
    }
}


// cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) of uint8 images for P destination images at once — the drivers' proposal
// crops (utils/data_utils.py:239-255 called twice, eval_linemod_json.py:83-90).  minv[p][6] = the INVERSE map (destination
// pixel -> source position, what cv::warpAffine derives from the forward matrix) in fp64; evaluated per destination pixel
// the way OpenCV's 8-bit path does: 10-bit fixed point with a 1/64 px rounding offset, truncated to 1/32 px, the four
// neighbours blended with integer weights (32 - fx)(32 - fy) ... fx fy and rounded to nearest.  win[p] = (x0, y0, w, h):
// the source of image p is the w x h window of `img` whose top-left corner is (x0, y0) — pixels outside the window or
// outside `img` read as 0, which is exactly the intermediate zero-padded crop of the reference's first (integer
// translation) step, so the two warps of a proposal are ONE gather from the frame.
__global__ __launch_bounds__(256) void crop_warp_kernel(const unsigned char* __restrict__ img, int H, int W, int C,
                                                        const double* __restrict__ minv, const int* __restrict__ win, int P, int oh,
                                                        int ow, unsigned char* __restrict__ out) {
    const size_t total = size_t(P) * oh * ow;
    for (size_t id = size_t(blockIdx.x) * 256 + threadIdx.x; id < total; id += size_t(gridDim.x) * 256) {
        const int x = int(id % ow), y = int((id / ow) % oh), p = int(id / (size_t(ow) * oh));
        const double* m = minv + 6 * p;
        const int x0 = win[4 * p], y0 = win[4 * p + 1], ww = win[4 * p + 2], wh = win[4 * p + 3];
        // saturate_cast<int>(double) rounds to nearest even (rint)
        const long long adelta = (long long)rint(m[0] * x * 1024.0), bdelta = (long long)rint(m[3] * x * 1024.0);
        const long long X0 = (long long)rint((m[1] * y + m[2]) * 1024.0) + 16, Y0 = (long long)rint((m[4] * y + m[5]) * 1024.0) + 16;
        const long long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
        const long long sx = X >> 5, sy = Y >> 5;
        const int fx = int(X & 31), fy = int(Y & 31);
        const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
        const bool okx0 = sx >= 0 && sx < ww && sx + x0 >= 0 && sx + x0 < W, okx1 = sx + 1 >= 0 && sx + 1 < ww && sx + 1 + x0 >= 0 && sx + 1 + x0 < W;
        const bool oky0 = sy >= 0 && sy < wh && sy + y0 >= 0 && sy + y0 < H, oky1 = sy + 1 >= 0 && sy + 1 < wh && sy + 1 + y0 >= 0 && sy + 1 + y0 < H;
        const unsigned char* r0 = img + (size_t(oky0 ? sy + y0 : 0) * W) * C;
        const unsigned char* r1 = img + (size_t(oky1 ? sy + 1 + y0 : 0) * W) * C;
        const size_t c0 = size_t(okx0 ? sx + x0 : 0) * C, c1 = size_t(okx1 ? sx + 1 + x0 : 0) * C;
        unsigned char* o = out + id * C;
        for (int c = 0; c < C; ++c) {
            const int p00 = (oky0 && okx0) ? r0[c0 + c] : 0, p01 = (oky0 && okx1) ? r0[c1 + c] : 0;
            const int p10 = (oky1 && okx0) ? r1[c0 + c] : 0, p11 = (oky1 && okx1) ? r1[c1 + c] : 0;
            o[c] = (unsigned char)((p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 512) >> 10);
        }
    }
}

// The image pair of the image-conditioned pose heads (pose/dataset.py:102-106 -> train0604.py:148-151): cv2.resize(img, (OW, OH))
// of uint8 images (OpenCV's generic 8-bit INTER_LINEAR path: per axis a first tap and two coefficients with 11 fractional bits
// from the host, pope_amd/preprocess.py:resize_linear_cv_tables; horizontal pass in int32, vertical pass on the row sums >> 4 with
// two 16-bit shifts and a rounding >> 2), `.float()`, and the layout the heads are fed: out[q][c][x][y] (transposed: the
// reference's permute(0, 3, 2, 1)) or out[q][c][y][x], raw 0..255 values, channels as stored.  Image q is the resize of
// src[rows[q]] (rows == NULL: src[q]); a row outside [0, P) gives zeros and reads nothing.  `area`: both axes shrink exactly
// 2 x, where OpenCV averages the 2 x 2 block instead.  Integer arithmetic only.
// A workgroup owns a 32 x 32 tile of one output image: it computes the tile with x along the lanes (the source is contiguous along
// x), parks the three planes in LDS (rows padded to 33 words) and stores them with the output's fast axis along the lanes.
// Taps are clamped to the image whatever the tables say.
constexpr int PI_TILE = 32;

__global__ __launch_bounds__(256) void pose_images_kernel(const unsigned char* __restrict__ src, int P, int Hin, int Win,
                                                           const int* __restrict__ rows, const int* __restrict__ xstart,
                                                           const int* __restrict__ xcoef, const int* __restrict__ ystart,
                                                           const int* __restrict__ ycoef, int OH, int OW, int tiles_x, int tiles_y,
                                                           int transposed, int area, float* __restrict__ out) {
    __shared__ float tile[3][PI_TILE][PI_TILE + 1];
    const int per_image = tiles_x * tiles_y;
    const int q = int(blockIdx.x) / per_image, t = int(blockIdx.x) % per_image;
    const int oy0 = (t / tiles_x) * PI_TILE, ox0 = (t % tiles_x) * PI_TILE;
    const int r = rows ? rows[q] : q;
    const bool live = r >= 0 && r < P;
    const unsigned char* img = src + (live ? size_t(r) : size_t(0)) * Hin * Win * 3;
    const int lane = int(threadIdx.x) & 31, group = int(threadIdx.x) >> 5;

    const int ox = ox0 + lane;
    int sx = 0, sx1 = 0, ax0 = 0, ax1 = 0;
    if (live && ox < OW) {
        if (area) {
            sx = 2 * ox; sx1 = sx + 1;
        } else {
            sx = xstart[ox];
            sx = sx < 0 ? 0 : (sx > Win - 1 ? Win - 1 : sx);
            sx1 = sx + 1 > Win - 1 ? Win - 1 : sx + 1;
            ax0 = xcoef[2 * ox]; ax1 = xcoef[2 * ox + 1];
        }
    }
#pragma unroll
    for (int k = 0; k < PI_TILE / 8; ++k) {
        const int ly = group + 8 * k, oy = oy0 + ly;
        int v[3] = {0, 0, 0};
        if (live && ox < OW && oy < OH) {
            if (area) {
                const unsigned char* r0 = img + size_t(2 * oy) * Win * 3;
                const unsigned char* r1 = r0 + size_t(Win) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    v[c] = (int(r0[3 * sx + c]) + int(r0[3 * sx1 + c]) + int(r1[3 * sx + c]) + int(r1[3 * sx1 + c]) + 2) >> 2;
            } else {
                int sy = ystart[oy];
                sy = sy < 0 ? 0 : (sy > Hin - 1 ? Hin - 1 : sy);
                const int sy1 = sy + 1 > Hin - 1 ? Hin - 1 : sy + 1;
                const int ay0 = ycoef[2 * oy], ay1 = ycoef[2 * oy + 1];
                const unsigned char* r0 = img + size_t(sy) * Win * 3;
                const unsigned char* r1 = img + size_t(sy1) * Win * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int h0 = int(r0[3 * sx + c]) * ax0 + int(r0[3 * sx1 + c]) * ax1;
                    const int h1 = int(r1[3 * sx + c]) * ax0 + int(r1[3 * sx1 + c]) * ax1;
                    v[c] = (((ay0 * (h0 >> 4)) >> 16) + ((ay1 * (h1 >> 4)) >> 16) + 2) >> 2;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) tile[c][ly][lane] = float(v[c]);
    }
    __syncthreads();
    const size_t plane = size_t(OH) * OW;
    float* o = out + size_t(q) * 3 * plane;
#pragma unroll
    for (int k = 0; k < PI_TILE / 8; ++k) {
        const int far = group + 8 * k;
        // transposed: lanes run along y, the output's fast axis; else along x
        const int ly = transposed ? lane : far, lx = transposed ? far : lane;
        const int y = oy0 + ly, x = ox0 + lx;
        if (y < OH && x < OW) {
            const size_t at = transposed ? size_t(x) * OH + y : size_t(y) * OW + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c * plane + at] = tile[c][ly][lx];
        }
    }
}

inline unsigned grid_for(size_t n) { return unsigned(n / 256 + 1 < 16384 ? n / 256 + 1 : 16384); }

}  // namespace

int pope_launch_preprocess(const PreprocParams& p, hipStream_t stream) {
    if (!p.img || !p.out || !p.tmp || !p.hstart || !p.hcount || !p.hk || !p.vstart || !p.vcount || !p.vk) return POPE_ERR_ARG;
    if (p.P <= 0 || p.Hin <= 0 || p.Win <= 0 || p.ch <= 0 || p.cw <= 0 || p.top < 0 || p.left < 0 || p.kh <= 0 || p.kv <= 0) return POPE_ERR_ARG;
    if (p.row0 < 0 || p.nrows <= 0 || p.row0 + p.nrows > p.Hin) return POPE_ERR_ARG;
    hipLaunchKernelGGL(resize_h_kernel, dim3(grid_for(size_t(p.P) * p.nrows * p.cw)), dim3(256), 0, stream, p.img, p.P, p.Hin, p.Win,
                       p.hstart, p.hcount, p.hk, p.kh, p.row0, p.nrows, p.left, p.cw, p.tmp);
    hipLaunchKernelGGL(resize_v_norm_kernel, dim3(grid_for(size_t(p.P) * p.ch * p.cw)), dim3(256), 0, stream, p.tmp, p.P, p.row0,
                       p.nrows, p.vstart, p.vcount, p.vk, p.kv, p.top, p.ch, p.cw, p.mean[0], p.mean[1], p.mean[2], p.std[0],
                       p.std[1], p.std[2], p.out);
    return pope_check_launch();
}

int pope_resize_check(const ResizeParams& p) {
    if (!p.img || !p.out || !p.tmp || !p.hstart || !p.hcount || !p.hk || !p.vstart || !p.vcount || !p.vk) return POPE_ERR_ARG;
    if (p.P <= 0 || p.Hin <= 0 || p.Win <= 0 || p.OH <= 0 || p.OW <= 0 || p.kh <= 0 || p.kv <= 0) return POPE_ERR_ARG;
    if (p.f32 && (p.S <= 0 || (p.S & 3) || p.OH > p.S || p.OW > p.S || (reinterpret_cast<uintptr_t>(p.out) & 15))) return POPE_ERR_ARG;
    if (p.tmp_bytes < size_t(p.P) * p.Hin * p.OW * 3) return POPE_ERR_WORKSPACE;
    return POPE_OK;
}

int pope_launch_resize(const ResizeParams& p, hipStream_t stream) {
    POPE_TRY(pope_resize_check(p));
    hipLaunchKernelGGL(resize_h_kernel, dim3(grid_for(size_t(p.P) * p.Hin * p.OW)), dim3(256), 0, stream, p.img, p.P, p.Hin, p.Win,
                       p.hstart, p.hcount, p.hk, p.kh, 0, p.Hin, 0, p.OW, p.tmp);
    const int vec = !(p.OW & 3) && !(reinterpret_cast<uintptr_t>(p.tmp) & 3) && (p.f32 || !(reinterpret_cast<uintptr_t>(p.out) & 3));
    if (p.f32) {
        hipLaunchKernelGGL(resize_v_kernel<true>, dim3(grid_for(size_t(p.P) * p.S * (p.S / 4))), dim3(256), 0, stream, p.tmp, p.P, p.Hin,
                           p.vstart, p.vcount, p.vk, p.kv, p.OH, p.OW, p.S, p.flip ? 1 : 0, vec, p.mean[0], p.mean[1], p.mean[2], p.std[0],
                           p.std[1], p.std[2], p.out);
    } else {
        hipLaunchKernelGGL(resize_v_kernel<false>, dim3(grid_for(size_t(p.P) * p.OH * ((p.OW + 3) / 4))), dim3(256), 0, stream, p.tmp, p.P,
                           p.Hin, p.vstart, p.vcount, p.vk, p.kv, p.OH, p.OW, 0, 0, vec, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, p.out);
    }
    return pope_check_launch();
}

int pope_launch_crop_norm(const unsigned char* img, int P, int Hin, int Win, int top, int left, int ch, int cw, const float* mean,
                          const float* std, float* out, hipStream_t stream) {
    if (!img || !out || !mean || !std || P <= 0 || ch <= 0 || cw <= 0 || top < 0 || left < 0 || top + ch > Hin || left + cw > Win)
        return POPE_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(out) & 15) return POPE_ERR_ARG;
    hipLaunchKernelGGL(crop_norm_kernel, dim3(grid_for(size_t(P) * ch * ((cw + 3) / 4))), dim3(256), 0, stream, img, P, Hin, Win, top,
                       left, ch, cw, mean[0], mean[1], mean[2], std[0], std[1], std[2], out);
    return pope_check_launch();
}

int pope_pose_images_check(const PoseImagesParams& p) {
    if (!p.src || !p.out || !p.xstart || !p.xcoef || !p.ystart || !p.ycoef) return POPE_ERR_ARG;
    if (p.P <= 0 || p.Hin <= 0 || p.Win <= 0 || p.OH <= 0 || p.OW <= 0 || p.Q < 0) return POPE_ERR_ARG;
    if (!p.rows && p.Q != p.P) return POPE_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(p.out) & 3) return POPE_ERR_ARG;
    const size_t tiles = size_t((p.OW + PI_TILE - 1) / PI_TILE) * size_t((p.OH + PI_TILE - 1) / PI_TILE);
    if (tiles > 0x7fffffffu || tiles * size_t(p.Q) > 0x7fffffffu) return POPE_ERR_ARG;   // one workgroup per tile, a flat grid
    return POPE_OK;
}

int pope_launch_pose_images(const PoseImagesParams& p, hipStream_t stream) {
    POPE_TRY(pope_pose_images_check(p));
    if (p.Q == 0) return POPE_OK;
    const int tiles_x = (p.OW + PI_TILE - 1) / PI_TILE, tiles_y = (p.OH + PI_TILE - 1) / PI_TILE;
    const int area = p.Hin == 2 * p.OH && p.Win == 2 * p.OW;
    hipLaunchKernelGGL(pose_images_kernel, dim3(unsigned(p.Q) * tiles_x * tiles_y), dim3(256), 0, stream, p.src, p.P, p.Hin, p.Win,
                       p.rows, p.xstart, p.xcoef, p.ystart, p.ycoef, p.OH, p.OW, tiles_x, tiles_y, p.transposed ? 1 : 0, area, p.out);
    return pope_check_launch();
}

int pope_launch_gray(const unsigned char* bgr, size_t npix, float* out, hipStream_t stream) {
    if (!bgr || !out || !npix) return POPE_ERR_ARG;
    hipLaunchKernelGGL(gray_kernel, dim3(grid_for(npix)), dim3(256), 0, stream, bgr, npix, out);
    return pope_check_launch();
}

int pope_launch_crop_warp(const unsigned char* img, int H, int W, int C, const double* minv, const int* win, int P, int oh, int ow,
                          unsigned char* out, hipStream_t stream) {
    if (!img || !minv || !win || !out || H <= 0 || W <= 0 || C <= 0 || C > 4 || P <= 0 || oh <= 0 || ow <= 0) return POPE_ERR_ARG;
    hipLaunchKernelGGL(crop_warp_kernel, dim3(grid_for(size_t(P) * oh * ow)), dim3(256), 0, stream, img, H, W, C, minv, win, P, oh, ow, out);
    return pope_check_launch();
}
