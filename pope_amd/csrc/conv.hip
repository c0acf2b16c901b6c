// LoFTR local-feature CNN (ResNetFPN_8_2, src/matcher/backbone/resnet_fpn.py:43-118) on the f16x3 planes GEMM.
//
// Activations live as activation planes (pope_hip.h layout, scale 8) in NHWC with a ONE-PIXEL ZERO BORDER:
//     T[n][Hp = H + 2][Wp = W + 2][Cp = channels rounded up to 32],   one pixel = one planes row of Cp * 4 bytes.
// A 3x3 stride-1 convolution is then ONE planes GEMM with no im2col at all (gemm_planes.hip, CONV): output row R
// is pixel R + Wp + 1, and the A row of tap (dy, dx) is row R + dy * Wp + dx — the same shift for every row, i.e. a
// scalar offset per K-step of the loader.  Rows that are border pixels come out as garbage and are zeroed afterwards
// (`zero_border_kernel`, (2 Hp + 2 Wp) / (Hp Wp) of the rows); eval-mode BatchNorm is folded into filter and bias by the
// host (pope_amd/loftr.py), ReLU / LeakyReLU / the BasicBlock shortcut are the GEMM's epilogue (EPI_CONV).
// The three stride-2 layers (7x7 stem on the gray image, the first 3x3 and the 1x1 shortcut of layer2 / layer3) gather
// their taps into planes rows first (their outputs are 4x smaller than their inputs), 1x1 convolutions are plain GEMMs
// over the pixel rows, and the FPN's bilinear x2 (align_corners) + lateral add is the epilogue of the lateral convolution.
// The GemmParams of every form and the one-layer launch sequences have names (conv_layer.h); pope_launch_conv_layer runs one of them.
// POPE_PREC_F16 (opt-in, ResNetFPN_8_2.precision = "f16"): the same sequence on plain f16 rows (value * 8, 64-column chunks) and
// f16 weights (value * 256) — one MFMA per product (gemm_planes.hip PLAIN), every layer output rounded once in its epilogue; same
// buffers with narrower pitches (kPitchF16), stride-2 layers always gathered, the stem's 49 taps as one chunk plus a zero chunk.
#include "common.h"
#include "conv_layer.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr float A_SCALE = K_PLANES_ACT_SCALE;

// 7x7 stride-2 pad-3 taps of the gray image as planes rows [n * Hp * Wp, 64] (49 taps, zero-filled to two 32-column
// chunks), one row per pixel of the zero-bordered H/2 x W/2 output grid (border rows all zero).
// STEM_F16: plain f16 rows, value * 8 — the 49 taps as ONE 64-column chunk; the row keeps the pitch (256 bytes) and its second
// chunk is written as zeros: the tile kernel's stream wants two K-steps, and the weights' second chunk is zero too
enum { STEM_F32 = 0, STEM_PLANES = 1, STEM_F16 = 2 };
template <int FORM>   // STEM_F32: the fp32 twin (rows of 64 floats, same pitch in bytes)
__global__ __launch_bounds__(256) void stem_gather_kernel(const float* __restrict__ img, _Float16* __restrict__ out,
                                                          int n, int H, int W, unsigned* range_flag) {
    const int Hp = H / 2 + 2, Wp = W / 2 + 2;
    const long long total = (long long)n * Hp * Wp * 8;   // eight 8-column pieces per row
    float amax = 0.f;
    for (long long id = blockIdx.x * 256ll + threadIdx.x; id < total; id += 256ll * gridDim.x) {
        const int t = int(id & 7);
        const long long row = id >> 3;
        const int xo = int(row % Wp), yo = int((row / Wp) % Hp), b = int(row / ((long long)Wp * Hp));
        const bool interior = xo >= 1 && xo < Wp - 1 && yo >= 1 && yo < Hp - 1;
        pope_f16x8 hi, lo;
        float raw[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 8 * t + e, ky = c / 7, kx = c - 7 * ky;
            const int y = 2 * (yo - 1) + ky - 3, x = 2 * (xo - 1) + kx - 3;
            float v = 0.f;
            if (interior && c < 49 && y >= 0 && y < H && x >= 0 && x < W) v = img[((size_t)b * H + y) * W + x];
            amax = fmaxf(amax, fabsf(v));
            if (!(v == v)) amax = INFINITY;
            raw[e] = v;
            const float s = v * A_SCALE;
            hi[e] = _Float16(s);
            lo[e] = _Float16(s - float(hi[e]));
        }
        if constexpr (FORM == STEM_F16) {
            _Float16* o = out + row * 128 + 8 * t;
            *reinterpret_cast<pope_f16x8*>(o) = hi;
            *reinterpret_cast<pope_f16x8*>(o + 64) = pope_f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        } else if constexpr (FORM == STEM_PLANES) {
            // its own split and store (the same map as pope_planes_col(8 * t)): through pope_planes_store this kernel measured
            // 3 % slower on its own, see profiles/operand_producers.md
            _Float16* o = out + row * 128 + (t >> 2) * 64 + (t & 3) * 8;
            *reinterpret_cast<pope_f16x8*>(o) = hi;
            *reinterpret_cast<pope_f16x8*>(o + 32) = lo;
        } else {
            float* o = reinterpret_cast<float*>(out) + row * 64 + 8 * t;
            *reinterpret_cast<f32x4*>(o) = f32x4{raw[0], raw[1], raw[2], raw[3]};
            *reinterpret_cast<f32x4*>(o + 4) = f32x4{raw[4], raw[5], raw[6], raw[7]};
        }
    }
    if constexpr (FORM != STEM_F32) pope_range_flag(range_flag, POPE_RANGE_INPUT, !(amax * A_SCALE < POPE_F16_OVERFLOW));
}

// Stride-2 taps of a zero-bordered planes tensor [n, Hpi, Wpi, cch chunks] as planes rows [n * Hpo * Wpo, taps * cch
// chunks] over the zero-bordered output grid (Hpo = (Hpi - 2) / 2 + 2): taps = 9 (3x3, pad 1; tap-major as the
// weights) or 1 (the 1x1 shortcut: the centre).  A pure 16-byte copy: planes stay planes.
__global__ __launch_bounds__(256) void gather_s2_kernel(const u32x4* __restrict__ in, u32x4* __restrict__ out, int n, int Hpi,
                                                        int Wpi, int cch, int taps) {
    const int Hpo = (Hpi - 2) / 2 + 2, Wpo = (Wpi - 2) / 2 + 2;
    const int per_row = taps * cch * 8;
    const long long total = (long long)n * Hpo * Wpo * per_row;
    for (long long id = blockIdx.x * 256ll + threadIdx.x; id < total; id += 256ll * gridDim.x) {
        const int piece = int(id % per_row);
        const long long row = id / per_row;
        const int xo = int(row % Wpo), yo = int((row / Wpo) % Hpo), b = int(row / ((long long)Wpo * Hpo));
        const int pc = piece & 7, chunk = (piece >> 3) % cch, tap = (piece >> 3) / cch;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (xo >= 1 && xo < Wpo - 1 && yo >= 1 && yo < Hpo - 1) {
            const int ky = taps == 9 ? tap / 3 : 1, kx = taps == 9 ? tap - 3 * (tap / 3) : 1;
            const int yi = 2 * (yo - 1) + ky, xi = 2 * (xo - 1) + kx;   // padded input coordinates
            v = in[(((size_t)b * Hpi + yi) * Wpi + xi) * (cch * 8) + chunk * 8 + pc];
        }
        out[id] = v;
    }
}

// zero the border pixels' rows of a [n, Hp, Wp] pixel-row tensor (row_bytes per pixel: planes or fp32, same pitch)
__global__ __launch_bounds__(256) void zero_border_kernel(u32x4* __restrict__ buf, int n, int Hp, int Wp, int row_pieces) {
    const int per_img = 2 * Wp + 2 * (Hp - 2);
    const long long total = (long long)n * per_img * row_pieces;
    for (long long id = blockIdx.x * 256ll + threadIdx.x; id < total; id += 256ll * gridDim.x) {
        const int piece = int(id % row_pieces);
        const long long bp = id / row_pieces;
        const int k = int(bp % per_img), b = int(bp / per_img);
        int y, x;
        if (k < Wp) { y = 0; x = k; }
        else if (k < 2 * Wp) { y = Hp - 1; x = k - Wp; }
        else { const int j = k - 2 * Wp; y = 1 + (j >> 1); x = (j & 1) ? Wp - 1 : 0; }
        buf[(((size_t)b * Hp + y) * Wp + x) * row_pieces + piece] = u32x4{0u, 0u, 0u, 0u};
    }
}

// FPN merge (resnet_fpn.py:109-115) of the fp32 mode: out = lateral + bilinear_x2(src, align_corners=True), written into the
// interior of a zero-bordered tensor.  lateral [n, Hp, Wp, ldl] fp32, src [n, Hsp, Wsp, lds] fp32 (half resolution,
// both zero-bordered), out fp32 rows [n, Hp, Wp, Cp]; channels c < C in groups of four (C % 4 == 0).  The f16x3 mode has this
// arithmetic, term for term, in the lateral convolution's epilogue (gemm_planes.hip EPI_CONV_UP).
__global__ __launch_bounds__(256) void upsample_add_f32_kernel(const float* __restrict__ lat, int ldl, const float* __restrict__ src, int lds,
                                                               float* __restrict__ out, int Cp, int C, int n, int Hp, int Wp) {
    const int H = Hp - 2, W = Wp - 2, Hs = H / 2, Ws = W / 2, Hsp = Hs + 2, Wsp = Ws + 2;
    const int groups = Cp / 4;   // the channel padding (C <= c < Cp) is written as zeros
    // torch's area_pixel_compute_scale for align_corners: (in - 1) / (out - 1), 0 for a single output pixel
    const float sh = H > 1 ? float(Hs - 1) / float(H - 1) : 0.f, sw = W > 1 ? float(Ws - 1) / float(W - 1) : 0.f;
    const long long total = (long long)n * H * W * groups;
    for (long long id = blockIdx.x * 256ll + threadIdx.x; id < total; id += 256ll * gridDim.x) {
        const int gidx = int(id % groups);
        const long long pix = id / groups;
        const int x = int(pix % W), y = int((pix / W) % H), b = int(pix / ((long long)W * H));
        const float ry = sh * float(y), rx = sw * float(x);
        const int y0 = int(ry), x0 = int(rx);
        const int y1 = y0 + (y0 < Hs - 1 ? 1 : 0), x1 = x0 + (x0 < Ws - 1 ? 1 : 0);
        const float ly1 = ry - float(y0), lx1 = rx - float(x0), ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        const int c = 4 * gidx;
        auto at = [&](int yy, int xx) {
            return *reinterpret_cast<const f32x4*>(src + (((size_t)b * Hsp + yy + 1) * Wsp + xx + 1) * lds + c);
        };
        const size_t prow = ((size_t)b * Hp + y + 1) * Wp + x + 1;
        float* of = out + prow * Cp + c;
        if (c >= C) {
            *reinterpret_cast<f32x4*>(of) = f32x4{0.f, 0.f, 0.f, 0.f};
            continue;
        }
        const f32x4 v00 = at(y0, x0), v01 = at(y0, x1), v10 = at(y1, x0), v11 = at(y1, x1);
        const f32x4 l = *reinterpret_cast<const f32x4*>(lat + prow * ldl + c);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // upsample_bilinear2d: h0lambda * (w0lambda * v00 + w1lambda * v01) + h1lambda * (w0lambda * v10 + w1lambda * v11)
            const float up = ly0 * (lx0 * v00[e] + lx1 * v01[e]) + ly1 * (lx0 * v10[e] + lx1 * v11[e]);
            v[e] = l[e] + up;
        }
        *reinterpret_cast<f32x4*>(of) = v;
    }
}

struct Plan {
    int n, H, W;
    int Hp[4], Wp[4];           // zero-bordered grids at 1/2, 1/4, 1/8 (index 1..3)
    size_t rows[4];
    ConvGrid grid(int level) const { return ConvGrid{n, Hp[level], Wp[level]}; }
};
inline Plan make_plan(int n, int H, int W) {
    Plan p = {};
    p.n = n; p.H = H; p.W = W;
    for (int k = 1; k <= 3; ++k) {
        p.Hp[k] = (H >> k) + 2;
        p.Wp[k] = (W >> k) + 2;
        p.rows[k] = size_t(n) * p.Hp[k] * p.Wp[k];
    }
    return p;
}

// workspace buffers, in floats-per-row (= bytes / 4 of a planes row or an fp32 row)
enum Buf { G0, P1A, P1B, P1C, F1, T1A, T1B, G2, D2, P2A, P2B, P2C, F2, T2A, T2B, X2O, G3, D3, P3A, P3B, P3C, NBUF };
struct BufSpec { int level, pitch; };
constexpr BufSpec kBufs[NBUF] = {
    {1, 64},  {1, 128}, {1, 128}, {1, 128}, {1, 224}, {1, 224}, {1, 224},
    {2, 1152}, {2, 128}, {2, 224}, {2, 224}, {2, 224}, {2, 256}, {2, 256}, {2, 256}, {2, 224},
    {3, 2016}, {3, 224}, {3, 256}, {3, 256}, {3, 256}};
// POPE_PREC_F16: the same buffers hold plain f16 rows (value * 8), channels padded to the 64-column chunk (196 -> 256); pitches
// in column PAIRS, none wider than the planes row it replaces.  The fp32 maps (F1, F2: unused here; X2O) keep theirs.
constexpr int kPitchF16[NBUF] = {64, 64, 64, 64, 224, 128, 128, 576, 64, 128, 128, 128, 256, 128, 128, 224, 1152, 128, 128, 128, 128};
constexpr bool f16_rows_fit() {
    for (int b = 0; b < NBUF; ++b)
        if (kPitchF16[b] > kBufs[b].pitch) return false;
    return true;
}
static_assert(f16_rows_fit(), "the f16 mode lives in the planes mode's workspace");

// the router of a precision's GEMMs: gemm_f32.hip for POPE_PREC_F32_MFMA, gemm_planes.hip for planes and plain f16
inline int launch_gemm(int precision, const GemmParams& g, hipStream_t stream) {
    return precision == POPE_PREC_F32_MFMA ? pope_launch_gemm_nt_f32(g, stream) : pope_launch_gemm_planes(g, stream);
}

}  // namespace

int pope_conv_zero_border(void* buf, const ConvGrid& grid, int pitch, hipStream_t stream) {
    const long long total = (long long)grid.n * (2 * grid.Wp + 2 * (grid.Hp - 2)) * (pitch / 4);
    hipLaunchKernelGGL(zero_border_kernel, dim3(pope_grid_for(total)), dim3(256), 0, stream, static_cast<u32x4*>(buf), grid.n, grid.Hp,
                       grid.Wp, pitch / 4);
    return pope_check_launch();
}

int pope_conv3_layer(int precision, const void* a, int a_pitch, const void* w, const float* bias, int N, const ConvGrid& grid, void* out_pl,
                     float* out_f32, int out_pitch, float slope, const void* res, int res_pitch, bool zero_border, unsigned* range_flag,
                     hipStream_t stream) {
    const GemmParams g = pope_conv_gemm_params(precision, a, a_pitch, w, bias, 0, N, grid, true, out_pl, out_f32, out_pitch, slope, res,
                                               res_pitch, range_flag);
    POPE_TRY(launch_gemm(precision, g, stream));
    return zero_border ? pope_conv_zero_border(out_pl ? out_pl : out_f32, grid, out_pitch, stream) : POPE_OK;
}

int pope_conv_s2_layer(int precision, const void* x, int x_pitch, const ConvGrid& in, int taps, const void* w, const float* bias, int N,
                       void* gathered, void* out, int out_pitch, float slope, bool zero_border, unsigned* range_flag, hipStream_t stream) {
    const ConvGrid og = in.half();
    // straight from x's planes (gemm_plain.hip, CONV = 2) where the call fills a round of the CUs; else the taps are gathered: the same bits
    const GemmParams s2 = pope_conv_s2_params(x, x_pitch, in, taps, w, bias, N, out, out_pitch, slope, range_flag);
    if (precision == POPE_PREC_F16X3 && pope_wide_conv_s2_supported(s2)) {
        POPE_TRY(pope_launch_gemm_planes(s2, stream));
    } else {
        const int cch = x_pitch / 32;
        const long long total = (long long)og.rows() * taps * cch * 8;
        hipLaunchKernelGGL(gather_s2_kernel, dim3(pope_grid_for(total)), dim3(256), 0, stream, static_cast<const u32x4*>(x),
                           static_cast<u32x4*>(gathered), in.n, in.Hp, in.Wp, cch, taps);
        POPE_TRY(pope_check_launch());
        const GemmParams g = pope_conv_gemm_params(precision, gathered, taps * x_pitch, w, bias, taps * x_pitch, N, og, false, out, nullptr,
                                                   out_pitch, slope, nullptr, 0, range_flag);
        POPE_TRY(launch_gemm(precision, g, stream));
    }
    return zero_border ? pope_conv_zero_border(out, og, out_pitch, stream) : POPE_OK;
}

int pope_conv1_up_layer(int precision, const void* a, int a_pitch, const void* w, const float* bias, int N, const ConvGrid& grid,
                        const float* up_src, int up_lds, void* out_pl, int out_pitch, float slope, unsigned* range_flag, hipStream_t stream) {
    GemmParams g = pope_conv_gemm_params(precision, a, a_pitch, w, bias, a_pitch, N, grid, false, out_pl, nullptr, out_pitch, slope,
                                         nullptr, 0, range_flag);
    pope_conv_up_params(g, up_src, up_lds, grid);
    POPE_TRY(pope_launch_gemm_planes(g, stream));
    return pope_conv_zero_border(out_pl, grid, out_pitch, stream);
}

int pope_conv_stem_layer(int precision, const float* img, int n, int H, int W, void* gathered, const void* w, const float* bias, int N,
                         void* out, int out_pitch, float slope, unsigned* range_flag, hipStream_t stream) {
    const ConvGrid grid = {n, H / 2 + 2, W / 2 + 2};
    const long long total = (long long)grid.rows() * 8;
    if (precision == POPE_PREC_F32_MFMA)
        hipLaunchKernelGGL(stem_gather_kernel<STEM_F32>, dim3(pope_grid_for(total)), dim3(256), 0, stream, img, static_cast<_Float16*>(gathered), n,
                           H, W, range_flag);
    else if (precision == POPE_PREC_F16)
        hipLaunchKernelGGL(stem_gather_kernel<STEM_F16>, dim3(pope_grid_for(total)), dim3(256), 0, stream, img, static_cast<_Float16*>(gathered), n,
                           H, W, range_flag);
    else
        hipLaunchKernelGGL(stem_gather_kernel<STEM_PLANES>, dim3(pope_grid_for(total)), dim3(256), 0, stream, img, static_cast<_Float16*>(gathered), n,
                           H, W, range_flag);
    POPE_TRY(pope_check_launch());
    const GemmParams g = pope_conv_gemm_params(precision, gathered, 64, w, bias, 64, N, grid, false, out, nullptr, out_pitch, slope, nullptr, 0,
                                               range_flag);
    POPE_TRY(launch_gemm(precision, g, stream));
    return pope_conv_zero_border(out, grid, out_pitch, stream);
}

size_t pope_resnetfpn_workspace(int n, int H, int W) {
    const Plan p = make_plan(n, H, W);
    size_t total = 0;
    for (int b = 0; b < NBUF; ++b) total += pope_align256(p.rows[kBufs[b].level] * kBufs[b].pitch * 4);
    return total;
}

int pope_launch_resnetfpn(const ResnetFpnParams& q, hipStream_t stream) {
    if (!q.img || !q.out_c || !q.out_f || !q.ws || q.n <= 0 || q.H < 16 || q.W < 16 || (q.H & 7) || (q.W & 7)) return POPE_ERR_ARG;
    const bool f32 = q.precision == POPE_PREC_F32_MFMA;
    const bool f16 = q.precision == POPE_PREC_F16;
    if (!f32 && !f16 && q.precision != POPE_PREC_F16X3) return POPE_ERR_ARG;
    for (int i = 0; i < 22; ++i)
        if (!(f32 ? static_cast<const void*>(q.wf[i]) : q.w[i])) return POPE_ERR_ARG;
    const Plan p = make_plan(q.n, q.H, q.W);
    for (int b = 0; b < NBUF; ++b)   // 32-bit buffer offsets everywhere: the caller splits larger batches
        if (p.rows[kBufs[b].level] * kBufs[b].pitch * 4ull >= (1ull << 32)) return POPE_ERR_ARG;
    if (q.ws_bytes < pope_resnetfpn_workspace(q.n, q.H, q.W)) return POPE_ERR_WORKSPACE;
    char* base = static_cast<char*>(q.ws);
    char* buf[NBUF];
    for (int b = 0; b < NBUF; ++b) {
        buf[b] = base;
        base += pope_align256(p.rows[kBufs[b].level] * kBufs[b].pitch * 4);
    }
    // Borders and the channel padding (196 -> 224) must read as zeros.  Nothing is cleared wholesale: every planes
    // buffer is written in full by its producer — the GEMM epilogue zero-fills the padding columns, the gathers and
    // the FPN merge write zeros where they have no source — and has its border rows zeroed right after.

    int rc;
    // POPE_PREC_F32_MFMA (the range guard's re-run): the same buffers hold fp32 rows of the same pitch, every GEMM runs on
    // gemm_f32.hip (EPI_CONV, implicit 3x3 loader).  Its epilogue writes only the N real channels, so the channel padding
    // (196 -> 224) is cleared once up front; speed is not a goal of this path.
    if (f32 && hipMemsetAsync(q.ws, 0, pope_resnetfpn_workspace(q.n, q.H, q.W), stream) != hipSuccess) return POPE_ERR_LAUNCH;
    const int prec = q.precision;
    unsigned* const flag = q.range_flag;
    auto wt = [&](int wi) -> const void* { return f32 ? static_cast<const void*>(q.wf[wi]) : q.w[wi]; };
    auto pitch = [&](int b) -> int { return f16 ? kPitchF16[b] : kBufs[b].pitch; };
    // the layer forms of conv_layer.h on the workspace buffers (one GEMM each, border rows zeroed after a planes output)
    auto conv3 = [&](Buf in, int wi, int N, int level, Buf out, float slope, int res /* Buf or -1 */) -> int {
        return pope_conv3_layer(prec, buf[in], pitch(in), wt(wi), q.b[wi], N, p.grid(level), buf[out], nullptr, pitch(out), slope,
                                res >= 0 ? buf[res] : nullptr, res >= 0 ? pitch(res) : 0, true, flag, stream);
    };
    // 3 x 3 or 1 x 1 -> an fp32 map (the FPN's outputs): no border pass
    auto conv3_f32 = [&](Buf in, int wi, int N, int level, float* out, int out_pitch) -> int {
        return pope_conv3_layer(prec, buf[in], pitch(in), wt(wi), q.b[wi], N, p.grid(level), nullptr, out, out_pitch, 1.f, nullptr, 0,
                                false, flag, stream);
    };
    auto conv1_f32 = [&](Buf in, int K, int wi, int N, int level, float* out, int out_pitch) -> int {
        return launch_gemm(prec, pope_conv_gemm_params(prec, buf[in], pitch(in), wt(wi), q.b[wi], K, N, p.grid(level), false, nullptr, out,
                                                       out_pitch, 1.f, nullptr, 0, flag), stream);
    };
    // BasicBlock (resnet_fpn.py:15-40) with stride 1: x -> t -> y; returns with the block output in `y`
    auto block_s1 = [&](Buf x, Buf t, Buf y, int w0, int N, int level) -> int {
        int r = conv3(x, w0, N, level, t, 0.f, -1);
        return r ? r : conv3(t, w0 + 1, N, level, y, 0.f, x);
    };
    // BasicBlock with stride 2: x (level L) -> t (3 x 3 stride 2, border rows zeroed); shortcut 1 x 1 stride 2 -> s;
    // y = relu(conv2(t) + s).  g9 / g1 hold the gathered taps where the implicit route does not serve the call.
    auto block_s2 = [&](Buf x, int level_in, Buf g9, Buf g1, Buf t, Buf s, Buf y, int w0, int N) -> int {
        const int lo = level_in + 1;
        int r = pope_conv_s2_layer(prec, buf[x], pitch(x), p.grid(level_in), 9, wt(w0), q.b[w0], N, buf[g9], buf[t], pitch(t), 0.f,
                                   true, flag, stream);
        if (r) return r;
        r = pope_conv_s2_layer(prec, buf[x], pitch(x), p.grid(level_in), 1, wt(w0 + 2), q.b[w0 + 2], N, buf[g1], buf[s], pitch(s),
                               1.f, false, flag, stream);
        return r ? r : conv3(t, w0 + 1, N, lo, y, 0.f, s);
    };
    // the fp32 mode's FPN merge: lateral map + bilinear x2 of the coarser map -> fp32 rows, border rows zeroed
    auto upsample_add = [&](Buf lat, const float* src, int lds, Buf out, int C, int level) -> int {
        const int pitch = kBufs[out].pitch;
        const long long total = (long long)q.n * (p.Hp[level] - 2) * (p.Wp[level] - 2) * (pitch / 4);
        hipLaunchKernelGGL(upsample_add_f32_kernel, dim3(pope_grid_for(total)), dim3(256), 0, stream, reinterpret_cast<const float*>(buf[lat]),
                           kBufs[lat].pitch, src, lds, reinterpret_cast<float*>(buf[out]), pitch, C, q.n, p.Hp[level], p.Wp[level]);
        int r = pope_check_launch();
        return r ? r : pope_conv_zero_border(buf[out], p.grid(level), pitch, stream);
    };

    // stem (resnet_fpn.py:60-62,101)
    if ((rc = pope_conv_stem_layer(prec, q.img, q.n, q.H, q.W, buf[G0], wt(0), q.b[0], 128, buf[P1A], pitch(P1A), 0.f, flag, stream))) return rc;
    // layer1 (1/2), layer2 (1/4), layer3 (1/8)
    if ((rc = block_s1(P1A, P1B, P1C, 1, 128, 1))) return rc;
    if ((rc = block_s1(P1C, P1A, P1B, 3, 128, 1))) return rc;             // x1 = P1B
    if ((rc = block_s2(P1B, 1, G2, D2, P2A, P2C, P2B, 5, 196))) return rc;
    if ((rc = block_s1(P2B, P2A, P2C, 8, 196, 2))) return rc;             // x2 = P2C
    if ((rc = block_s2(P2C, 2, G3, D3, P3A, P3C, P3B, 10, 256))) return rc;
    if ((rc = block_s1(P3B, P3A, P3C, 13, 256, 3))) return rc;            // x3 = P3C
    // FPN (resnet_fpn.py:107-117)
    if ((rc = conv1_f32(P3C, pitch(P3C), 15, 256, 3, q.out_c, 256))) return rc;                                                   // x3_out
    // f16x3: the lateral 1 x 1 convolution's epilogue adds the bilinear x2 sample of the coarser map and writes the merged planes
    // (round 4: the fp32 lateral map and the upsample_add pass are gone — 1.9 GB of the call's fabric traffic at 48 images); the
    // fp32 mode keeps the two-step form; the f16 mode runs the plain instantiation of the same epilogue
    if (!f32) {
        if ((rc = pope_conv1_up_layer(prec, buf[P2C], pitch(P2C), q.w[16], q.b[16], 256, p.grid(2), q.out_c, 256, buf[T2A], pitch(T2A), 1.f, flag,
                                      stream)))
            return rc;
    } else {
        if ((rc = conv1_f32(P2C, 224, 16, 256, 2, reinterpret_cast<float*>(buf[F2]), 256))) return rc;
        if ((rc = upsample_add(F2, q.out_c, 256, T2A, 256, 2))) return rc;
    }
    if ((rc = conv3(T2A, 17, 256, 2, T2B, 0.01f, -1))) return rc;
    if ((rc = conv3_f32(T2B, 18, 196, 2, reinterpret_cast<float*>(buf[X2O]), 224))) return rc;
    if (!f32) {
        if ((rc = pope_conv1_up_layer(prec, buf[P1B], pitch(P1B), q.w[19], q.b[19], 196, p.grid(1), reinterpret_cast<const float*>(buf[X2O]), 224,
                                      buf[T1A], pitch(T1A), 1.f, flag, stream)))
            return rc;
    } else {
        if ((rc = conv1_f32(P1B, 128, 19, 196, 1, reinterpret_cast<float*>(buf[F1]), 224))) return rc;
        if ((rc = upsample_add(F1, reinterpret_cast<const float*>(buf[X2O]), 224, T1A, 196, 1))) return rc;
    }
    if ((rc = conv3(T1A, 20, 196, 1, T1B, 0.01f, -1))) return rc;
    return conv3_f32(T1B, 21, 128, 1, q.out_f, 128);                                                                       // x1_out
}

// ---- pope_conv_layer_f32: one of the layer forms above on the caller's buffers ----------------------------------------------------
namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// every kernel addresses its buffers through 32-bit byte offsets, a tile of rows past the end included
inline bool fits32(size_t rows, size_t pitch) { return (rows + 256) * pitch * 4 < (size_t(1) << 32) - 512; }

}  // namespace

size_t pope_conv_layer_scratch(int form, int n, int H, int W, int cch, int taps) {
    if (n <= 0 || H <= 0 || W <= 0 || cch < 0 || taps < 0) return 0;
    const size_t out_rows = size_t(n) * (H / 2 + 2) * (W / 2 + 2);
    if (form == POPE_CONV_S2) return out_rows * taps * cch * 128;   // the gathered taps
    if (form == POPE_CONV_STEM) return out_rows * 256;              // 49 taps in two chunks
    return 0;
}

int pope_conv_layer_check(const pope_conv_layer_args& a) {
    const int form = a.form, prec = a.precision;
    if (form != POPE_CONV3 && form != POPE_CONV_S2 && form != POPE_CONV1_UP && form != POPE_CONV_STEM) return POPE_ERR_ARG;
    if (prec != POPE_PREC_F16X3) {
        if (prec == POPE_PREC_F32_MFMA ? form != POPE_CONV3 && form != POPE_CONV_STEM : prec != POPE_PREC_F16 || form != POPE_CONV3)
            return POPE_ERR_ARG;
    }
    const bool f32 = prec == POPE_PREC_F32_MFMA;
    if (a.n < 1 || a.H < 1 || a.W < 1 || a.N < 4 || (a.N & 3) || a.N > 256) return POPE_ERR_ARG;
    if (form != POPE_CONV3 && ((a.H | a.W) & 1)) return POPE_ERR_ARG;   // stride 2 halves the grid; CONV1_UP doubles one (and needs Wp >= 4)
    const bool stem = form == POPE_CONV_STEM, s2 = form == POPE_CONV_S2;
    if (stem ? a.cch != 0 || a.taps != 0 : a.cch < 1) return POPE_ERR_ARG;
    if (s2 ? a.taps != 9 && a.taps != 1 : a.taps != 0) return POPE_ERR_ARG;
    const int taps = form == POPE_CONV3 ? 9 : s2 ? a.taps : 1;
    if (!stem && taps * a.cch < 2) return POPE_ERR_ARG;                  // the routers' minimum: two K-steps
    if (!a.a || !a.w || !aligned16(a.a) || !aligned16(a.w) || (a.bias && !aligned16(a.bias))) return POPE_ERR_ARG;
    const ConvGrid in = {a.n, a.H + 2, a.W + 2};
    const ConvGrid out = form == POPE_CONV3 || form == POPE_CONV1_UP ? in : in.half();
    const size_t pitch_in = stem ? 64 : size_t(32) * a.cch;
    if (!stem && (a.a_rows < in.rows() || !fits32(in.rows(), pitch_in))) return POPE_ERR_ARG;
    if (stem && size_t(a.n) * a.H * a.W * 4 >= (size_t(1) << 32)) return POPE_ERR_ARG;
    if (!fits32(256, size_t(taps) * pitch_in)) return POPE_ERR_ARG;      // the weight rows
    // outputs
    if ((a.out_planes == nullptr) == (a.out_f32 == nullptr)) return POPE_ERR_ARG;
    if (a.out_planes) {
        if (f32 || prec == POPE_PREC_F16 || a.ldc != ((a.N + 31) & ~31) || !aligned16(a.out_planes)) return POPE_ERR_ARG;
    } else {
        if (s2 || form == POPE_CONV1_UP || (stem && !f32)) return POPE_ERR_ARG;   // planes-only forms
        if (a.ldc < a.N || (a.ldc & 3) || !aligned16(a.out_f32)) return POPE_ERR_ARG;
    }
    if (!a.zero_border && (stem || (a.out_planes && !s2))) return POPE_ERR_ARG;   // the next layer reads the border as its padding
    if (!fits32(out.rows(), size_t(a.ldc))) return POPE_ERR_ARG;
    // the shortcut and the FPN source
    if (a.res) {
        if (form != POPE_CONV3 || prec == POPE_PREC_F16 || a.ldres < a.N || (a.ldres & (f32 ? 3 : 31)) || !aligned16(a.res)) return POPE_ERR_ARG;
        if (!fits32(out.rows(), size_t(a.ldres))) return POPE_ERR_ARG;
    }
    if (form == POPE_CONV1_UP) {
        if (!a.up_src || a.up_lds < a.N || (a.up_lds & 3) || !aligned16(a.up_src) || in.Wp < 4) return POPE_ERR_ARG;
        if (!fits32(in.half().rows(), size_t(a.up_lds))) return POPE_ERR_ARG;
    } else if (a.up_src) {
        return POPE_ERR_ARG;
    }
    if (s2 || stem) {
        if (!a.scratch || !aligned16(a.scratch) || !fits32(out.rows(), size_t(taps) * pitch_in)) return POPE_ERR_ARG;
        if (a.scratch_bytes < pope_conv_layer_scratch(form, a.n, a.H, a.W, a.cch, a.taps)) return POPE_ERR_WORKSPACE;
    }
    return POPE_OK;
}

// The argument contract of pope_conv_layer_f16 (pope_hip.h has it in words): every form on plain f16 rows.  Pitches (ldc of
// out_planes, ldres) count column PAIRS, i.e. 4-byte units like every other pitch here; a chunk is 64 columns.
int pope_conv_layer_f16_check(const pope_conv_layer_args& a) {
    const int form = a.form;
    if (form != POPE_CONV3 && form != POPE_CONV_S2 && form != POPE_CONV1_UP && form != POPE_CONV_STEM) return POPE_ERR_ARG;
    if (a.precision != POPE_PREC_F16) return POPE_ERR_ARG;
    if (a.n < 1 || a.H < 1 || a.W < 1 || a.N < 4 || (a.N & 3) || a.N > 256) return POPE_ERR_ARG;
    if (form != POPE_CONV3 && ((a.H | a.W) & 1)) return POPE_ERR_ARG;
    const bool stem = form == POPE_CONV_STEM, s2 = form == POPE_CONV_S2;
    if (stem ? a.cch != 0 || a.taps != 0 : a.cch < 1) return POPE_ERR_ARG;
    if (s2 ? a.taps != 9 && a.taps != 1 : a.taps != 0) return POPE_ERR_ARG;
    const int taps = form == POPE_CONV3 ? 9 : s2 ? a.taps : 1;
    if (!stem && taps * a.cch < 2) return POPE_ERR_ARG;                  // the tile kernel's minimum: two K-steps
    if (!a.a || !a.w || !aligned16(a.a) || !aligned16(a.w) || (a.bias && !aligned16(a.bias))) return POPE_ERR_ARG;
    const ConvGrid in = {a.n, a.H + 2, a.W + 2};
    const ConvGrid out = form == POPE_CONV3 || form == POPE_CONV1_UP ? in : in.half();
    const size_t pitch_in = stem ? 64 : size_t(32) * a.cch;
    if (!stem && (a.a_rows < in.rows() || !fits32(in.rows(), pitch_in))) return POPE_ERR_ARG;
    if (stem && size_t(a.n) * a.H * a.W * 4 >= (size_t(1) << 32)) return POPE_ERR_ARG;
    if (!fits32(256, size_t(taps) * pitch_in)) return POPE_ERR_ARG;      // the weight rows
    if ((a.out_planes == nullptr) == (a.out_f32 == nullptr)) return POPE_ERR_ARG;
    if (a.out_planes) {
        if (a.ldc != ((a.N + 63) & ~63) / 2 || !aligned16(a.out_planes)) return POPE_ERR_ARG;
    } else {
        if (form != POPE_CONV3) return POPE_ERR_ARG;                     // the other forms feed the next layer
        if (a.ldc < a.N || (a.ldc & 3) || !aligned16(a.out_f32)) return POPE_ERR_ARG;
    }
    if (!a.zero_border && (stem || (a.out_planes && !s2))) return POPE_ERR_ARG;   // the next layer reads the border as its padding
    if (!fits32(out.rows(), size_t(a.ldc))) return POPE_ERR_ARG;
    if (a.res) {
        if (form != POPE_CONV3 || 2 * a.ldres < a.N || (a.ldres & 31) || !aligned16(a.res)) return POPE_ERR_ARG;
        if (!fits32(out.rows(), size_t(a.ldres))) return POPE_ERR_ARG;
    }
    if (form == POPE_CONV1_UP) {
        if (!a.up_src || a.up_lds < a.N || (a.up_lds & 3) || !aligned16(a.up_src) || in.Wp < 4) return POPE_ERR_ARG;
        if (!fits32(in.half().rows(), size_t(a.up_lds))) return POPE_ERR_ARG;
    } else if (a.up_src) {
        return POPE_ERR_ARG;
    }
    if (s2 || stem) {
        if (!a.scratch || !aligned16(a.scratch) || !fits32(out.rows(), size_t(taps) * pitch_in)) return POPE_ERR_ARG;
        if (a.scratch_bytes < pope_conv_layer_scratch(form, a.n, a.H, a.W, a.cch, a.taps)) return POPE_ERR_WORKSPACE;
    }
    return POPE_OK;
}

int pope_launch_conv_layer(const pope_conv_layer_args& a, bool f16_entry, hipStream_t stream) {
    POPE_TRY(f16_entry ? pope_conv_layer_f16_check(a) : pope_conv_layer_check(a));
    const ConvGrid in = {a.n, a.H + 2, a.W + 2};
    const int pitch = 32 * a.cch;
    switch (a.form) {
        case POPE_CONV3:
            return pope_conv3_layer(a.precision, a.a, pitch, a.w, a.bias, a.N, in, a.out_planes, a.out_f32, a.ldc, a.slope, a.res, a.ldres,
                                    a.zero_border != 0, a.range_flag, stream);
        case POPE_CONV_S2:
            return pope_conv_s2_layer(a.precision, a.a, pitch, in, a.taps, a.w, a.bias, a.N, a.scratch, a.out_planes, a.ldc, a.slope,
                                      a.zero_border != 0, a.range_flag, stream);
        case POPE_CONV1_UP:
            return pope_conv1_up_layer(a.precision, a.a, pitch, a.w, a.bias, a.N, in, a.up_src, a.up_lds, a.out_planes, a.ldc, a.slope, a.range_flag, stream);
        case POPE_CONV_STEM:
            return pope_conv_stem_layer(a.precision, static_cast<const float*>(a.a), a.n, a.H, a.W, a.scratch, a.w, a.bias, a.N,
                                        a.out_planes ? a.out_planes : static_cast<void*>(a.out_f32), a.ldc, a.slope, a.range_flag, stream);
    }
    return POPE_ERR_ARG;
}
