// The GemmParams of the convolution forms of the GEMM routers, built in one place (host only), and the one-layer launch
// sequences of conv.hip.  Used by the ResNet-FPN forward (conv.hip), by the SAM neck (sam.hip) and by the test entry
// pope_conv_layer_f32 (capi.hip): what a test drives through the entry is what the models run.
#pragma once
#include "kernels.h"

// A zero-bordered NHWC pixel-row tensor [n, Hp, Wp, pitch]: one pixel = one row of `pitch` floats-worth (pitch * 4 bytes:
// planes of `pitch` columns, fp32 rows of `pitch` columns, or plain f16 rows of 2 * pitch columns).
struct ConvGrid {
    int n, Hp, Wp;
    size_t rows() const { return size_t(n) * Hp * Wp; }
    ConvGrid half() const { return ConvGrid{n, (Hp - 2) / 2 + 2, (Wp - 2) / 2 + 2}; }   // the grid of a stride-2 layer's output
};

// One GEMM over the pixel rows of `grid`: out[rows, N] = act(A . W^T + bias [+ res]) with EPI_CONV.
//   conv3: the implicit 3 x 3 stride-1 convolution (K = 9 * a_pitch; output row R is pixel R + Wp + 1, so C and res start there
//          and M leaves the last 2 Wp + 2 rows out); else a plain GEMM over all rows with the caller's K (1 x 1, gathered taps)
//   precision POPE_PREC_F32_MFMA: fp32 operands for pope_launch_gemm_nt_f32 (an `out_pl` then holds fp32 rows of the same pitch);
//   POPE_PREC_F16X3: planes, POPE_PREC_F16: plain f16 rows with a_pitch and K in column PAIRS, both for pope_launch_gemm_planes
inline GemmParams pope_conv_gemm_params(int precision, const void* a, int a_pitch, const void* w, const float* bias, int K, int N,
                                        const ConvGrid& grid, bool conv3, void* out_pl, float* out_f32, int out_pitch, float slope,
                                        const void* res, int res_pitch, unsigned* range_flag) {
    GemmParams g = {};
    const int Wp = grid.Wp;
    const size_t shift = conv3 ? size_t(Wp) + 1 : 0;
    if (conv3) K = 9 * a_pitch;
    g.lda = a_pitch; g.ldw = K; g.ldc = out_pitch;
    g.M = int(grid.rows() - (conv3 ? 2 * size_t(Wp) + 2 : 0)); g.N = N; g.K = K;
    g.epilogue = EPI_CONV;
    g.act_slope = slope;
    g.bias = bias;
    if (precision == POPE_PREC_F32_MFMA) {
        g.A = static_cast<const float*>(a); g.W = static_cast<const float*>(w);
        g.C = (out_pl ? static_cast<float*>(out_pl) : out_f32) + shift * out_pitch;
        if (res) { g.res = static_cast<const float*>(res) + shift * res_pitch; g.ldres = res_pitch; }
        if (conv3) g.conv_wp = Wp;
        return g;
    }
    g.a_pl = a; g.w_pl = w;
    g.plain = precision == POPE_PREC_F16;
    if (out_pl) g.c_pl = static_cast<char*>(out_pl) + shift * out_pitch * 4;
    else g.C = out_f32 + shift * out_pitch;
    if (res) { g.res_pl = static_cast<const char*>(res) + shift * res_pitch * 4; g.ldres_pl = res_pitch; }
    if (conv3) { g.conv_cch = a_pitch / 32; g.conv_wp = Wp; }
    g.range_flag = range_flag; g.range_bit = POPE_RANGE_INPUT;
    g.nbatch = 1;
    return g;
}

// EPI_CONV_UP on a 1 x 1 convolution over `grid`: the bilinear x2 (align_corners) sample of the half-resolution fp32 map
// up_src [n, grid.half(), up_lds] is added before the activation (kernels.h GemmParams::up_src).  grid.Wp >= 4: the epilogue
// walks four rows ahead with one carry.
inline void pope_conv_up_params(GemmParams& g, const float* up_src, int up_lds, const ConvGrid& grid) {
    g.up_src = up_src; g.up_lds = up_lds; g.up_hp = grid.Hp; g.up_wp = grid.Wp; g.up_n = grid.n;
    const int H = g.up_hp - 2, W = g.up_wp - 2, Hs = H / 2, Ws = W / 2;
    g.up_sh = H > 1 ? float(Hs - 1) / float(H - 1) : 0.f;   // torch's area_pixel_compute_scale for align_corners
    g.up_sw = W > 1 ? float(Ws - 1) / float(W - 1) : 0.f;
    g.up_m_hw = unsigned((1ull << 32) / (unsigned long long)(g.up_hp) / (unsigned long long)(g.up_wp));
    g.up_m_w = unsigned((1ull << 32) / (unsigned long long)(g.up_wp));
}

// The stride-2 convolution (taps = 9: 3 x 3 pad 1, taps = 1: the 1 x 1 shortcut) read straight from the zero-bordered planes
// x [in, x_pitch] (gemm_plain.hip CONV = 2) -> planes out [in.half(), out_pitch].  pope_wide_conv_s2_supported decides whether
// the router takes it; where it does not, the caller gathers the taps (conv.hip pope_conv_s2_layer does both).
inline GemmParams pope_conv_s2_params(const void* x, int x_pitch, const ConvGrid& in, int taps, const void* w, const float* bias, int N,
                                      void* out_pl, int out_pitch, float slope, unsigned* range_flag) {
    const ConvGrid out = in.half();
    GemmParams g = {};
    g.a_pl = x; g.w_pl = w; g.bias = bias;
    g.lda = x_pitch; g.ldw = taps * x_pitch; g.ldc = out_pitch;
    g.M = int(out.rows()); g.N = N; g.K = taps * x_pitch;
    g.epilogue = EPI_CONV; g.act_slope = slope; g.c_pl = out_pl;
    g.conv_cch = x_pitch / 32; g.conv_wp = in.Wp;
    g.conv_s2_taps = taps; g.conv_s2_hpi = in.Hp; g.conv_s2_hpo = out.Hp; g.conv_s2_wpo = out.Wp;
    g.conv_s2_in_rows = int(in.rows());
    g.range_flag = range_flag; g.range_bit = POPE_RANGE_INPUT; g.nbatch = 1;
    return g;
}

// ---- one layer each (conv.hip): the launch sequences of pope_launch_resnetfpn, on the caller's buffers -------------------------
// zero the border pixels' rows of [grid, pitch]
int pope_conv_zero_border(void* buf, const ConvGrid& grid, int pitch, hipStream_t stream);
// 3 x 3 stride 1: the implicit GEMM, then (zero_border) the border rows of the output
int pope_conv3_layer(int precision, const void* a, int a_pitch, const void* w, const float* bias, int N, const ConvGrid& grid, void* out_pl,
                     float* out_f32, int out_pitch, float slope, const void* res, int res_pitch, bool zero_border, unsigned* range_flag,
                     hipStream_t stream);
// stride 2 (POPE_PREC_F16X3: planes -> planes; POPE_PREC_F32_MFMA: fp32 rows, POPE_PREC_F16: f16 rows, both always gathered):
// the implicit route where the router serves it, else gather_s2 into `gathered` [in.half(), taps * x_pitch] + a plain GEMM — the
// same bits; then (zero_border) the border rows.  The implicit route leaves `gathered` untouched and the border rows of `out`
// undefined.
int pope_conv_s2_layer(int precision, const void* x, int x_pitch, const ConvGrid& in, int taps, const void* w, const float* bias, int N,
                       void* gathered, void* out, int out_pitch, float slope, bool zero_border, unsigned* range_flag, hipStream_t stream);
// 1 x 1 lateral convolution with the FPN merge in its epilogue (POPE_PREC_F16X3 or POPE_PREC_F16), then the border rows
int pope_conv1_up_layer(int precision, const void* a, int a_pitch, const void* w, const float* bias, int N, const ConvGrid& grid,
                        const float* up_src, int up_lds, void* out_pl, int out_pitch, float slope, unsigned* range_flag, hipStream_t stream);
// 7 x 7 stride-2 pad-3 stem on the gray image [n, H, W]: stem_gather into `gathered` [grid of H/2 x W/2, 64] + the K = 64 GEMM +
// the border rows
int pope_conv_stem_layer(int precision, const float* img, int n, int H, int W, void* gathered, const void* w, const float* bias, int N,
                         void* out, int out_pitch, float slope, unsigned* range_flag, hipStream_t stream);

// The argument contract of pope_conv_layer_f32 (pope_hip.h has it in words; host only: no HIP call) and the call itself
int pope_conv_layer_check(const pope_conv_layer_args& a);
// ... and of pope_conv_layer_f16: POPE_PREC_F16 only, all four forms, out_planes / res as f16 rows with pitches in column pairs
int pope_conv_layer_f16_check(const pope_conv_layer_args& a);
size_t pope_conv_layer_scratch(int form, int n, int H, int W, int cch, int taps);
int pope_launch_conv_layer(const pope_conv_layer_args& a, bool f16_entry, hipStream_t stream);
