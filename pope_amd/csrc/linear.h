// The GemmParams of a dense Linear, C = epi(A . W^T + bias [, gamma, res]), built in one place (host only).  Everything that
// is not a plain Linear keeps its own builder: the convolutions (conv_layer.h), EPI_SIM (match.hip), EPI_SAM_QKV
// (sam_attention.hip) and the patch gather EPI_POSB.
#pragma once
#include "kernels.h"

enum LinearForm {
    LINEAR_F32,      // fp32 operands (GemmParams::A / W): gemm_f32.hip, gemm_f16x3.hip
    LINEAR_PLANES,   // f16x3 planes (GemmParams::a_pl / w_pl): gemm_planes.hip, gemm_rowln.hip
    LINEAR_PLAIN,    // plain f16 row-major operands (GemmParams::plain): gemm_planes.hip
};

// a [M, K], w [N, K] (torch Linear layout), M / N / K in REAL columns; the output is fp32 `C` or the packed `c_packed` (planes, or
// f16 rows in the plain form).  Fields of one epilogue or one site (sam_dim / sam_qscale, ln_*, act_slope, nbatch) are the
// caller's to set on the result.
inline GemmParams pope_linear_params(LinearForm form, const void* a, const void* w, const float* bias, float* C, void* c_packed,
                                     int M, int N, int K, int epilogue, const float* gamma = nullptr, const float* res = nullptr,
                                     int res_mod = 0, unsigned* range_flag = nullptr) {
    GemmParams g = {};
    if (form == LINEAR_F32) {
        g.A = static_cast<const float*>(a); g.W = static_cast<const float*>(w);
    } else {
        g.a_pl = a; g.w_pl = w;
    }
    g.bias = bias; g.C = C; g.c_pl = c_packed;
    g.plain = form == LINEAR_PLAIN;
    // dense rows: the pitch of A and W is K.  The plain form counts K, lda, ldw and a packed output's ldc in column PAIRS
    // (kernels.h GemmParams::plain) — a real-column count there is silently wrong
    const int pair = g.plain ? 2 : 1;
    g.M = M; g.N = N; g.K = K / pair;
    g.lda = g.ldw = g.K;
    // SwiGLU reads N = 2 hidden columns and writes [M, N / 2]: ldc is the pitch of the HIDDEN rows (kernels.h EPI_BIAS_SWIGLU)
    const int out_cols = epilogue == EPI_BIAS_SWIGLU ? N / 2 : N;
    g.ldc = g.plain && c_packed ? out_cols / 2 : out_cols;
    g.epilogue = epilogue;
    g.gamma = gamma; g.res = res; g.res_mod = res_mod;
    g.ldres = N;   // the residual (or the [res_mod, N] table) is as wide as the output
    g.range_flag = range_flag;
    // the bit a packed-operand GEMM's packed output reports under: FC1's producers (GELU, SwiGLU) have their own; the fp32 form
    // writes no packed output (gemm_f16x3.hip checks its inputs under POPE_RANGE_INPUT)
    if (form != LINEAR_F32) g.range_bit = epilogue == EPI_BIAS_GELU || epilogue == EPI_BIAS_SWIGLU ? POPE_RANGE_GELU : POPE_RANGE_QKV;
    return g;
}

// The residual GEMM with the following LayerNorm fused (gemm_rowln.hip, N = 384): x = res + gamma * (a . w^T + bias) -> x,
// LayerNorm(x; ln_w, ln_b) -> ln_planes or ln_f32 (exactly one).  The LayerNorm reports under POPE_RANGE_LAYERNORM: no range_bit.
inline GemmParams pope_linear_rowln_params(const void* a_planes, const void* w_planes, int M, int N, int K, const float* bias,
                                           const float* gamma, const float* res, int res_mod, float* x, const float* ln_w,
                                           const float* ln_b, float eps, void* ln_planes, float* ln_f32, unsigned* range_flag) {
    GemmParams g = pope_linear_params(LINEAR_PLANES, a_planes, w_planes, bias, x, nullptr, M, N, K, EPI_BIAS_LS_RES, gamma, res,
                                      res_mod, range_flag);
    g.range_bit = 0;
    g.ln_w = ln_w; g.ln_b = ln_b; g.ln_eps = eps; g.ln_planes = ln_planes; g.ln_f32 = ln_f32;
    return g;
}
