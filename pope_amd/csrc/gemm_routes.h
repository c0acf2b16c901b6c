// Routes of pope_launch_gemm_planes (gemm_planes.hip) that live in the other GEMM files.  Included by gemm_*.hip only: every
// other file goes through pope_launch_gemm_planes.  A launcher may be called only when its predicate holds; the router does that.
#pragma once
#include "kernels.h"

// plain-f16 long-K mainloop (gemm_plain.hip: 256-row tiles, LDS-direct staging) for the GemmParams::plain shapes it serves
bool pope_plain256_supported(const GemmParams& g);
int pope_launch_plain256(const GemmParams& g, hipStream_t stream);
// the same mainloop on f16x3 planes -> planes (BIAS, BIAS_GELU) at large M
bool pope_wide_x3_supported(const GemmParams& g);
int pope_launch_wide_x3(const GemmParams& g, hipStream_t stream);
// ... on the implicit 3 x 3 convolutions (EPI_CONV, conv_cch > 0) at large M
bool pope_wide_conv_supported(const GemmParams& g);
int pope_launch_wide_conv(const GemmParams& g, hipStream_t stream);
// ... on the stride-2 convolutions without the gathered tap tensor (predicate pope_wide_conv_s2_supported: kernels.h)
int pope_launch_wide_conv_s2(const GemmParams& g, hipStream_t stream);
// the 192 x 384 LDS-direct tile stream of gemm_rowln.hip for planes -> planes Linears whose width is a multiple of 384
bool pope_stream384_supported(const GemmParams& g);
int pope_launch_stream384(const GemmParams& g, hipStream_t stream);
