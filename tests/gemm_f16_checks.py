"""Operands, fp64 references, bounds and the case table of test_gpu_gemm_f16_routes.py (host only; test_gemm_f16_checks_cpu.py
shows that the comparisons reject the faults a plain-f16 GEMM epilogue is likely to have, on this very data).

pope_linear_f16 (pope_hip.h): A [M, K] f16 = value * 8, W [N, K] f16 = value * 256, fp32 accumulation, then
  BIAS     fp32  lin + bias
  GELU     f16   gelu(lin + bias) * 8                                one rounding
  QKV      f16   (lin + bias) * (col < N / 3 ? 0.125 log2 e : 1)     one rounding, no scale
  LS_RES   fp32  res + gamma * (lin + bias), res [M, N] (in place) or row % res_mod of a [res_mod, N] table
The reference is fp64 on the f16 operand values, so it sees exactly what the kernel sees.  Bounds:
  fp32 out  |got - want| <= 1e-5 + 1e-5 |want|                       the constants of test_gpu_ops.py / test_gpu_gemm_routes.py
  f16 out   |got - s want| <= ulp_f16(s want) / 2 + s (1e-5 + 1e-5 |want|),  s = 8 (GELU) or 1 (QKV): the fp32 bound on the
            value that is rounded, plus the one RNE rounding."""
import importlib.util
import math
import os

import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location("gemm_routes", os.path.join(os.path.dirname(__file__), "test_gpu_gemm_routes.py"))
R = importlib.util.module_from_spec(_spec)     # check_rows_of, check_rows, F32_ATOL / F32_RTOL, the profiler control
_spec.loader.exec_module(R)

EPI_BIAS, EPI_GELU, EPI_LS_RES, EPI_QKV = 0, 1, 2, 8      # pope_hip.h POPE_EPI_*
EPI_NAME = {EPI_BIAS: "BIAS", EPI_GELU: "GELU", EPI_LS_RES: "LS_RES", EPI_QKV: "QKV"}
OUT_F16 = (EPI_GELU, EPI_QKV)
ACT, WSC = 8.0, 256.0                                     # POPE_PLANES_ACT_SCALE, POPE_PLANES_W_SCALE
QSCALE = 0.125 * math.log2(math.e)                        # head_dim^-0.5 * log2 e at heads of 64
F32_ATOL, F32_RTOL = R.F32_ATOL, R.F32_RTOL
TILE_ROWS = {"plain256": 256, "tile16": 128}
KERNEL = {"plain256": "gemm_plain256_kernel", "tile16": "gemm_planes16_kernel"}
RES_MOD = 289                                             # 17^2: divides no tile height


def plain_route(M, N, K, epi):
    """gemm_plain.hip pope_plain256_supported in real columns, for the calls pope_linear_f16 makes (lda = ldw = K / 2 pairs;
    the four epilogues all pass its switch)."""
    assert epi in EPI_NAME
    return "plain256" if M >= 2048 and N >= 256 and N % 64 == 0 and K >= 128 and K % 64 == 0 else "tile16"


# ---- cases ------------------------------------------------------------------------------------------------------------------
MS = (2047, 2048, 2049, 2303, 129, 1)     # tile16 16 tiles (last 127 rows) | 8 full 256-row tiles | last 1 row | last 255 | small
# (N, K) per epilogue: N 256 the smallest plain256 width, 320 a partial 256- and 128-column tile, 192 / 260 stay on tile16 at
# every M (N < 256, N % 64 != 0), 960 = QKV with q|k and k|v inside a 128- and a 256-column tile, 1152 = QKV of dim 384 (on a
# 128 edge, in the middle of a 256 tile); K 128 two K-steps, 192 an odd count, 768 SAM's patch embed, 1536 the long loop
NK = {
    EPI_BIAS: ((256, 128), (320, 768), (320, 1536), (192, 192), (260, 128)),
    EPI_GELU: ((256, 192), (320, 128), (320, 1536), (192, 768)),
    EPI_QKV: ((960, 128), (960, 768), (1152, 192), (1152, 1536), (192, 128)),
    EPI_LS_RES: ((256, 768), (320, 192), (320, 1536), (192, 128)),
}
CASES = [(epi, M, N, K) for epi in NK for (N, K) in NK[epi] for M in MS]
RES_MOD_CASES = [(8 * RES_MOD, 1152, 1536), (8 * RES_MOD, 320, 768), (2 * RES_MOD, 1152, 1536), (2 * RES_MOD, 320, 768)]


def case_id(case):
    epi, M, N, K = case
    return f"{EPI_NAME[epi]}-M{M}-N{N}-K{K}"


# ---- operands ---------------------------------------------------------------------------------------------------------------
_OPERANDS = {}


def operands(M, N, K):
    """a16 [M, K] = f16(a * 8), a = randn * 1.3; w16 [N, K] = f16(w * 256), w = randn * K^-0.5; bias, gamma (0.5 .. 1.5, signs
    mixed), the in-place residual [M, N] and the residual table [RES_MOD, N] (randn * 2: neighbouring rows differ by ~ 3, five
    orders of magnitude past the bound).  Host tensors, cached per shape."""
    key = (M, N, K)
    if key not in _OPERANDS:
        if len(_OPERANDS) > 8:
            _OPERANDS.clear()
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
        a16 = (torch.randn(M, K, generator=g) * 1.3 * ACT).half()
        gw = torch.Generator().manual_seed(N * 5 + K)
        w16 = (torch.randn(N, K, generator=gw) * K ** -0.5 * WSC).half()
        bias = torch.randn(N, generator=gw)
        gamma = (0.5 + torch.rand(N, generator=gw)) * torch.where(torch.rand(N, generator=gw) < 0.5, -1.0, 1.0)
        res = torch.randn(M, N, generator=g) * 2.0
        table = torch.randn(RES_MOD, N, generator=gw) * 2.0
        _OPERANDS[key] = dict(a16=a16, w16=w16, bias=bias, gamma=gamma, res=res, table=table)
    return _OPERANDS[key]


# ---- references and bounds --------------------------------------------------------------------------------------------------
def ref64(a16, w16, bias, epi, gamma=None, res=None):
    """fp64 on the f16 operand values: what the epilogue rounds (GELU: before the * 8)."""
    lin = F.linear(a16.double() / ACT, w16.double() / WSC, None if bias is None else bias.double())
    if epi == EPI_GELU:
        return F.gelu(lin)
    if epi == EPI_QKV:
        N = w16.shape[0]
        return lin * torch.where(torch.arange(N) < N // 3, QSCALE, 1.0).double()
    if epi == EPI_LS_RES:
        return res.double() + (1.0 if gamma is None else gamma.double()) * lin
    return lin


def ulp_f16(v):
    """2^(floor(log2 |v|) - 10), floored at 2^-24 (the subnormal spacing)."""
    e = torch.frexp(v.double().abs().clamp_min(2.0 ** -14))[1]      # |v| = m 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 11)


def _report(err, allowed, what):
    bad = err > allowed
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bounds, max |err| {float(err.max()):.3e}, "
                                 f"first bad (compared row index, col) {tuple(bad.nonzero()[0].tolist())}: |err| "
                                 f"{float(err[bad][0]):.3e} > {float(allowed[bad][0]):.3e}")
    return float(err.max()), float((err / allowed).max())


def check_f32(got, want, what):
    """fp32 output rows against fp64; returns (max |err|, max |err| / allowed)."""
    assert got.dtype == torch.float32
    return _report((got.double() - want).abs(), F32_ATOL + F32_RTOL * want.abs(), what)


def check_f16(got, want, scale, what):
    """f16 output rows (stored value = want * scale, rounded once) against fp64; returns (max |err| of the stored value, max
    |err| / allowed)."""
    assert got.dtype == torch.float16
    ws = want * scale
    return _report((got.double() - ws).abs(), 0.5 * ulp_f16(ws) + scale * (F32_ATOL + F32_RTOL * want.abs()), what)


def check_out(got, want, epi, what):
    return check_f16(got, want, ACT if epi == EPI_GELU else 1.0, what) if epi in OUT_F16 else check_f32(got, want, what)


def stored(want, epi):
    """An fp64 result in the output format of its epilogue: what a kernel with no error but the format's would write."""
    return (want * ACT).half() if epi == EPI_GELU else want.half() if epi == EPI_QKV else want.float()


def check_rows_of(M, route):
    return R.check_rows_of(M, TILE_ROWS[route])
