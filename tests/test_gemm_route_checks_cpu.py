"""The comparison helpers of test_gpu_gemm_routes.py reject outputs with the faults a GEMM route is likely to have: the last
K-step dropped, the bias missing on one 128-column tile, the last ragged row tile shifted by one row.  Host only."""
import importlib.util
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("gemm_routes", os.path.join(os.path.dirname(__file__), "test_gpu_gemm_routes.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

M, N, K = 1000, 384, 96


def _operands():
    from pope_amd import _lib
    g = torch.Generator().manual_seed(3)
    a = R.from_planes(_lib.to_planes(torch.randn(M, K, generator=g) * 1.3, R.ACT), R.ACT)
    w = R.from_planes(_lib.to_planes(torch.randn(N, K, generator=g) * K ** -0.5, R.WSC), R.WSC)
    return a, w, torch.randn(N, generator=g)


def _corrupt(kind, a, w, b, epi):
    want = R.fp64_linear(a, w, b, epi)
    if kind == "none":
        return want.float()
    if kind == "last_k_step_dropped":
        return R.fp64_linear(a[:, :K - 32], w[:, :K - 32], b, epi).float()
    if kind == "bias_missing_on_one_column_tile":
        return R.fp64_linear(a, w, torch.cat([b[:128], torch.zeros(128), b[256:]]), epi).float()
    if kind == "last_row_tile_shifted":
        got = want.float().clone()
        last0 = (M - 1) // 192 * 192
        got[last0 + 1:M] = want[last0:M - 1].float()
        return got
    raise ValueError(kind)


@pytest.mark.parametrize("epi", [R.EPI_BIAS, R.EPI_GELU], ids=["bias", "gelu"])
@pytest.mark.parametrize("out_planes", [False, True], ids=["fp32_out", "planes_out"])
@pytest.mark.parametrize("kind", ["none", "last_k_step_dropped", "bias_missing_on_one_column_tile", "last_row_tile_shifted"])
def test_checks_reject_corrupted_outputs(kind, out_planes, epi):
    from pope_amd import _lib
    a, w, b = _operands()
    got = _corrupt(kind, a, w, b, epi)
    if out_planes:
        got = R.from_planes(_lib.to_planes(got, R.ACT), R.ACT)
    rows = R.check_rows_of(M, 192)   # stream384's row tile: the last one is ragged (40 rows)
    want = R.fp64_linear(a[rows], w, b, epi)
    atol, rtol = (R.PLANES_ATOL, 0.0) if out_planes else (R.F32_ATOL, R.F32_RTOL)
    if kind == "none":
        R.check_rows(got[rows], want, atol, rtol, kind)
        return
    with pytest.raises(AssertionError) as e:
        R.check_rows(got[rows], want, atol, rtol, kind)
    print(f"{kind} ({'planes' if out_planes else 'fp32'} out, {'GELU' if epi else 'BIAS'}): {e.value}")
    # the bit-identity check of the routes rejects it as well
    assert not torch.equal(got, _corrupt("none", a, w, b, epi) if not out_planes else
                           R.from_planes(_lib.to_planes(_corrupt("none", a, w, b, epi), R.ACT), R.ACT))
