"""Host only: the argument contract of the two rowln test entries (rejected before any HIP call), the launcher mirrors at the
MI355X's 256 CUs, and the comparison helpers of test_gpu_rowln.py rejecting plausible wrong kernels restated in fp32 torch:
a one-pass variance, eps ignored, the residual table indexed by row instead of row % res_mod, gamma dropped, the last ragged
tile shifted by one row."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("gpu_rowln", os.path.join(os.path.dirname(__file__), "test_gpu_rowln.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

FAKE = C.c_void_p(0x1000)   # never dereferenced: every call below is rejected before it reaches the device


def _rowln(hip_lib, a=FAKE, w=FAKE, M=1000, K=64, bias=FAKE, gamma=FAKE, res=FAKE, res_mod=0, x=FAKE, lw=FAKE, lb=FAKE,
           ln_planes=FAKE, ln_out=None):
    return hip_lib.pope_linear_rowln_f32(a, w, M, K, bias, gamma, res, res_mod, x, lw, lb, 1e-6, ln_planes, ln_out, None, None)


def test_rowln_entry_rejections_without_gpu(hip_lib):
    rejected = {
        "K % 32 != 0": dict(K=80), "K < 64": dict(K=32), "K = 0": dict(K=0),
        "null A": dict(a=None), "null W": dict(w=None), "null x": dict(x=None), "null res": dict(res=None),
        "null ln_w": dict(lw=None), "null ln_b": dict(lb=None),
        "both LayerNorm outputs": dict(ln_out=FAKE), "no LayerNorm output": dict(ln_planes=None),
        "res_mod < 0": dict(res_mod=-1), "res_mod == 0 with a null gamma": dict(gamma=None),
        "M = 0": dict(M=0), "M < 0": dict(M=-5),
        "M past the 32-bit offsets at K = 64": dict(M=R.MAX_M_K64 + 1),
        "M past the 32-bit offsets of A at K = 1536": dict(M=(1 << 32) // (1536 * 4) - 191, K=1536),
    }
    for what, kw in rejected.items():
        assert _rowln(hip_lib, **kw) == R.ERR_ARG, what
    assert R.MAX_M_K64 == 2_796_010


def test_layernorm_rowln_order_entry_rejections_without_gpu(hip_lib):
    f = hip_lib.pope_layernorm_rowln_order_f32
    assert f(None, FAKE, FAKE, FAKE, None, 10, 1e-6, None, None) == R.ERR_ARG
    assert f(FAKE, None, FAKE, FAKE, None, 10, 1e-6, None, None) == R.ERR_ARG
    assert f(FAKE, FAKE, None, FAKE, None, 10, 1e-6, None, None) == R.ERR_ARG
    assert f(FAKE, FAKE, FAKE, FAKE, FAKE, 10, 1e-6, None, None) == R.ERR_ARG      # both outputs
    assert f(FAKE, FAKE, FAKE, None, None, 10, 1e-6, None, None) == R.ERR_ARG      # neither
    assert f(FAKE, FAKE, FAKE, FAKE, None, 0, 1e-6, None, None) == R.ERR_ARG
    assert f(FAKE, FAKE, FAKE, None, FAKE, -1, 1e-6, None, None) == R.ERR_ARG


def test_mirrors_at_256_cus():
    """The switches of the issue at the MI355X's CU count: geometry flips near 32 768, 49 152 and 65 536 rows, the ViT's
    small switch at 21 760 rows, the production chunk of 97 984 rows on 192-row tiles in 2 rounds with a 255-tile tail."""
    assert R.geometry_flips(256) == [32769, 49153, 65537]
    assert [R.rowln_geo(m, 256) for m in (32768, 32769, 49152, 49153, 65536, 65537)] == [128, 192, 192, 128, 128, 192]
    assert R.small_switch(256) == 21760 and R.vit_small(21760, 256) and not R.vit_small(21761, 256)
    assert R.rowln_grid(97984, 256) == (192, 511, 256, 1, 255, 64)
    assert R.rowln_grid(30620, 256) == (128, 240, 240, 1, 0, 28)
    assert R.kernel_info("void (anonymous namespace)::gemm_rowln16_kernel<(anonymous namespace)::RlGeo<192, 2>, 0, true>"
                         "(GemmParams, int, int)") == (192, 0, True)
    assert R.kernel_info("_ZN12_GLOBAL__N_119gemm_rowln16_kernelINS_5RlGeoILi128ELi2EEELi1ELb0EEEv10GemmParamsii") == (128, 1, False)
    assert R.kernel_info("gemm_planes16_kernel") is None


# ---- wrong kernels in fp32 torch ---------------------------------------------------------------------------------------------
def ln_fp32(x, lw, lb, eps, one_pass=False):
    """LayerNorm in fp32: two-pass (the kernel's form) or one-pass E[x^2] - mean^2."""
    mean = x.mean(dim=1, keepdim=True)
    if one_pass:
        var = (x * x).mean(dim=1, keepdim=True) - mean * mean
    else:
        d = x - mean
        var = (d * d).mean(dim=1, keepdim=True)
    return (x - mean) * (1.0 / torch.sqrt(var + eps)) * lw + lb


def _ln_rows(kind, M=300):
    g = torch.Generator().manual_seed(11)
    n = torch.randn(M, R.RN, generator=g)
    if kind == "offset500":
        return 500.0 + 0.05 * n
    if kind == "near_eps":
        return 0.3 * torch.randn(M, 1, generator=g) + 1e-3 * n
    return n


@pytest.mark.parametrize("out_planes", [False, True], ids=["fp32_out", "planes_out"])
@pytest.mark.parametrize("kind", ["correct_offset500", "correct_near_eps", "one_pass_variance", "eps_ignored"])
def test_layernorm_bound_rejects_wrong_kernels(kind, out_planes):
    from pope_amd import _lib
    g = torch.Generator().manual_seed(12)
    lw, lb = 1.0 + 0.1 * torch.randn(R.RN, generator=g), 0.1 * torch.randn(R.RN, generator=g)
    eps = 1e-6
    if kind in ("correct_offset500", "one_pass_variance"):
        x = _ln_rows("offset500")
    else:
        x = _ln_rows("near_eps")
    if kind.startswith("correct"):
        got = ln_fp32(x, lw, lb, eps)
    elif kind == "one_pass_variance":
        got = ln_fp32(x, lw, lb, eps, one_pass=True)
    else:
        got = ln_fp32(x, lw, lb, 0.0)
    if out_planes:
        got = _lib.from_planes(_lib.to_planes(got, R.ACT), R.ACT)
    if kind.startswith("correct"):   # honest fp32 arithmetic sits inside the bound
        ratio = R.check_ln(got, x, lw, lb, eps, kind)
        print(f"{kind}: fp32 two-pass LayerNorm err / (2^-24 scale) = {ratio:.2f} (bound {R.LN_C})")
        return
    with pytest.raises(AssertionError) as e:
        R.check_ln(got, x, lw, lb, eps, kind)
    print(f"{kind}: {e.value}")


def _residual_operands(M=1000, K=96, res_mod=197):
    from pope_amd import _lib
    g = torch.Generator().manual_seed(13)
    a = _lib.from_planes(_lib.to_planes(torch.randn(M, K, generator=g) * 1.3, R.ACT), R.ACT)
    w = _lib.from_planes(_lib.to_planes(torch.randn(R.RN, K, generator=g) * K ** -0.5, R.WSC), R.WSC)
    bias, gamma = torch.randn(R.RN, generator=g), 0.5 + torch.rand(R.RN, generator=g)
    table = torch.randn(res_mod, R.RN, generator=g)
    return a, w, bias, gamma, table


@pytest.mark.parametrize("kind", ["none", "residual_by_row", "gamma_dropped", "last_tile_shifted"])
def test_residual_check_rejects_wrong_kernels(kind):
    M, res_mod, T = 1000, 197, 192
    a, w, bias, gamma, table = _residual_operands(M, res_mod=res_mod)
    full = torch.cat([table] * (M // res_mod + 1))[:M + res_mod]   # the table expanded; rows past res_mod for the wrong index
    idx = torch.arange(M)
    lin = (a @ w.T + bias)
    if kind == "residual_by_row":          # table row `row` (a neighbouring buffer) instead of row % res_mod
        wrong_table = torch.cat([table, torch.randn(M, R.RN, generator=torch.Generator().manual_seed(14))])
        got = wrong_table[idx] + gamma * lin
    elif kind == "gamma_dropped":
        got = full[idx] + lin
    else:
        got = table[idx % res_mod] + gamma * lin
        if kind == "last_tile_shifted":
            last0 = (M - 1) // T * T
            got = got.clone()
            got[last0 + 1:M] = got[last0:M - 1].clone()
    rows = R.check_rows_of(M, T)
    want = R.fp64_residual(a[rows], w, bias, gamma, R.residual_rows(table, res_mod, rows))
    if kind == "none":
        R.check_rows(got[rows], want, R.X_ATOL, R.X_RTOL, kind)
        return
    with pytest.raises(AssertionError) as e:
        R.check_rows(got[rows], want, R.X_ATOL, R.X_RTOL, kind)
    print(f"{kind}: {e.value}")
