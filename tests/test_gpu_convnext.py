"""GPU: the ConvNeXtV2 backbone (pope_amd/convnextv2.py, convnext.hip) against the reference module's fp64 evaluation
(tests/golden/convnext.npz, scripts/gen_golden_convnext.py), the two new arithmetic kernels alone against fp64 torch on the CPU,
batch independence, determinism and the range guard.

Bound of every comparison: MARGIN x the fp32 reference's own error against fp64 on the same input (e32 of the fixture for the
taps, the fp32 torch op's error for the op-level checks) — never a figure taken from the code under test."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from pope_amd import _lib, convnextv2, synth

pytestmark = pytest.mark.gpu
MARGIN = 4.0
PRECISIONS = ("f32", "f16x3")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "convnext.npz"))


_cache = {}


def run_case(name, precision):
    """(model, x, features, logits, taps) of one fixture case, computed once per precision."""
    key = (name, precision)
    if key not in _cache:
        case = synth.convnext_case(name)
        model = convnextv2.ConvNeXtV2(precision=precision, **case["cfg"])
        model.load_state_dict(case["state_dict"], strict=True)
        model = model.cuda()
        x = case["x"].cuda()
        f, o, t = model.forward_with_taps(x)
        torch.cuda.synchronize()
        assert model.overflow_events == 0
        _cache[key] = (model, x, f, o, [v.contiguous() for v in t])
    return _cache[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(synth.CONVNEXT_CASES))
def test_taps_against_fp64(gold, name, precision):
    _, _, f, o, t = run_case(name, precision)
    got = dict(zip(synth.CONVNEXT_TAPS, t + [f, o]))
    worst = {}
    for tap in synth.CONVNEXT_TAPS:
        want = torch.from_numpy(gold[f"{name}.{tap}64"])
        idx = synth.convnext_tap_index(name, tap, got[tap].numel())
        g = got[tap].reshape(-1).cpu()[idx].double()
        assert torch.isfinite(g).all()
        e32 = float(gold[f"{name}.e32_{tap}"])
        worst[tap] = float((g - want).abs().max()) / e32
        print(f"{name} {precision} {tap}: max |gpu - fp64| = {worst[tap]:.2f} x e32 ({e32:.3g})")
    assert all(r <= MARGIN for r in worst.values()), worst


def _dw_ref(x, w, b, dtype):
    """x [B, H, W, C] channels-last -> the same layout, torch conv2d on the CPU in `dtype`."""
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), b.to(dtype), padding=3, groups=x.shape[3])
    return y.permute(0, 2, 3, 1).contiguous()


# a 3 x 5 and a 1 x 1 map (smaller than the kernel), C = 80 (a partial 64-channel group) and 320; 13 x 21: six tiles with ragged edges
@pytest.mark.parametrize("B,H,W,Cc", [(2, 3, 5, 80), (1, 1, 1, 320), (2, 13, 21, 80), (1, 8, 16, 320)])
def test_dwconv_against_fp64(hip_lib, B, H, W, Cc):
    g = torch.Generator().manual_seed(100 * H + W + Cc)
    x = torch.randn(B, H, W, Cc, generator=g)
    w = torch.randn(Cc, 1, 7, 7, generator=g) / 7
    b = 0.2 * torch.randn(Cc, generator=g)
    want = _dw_ref(x, w, b, torch.float64)
    e32 = float((_dw_ref(x, w, b, torch.float32).double() - want).abs().max())
    xd, bd = x.cuda(), b.cuda()
    w49 = w.reshape(Cc, 49).t().contiguous().cuda()
    y = torch.full_like(xd, float("nan"))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(hip_lib.pope_convnext_dwconv_f32(p(xd), p(w49), p(bd), p(y), B, H, W, Cc, _lib.stream_of(xd.device)), "dwconv")
    torch.cuda.synchronize()
    err = float((y.cpu().double() - want).abs().max())
    print(f"dwconv {B}x{H}x{W}x{Cc}: max err {err:.3g} = {err / max(e32, 1e-30):.2f} x the fp32 op's {e32:.3g}")
    assert err <= MARGIN * e32


def _grn_ref(x, gamma, beta, dtype):
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    Gx = torch.norm(x, p=2, dim=1, keepdim=True)            # x [B, HW, C]: the reference's dim=(1, 2) of [B, H, W, C]
    Nx = Gx / (Gx.mean(dim=-1, keepdim=True) + 1e-6)
    return gamma * (x * Nx) + beta + x


# HW = 15 (the 3 x 5 map) and 1, one partial chunk, several chunks with a ragged last one; C = 320 and 1280
@pytest.mark.parametrize("B,HW,Cc", [(2, 15, 320), (1, 1, 1280), (3, 200, 320), (2, 64, 1280)])
def test_grn_against_fp64(hip_lib, B, HW, Cc):
    g = torch.Generator().manual_seed(7 * HW + Cc)
    x = torch.randn(B, HW, Cc, generator=g) * (0.5 + torch.rand(1, 1, Cc, generator=g))
    gamma = 0.5 + torch.rand(Cc, generator=g)
    beta = 0.3 * torch.randn(Cc, generator=g)
    want = _grn_ref(x, gamma, beta, torch.float64)
    e32 = float((_grn_ref(x, gamma, beta, torch.float32).double() - want).abs().max())
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    need = hip_lib.pope_convnext_grn_workspace_bytes(B, HW, Cc)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    y = torch.full_like(xd, float("nan"))
    pl = torch.zeros(B * HW, 2 * Cc, dtype=torch.float16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = _lib.stream_of(xd.device)
    _lib.check(hip_lib.pope_convnext_grn_f32(p(xd), p(gd), p(bd), B, HW, Cc, p(y), None, p(ws), need, None, st), "grn")
    _lib.check(hip_lib.pope_convnext_grn_f32(p(xd), p(gd), p(bd), B, HW, Cc, None, p(pl), p(ws), need, p(flag), st), "grn planes")
    torch.cuda.synchronize()
    err = float((y.cpu().double() - want).abs().max())
    print(f"grn {B}x{HW}x{Cc}: max err {err:.3g} = {err / e32:.2f} x the fp32 op's {e32:.3g}")
    assert err <= MARGIN * e32
    # the planes form is the same arithmetic followed by the hi / lo split, and an in-range call leaves the flag alone
    assert torch.equal(pl.view(B * HW, Cc // 32, 2, 32), _lib.to_planes(y.view(B * HW, Cc), _lib.PLANES_ACT_SCALE))
    assert int(flag.item()) == 0
    # one image's result does not depend on its batch neighbours
    if B > 1:
        y1 = torch.empty(1, HW, Cc, device="cuda")
        _lib.check(hip_lib.pope_convnext_grn_f32(p(xd[B - 1:]), p(gd), p(bd), 1, HW, Cc, p(y1), None, p(ws), need, None, st), "grn")
        assert torch.equal(y1[0], y[B - 1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_independence_and_determinism(precision):
    model, x, f, o, t = run_case("small", precision)
    f2, o2, t2 = model.forward_with_taps(x)
    assert torch.equal(f2, f) and torch.equal(o2, o) and all(torch.equal(a, b) for a, b in zip(t2, t))
    for b in range(x.shape[0]):
        fb, ob, tb = model.forward_with_taps(x[b:b + 1])
        assert torch.equal(fb[0], f[b]) and torch.equal(ob[0], o[b]), b
        assert all(torch.equal(a[0], w[b]) for a, w in zip(tb, t)), b
    assert torch.equal(model.forward_features(x), f) and torch.equal(model(x), o)
    assert model.overflow_events == 0


def test_range_guard_reruns_in_f32():
    """The stem's LayerNorm makes the network invariant to the scale of the image, so no scaling of the image can push an f16x3
    producer out of range; the operand that is scaled here is the first block's LayerNorm gain (x 3e4), whose output is the
    planes operand of pwconv1 (K = 64): |y| x 8 passes 65520 and POPE_RANGE_LAYERNORM is raised."""
    case = synth.convnext_case("small")
    sd = dict(case["state_dict"])
    sd["stages.0.0.norm.weight"] = sd["stages.0.0.norm.weight"] * 3e4
    models = {}
    for precision in PRECISIONS:
        m = convnextv2.ConvNeXtV2(precision=precision, **case["cfg"])
        m.load_state_dict(sd, strict=True)
        models[precision] = m.cuda()
    x = case["x"].cuda()
    want_f, want_o, want_t = models["f32"].forward_with_taps(x)
    with pytest.warns(UserWarning, match="f16x3 range"):
        got_f, got_o, got_t = models["f16x3"].forward_with_taps(x)
    assert models["f16x3"].overflow_events == 1 and models["f32"].overflow_events == 0
    assert torch.isfinite(want_o).all()
    assert torch.equal(got_f, want_f) and torch.equal(got_o, want_o) and all(torch.equal(a, b) for a, b in zip(got_t, want_t))
    # an in-range call leaves the counter alone
    model, xs, _, o, _ = run_case("small", "f16x3")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert torch.equal(model(xs), o)
    assert model.overflow_events == 0


def test_sizes_must_be_multiples_of_32():
    model, x, *_ = run_case("small", "f32")
    for shape in ((1, 3, 96, 150), (1, 3, 100, 160), (1, 3, 16, 32)):
        with pytest.raises(ValueError, match="multiples of 32"):
            model(torch.zeros(shape, device="cuda"))
    with pytest.raises(ValueError):
        model(torch.zeros(1, 1, 96, 160, device="cuda"))
    assert model(torch.zeros(1, 3, 32, 32, device="cuda")).shape == (1, 32)       # the smallest input: every map is 1 x 1 from stage 1 on
