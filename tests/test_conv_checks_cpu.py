"""The host side of test_gpu_conv_routes.py (conv_checks.py): its fp64 restatements are torch's convolutions and torch's bilinear
interpolation, its comparison passes a faultless output and rejects the faults a convolution kernel is likely to have — on the
very case data —, its route mirrors straddle the switches, and pope_conv_layer_f32 refuses every call outside its contract
before any HIP call.  Host only."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_checks as K


def _find(form, prec=K.F16X3, **kw):
    for c in K.SMALL_CASES:
        if c["form"] == form and c["prec"] == prec and all(c[k] == v for k, v in kw.items()):
            return c
    raise AssertionError(f"no case {form} {prec} {kw}")


def _conv2d64(c, op):
    """F.conv2d in fp64 on the same operand values: [n, Ho, Wo, N]."""
    form = c["form"]
    k, stride, pad = {K.CONV3: (3, 1, 1), K.CONV1_UP: (1, 1, 0), K.STEM: (7, 2, 3)}.get(form, (3, 2, 1) if c["taps"] == 9 else (1, 2, 0))
    C = K.in_channels(c)
    w = op["w64"][:, :k * k * C].reshape(c["N"], k, k, C).permute(0, 3, 1, 2)     # tap-major (ky, kx, c) columns -> OIHW
    y = F.conv2d(op["x64"].permute(0, 3, 1, 2), w, op["bias"].double() if c["bias"] else None, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("c", [c for c in K.SMALL_CASES if c["H"] <= 14], ids=K.case_id)
def test_restatement_is_torch_conv2d(c):
    """ref64 = act(F.conv2d + res + upsample) in fp64, for every pixel."""
    op = K.operands(c)
    Ho, Wo = K.out_grid(c)
    pix = K.all_pixels(c["n"], Ho, Wo)
    want = _conv2d64(c, op)
    if c["res"]:
        want = want + op["res64"].reshape(c["n"], Ho + 2, Wo + 2, -1)[:, 1:-1, 1:-1]
    if c["form"] == K.CONV1_UP:
        up = F.interpolate(op["up64"].permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        # source coordinates in fp32: each of the two interpolation weights is off by at most max(H, W) 2^-24 per axis
        tol = 4 * max(c["H"], c["W"]) * 2.0 ** -24 * float(op["up64"].abs().max())
        got_up = K.bilinear64(op["up64"], pix, c["H"], c["W"]).reshape(up.shape)
        assert float((got_up - up).abs().max()) <= tol
        want = want + got_up
    want = want.clamp(min=0) + c["slope"] * want.clamp(max=0)
    got = K.ref64(c, op, pix).reshape(want.shape)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("H,W", [(4, 4), (4, 6), (6, 4), (14, 22), (36, 50), (64, 96)])
def test_bilinear_restatement_is_torch_interpolate(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    src = torch.randn(2, H // 2, W // 2, 8, generator=g, dtype=torch.float64)
    up = F.interpolate(src.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    got = K.bilinear64(src, K.all_pixels(2, H, W), H, W).reshape(up.shape)
    assert float((got - up).abs().max()) <= 4 * max(H, W) * 2.0 ** -24 * float(src.abs().max())


@pytest.mark.parametrize("c", [c for c in K.SMALL_CASES if c["H"] <= 14], ids=K.case_id)
def test_comparison_accepts_a_faultless_output(c):
    op = K.operands(c)
    Ho, Wo = K.out_grid(c)
    err, frac = K.check_output(c, op, K.stored(c, op), K.all_pixels(c["n"], Ho, Wo), K.case_id(c))
    assert frac < 0.5      # the format's own error is well inside the bound: a kernel has room


# fault -> the case that carries it
_C3 = dict(n=3, H=14, W=18)
FAULTS = [
    ("transpose", _find(K.CONV3, cch=4, N=128, **_C3)),                 # (dy, dx) transposed
    ("shift_right", _find(K.CONV3, cch=1, N=128, **_C3)),               # one tap shifted a pixel at the right border
    ("chunk_major", _find(K.CONV3, cch=8, N=196, out="planes", **_C3)), # chunk-major and tap-major weight columns mixed up
    ("no_res", _find(K.CONV3, cch=4, N=196, res=True, **_C3)),                 # the residual missing
    ("slope_pos", _find(K.CONV3, slope=0.01, out="f32", **_C3)),               # the slope applied to positives (0.01)
    ("slope_pos", _find(K.CONV3, slope=0.0, res=False, cch=7, **_C3)),               # ... (0: ReLU of the wrong sign)
    ("pad_nonzero", _find(K.CONV3, cch=1, N=196, out="planes", **_C3)), # a non-zero value in a padding column (196 -> 224)
    ("border_row", _find(K.CONV3, cch=1, N=128, **_C3)),                # one border row left unzeroed
    ("seam", _find(K.CONV3, cch=1, N=128, **_C3)),                      # a row of the next image used at a seam
    ("seam", _find(K.CONV_S2, taps=9, cch=4, N=196)),
    ("transpose", _find(K.CONV_S2, taps=9, cch=7, N=256)),
    ("x1_clamp", _find(K.CONV1_UP, n=2, H=4, W=4, N=256)),              # x1 clamp off by one at the last column
    ("x1_clamp", _find(K.CONV1_UP, n=3, H=14, W=22, N=196)),
    ("scale", _find(K.CONV1_UP, n=2, H=4, W=6, N=196)),                 # Hs / H as the scale in place of (Hs - 1) / (H - 1)
    ("scale", _find(K.CONV1_UP, n=3, H=14, W=22, N=256)),
    ("border_row", _find(K.CONV1_UP, n=2, H=6, W=4, N=256)),
    ("pad2", _find(K.STEM, n=2, H=8, W=12)),                            # the stem's pad 3 treated as pad 2
    ("pad2", _find(K.STEM, K.F32, n=2, H=4, W=4)),
    ("transpose", _find(K.STEM, n=2, H=8, W=12)),
    ("border_row", _find(K.STEM, K.F32, n=2, H=8, W=12)),
    ("transpose", _find(K.CONV3, K.F16, n=2, H=5, W=5)),
    ("shift_right", _find(K.CONV3, K.F32, n=2, H=5, W=5)),
]


@pytest.mark.parametrize("fault,c", FAULTS, ids=[f"{f}-{K.case_id(c)}" for f, c in FAULTS])
def test_comparison_rejects_planted_faults(fault, c):
    op = K.operands(c)
    Ho, Wo = K.out_grid(c)
    with pytest.raises(AssertionError):
        K.check_output(c, op, K.stored(c, op, fault), K.all_pixels(c["n"], Ho, Wo), f"{fault} planted")


def test_comparison_rejects_a_written_guard_row_and_fp32_padding():
    c = _find(K.CONV3, cch=7, N=196, out="f32", ldc=196)
    c224 = _find(K.CONV3, N=196, out="f32", ldc=224, **_C3)
    for cc, where in ((c, (K.out_rows(c), 0)), (c224, (K.out_rows(c224) // 2 + 3, 200))):
        op = K.operands(cc)
        out = K.stored(cc, op)
        out[where] = 0.5
        with pytest.raises(AssertionError):
            K.check_output(cc, op, out, K.all_pixels(cc["n"], *K.out_grid(cc)), "planted")


@pytest.mark.parametrize("cu", [256, 304, 64])
def test_route_mirrors_straddle_the_switches(cu):
    """Below / at the switch by exactly one tile; every image of a switch case alone stays below it."""
    cs = K.conv3_switch_cases(cu)
    for below, at in zip(cs[0::2], cs[1::2]):
        assert K.wide_tiles(below) == cu - 1 and K.wide_tiles(at) == cu
        assert K.kernels_of(below, cu)[0] == "tile16" and K.kernels_of(at, cu)[0] == "wide"
        assert not K.wide_conv_supported(dict(at, n=1), cu)
    ss = K.s2_switch_cases(cu)
    for below, at in zip(ss[0::2], ss[1::2]):
        assert K.wide_tiles(below) < cu <= K.wide_tiles(at) and K.wide_tiles(at) - K.wide_tiles(below) <= 1
        assert K.kernels_of(below, cu)[:2] == ["gather", "tile16"] and K.kernels_of(at, cu)[0] == "wide"
        assert not K.wide_conv_s2_supported(dict(at, n=1), cu)
        Ho, Wo = K.out_grid(at)
        assert Ho + 2 != Wo + 2
    assert all(K.kernels_of(c, cu)[0] != "wide" for c in K.SMALL_CASES)


def test_check_pixels_cover_tiles_and_seams():
    c = K.conv3_switch_cases(256)[1]
    pix = K.check_pixels(c, 256)
    Ho, Wo = K.out_grid(c)
    rows = K.pixel_rows(c, pix) - (Wo + 3)                    # GEMM rows
    m = K.gemm_m(c)
    assert int(rows.min()) == 0 and int(rows.max()) == m - 1
    assert bool(((rows < 256).sum() >= 200) and ((rows >= (m - 1) // 256 * 256).sum() >= 100))
    mid = rows[(rows >= 256) & (rows < (m - 1) // 256 * 256)]
    assert len(mid) >= 48
    for b in range(c["n"]):
        for y in (0, Ho - 1):
            assert int(((pix[:, 0] == b) & (pix[:, 1] == y)).sum()) == Wo


def _args(hip_lib, **kw):
    from pope_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    base = dict(form=K.CONV3, precision=K.F16X3, n=2, H=6, W=8, cch=4, taps=0, a=p, a_rows=2 * 8 * 10, w=p, bias=p, N=128, ldc=128,
                slope=0.0, out_planes=p, out_f32=None, zero_border=1, res=None, ldres=0, up_src=None, up_lds=0, scratch=None,
                scratch_bytes=0, range_flag=None)
    base.update(kw)
    a = _lib.ConvLayerArgs(**base)
    a._keep = buf
    return a, p


def test_conv_layer_argument_validation_without_gpu(hip_lib):
    """Every rejection of pope_conv_layer_f32's contract comes back before the stream's device is touched (this machine has
    none); the pointers are never dereferenced."""
    _, p = _args(hip_lib)
    big = 1 << 40
    s2 = dict(form=K.CONV_S2, taps=9, scratch=p, scratch_bytes=big, zero_border=1)
    up = dict(form=K.CONV1_UP, up_src=p, up_lds=128)
    stem = dict(form=K.STEM, cch=0, a_rows=0, scratch=p, scratch_bytes=big)
    f32o = dict(out_planes=None, out_f32=p, zero_border=0)
    bad = {
        "form 4": dict(form=4), "form -1": dict(form=-1), "precision 3": dict(precision=3),
        "CONV_S2 in fp32": dict(s2, precision=K.F32, **f32o), "CONV1_UP in fp32": dict(up, precision=K.F32, **f32o),
        "CONV_S2 in f16": dict(s2, precision=K.F16), "STEM in f16": dict(stem, precision=K.F16),
        "f16 to planes": dict(precision=K.F16), "f16 with res": dict(precision=K.F16, res=p, ldres=128, **f32o),
        "fp32 to planes": dict(precision=K.F32),
        "n=0": dict(n=0), "H=0": dict(H=0), "W=-2": dict(W=-2),
        "N=0": dict(N=0, ldc=0), "N=130": dict(N=130, ldc=160), "N=260": dict(N=260, ldc=288), "N=512": dict(N=512, ldc=512),
        "cch=0": dict(cch=0), "CONV3 with taps": dict(taps=9),
        "CONV_S2 taps 3": dict(s2, taps=3), "CONV_S2 taps 0": dict(s2, taps=0), "CONV_S2 taps 1 cch 1": dict(s2, taps=1, cch=1),
        "CONV1_UP cch 1": dict(up, cch=1), "STEM with cch": dict(stem, cch=2), "STEM with taps": dict(stem, taps=9),
        "CONV_S2 odd H": dict(s2, H=7, a_rows=2 * 9 * 10), "CONV_S2 odd W": dict(s2, W=9, a_rows=2 * 8 * 11),
        "CONV1_UP odd W (up_wp 3)": dict(up, W=1, a_rows=2 * 8 * 3), "CONV1_UP odd H": dict(up, H=5),
        "STEM odd H": dict(stem, H=7), "STEM odd W": dict(stem, W=9),
        "null a": dict(a=None), "null w": dict(w=None), "misaligned a": dict(a=p + 4), "misaligned w": dict(w=p + 8),
        "misaligned bias": dict(bias=p + 4),
        "a one row short": dict(a_rows=2 * 8 * 10 - 1), "fp32 loader: a one row short": dict(precision=K.F32, a_rows=2 * 8 * 10 - 1, **f32o),
        "a_rows of the interior only": dict(a_rows=2 * 6 * 8),
        "no output": dict(out_planes=None), "both outputs": dict(out_f32=p),
        "planes ldc 160": dict(ldc=160), "planes ldc 196 for N 196": dict(N=196, ldc=196), "planes ldc 256 for N 196": dict(N=196, ldc=256),
        "planes without the border pass": dict(zero_border=0), "CONV1_UP without the border pass": dict(up, zero_border=0),
        "STEM without the border pass": dict(stem, zero_border=0),
        "fp32 ldc below N": dict(f32o, ldc=124), "fp32 ldc 130": dict(f32o, ldc=130), "misaligned out": dict(out_planes=p + 2),
        "CONV_S2 to fp32": dict(s2, **f32o), "CONV1_UP to fp32": dict(up, **f32o), "f16x3 STEM to fp32": dict(stem, **f32o),
        "res below N": dict(res=p, ldres=96), "res pitch 132 (planes)": dict(res=p, ldres=132), "res misaligned": dict(res=p + 4, ldres=128),
        "fp32 res pitch 130": dict(precision=K.F32, res=p, ldres=130, **f32o),
        "res with CONV_S2": dict(s2, res=p, ldres=128), "res with CONV1_UP": dict(up, res=p, ldres=128),
        "CONV1_UP without up_src": dict(up, up_src=None), "up_lds below N": dict(up, up_lds=124), "up_lds 130": dict(up, up_lds=130),
        "up_src misaligned": dict(up, up_src=p + 4), "up_src with CONV3": dict(up_src=p, up_lds=128),
        "CONV_S2 without scratch": dict(s2, scratch=None), "STEM without scratch": dict(stem, scratch=None),
        "scratch misaligned": dict(s2, scratch=p + 4),
        "operand of 4 GiB": dict(n=1, H=4094, W=2046, a_rows=4096 * 2048, cch=4),
        "output of 4 GiB": dict(n=1, H=8190, W=4094, a_rows=8192 * 4096, cch=1),
    }
    for what, kw in bad.items():
        a, _ = _args(hip_lib, **kw)
        assert hip_lib.pope_conv_layer_f32(ctypes.byref(a), None) == -1, what
    short = {"CONV_S2 scratch one byte short": dict(s2, scratch_bytes=2 * 5 * 6 * 9 * 4 * 128 - 1),
             "STEM scratch one byte short": dict(stem, scratch_bytes=2 * 5 * 6 * 256 - 1)}
    for what, kw in short.items():
        a, _ = _args(hip_lib, **kw)
        assert hip_lib.pope_conv_layer_f32(ctypes.byref(a), None) == -3, what      # POPE_ERR_WORKSPACE
    assert hip_lib.pope_conv_layer_f32(None, None) == -1
    assert hip_lib.pope_conv_layer_scratch_bytes(K.CONV_S2, 2, 6, 8, 4, 9) == 2 * 5 * 6 * 9 * 4 * 128
    assert hip_lib.pope_conv_layer_scratch_bytes(K.STEM, 2, 6, 8, 0, 0) == 2 * 5 * 6 * 256
    assert hip_lib.pope_conv_layer_scratch_bytes(K.CONV3, 2, 6, 8, 4, 0) == 0
