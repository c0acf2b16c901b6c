"""GPU: every convolution route of the LoFTR CNN and of the SAM neck, one layer at a time through pope_conv_layer_f32, against fp64.

The entry runs exactly one layer's launch sequence of pope_launch_resnetfpn (conv.hip, conv_layer.h) on the caller's buffers:
  CONV3     implicit 3x3: gemm_planes16_kernel<EPI_CONV, .., CONV> below one round of the CUs, gemm_plain256_kernel<.., CONV = 1>
            from `ceil(M / 256) ceil(N / bn) >= CUs` on; fp32: gemm_nt_f32_kernel<EPI_CONV, LOAD_CONV>; plain f16: the SAM neck's form
  CONV_S2   gemm_plain256_kernel<.., CONV = 2> from the same switch on, else gather_s2_kernel + the tile kernel
  CONV1_UP  gemm_planes16_kernel<EPI_CONV_UP>: the FPN merge in the lateral convolution's epilogue
  STEM      stem_gather_kernel + the K = 64 GEMM
each followed by zero_border_kernel where the model has it.  Cases, operands, fp64 restatements, route mirrors and the
comparison are conv_checks.py's (test_conv_checks_cpu.py shows what the comparison rejects).  Every case checks the kernels that
ran (torch.profiler, with test_gpu_gemm_routes.py's control), fp64 parity (first and last row tile, image seams, 48 rows in
between; small cases in full), exact zeros on border rows and padding columns, the guard rows past the output, and the range
flag; the 256-row routes are also held bit for bit to the small-batch route, image by image.  Measured errors: profiles/conv_routes.md."""
import ctypes as C
import re

import pytest
import torch

import conv_checks as K

R = K.R
pytestmark = pytest.mark.gpu

RANGE_INPUT = 32                        # pope_hip.h POPE_RANGE_INPUT: what every convolution epilogue reports under
FOREIGN = 4                             # POPE_RANGE_QKV: a bit no convolution reports, pre-set in the flag word

dev = R.dev                             # module-scoped fixtures of test_gpu_gemm_routes.py
cu = R.cu
profiler_ok = R.profiler_ok


def test_profiler_sees_library_kernels(profiler_ok):
    """The control of the kernel assertions below; when it fails they check numerics only."""
    if profiler_ok is not None:
        pytest.skip(f"kernel-name assertions are off: {profiler_ok}")


def _kernel_matches(key, c, name):
    if K.KERNEL[key] not in name:
        return False
    if key == "f32":      # gemm_nt_f32_kernel<EPI_CONV = 6, LOADER>: LOAD_CONV = 3 for the implicit 3x3, LOAD_GENERIC = 0 for the stem
        m = re.search(r"gemm_nt_f32_kernel(?:<\s*(\d+)\s*,\s*(\d+)\s*>|ILi(\d+)ELi(\d+)E)", name)
        return bool(m) and (int(m.group(1) or m.group(3)), int(m.group(2) or m.group(4))) == (6, 3 if c["form"] == K.CONV3 else 0)
    if key == "tile16":   # gemm_planes16_kernel<EPI, ..>: EPI_CONV_UP = 9 with up_src, else EPI_CONV = 6
        m = re.search(r"gemm_planes16_kernel(?:<\s*(\d+)\s*,|ILi(\d+)E)", name)
        return bool(m) and int(m.group(1) or m.group(2)) == (9 if c["form"] == K.CONV1_UP else 6)
    return True


def _run_routed(c, cu, fn, profiler_ok, what):
    """Run fn (one library call); assert that the device kernels it launched are the sequence the mirror names."""
    if profiler_ok is not None:
        return fn()
    ret, names = R._device_kernels(fn)
    want = K.kernels_of(c, cu)
    assert len(names) == len(want) and all(_kernel_matches(k, c, n) for k, n in zip(want, names)), f"{what}: expected {want}, ran {names}"
    print(f"route confirmed: {'+'.join(want):22s} {what}")
    return ret


def _device_operands(c, dev):
    op = K.operands(c)
    d = {k: op[k].to(dev) for k in ("a", "img", "w", "bias", "res", "up_src") if k in op}
    return op, d


def _call(hip_lib, c, d, out, dev, flag=None, img=None, routed=None):
    """One pope_conv_layer_f32 call of case c into `out`; img = b: image b alone (n = 1) on its rows of the same buffers."""
    from pope_amd import _lib
    n, H, W = c["n"], c["H"], c["W"]
    in_rows, o_rows = (H + 2) * (W + 2), K.out_rows(c) // n
    stem = c["form"] == K.STEM
    a = d["img"] if stem else d["a"]
    res, up, o = d.get("res"), d.get("up_src"), out
    if img is not None:
        a = a[img:] if stem else a[img * in_rows:]
        res = res[img * o_rows:] if res is not None else None
        up = up[img * (H // 2 + 2) * (W // 2 + 2):] if up is not None else None
        o = out[img * o_rows:]
        n = 1
    nbytes = hip_lib.pope_conv_layer_scratch_bytes(c["form"], n, H, W, c["cch"], c["taps"])
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    p = lambda t: t.data_ptr() if t is not None else None
    args = _lib.ConvLayerArgs(
        form=c["form"], precision=c["prec"], n=n, H=H, W=W, cch=c["cch"], taps=c["taps"], a=p(a), a_rows=0 if stem else n * in_rows,
        w=p(d["w"]), bias=p(d["bias"]) if c["bias"] else None, N=c["N"], ldc=c["ldc"], slope=c["slope"],
        out_planes=p(o) if c["out"] == "planes" else None, out_f32=p(o) if c["out"] == "f32" else None, zero_border=int(c["border"]),
        res=p(res), ldres=c["ldc"] if res is not None else 0, up_src=p(up), up_lds=c["ldc"] if up is not None else 0,
        scratch=p(scratch), scratch_bytes=nbytes, range_flag=p(flag))
    call = lambda: hip_lib.pope_conv_layer_f32(C.byref(args), R._stream())
    rc = _run_routed(dict(c, n=n), routed[0], call, routed[1], routed[2]) if routed else call()
    torch.cuda.synchronize()
    assert rc == 0, f"pope_conv_layer_f32 returned {rc}"


def _interior_bits(c, out, b):
    """The raw bits of image b's interior output rows."""
    Ho, Wo = K.out_grid(c)
    o_rows = (Ho + 2) * (Wo + 2)
    t = out[b * o_rows:(b + 1) * o_rows].reshape(Ho + 2, Wo + 2, -1)[1:-1, 1:-1]
    if c["out"] == "f32":
        t = t[..., :c["N"]]
    return t.contiguous().view(torch.int16 if out.dtype == torch.float16 else torch.int32)


def _run_and_check(hip_lib, dev, cu, profiler_ok, c):
    op, d = _device_operands(c, dev)
    label = K.case_id(c)
    flag = torch.full((1,), FOREIGN, dtype=torch.int32, device=dev)
    out = K.fresh_out(c, dev)
    _call(hip_lib, c, d, out, dev, flag, routed=(cu, profiler_ok, label))
    assert int(flag.item()) == FOREIGN, f"{label}: range flag {int(flag.item())} on ordinary data"
    err, frac = K.check_output(c, op, out, K.check_pixels(c, K.tile_rows(c, cu)), label)
    print(f"measured: {label}: {'+'.join(K.kernels_of(c, cu))}, max |err| {err:.3e}, max |err| / bound {frac:.3f}")
    return d, out


@pytest.mark.parametrize("c", K.SMALL_CASES, ids=K.case_id)
def test_small_cases(dev, hip_lib, cu, profiler_ok, c):
    """The smallest shapes at which each form can go wrong: ragged tiles, windows on every border, seams and tile edges mid-image,
    the 4 x 4 grid of the FPN merge (Wp = 6) and its multiply-high correction (14 x 22: Hp Wp = 384 = 3 x 128)."""
    assert "wide" not in K.kernels_of(c, cu)
    _run_and_check(hip_lib, dev, cu, profiler_ok, c)


def _image_by_image(hip_lib, dev, cu, profiler_ok, c, d, out):
    """Every image of a call on a 256-row route equals its stand-alone result (below the switch) bit for bit on interior rows."""
    alone = K.fresh_out(c, dev)
    for b in range(c["n"]):
        one = dict(c, n=1)
        assert "wide" not in K.kernels_of(one, cu)
        _call(hip_lib, c, d, alone, dev, img=b, routed=(cu, profiler_ok, f"image {b} alone: {K.case_id(c)}") if b == 0 else None)
        assert torch.equal(_interior_bits(c, out, b), _interior_bits(c, alone, b)), f"{K.case_id(c)}: image {b} differs from its stand-alone result"


@pytest.mark.parametrize("i", range(12))
def test_conv3_at_the_wide_switch(dev, hip_lib, cu, profiler_ok, i):
    """ceil(M / 256) ceil(N / bn) = CUs - 1 (tile kernel) and = CUs (256-row LDS-direct kernel, 128- and 256-column tiles)."""
    c = K.conv3_switch_cases(cu)[i]
    wide = bool(i & 1)
    assert (K.kernels_of(c, cu)[0] == "wide") == wide and K.wide_tiles(c) == cu - 1 + wide
    d, out = _run_and_check(hip_lib, dev, cu, profiler_ok, c)
    if wide:
        _image_by_image(hip_lib, dev, cu, profiler_ok, c, d, out)


@pytest.mark.parametrize("i", range(8))
def test_conv_s2_at_the_implicit_switch(dev, hip_lib, cu, profiler_ok, i):
    """Three images of a non-square grid just below the switch (gather_s2 + tile kernel) and just at it (CONV = 2: the per-lane row
    base from b, yo, xo); the implicit route equals the gathered one bit for bit on interior rows."""
    c = K.s2_switch_cases(cu)[i]
    wide = bool(i & 1)
    assert (K.kernels_of(c, cu)[0] == "wide") == wide
    d, out = _run_and_check(hip_lib, dev, cu, profiler_ok, c)
    if wide:
        _image_by_image(hip_lib, dev, cu, profiler_ok, c, d, out)


def _flag_cases(cu):
    """One planes-output call per form and route, and the fp32-output forms."""
    return [K.SMALL_CASES[0],                                                       # CONV3 tile16 -> planes
            K.case(K.CONV3, K.F16X3, 2, 5, 7, 1, 196, "f32", False, 1.0),            # -> fp32: no report
            K.case(K.CONV3, K.F16, 2, 5, 5, 4, 256, "f32", False, 1.0),
            K.case(K.CONV_S2, K.F16X3, 2, 6, 10, 4, 196, "planes", False, 1.0, taps=1),
            K.case(K.CONV1_UP, K.F16X3, 2, 4, 6, 4, 196, "planes", False, 1.0),
            K.case(K.STEM, K.F16X3, 2, 8, 12, 0, 128, "planes", False, 0.0),
            K.conv3_switch_cases(cu)[1], K.s2_switch_cases(cu)[1]]                   # the 256-row routes


@pytest.mark.parametrize("i", range(8))
def test_range_flag(dev, hip_lib, cu, profiler_ok, i):
    """On a zero operand the output is act(bias): one bias entry of 8190 (x 8 = 65520, the first magnitude that rounds to f16
    infinity) raises POPE_RANGE_INPUT from a planes output, 8189 raises nothing, and an fp32 output reports nothing at all.  The
    flag is ORed into the word."""
    c = _flag_cases(cu)[i]
    op, d = _device_operands(c, dev)
    d = dict(d)
    for k in ("a", "img", "up_src"):
        if k in d:
            d[k] = torch.zeros_like(d[k])
    d.pop("res", None)
    c = dict(c, res=False, bias=True)
    col = c["N"] - 3
    for value in (8190.0, 8189.0):
        b = op["bias"].abs()
        b[col] = value
        d["bias"] = b.to(dev)
        flag = torch.full((1,), FOREIGN, dtype=torch.int32, device=dev)
        out = K.fresh_out(c, dev)
        _call(hip_lib, c, d, out, dev, flag, routed=(cu, profiler_ok, f"bias[{col}] = {value}: {K.case_id(c)}"))
        want = FOREIGN | (RANGE_INPUT if value == 8190.0 and c["out"] == "planes" else 0)
        assert int(flag.item()) == want, f"{K.case_id(c)}: bias {value} left the flag word at {int(flag.item())}, want {want}"
        assert bool((out[K.out_rows(c):] == (K.F16_FILL if c["out"] == "planes" else K.F32_FILL)).all())
        if value == 8189.0:      # act(bias) on every interior pixel, to the format
            Ho, Wo = K.out_grid(c)
            pix = K.all_pixels(c["n"], Ho, Wo)[:: max(1, K.out_rows(c) // 512)]
            got = K.out_values(c, out, K.pixel_rows(c, pix))[:, :c["N"]]
            wantv = b.double().expand_as(got)
            assert bool(((got - wantv).abs() <= K.bound(c, wantv)).all())
