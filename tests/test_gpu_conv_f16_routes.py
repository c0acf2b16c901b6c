"""GPU: every layer form of the plain-f16 ResNet-FPN (precision="f16"), one layer at a time through pope_conv_layer_f16, against fp64.

The entry runs one layer's launch sequence of pope_launch_resnetfpn (conv.hip, conv_layer.h) with POPE_PREC_F16 on the caller's
buffers: activations are f16 rows (value * 8) over the zero-bordered grid, one chunk = 64 columns; weights f16 rows (value * 256),
tap-major; one f16 MFMA per product, fp32 accumulation (gemm_planes16_kernel<EPI_CONV / EPI_CONV_UP, .., PLAIN>).  An f16 output is
rounded once, f16(act(acc + bias [+ res]) * 8), with the shortcut read as f16 rows.  The cases are conv_checks.py's small cases
restated for 64-column chunks; operands, the fp64 restatements and the check pixels are conv_checks.py's, the bounds
gemm_f16_checks.py's:
    fp32 outputs    1e-5 + 1e-5 |want|                                 (the project's constant)
    f16 outputs     ulp_f16(8 want) / 2 + 8 (1e-5 + 1e-5 |want|)       (one rounding of the stored value)
Also checked: padding columns (196 -> 256) exactly zero, border rows zero where the form zeroes them, the sentinel rows past every
output untouched, and the range flag: up for a value of 9000 (x 8 leaves f16), down otherwise."""
import ctypes as C

import pytest
import torch

import conv_checks as K
import gemm_f16_checks as G
from loftr_f16_checks import up64

R = K.R
pytestmark = pytest.mark.gpu

RANGE_INPUT = 32                        # pope_hip.h POPE_RANGE_INPUT
FOREIGN = 4                             # a bit no convolution reports, pre-set in the flag word

dev = R.dev                             # module-scoped fixture of test_gpu_gemm_routes.py


def _conv3_cases():
    # every (chunks, N) pair on both grids; output, shortcut and slope rotate so that every chunk count and every N meets both
    # outputs, the shortcut on both, and the three slopes
    variants = [("planes", False, 0.0), ("f32", False, 1.0), ("planes", True, 0.01), ("planes", True, 0.0), ("f32", True, 0.01),
                ("planes", False, 1.0)]
    cs = []
    for gi, (n, H, W) in enumerate(((2, 5, 7), (3, 14, 18))):
        for ci, cch in enumerate((1, 2, 4)):
            for ni, N in enumerate((128, 196, 256)):
                out, res, slope = variants[(ci + 2 * ni + 3 * gi) % 6]
                cs.append(K.case(K.CONV3, K.F16, n, H, W, cch, N, out, res, slope))
    cs.append(K.case(K.CONV3, K.F16, 2, 5, 7, 2, 128, "planes", False, 0.0, bias=False))
    return cs


def _s2_cases():
    return [K.case(K.CONV_S2, K.F16, 2, 6, 10, cch, N, "planes", False, slope, taps=taps)
            for taps, slope in ((9, 0.0), (1, 1.0)) for cch, N in ((2, 128), (2, 196), (4, 256))]


def _up_cases():
    # (2, 2, 2): Wp = 4, the smallest grid of the form (a 1 x 1 source: both scales 0); (2, 6, 10): a 3 x 5 source, odd both ways;
    # (3, 14, 22): Hp Wp = 384 = 3 x 128, the multiply-high correction of the epilogue's pixel decomposition
    return [K.case(K.CONV1_UP, K.F16, n, H, W, cch, N, "planes", False, 1.0)
            for cch, N in ((4, 256), (2, 196)) for n, H, W in ((2, 2, 2), (2, 6, 10), (3, 14, 22))]


CASES = _conv3_cases() + _s2_cases() + _up_cases() + [K.case(K.STEM, K.F16, 2, 16, 24, 0, 128, "planes", False, 0.0)]


def _operands(c):
    """conv_checks.operands for the case without its shortcut (that module lays a shortcut out as planes), plus: the shortcut as
    f16 rows [rows, 2 * pitch] = value * 8 with fp64 values of what the kernel reads; the stem's image as the f16 values the
    gather makes of it, and its [N, 64] filter zero-filled to the two chunks the f16 mode's stem GEMM reads."""
    op = dict(K.operands(dict(c, res=False)))
    if c["res"]:
        g = torch.Generator().manual_seed(K._seed(c) + 1)
        r = torch.randn(K.out_rows(c), up64(c["N"]), generator=g) * 2.0
        op["res"] = (r * K.ACT).half()
        op["res64"] = (op["res"].double() / K.ACT)[:, :c["N"]]
    if c["form"] == K.STEM:
        op["x64"] = (op["img"] * K.ACT).half().double().unsqueeze(-1) / K.ACT
        op["w"] = torch.nn.functional.pad(op["w"], (0, 64))
    return op


def _fresh_out(c, device):
    rows = K.out_rows(c) + K.GUARD_ROWS
    if c["out"] == "planes":      # f16 rows, channels padded to the chunk
        return torch.full((rows, up64(c["N"])), K.F16_FILL, dtype=torch.float16, device=device)
    return torch.full((rows, c["ldc"]), K.F32_FILL, device=device)


def _call(hip_lib, c, op, out, device, flag):
    from pope_amd import _lib
    n, H, W = c["n"], c["H"], c["W"]
    stem = c["form"] == K.STEM
    d = {k: op[k].to(device) for k in ("a", "img", "w", "bias", "res", "up_src") if k in op}
    nbytes = hip_lib.pope_conv_layer_scratch_bytes(c["form"], n, H, W, c["cch"], c["taps"])
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
    p = lambda t: t.data_ptr() if t is not None else None
    f16_out = c["out"] == "planes"
    args = _lib.ConvLayerArgs(
        form=c["form"], precision=K.F16, n=n, H=H, W=W, cch=c["cch"], taps=c["taps"], a=p(d["img"] if stem else d["a"]),
        a_rows=0 if stem else n * (H + 2) * (W + 2), w=p(d["w"]), bias=p(d["bias"]) if c["bias"] else None, N=c["N"],
        ldc=up64(c["N"]) // 2 if f16_out else c["ldc"], slope=c["slope"], out_planes=p(out) if f16_out else None,
        out_f32=None if f16_out else p(out), zero_border=int(c["border"]), res=p(d.get("res")),
        ldres=up64(c["N"]) // 2 if "res" in d else 0, up_src=p(d.get("up_src")), up_lds=c["ldc"] if "up_src" in d else 0,
        scratch=p(scratch), scratch_bytes=nbytes, range_flag=p(flag))
    rc = hip_lib.pope_conv_layer_f16(C.byref(args), R._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"pope_conv_layer_f16 returned {rc}"


def _check(c, op, out, what):
    N, rows = c["N"], K.out_rows(c)
    f16_out = c["out"] == "planes"
    assert bool((out[rows:] == (K.F16_FILL if f16_out else K.F32_FILL)).all()), f"{what}: rows past the output written"
    pix = K.check_pixels(c, 128)
    want = K.ref64(c, op, pix)
    host = out[:rows].cpu()
    got = host[K.pixel_rows(c, pix)][:, :N]
    err, frac = G.check_f16(got, want, K.ACT, what) if f16_out else G.check_f32(got, want, what)
    bm = K.border_mask(c)
    if c["border"]:
        nz = (host[bm] != 0).any(1)
        assert not bool(nz.any()), f"{what}: {int(nz.sum())} border rows not zero"
    if f16_out and host.shape[1] > N:
        written = host if c["border"] or c["form"] != K.CONV3 else host[~bm]
        assert bool((written[:, N:] == 0).all()), f"{what}: non-zero halves in the padding columns {N} .. {host.shape[1]}"
    if not f16_out and host.shape[1] > N:
        assert bool((host[~bm][:, N:] == K.F32_FILL).all()), f"{what}: fp32 columns past N written"
    return err, frac


@pytest.mark.parametrize("c", CASES, ids=K.case_id)
def test_f16_layer(dev, hip_lib, c):
    op = _operands(c)
    flag = torch.full((1,), FOREIGN, dtype=torch.int32, device=dev)
    out = _fresh_out(c, dev)
    _call(hip_lib, c, op, out, dev, flag)
    assert int(flag.item()) == FOREIGN, f"{K.case_id(c)}: range flag {int(flag.item())} on ordinary data"
    err, frac = _check(c, op, out, K.case_id(c))
    print(f"measured: {K.case_id(c)}: max |err| {err:.3e} (of the stored value for f16 rows), max |err| / bound {frac:.3f}")


FLAG_CASES = [K.case(K.CONV3, K.F16, 2, 5, 7, 2, 196, "planes", False, 0.0),
              K.case(K.CONV3, K.F16, 2, 5, 7, 2, 196, "f32", False, 1.0),                 # fp32 rows: nothing is stored as f16
              K.case(K.CONV_S2, K.F16, 2, 6, 10, 2, 196, "planes", False, 1.0, taps=1),
              K.case(K.CONV1_UP, K.F16, 2, 6, 10, 2, 196, "planes", False, 1.0),
              K.case(K.STEM, K.F16, 2, 16, 24, 0, 128, "planes", False, 0.0)]


@pytest.mark.parametrize("c", FLAG_CASES, ids=K.case_id)
def test_range_flag(dev, hip_lib, c):
    """On a zero operand the output is act(bias): a bias entry of 9000 (x 8 = 72 000, past the f16 range) raises POPE_RANGE_INPUT
    from an f16 output, ORed into the word, and an fp32 output reports nothing; the stem's gather reports an image value of 9000
    itself.  8189 (x 8 = 65 512, which still rounds to 65 504) raises nothing and is stored to the format."""
    op = dict(_operands(c))
    for k in ("a", "img", "up_src"):
        if k in op:
            op[k] = torch.zeros_like(op[k])
    c = dict(c, bias=True)
    col = c["N"] - 3
    for value in (9000.0, 8189.0):
        b = op["bias"].abs()
        b[col] = value
        op["bias"] = b
        flag = torch.full((1,), FOREIGN, dtype=torch.int32, device=dev)
        out = _fresh_out(c, dev)
        _call(hip_lib, c, op, out, dev, flag)
        want = FOREIGN | (RANGE_INPUT if value == 9000.0 and c["out"] == "planes" else 0)
        assert int(flag.item()) == want, f"{K.case_id(c)}: bias {value} left the flag word at {int(flag.item())}, want {want}"
        rows = K.out_rows(c)
        assert bool((out[rows:] == (K.F16_FILL if c["out"] == "planes" else K.F32_FILL)).all())
        if value == 8189.0:
            Ho, Wo = K.out_grid(c)
            pix = K.all_pixels(c["n"], Ho, Wo)
            got = out[:rows].cpu()[K.pixel_rows(c, pix)][:, :c["N"]]
            wantv = b.double().expand(len(pix), -1)
            if c["out"] == "planes":
                G.check_f16(got, wantv, K.ACT, K.case_id(c))
            else:
                G.check_f32(got, wantv, K.case_id(c))
    if c["form"] == K.STEM:     # the image itself
        op["bias"] = op["bias"].clamp(max=1.0)
        op["img"] = op["img"].clone()
        op["img"][1, 7, 9] = 9000.0
        flag = torch.full((1,), FOREIGN, dtype=torch.int32, device=dev)
        _call(hip_lib, c, op, _fresh_out(c, dev), dev, flag)
        assert int(flag.item()) == FOREIGN | RANGE_INPUT
