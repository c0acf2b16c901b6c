"""Cases, operands, fp64 restatements, route mirrors and comparisons of test_gpu_conv_routes.py (host only;
test_conv_checks_cpu.py holds the restatements to torch's fp64 convolutions and shows that the comparisons reject the faults a
convolution kernel is likely to have, on this very data).

pope_conv_layer_f32 (pope_hip.h) runs ONE layer of the ResNet-FPN forward, or the SAM neck's 3x3, on the caller's buffers.  A
pixel-row tensor is NHWC over the zero-bordered grid [n, H + 2, W + 2], one pixel = one row of cch chunks of 128 bytes:
  f16x3  planes [rows, cch, 2, 32] f16, value * 8 = hi + lo     f32  [rows, 32 cch] fp32     f16  [rows, 64 cch] f16 = value * 8
weights [N, K] with tap-major columns (ky, kx, channel): planes * 256, fp32, f16 * 256.  Forms:
  CONV3     3x3 stride 1 pad 1          CONV_S2   taps 9: 3x3 stride 2 pad 1; taps 1: 1x1 stride 2
  CONV1_UP  1x1 + bilinear x2 (align_corners) of a half-resolution fp32 map       STEM   7x7 stride 2 pad 3 on the gray image
out = act(conv + bias [+ res]), act(v) = max(v, 0) + slope min(v, 0).
Every reference is fp64 on the operand values the kernel sees (planes hi + lo, the f16 values), for chosen output pixels only.
Bounds (test_gpu_gemm_routes.py): fp32 outputs of the fp32 and plain-f16 kernels 1e-5 + 1e-5 |want|; f16x3 fp32 outputs
2e-5 + 1e-5 |want|; planes outputs that plus 2^-21 |want| for the hi / lo split."""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location("gemm_routes", os.path.join(os.path.dirname(__file__), "test_gpu_gemm_routes.py"))
R = importlib.util.module_from_spec(_spec)     # F32_ATOL / F32_RTOL / PLANES_ATOL, the profiler control, _ptr, _stream
_spec.loader.exec_module(R)

CONV3, CONV_S2, CONV1_UP, STEM = 0, 1, 2, 3               # pope_hip.h POPE_CONV_*
FORM_NAME = {CONV3: "CONV3", CONV_S2: "CONV_S2", CONV1_UP: "CONV1_UP", STEM: "STEM"}
F32, F16X3, F16 = 0, 1, 2                                 # POPE_PREC_*
PREC_NAME = {F32: "f32", F16X3: "f16x3", F16: "f16"}
ACT, WSC = 8.0, 256.0                                     # POPE_PLANES_ACT_SCALE, POPE_PLANES_W_SCALE
F32_ATOL, F32_RTOL, PLANES_ATOL = R.F32_ATOL, R.F32_RTOL, R.PLANES_ATOL
SPLIT_RTOL = 2.0 ** -21                                   # a planes value is hi + lo: 22 significand bits
F32_FILL, F16_FILL = 7.0, 1234.0                          # the sentinels of test_gpu_gemm_routes.py
GUARD_ROWS = 4                                            # sentinel rows past every output buffer
UP_BORDER = 1000.0                                        # the FPN source's border is undefined in the model: a read of it shows
KERNEL = {"tile16": "gemm_planes16_kernel", "wide": "gemm_plain256_kernel", "f32": "gemm_nt_f32_kernel",
          "border": "zero_border_kernel", "gather": "gather_s2_kernel", "stem": "stem_gather_kernel"}


def _cdiv(a, b):
    return -(-a // b)


def _up32(v):
    return (v + 31) // 32 * 32


# ---- cases ------------------------------------------------------------------------------------------------------------------
def case(form, prec, n, H, W, cch, N, out="planes", res=False, slope=0.0, taps=0, bias=True, ldc=None, border=None):
    """H, W: the interior of the INPUT grid (STEM: the image).  ldc: N rounded up to 32 unless given (fp32 outputs only)."""
    c = dict(form=form, prec=prec, n=n, H=H, W=W, cch=cch, N=N, out=out, res=res, slope=slope, taps=taps, bias=bias)
    c["ldc"] = _up32(N) if ldc is None else ldc
    # the border pass: every planes output but the stride-2 shortcut (block_s2's `s`), and the stem; fp32 outputs keep theirs
    c["border"] = (out == "planes" and not (form == CONV_S2 and taps == 1)) or form == STEM if border is None else border
    return c


def case_id(c):
    s = f"{FORM_NAME[c['form']]}-{PREC_NAME[c['prec']]}-n{c['n']}-{c['H']}x{c['W']}-cch{c['cch']}-N{c['N']}-{c['out']}"
    if c["taps"]:
        s += f"-taps{c['taps']}"
    if c["res"]:
        s += "-res"
    if c["out"] == "f32" and c["ldc"] != _up32(c["N"]):
        s += f"-ldc{c['ldc']}"
    return s + f"-slope{c['slope']:g}"


def out_grid(c):
    """(Ho, Wo): the interior of the output grid."""
    return (c["H"], c["W"]) if c["form"] in (CONV3, CONV1_UP) else (c["H"] // 2, c["W"] // 2)


def out_rows(c):
    Ho, Wo = out_grid(c)
    return c["n"] * (Ho + 2) * (Wo + 2)


def in_channels(c):
    """Real columns of an operand row."""
    return 1 if c["form"] == STEM else (64 if c["prec"] == F16 else 32) * c["cch"]


def kdim(c):
    """Columns of a weight row."""
    if c["form"] == STEM:
        return 64
    return {CONV3: 9, CONV_S2: c["taps"], CONV1_UP: 1}[c["form"]] * in_channels(c)


def gemm_m(c):
    """Rows of the layer's GEMM: CONV3 leaves the last 2 Wp + 2 pixel rows out (output row R is pixel R + Wp + 1)."""
    return out_rows(c) - (2 * (c["W"] + 2) + 2 if c["form"] == CONV3 else 0)


# The small cases: the smallest at which each thing can go wrong.
def _conv3_small():
    cs = []
    # every (cch, N) pair; output, shortcut and slope rotate so that every cch and every N meets both outputs, the shortcut and
    # more than one slope
    variants = [("planes", False, 0.0), ("f32", False, 1.0), ("planes", True, 0.01), ("planes", True, 0.0), ("f32", False, 0.01),
                ("planes", False, 1.0)]
    for (n, H, W) in ((2, 5, 7), (3, 14, 18)):      # one ragged tile, every window on a border | tile edges and seams mid-tile
        for ci, cch in enumerate((1, 4, 7, 8)):
            for ni, N in enumerate((128, 196, 256)):
                out, res, slope = variants[(ci + 2 * ni) % 6]
                cs.append(case(CONV3, F16X3, n, H, W, cch, N, out, res, slope))
    cs.append(case(CONV3, F16X3, 3, 14, 18, 7, 196, "f32", False, 1.0, ldc=196))     # an fp32 pitch that is no multiple of 32
    cs.append(case(CONV3, F16X3, 2, 5, 7, 4, 128, "planes", False, 0.0, bias=False))
    for prec in (F32, F16):     # the fp32 LOAD_CONV loader and the SAM neck's form (cch 4, N 256, no bias, identity)
        cs.append(case(CONV3, prec, 2, 5, 5, 4, 256, "f32", False, 1.0, bias=False))
        cs.append(case(CONV3, prec, 1, 64, 64, 4, 256, "f32", False, 1.0, bias=False))
    cs.append(case(CONV3, F32, 2, 5, 7, 7, 196, "f32", True, 0.0, ldc=224, border=True))   # the fp32 mode's block conv: shortcut, border pass
    return cs


def _s2_small():
    return [case(CONV_S2, F16X3, 2, 6, 10, cch, N, "planes", False, slope, taps=taps)
            for taps, slope in ((9, 0.0), (1, 1.0)) for cch, N in ((4, 128), (4, 196), (7, 256))]


def _up_small():
    cs = []
    for cch, N in ((7, 256), (4, 196)):             # (K, N, up_lds) = (224, 256, 256) and (128, 196, 224)
        for n, H, W in ((2, 4, 4), (2, 4, 6), (2, 6, 4), (3, 36, 50), (3, 14, 22)):
            cs.append(case(CONV1_UP, F16X3, n, H, W, cch, N, "planes", False, 1.0))
    return cs


def _stem_small():
    return [case(STEM, prec, n, H, W, 0, 128, "planes" if prec == F16X3 else "f32", False, 0.0)
            for prec in (F16X3, F32) for n, H, W in ((2, 4, 4), (2, 8, 12), (1, 64, 96))]


SMALL_CASES = _conv3_small() + _s2_small() + _up_small() + _stem_small()


# The switch cases, from the CU count: `tiles >= cu` sends CONV3 and CONV_S2 to the 256-row LDS-direct kernels.
WIDE_W = 62                                          # Wp = 64


def conv3_switch_cases(cu):
    """n = 2 images of H x 62: M = 128 Hp - 130, so Hp = 2 cu gives ceil(M / 256) = cu and Hp = 2 cu - 2 gives cu - 1."""
    cs = []
    for cch, N, out, res, slope in ((1, 128, "planes", True, 0.0), (1, 128, "f32", False, 1.0), (1, 196, "planes", False, 0.01),
                                    (1, 196, "f32", False, 1.0), (7, 256, "planes", True, 0.0), (7, 256, "f32", False, 1.0)):
        for hp in (2 * cu - 2, 2 * cu):
            cs.append(case(CONV3, F16X3, 2, hp - 2, WIDE_W, cch, N, out, res, slope))
    return cs


S2_WO = 30                                           # Wpo = 32, Wpi = 62


def s2_switch_cases(cu):
    """n = 3 images, output grid Ho x 30 (Hpo != Wpo): M = 96 Hpo; the smallest Hpo with ceil(M / 256) >= cu and the one below."""
    hpo = next(h for h in range(3, 1 << 20) if _cdiv(3 * h * (S2_WO + 2), 256) >= cu)
    cs = []
    for taps, slope in ((9, 0.0), (1, 1.0)):
        for cch, N in ((2, 128), (4, 196)):          # 128- and 256-column tiles; the input tensor is four times the output's rows
            for h in (hpo - 1, hpo):
                cs.append(case(CONV_S2, F16X3, 3, 2 * (h - 2), 2 * S2_WO, cch, N, "planes", False, slope, taps=taps))
    return cs


# ---- Python mirrors of the routers -----------------------------------------------------------------------------------------
def wide_tiles(c):
    """gemm_plain.hip: 256-row tiles, 128 columns for N <= 128, else 256."""
    return _cdiv(gemm_m(c), 256) * _cdiv(c["N"], 128 if c["N"] <= 128 else 256)


def wide_conv_supported(c, cu):
    """gemm_plain.hip pope_wide_conv_supported for the calls the entry makes."""
    return c["form"] == CONV3 and c["prec"] == F16X3 and c["N"] <= 256 and c["ldc"] % 32 == 0 and wide_tiles(c) >= cu


def wide_conv_s2_supported(c, cu):
    """gemm_plain.hip pope_wide_conv_s2_supported for the calls the entry makes (Wpi >= 4, Hpi >= 4, Hpo, Wpo >= 3 always hold)."""
    return c["form"] == CONV_S2 and c["prec"] == F16X3 and c["N"] <= 256 and wide_tiles(c) >= cu


def kernels_of(c, cu):
    """The kernel sequence of a call, as keys of KERNEL."""
    border = ["border"] if c["border"] else []
    if c["prec"] == F32:
        return (["stem"] if c["form"] == STEM else []) + ["f32"] + border
    if c["form"] == CONV3:
        return ["wide" if wide_conv_supported(c, cu) else "tile16"] + border
    if c["form"] == CONV_S2:
        return (["wide"] if wide_conv_s2_supported(c, cu) else ["gather", "tile16"]) + border
    if c["form"] == CONV1_UP:
        return ["tile16"] + border
    return ["stem", "tile16"] + border


def tile_rows(c, cu):
    return 256 if "wide" in kernels_of(c, cu) else 128


# ---- operands ---------------------------------------------------------------------------------------------------------------
def to_planes(t, scale):
    """pope_amd._lib.to_planes: [rows, cols] -> f16 [rows, cols / 32, 2, 32], t * scale = hi + lo."""
    ts = t.float() * scale
    hi = ts.half()
    lo = (ts - hi.float()).half()
    r, cols = t.shape
    return torch.stack([hi.view(r, cols // 32, 32), lo.view(r, cols // 32, 32)], dim=2).contiguous()


def from_planes(pl, scale):
    """fp64 values of a planes tensor [rows, chunks, 2, 32] -> [rows, 32 chunks]."""
    return (pl[:, :, 0].double() + pl[:, :, 1].double()).reshape(pl.shape[0], -1) / scale


def bordered(x):
    """[n, H, W, C] -> [n (H + 2) (W + 2), C] with a zero border."""
    return F.pad(x, (0, 0, 1, 1, 1, 1)).reshape(-1, x.shape[-1])


def _seed(c):
    return hash((c["form"], c["n"], c["H"], c["W"], c["cch"], c["N"], c["taps"])) % (1 << 31)


_OPERANDS = {}


def operands(c):
    """Host tensors of a case, cached.  Buffers as the entry takes them: a, w, bias, res, up_src, img; and the fp64 values the
    kernel sees: x64 [n, H, W, C], w64 [N, K], res64 [rows_out, N], up64 [n, Hs, Ws, N].  Activations N(0, 1), weights N(0, 1 / K)."""
    key = case_id(c)
    if key in _OPERANDS:
        return _OPERANDS[key]
    if len(_OPERANDS) > 2:
        _OPERANDS.clear()
    g = torch.Generator().manual_seed(_seed(c))
    n, H, W, N, prec = c["n"], c["H"], c["W"], c["N"], c["prec"]
    C, K = in_channels(c), kdim(c)
    op = {}
    x = torch.randn(n, H, W, C, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    if c["form"] == STEM:
        op["img"] = x[..., 0].contiguous()
        op["x64"] = x.double()
    elif prec == F16X3:
        op["a"] = to_planes(bordered(x), ACT)
        op["x64"] = from_planes(op["a"], ACT).reshape(n, H + 2, W + 2, C)[:, 1:-1, 1:-1]
    elif prec == F16:
        op["a"] = (bordered(x) * ACT).half()
        op["x64"] = (op["a"].double() / ACT).reshape(n, H + 2, W + 2, C)[:, 1:-1, 1:-1]
    else:
        op["a"] = bordered(x)
        op["x64"] = x.double()
    if prec == F16X3:
        op["w"] = to_planes(w, WSC)
        op["w64"] = from_planes(op["w"], WSC)
    elif prec == F16:
        op["w"] = (w * WSC).half()
        op["w64"] = op["w"].double() / WSC
    else:
        op["w"], op["w64"] = w, w.double()
    op["bias"] = torch.randn(N, generator=g)
    if c["res"]:      # the shortcut, over all rows of the output grid (its border rows are arbitrary: the output's are zeroed)
        r = torch.randn(out_rows(c), c["ldc"], generator=g) * 2.0
        op["res"] = r if prec == F32 else to_planes(r, ACT)
        op["res64"] = (r.double() if prec == F32 else from_planes(op["res"], ACT))[:, :N]
    if c["form"] == CONV1_UP:
        Hs, Ws, lds = H // 2, W // 2, c["ldc"]
        s = torch.randn(n, Hs, Ws, lds, generator=g) * 2.0
        op["up_src"] = F.pad(s, (0, 0, 1, 1, 1, 1), value=UP_BORDER).reshape(-1, lds)
        op["up64"] = s[..., :N].double()
    _OPERANDS[key] = op
    return op


# ---- fp64 restatements ------------------------------------------------------------------------------------------------------
def all_pixels(n, Ho, Wo):
    b, y, x = torch.meshgrid(torch.arange(n), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    return torch.stack([b.reshape(-1), y.reshape(-1), x.reshape(-1)], 1)


def patches64(x64, pix, k, stride, pad, fault=None):
    """The k x k windows of the output pixels `pix` [(b, y, x)] over x64 [n, H, W, C] (zero padded), tap-major (ky, kx, c):
    [P, k k C].  fault plants what a loader may get wrong."""
    n, H, W, C = x64.shape
    extra = 2
    xp = F.pad(x64, (0, 0, pad, pad + extra, pad, pad + extra))
    if fault == "seam":          # the padding rows below / above an image hold the first / last row of the next / previous one
        xp[:, pad + H, pad:pad + W] = x64[(torch.arange(n) + 1) % n, 0]
        xp[:, pad - 1, pad:pad + W] = x64[(torch.arange(n) - 1) % n, H - 1]
    b, y, x = pix[:, 0], pix[:, 1], pix[:, 2]
    wo_last = (W + 2 * pad - k) // stride
    cols = []
    for ky in range(k):
        for kx in range(k):
            ty, tx = (kx, ky) if fault == "transpose" else (ky, kx)
            iy, ix = stride * y + ty, stride * x + tx
            if fault == "shift_right" and kx == k - 1:
                ix = torch.where(x == wo_last, ix - 1, ix)
            if fault == "pad2":
                iy, ix = iy + 1, ix + 1
            cols.append(xp[b, iy, ix])
    p = torch.stack(cols, 1)                                  # [P, taps, C]
    if fault == "chunk_major":                                # [chunk][tap][32] where the weights are [tap][chunk][32]
        p = p.reshape(p.shape[0], k * k, C // 32, 32).permute(0, 2, 1, 3)
    return p.reshape(p.shape[0], -1)


def bilinear64(src64, pix, H, W, fault=None):
    """upsample_bilinear2d(align_corners=True) x2 at the output pixels `pix` of an H x W grid: source indices and weights in
    fp32 as torch computes them (scale (in - 1) / (out - 1), int(ry), clamp at the last row / column), blend in fp64."""
    n, Hs, Ws, C = src64.shape
    f = np.float32

    def axis(coord, size_in, size_out, clamp_fault):
        if fault == "scale":
            scale = f(size_in) / f(size_out)
        else:
            scale = f(size_in - 1) / f(size_out - 1) if size_out > 1 else f(0)
        r = (scale * coord.numpy().astype(np.float32)).astype(np.float32)
        i0 = r.astype(np.int64)
        last = size_in - (2 if clamp_fault else 1)
        i1 = i0 + (i0 < last)
        l1 = (r - i0.astype(np.float32)).astype(np.float32)
        l0 = (f(1) - l1).astype(np.float32)
        return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l0).double()[:, None], torch.from_numpy(l1).double()[:, None]

    b, y, x = pix[:, 0], pix[:, 1], pix[:, 2]
    y0, y1, ly0, ly1 = axis(y, Hs, H, False)
    x0, x1, lx0, lx1 = axis(x, Ws, W, fault == "x1_clamp")
    return ly0 * (lx0 * src64[b, y0, x0] + lx1 * src64[b, y0, x1]) + ly1 * (lx0 * src64[b, y1, x0] + lx1 * src64[b, y1, x1])


def act64(v, slope, fault=None):
    if fault == "slope_pos":
        return v.clamp(min=0) * slope + v.clamp(max=0)
    return v.clamp(min=0) + slope * v.clamp(max=0)


def pixel_rows(c, pix):
    """Rows of the output pixel-row tensor that hold the interior pixels `pix`."""
    Ho, Wo = out_grid(c)
    return (pix[:, 0] * (Ho + 2) + pix[:, 1] + 1) * (Wo + 2) + pix[:, 2] + 1


def ref64(c, op, pix, fault=None):
    """fp64 result of the case at the output pixels `pix`: [P, N]."""
    form = c["form"]
    k, stride, pad = {CONV3: (3, 1, 1), CONV1_UP: (1, 1, 0), STEM: (7, 2, 3)}.get(form, (3, 2, 1) if c["taps"] == 9 else (1, 2, 0))
    p = patches64(op["x64"], pix, k, stride, pad, fault)
    if form == STEM:
        p = F.pad(p, (0, 64 - p.shape[1]))                    # 49 taps, zero-filled to two chunks
    v = p @ op["w64"].T
    if c["bias"]:
        v = v + op["bias"].double()
    if c["res"] and fault != "no_res":
        v = v + op["res64"][pixel_rows(c, pix)]
    if form == CONV1_UP:
        v = v + bilinear64(op["up64"], pix, c["H"], c["W"], fault)
    return act64(v, c["slope"], fault)


# ---- what is compared -------------------------------------------------------------------------------------------------------
def check_pixels(c, tile):
    """Interior output pixels compared against fp64: the first and the last row tile of the GEMM in full, every pixel within
    one pixel row of an image seam (y = 0 and y = Ho - 1 of every image), and 48 rows in between."""
    Ho, Wo = out_grid(c)
    hp, wp = Ho + 2, Wo + 2
    rows = out_rows(c)
    if rows <= 4096:
        return all_pixels(c["n"], Ho, Wo)
    shift = wp + 1 if c["form"] == CONV3 else 0               # GEMM row R is pixel row R + shift
    m = gemm_m(c)
    last0 = (m - 1) // tile * tile
    r = torch.cat([torch.arange(0, min(tile, m)), torch.arange(last0, m), torch.linspace(tile, max(tile, last0 - 1), 48).long()]) + shift
    b, rem = r // (hp * wp), r % (hp * wp)
    y, x = rem // wp - 1, rem % wp - 1
    keep = (y >= 0) & (y < Ho) & (x >= 0) & (x < Wo)
    pix = torch.stack([b, y, x], 1)[keep]
    bs, ys, xs = torch.meshgrid(torch.arange(c["n"]), torch.tensor([0, Ho - 1]), torch.arange(Wo), indexing="ij")
    seam = torch.stack([bs.reshape(-1), ys.reshape(-1), xs.reshape(-1)], 1)
    return torch.unique(torch.cat([pix, seam]), dim=0)


def bound(c, want):
    atol = PLANES_ATOL if c["prec"] == F16X3 else F32_ATOL
    rtol = F32_RTOL + (SPLIT_RTOL if c["out"] == "planes" else 0.0)
    return atol + rtol * want.abs()


def fresh_out(c, device="cpu"):
    """Sentinel-filled output buffer with GUARD_ROWS rows past its end."""
    rows = out_rows(c) + GUARD_ROWS
    if c["out"] == "planes":
        return torch.full((rows, c["ldc"] // 32, 2, 32), F16_FILL, dtype=torch.float16, device=device)
    return torch.full((rows, c["ldc"]), F32_FILL, device=device)


def out_values(c, out, rows):
    """fp64 values of rows `rows` of an output buffer: [len(rows), ldc]."""
    sel = out[rows.to(out.device)].cpu()
    return from_planes(sel, ACT) if c["out"] == "planes" else sel.double()


def border_mask(c):
    Ho, Wo = out_grid(c)
    m = torch.ones(c["n"], Ho + 2, Wo + 2, dtype=torch.bool)
    m[:, 1:-1, 1:-1] = False
    return m.reshape(-1)


def check_output(c, op, out, pix, what):
    """The whole comparison of one call's output buffer (host or device); returns (max |err|, max |err| / bound).
      - fp64 parity at `pix`
      - guard rows untouched
      - border pass: every border pixel's row exactly zero, all ldc columns
      - planes: the padding columns N .. ldc exactly zero on every row the layer writes; fp32: untouched on interior rows."""
    N, ldc, rows = c["N"], c["ldc"], out_rows(c)
    fill = F16_FILL if c["out"] == "planes" else F32_FILL
    assert bool((out[rows:] == fill).all()), f"{what}: rows past the output written"
    want = ref64(c, op, pix)
    got = out_values(c, out, pixel_rows(c, pix))
    err, allowed = (got[:, :N] - want).abs(), bound(c, want)
    bad = ~(err <= allowed)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bounds, max |err| {float(err.max()):.3e}, "
                                 f"first bad (pixel, col) {tuple(pix[bad.nonzero()[0, 0]].tolist())}, {int(bad.nonzero()[0, 1])}: |err| "
                                 f"{float(err[bad][0]):.3e} > {float(allowed[bad][0]):.3e}")
    host = out[:rows].cpu()
    whole = host.reshape(rows, -1)
    bm = border_mask(c)
    if c["border"]:
        nz = (whole[bm] != 0).any(1)
        assert not bool(nz.any()), f"{what}: {int(nz.sum())} border rows not zero, first at border row index {int(nz.nonzero()[0])}"
    if ldc > N:
        if c["out"] == "planes":
            written = torch.ones(rows, dtype=torch.bool) if c["border"] or c["form"] != CONV3 else ~bm
            pad = host[written].reshape(-1, ldc // 32, 2, 32)[:, N // 32:, :, :]
            pad = pad[:, 0, :, N % 32:] if N % 32 else pad
            assert bool((pad == 0).all()), f"{what}: {int((pad != 0).sum())} non-zero halves in the padding columns {N} .. {ldc}"
        else:
            pad = whole[~bm][:, N:]
            assert bool((pad == F32_FILL).all()), f"{what}: fp32 columns {N} .. {ldc} written"
    return float(err.max()), float((err / allowed).max())


def stored(c, op, fault=None):
    """The output buffer a kernel with no error but the format's would leave (host): the fp64 result of every interior pixel in
    the output format, zero border rows (where the layer has the pass), zero padding columns, sentinel guard rows.  fault plants
    what an epilogue or the border pass may get wrong."""
    Ho, Wo = out_grid(c)
    pix = all_pixels(c["n"], Ho, Wo)
    rows, N, ldc = out_rows(c), c["N"], c["ldc"]
    full = torch.zeros(rows, ldc, dtype=torch.float64)
    if not c["border"]:
        full[:, :N] = 0.37                                    # undefined border rows: anything
    full[pixel_rows(c, pix), :N] = ref64(c, op, pix, fault)
    if fault == "pad_nonzero":
        full[pixel_rows(c, pix)[len(pix) // 2], N] = 2.0 ** -10
    if fault == "border_row":                                 # one border row left as the GEMM wrote it
        full[int(border_mask(c).nonzero()[-2]), :N] = 0.25
    out = fresh_out(c)
    if c["out"] == "planes":
        out[:rows] = to_planes(full.float(), ACT)
    else:
        if c["border"]:
            out[:rows][border_mask(c)] = 0.0                  # the pass zeroes whole rows, the columns past N included
        out[:rows, :N] = full[:, :N].float()
    return out
