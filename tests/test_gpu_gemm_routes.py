"""GPU: every route of the planes GEMM entry and every loader of the fp32 GEMM, at both sides of each switch, against fp64.

`pope_launch_gemm_planes` sends a planes -> planes BIAS / GELU Linear to one of three f16x3 mainloops, all claimed bit-identical:
  stream384  gemm_rowln16_kernel, 192 x 384 tiles     N & 255 != 0, N % 384 == 0, lda == ldw == K, >= 4 x CUs tiles
  wide_x3    gemm_plain256_kernel, 256 x 256 tiles    N >= 512, N % 64 == 0, >= 4 x CUs tiles
  tile16     gemm_planes16_kernel, 128 x 128 tiles    everything else (fp32 output, LS_RES, small M)
and the fp32 GEMM (`launch_linear`) picks one of three kernels:
  persistent   gemm_nt_f32_persistent_kernel          n_tiles * K <  2048 * 3 * CUs
  LOAD_BUFFER  gemm_nt_f32_kernel<EPI, 1>             n_tiles * K >= 2048 * 3 * CUs
  LOAD_GENERIC gemm_nt_f32_kernel<EPI, 0>             K % 32 != 0
Every threshold here is computed from the device's CU count; a Python mirror of the predicates names the route of each case,
and torch.profiler confirms the kernel that ran.  Each case checks fp64 parity (first and last row tile in full, rows in
between sampled), bit identity with the same rows computed in pieces on tile16 / the persistent kernel, the two guard rows
past M, and the range flag."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_GELU = 0, 1
RANGE_QKV, RANGE_GELU = 4, 8            # pope_hip.h POPE_RANGE_*
ERR_ARG = -1                            # POPE_ERR_ARG
ACT, WSC = 8.0, 256.0                   # _lib.PLANES_ACT_SCALE, _lib.PLANES_W_SCALE
TILE_ROWS = {"stream384": 192, "wide_x3": 256, "tile16": 128, "persistent": 128, "buffer": 128, "generic": 128}
KERNEL = {"stream384": "gemm_rowln16_kernel", "wide_x3": "gemm_plain256_kernel", "tile16": "gemm_planes16_kernel",
          "persistent": "gemm_nt_f32_persistent_kernel"}
F32_ATOL = F32_RTOL = 1e-5              # the bounds of test_gpu_ops.py
PLANES_ATOL = 2e-5


def _cdiv(a, b):
    return -(-a // b)


# ---- Python mirror of the routers ---------------------------------------------------------------------------------------
def planes_route(M, N, K, epi, out_planes, cu):
    """gemm_planes.hip pope_launch_gemm_planes, for the calls pope_linear_planes_f32 makes (lda = ldw = K, ldc = N)."""
    if out_planes and epi in (EPI_BIAS, EPI_GELU):
        if (N & 255) and N % 384 == 0 and _cdiv(M, 192) * (N // 384) >= 4 * cu:
            return "stream384"
        if N >= 512 and N % 64 == 0 and _cdiv(M, 256) * _cdiv(N, 256) >= 4 * cu:
            return "wide_x3"
    return "tile16"


def f32_route(M, N, K, cu):
    """gemm_f32.hip launch_linear (shapes well inside the 32-bit offset range)."""
    if K % 32:
        return "generic"
    return "buffer" if _cdiv(M, 128) * _cdiv(N, 128) * K >= 2048 * 3 * cu else "persistent"


def kernel_matches(route, name):
    if route in KERNEL:
        return KERNEL[route] in name
    # gemm_nt_f32_kernel<EPI, LOADER>: demangled "<0, 1>" or mangled "ILi0ELi1EE"
    import re
    m = re.search(r"gemm_nt_f32_kernel(?:<\s*\d+\s*,\s*(\d+)\s*>|ILi\d+ELi(\d+)E)", name)
    return bool(m) and int(m.group(1) or m.group(2)) == {"buffer": 1, "generic": 0}[route]


# ---- comparison helpers (host only; tests/test_gemm_route_checks_cpu.py shows that they reject corrupted outputs) --------
def check_rows(got, want, atol, rtol, what):
    """|got - want| <= atol + rtol |want| elementwise (want: fp64)."""
    err = (got.double() - want).abs()
    bad = err > atol + rtol * want.abs()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bounds, max |err| "
                                 f"{float(err.max()):.3e}, first bad (compared row index, col) {tuple(bad.nonzero()[0].tolist())}")


def check_rows_of(M, tile):
    """Rows compared against fp64: the first and the last (ragged) row tile in full, 48 rows in between."""
    last0 = (M - 1) // tile * tile
    rows = set(range(min(tile, M))) | set(range(last0, M))
    if last0 > tile:
        rows |= {int(r) for r in torch.linspace(tile, last0 - 1, 48).long()}
    return torch.tensor(sorted(rows))


def fp64_linear(a_rows, w, bias, epi):
    lin = F.linear(a_rows.double(), w.double(), None if bias is None else bias.double())
    return F.gelu(lin) if epi == EPI_GELU else lin


def from_planes(pl, scale):
    return (pl[:, :, 0].float() + pl[:, :, 1].float()).reshape(pl.shape[0], -1) / scale


# ---- fixtures ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cu(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ret = fn()
        torch.cuda.synchronize()
    return ret, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.fixture(scope="module")
def profiler_ok(dev, hip_lib):
    """Control: does torch.profiler see the library's device kernels at all?  (None = yes, else the reason it does not.)"""
    from pope_amd import _lib
    a, w = torch.ones(130, 64, device=dev), torch.ones(128, 64, device=dev)
    ap, wp = _lib.to_planes(a, ACT), _lib.to_planes(w, WSC)
    out = torch.empty(130, 128, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        rc, names = _device_kernels(lambda: hip_lib.pope_linear_planes_f32(
            C.c_void_p(ap.data_ptr()), C.c_void_p(wp.data_ptr()), None, C.c_void_p(out.data_ptr()), None, 130, 128, 64, 0,
            None, None, None, st))
    except Exception as e:   # the profiler itself failing is the same finding as it seeing nothing
        return f"torch.profiler raised {type(e).__name__}: {e}"
    assert rc == 0 and bool((out == 64.0).all())
    if not any(KERNEL["tile16"] in n for n in names):
        return f"torch.profiler saw no gemm_planes16_kernel launch (device events: {names[:5]})"
    return None


def test_profiler_sees_library_kernels(profiler_ok):
    """The control of the route assertions below; when it fails they check numerics only."""
    if profiler_ok is not None:
        pytest.skip(f"kernel-name assertions are off: {profiler_ok}")


def _run_routed(route, fn, profiler_ok, what):
    """Run fn (one library call); assert that every device kernel it launched belongs to `route`."""
    if profiler_ok is not None:
        return fn()
    ret, names = _device_kernels(fn)
    assert names, f"{what}: no device kernel seen"
    assert all(kernel_matches(route, n) for n in names), f"{what}: expected {route}, ran {sorted(set(names))}"
    print(f"route confirmed: {route:10s} {what}")
    return ret


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- planes GEMM: operands -------------------------------------------------------------------------------------------------
_OPERANDS = {}


def _operands(dev, M, N, K):
    """A (planes, generated on the device: up to 200k rows), W (planes) and bias, cached per shape."""
    from pope_amd import _lib
    key = (M, N, K)
    if key not in _OPERANDS:
        _OPERANDS.clear()   # one large shape at a time
        g = torch.Generator(device=dev).manual_seed(M * 7 + N * 3 + K)
        ap = _lib.to_planes(torch.randn(M, K, generator=g, device=dev) * 1.3, ACT)
        gc = torch.Generator().manual_seed(N * 5 + K)
        w = torch.randn(N, K, generator=gc) * K ** -0.5
        b = torch.randn(N, generator=gc)
        wp = _lib.to_planes(w, WSC).to(dev)
        _OPERANDS[key] = (ap, wp, from_planes(wp.cpu(), WSC), b)
    return _OPERANDS[key]


def _planes_call(hip_lib, ap, wp, bias, M, N, K, epi, out_planes, dev, flag=None, extra_rows=2, routed=None):
    """One call into rows [0, M) of a fresh sentinel-filled output with `extra_rows` guard rows; routed = (route,
    profiler_ok, label) checks the kernel of the call (the fill runs before the profiled window)."""
    if out_planes:
        out = torch.full((M + extra_rows, N // 32, 2, 32), 1234.0, dtype=torch.float16, device=dev)
        call = lambda: hip_lib.pope_linear_planes_f32(_ptr(ap), _ptr(wp), _ptr(bias), None, _ptr(out), M, N, K, epi, None,
                                                      None, _ptr(flag), _stream())
    else:
        out = torch.full((M + extra_rows, N), 7.0, device=dev)
        call = lambda: hip_lib.pope_linear_planes_f32(_ptr(ap), _ptr(wp), _ptr(bias), _ptr(out), None, M, N, K, epi, None,
                                                      None, _ptr(flag), _stream())
    rc = _run_routed(routed[0], call, routed[1], routed[2]) if routed else call()
    assert rc == 0, f"pope_linear_planes_f32 returned {rc}"
    return out


def _guard_intact(out, M, out_planes):
    tail = out[M:]
    return bool((tail == (1234.0 if out_planes else 7.0)).all())


def _tile16_piece_rows(N, cu):
    """Rows per piece such that every piece takes tile16 whatever its M."""
    cols = max(_cdiv(N, 256), N // 384 if N % 384 == 0 else 1)
    return 128 * max(1, (4 * cu - 1) // cols)


def _in_pieces(hip_lib, ap, wp, bias, M, N, K, epi, dev, cu, profiler_ok, flag=None):
    step = _tile16_piece_rows(N, cu)
    outs = []
    for lo in range(0, M, step):
        m = min(step, M - lo)
        assert planes_route(m, N, K, epi, True, cu) == "tile16"
        routed = ("tile16", profiler_ok, f"piece M={m} N={N} K={K}") if lo == 0 else None
        outs.append(_planes_call(hip_lib, ap[lo:], wp, bias, m, N, K, epi, True, dev, flag, extra_rows=0, routed=routed))
    return torch.cat(outs)


# Shapes: (M, N, K) from the CU count.  rows(t, T, +1 / -1): t tiles of T rows, the last one holding 1 row / T - 1 rows.
def _rows(t, T, ragged):
    return (t - 1) * T + (1 if ragged > 0 else T - 1)


def _big_shapes(cu):
    c4 = 4 * cu
    return [  # (name, M, N, K) — the route follows from planes_route and is asserted
        ("stream384 N=384 at 4xCU tiles exactly, K=64", _rows(c4, 192, +1), 384, 64),
        ("tile16 N=384 one tile below stream384, K=64", _rows(c4 - 1, 192, -1), 384, 64),
        ("stream384 N=1152 first row over, K=96 (3 K-steps)", _rows(_cdiv(c4, 3), 192, -1), 1152, 96),
        ("wide_x3 N=1152 one row below stream384, K=96", (_cdiv(c4, 3) - 1) * 192, 1152, 96),
        ("stream384 N=1920, K=416 (13 K-steps)", _rows(_cdiv(c4, 5), 192, +1), 1920, 416),
        ("wide_x3 N=1920 at 4xCU tiles exactly (below stream384), K=64", _rows(_cdiv(c4, 8), 256, +1), 1920, 64),
        ("tile16 N=1920 one row below wide_x3, K=64", _rows(_cdiv(c4, 8) - 1, 256, -1), 1920, 64),
        ("wide_x3 N=576 (partial column tile), K=384", _rows(_cdiv(c4, 3), 256, +1), 576, 384),
        ("wide_x3 N=1088 (partial column tile), K=96", _rows(_cdiv(c4, 5), 256, -1), 1088, 96),
        ("wide_x3 N=1536, K=1536", _rows(_cdiv(c4, 6), 256, +1), 1536, 1536),
    ]


BIG_IDS = ["s384_n384", "t16_n384_below", "s384_n1152", "wx3_n1152_below", "s384_n1920", "wx3_n1920", "t16_n1920_below",
           "wx3_n576", "wx3_n1088", "wx3_n1536"]
EXPECT = ["stream384", "tile16", "stream384", "wide_x3", "stream384", "wide_x3", "tile16", "wide_x3", "wide_x3", "wide_x3"]


def test_route_mirror_matches_the_case_table(cu):
    """The mirror names the intended route for every case, and each threshold pair straddles its switch."""
    for (what, M, N, K), want in zip(_big_shapes(cu), EXPECT):
        assert planes_route(M, N, K, EPI_BIAS, True, cu) == want, what
        assert planes_route(M, N, K, EPI_GELU, True, cu) == want, what
        assert planes_route(M, N, K, EPI_BIAS, False, cu) == "tile16", what   # fp32 output: always the tile kernel
    sh = _big_shapes(cu)
    assert _cdiv(sh[0][1], 192) == 4 * cu and _cdiv(sh[1][1], 192) == 4 * cu - 1          # exactly 4 x CUs / one fewer
    assert _cdiv(sh[5][1], 256) * 8 >= 4 * cu > _cdiv(sh[6][1], 256) * 8
    assert _cdiv(sh[2][1], 192) * 3 >= 4 * cu > _cdiv(sh[3][1], 192) * 3


@pytest.mark.parametrize("bias_on", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU], ids=["bias_epi", "gelu_epi"])
@pytest.mark.parametrize("case", range(10), ids=BIG_IDS)
def test_planes_routes_at_the_switches(dev, hip_lib, cu, profiler_ok, case, epi, bias_on):
    """planes -> planes at large M: the route the mirror names ran, fp64 parity, guard rows, no range flag on ordinary data,
    and bit identity with the same rows computed in pieces on tile16."""
    what, M, N, K = _big_shapes(cu)[case]
    route = planes_route(M, N, K, epi, True, cu)
    assert route == EXPECT[case]
    ap, wp, w_dec, b = _operands(dev, M, N, K)
    bias = b.to(dev) if bias_on else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    label = f"{what}, M={M} {'GELU' if epi else 'BIAS'} {'bias' if bias_on else 'null bias'}"
    out = _planes_call(hip_lib, ap, wp, bias, M, N, K, epi, True, dev, flag, routed=(route, profiler_ok, label))
    torch.cuda.synchronize()
    assert _guard_intact(out, M, True), f"{label}: rows M, M+1 written"
    assert int(flag.item()) == 0, f"{label}: range flag {int(flag.item())} on ordinary data"
    rows = check_rows_of(M, TILE_ROWS[route])
    want = fp64_linear(from_planes(ap[rows.to(dev)].cpu(), ACT), w_dec, b if bias_on else None, epi)
    check_rows(from_planes(out[rows.to(dev)].cpu(), ACT), want, PLANES_ATOL, 0.0, label)
    if route != "tile16":
        small = _in_pieces(hip_lib, ap, wp, bias, M, N, K, epi, dev, cu, profiler_ok)
        assert torch.equal(out[:M].view(torch.int16), small.view(torch.int16)), f"{label}: differs from tile16 in pieces"


SMALL = [  # tile16 at small M: (M, N, K, out_planes) — ragged by +1 / tile - 1, every K of the matrix
    (129, 448, 64, True), (255, 448, 96, True), (257, 1152, 416, True), (127, 1536, 1536, True), (385, 576, 384, True),
    (129, 1100, 416, False), (255, 448, 1536, False), (257, 384, 96, False), (383, 1920, 64, False), (129, 1088, 384, False),
]


@pytest.mark.parametrize("bias_on", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU], ids=["bias_epi", "gelu_epi"])
@pytest.mark.parametrize("M,N,K,out_planes", SMALL)
def test_planes_tile16_small(dev, hip_lib, cu, profiler_ok, M, N, K, out_planes, epi, bias_on):
    assert planes_route(M, N, K, epi, out_planes, cu) == "tile16"
    ap, wp, w_dec, b = _operands(dev, M, N, K)
    bias = b.to(dev) if bias_on else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    label = f"M={M} N={N} K={K} {'planes' if out_planes else 'fp32'} out {'GELU' if epi else 'BIAS'} {'bias' if bias_on else 'null bias'}"
    out = _planes_call(hip_lib, ap, wp, bias, M, N, K, epi, out_planes, dev, flag, routed=("tile16", profiler_ok, label))
    torch.cuda.synchronize()
    assert _guard_intact(out, M, out_planes), f"{label}: rows M, M+1 written"
    assert int(flag.item()) == 0
    want = fp64_linear(from_planes(ap.cpu(), ACT), w_dec, b if bias_on else None, epi)
    if out_planes:
        check_rows(from_planes(out[:M].cpu(), ACT), want, PLANES_ATOL, 0.0, label)
    else:
        check_rows(out[:M].cpu(), want, F32_ATOL, F32_RTOL, label)


FLAG_CASES = [0, 5, None]   # stream384 (N=384), wide_x3 (N=1920), tile16 at small M


@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU], ids=["bias_epi", "gelu_epi"])
@pytest.mark.parametrize("case", FLAG_CASES, ids=["stream384", "wide_x3", "tile16"])
def test_planes_range_flags(dev, hip_lib, cu, profiler_ok, case, epi):
    """A bias column at 8000 (planes limit 8190) with tiny products on a ragged M raises nothing — the rows past M that the
    tile epilogue computes from zero operands hold bias / gelu(bias) — and one outlier raises exactly the epilogue's bit, on
    every route and in the tile16 pieces alike."""
    from pope_amd import _lib
    M, N, K = (257, 384, 64) if case is None else _big_shapes(cu)[case][1:]
    route = planes_route(M, N, K, epi, True, cu)
    assert route == ("tile16" if case is None else EXPECT[case])
    ap, wp, w_dec, b = _operands(dev, M, N, K)
    # tiny products: W / 1000; one bias column near the limit, in the last column tile
    w_tiny = w_dec * 1e-3
    wp_tiny = _lib.to_planes(w_tiny, WSC).to(dev)
    big_b = b.clone()
    big_b[N - 3] = 8000.0
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = _planes_call(hip_lib, ap, wp_tiny, big_b.to(dev), M, N, K, epi, True, dev, flag,
                       routed=(route, profiler_ok, f"range flags, bias column 8000, M={M} N={N} K={K}"))
    torch.cuda.synchronize()
    assert int(flag.item()) == 0, f"{route}: flag {int(flag.item())} raised by a bias column of 8000"
    assert _guard_intact(out, M, True)
    rows = check_rows_of(M, TILE_ROWS[route])
    want = fp64_linear(from_planes(ap[rows.to(dev)].cpu(), ACT), from_planes(wp_tiny.cpu(), WSC), big_b, epi)
    check_rows(from_planes(out[rows.to(dev)].cpu(), ACT), want, PLANES_ATOL, 1e-6, f"{route} bias column 8000")
    # one outlier: a[M - 5, 7] = 3000, w[11, 7] = 3 -> an output near 9000, past the planes range
    row = ap[M - 5:M - 4].clone()
    a_row = from_planes(row.cpu(), ACT)
    a_row[0, 7] = 3000.0
    ap[M - 5:M - 4] = _lib.to_planes(a_row, ACT).to(dev)
    w_out = w_dec.clone()
    w_out[11, 7] = 3.0
    wp_out = _lib.to_planes(w_out, WSC).to(dev)
    try:
        bias = b.to(dev)
        flag.zero_()
        big = _planes_call(hip_lib, ap, wp_out, bias, M, N, K, epi, True, dev, flag,
                           routed=(route, profiler_ok, f"range flags, one outlier, M={M} N={N} K={K}"))
        torch.cuda.synchronize()
        bit = RANGE_GELU if epi == EPI_GELU else RANGE_QKV
        assert int(flag.item()) == bit, f"{route}: outlier raised {int(flag.item())}, want exactly {bit}"
        if route != "tile16":
            pflag = torch.zeros(1, dtype=torch.int32, device=dev)
            small = _in_pieces(hip_lib, ap, wp_out, bias, M, N, K, epi, dev, cu, profiler_ok, pflag)
            assert int(pflag.item()) == bit
            assert torch.equal(big[:M].view(torch.int16), small.view(torch.int16))
    finally:
        ap[M - 5:M - 4] = row   # the cached operands stay as generated


def test_planes_entry_rejections(dev, hip_lib):
    """The argument contract of pope_linear_planes_f32: each rejected call returns POPE_ERR_ARG and writes nothing."""
    from pope_amd import _lib
    M, N, K = 300, 384, 96
    g = torch.Generator().manual_seed(5)
    ap = _lib.to_planes(torch.randn(M, 416, generator=g), ACT).to(dev)          # enough rows / columns for every K below
    wp = _lib.to_planes(torch.randn(388, 416, generator=g) * 0.05, WSC).to(dev)
    b = torch.randn(388, generator=g).to(dev)
    gamma = torch.ones(N, device=dev)
    st = _stream()
    f32 = torch.full((M + 2, 388), 7.0, device=dev)
    pl = torch.full((M + 2, 416 // 32, 2, 32), 1234.0, dtype=torch.float16, device=dev)
    res = torch.full((M, N), 3.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    P = _ptr
    calls = {
        "K=32": lambda: hip_lib.pope_linear_planes_f32(P(ap), P(wp), P(b), None, P(pl), M, N, 32, 0, None, None, P(flag), st),
        "K=80": lambda: hip_lib.pope_linear_planes_f32(P(ap), P(wp), P(b), P(f32), None, M, N, 80, 0, None, None, P(flag), st),
        "N=386": lambda: hip_lib.pope_linear_planes_f32(P(ap), P(wp), P(b), P(f32), None, M, 386, K, 0, None, None, P(flag), st),
        "LS_RES to planes": lambda: hip_lib.pope_linear_planes_f32(P(ap), P(wp), P(b), None, P(pl), M, N, K, 2, P(gamma), P(res), P(flag), st),
        "LS_RES without gamma": lambda: hip_lib.pope_linear_planes_f32(P(ap), P(wp), P(b), P(f32), None, M, N, K, 2, None, P(res), P(flag), st),
        "null A": lambda: hip_lib.pope_linear_planes_f32(None, P(wp), P(b), None, P(pl), M, N, K, 1, None, None, P(flag), st),
        "null W": lambda: hip_lib.pope_linear_planes_f32(P(ap), None, P(b), P(f32), None, M, N, K, 0, None, None, P(flag), st),
        "M=0": lambda: hip_lib.pope_linear_planes_f32(P(ap), P(wp), P(b), None, P(pl), 0, N, K, 1, None, None, P(flag), st),
        "epilogue 3": lambda: hip_lib.pope_linear_planes_f32(P(ap), P(wp), P(b), P(f32), None, M, N, K, 3, None, None, P(flag), st),
    }
    for what, call in calls.items():
        assert call() == ERR_ARG, what
        torch.cuda.synchronize()
        assert bool((f32 == 7.0).all()) and bool((pl == 1234.0).all()) and bool((res == 3.0).all()), f"{what}: output written"
        assert int(flag.item()) == 0, what


# ---- fp32 GEMM: the three loaders ------------------------------------------------------------------------------------------
def _f32_shapes(cu):
    slots_k = 2048 * 3 * cu
    rt = _cdiv(slots_k, 8 * 1536)               # N = 1024 (8 column tiles), K = 1536: row tiles at the LOAD_BUFFER switch
    rt2 = _cdiv(slots_k, 9 * 416)               # N = 1100 (9 column tiles, the last ragged), K = 416
    return [  # (name, M, N, K, epi)
        ("persistent, one row of tiles below LOAD_BUFFER", _rows(rt - 1, 128, -1), 1024, 1536, EPI_BIAS),
        ("LOAD_BUFFER, first row of tiles over", _rows(rt, 128, +1), 1024, 1536, EPI_BIAS),
        ("LOAD_BUFFER, ragged N, GELU", _rows(rt2, 128, -1), 1100, 416, EPI_GELU),
        ("LOAD_GENERIC K=1000 past the LOAD_BUFFER size", _rows(_cdiv(slots_k, 9 * 1000), 128, +1), 1152, 1000, EPI_BIAS),
        ("LOAD_GENERIC K=1000 small M, GELU", 129, 384, 1000, EPI_GELU),
    ]


F32_EXPECT = ["persistent", "buffer", "buffer", "generic", "generic"]


@pytest.mark.parametrize("case", range(5), ids=["persistent", "buffer", "buffer_n1100_gelu", "generic_large", "generic_small"])
def test_f32_loaders(dev, hip_lib, cu, profiler_ok, case):
    """ops.linear(precision="f32") on each kernel of launch_linear, against fp64; a LOAD_BUFFER result equals, bit for bit,
    the same rows computed in pieces on the persistent kernel (same mainloop order, same tile_epilogue)."""
    from pope_amd import ops
    what, M, N, K, epi = _f32_shapes(cu)[case]
    route = f32_route(M, N, K, cu)
    assert route == F32_EXPECT[case], what
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, device=dev)
    gc = torch.Generator().manual_seed(K)
    w, b = torch.randn(N, K, generator=gc) * K ** -0.5, torch.randn(N, generator=gc)
    wd, bd = w.to(dev), b.to(dev)
    out = torch.full((M + 2, N), 7.0, device=dev)
    label = f"{what}: M={M} N={N} K={K}"
    _run_routed(route, lambda: ops.linear(a, wd, bd, epilogue=epi, out=out[:M], precision="f32"), profiler_ok, label)
    torch.cuda.synchronize()
    assert bool((out[M:] == 7.0).all()), f"{label}: rows M, M+1 written"
    rows = check_rows_of(M, 128)
    check_rows(out[rows.to(dev)].cpu(), fp64_linear(a[rows.to(dev)].cpu(), w, b, epi), F32_ATOL, F32_RTOL, label)
    if route == "buffer":
        step = 128 * ((2048 * 3 * cu - 1) // (_cdiv(N, 128) * K))
        parts = []
        for lo in range(0, M, step):
            m = min(step, M - lo)
            assert f32_route(m, N, K, cu) == "persistent"
            call = lambda: ops.linear(a[lo:lo + m], wd, bd, epilogue=epi, precision="f32")
            parts.append(_run_routed("persistent", call, profiler_ok, f"piece M={m} N={N} K={K}") if lo == 0 else call())
        assert torch.equal(out[:M], torch.cat(parts)), f"{label}: LOAD_BUFFER differs from the persistent kernel"
