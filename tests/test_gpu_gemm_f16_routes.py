"""GPU: the plain-f16 GEMM family (POPE_PREC_F16: every block Linear of the f16 ViT and SAM encoder paths) through
pope_linear_f16, on both mainloops and at both sides of their switch, against fp64.

`pope_launch_gemm_planes` sends a GemmParams::plain call to
  plain256  gemm_plain256_kernel, 256-row LDS-direct tiles    M >= 2048, N >= 256, N % 64 == 0 (K % 64 == 0, K >= 128)
  tile16    gemm_planes16_kernel<PLAIN>, 128 x 128 tiles      everything else
claimed bit-identical, with one shared epilogue code per form: BIAS -> fp32, GELU -> f16 x 8, QKV (q pre-scaled) -> f16,
LS_RES -> fp32 in place or from a [res_mod, N] table.  A Python mirror of the predicate names the route of each case and
torch.profiler confirms the kernel that ran (test_gpu_gemm_routes.py's control: numerics only when the profiler sees nothing).
Operands, references, bounds and the case table: gemm_f16_checks.py (test_gemm_f16_checks_cpu.py shows what the comparisons
reject).  Each case checks fp64 parity (first and last row tile in full, rows between sampled), the two guard rows past M, the
range flag, and on plain256 bit identity with the same rows computed in pieces on tile16.  Measured errors: profiles/gemm_f16_routes.md."""
import ctypes as C

import pytest
import torch

import gemm_f16_checks as K

R = K.R
pytestmark = pytest.mark.gpu

RANGE_QKV, RANGE_GELU = 4, 8            # pope_hip.h POPE_RANGE_*
FOREIGN = 32                            # POPE_RANGE_INPUT: a bit no GEMM epilogue reports, pre-set in the flag word
F32_FILL, F16_FILL = 7.0, 1234.0        # the sentinels of test_gpu_gemm_routes.py
PIECE = 1000                            # rows per tile16 piece: below the switch, no multiple of a tile height

dev = R.dev                             # module-scoped fixtures of test_gpu_gemm_routes.py
profiler_ok = R.profiler_ok


def test_profiler_sees_library_kernels(profiler_ok):
    """The control of the route assertions below; when it fails they check numerics only."""
    if profiler_ok is not None:
        pytest.skip(f"kernel-name assertions are off: {profiler_ok}")


def _run_routed(route, fn, profiler_ok, what):
    """Run fn (one library call); assert that every device kernel it launched is `route`'s."""
    if profiler_ok is not None:
        return fn()
    ret, names = R._device_kernels(fn)
    assert names, f"{what}: no device kernel seen"
    assert all(K.KERNEL[route] in n for n in names), f"{what}: expected {route}, ran {sorted(set(names))}"
    print(f"route confirmed: {route:8s} {what}")
    return ret


_DEVICE = {}


def _device_operands(dev, M, N, K_):
    key = (M, N, K_)
    if key not in _DEVICE:
        _DEVICE.clear()   # one shape at a time
        _DEVICE[key] = {k: v.to(dev) for k, v in K.operands(M, N, K_).items()}
    return _DEVICE[key]


def _fresh_out(dev, M, N, epi, res=None):
    """Sentinel-filled output with two guard rows; LS_RES in place: rows [0, M) hold the residual."""
    if epi in K.OUT_F16:
        return torch.full((M + 2, N), F16_FILL, dtype=torch.float16, device=dev)
    out = torch.full((M + 2, N), F32_FILL, device=dev)
    if res is not None:
        out[:M] = res
    return out


def _guard_intact(out, M):
    return bool((out[M:] == (F16_FILL if out.dtype == torch.float16 else F32_FILL)).all())


def _call(hip_lib, a, w, bias, out, M, N, K_, epi, gamma=None, res=None, res_mod=0, flag=None, routed=None):
    """One pope_linear_f16 call into rows [0, M) of `out`; routed = (route, profiler_ok, label) checks its kernel."""
    p = R._ptr
    f16 = epi in K.OUT_F16
    call = lambda: hip_lib.pope_linear_f16(p(a), p(w), p(bias), None if f16 else p(out), p(out) if f16 else None, M, N, K_, epi,
                                           p(gamma), p(res), res_mod, p(flag), R._stream())
    rc = _run_routed(routed[0], call, routed[1], routed[2]) if routed else call()
    assert rc == 0, f"pope_linear_f16 returned {rc}"


def _in_pieces(hip_lib, dev, d, bias, M, N, K_, epi, profiler_ok, step=PIECE, gamma=None, res=None, table=None):
    """The same rows in pieces of `step` < 2048 rows, each on tile16.  res: the in-place residual; table: the res_mod form (step a
    multiple of RES_MOD, so that a piece's row % RES_MOD is the whole call's)."""
    out = _fresh_out(dev, M, N, epi, res)
    for lo in range(0, M, step):
        m = min(step, M - lo)
        assert K.plain_route(m, N, K_, epi) == "tile16"
        routed = ("tile16", profiler_ok, f"piece M={m} N={N} K={K_} {K.EPI_NAME[epi]}") if lo == 0 else None
        _call(hip_lib, d["a16"][lo:], d["w16"], bias, out[lo:], m, N, K_, epi, gamma,
              table if table is not None else out[lo:] if res is not None else None, K.RES_MOD if table is not None else 0, routed=routed)
    return out


def _same_bits(a, b):
    it = torch.int16 if a.dtype == torch.float16 else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("bias_on", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_plain_f16_routes(dev, hip_lib, profiler_ok, case, bias_on):
    """The route the mirror names ran; fp64 parity within the format's bound; guard rows; no range flag on ordinary data; plain256
    equals tile16 in pieces, bit for bit.  LS_RES runs as the models run it: in place (res aliases C), non-trivial gamma."""
    epi, M, N, K_ = case
    route = K.plain_route(M, N, K_, epi)
    op, d = K.operands(M, N, K_), _device_operands(dev, M, N, K_)
    bias = d["bias"] if bias_on else None
    ls = epi == K.EPI_LS_RES
    gamma = d["gamma"] if ls else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    label = f"{K.case_id(case)} {'bias' if bias_on else 'null bias'}"
    out = _fresh_out(dev, M, N, epi, d["res"] if ls else None)
    _call(hip_lib, d["a16"], d["w16"], bias, out, M, N, K_, epi, gamma, out if ls else None, 0, flag, routed=(route, profiler_ok, label))
    torch.cuda.synchronize()
    assert _guard_intact(out, M), f"{label}: rows M, M+1 written"
    assert int(flag.item()) == 0, f"{label}: range flag {int(flag.item())} on ordinary data"
    rows = K.check_rows_of(M, route)
    want = K.ref64(op["a16"][rows], op["w16"], op["bias"] if bias_on else None, epi, op["gamma"], op["res"][rows])
    err, frac = K.check_out(out[rows.to(dev)].cpu(), want, epi, label)
    print(f"measured: {label}: {route}, max |err| {err:.3e}, max |err| / bound {frac:.3f}")
    if route == "plain256":
        small = _in_pieces(hip_lib, dev, d, bias, M, N, K_, epi, profiler_ok, gamma=gamma, res=d["res"] if ls else None)
        assert _same_bits(out, small), f"{label}: differs from tile16 in pieces"


@pytest.mark.parametrize("M,N,K_", K.RES_MOD_CASES)
def test_ls_res_table_rows(dev, hip_lib, profiler_ok, M, N, K_):
    """LS_RES with the residual from a [289, N] table (SAM's patch embed + position table): EVERY output row carries table row
    row % 289, on both mainloops; gamma = ones."""
    route = K.plain_route(M, N, K_, K.EPI_LS_RES)
    assert route == ("plain256" if M >= 2048 else "tile16")
    op, d = K.operands(M, N, K_), _device_operands(dev, M, N, K_)
    ones = torch.ones(N, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    label = f"LS_RES res_mod={K.RES_MOD} M={M} N={N} K={K_}"
    out = _fresh_out(dev, M, N, K.EPI_LS_RES)
    _call(hip_lib, d["a16"], d["w16"], d["bias"], out, M, N, K_, K.EPI_LS_RES, ones, d["table"], K.RES_MOD, flag,
          routed=(route, profiler_ok, label))
    torch.cuda.synchronize()
    assert _guard_intact(out, M), f"{label}: rows M, M+1 written"
    assert int(flag.item()) == 0
    rows = torch.arange(M)
    want = K.ref64(op["a16"], op["w16"], op["bias"], K.EPI_LS_RES, None, op["table"][rows % K.RES_MOD])
    err, frac = K.check_f32(out[:M].cpu(), want, label)
    print(f"measured: {label}: {route}, max |err| {err:.3e}, max |err| / bound {frac:.3f}")
    if route == "plain256":
        small = _in_pieces(hip_lib, dev, d, d["bias"], M, N, K_, K.EPI_LS_RES, profiler_ok, step=7 * K.RES_MOD, gamma=ones, table=d["table"])
        assert _same_bits(out, small), f"{label}: differs from tile16 in pieces"


FLAG_MS = (2049, 129)      # plain256 with a one-row last tile; tile16 with a one-row last tile


def _flag_run(hip_lib, dev, d, a16, bias, M, N, K_, epi, route, profiler_ok, what):
    flag = torch.full((1,), FOREIGN, dtype=torch.int32, device=dev)
    out = _fresh_out(dev, M, N, epi)
    _call(hip_lib, a16, d["w16"], bias, out, M, N, K_, epi, flag=flag, routed=(route, profiler_ok, what))
    torch.cuda.synchronize()
    assert _guard_intact(out, M), f"{what}: rows M, M+1 written"
    return out, int(flag.item())


@pytest.mark.parametrize("M", FLAG_MS, ids=["plain256", "tile16"])
def test_gelu_range_flag(dev, hip_lib, profiler_ok, M):
    """A bias entry of 8191 (x 8 = 65528 >= 65520, the first magnitude that rounds to f16 infinity) raises POPE_RANGE_GELU, one of
    8100 raises nothing; the flag is ORed into the word."""
    N, K_, col = 320, 128, 300      # in the ragged column tile
    route = K.plain_route(M, N, K_, K.EPI_GELU)
    op, d = K.operands(M, N, K_), _device_operands(dev, M, N, K_)
    for value, bit in ((8191.0, RANGE_GELU), (8100.0, 0)):
        b = op["bias"].clone()
        b[col] = value
        out, flag = _flag_run(hip_lib, dev, d, d["a16"], b.to(dev), M, N, K_, K.EPI_GELU, route, profiler_ok, f"GELU bias[{col}]={value} M={M}")
        assert flag == FOREIGN | bit, f"{route}: bias {value} left the flag word at {flag}, want {FOREIGN | bit}"
        if not bit:
            rows = K.check_rows_of(M, route)
            K.check_out(out[rows.to(dev)].cpu(), K.ref64(op["a16"][rows], op["w16"], b, K.EPI_GELU), K.EPI_GELU, f"{route} bias {value}")


@pytest.mark.parametrize("M", FLAG_MS, ids=["plain256", "tile16"])
def test_qkv_range_flag(dev, hip_lib, profiler_ok, M):
    """QKV rows carry no scale: a k column at 65530 raises POPE_RANGE_QKV, at 65000 nothing.  The q scale comes BEFORE the check
    and the one rounding: a q column at 65530 (x 0.18 = 11818) raises nothing and is stored finite, the rounded scaled reference.
    The columns are the first k group and the last q group: the 4-column groups at the q | k boundary."""
    N, K_ = 960, 128
    kcol, qcol = N // 3 + 1, N // 3 - 1
    route = K.plain_route(M, N, K_, K.EPI_QKV)
    op, d = K.operands(M, N, K_), _device_operands(dev, M, N, K_)
    rows = K.check_rows_of(M, route)
    for col, value, bit in ((kcol, 65530.0, RANGE_QKV), (kcol, 65000.0, 0), (qcol, 65530.0, 0)):
        b = op["bias"].clone()
        b[col] = value
        what = f"QKV bias[{col}]={value} M={M}"
        out, flag = _flag_run(hip_lib, dev, d, d["a16"], b.to(dev), M, N, K_, K.EPI_QKV, route, profiler_ok, what)
        assert flag == FOREIGN | bit, f"{route}: {what} left the flag word at {flag}, want {FOREIGN | bit}"
        if not bit:
            got = out[rows.to(dev)].cpu()
            assert bool(torch.isfinite(got).all()), what
            K.check_out(got, K.ref64(op["a16"][rows], op["w16"], b, K.EPI_QKV), K.EPI_QKV, what)


@pytest.mark.parametrize("M", FLAG_MS, ids=["plain256", "tile16"])
@pytest.mark.parametrize("epi,N,bit", [(K.EPI_GELU, 320, RANGE_GELU), (K.EPI_QKV, 960, RANGE_QKV), (K.EPI_BIAS, 320, 0)], ids=["gelu", "qkv", "bias"])
def test_nan_operand_sets_the_bit_of_the_output_form(dev, hip_lib, profiler_ok, M, epi, N, bit):
    """One f16 NaN in A makes a row of NaNs: the f16 forms report it under their bit (a maximum alone drops a NaN); the fp32
    forms convert nothing and report nothing.  Every other row is untouched."""
    K_ = 128
    route = K.plain_route(M, N, K_, epi)
    op, d = K.operands(M, N, K_), _device_operands(dev, M, N, K_)
    a16 = d["a16"].clone()
    a16[M - 1, 5] = float("nan")     # the one-row last tile
    what = f"{K.EPI_NAME[epi]} NaN in A[{M - 1}, 5] M={M}"
    out, flag = _flag_run(hip_lib, dev, d, a16, d["bias"], M, N, K_, epi, route, profiler_ok, what)
    assert flag == FOREIGN | bit, f"{route}: {what} left the flag word at {flag}, want {FOREIGN | bit}"
    assert bool(torch.isnan(out[M - 1]).all()), what
    rows = K.check_rows_of(M - 1, route)
    K.check_out(out[rows.to(dev)].cpu(), K.ref64(op["a16"][rows], op["w16"], op["bias"], epi), epi, what)
