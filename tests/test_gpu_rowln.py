"""GPU: the LayerNorm-fused residual GEMM (gemm_rowln.hip, modes RL_LN_PLANES / RL_LN_F32, with and without RES_TABLE) against
fp64 at its edges, and bit for bit against its small-batch twin.

`pope_linear_rowln_f32` computes, for N = 384,
    x  = res + gamma * (A . W^T + bias)          fp32 residual stream (may alias res; res_mod > 0: row % res_mod of a table)
    xn = LayerNorm(x; ln_w, ln_b, eps)           activation planes, or fp32 (the final norm)
on RM x 384 row tiles (RM = 192 or 128, chosen per launch from the CU count) in a persistent stream over min(tiles, CUs)
workgroups.  The ViT runs it past the `small` switch of vit_forward.hip; below the switch it runs the twin instead:
`pope_linear_planes_f32(..., EPI_BIAS_LS_RES)` (tile16) followed by `pope_layernorm_rowln_order_f32`, claimed bit-identical.
Every threshold here is computed from the device's CU count by a Python mirror of the launcher; torch.profiler confirms the
geometry and the RES_TABLE instantiation by kernel name.  Each case checks x against fp64 computed from the decoded planes
(first and last row tile in full, rows in between sampled), xn against the fp64 LayerNorm of the kernel's own x, the two
guard rows past M, the range flag, run-to-run determinism and, for res_mod == 0, bit identity with the twin."""
import ctypes as C
import re

import pytest
import torch

from test_gpu_gemm_routes import _device_kernels, check_rows, check_rows_of, cu, dev, from_planes, profiler_ok  # noqa: F401

pytestmark = pytest.mark.gpu

RN = 384
ACT, WSC = 8.0, 256.0                   # _lib.PLANES_ACT_SCALE, _lib.PLANES_W_SCALE
RANGE_LAYERNORM = 2                     # pope_hip.h POPE_RANGE_LAYERNORM
ERR_ARG = -1                            # POPE_ERR_ARG
F16_OVERFLOW = 65520.0                  # common.h POPE_F16_OVERFLOW
X_ATOL = X_RTOL = 1e-5                  # x: the fp32-output bounds of test_gpu_ops.py / test_gpu_gemm_routes.py
# LayerNorm stage: |xn - LN64(x)| <= LN_C * 2^-24 * ((max|x - mean| + |mean|) * rstd * |ln_w| + |ln_b|) per element, LN64 the
# fp64 LayerNorm of the kernel's own x.  The |mean| term is the fp32 mean's own rounding (of order ulp(mean)), which
# (x - mean) * rstd amplifies: rows offset by 500 with a standard deviation of 0.05 carry it 10^4-fold.  Measured on one
# MI355X at <= 5.11 over every case of this file (planes and fp32 output alike; an fp32 torch two-pass LayerNorm gives 2.6);
# 16 keeps ~3x headroom.  A one-pass variance or an ignored eps exceeds it by orders of magnitude (test_rowln_checks_cpu.py).
LN_C = 16.0
MAX_M_K64 = ((1 << 32) - 512 - 1) // (RN * 4) - 192   # the largest M pope_gemm_rowln_supported accepts at K = 64


def _cdiv(a, b):
    return -(-a // b)


# ---- Python mirrors of the launcher and of the ViT's switch ---------------------------------------------------------------
def rowln_geo(M, cu):
    """gemm_rowln.hip launch_rowln: 192-row tiles when their rounds over the CUs cost no more rows than 128-row tiles'."""
    r128 = _cdiv(_cdiv(M, 128), cu) * 128
    r192 = _cdiv(_cdiv(M, 192), cu) * 192
    return 192 if r192 <= r128 else 128


def rowln_grid(M, cu):
    """launch_rowln_geo: (tile rows, tiles, workgroups, full rounds, tiles of the partial tail round, rows of the last tile)."""
    T = rowln_geo(M, cu)
    tiles = _cdiv(M, T)
    grid = min(tiles, cu)
    return T, tiles, grid, tiles // grid, tiles % grid, M - (tiles - 1) * T


def vit_small(rows, cu):
    """vit_forward.hip vit_forward_impl: below this the ViT runs the twin (tile16 LS_RES GEMM + layernorm_rowln_order)."""
    return 3 * _cdiv(rows, 128) <= 2 * cu


def geometry_flips(cu, n=3):
    """The first n values of M at which rowln_geo changes (the first M on the new side)."""
    flips, prev, M = [], rowln_geo(1, cu), 1
    while len(flips) < n:
        M += 1
        g = rowln_geo(M, cu)
        if g != prev:
            flips.append(M)
            prev = g
    return flips


def small_switch(cu):
    """The largest row count the ViT still runs on the twin."""
    return (2 * cu) // 3 * 128


# ---- fp64 references and bounds (host only; tests/test_rowln_checks_cpu.py shows that they reject wrong kernels) ---------
def fp64_residual(a, w, bias, gamma, res_rows):
    """x = res + gamma * (a . w^T + bias) in fp64 (a, w: decoded planes; bias / gamma None = 0 / 1)."""
    lin = a.double() @ w.double().T
    if bias is not None:
        lin = lin + bias.double()
    if gamma is not None:
        lin = lin * gamma.double()
    return res_rows.double() + lin


def fp64_layernorm(x, lw, lb, eps):
    """(LN(x) * lw + lb in fp64, the per-element error scale (max|x - mean| + |mean|) * rstd * |lw| + |lb|)."""
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    d = xd - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=1, keepdim=True) + eps)
    y = d * rstd * lw.double() + lb.double()
    scale = (d.abs().amax(dim=1, keepdim=True) + mean.abs()) * rstd * lw.double().abs() + lb.double().abs()
    return y, scale


def check_ln(got, x, lw, lb, eps, what, c=LN_C):
    """xn (fp32 or decoded planes) against the fp64 LayerNorm of the kernel's own x; returns the measured err / (2^-24 scale)."""
    want, scale = fp64_layernorm(x, lw, lb, eps)
    err = (got.double() - want).abs()
    unit = scale * 2.0 ** -24
    ratio = float((err / unit).nan_to_num(nan=float("inf")).max())
    bad = ~(err <= c * unit)   # (a NaN output is out of bounds too)
    assert not bool(bad.any()), (f"{what}: LayerNorm {int(bad.sum())} of {bad.numel()} elements out of bounds, max err / "
                                 f"(2^-24 scale) {ratio:.2f} > {c}, first bad {tuple(bad.nonzero()[0].tolist())}")
    return ratio


def residual_rows(res, res_mod, rows):
    return res[rows % res_mod] if res_mod else res[rows]


# ---- calls -----------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


X_SENT, PL_SENT, F32_SENT = -777.0, 1234.0, 7.0
LN_RATIOS = {}   # case -> measured LayerNorm err / (2^-24 scale), printed per case


def _ln_out(M, out_planes, device):
    if out_planes:
        return torch.full((M + 2, RN // 32, 2, 32), PL_SENT, dtype=torch.float16, device=device)
    return torch.full((M + 2, RN), F32_SENT, device=device)


def _x_buf(M, res0, alias, device):
    """x with two guard rows; with alias it starts as the residual and is passed as res too."""
    x = torch.full((M + 2, RN), X_SENT, device=device)
    if alias:
        x[:M] = res0
    return x


def rowln(hip_lib, op, M, alias, out_planes, eps, flag):
    """One pope_linear_rowln_f32 call into fresh sentinel-filled buffers: (rc, x, xn)."""
    x = _x_buf(M, op["res"], alias, op["res"].device)
    ln = _ln_out(M, out_planes, x.device)
    res = x if alias else op["res"]
    rc = hip_lib.pope_linear_rowln_f32(_ptr(op["ap"]), _ptr(op["wp"]), M, op["K"], _ptr(op["bias"]), _ptr(op["gamma"]),
                                       _ptr(res), op["res_mod"], _ptr(x), _ptr(op["lw"]), _ptr(op["lb"]), eps,
                                       _ptr(ln) if out_planes else None, None if out_planes else _ptr(ln), _ptr(flag), _stream())
    return rc, x, ln


def twin(hip_lib, op, M, alias, out_planes, eps, flag):
    """The small-batch path of the ViT: tile16 LS_RES GEMM, then layernorm_rowln_order (res_mod == 0 only)."""
    assert op["res_mod"] == 0 and op["gamma"] is not None
    x = _x_buf(M, op["res"], alias, op["res"].device)
    ln = _ln_out(M, out_planes, x.device)
    res = x if alias else op["res"]
    rc = hip_lib.pope_linear_planes_f32(_ptr(op["ap"]), _ptr(op["wp"]), _ptr(op["bias"]), _ptr(x), None, M, RN, op["K"], 2,
                                        _ptr(op["gamma"]), _ptr(res), None, _stream())   # (no range flag: as in the ViT)
    assert rc == 0, f"pope_linear_planes_f32 returned {rc}"
    rc = hip_lib.pope_layernorm_rowln_order_f32(_ptr(x), _ptr(op["lw"]), _ptr(op["lb"]), _ptr(ln) if out_planes else None,
                                                None if out_planes else _ptr(ln), M, eps, _ptr(flag), _stream())
    assert rc == 0, f"pope_layernorm_rowln_order_f32 returned {rc}"
    return x, ln


def operands(device, M, K, bias_on=True, gamma_on=True, res_mod=0, seed=0):
    """A planes [M, K] (generated on the device), W planes [384, K], bias, gamma, the residual [M or res_mod, 384], ln_w, ln_b."""
    from pope_amd import _lib
    g = torch.Generator(device=device).manual_seed(M * 7 + K + seed)
    ap = _lib.to_planes(torch.randn(M, K, generator=g, device=device) * 1.3, ACT)
    res = torch.randn(res_mod or M, RN, generator=g, device=device)
    gc = torch.Generator().manual_seed(K * 3 + seed)
    w = torch.randn(RN, K, generator=gc) * K ** -0.5
    wp = _lib.to_planes(w, WSC).to(device)
    bias = torch.randn(RN, generator=gc) if bias_on else None
    gamma = 0.5 + torch.rand(RN, generator=gc) if gamma_on else None
    lw, lb = 1.0 + 0.1 * torch.randn(RN, generator=gc), 0.1 * torch.randn(RN, generator=gc)
    on = lambda t: None if t is None else t.to(device)
    return dict(ap=ap, wp=wp, w_dec=from_planes(wp.cpu(), WSC), K=K, bias=on(bias), gamma=on(gamma), res=res, res_mod=res_mod,
                lw=on(lw), lb=on(lb))


def kernel_info(name):
    """(tile rows, mode, RES_TABLE) of a gemm_rowln16_kernel launch name (demangled or mangled), else None."""
    if "gemm_rowln16_kernel" not in name:
        return None
    m = re.search(r"RlGeo<\s*(\d+)\s*,\s*\d+\s*>\s*,\s*(\d+)\s*,\s*(true|false|1|0)\s*>", name)
    if m:
        return int(m.group(1)), int(m.group(2)), m.group(3) in ("true", "1")
    m = re.search(r"RlGeoILi(\d+)ELi\d+EEELi(\d+)ELb([01])E", name)
    return (int(m.group(1)), int(m.group(2)), m.group(3) == "1") if m else None


def run_checked(fn, geo, out_planes, table, profiler_ok, what):
    """Run one library call; with a working profiler assert that it launched exactly the intended rowln instantiation."""
    if profiler_ok is not None:
        return fn()
    ret, names = _device_kernels(fn)
    infos = [kernel_info(n) for n in names if "gemm_rowln16_kernel" in n]   # (the buffer fills are torch's)
    want = (geo, 0 if out_planes else 1, table)
    assert infos and all(i == want for i in infos), f"{what}: expected RlGeo<{geo}> mode {want[1]} table {table}, ran {names}"
    return ret


def check_case(hip_lib, op, M, alias, out_planes, eps, cu, profiler_ok, what, determinism=True, twin_check=True):
    """Every per-case check of the module docstring; returns (x, xn) of the first call."""
    geo = rowln_geo(M, cu)
    flag = torch.zeros(1, dtype=torch.int32, device=op["res"].device)
    rc, x, ln = run_checked(lambda: rowln(hip_lib, op, M, alias, out_planes, eps, flag), geo, out_planes, op["res_mod"] > 0,
                            profiler_ok, what)
    assert rc == 0, f"{what}: pope_linear_rowln_f32 returned {rc}"
    torch.cuda.synchronize()
    assert bool((x[M:] == X_SENT).all()), f"{what}: x rows M, M+1 written"
    assert bool((ln[M:] == (PL_SENT if out_planes else F32_SENT)).all()), f"{what}: LayerNorm rows M, M+1 written"
    assert int(flag.item()) == 0, f"{what}: range flag {int(flag.item())} on ordinary data"
    rows = check_rows_of(M, geo)
    rd = rows.to(x.device)
    a_dec = from_planes(op["ap"][rd].cpu(), ACT)
    cpu = lambda t: None if t is None else t.cpu()
    want_x = fp64_residual(a_dec, op["w_dec"], cpu(op["bias"]), cpu(op["gamma"]), residual_rows(op["res"], op["res_mod"], rd).cpu())
    got_x = x[rd].cpu()
    assert bool(torch.isfinite(got_x).all()), f"{what}: x not finite"   # (check_rows passes NaN)
    check_rows(got_x, want_x, X_ATOL, X_RTOL, f"{what}: x")
    got_ln = from_planes(ln[rd].cpu(), ACT) if out_planes else ln[rd].cpu()
    LN_RATIOS[what] = check_ln(got_ln, got_x, op["lw"].cpu(), op["lb"].cpu(), eps, what)
    print(f"{what}: LayerNorm err / (2^-24 scale) = {LN_RATIOS[what]:.3f}")
    if determinism:
        rc2, x2, ln2 = rowln(hip_lib, op, M, alias, out_planes, eps, flag)
        assert rc2 == 0
        assert torch.equal(x2.view(torch.int32), x.view(torch.int32)), f"{what}: x differs between two identical calls"
        assert torch.equal(ln2.view(torch.int16), ln.view(torch.int16)), f"{what}: xn differs between two identical calls"
    if twin_check and op["res_mod"] == 0:
        tflag = torch.zeros(1, dtype=torch.int32, device=x.device)
        tx, tln = twin(hip_lib, op, M, alias, out_planes, eps, tflag)
        assert torch.equal(tx[:M].view(torch.int32), x[:M].view(torch.int32)), f"{what}: x differs from the tile16 twin"
        assert torch.equal(tln[:M].view(torch.int16), ln[:M].view(torch.int16)), f"{what}: xn differs from layernorm_rowln_order"
        assert int(tflag.item()) == 0
    return x, ln


# ---- the case table ----------------------------------------------------------------------------------------------------------
def cases(cu):
    """(id, M, K, out_planes, bias, gamma, res_mod, alias, what the case is for) from the CU count."""
    f1, f2, f3 = geometry_flips(cu)
    s = small_switch(cu)
    return [
        ("m1", 1, 64, True, True, True, 0, True, "M=1"),
        ("m127", 127, 96, False, True, True, 0, False, "M=127"),
        ("m129", 129, 608, True, False, True, 1531, False, "M=129"),
        ("m191", 191, 384, False, True, False, 197, False, "M=191"),
        ("m193", 193, 1536, True, True, True, 0, False, "M=193"),
        ("small_last", s, 384, True, True, True, 0, True, "largest M of the twin side"),
        ("small_first", s + 1, 384, True, True, True, 0, True, "first M of the fused side"),
        ("flip1_lo", f1 - 1, 64, True, True, True, 0, True, "below geometry flip 1"),
        ("flip1_hi", f1, 96, False, True, True, 1531, False, "at geometry flip 1"),
        ("flip2_lo", f2 - 1, 608, True, False, True, 0, False, "below geometry flip 2"),
        ("flip2_hi", f2, 64, True, True, False, 197, False, "at geometry flip 2"),
        ("flip3_lo", f3 - 1, 96, False, True, True, 0, True, "below geometry flip 3"),
        ("flip3_hi", f3, 384, True, True, True, 1, False, "at geometry flip 3"),
        ("prod_30620", 30620, 1536, True, True, True, 0, True, "production FC2 + norm1, 20 images"),
        ("prod_97984_final", 97984, 1536, False, True, True, 0, True, "production FC2 + final norm, 64 images"),
        ("prod_97984_embed", 97984, 608, True, False, False, 1531, False, "production patch embed + norm1, 64 images"),
        ("two_rounds", 2 * cu * 192, 1536, True, True, True, 0, True, "2 x CUs tiles of 192, no tail"),
        ("three_rounds_plus1", 3 * cu * 128 + 1, 384, True, True, True, 0, True, "3 x CUs + 1 tiles of 128"),
        ("ragged128_full", 240 * 128 - 1, 96, False, False, True, 0, False, "last 128-row tile holds 127 rows"),
        ("ragged192_full", 400 * 192 - 1, 608, True, True, True, 197, False, "last 192-row tile holds 191 rows"),
        ("ragged192_one", 400 * 192 + 1, 64, False, True, False, 1531, False, "last 192-row tile holds 1 row"),
    ]


# (tile rows, side of the ViT switch) each case is meant for; a few structural claims are asserted by name below
EXPECT = {"m1": (128, "twin"), "m127": (128, "twin"), "m129": (128, "twin"), "m191": (128, "twin"), "m193": (128, "twin"),
          "small_last": (128, "twin"), "small_first": (128, "fused"), "flip1_lo": (128, "fused"), "flip1_hi": (192, "fused"),
          "flip2_lo": (192, "fused"), "flip2_hi": (128, "fused"), "flip3_lo": (128, "fused"), "flip3_hi": (192, "fused"),
          "prod_30620": (128, "fused"), "prod_97984_final": (192, "fused"), "prod_97984_embed": (192, "fused"),
          "two_rounds": (192, "fused"), "three_rounds_plus1": (128, "fused"), "ragged128_full": (128, "fused"),
          "ragged192_full": (192, "fused"), "ragged192_one": (192, "fused")}


def test_mirror_places_every_case(cu):
    """Every case sits on the intended side of its switch: geometry, tile rounds and tail, the ViT's small switch."""
    table = {c[0]: c for c in cases(cu)}
    assert set(table) == set(EXPECT)
    for name, (geo, side) in EXPECT.items():
        M = table[name][1]
        assert rowln_geo(M, cu) == geo, f"{name}: M={M} runs RlGeo<{rowln_geo(M, cu)}>"
        assert vit_small(M, cu) == (side == "twin"), f"{name}: M={M} on the wrong side of the small switch"
    f = geometry_flips(cu)
    for M in f:
        assert rowln_geo(M, cu) != rowln_geo(M - 1, cu)
    g = {n: rowln_grid(table[n][1], cu) for n in table}
    # (T, tiles, grid, full rounds, tail tiles, rows of the last tile)
    assert g["flip1_lo"][1] == cu and g["flip1_lo"][4] == 0                       # exactly one round, no tail
    assert g["two_rounds"][1] == 2 * cu and g["two_rounds"][4] == 0               # exactly two rounds
    assert g["three_rounds_plus1"][1] == 3 * cu + 1 and g["three_rounds_plus1"][5] == 1
    assert g["prod_30620"][1] < cu and g["prod_30620"][2] == g["prod_30620"][1]    # fewer tiles than CUs
    assert g["ragged128_full"][5] == 127 and g["ragged192_full"][5] == 191 and g["ragged192_one"][5] == 1
    if cu == 256:   # the MI355X: the production chunk is 2 rounds with a 255-tile tail; the flips of the issue
        assert g["prod_97984_final"][3] == 1 and g["prod_97984_final"][4] == 255
        assert f == [32769, 49153, 65537] and g["flip2_hi"][5] == 1
    assert not vit_small(small_switch(cu) + 1, cu) and vit_small(small_switch(cu), cu)
    for c in cases(cu):
        assert c[6] > 0 or c[5], f"{c[0]}: res_mod == 0 needs gamma"
        assert not (c[7] and c[6]), f"{c[0]}: x aliases the residual only for res_mod == 0"
        assert c[6] in (0, 1, 197, 1531) and (c[6] <= 1 or (192 % c[6] and 128 % c[6]))


def test_profiler_sees_library_kernels(profiler_ok):
    """The control of the kernel-name assertions; when it fails they check numerics only."""
    if profiler_ok is not None:
        pytest.skip(f"kernel-name assertions are off: {profiler_ok}")


CASE_IDS = [c[0] for c in cases(256)]


@pytest.mark.parametrize("case", range(len(CASE_IDS)), ids=CASE_IDS)
def test_rowln_case(dev, hip_lib, cu, profiler_ok, case):
    name, M, K, out_planes, bias_on, gamma_on, res_mod, alias, what = cases(cu)[case]
    op = operands(dev, M, K, bias_on, gamma_on, res_mod, seed=case)
    label = (f"{name} ({what}): M={M} K={K} {'planes' if out_planes else 'fp32'} out, {'bias' if bias_on else 'null bias'}, "
             f"{'gamma' if gamma_on else 'null gamma'}, res_mod={res_mod}{', x aliases res' if alias else ''}, "
             f"RlGeo<{rowln_geo(M, cu)}>")
    check_case(hip_lib, op, M, alias, out_planes, 1e-6, cu, profiler_ok, label)


@pytest.mark.parametrize("flip", [0, 1, 2], ids=["flip1", "flip2", "flip3"])
def test_geometries_agree(dev, hip_lib, cu, profiler_ok, flip):
    """The first M' rows of a call on one tile geometry equal, bit for bit, a call over M' rows on the other geometry."""
    M = geometry_flips(cu)[flip]
    Mp = M - 1
    assert rowln_geo(M, cu) != rowln_geo(Mp, cu)
    res_mod = 197 if flip == 1 else 0
    out_planes = flip != 1
    op = operands(dev, M, 96, True, True, res_mod, seed=40 + flip)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _, x, ln = run_checked(lambda: rowln(hip_lib, op, M, False, out_planes, 1e-6, flag), rowln_geo(M, cu), out_planes,
                           res_mod > 0, profiler_ok, f"M={M}")
    opp = dict(op, ap=op["ap"][:Mp], res=op["res"] if res_mod else op["res"][:Mp])
    _, xp, lnp = run_checked(lambda: rowln(hip_lib, opp, Mp, False, out_planes, 1e-6, flag), rowln_geo(Mp, cu), out_planes,
                             res_mod > 0, profiler_ok, f"M={Mp}")
    torch.cuda.synchronize()
    assert torch.equal(x[:Mp].view(torch.int32), xp[:Mp].view(torch.int32)), f"x: RlGeo<{rowln_geo(M, cu)}> vs <{rowln_geo(Mp, cu)}>"
    assert torch.equal(ln[:Mp].view(torch.int16), lnp[:Mp].view(torch.int16)), "xn differs between the geometries"
    assert int(flag.item()) == 0


@pytest.mark.parametrize("M,K,res_mod,out_planes", [(193, 64, 197, False), (30620, 608, 1531, True), (32769, 96, 1, True)])
def test_residual_table_equals_expanded_rows(dev, hip_lib, cu, profiler_ok, M, K, res_mod, out_planes):
    """res_mod > 0 with a null gamma equals res_mod == 0 over the table expanded row by row with gamma = ones, bit for bit."""
    op = operands(dev, M, K, True, False, res_mod, seed=50)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    geo = rowln_geo(M, cu)
    _, x, ln = run_checked(lambda: rowln(hip_lib, op, M, False, out_planes, 1e-6, flag), geo, out_planes, True, profiler_ok,
                           f"table M={M}")
    expanded = dict(op, res=op["res"][torch.arange(M, device=dev) % res_mod].contiguous(), res_mod=0,
                    gamma=torch.ones(RN, device=dev))
    _, xe, lne = run_checked(lambda: rowln(hip_lib, expanded, M, False, out_planes, 1e-6, flag), geo, out_planes, False,
                             profiler_ok, f"expanded M={M}")
    torch.cuda.synchronize()
    assert torch.equal(x[:M].view(torch.int32), xe[:M].view(torch.int32)), "x: table vs expanded rows"
    assert torch.equal(ln[:M].view(torch.int16), lne[:M].view(torch.int16)), "xn: table vs expanded rows"
    assert int(flag.item()) == 0


# ---- LayerNorm numerics ------------------------------------------------------------------------------------------------------
def numerics_operands(device, M, kind):
    """Residual rows of a given character; gamma small or zero so that x is (almost) the residual."""
    op = operands(device, M, 64, True, True, 0, seed=60)
    g = torch.Generator(device=device).manual_seed(61)
    n = torch.randn(M, RN, generator=g, device=device)
    row = torch.randn(M, 1, generator=g, device=device)
    if kind == "offset500":        # a one-pass E[x^2] - mean^2 loses every digit of the variance here
        op["res"] = 500.0 + 0.05 * n
        op["gamma"] = op["gamma"] * 1e-3
    elif kind == "constant":       # zero variance: xn = ln_b
        op["res"] = (10.0 * row).expand(M, RN).contiguous()
        op["gamma"] = torch.zeros(RN, device=device)
    elif kind == "near_eps":       # variance 1e-6, of the order of eps
        op["res"] = 0.3 * row + 1e-3 * n
        op["gamma"] = torch.zeros(RN, device=device)
    elif kind == "spread1e3":
        op["res"] = 1e3 * n
    else:
        raise ValueError(kind)
    return op


@pytest.mark.parametrize("out_planes", [True, False], ids=["planes", "fp32"])
@pytest.mark.parametrize("kind,eps", [("offset500", 1e-6), ("constant", 1e-6), ("near_eps", 1e-5), ("near_eps", 1e-6),
                                      ("spread1e3", 1e-6)], ids=["offset500", "constant", "near_eps_1e-5", "near_eps_1e-6",
                                                                 "spread1e3"])
def test_layernorm_numerics(dev, hip_lib, cu, profiler_ok, kind, eps, out_planes):
    M = 1000
    op = numerics_operands(dev, M, kind)
    label = f"LayerNorm {kind} eps={eps:g} {'planes' if out_planes else 'fp32'} M={M}"
    _, ln = check_case(hip_lib, op, M, True, out_planes, eps, cu, profiler_ok, label)
    if kind == "near_eps":         # eps reaches the kernel: the other eps gives a clearly different result
        other = 1e-6 if eps == 1e-5 else 1e-5
        _, _, ln_o = rowln(hip_lib, op, M, True, out_planes, other, None)
        torch.cuda.synchronize()
        dec = (lambda t: from_planes(t[:M].cpu(), ACT)) if out_planes else (lambda t: t[:M].cpu())
        assert float((dec(ln) - dec(ln_o)).abs().max()) > 0.1, "eps does not change the result"


# ---- range flag ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1000, 30620])
def test_range_flag_real_rows(dev, hip_lib, cu, profiler_ok, M):
    """A real row whose LayerNorm passes the planes limit raises exactly POPE_RANGE_LAYERNORM, as the twin does; so does a
    NaN in one residual row; the fp32-output mode leaves the flag word untouched."""
    c, r = 100, M - 5
    for poison in ("spike", "nan"):
        op = operands(dev, M, 64, True, True, 0, seed=70)
        lw = op["lw"].clone()
        if poison == "spike":      # normalised ~ sqrt(383) * 500 * 8 = 78 000 >= 65 520; ordinary rows stay below 20 000
            lw[c] = 500.0
            op["res"][r, c] += 400.0
        else:
            op["res"][r, 7] = float("nan")
        op["lw"] = lw
        for out_planes in (True, False):
            start = 0 if out_planes else 64
            flag = torch.full((1,), start, dtype=torch.int32, device=dev)
            tflag = torch.full((1,), start, dtype=torch.int32, device=dev)
            rc, x, ln = run_checked(lambda: rowln(hip_lib, op, M, True, out_planes, 1e-6, flag), rowln_geo(M, cu), out_planes,
                                    False, profiler_ok, f"flag {poison}")
            assert rc == 0
            twin(hip_lib, op, M, True, out_planes, 1e-6, tflag)
            torch.cuda.synchronize()
            want = RANGE_LAYERNORM if out_planes else 64
            assert int(flag.item()) == want, f"{poison} M={M} {'planes' if out_planes else 'fp32'}: flag {int(flag.item())}"
            assert int(tflag.item()) == want, f"twin, {poison} M={M}: flag {int(tflag.item())}"
            if poison == "spike" and out_planes:   # the spike row itself is out of range; the others still hold their values
                ok = torch.tensor([i for i in range(M) if i != r][:64] + [M - 1])
                got_x = x[ok.to(dev)].cpu()
                check_ln(from_planes(ln[ok.to(dev)].cpu(), ACT), got_x, lw.cpu(), op["lb"].cpu(), 1e-6, "spike, other rows")


@pytest.mark.parametrize("construction", ["bias_spike", "eps0_nobias"])
@pytest.mark.parametrize("M", [193, "flip1"])
def test_phantom_rows_raise_nothing(dev, hip_lib, cu, profiler_ok, construction, M):
    """On a ragged M the flag depends on the rows below M only and equals the twin's.  The rows past M of the last tile are
    computed from zero A rows and a zero residual: x = bias * gamma there.  bias_spike: gamma = 1, bias B at column c,
    res = -B + noise there, ln_w[c] = 500: real rows hold about A.W^T, a phantom row's LayerNorm at c is about
    sqrt(383) * 500 * 8 = 78 000 > 65 520.  eps0_nobias: eps = 0 and a null bias: a phantom row is all zeros, its rstd inf."""
    M = geometry_flips(cu)[0] if M == "flip1" else M
    T, tiles, _, _, _, last_rows = rowln_grid(M, cu)
    assert last_rows < T, "the last tile must hold rows past M"
    c, B = 100, 16.0
    if construction == "bias_spike":
        op = operands(dev, M, 64, True, True, 0, seed=80)
        op["gamma"] = torch.ones(RN, device=dev)
        bias = torch.zeros(RN, device=dev)
        bias[c] = B
        op["bias"] = bias
        op["res"] = 0.5 * op["res"]
        op["res"][:, c] -= B
        op["lw"] = op["lw"].clone()
        op["lw"][c] = 500.0
        eps = 1e-6
    else:
        op = operands(dev, M, 64, False, True, 0, seed=81)
        eps = 0.0
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tflag = torch.zeros(1, dtype=torch.int32, device=dev)
    rc, x, ln = run_checked(lambda: rowln(hip_lib, op, M, False, True, eps, flag), T, True, False, profiler_ok,
                            f"phantom {construction}")
    assert rc == 0
    tx, tln = twin(hip_lib, op, M, False, True, eps, tflag)
    torch.cuda.synchronize()
    assert int(tflag.item()) == 0, f"twin raised {int(tflag.item())}"
    assert int(flag.item()) == int(tflag.item()), (f"{construction} M={M} (RlGeo<{T}>, last tile {last_rows} of {T} rows): "
                                                   f"flag {int(flag.item())} raised by rows past M; the twin raises nothing")
    assert torch.equal(tx[:M].view(torch.int32), x[:M].view(torch.int32))
    assert torch.equal(tln[:M].view(torch.int16), ln[:M].view(torch.int16))
    assert bool((x[M:] == X_SENT).all()) and bool((ln[M:] == PL_SENT).all())


# ---- 32-bit offsets ----------------------------------------------------------------------------------------------------------
def test_largest_m_at_k64(dev, hip_lib, cu, profiler_ok):
    """The largest M the launcher accepts at K = 64 (x, its LayerNorm and the phantom rows of the last tile just inside 32-bit
    byte offsets), x aliasing the residual as in the ViT: the last tile in full and rows in between against fp64."""
    M, K = MAX_M_K64, 64
    assert (M + 192) * RN * 4 < (1 << 32) - 512 <= (M + 193) * RN * 4
    geo = rowln_geo(M, cu)
    rows = check_rows_of(M, geo)
    op = operands(dev, M, K, True, True, 0, seed=90)
    rd = rows.to(dev)
    res_rows = op["res"][rd].cpu()
    a_dec = from_planes(op["ap"][rd].cpu(), ACT)
    x = torch.full((M + 2, RN), X_SENT, device=dev)
    x[:M] = op["res"]
    del op["res"]
    torch.cuda.empty_cache()
    ln = torch.full((M + 2, RN // 32, 2, 32), PL_SENT, dtype=torch.float16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    call = lambda: hip_lib.pope_linear_rowln_f32(_ptr(op["ap"]), _ptr(op["wp"]), M, K, _ptr(op["bias"]), _ptr(op["gamma"]),
                                                 _ptr(x), 0, _ptr(x), _ptr(op["lw"]), _ptr(op["lb"]), 1e-6, _ptr(ln), None,
                                                 _ptr(flag), _stream())
    rc = run_checked(call, geo, True, False, profiler_ok, f"M={M}")
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((x[M:] == X_SENT).all()) and bool((ln[M:] == PL_SENT).all()), "guard rows written"
    assert int(flag.item()) == 0
    got_x = x[rd].cpu()
    check_rows(got_x, fp64_residual(a_dec, op["w_dec"], op["bias"].cpu(), op["gamma"].cpu(), res_rows), X_ATOL, X_RTOL, "x")
    r = check_ln(from_planes(ln[rd].cpu(), ACT), got_x, op["lw"].cpu(), op["lb"].cpu(), 1e-6, f"M={M}")
    print(f"M={M} RlGeo<{geo}>: LayerNorm err / (2^-24 scale) = {r:.3f}")
