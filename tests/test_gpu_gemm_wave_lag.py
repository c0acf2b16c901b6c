"""GPU: the wave lag of the full-row-tile GEMM's K loop (gemm_rowln.hip, RL_LAG) at the smallest shapes where it can go wrong.

Waves 4 - 7 of the workgroup run the last RL_LAG column blocks of every K-step one K-step late, from W fragments they keep in
registers across the barrier, and flush them behind the tile-end barrier.  Per accumulator the order of the partial products
is unchanged, so every output must stay bit-identical to the kernels that have no lag (the 128 x 128 tile kernel / the
small-batch twin).  What can go wrong: a deferred fragment read after its LDS stage has been overwritten (shows as a
difference between two runs, or from the twin), a deferred block dropped or doubled at a tile seam or at the end of the
stream, a lag that does not restart with the tile, the residual prefetch (first K-step count with it: K = 192 on 192-row
tiles) landing in a different place.

Shapes, from the device's CU count `cu`:
  planes modes (BIAS, GELU; pope_linear_planes_f32 on the stream384 route): N = 1152, M = 192 * ceil(4 cu / 3) + 5 (one tile
    over the route's tile threshold, the last tile ragged), K = 64, 96, 128: 2, 3, 4 K-steps — both stage parities, and a
    deferred part as large as the immediate part at RL_LAG = 3.
  LayerNorm modes (pope_linear_rowln_f32): M = 192 (2 cu + 1) + 5 and M = 128 cu + 3, and — because the launcher chooses the
    geometry by rounds x rows, which on a 256-CU device gives the first of these to the 128-row tile and the second to the
    192-row tile — the first M >= each of them of the same raggedness that the launcher gives to the 192-row / 128-row
    geometry, so that both geometries see full rounds, a partial tail round, a ragged last tile and tile seams;
    K = 64, 96, 160, 192; with and without a residual table; planes and fp32 LayerNorm output.
Checks per case: fp64 parity with the bounds of test_gpu_gemm_routes.py / test_gpu_rowln.py (X_ATOL / X_RTOL 1e-5, PLANES_ATOL
2e-5, LN_C), bit identity with tile16 in pieces / with the twin (for a residual table: the twin over the table expanded row by
row), the two guard rows past M, range flag zero, two runs bit-equal; the kernel is asserted by name."""
import pytest
import torch

import test_gpu_gemm_routes as routes
import test_gpu_rowln as rl
from test_gpu_gemm_routes import cu, dev, profiler_ok  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_GELU = routes.EPI_BIAS, routes.EPI_GELU
N_PLANES = 1152
K_PLANES = [64, 96, 128]
K_LN = [64, 96, 160, 192]
RES_MOD = 197          # a table length that divides neither tile height


def _cdiv(a, b):
    return -(-a // b)


def planes_m(cu):
    return 192 * _cdiv(4 * cu, 3) + 5


def first_m_of_geometry(start, geo, cu):
    """The first M >= start with M = start (mod 384) that launch_rowln gives to the `geo`-row tile."""
    M = start
    while rl.rowln_geo(M, cu) != geo:
        M += 384
    return M


def ln_ms(cu):
    """(id, M, geometry the case is meant for or None = whatever the launcher picks)."""
    a, b = 192 * (2 * cu + 1) + 5, 128 * cu + 3
    return [("m_2rounds", a, None), ("m_1round", b, None), ("geo192", first_m_of_geometry(a, 192, cu), 192),
            ("geo128", first_m_of_geometry(b, 128, cu), 128)]


def test_shapes_sit_where_intended(cu):
    """Host only: the planes shape takes the stream384 route with a ragged last tile one tile over the threshold; the LayerNorm
    shapes give each geometry at least two tiles per workgroup somewhere, a partial tail round and a ragged last tile; the
    residual prefetch is off at K = 160 and on at K = 192 for the 192-row geometry (NPF = 5)."""
    M = planes_m(cu)
    for K in K_PLANES:
        assert routes.planes_route(M, N_PLANES, K, EPI_BIAS, True, cu) == "stream384"
        assert routes.planes_route(M - 2 * 192, N_PLANES, K, EPI_BIAS, True, cu) != "stream384"   # one spare tile, no more
    assert M % 192 == 5
    seen = set()
    for name, M, geo in ln_ms(cu):
        T, tiles, grid, full, tail, last_rows = rl.rowln_grid(M, cu)
        assert geo is None or T == geo, f"{name}: M={M} runs RlGeo<{T}>"
        assert last_rows < T, f"{name}: the last tile must be ragged"
        seen.add(T)
        if geo is not None:
            assert tiles > grid and tail > 0, f"{name}: M={M} needs a tile seam and a partial tail round"
        if name == "geo192":
            assert full >= 2, "two full rounds of 192-row tiles"
    assert seen == {128, 192}
    npf192 = _cdiv(192 * 12, 512)
    assert npf192 == 5 and not 160 // 32 > npf192 and 192 // 32 > npf192


# ---- planes modes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU], ids=["bias_epi", "gelu_epi"])
@pytest.mark.parametrize("K", K_PLANES)
def test_planes_stream_lag(dev, hip_lib, cu, profiler_ok, K, epi):
    M, N = planes_m(cu), N_PLANES
    assert routes.planes_route(M, N, K, epi, True, cu) == "stream384"
    ap, wp, w_dec, b = routes._operands(dev, M, N, K)
    bias = b.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    label = f"stream384 M={M} N={N} K={K} ({K // 32} K-steps) {'GELU' if epi else 'BIAS'}"
    out = routes._planes_call(hip_lib, ap, wp, bias, M, N, K, epi, True, dev, flag, routed=("stream384", profiler_ok, label))
    again = routes._planes_call(hip_lib, ap, wp, bias, M, N, K, epi, True, dev, flag)
    torch.cuda.synchronize()
    assert routes._guard_intact(out, M, True), f"{label}: rows M, M+1 written"
    assert int(flag.item()) == 0, f"{label}: range flag {int(flag.item())} on ordinary data"
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), f"{label}: two identical calls differ"
    rows = routes.check_rows_of(M, 192)
    want = routes.fp64_linear(routes.from_planes(ap[rows.to(dev)].cpu(), routes.ACT), w_dec, b, epi)
    routes.check_rows(routes.from_planes(out[rows.to(dev)].cpu(), routes.ACT), want, routes.PLANES_ATOL, 0.0, label)
    small = routes._in_pieces(hip_lib, ap, wp, bias, M, N, K, epi, dev, cu, profiler_ok)
    assert torch.equal(out[:M].view(torch.int16), small.view(torch.int16)), f"{label}: differs from tile16 in pieces"


# ---- LayerNorm modes ---------------------------------------------------------------------------------------------------------
_LN_OPERANDS = {}


def _ln_operands(dev, M, K):
    """Operands of one (M, K), shared by the four cases on it (one shape at a time); never modified."""
    if (M, K) not in _LN_OPERANDS:
        _LN_OPERANDS.clear()
        _LN_OPERANDS[(M, K)] = rl.operands(dev, M, K, True, True, 0, seed=7)
    return _LN_OPERANDS[(M, K)]


LN_IDS = [m[0] for m in ln_ms(256)]


@pytest.mark.parametrize("out_planes", [True, False], ids=["planes", "fp32"])
@pytest.mark.parametrize("table", [False, True], ids=["rows", "table"])
@pytest.mark.parametrize("K", K_LN)
@pytest.mark.parametrize("which", range(len(LN_IDS)), ids=LN_IDS)
def test_rowln_lag(dev, hip_lib, cu, profiler_ok, which, K, table, out_planes):
    name, M, geo = ln_ms(cu)[which]
    base = _ln_operands(dev, M, K)
    op = dict(base, res=base["res"][:RES_MOD].contiguous(), res_mod=RES_MOD) if table else base
    T, tiles, grid, _, tail, last_rows = rl.rowln_grid(M, cu)
    label = (f"{name}: M={M} K={K} ({K // 32} K-steps) RlGeo<{T}> {tiles} tiles on {grid} workgroups, tail {tail}, last tile "
             f"{last_rows} rows, {'table' if table else 'rows'}, {'planes' if out_planes else 'fp32'} out")
    # fp64 parity, guard rows, range flag, two runs bit-equal, the instantiation by name, and (rows) the twin
    x, ln = rl.check_case(hip_lib, op, M, False, out_planes, 1e-6, cu, profiler_ok, label)
    if table:   # the twin has no table: expand it row by row
        expanded = dict(op, res=op["res"][torch.arange(M, device=dev) % RES_MOD].contiguous(), res_mod=0)
        tflag = torch.zeros(1, dtype=torch.int32, device=dev)
        tx, tln = rl.twin(hip_lib, expanded, M, False, out_planes, 1e-6, tflag)
        torch.cuda.synchronize()
        assert torch.equal(tx[:M].view(torch.int32), x[:M].view(torch.int32)), f"{label}: x differs from the tile16 twin"
        assert torch.equal(tln[:M].view(torch.int16), ln[:M].view(torch.int16)), f"{label}: xn differs from layernorm_rowln_order"
        assert int(tflag.item()) == 0
