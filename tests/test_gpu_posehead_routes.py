"""GPU: the transformer kernels of the pose heads (csrc/mocope.hip, csrc/pose_regressor.hip, csrc/posereg_tile.h) against fp64 at
their group seams, tile tails and route switches, through the op-level entries pope_mocope_*_f32 and
pope_pose_regressor_{layer,stream_linear,tail}_f32.

Cases, inputs, references and the comparison are tests/posehead_checks.py (proven on the CPU by test_posehead_checks_cpu.py):
the error against the fp64 torch reference is at most MARGIN = 4 times the error of the same torch op in fp32 on the CPU (2 ulp of
the rounded fp64 result for the Linears with K <= 4).  Every output buffer carries a guard row behind it that must stay
bit-unchanged.  Measured ratios are printed (-s) and recorded in profiles/posehead_routes.md."""
import ctypes as C

import pytest
import torch

import posehead_checks as pc
from pope_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _p(t, offset=0):
    return C.c_void_p(t.data_ptr() + 4 * offset) if t is not None else None


def _guarded(rows, cols, dev, fill=None):
    """[rows + 1, cols] on the device: `fill` (or the sentinel) in the first rows, the sentinel in the guard row"""
    buf = torch.full((rows + 1, cols), pc.SENTINEL, dtype=torch.float32, device=dev)
    if fill is not None:
        buf[:rows] = fill.to(dev)
    return buf


def _ok(status, what):
    """A launch that fails ends the session: nothing more is started on a device that may have faulted"""
    if status != 0:
        pytest.exit(f"{what}: status {status} ({_lib.lib().pope_error_string(status).decode()})", returncode=3)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _take(buf, rows, what):
    _sync(what)
    out = buf.cpu()
    assert bool((out[rows:] == pc.SENTINEL).all()), f"{what}: the guard row was written"
    return out[:rows]


def _verdict(tag, got, want64, want32):
    err, bound = pc.measure(got, want64, want32)
    own = None if want32 is None else 1.0 / pc.MARGIN
    pc.report(tag, err, bound, own)
    assert err <= bound, (tag, err, bound)


# ---- Linears ------------------------------------------------------------------------------------------------------------------
def _run_mocope_linear(lib, dev, c, x):
    A, W, b = (x[k].to(dev) for k in ("A", "W", "bias"))
    Y = _guarded(c["R"], c["N"], dev)
    _ok(lib.pope_mocope_linear_f32(_p(A), _p(W), _p(b), _p(Y), c["R"], c["K"], c["N"], c["act"], _lib.stream_of(dev)), c["id"])
    return _take(Y, c["R"], c["id"])


@pytest.mark.parametrize("c", pc.LINEAR_CASES, ids=lambda c: c["id"])
def test_mocope_linear(dev, hip_lib, c):
    x, ref = pc.linear_case(c)
    _verdict(c["id"], _run_mocope_linear(hip_lib, dev, c, x), ref["want64"], ref["want32"])


def test_mocope_linear_second_launch(dev, hip_lib):
    """More than MAX_GRID_Y row chunks: the second launch serves rows 524 280 .."""
    c = pc.SEAM_CASE
    x, ref = pc.linear_case(c)
    got = _run_mocope_linear(hip_lib, dev, c, x)
    rows = list(pc.SEAM_ROWS) + [c["R"] - 3, c["R"] - 2, c["R"] - 1]
    _verdict(c["id"] + " seam rows", got[rows], ref["want64"][rows], None)
    _verdict(c["id"], got, ref["want64"], ref["want32"])


def _run_stream(lib, dev, c, x, offset=None):
    offset = c["offset"] if offset is None else offset
    R, K, N = c["R"], c["K"], c["N"]
    flat = torch.zeros(R * K + 4, dtype=torch.float32, device=dev)
    flat[offset:offset + R * K] = x["A"].to(dev).flatten()
    assert flat.data_ptr() % 16 == 0
    W, b = x["W"].to(dev), x["bias"].to(dev)
    Y = _guarded(R, N, dev)
    _ok(lib.pope_pose_regressor_stream_linear_f32(_p(flat, offset), _p(W), _p(b), _p(Y), R, K, N, _lib.stream_of(dev)), c["id"])
    return _take(Y, R, c["id"])


@pytest.mark.parametrize("c", pc.STREAM_CASES, ids=lambda c: c["id"])
def test_stream_linear(dev, hip_lib, c):
    x, ref = pc.linear_case(c)
    _verdict(f"{c['id']} V{pc.stream_route(c)[0]}", _run_stream(hip_lib, dev, c, x), ref["want64"], ref["want32"])


def test_stream_linear_routes_agree(dev, hip_lib):
    """One (K, N) both routes serve, one input: 16-byte loads against single floats, each within the bound of the reference and
    of each other"""
    c = next(k for k in pc.STREAM_CASES if (k["R"], k["K"], k["N"]) == pc.STREAM_TWIN and not k["offset"])
    x, ref = pc.linear_case(c)
    vec, scalar = _run_stream(hip_lib, dev, c, x, offset=0), _run_stream(hip_lib, dev, c, x, offset=1)
    bound = pc.MARGIN * pc.max_err(ref["want32"], ref["want64"])
    between = float((vec.double() - scalar.double()).abs().max())
    pc.report("stream twin, route against route", between, bound)
    assert between <= bound
    for name, got in (("vector", vec), ("scalar", scalar)):
        _verdict(f"stream twin {name}", got, ref["want64"], ref["want32"])


# ---- attention ----------------------------------------------------------------------------------------------------------------
def _run_attention(lib, dev, c, x, rows=None):
    """rows: a slice of whole groups to run alone (same buffers, offset pointers)"""
    bufs, views = pc.attention_buffers(c, x)
    r0, r1 = (0, c["R"]) if rows is None else rows
    on = [b[r0:r1].contiguous().to(dev) for b in bufs]
    R = r1 - r0
    O = _guarded(R, c["d"], dev)
    args = []
    for i, off, ld in views:
        args += [_p(on[i], off), ld]
    _ok(lib.pope_mocope_attention_f32(*args, _p(O), R, c["S"], c["G"], c["d"], _lib.stream_of(dev)), c["id"])
    return _take(O, R, c["id"])


@pytest.mark.parametrize("c", pc.ATTENTION_CASES, ids=lambda c: c["id"])
def test_mocope_attention(dev, hip_lib, c):
    x, ref = pc.attention_case(c)
    got = _run_attention(hip_lib, dev, c, x)
    _verdict(c["id"], got, ref["want64"], ref["want32"])
    if c["q"] == 2:      # a group's rows do not depend on the other groups of the call
        half = c["R"] // 2
        for r0 in (0, half):
            assert torch.equal(_run_attention(hip_lib, dev, c, x, rows=(r0, r0 + half)), got[r0:r0 + half]), (c["id"], r0)


# ---- add_ln, ffn76 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.ADD_LN_CASES, ids=lambda c: c["id"])
def test_mocope_add_ln(dev, hip_lib, c):
    x, ref = pc.add_ln_case(c)
    X = _guarded(c["R"], c["d"], dev, x["X"])
    on = {k: x[k].to(dev) for k in ("Y", "w1", "b1", "w2", "b2")}
    w2, b2 = (_p(on["w2"]), _p(on["b2"])) if c["closing"] else (None, None)
    _ok(hip_lib.pope_mocope_add_ln_f32(_p(X), _p(on["Y"]), _p(on["w1"]), _p(on["b1"]), w2, b2, c["R"], c["d"], _lib.stream_of(dev)), c["id"])
    _verdict(c["id"], _take(X, c["R"], c["id"]), ref["want64"], ref["want32"])


@pytest.mark.parametrize("c", pc.FFN76_CASES, ids=lambda c: c["id"])
def test_mocope_ffn76(dev, hip_lib, c):
    x, ref = pc.ffn76_case(c)
    R = c["R"]
    spare = -(-R // 32) * 32 - R + 1            # the rest of the last tile and one row more: live values the launch must not touch
    after = torch.randn(spare, pc.D76, generator=torch.Generator().manual_seed(R))
    X = torch.cat([x["X"], after]).to(dev)
    on = {k: x[k].to(dev) for k in ("l1w", "l1b", "l2w", "l2b", "nw", "nb", "fw", "fb")}
    fw, fb = (_p(on["fw"]), _p(on["fb"])) if c["closing"] else (None, None)
    _ok(hip_lib.pope_mocope_ffn76_f32(_p(X), *(_p(on[k]) for k in ("l1w", "l1b", "l2w", "l2b", "nw", "nb")), fw, fb, R, _lib.stream_of(dev)),
               c["id"])
    _sync(c["id"])
    out = X.cpu()
    assert torch.equal(out[R:], after), f"{c['id']}: rows at or beyond R were written"
    _verdict(c["id"], out[:R], ref["want64"], ref["want32"])


# ---- encoder layer ------------------------------------------------------------------------------------------------------------
def _run_layer(lib, dev, c, x, pairs=None):
    """pairs: a slice of whole groups to run alone"""
    b0, b1 = (0, c["B"]) if pairs is None else pairs
    B, S = b1 - b0, c["S"]
    on = [x["sd"][k].to(dev) for k in pc.LAYER_KEYS]
    w = _lib.PoseRegressorLayer(*(t.data_ptr() for t in on))
    X = _guarded(B * S, pc.D76, dev, x["X"][b0:b1].reshape(B * S, pc.D76))
    _ok(lib.pope_pose_regressor_layer_f32(C.byref(w), _p(X), B, S, c["G"], _lib.stream_of(dev)), c["id"])
    return _take(X, B * S, c["id"]).view(B, S, pc.D76)


@pytest.mark.parametrize("c", pc.LAYER_CASES, ids=lambda c: c["id"])
def test_posereg_layer(dev, hip_lib, c):
    x, ref = pc.layer_case(c)
    got = _run_layer(hip_lib, dev, c, x)
    RB, T, live, tiles, last = pc.layer_route(c)
    _verdict(f"{c['id']} <{RB}> T{T} live {live} tiles {tiles} last {last}", got, ref["want64"], ref["want32"])
    if c["B"] == 2 * c["G"]:      # two groups: each bit-equal to its run alone
        for b0 in (0, c["G"]):
            assert torch.equal(_run_layer(hip_lib, dev, c, x, pairs=(b0, b0 + c["G"])), got[b0:b0 + c["G"]]), (c["id"], b0)


# ---- tail ---------------------------------------------------------------------------------------------------------------------
def _run_tail(lib, dev, c, x):
    on = {k: v.to(dev) for k, v in x.items()}
    w = _lib.PoseRegressorWeights()
    w.num_sample, w.mode = c["S"], pc.MODES[c["mode"]][0]
    for i in range(5):
        w.mlp_w[2 + i], w.mlp_b[2 + i] = on[f"w{i}"].data_ptr(), on[f"b{i}"].data_ptr()
    w.trans_w, w.trans_b, w.rot_w, w.rot_b = (on[k].data_ptr() for k in ("trans_w", "trans_b", "rot_w", "rot_b"))
    status = torch.tensor(c["status"], dtype=torch.int32, device=dev)
    t, r = _guarded(pc.TAIL_B, 3, dev), _guarded(pc.TAIL_B, 9, dev)
    _ok(lib.pope_pose_regressor_tail_f32(C.byref(w), _p(on["Y2"]), _p(status), pc.TAIL_B, _p(t), _p(r), _lib.stream_of(dev)), c["id"])
    return _take(t, pc.TAIL_B, c["id"]), _take(r, pc.TAIL_B, c["id"])


@pytest.mark.parametrize("c", pc.TAIL_CASES, ids=lambda c: c["id"])
def test_posereg_tail(dev, hip_lib, c):
    x, ref = pc.tail_case(c)
    t, r = _run_tail(hip_lib, dev, c, x)
    _verdict(c["id"] + " trans", t, ref["t64"], ref["t32"])
    _verdict(c["id"] + " rot", r, ref["r64"], ref["r32"])


def test_posereg_tail_refused_pair(dev, hip_lib):
    c = pc.TAIL_STATUS_CASE
    x, ref = pc.tail_case(c)
    t, r = _run_tail(hip_lib, dev, c, x)
    t_all, r_all = _run_tail(hip_lib, dev, dict(c, status=(0, 0, 0)), x)
    assert float(t[1].abs().max()) == 0 and float(r[1].abs().max()) == 0
    keep = [0, 2]
    assert torch.equal(t[keep], t_all[keep]) and torch.equal(r[keep], r_all[keep])
    _verdict(c["id"] + " trans", t[keep], ref["t64"][keep], ref["t32"][keep])
    _verdict(c["id"] + " rot", r[keep], ref["r64"][keep], ref["r32"][keep])


# ---- the whole nn.Transformer under groupings the callers never use -----------------------------------------------------------
@pytest.fixture(scope="module")
def fusion(dev):
    from pope_amd import convnextv2, synth
    from pope_amd.mocope import MoCoPE
    sd = synth.mocope_state_dict(pc.XFMR_S, "6d")
    model = MoCoPE(pc.XFMR_S, "6d", backbone=convnextv2.ConvNeXtV2(**synth.MOCOPE_TRUNK))
    model.load_state_dict(sd, strict=True)
    refs = {}
    for prefix, d in (("transformer_mkpts", 76), ("mkpts_as_q", 512), ("cnn_as_q", 512)):
        refs[prefix] = tuple(pc.load_transformer(sd, prefix, d, dt) for dt in (torch.float64, torch.float32))
    return model.to(dev), refs


def _taps(model, dev, B, G, pairs=None):
    from pope_amd import synth
    from pope_amd.mocope import _run
    b0, b1 = (0, B) if pairs is None else pairs
    d0, d1 = (t[b0:b1].contiguous().to(dev) for t in synth.pose_regressor_case(pc.XFMR_S, B))
    g = torch.Generator().manual_seed(12000 + B)
    f0, f1 = (torch.randn(B, 1000, generator=g)[b0:b1].contiguous().to(dev) for _ in range(2))
    stages = ("embedding", "memory", "transformer_mkpts", "x_mkpts", "x_img", "qmkpts", "qimg")
    out = {s: _run(model, s, b1 - b0, G, f0, f1, dense=(d0, d1))["x"] for s in stages}
    _sync(f"taps B{B} G{G}")
    return {s: t.cpu() for s, t in out.items()}


@pytest.mark.parametrize("B,G", pc.XFMR_BG)
def test_transformers_under_foreign_grouping(dev, fusion, B, G):
    model, refs = fusion
    got = _taps(model, dev, B, G)
    bounds = {}
    for tap, (prefix, d, feeds, what) in pc.XFMR_TAPS.items():
        t64, t32 = refs[prefix]
        src, tgt = (got[f] for f in feeds)        # the GPU's own preceding taps: only the transformer is under test
        want64 = pc.run_grouped(t64, src.double(), tgt.double(), G)[what]
        want32 = pc.run_grouped(t32, src, tgt, G)[what]
        _verdict(f"xfmr B{B} G{G} {tap}", got[tap], want64, want32)
        bounds[tap] = pc.MARGIN * pc.max_err(want32, want64)
    if (B, G) != (6, 3):
        return
    whole = _taps(model, dev, 6, 6)              # the callers' grouping: a different function of the same input
    for tap in pc.XFMR_TAPS:
        assert float((whole[tap] - got[tap]).abs().max()) >= pc.PLANT * bounds[tap], tap
    for b0 in (0, 3):                            # a group's rows do not depend on the other group of the call
        alone = _taps(model, dev, 6, 3, pairs=(b0, b0 + 3))
        for tap in ("embedding",) + tuple(pc.XFMR_TAPS):
            assert torch.equal(alone[tap], got[tap][b0:b0 + 3]), (tap, b0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_argument_refusals(hip_lib):
    for what, status in pc.argument_refusals(hip_lib):
        assert status == -1, what
