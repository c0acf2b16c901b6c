"""GPU: the LoFTR linear attention (csrc/loftr.hip, through pope_loftr_linear_attention_f32), one encoder layer around it
(LoFTREncoderLayer.update_) and the fine stage (csrc/fine.hip) against fp64 at their seams: source lengths around the reduction
chunk, query lengths around the rows of a message workgroup, both head widths, padding masks, four matches per workgroup of the
fine matching, two fine maps with nothing in common.

Cases, inputs, references and the comparison are tests/loftr_layer_checks.py (proven on the CPU by
test_loftr_layer_checks_cpu.py): per group, max |gpu - fp64| <= 4 max(e32, 2^-23 max |fp64|) with e32 the error of the same torch
restatement in fp32.  Output buffers of the attention entry carry a guard row that must stay bit-unchanged.  Measured ratios are
printed (-s) and recorded in profiles/loftr_layer_routes.md.  Not covered here: the graph path, lengths beyond a few chunks."""
import ctypes as C

import pytest
import torch

import loftr_layer_checks as lc
from pope_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def seams(hip_lib):
    c, r = C.c_int(0), C.c_int(0)
    hip_lib.pope_loftr_linear_attention_seams(C.byref(c), C.byref(r))
    return c.value, r.value


@pytest.fixture(scope="module")
def msd():
    from pope_amd import synth
    return synth.synthetic_matcher_state_dict(seed=0)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ok(status, what):
    """A launch that fails ends the session: nothing more is started on a device that may have faulted"""
    if status != 0:
        pytest.exit(f"{what}: status {status} ({_lib.lib().pope_error_string(status).decode()})", returncode=3)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _attention(lib, dev, q, kv, qm, km, planes=False, what="attention"):
    """-> (message [n, L, C] fp32 on the CPU, or the planes [n L, C / 32, 2, 32] f16; the range-flag word)"""
    n, L, Cd = q.shape
    S = kv.shape[1]
    nbytes = lib.pope_loftr_linear_attention_workspace_bytes(n, S, Cd, lc.NHEAD)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    qd, kvd = q.to(dev).contiguous(), kv.to(dev).contiguous()
    qmd, kmd = (None if m is None else m.to(dev).contiguous() for m in (qm, km))
    rows = n * L
    out = torch.full((rows + 1, Cd), lc.SENTINEL, dtype=torch.float32, device=dev)      # planes: the same bytes per row
    _ok(lib.pope_loftr_linear_attention_f32(_p(qd), _p(kvd), _p(qmd), _p(kmd), n, L, S, Cd, lc.NHEAD, None if planes else _p(out),
                                            _p(out) if planes else None, _p(ws), nbytes, _p(flag), _lib.stream_of(dev)), what)
    _sync(what)
    host = out.cpu()
    assert bool((host[rows:] == lc.SENTINEL).all()), f"{what}: the guard row was written"
    bits = int(flag.item())
    if planes:
        return host[:rows].view(torch.float16).view(rows, Cd // 32, 2, 32), bits
    return host[:rows].view(n, L, Cd), bits


@pytest.mark.parametrize("Cd", [256, 128])
def test_linear_attention_matches_fp64_at_the_seams(dev, hip_lib, seams, Cd):
    c, r = seams
    worst = (0.0, None)
    for case in (k for k in lc.attention_cases(c, r) if k["C"] == Cd):
        q, kv, qm, km = lc.attention_inputs(case, c)
        want64, want32 = lc.attention_ref(q, kv, qm, km), lc.attention_ref(q, kv, qm, km, torch.float32)
        got, bits = _attention(hip_lib, dev, q, kv, qm, km, what=case["id"])
        ratios = lc.head_ratios(got, want64, want32)
        worst = max(worst, (lc.report(case["id"], ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
        assert bits == 0
        if case["mask"] == "image":
            assert float(got[lc.MASKED_IMAGE].abs().max()) == 0.0            # a source without a valid row: the message is exactly 0
        if case["mask"] in ("qmask", "both"):
            assert float(got[qm == 0].abs().max()) == 0.0
    print(f"linear attention C={Cd}: worst ratio {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("Cd", [256, 128])
def test_linear_attention_bit_identities(dev, hip_lib, seams, Cd):
    """all-ones masks = no masks; planes = to_planes(fp32 rows); an image alone = inside its batch; two runs agree"""
    c, r = seams
    case = dict(id=f"attn-bits-C{Cd}", C=Cd, n=3, L=r + 1, S=2 * c + 1, mask="both", seed=77 + Cd)
    q, kv, qm, km = lc.attention_inputs(case, c)
    L, S = case["L"], case["S"]
    plain, _ = _attention(hip_lib, dev, q, kv, None, None)
    again, _ = _attention(hip_lib, dev, q, kv, None, None)
    assert torch.equal(plain, again)
    ones, _ = _attention(hip_lib, dev, q, kv, torch.ones(3, L), torch.ones(3, S))
    assert torch.equal(plain, ones)
    masked, _ = _attention(hip_lib, dev, q, kv, qm, km)
    assert torch.equal(masked, _attention(hip_lib, dev, q, kv, qm, km)[0])
    for b in range(3):
        alone, _ = _attention(hip_lib, dev, q[b:b + 1], kv[b:b + 1], None, None)
        assert torch.equal(alone[0], plain[b]), b
        alone, _ = _attention(hip_lib, dev, q[b:b + 1], kv[b:b + 1], qm[b:b + 1], km[b:b + 1])
        assert torch.equal(alone[0], masked[b]), b
    for rows, (a, m) in ((plain, (None, None)), (masked, (qm, km))):
        planes, bits = _attention(hip_lib, dev, q, kv, a, m, planes=True)
        assert bits == 0
        assert torch.equal(planes, _lib.to_planes(rows.reshape(3 * L, Cd), _lib.PLANES_ACT_SCALE))


def test_linear_attention_planes_raise_the_range_flag(dev, hip_lib, seams):
    c, r = seams
    case, q, kv = lc.flag_case(c, r)
    rows, bits = _attention(hip_lib, dev, q, kv, None, None)
    assert bits == 0 and float(rows.abs().max()) > lc.PLANES_LIMIT           # fp32 rows: no range contract
    ratios = lc.head_ratios(rows, lc.attention_ref(q, kv), lc.attention_ref(q, kv, dtype=torch.float32))
    lc.report(case["id"], ratios)
    assert max(ratios) <= 1.0, ratios
    _, bits = _attention(hip_lib, dev, q, kv, None, None, planes=True)
    assert bits != 0


def test_linear_attention_refusals(hip_lib):
    """return codes only: every refused call returns on the host, before any HIP call"""
    lc.assert_attention_refusals(hip_lib)


# ---- the encoder layer --------------------------------------------------------------------------------------------------------
def _layer_module(dev, msd, case):
    from pope_amd.loftr import LoFTREncoderLayer
    m = LoFTREncoderLayer(case["C"], lc.NHEAD).eval()
    m.load_state_dict(lc.layer_state(msd, case["prefix"]), strict=True)
    return m.to(dev)


@pytest.mark.parametrize("precision", lc.LAYER_PRECISIONS)
def test_encoder_layer_matches_fp64(dev, hip_lib, seams, msd, precision):
    c, r = seams
    worst = (0.0, None)
    modules = {}
    for case in (k for k in lc.layer_cases(c, r) if k["precision"] == precision):
        x, source, xm, sm = lc.layer_inputs(case)
        want64, want32 = lc.layer_ref(msd, case, x, source, xm, sm), lc.layer_ref(msd, case, x, source, xm, sm, torch.float32)
        m = modules.setdefault(case["prefix"], _layer_module(dev, msd, case))
        xd = x.to(dev).contiguous()
        sd_ = xd if case["kind"] == "self" else source.to(dev).contiguous()
        nbytes = hip_lib.pope_loftr_layer_workspace_bytes(case["n"], case["L"], case["S"], case["C"], lc.NHEAD)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        try:
            flag = m.update_(xd, sd_, ws, precision, None if xm is None else xm.to(dev), None if sm is None else sm.to(dev))
        except _lib.PopeHipError as e:
            pytest.exit(f"{case['id']}: {e}", returncode=3)
        _sync(case["id"])
        assert int(flag.item()) == 0
        ratio = lc.group_ratio(xd.cpu(), want64, want32)
        worst = max(worst, (lc.report(case["id"], [ratio]), case["id"]))
        assert ratio <= 1.0, (case["id"], ratio)
    print(f"encoder layer {precision}: worst ratio {worst[0]:.3f} at {worst[1]}")


# ---- the fine stage -----------------------------------------------------------------------------------------------------------
def _fine_match(lib, dev, case, x):
    w0, w1, mk, b_ids, scale1 = x
    M = w0.shape[0]
    w0d, w1d, mkd = w0.to(dev).contiguous(), w1.to(dev).contiguous(), mk.to(dev).contiguous()
    expec = torch.full((M + 1, 3), lc.SENTINEL, dtype=torch.float32, device=dev)
    mk1f = torch.full((M + 1, 2), lc.SENTINEL, dtype=torch.float32, device=dev)
    s1 = bd = None                                                           # plain: no scale1, no b_ids
    if case["entry"] == "scaled":
        s1, bd = scale1.to(dev).contiguous(), b_ids.to(dev).contiguous()
    _ok(lib.pope_fine_match_f32(_p(w0d), _p(w1d), M, case["W"], case["C"], _p(mkd), lc.SCALE_PX, _p(s1), _p(bd), _p(expec), _p(mk1f),
                                _lib.stream_of(dev)), case["id"])
    _sync(case["id"])
    out = torch.cat([expec.cpu(), mk1f.cpu()], 1)
    assert bool((out[M:] == lc.SENTINEL).all()), f"{case['id']}: the guard row was written"
    return out[:M]


@pytest.mark.parametrize("entry", lc.FINE_ENTRIES)
def test_fine_match_matches_fp64(dev, hip_lib, entry):
    worst = (0.0, None)
    for case in (k for k in lc.fine_match_cases() if k["entry"] == entry):
        xs = [lc.fine_match_inputs(case, M) for M in lc.FINE_M]
        want64 = torch.cat([lc.fine_match_ref(*x) for x in xs])
        want32 = torch.cat([lc.fine_match_ref(*x, dtype=torch.float32) for x in xs])
        got = torch.cat([_fine_match(hip_lib, dev, case, x) for x in xs])
        ratios = lc.fine_match_ratios(case, got, want64, want32)
        worst = max(worst, (lc.report(case["id"], ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
        if case["kind"] == "saturated":
            assert bool(torch.isfinite(got[:, 2]).all()) and float(got[:, 2].min()) >= lc.SPREAD_CLAMP
    print(f"fine match {entry}: worst ratio {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("precision", lc.LAYER_PRECISIONS)
def test_fine_preprocess_matches_fp64(dev, hip_lib, msd, precision):
    from pope_amd.loftr import FinePreprocess
    from pope_amd.matcher import default_cfg
    fp = FinePreprocess(default_cfg).eval()
    fp.load_state_dict({k[len("fine_preprocess."):]: v for k, v in msd.items() if k.startswith("fine_preprocess.")}, strict=True)
    fp = fp.to(dev)
    assert fp.W == lc.PRE_W and fp._weights(precision) is not None
    worst = (0.0, None)
    for case in (k for k in lc.fine_pre_cases() if k["precision"] == precision):
        f0, f1, c0, c1, b, i, j = lc.fine_pre_inputs(case)
        want64, want32 = lc.fine_pre_ref(msd, f0, f1, c0, c1, b, i, j), lc.fine_pre_ref(msd, f0, f1, c0, c1, b, i, j, torch.float32)
        if case["layout"] == "nchw":
            f0d, f1d = f0.to(dev), f1.to(dev)
        else:   # what the HIP backbone hands over: the interior of a bordered NHWC buffer, permuted
            def bordered(f):
                n, ch, h, w = f.shape
                buf = torch.full((n, h + 2, w + 2, ch), lc.SENTINEL, dtype=torch.float32, device=dev)
                buf[:, 1:-1, 1:-1, :] = f.permute(0, 2, 3, 1).to(dev)
                return buf[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)
            f0d, f1d = bordered(f0), bordered(f1)
        data = {"hw0_f": tuple(f0.shape[2:]), "hw0_c": lc.PRE_GRID0, "hw1_c": lc.PRE_GRID1, "b_ids": b.to(dev), "i_ids": i.to(dev),
                "j_ids": j.to(dev)}
        try:
            (g0, g1), flag = fp._run(f0d, f1d, c0.to(dev).contiguous(), c1.to(dev).contiguous(), data, lc.PRE_STRIDE, precision)
        except _lib.PopeHipError as e:
            pytest.exit(f"{case['id']}: {e}", returncode=3)
        _sync(case["id"])
        assert int(flag.item()) == 0
        ratios = [lc.group_ratio(g0.cpu().contiguous(), want64[0], want32[0]), lc.group_ratio(g1.cpu().contiguous(), want64[1], want32[1])]
        worst = max(worst, (lc.report(case["id"], ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
    print(f"fine preprocess {precision}: worst ratio {worst[0]:.3f} at {worst[1]}")
