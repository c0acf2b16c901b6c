"""CPU: the checker of test_gpu_posehead_routes.py (tests/posehead_checks.py) proven on its own data — the case lists hold every
seam value, the inputs discriminate (softmax spread, sign balance, plants that move the fp64 result by >= 100 bounds), a torch
fp32 restatement of every op passes and every planted fault fails."""
import pytest
import torch

import posehead_checks as pc


def _passes(got, want64, want32=None):
    err, bound = pc.measure(got, want64, want32)
    return err <= bound


def _stale_last_row(t):
    t = t.clone()
    t[-1] = pc.SENTINEL
    return t


def _stale_last_col(t):
    t = t.clone()
    t[..., -1] = pc.SENTINEL
    return t


# ---- case lists -------------------------------------------------------------------------------------------------------------
def test_case_lists_hold_every_seam_value():
    lin = pc.LINEAR_CASES
    assert 20 <= len(lin) <= 28 and len({c["id"] for c in lin}) == len(lin)
    assert {c["N"] for c in lin} == set(pc.LINEAR_N) and {c["R"] for c in lin} == set(pc.LINEAR_R)
    assert {c["K"] for c in lin} == set(pc.LINEAR_K) and {c["act"] for c in lin} == {0, 1}
    for N in (1023, 1025, 1027):
        assert any(c["N"] == N and c["R"] == 9 for c in lin), N
    assert {-(-(K // 4) // 64) for K in pc.LINEAR_K} == {1, 2, 8} and 64 in {K // 4 for K in pc.LINEAR_K} and 65 in {K // 4 for K in pc.LINEAR_K}
    s = pc.SEAM_CASE
    assert (s["R"], s["K"], s["N"]) == (8 * 65535 + 3, 4, 2) and pc.SEAM_ROWS == (524279, 524280, 524281, 524282)
    assert -(-s["R"] // pc.NB) == pc.MAX_GRID_Y + 1          # one row chunk in the second launch

    att = pc.ATTENTION_CASES
    assert {c["d"] for c in att} == {76, 512} and {c["G"] for c in att} == {2, 3, 5, 31, 32, 33, 63, 64}
    assert {c["S"] for c in att} == {1, 3} and {c["layout"] for c in att} == {"self", "cross"}
    for d in (76, 512):
        for layout in pc.ATT_LAYOUTS:
            mine = [c for c in att if c["d"] == d and c["layout"] == layout]
            assert {(c["G"], c["q"]) for c in mine} == {(G, q) for G in pc.ATT_G for q in (1, 2, 3) if q == 1 or G < 63}
            assert any(c["R"] % 4 for c in mine) and any(c["R"] == 3 for c in mine)
    assert all(c["R"] == c["q"] * c["G"] * c["S"] for c in att)

    assert {(c["d"], c["R"], c["closing"]) for c in pc.ADD_LN_CASES} == {(d, R, cl) for d in (76, 512) for R in (1, 3, 4, 5, 130)
                                                                          for cl in (False, True)}
    assert {(c["R"], c["closing"]) for c in pc.FFN76_CASES} == {(R, cl) for R in (1, 31, 32, 33, 65) for cl in (False, True)}

    assert [(c["G"], c["B"], c["S"]) for c in pc.LAYER_CASES] == list(pc.LAYER_GBS) and len(pc.LAYER_GBS) == 11
    routes = {(c["G"], c["B"], c["S"]): pc.layer_route(c) for c in pc.LAYER_CASES}
    assert [routes[k][2] for k in ((3, 6, 7), (5, 10, 7), (7, 7, 5))] == [30, 30, 28]          # live rows of 32
    assert routes[(3, 6, 7)][1:] == (10, 30, 2, 4) and routes[(5, 10, 7)][1:] == (6, 30, 3, 2)   # NU = 14: partial last tiles
    assert routes[(32, 64, 2)][:2] == (1, 1) and routes[(16, 32, 3)][:2] == (1, 2)
    assert routes[(33, 33, 2)][0] == routes[(64, 64, 3)][0] == routes[(33, 66, 1)][0] == 2 and routes[(31, 31, 2)][0] == 1
    assert routes[(33, 66, 1)][3] == 2                                                          # two groups on the <2> instantiation

    st = pc.STREAM_CASES
    assert 28 <= len(st) <= 36 and len({c["id"] for c in st}) == len(st)
    assert {c["R"] for c in st} == set(pc.STREAM_B) and {c["N"] for c in st} == set(pc.STREAM_N) and {c["K"] for c in st} == set(pc.STREAM_K)
    for V in (1, 4):
        rems = {pc.stream_route(c)[2] for c in st if pc.stream_route(c)[0] == V}
        assert rems >= set(range(1, 8)), (V, rems)                        # every remainder instantiation of both routes
        assert any(pc.stream_route(c)[1] and pc.stream_route(c)[2] for c in st if pc.stream_route(c)[0] == V)
    assert {c["R"] for c in st if pc.stream_route(c)[1] == 0} >= set(range(1, 8))
    off = [c for c in st if c["offset"]]
    assert len(off) == 1 and off[0]["K"] == 256 and pc.stream_route(off[0])[0] == 1
    assert any((c["R"], c["K"], c["N"]) == pc.STREAM_TWIN and pc.stream_route(c)[0] == 4 for c in st)
    assert (off[0]["R"], off[0]["K"], off[0]["N"]) == pc.STREAM_TWIN

    assert {c["S"] for c in pc.TAIL_CASES} == {1, 63, 64, 65, 512}
    assert {c["mode"] for c in pc.TAIL_CASES if c["S"] == 64} == {"matrix", "quat", "6d"}
    assert pc.TAIL_STATUS_CASE["status"][1] != 0 and pc.TAIL_STATUS_CASE["status"][0] == pc.TAIL_STATUS_CASE["status"][2] == 0
    assert pc.XFMR_BG == ((6, 3), (6, 1), (64, 32)) and set(pc.XFMR_TAPS) == {"memory", "transformer_mkpts", "qmkpts", "qimg"}


# ---- Linears ------------------------------------------------------------------------------------------------------------------
def _check_signs(pres, family):
    """>= 25 % of each sign per case with enough pre-activations, and over the family"""
    for cid, pre in pres:
        if pre.numel() >= pc.SIGN_MIN_COUNT:
            neg, pos = pc.sign_shares(pre)
            assert neg >= pc.SIGN_SHARE and pos >= pc.SIGN_SHARE, (cid, neg, pos)
    neg, pos = pc.sign_shares(torch.cat([p.flatten() for _, p in pres]))
    assert neg >= pc.SIGN_SHARE and pos >= pc.SIGN_SHARE, (family, neg, pos)


@pytest.mark.parametrize("family", ["mocope_linear", "stream_linear"])
def test_linear_checker(family):
    cases = pc.LINEAR_CASES if family == "mocope_linear" else pc.STREAM_CASES
    pres = []
    for c in cases:
        x, ref = pc.linear_case(c)
        pres.append((c["id"], ref["pre"]))
        good = pc.linear_restated(c, x)
        err, bound = pc.measure(good, ref["want64"], ref["want32"])
        pc.report(c["id"], err, bound)
        assert err <= bound, (c["id"], err, bound)
        assert (ref["want32"] is None) == (c["K"] <= 4)
        if c["N"] > 1:
            assert not _passes(_stale_last_col(good), ref["want64"], ref["want32"]), c["id"]
        if c["R"] > 1:
            assert not _passes(_stale_last_row(good), ref["want64"], ref["want32"]), c["id"]
        if c["act"] != pc.ACT_NONE and ref["pre"].numel() >= pc.SIGN_MIN_COUNT:
            plain = pc.linear_restated(dict(c, act=pc.ACT_NONE), x)                 # ReLU / LeakyReLU omitted
            assert not _passes(plain, ref["want64"], ref["want32"]), c["id"]
    _check_signs([(cid, p) for (cid, p), c in zip(pres, cases) if c["act"] != pc.ACT_NONE], family)


def test_linear_seam_checker():
    c = pc.SEAM_CASE
    x, ref = pc.linear_case(c)
    good = pc.linear_restated(c, x)
    err, bound = pc.measure(good, ref["want64"], ref["want32"])
    pc.report(c["id"], err, bound)
    assert err <= bound
    neg, pos = pc.sign_shares(ref["pre"])
    assert neg >= pc.SIGN_SHARE and pos >= pc.SIGN_SHARE
    # the second launch based at row 0: rows SEAM_ROW .. are computed from A's first rows (and the true rows stay unwritten)
    bad = good.clone()
    n = c["R"] - pc.SEAM_ROW
    bad[pc.SEAM_ROW:] = pc.linear_restated(dict(c, R=n), dict(x, A=x["A"][:n]))
    assert not _passes(bad, ref["want64"], ref["want32"])
    rows = list(pc.SEAM_ROWS) + [c["R"] - 3, c["R"] - 2, c["R"] - 1]
    assert not _passes(bad[rows], ref["want64"][rows]) and _passes(good[rows], ref["want64"][rows])
    assert not _passes(_stale_last_row(good), ref["want64"], ref["want32"])


def test_stream_twin_routes_share_one_reference():
    a = next(c for c in pc.STREAM_CASES if (c["R"], c["K"], c["N"]) == pc.STREAM_TWIN and not c["offset"])
    b = next(c for c in pc.STREAM_CASES if c["offset"])
    # the GPU test feeds case a's input to both routes; the twin's own case has its own seed
    assert pc.stream_route(a)[0] == 4 and pc.stream_route(b)[0] == 1 and a["id"] != b["id"]


# ---- attention ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", pc.ATT_D)
def test_attention_checker(d):
    for c in (c for c in pc.ATTENTION_CASES if c["d"] == d and c["layout"] == "self"):
        x, ref = pc.attention_case(c)
        peak = ref["weights"].amax(-1)
        assert float(peak.min()) >= pc.SPREAD[0] and float(peak.max()) <= pc.SPREAD[1], (c["id"], float(peak.min()), float(peak.max()))
        want64, want32 = ref["want64"], ref["want32"]
        for plant in ("drop64", "swap64"):
            assert pc.moved(want64, ref[plant], want32) >= pc.PLANT, (c["id"], plant)
        err, bound = pc.measure(want32, want64, want32)
        assert err <= bound and bound > 0
        S, G = c["S"], c["G"]
        for kw in (dict(drop_last=True), dict(swap=True)):
            assert not _passes(pc.attention_ref(x["q"], x["k"], x["v"], S, G, **kw)[0], want64, want32), (c["id"], kw)
        assert not _passes(_stale_last_col(want32), want64, want32) and not _passes(_stale_last_row(want32), want64, want32)
        # the two layouts carry the same operands
        for layout in pc.ATT_LAYOUTS:
            bufs, views = pc.attention_buffers(dict(c, layout=layout), x)
            for name, (i, off, ld) in zip("qkv", views):
                assert bufs[i].shape[1] == ld and torch.equal(bufs[i][:, off:off + d], x[name])


# ---- add_ln, ffn76 --------------------------------------------------------------------------------------------------------------
def test_add_ln_checker():
    for c in pc.ADD_LN_CASES:
        x, ref = pc.add_ln_case(c)
        assert float((x["w1"] - 1).abs().max()) > 0.1 and float(x["b1"].abs().max()) > 0.1
        assert _passes(ref["want32"], ref["want64"], ref["want32"])
        other = pc.add_ln_ref(x, not c["closing"])              # closing norm omitted / applied unasked
        assert not _passes(other, ref["want64"], ref["want32"]), c["id"]
        assert not _passes(_stale_last_row(ref["want32"]), ref["want64"], ref["want32"])
        assert not _passes(_stale_last_col(ref["want32"]), ref["want64"], ref["want32"])


def test_ffn76_checker():
    pres = []
    for c in pc.FFN76_CASES:
        x, ref = pc.ffn76_case(c)
        pres.append((c["id"], ref["pre"]))
        assert _passes(ref["want32"], ref["want64"], ref["want32"])
        assert not _passes(pc.ffn76_ref(x, not c["closing"])[0], ref["want64"], ref["want32"]), c["id"]
        assert not _passes(pc.ffn76_ref(x, c["closing"], relu=False)[0], ref["want64"], ref["want32"]), c["id"]
        assert not _passes(_stale_last_row(ref["want32"]), ref["want64"], ref["want32"])
    _check_signs(pres, "ffn76")


# ---- encoder layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.LAYER_CASES, ids=lambda c: c["id"])
def test_layer_checker(c):
    x, ref = pc.layer_case(c)
    G, B, S = c["G"], c["B"], c["S"]
    want64, want32 = ref["want64"], ref["want32"]
    assert pc.max_err(ref["restated64"], want64) < 1e-11          # the written-out layer IS nn.TransformerEncoderLayer
    _check_signs([(c["id"], ref["pre"])], "layer")
    sd = x["sd"]
    assert float((sd["norm1.weight"] - 1).abs().max()) > 0.1 and float(sd["norm2.bias"].abs().max()) > 0.1
    good = pc.from_seq(pc.layer_restated(sd, pc.to_seq(x["X"], G))[0], B, S)
    err, bound = pc.measure(good, want64, want32)
    pc.report(c["id"], err, bound)
    assert err <= bound
    assert not _passes(_stale_last_row(good.view(B * S, -1)), want64.view(B * S, -1), want32.view(B * S, -1))
    assert not _passes(pc.from_seq(pc.layer_restated(sd, pc.to_seq(x["X"], G), relu=False)[0], B, S), want64, want32)
    if G == 1:
        return                                                     # the softmax of one member is 1: nothing to plant
    peak = ref["weights"].amax(-1)
    assert float(peak.min()) >= pc.SPREAD[0] and float(peak.max()) <= pc.SPREAD[1], (float(peak.min()), float(peak.max()))
    for plant in ("drop64", "swap64", "head64"):
        assert pc.moved(want64, ref[plant], want32) >= pc.PLANT, plant
    for kw in (dict(drop_last=True), dict(swap=True), dict(nhead=1)):
        bad = pc.from_seq(pc.layer_restated(sd, pc.to_seq(x["X"], G), **kw)[0], B, S)
        assert not _passes(bad, want64, want32), kw


# ---- tail ---------------------------------------------------------------------------------------------------------------------
def test_tail_checker():
    pres = []
    for c in pc.TAIL_CASES:
        x, ref = pc.tail_case(c)
        pres.append((c["id"], ref["pre"]))
        assert _passes(ref["t32"], ref["t64"], ref["t32"]) and _passes(ref["r32"], ref["r64"], ref["r32"])
        t, r, _ = pc.tail_ref(x, c["mode"], leaky=False)
        assert not _passes(t, ref["t64"], ref["t32"]) and not _passes(r, ref["r64"], ref["r32"]), c["id"]
        assert not _passes(_stale_last_row(ref["r32"]), ref["r64"], ref["r32"])
        if c["mode"] != "matrix":                                  # a rotation: orthonormal, determinant + 1
            R = ref["r64"].view(-1, 3, 3)
            assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
            assert float((torch.linalg.det(R) - 1).abs().max()) < 1e-12
    _check_signs(pres, "tail")
    # the three modes read their heads differently: the 6d columns are x, y, z
    x, ref = pc.tail_case(pc.TAIL_CASES[2])
    R = ref["r64"].view(-1, 3, 3)
    assert float(R[:, :, 0].norm(dim=1).sub(1).abs().max()) < 1e-12


# ---- grouped nn.Transformer ---------------------------------------------------------------------------------------------------
def test_grouped_transformer_reference():
    from pope_amd import synth
    sd = {k: v for k, v in synth.mocope_state_dict(pc.XFMR_S, "6d").items() if k.startswith("transformer_mkpts.")}
    t64, t32 = (pc.load_transformer(sd, "transformer_mkpts", 76, dt) for dt in (torch.float64, torch.float32))
    g = torch.Generator().manual_seed(9)
    x = torch.randn(6, pc.XFMR_S, 76, generator=g)
    by3, by6, by3_32 = pc.run_grouped(t64, x.double(), x.double(), 3), pc.run_grouped(t64, x.double(), x.double(), 6), pc.run_grouped(t32, x, x, 3)
    # group by group, literally
    for q in range(2):
        one = pc.run_grouped(t64, x[3 * q:3 * q + 3].double(), x[3 * q:3 * q + 3].double(), 3)
        for k in ("memory", "out"):
            assert pc.max_err(one[k], by3[k][3 * q:3 * q + 3]) < 1e-12
    for k in ("memory", "out"):
        assert _passes(by3_32[k], by3[k], by3_32[k])
        assert pc.moved(by3[k], by6[k], by3_32[k]) >= pc.PLANT          # the grouping shows
        assert not _passes(by6[k].float(), by3[k], by3_32[k])


# ---- the op-level entries refuse what their launchers cannot serve (no HIP call is made) ------------------------------------------
def test_argument_refusals_without_gpu(hip_lib):
    table = pc.argument_refusals(hip_lib)
    assert len(table) > 60
    for what, status in table:
        assert status == -1, what
