"""CPU: the rig of test_gpu_loftr_layer_routes.py (tests/loftr_layer_checks.py) is sound — the case lists hold every seam value
of the linear attention, the inputs reach the regime each case is about, the comparison accepts a torch fp32 restatement that
sums in the kernels' order and rejects every planted fault on at least one case of the list."""
import functools

import pytest
import torch

import loftr_layer_checks as lc


@pytest.fixture(scope="module")
def seams(hip_lib):
    import ctypes
    c, r = ctypes.c_int(0), ctypes.c_int(0)
    hip_lib.pope_loftr_linear_attention_seams(ctypes.byref(c), ctypes.byref(r))
    assert c.value > 1 and r.value > 1
    return c.value, r.value


@pytest.fixture(scope="module")
def msd():
    from pope_amd import synth
    return synth.synthetic_matcher_state_dict(seed=0)


@functools.lru_cache(maxsize=None)
def _attention(case_id, c, r):
    case = next(k for k in lc.attention_cases(c, r) if k["id"] == case_id)
    q, kv, qm, km = lc.attention_inputs(case, c)
    return case, (q, kv, qm, km), lc.attention_ref(q, kv, qm, km), lc.attention_ref(q, kv, qm, km, torch.float32)


def test_attention_case_list_holds_every_seam(seams):
    c, r = seams
    Ss, Ls = lc.attention_lengths(c, r)
    assert Ss == (1, c - 1, c, c + 1, 2 * c + 1, 3 * c + 8) and Ls == (1, r - 1, r, r + 1, 2 * r + 1)
    cases = lc.attention_cases(c, r)
    assert len({k["id"] for k in cases}) == len(cases)
    for Cd in (256, 128):
        plain = [k for k in cases if k["C"] == Cd and k["mask"] is None]
        assert {k["S"] for k in plain} == set(Ss) and {k["L"] for k in plain} == set(Ls)
        assert {k["n"] for k in plain} == {1, 3}
        assert any(k["L"] == Ls[0] and k["S"] == Ss[0] for k in plain)                     # the smallest with each other
        assert any(k["L"] == Ls[0] and k["S"] == Ss[-1] for k in plain) and any(k["L"] == Ls[-1] and k["S"] == Ss[0] for k in plain)
        assert any(k["L"] % 2 == 1 and k["L"] > 1 for k in plain)                          # the two-rows-per-pass tail of C = 128
        masked = [k for k in cases if k["C"] == Cd and k["mask"] is not None]
        assert [k["mask"] for k in masked] == list(lc.MASK_KINDS)
        assert all((k["n"], k["L"], k["S"]) == (3, r + 1, 2 * c + 1) for k in masked)
    lay = lc.layer_cases(c, r)
    for prec in lc.LAYER_PRECISIONS:
        got = {(k["kind"], k["C"], k["n"], k["L"], k["S"], k["masked"]) for k in lay if k["precision"] == prec}
        assert got >= {("cross", 256, 1, 1, 1, False), ("cross", 256, 2, r + 1, c + 1, False), ("cross", 256, 3, c, 2 * c + 1, False),
                       ("self", 256, 2, c + 1, c + 1, False), ("self", 128, 2, 25, 25, False), ("cross", 128, 5, 25, 25, False),
                       ("cross", 256, 2, r + 1, c + 1, True)}


def test_masked_restatements_are_the_oracle_without_masks(seams, msd):
    from oracle import loftr_ref
    c, r = seams
    case = dict(C=128, n=2, L=r + 1, S=c + 1, mask=None, seed=7)
    q, kv, _, _ = lc.attention_inputs(case, c)
    Q, K, V = lc._split(q.double(), kv.double())
    want = loftr_ref.linear_attention(Q, K, V)
    assert torch.equal(lc.masked_linear_attention(Q, K, V), want)
    assert torch.equal(lc.masked_linear_attention(Q, K, V, torch.ones(2, r + 1), torch.ones(2, c + 1)), want)
    lcase = dict(prefix=lc.FINE, kind="cross", C=128, n=2, L=25, S=25, masked=False, seed=8)
    x, s, _, _ = lc.layer_inputs(lcase)
    sd64 = lc.as_dtype(lc.layer_state_full(msd, lc.FINE), torch.float64)
    assert torch.equal(lc.masked_encoder_layer(sd64, lc.FINE, x.double(), s.double(), lc.NHEAD),
                       loftr_ref.encoder_layer(sd64, lc.FINE, x.double(), s.double(), lc.NHEAD))


def test_attention_inputs_reach_their_regimes(seams):
    c, r = seams
    for case in lc.attention_cases(c, r):
        q, kv, qm, km = lc.attention_inputs(case, c)
        D = case["C"] // lc.NHEAD
        neg = slice(lc.NEG_HEAD * D, (lc.NEG_HEAD + 1) * D)
        assert float(q[..., neg].max()) < -5 and float(kv[..., neg].max()) < -5           # elu's negative branch carries the value
        den = lc.attention_denominator(q, kv, None, None)[..., lc.NEG_HEAD]
        assert lc.EPS / 100 <= float(den.min()) and float(den.max()) <= lc.EPS * 100, (case["id"], float(den.min()), float(den.max()))
        other = lc.attention_denominator(q, kv, None, None)[..., [h for h in range(lc.NHEAD) if h != lc.NEG_HEAD]]
        assert float(other.min()) > 1e3 * lc.EPS
        if case["mask"] in ("qmask", "both"):
            assert 0 < float(qm.sum()) < qm.numel()
        if case["mask"] in ("kvmask", "both"):
            assert 0 < float(km.sum()) < km.numel()
        if case["mask"] == "kvtail":
            tail = ((case["S"] - 1) // c) * c
            assert case["S"] - tail < c and float(km[:, tail:].sum()) == 0 and float(km[:, :tail].sum(1).min()) > 0
        if case["mask"] == "image":
            assert float(km[lc.MASKED_IMAGE].sum()) == 0 and float(km.sum(1)[[0, 2]].min()) > 0
            want = lc.attention_ref(q, kv, qm, km)
            assert float(want[lc.MASKED_IMAGE].abs().max()) == 0.0 and float(want[0].abs().max()) > 0
    _, q, kv = lc.flag_case(c, r)
    assert float(lc.attention_ref(q, kv).abs().max()) > lc.PLANES_LIMIT


def test_comparison_accepts_the_kernel_order_in_fp32(seams):
    c, r = seams
    worst = (0.0, None)
    for k in lc.attention_cases(c, r):
        case, (q, kv, qm, km), want64, want32 = _attention(k["id"], c, r)
        got = lc.attention_kernel_order(q, kv, qm, km, c)
        ratios = lc.head_ratios(got, want64, want32)
        worst = max(worst, (max(ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
    print(f"kernel-order fp32 restatement: worst ratio {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("fault", lc.ATTENTION_FAULTS)
def test_comparison_rejects_attention_faults(seams, fault):
    c, r = seams
    caught = []
    for k in lc.attention_cases(c, r):
        if fault in ("qmask_ignored", "kvmask_ignored") and k["mask"] is None:
            continue
        if fault == "wrong_image" and k["n"] == 1:
            continue
        case, (q, kv, qm, km), want64, want32 = _attention(k["id"], c, r)
        got = lc.attention_kernel_order(q, kv, qm, km, c, fault=fault, dtype=torch.float64).float()
        ratios = lc.head_ratios(got, want64, want32)
        if max(ratios) > 1.0:
            caught.append((max(ratios), case["id"]))
    assert caught, fault
    print(f"{fault}: caught on {len(caught)} cases, at most {max(caught)[0]:.3g} bounds ({max(caught)[1]})")
    if fault == "no_eps":       # without masks (a masked query row has 0 / 0) only the strongly negative head can tell
        for k in (k for k in lc.attention_cases(c, r) if k["mask"] is None):
            case, (q, kv, qm, km), want64, want32 = _attention(k["id"], c, r)
            ratios = lc.head_ratios(lc.attention_kernel_order(q, kv, qm, km, c, fault=fault, dtype=torch.float64).float(), want64, want32)
            assert ratios[lc.NEG_HEAD] > 1.0 and max(x for h, x in enumerate(ratios) if h != lc.NEG_HEAD) <= 1.0, (case["id"], ratios)


def _fine_case(case):
    xs = [lc.fine_match_inputs(case, M) for M in lc.FINE_M]
    want64 = torch.cat([lc.fine_match_ref(*x) for x in xs])
    want32 = torch.cat([lc.fine_match_ref(*x, dtype=torch.float32) for x in xs])
    return xs, want64, want32


def test_fine_match_inputs_reach_their_regimes():
    cases = lc.fine_match_cases()
    assert {k["W"] for k in cases} == set(lc.FINE_W) and {k["C"] for k in cases} == set(lc.FINE_C)
    assert 4 in lc.FINE_M and 5 in lc.FINE_M and 1 in lc.FINE_M          # four matches per workgroup: 5 crosses the seam
    assert 8 * 8 == 64                                                    # side 8 fills the wave
    for entry in lc.FINE_ENTRIES:
        assert {k["kind"] for k in cases if k["entry"] == entry} == set(lc.FINE_KINDS) | {"saturated"}
    for case in cases:
        for M in lc.FINE_M:
            w0, w1, mk, b_ids, scale1 = lc.fine_match_inputs(case, M)
            WW = case["W"] ** 2
            var, heat = lc.fine_match_variances(w0, w1)
            want = lc.fine_match_ref(w0, w1, mk, b_ids, scale1)
            if 2 in lc.fine_match_checked_columns(case["kind"]):
                assert float(var.min()) >= lc.VAR_FLOOR, (case["id"], M, float(var.min()))
            if case["kind"] == "peak_first":
                assert bool((heat.argmax(1) == 0).all()) and float(heat.max()) < 0.9
            if case["kind"] == "peak_last":
                assert bool((heat.argmax(1) == WW - 1).all()) and float(heat.max()) < 0.9
            if case["kind"] == "flat":
                assert float(want[:, :2].abs().max()) < 1e-12
            if case["kind"] == "saturated":
                assert float(heat.max(1).values.min()) > 1 - 1e-12
                assert float(want[:, 2].min()) >= lc.SPREAD_CLAMP
            if case["entry"] == "scaled":
                assert scale1.shape == (lc.FINE_IMAGES, 2) and len(set(scale1.flatten().tolist())) == 2 * lc.FINE_IMAGES
                assert M == 1 or len(set(b_ids.tolist())) > 1


@pytest.mark.parametrize("fault", lc.FINE_FAULTS)
def test_comparison_rejects_fine_match_faults(fault):
    caught = []
    for case in lc.fine_match_cases():
        if fault == "scale_axes_swapped" and case["entry"] != "scaled":
            continue
        xs, want64, want32 = _fine_case(case)
        got = torch.cat([lc.fine_match_fault(fault, *x) for x in xs]).float()
        ratios = lc.fine_match_ratios(case, got, want64, want32)
        if max(ratios) > 1.0:
            caught.append((max(ratios), case["id"]))
    assert caught, fault
    print(f"{fault}: caught on {len(caught)} cases, at most {max(caught)[0]:.3g} bounds ({max(caught)[1]})")


def test_comparison_accepts_fine_match_in_fp32():
    """the fp32 restatement itself sits at 1 / MARGIN of its own bound or below (the floor can only lower the ratio)"""
    for case in lc.fine_match_cases():
        xs, want64, want32 = _fine_case(case)
        assert max(lc.fine_match_ratios(case, want32, want64, want32)) <= 1.0 / lc.MARGIN + 1e-12


def test_fine_preprocess_streams_differ_and_the_fault_shows(msd):
    (h0, w0), (h1, w1) = lc.PRE_GRID0, lc.PRE_GRID1
    assert h0 != h1 and w0 != w1 and h0 * w0 != h1 * w1
    b, i, j = lc.fine_pre_matches(9)
    for ids, (h, w) in ((i, lc.PRE_GRID0), (j, lc.PRE_GRID1)):
        cells = {(int(v) // w, int(v) % w) for v in ids}
        assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)} <= cells
        inner = lambda y, x: 0 < y < h - 1 and 0 < x < w - 1   # noqa: E731
        assert any(y == 0 and 0 < x < w - 1 for y, x in cells) and any(y == h - 1 and 0 < x < w - 1 for y, x in cells)
        assert any(x == 0 and 0 < y < h - 1 for y, x in cells) and any(x == w - 1 and 0 < y < h - 1 for y, x in cells)
        assert any(inner(y, x) for y, x in cells)
    assert len(set(b.tolist())) == lc.PRE_N
    assert {(k["precision"], k["layout"], k["M"]) for k in lc.fine_pre_cases()} == {
        (p, lay, M) for p in lc.LAYER_PRECISIONS for lay in lc.PRE_LAYOUTS for M in (9, 1)}
    case = next(k for k in lc.fine_pre_cases() if k["M"] == 9)
    x = lc.fine_pre_inputs(case)
    want64, want32 = lc.fine_pre_ref(msd, *x), lc.fine_pre_ref(msd, *x, dtype=torch.float32)
    bad = lc.fine_pre_ref(msd, *x, fault="wc_of_stream0")
    assert lc.group_ratio(bad[0].float(), want64[0], want32[0]) <= 1.0       # stream 0 is not touched by the fault
    ratio = lc.group_ratio(bad[1].float(), want64[1], want32[1])
    print(f"wc_of_stream0: {ratio:.3g} bounds on stream 1")
    assert ratio > 1.0


def test_attention_entry_refuses_on_the_host(hip_lib):
    lc.assert_attention_refusals(hip_lib)
