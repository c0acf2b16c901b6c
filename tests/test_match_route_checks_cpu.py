"""The host side of test_gpu_match_routes.py (match_route_checks.py): the case table straddles every switch of the confidence
pass, the seeded inputs leave no decision of the fp64 reference near flipping (which is what lets the GPU test demand exact
lists) and do not saturate the confidences, the comparison accepts the fp32 oracle standing in for the kernels on every case,
and it rejects stand-ins with the faults a chunked confidence pass is likely to have — on the very case data.  Host only."""
import pytest
import torch

import match_route_checks as K
from pope_amd import sinkhorn_cpu


def test_table_straddles_every_switch():
    """The route mirror on the table: each NK with its largest S and the first S of the next, one / two / three chunks of every
    kernel with last chunks of 1, 2 and 4 columns, and the row tails."""
    routes = {(c["S"], c["L"]): K.route(c["kind"], c["L"], c["S"]) for c in K.DS_CASES}
    fast = lambda S: routes[S, 63][1:3]
    assert [fast(S) for S in (512, 516, 1024, 1026, 1536, 1540, 2048, 2050, 4100)] == \
        [(4, 1), (8, 1), (8, 1), (12, 1), (12, 1), (16, 1), (16, 1), (16, 2), (16, 3)]
    assert 2050 - K.FAST_CHUNK == 2 and 4100 - 2 * K.FAST_CHUNK == 4
    odd = lambda S: routes[S, 63]
    assert [odd(S)[0] for S in (1023, 1025, 2057)] == ["conf_pass_kernel"] * 3 and [odd(S)[2] for S in (1023, 1025, 2057)] == [1, 2, 3]
    assert {K.route("skh", c["L"], c["S"])[2] for c in K.SKH_CASES} == {1, 2, 3}
    assert (1023 + 1) % 64 == 0                                               # skh_cols_kernel's last block is full
    assert sorted({c["L"] for c in K.ROW_CASES}) == [1, 7, 33, 65]
    assert {K.route("ds", c["L"], c["S"])[0] for c in K.ROW_CASES} == {"conf_pass_kernel", "conf_pass_fast_kernel"}
    assert all(K.route("ds", c["L"], c["S"])[3] == 65 and -(-c["L"] // 256) == 9 for c in K.MANY_ROW_CASES)
    assert all(c["border"] == (0 if c in K.ROW_CASES or c["L"] == 7 else 2) for c in K.ALL_CASES)


def _loftr_clear_decisions(conf, thr, border, hw0, hw1):
    """tests/test_gpu_loftr.py:_clear_decisions, verbatim (border >= 1, L and S >= 2)."""
    n, L, S = conf.shape
    m = torch.ones(n, hw0[0], hw0[1], hw1[0], hw1[1], dtype=torch.bool)
    bd = border
    m[:, :bd] = m[:, -bd:] = False
    m[:, :, :bd] = m[:, :, -bd:] = False
    m[:, :, :, :bd] = m[:, :, :, -bd:] = False
    m[:, :, :, :, :bd] = m[:, :, :, :, -bd:] = False
    inside = m.reshape(n, L, S)
    top2r = conf.topk(2, dim=2).values
    top2c = conf.topk(2, dim=1).values
    rmax, rsec = top2r[..., 0:1], top2r[..., 1:2]
    cmax, csec = top2c[:, 0:1, :], top2c[:, 1:2, :]
    must = inside & (conf > thr + K.CLEAR) & (conf == rmax) & (conf == cmax) & (rmax - rsec > K.CLEAR) & (cmax - csec > K.CLEAR)
    may = inside & (conf > thr - K.CLEAR) & (conf >= rmax - K.CLEAR) & (conf >= cmax - K.CLEAR)
    return must, may


def test_clear_decisions_generalise_the_loftr_rule():
    d = K.build(K.find("ds", S=1026))
    must, may = _loftr_clear_decisions(d["conf64"], K.THR, 2, d["case"]["hw0"], d["case"]["hw1"])
    assert torch.equal(must, d["must"]) and torch.equal(may, d["may"]) and int(must.sum()) > 0
    # border 0 keeps every cell; a single row has no runner-up in its column
    d = K.build(K.find("ds", S=130, L=1))
    assert int(d["must"].sum()) == 2 and torch.equal(d["must"], d["may"])
    conf = d["conf64"]
    assert torch.equal(d["must"], (conf == conf.max(2, keepdim=True)[0]) & (conf > K.THR))


@pytest.mark.parametrize("c", K.ALL_CASES, ids=K.case_id)
def test_inputs_leave_no_decision_near_flipping(c):
    d = K.build(c)
    ref = d["ref"]
    unclear = int((d["may"] != d["must"]).sum())
    got = torch.zeros_like(d["must"])
    got[ref["b_ids"], ref["i_ids"], ref["j_ids"]] = True
    mc = d["conf64"][ref["b_ids"], ref["i_ids"], ref["j_ids"]]
    print(f"{c['id']}: {K.route_name(c)}; {len(mc)} matches {ref['counts'].tolist()}, conf {float(mc.min()):.3f} .. {float(mc.max()):.3f}, "
          f"{unclear} unclear decisions, fp32 oracle at {d['oracle_units']:.3f} of the bound")
    assert unclear == 0 and torch.equal(got, d["must"])
    assert len(mc) > 0 and int(ref["counts"].min()) > 0
    assert tuple(d["f0"].shape) == (K.N_PAIRS, c["L"], K.C_DS if c["kind"] == "ds" else K.C_SKH) and d["f0"].dtype == torch.float32
    if c["kind"] == "skh":
        a = sinkhorn_cpu.assignment(d["f0"].double(), d["f1"].double(), K.SKH_BIN_SCORE, K.SKH_ITERS)
        rows, cols = sinkhorn_cpu.dustbin_margins(a)
        assert float(rows.min()) > 1e-3 and float(cols.min()) > 1e-3, (float(rows.min()), float(cols.min()))


def test_confidences_are_not_saturated():
    """Matched confidences spread instead of sitting at 1.000 (the amplitude-3 recipe of test_gpu_match.py gives 1.000 to nine
    digits, so a wrong column statistic could not move a decision or fail a value check)."""
    lo, hi = 1.0, 0.0
    for c in K.DS_CASES:
        d = K.build(c)
        mc = d["conf64"][d["ref"]["b_ids"], d["ref"]["i_ids"], d["ref"]["j_ids"]]
        lo, hi = min(lo, float(mc.min())), max(hi, float(mc.max()))
        if c in K.COLUMN_CASES:
            assert float(mc.min()) < 0.7 < 0.9 < float(mc.max()), c["id"]
    assert lo < 0.7 and hi > 0.9


def test_sinkhorn_prefilter_zeroes_some_and_keeps_some():
    for c in K.SKH_CASES:
        if not c["prefilter"]:
            continue
        d = K.build(c)
        conf = d["conf64"]
        dead_rows, dead_cols = (conf.sum(2) == 0), (conf.sum(1) == 0)
        assert bool(dead_rows.any()) and bool((~dead_rows).any()) and bool(dead_cols.any()) and bool((~dead_cols).any()), c["id"]
        open_ = sinkhorn_cpu.conf_matrix(d["f0"].double(), d["f1"].double(), K.SKH_BIN_SCORE, K.SKH_ITERS, False)
        assert bool((open_ > 0).all())   # the zeros are the prefilter's


@pytest.mark.parametrize("c", [c for c in K.ALL_CASES if c["tie"]], ids=K.case_id)
def test_tie_cases_tie_across_chunks(c):
    d = K.build(c)
    chunk = K.chunk_of(c["kind"], c["S"])
    w1, b = c["hw1"][1], c["border"]
    interior = lambda s: b <= s // w1 < c["hw1"][0] - b and b <= s % w1 < w1 - b
    for pair, i, j, j2, e in K.expected_ties(d):
        assert j < chunk <= j2 and torch.equal(d["f1"][pair, j], d["f1"][pair, j2])
        assert torch.equal(d["conf64"][pair, :, j], d["conf64"][pair, :, j2])
        row = d["conf64"][pair, i]
        assert float(row[j]) == float(row.max()) > K.THR + K.CLEAR and int((row == row.max()).sum()) == 2
        assert interior(j) == (c["tie"] == "a") and (c["tie"] == "a" or j // w1 < b)
        assert e == (j if c["tie"] == "a" else j2 if interior(j2) else -1)
        # only S = 2050 and S = 1025 have no interior cell beyond chunk 0: every other variant b expects j'
        assert interior(j2) or c["S"] in (2050, 1025)
    K.check_ties(d, dict(d["ref"], conf_matrix=d["conf64"]))


@pytest.mark.parametrize("c", K.ALL_CASES, ids=K.case_id)
def test_comparison_accepts_the_fp32_oracle(c):
    d = K.build(c)
    e, e32 = K.check(d, K.stand_in(d, K.oracle32(d)), "fp32 oracle")
    assert e == pytest.approx(e32) or e32 < e <= 1.0
    assert e32 < 0.5      # measured: at most 0.14 of the bound


# ---- stand-ins that are subtly wrong, each from the fp32 oracle's conf -------------------------------------------------------
def test_rejects_a_column_denominator_off_by_1e_3_in_the_last_chunk():
    """Case L2050 x S2050: every column is planted, so column 2049 (the last chunk's second) carries a confidence near 1."""
    d = K.build(K.find("ds", S=2050, L=2050))
    conf = K.oracle32(d)
    assert float(d["conf64"][:, :, 2049].max()) > 0.2
    conf[:, :, 2049] /= 1.0 + 1e-3
    with pytest.raises(AssertionError, match="conf_matrix is .* of the bound"):
        K.check(d, K.stand_in(d, conf))


@pytest.mark.parametrize("S", [4100, 2057])
def test_rejects_a_row_argmax_over_the_first_chunk_only(S):
    d = K.build(K.find("ds", S=S, L=63))
    conf = K.oracle32(d)
    first = conf.clone()
    first[:, :, K.chunk_of("ds", S):] = 0
    assert int((d["ref"]["j_ids"] >= K.chunk_of("ds", S)).sum()) > 0
    with pytest.raises(AssertionError, match="j_ids|i_ids|b_ids"):
        K.check(d, K.stand_in(d, conf, lists_from=first))


@pytest.mark.parametrize("S", [2050, 4100, 1025, 2057])
def test_rejects_a_tie_resolved_to_the_highest_index(S):
    d = K.build(K.find("ds", S=S, tie="a"))
    out = K.stand_in(d, K.oracle32(d))
    for b, i, j, j2, e in K.expected_ties(d):
        k = int(((out["b_ids"] == b) & (out["i_ids"] == i)).nonzero())
        assert int(out["j_ids"][k]) == j
        out["j_ids"][k] = j2
    with pytest.raises(AssertionError, match="j_ids"):
        K.check(d, out)
    with pytest.raises(AssertionError, match="expected j_id"):
        K.check_ties(d, out)


@pytest.mark.parametrize("L", [33, 65])
def test_rejects_column_maxima_that_ignore_the_last_row_block(L):
    """In general such a pass accepts a row whose column holds a larger value in the last block (a match that is not mutual);
    with injective plants it shows as the last block's own matches failing `conf == column maximum`.  Either way the lists
    differ.  (The row cases have border_rm = 0 for this: at L = 2050, border 2, the last block's two rows lie in the border.)"""
    d = K.build(K.find("ds", S=130, L=L))
    conf = K.oracle32(d)
    blind = conf.clone()
    blind[:, (L - 1) // K.CP_ROWS * K.CP_ROWS:] = 0     # what the selection sees: column maxima of the earlier blocks only
    with pytest.raises(AssertionError, match="j_ids|i_ids|b_ids"):
        K.check(d, K.stand_in(d, conf, lists_from=blind))


def test_rejects_two_rows_swapped_in_the_compacted_list():
    d = K.build(K.find("ds", S=512))
    out = K.stand_in(d, K.oracle32(d))
    for k in K.LIST_KEYS + ("mconf",):
        if k != "b_ids":
            out[k][[0, 1]] = out[k][[1, 0]]
    with pytest.raises(AssertionError, match="i_ids"):
        K.check(d, out)


@pytest.mark.parametrize("S", [1025, 2057, 99])
def test_rejects_a_last_odd_column_left_at_its_sim_value(S):
    d = K.build(K.find("ds", S=S))
    conf = K.oracle32(d)
    good = conf.clone()
    f0, f1 = d["f0"] / K.C_DS ** .5, d["f1"] / K.C_DS ** .5
    conf[:, :, -1] = torch.einsum("nlc,nc->nl", f0, f1[:, -1]) / K.TEMPERATURE
    with pytest.raises(AssertionError, match="conf_matrix"):
        K.check(d, K.stand_in(d, conf, lists_from=good))


def test_rejects_a_wrong_mconf_and_a_wrong_count():
    d = K.build(K.find("ds", S=1540))
    out = K.stand_in(d, K.oracle32(d))
    out["mconf"] = out["mconf"] * (1 + 3e-4)
    with pytest.raises(AssertionError, match="mconf"):
        K.check(d, out)
    out = K.stand_in(d, K.oracle32(d))
    out["counts"] = out["counts"].flip(0)
    with pytest.raises(AssertionError, match="counts"):
        K.check(d, out)
