"""GPU: the dense matcher's confidence pass at every switch of its route table, against fp64.

launch_conf_pass (match.hip) picks a kernel from S alone — conf_pass_kernel for odd S (chunks of 1024), conf_pass_fast_kernel<NK>
for even S (NK = 4 / 8 / 12 / 16, chunks of 2048 beyond S = 2048) — and the Sinkhorn matcher ends in skh_conf_kernel (chunks of
1024); each has a row tail and a PUBLISH / non-PUBLISH twin.  Cases, seeded inputs, fp64 references and the comparison are
match_route_checks.py's (test_match_route_checks_cpu.py shows that no decision of a case lies within 1e-3 of flipping and which
faults the comparison rejects).  Every case asserts, in both arithmetic modes of the contraction:
  want_conf=True   match lists, counts and coarse keypoints equal to the fp64 reference's; mconf and the WHOLE conf_matrix within
                   rtol 1e-4, atol 1e-7 of it (the bounds of test_gpu_match.py / test_gpu_sinkhorn.py)
  want_conf=False  every list entry bit for bit that of the published run: the non-PUBLISH kernels, and for the tie cases the
                   scalar conf_value of select_kernel's re-scan against the packed conf_value2 of the fast pass
  tie cases        the expected j_id of a row whose two maxima lie in different chunks, and bit-equal twin columns
Measured errors: profiles/match_routes.md."""
import pytest
import torch

import match_route_checks as K

pytestmark = pytest.mark.gpu
SAME_KEYS = ("b_ids", "i_ids", "j_ids", "m_bids", "mconf", "mkpts0_c", "mkpts1_c", "gt_mask")


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True, params=["f16x3", "f32"])
def precision(request, monkeypatch):
    """Every test of this module runs with both arithmetic modes of the L x S x C contraction."""
    import pope_amd.matcher as m
    monkeypatch.setattr(m, "DEFAULT_PRECISION", request.param)
    return request.param


_on_dev = {}


def run(d, dev, want_conf=True, pair=None):
    """dense_match on a built case (pair: that pair alone, as a batch of one)."""
    from pope_amd.matcher import dense_match
    c = d["case"]
    if c["id"] not in _on_dev:
        _on_dev[c["id"]] = (d["f0"].to(dev), d["f1"].to(dev))
    f0, f1 = _on_dev[c["id"]]
    if pair is not None:
        f0, f1 = f0[pair:pair + 1], f1[pair:pair + 1]
    if c["kind"] == "skh":
        how = dict(match_type="sinkhorn", bin_score=torch.tensor(K.SKH_BIN_SCORE, device=dev), skh_iters=K.SKH_ITERS,
                   skh_prefilter=c["prefilter"])
    else:
        how = dict(temperature=K.TEMPERATURE)
    out = dense_match(f0, f1, c["hw0"], c["hw1"], d["hw0_i"], K.THR, c["border"], want_conf=want_conf, on_overflow="raise", **how)
    torch.cuda.synchronize()
    return out


def assert_same_lists(a, b, what):
    for k in SAME_KEYS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{what}: {k}"
    assert a["counts"].tolist() == b["counts"].tolist(), f"{what}: counts"


@pytest.mark.parametrize("c", K.ALL_CASES, ids=K.case_id)
def test_route_against_fp64(dev, precision, c):
    d = K.build(c)
    full = run(d, dev)
    e, e32 = K.check(d, full, precision)
    print(f"{c['id']:48s} {precision:5s} {K.route_name(c)}: {len(full['b_ids'])} matches, error {e:.3f} of the bound "
          f"(fp32 oracle {e32:.3f}); pins {c['pins']}")
    lists = run(d, dev, want_conf=False)
    assert lists["conf_matrix"] is None
    assert_same_lists(lists, full, f"{c['id']} want_conf=False against want_conf=True")
    if c["tie"]:
        K.check_ties(d, full)
        K.check_ties(d, lists)


@pytest.mark.parametrize("c", [K.find("ds", S=2050, L=63), K.find("ds", S=1025, L=63), K.find("skh", S=2057)], ids=K.case_id)
def test_pair_does_not_depend_on_its_batch(dev, c):
    """One chunked case per kernel family: pair 1 alone gives the bits it gives inside the batch, published or not."""
    d = K.build(c)
    for want_conf in (True, False):
        out, one = run(d, dev, want_conf), run(d, dev, want_conf, pair=1)
        sel = out["b_ids"] == 1
        assert int(sel.sum()) == len(one["b_ids"]) == int(d["ref"]["counts"][1]) > 0
        for k in ("i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c"):
            assert torch.equal(out[k][sel], one[k]), (want_conf, k)
        if want_conf:
            assert torch.equal(out["conf_matrix"][1], one["conf_matrix"][0])
