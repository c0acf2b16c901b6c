"""GPU: the Sinkhorn coarse matcher (match_type='sinkhorn', csrc/sinkhorn.hip) against the fixture the reference's own
CoarseMatching / Matcher wrote (tests/golden/sinkhorn.npz, scripts/gen_golden_sinkhorn.py) and against the fp64 definition
(pope_amd/sinkhorn_cpu.py).  Match lists and coarse keypoints are exact; mconf and conf_matrix are held to the bound the
dual-softmax matcher's conf_matrix is held to (tests/test_gpu_match.py: rtol 1e-4, atol 1e-7).  The fixture script asserts
that no decision (threshold, dustbin prefilter) of any case or setting used here lies within 1e-3 of flipping.
Every test runs with both arithmetic modes of the L x S x C contraction."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-7
THR, BORDER = 0.2, 2


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "sinkhorn.npz"))


@pytest.fixture(autouse=True, params=["f16x3", "f32"])
def precision(request, monkeypatch):
    import pope_amd.matcher as m
    monkeypatch.setattr(m, "DEFAULT_PRECISION", request.param)
    return request.param


_cases = {}


def case_on(name, dev):
    """The seeded inputs of a case, built once and left unchanged."""
    if name not in _cases:
        from pope_amd import synth
        c = synth.sinkhorn_case(name)
        _cases[name] = {k: v.to(dev) if torch.is_tensor(v) else v for k, v in c.items()}
    return _cases[name]


def run(c, dev, bin_score=1.0, **kw):
    from pope_amd.matcher import dense_match
    return dense_match(c["feat0"], c["feat1"], c["hw0"], c["hw1"], c["hw0_i"], THR, BORDER, match_type="sinkhorn",
                       bin_score=torch.tensor(bin_score, device=dev), **kw)


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (ATOL / RTOL + np.abs(want))).max()) if got.size else 0.0


def same_lists(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("b_ids", "i_ids", "j_ids", "m_bids", "mconf", "mkpts0_c", "mkpts1_c"))


@pytest.mark.parametrize("name", ["12x16_vs_10x14", "32x32", "16x16_vs_12x16"])
def test_op_against_the_reference_fixture(dev, fx, name):
    c = case_on(name, dev)
    out = run(c, dev)
    st = int(fx[f"{name}.conf_stride"])
    conf = out["conf_matrix"][:, ::st, ::st].cpu().numpy()
    print(f"{name}: {len(out['b_ids'])} matches; error in units of the bound (rtol {RTOL:g}, atol {ATOL:g}): conf_matrix "
          f"{rel_err(conf, fx[f'{name}.conf_matrix']) / RTOL:.3f}, mconf {rel_err(out['mconf'].cpu(), fx[f'{name}.mconf']) / RTOL:.3f}")
    for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c"):
        assert np.array_equal(out[k].cpu().numpy(), fx[f"{name}.{k}"]), k
    assert np.array_equal(out["m_bids"].cpu().numpy(), fx[f"{name}.b_ids"])
    assert out["counts"].tolist() == np.bincount(fx[f"{name}.b_ids"], minlength=c["feat0"].shape[0]).tolist()
    np.testing.assert_allclose(out["mconf"].cpu().numpy(), fx[f"{name}.mconf"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(conf, fx[f"{name}.conf_matrix"], rtol=RTOL, atol=ATOL)


def test_iterations_dustbin_score_and_prefilter(dev):
    """Each of skh_iters {1, 3} x bin_score {1.0, 2.5, -0.5} x skh_prefilter {on, off} against the fp64 definition pushed through
    the CPU restatement of get_coarse_match; then one module whose parameter is overwritten in place between two calls."""
    from oracle import coarse_match_ref as cm
    from pope_amd import sinkhorn_cpu, synth
    from pope_amd.matcher import CoarseMatching, default_cfg
    c = case_on("12x16_vs_10x14", dev)
    f0, f1 = c["feat0"].cpu().double(), c["feat1"].cpu().double()
    want = {}
    for it, b, pre in synth.SINKHORN_SETTINGS:
        conf64 = sinkhorn_cpu.conf_matrix(f0, f1, b, it, pre)
        ref = cm.coarse_match(conf64, c["hw0"], c["hw1"], c["hw0_i"], THR, BORDER)
        want[it, b, pre] = (conf64, ref)
        out = run(c, dev, b, skh_iters=it, skh_prefilter=pre)
        e = rel_err(out["conf_matrix"].cpu(), conf64)
        print(f"iters {it} bin {b} prefilter {pre}: {len(ref['b_ids'])} matches, conf_matrix error {e / RTOL:.3f} of the bound")
        for k in ("b_ids", "i_ids", "j_ids"):
            assert torch.equal(out[k].cpu(), ref[k]), (it, b, pre, k)
        assert torch.equal(out["mkpts1_c"].cpu().double(), ref["mkpts1_c"].double())
        np.testing.assert_allclose(out["mconf"].cpu().numpy(), ref["mconf"].numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(out["conf_matrix"].cpu().numpy(), conf64.numpy(), rtol=RTOL, atol=ATOL)
    assert not torch.equal(want[3, 1.0, True][0], want[3, 2.5, True][0]) and not torch.equal(want[1, 1.0, True][0], want[3, 1.0, True][0])
    assert not torch.equal(want[3, 1.0, True][0], want[3, 1.0, False][0])
    # the kernels follow the parameter's storage: no value is cached on the host
    m = CoarseMatching(dict(default_cfg["match_coarse"], match_type="sinkhorn")).eval().to(dev)
    results = []
    for b in (1.0, 2.5):
        m.bin_score.data.fill_(b)
        data = {"hw0_c": c["hw0"], "hw1_c": c["hw1"], "hw0_i": c["hw0_i"]}
        m(c["feat0"], c["feat1"], data)
        results.append(data["conf_matrix"].clone())
        assert torch.equal(data["conf_matrix"], run(c, dev, b)["conf_matrix"])
        np.testing.assert_allclose(data["conf_matrix"].cpu().numpy(), want[3, b, True][0].numpy(), rtol=RTOL, atol=ATOL)
        assert torch.equal(data["i_ids"].cpu(), want[3, b, True][1]["i_ids"])
    assert not torch.equal(results[0], results[1])


def test_padding_masks_and_scales(dev, fx):
    """Pair 1 padded to 12 x 10 and 14 x 16 valid cells: fill masks, padded border, scales, as the reference publishes them; a
    row or column filled with -1e9 keeps only its dustbin (this is where a NaN would come from)."""
    name = "masked_16x16"
    c = case_on(name, dev)
    masks = dict(mask0=c["mask0"], mask1=c["mask1"], border_mask0=c["mask0"], border_mask1=c["mask1"])
    out = run(c, dev, scale0=c["scale0"], scale1=c["scale1"], **masks)
    for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c"):
        assert np.array_equal(out[k].cpu().numpy(), fx[f"{name}.{k}"]), k
    np.testing.assert_allclose(out["mconf"].cpu().numpy(), fx[f"{name}.mconf"], rtol=RTOL, atol=ATOL)
    conf = out["conf_matrix"]
    assert bool(conf.isfinite().all())
    np.testing.assert_allclose(conf.cpu().numpy(), fx[f"{name}.conf_matrix"], rtol=RTOL, atol=ATOL)
    m0, m1 = c["mask0"].flatten(1), c["mask1"].flatten(1)
    assert bool((~m0).any()) and bool((~m1).any())
    assert bool((conf[~m0] == 0).all()) and bool((conf.transpose(1, 2)[~m1] == 0).all())
    assert bool(m0[out["b_ids"], out["i_ids"]].all()) and bool(m1[out["b_ids"], out["j_ids"]].all())
    assert int(out["counts"][1]) >= 16
    plain = run(c, dev, **masks)
    assert all(torch.equal(plain[k], out[k]) for k in ("b_ids", "i_ids", "j_ids", "mconf", "conf_matrix"))
    b = out["b_ids"]
    assert torch.equal(out["mkpts0_c"], plain["mkpts0_c"] * c["scale0"][b]) and torch.equal(out["mkpts1_c"], plain["mkpts1_c"] * c["scale1"][b])
    assert not torch.equal(out["mkpts0_c"], plain["mkpts0_c"])


def test_degenerate_inputs(dev, fx):
    c = case_on("unrelated", dev)
    out = run(c, dev)
    assert out["counts"].tolist() == [0, 0] and out["counts"].dtype == torch.int32
    for k in ("b_ids", "i_ids", "j_ids", "m_bids"):
        assert out[k].shape == (0,) and out[k].dtype == torch.int64, k
    assert out["mconf"].shape == (0,) and out["mconf"].dtype == torch.float32 and out["gt_mask"].dtype == torch.bool
    assert out["mkpts0_c"].shape == (0, 2) and out["mkpts1_c"].shape == (0, 2) and out["mkpts0_c"].dtype == torch.float32
    np.testing.assert_allclose(out["conf_matrix"].cpu().numpy(), fx["unrelated.conf_matrix"], rtol=RTOL, atol=ATOL)
    empty = dict(c, feat0=c["feat0"][:0], feat1=c["feat1"][:0])
    out = run(empty, dev)
    assert out["b_ids"].shape == (0,) and out["conf_matrix"].shape == (0, 192, 140) and out["counts"].shape == (0,)
    c = case_on("12x16_vs_10x14", dev)
    full, lists = run(c, dev), run(c, dev, want_conf=False)
    assert lists["conf_matrix"] is None and len(full["b_ids"]) > 0 and same_lists(full, lists)
    assert full["counts"].tolist() == lists["counts"].tolist()


def test_pairs_do_not_depend_on_their_batch(dev):
    c = case_on("32x32", dev)
    out = run(c, dev)
    for b in range(3):
        one = run(dict(c, feat0=c["feat0"][b:b + 1], feat1=c["feat1"][b:b + 1]), dev)
        sel = out["b_ids"] == b
        assert int(sel.sum()) == len(one["b_ids"]) > 0
        for k in ("i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c"):
            assert torch.equal(out[k][sel], one[k]), (b, k)
        assert torch.equal(out["conf_matrix"][b], one["conf_matrix"][0])


def test_range_guard(dev, precision):
    """A feature beyond the f16x3 contract: the call warns and returns what the fp32 contraction returns, or raises."""
    from pope_amd._lib import PopeRangeError
    c = case_on("16x16_vs_12x16", dev)
    big = dict(c, feat0=c["feat0"].clone())
    big["feat0"][0, 70, 5] = 6000.0   # |feat| / sqrt(C) * 256 >= 65504 from |feat| = 4094
    want = run(big, dev, precision="f32")
    if precision == "f32":   # no planes, no contract
        assert same_lists(run(big, dev), want)
        return
    with pytest.warns(UserWarning, match="dense_match"):
        got = run(big, dev)
    assert same_lists(got, want) and torch.equal(got["conf_matrix"], want["conf_matrix"]) and len(want["b_ids"]) > 0
    with pytest.raises(PopeRangeError):
        run(big, dev, on_overflow="raise")


def test_matcher_end_to_end(dev, fx, golden_dir):
    """The reference's Matcher with match_type='sinkhorn' on two pairs of 128 x 128 images: strict load of a state dict with
    coarse_matching.bin_score, coarse ids equal, fine keypoints within the bounds tests/test_gpu_loftr.py uses; the captured-
    graph front and a shared reference encoding give the eager result bit for bit; a dual-softmax Matcher beside it is unmoved."""
    from pope_amd import synth
    from pope_amd.matcher import Matcher, default_cfg
    peaked = np.load(os.path.join(golden_dir, "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(peaked["outconv_mean"]), seed=0, gain=float(fx["matcher.gain"]))
    sd.pop("_calibration_mean")
    ds = Matcher(default_cfg).eval()
    ds.load_state_dict(dict(sd), strict=True)
    sd["coarse_matching.bin_score"] = torch.tensor(float(fx["matcher.bin_score"]))
    cfg = dict(default_cfg, match_coarse=dict(default_cfg["match_coarse"], match_type="sinkhorn", sparse_spvs=False))
    m = Matcher(cfg).eval()
    m.load_state_dict(dict(sd), strict=True)
    m, ds = m.to(dev), ds.to(dev)
    i0, i1 = (t.to(dev) for t in synth.synthetic_gray_pairs(2, 128, 128, seed=61))
    data = {"image0": i0, "image1": i1}
    m(data)
    for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c"):
        assert np.array_equal(data[k].cpu().numpy(), fx[f"matcher.{k}"]), k
    e_conf = float(np.abs(data["mconf"].cpu().numpy() - fx["matcher.mconf"]).max())
    e_px = max(float(np.abs(data[k].cpu().numpy() - fx[f"matcher.{k}"]).max()) for k in ("mkpts0_f", "mkpts1_f"))
    print(f"matcher: {len(data['b_ids'])} matches, mconf max err {e_conf:.2e} (bound 2e-4), mkpts*_f max err {e_px:.2e} px (bound 5e-4)")
    assert e_conf <= 2e-4 and e_px <= 5e-4
    keys = ("b_ids", "i_ids", "j_ids", "mconf", "conf_matrix", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f")
    m.use_graph = True
    for _ in range(3):   # eager, capture, replay
        again = {"image0": i0, "image1": i1}
        m(again)
        assert all(torch.equal(again[k], data[k]) for k in keys)
    m.use_graph = False
    ref = m.encode_reference(i0[:1])
    shared = {"reference": ref, "image0_index": torch.tensor([0, 0]), "image1": i1}
    m(shared)
    plain = {"image0": i0[:1].expand(2, -1, -1, -1).contiguous(), "image1": i1}
    m(plain)
    assert len(plain["b_ids"]) > 0 and all(torch.equal(shared[k], plain[k]) for k in keys)
    # a dual-softmax Matcher beside it: its own state-dict keys, and the reference fixture of the default configuration
    assert "coarse_matching.bin_score" not in ds.state_dict() and not hasattr(ds.coarse_matching, "bin_score")
    fd = np.load(os.path.join(golden_dir, "loftr_256.npz"))
    dsm = Matcher(dict(default_cfg, match_coarse=dict(default_cfg["match_coarse"], thr=float(fd["thr"])))).eval()
    dsm.load_state_dict(synth.synthetic_matcher_state_dict(seed=0), strict=True)
    j0, j1 = (t.to(dev) for t in synth.synthetic_gray_pairs(int(fd["n"]), *(int(v) for v in fd["shape0"]), seed=21))
    out = {"image0": j0, "image1": j1}
    dsm.to(dev)(out)
    got = set(zip(*(out[k].tolist() for k in ("b_ids", "i_ids", "j_ids"))))
    clear = [t for t, c in zip(zip(fd["b_ids"].tolist(), fd["i_ids"].tolist(), fd["j_ids"].tolist()), fd["mconf"]) if abs(c - THR) > 1e-3]
    assert len(clear) > 10 and set(clear) <= got and len(got) <= len(fd["b_ids"]) + (len(fd["b_ids"]) - len(clear))
    np.testing.assert_allclose(out["conf_matrix"].max(2)[0].cpu().numpy(), fd["conf_rowmax"], rtol=2e-3, atol=1e-7)
