"""GPU: padded batches (mask0 / mask1) and per-pair rescaling (scale0 / scale1) through the drop-in LoFTR `Matcher`, its
`CoarseMatching`, `LocalFeatureTransformer`, `LoFTREncoderLayer` and `FineMatching` — against the fixtures the reference's own
modules wrote (scripts/gen_golden_masked.py), with the bounds of tests/test_gpu_loftr.py: features <= 1e-4, mconf <= 2e-4,
mkpts1_f <= 5e-4 px, the match list index-exact wherever the reference's decision is clear by 1e-3; coarse keypoints and
mkpts0_f bit-equal on common matches.  All-ones masks must reproduce the unmasked results bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT_ATOL = 1e-4
PX_ATOL = 5e-4
CLEAR = 1e-3
BORDER = 2


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def build(thr, dev):
    from pope_amd import synth
    from pope_amd.matcher import Matcher, default_cfg
    cfg = copy.deepcopy(default_cfg)
    cfg["match_coarse"]["thr"] = float(thr)
    m = Matcher(cfg).eval()
    m.load_state_dict(synth.synthetic_matcher_state_dict(seed=0), strict=True)
    return m.to(dev)


def case(name, dev, keys=("image0", "image1", "mask0", "mask1", "scale0", "scale1")):
    from pope_amd import synth
    inp, thr = synth.masked_loftr_case(name)
    return {k: inp[k].to(dev) for k in keys}, thr


def padded_limit(e, b, n):
    """First index of the bottom / right border: the reference's `m[k, e - b:]` (Python slice start)."""
    s = e - b
    if s < 0:
        s += n
    return max(s, 0)


def inside(m0, m1, b_ids, i_ids, j_ids, border=BORDER):
    """Per match: inside the padded border rule (coarse_matching.py:28-43) computed from the [n, h, w] masks."""
    out = []
    for b, i, j in zip(b_ids, i_ids, j_ids):
        ok = True
        for m, idx in ((m0[b], i), (m1[b], j)):
            H, W = m.shape
            y, x = divmod(int(idx), W)
            eh, ew = int(m.sum(0).max()), int(m.sum(1).max())
            ok &= border <= y < padded_limit(eh, border, H) and border <= x < padded_limit(ew, border, W)
        out.append(ok)
    return np.array(out, bool)


def clear_decisions(fx, thr, got):
    """The clear-decision rule of test_gpu_loftr.py:_clear_decisions from the fixture's top-2 values per row and column:
    (reference matches clear by CLEAR, published matches the reference could accept within CLEAR)."""
    rv, ri, cv, ci = fx["conf_row_top2"], fx["conf_row_top2_idx"], fx["conf_col_top2"], fx["conf_col_top2_idx"]
    n, L = rv.shape[:2]
    bb, ii = np.meshgrid(np.arange(n), np.arange(L), indexing="ij")
    jj = ri[..., 0]
    v = rv[..., 0]
    ins = inside(fx["mask0"], fx["mask1"], bb.ravel(), ii.ravel(), jj.ravel()).reshape(n, L)
    must = ins & (v > thr + CLEAR) & (ci[bb, 0, jj] == ii) & (cv[bb, 0, jj] == v) & (rv[..., 0] - rv[..., 1] > CLEAR) \
        & (cv[bb, 0, jj] - cv[bb, 1, jj] > CLEAR)
    must_set = {(int(b), int(i), int(jj[b, i])) for b, i in zip(*np.nonzero(must))}
    may = []
    for b, i, j in got:
        val = rv[b, i, 0] if j == ri[b, i, 0] else rv[b, i, 1]   # not in the top 2: bounded by the runner-up
        ok = inside(fx["mask0"], fx["mask1"], [b], [i], [j])[0]
        may.append(bool(ok and val > thr - CLEAR and val >= rv[b, i, 0] - CLEAR and val >= cv[b, 0, j] - CLEAR))
    return must_set, np.array(may, bool)


@pytest.mark.parametrize("name", ["loftr_masked_256", "loftr_masked_192x256_vs_256x192"])
def test_masked_matcher_end_to_end(dev, golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    data, thr = case(name, dev)
    m = build(thr, dev)
    assert m(data) is None
    f0, f1 = m(case(name, dev)[0], only_att_fea=True)          # only_att_fea honours the masks
    tap = int(fx["tap"])
    err_f = max(float(np.abs(f0[:, ::tap].cpu().numpy() - fx["feat_c0"]).max()),
                float(np.abs(f1[:, ::tap].cpu().numpy() - fx["feat_c1"]).max()))
    got = [tuple(t) for t in torch.stack([data["b_ids"], data["i_ids"], data["j_ids"]], 1).cpu().tolist()]
    must, may = clear_decisions(fx, float(fx["thr"]), got)
    ref = [(int(b), int(i), int(j)) for b, i, j in zip(fx["b_ids"], fx["i_ids"], fx["j_ids"])]
    print(f"{name}: features max err {err_f:.2e}; {len(ref)} reference matches, {len(must)} clear; published {len(got)}")
    assert err_f <= FEAT_ATOL
    assert must <= set(got), "a clear reference match is missing"
    assert bool(may.all()), "a match the reference clearly rejects was published"
    assert len(must) >= 0.8 * len(ref) > 0
    if len(must) == len(ref):
        assert got == ref
    pos = {t: k for k, t in enumerate(ref)}
    gi = [k for k, t in enumerate(got) if t in pos]
    ri = [pos[got[k]] for k in gi]
    e_conf = float(np.abs(data["mconf"].cpu().numpy()[gi] - fx["mconf"][ri]).max())
    e_px = float(np.abs(data["mkpts1_f"].cpu().numpy()[gi] - fx["mkpts1_f"][ri]).max())
    print(f"{name}: mconf max err {e_conf:.2e}, mkpts1_f max err {e_px:.2e} px")
    assert e_conf <= 2e-4 and e_px <= PX_ATOL
    for k in ("mkpts0_c", "mkpts1_c", "mkpts0_f"):
        assert np.array_equal(data[k].cpu().numpy()[gi], fx[k][ri]), k
    order = data["b_ids"].cpu().numpy() * 10 ** 6 + data["i_ids"].cpu().numpy()
    assert np.all(np.diff(order) > 0)
    # the conf matrix the GPU published agrees with the reference's row maxima
    np.testing.assert_allclose(data["conf_matrix"].max(2)[0].cpu().numpy(), fx["conf_row_top2"][..., 0], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("name", ["loftr_masked_256", "loftr_masked_192x256_vs_256x192"])
def test_scale1_without_scale0_keeps_the_fine_offset_unscaled(dev, golden_dir, name):
    """fine_matching.py:68 keys the fine rescaling on 'scale0': with only scale1, mkpts1_c is scaled and the offset is not."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    data, thr = case(name, dev, keys=("image0", "image1", "mask0", "mask1", "scale1"))
    build(thr, dev)(data)
    got = [tuple(t) for t in torch.stack([data["b_ids"], data["i_ids"], data["j_ids"]], 1).cpu().tolist()]
    pos = {(int(b), int(i), int(j)): k for k, (b, i, j) in enumerate(zip(fx["b_ids"], fx["i_ids"], fx["j_ids"]))}
    gi = [k for k, t in enumerate(got) if t in pos]
    ri = [pos[got[k]] for k in gi]
    assert len(gi) >= 0.8 * len(pos)
    assert np.array_equal(data["mkpts1_c"].cpu().numpy()[gi], fx["s1only_mkpts1_c"][ri])
    assert np.array_equal(data["mkpts0_f"].cpu().numpy()[gi], fx["s1only_mkpts0_f"][ri])
    assert float(np.abs(data["mkpts1_f"].cpu().numpy()[gi] - fx["s1only_mkpts1_f"][ri]).max()) <= PX_ATOL


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_masked_coarse_stage_at_the_loftr_grid_is_index_exact(dev, golden_dir, precision, monkeypatch):
    """CoarseMatching at the 32 x 32 grid of 256 x 256 images with the loftr_masked_256 masks and scales (coarse_masked_1024):
    fill from mask_c0 / mask_c1, padded border from data['mask0'/'mask1'], scales from data; identical (b, i, j), ordering
    included, coarse keypoints bit-equal."""
    from pope_amd import matcher, synth
    from pope_amd.matcher import CoarseMatching, default_cfg
    fx = np.load(os.path.join(golden_dir, "coarse_masked_1024.npz"))
    f0, f1, m0, m1, s0, s1, thr = synth.masked_coarse_case_large()
    assert np.allclose([float(f0.double().sum()), float(f1.double().sum())], fx["feat_digest"], rtol=0, atol=1e-6)
    h, w = m0.shape[1:]
    m0, m1 = m0.to(dev), m1.to(dev)
    data = {"hw0_i": (8 * h, 8 * w), "hw1_i": (8 * h, 8 * w), "hw0_c": (h, w), "hw1_c": (h, w), "mask0": m0, "mask1": m1,
            "scale0": s0.to(dev), "scale1": s1.to(dev)}
    monkeypatch.setattr(matcher, "DEFAULT_PRECISION", precision)   # CoarseMatching's contraction route
    CoarseMatching(dict(default_cfg["match_coarse"], thr=thr)).eval()(f0.to(dev), f1.to(dev), data, m0.flatten(-2), m1.flatten(-2))
    for k in ("b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c"):
        assert np.array_equal(data[k].cpu().numpy(), fx[k]), k
    np.testing.assert_allclose(data["mconf"].cpu().numpy(), fx["mconf"], rtol=1e-4, atol=1e-7)
    conf = data["conf_matrix"]
    assert not bool(conf.isnan().any())
    np.testing.assert_allclose(conf.max(2)[0].cpu().numpy(), fx["conf_row_top2"][..., 0], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(conf.max(1)[0].cpu().numpy(), fx["conf_col_top2"][:, 0], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_masked_coarse_fixture(dev, golden_dir, precision):
    """coarse_masked: both sides padded, an extent <= 2 * border, a fully padded image; both contraction routes."""
    from pope_amd import synth
    from pope_amd.matcher import dense_match
    fx = np.load(os.path.join(golden_dir, "coarse_masked.npz"))
    f0, f1, m0, m1, s0, s1, thr = synth.masked_coarse_case()
    assert np.allclose([float(f0.double().sum()), float(f1.double().sum())], fx["feat_digest"], rtol=0, atol=1e-6)
    h, w = m0.shape[1:]
    L = h * w
    out = dense_match(f0.to(dev), f1.to(dev), (h, w), (h, w), (8 * h, 8 * w), thr=thr, precision=precision,
                      mask0=m0.to(dev).flatten(-2), mask1=m1.to(dev).flatten(-2), border_mask0=m0.to(dev), border_mask1=m1.to(dev),
                      scale0=s0.to(dev), scale1=s1.to(dev))
    for k in ("b_ids", "i_ids", "j_ids"):
        assert np.array_equal(out[k].cpu().numpy(), fx[k]), k
    assert out["counts"].tolist()[1:] == [0, 0]
    for k in ("mkpts0_c", "mkpts1_c"):
        assert np.array_equal(out[k].cpu().numpy(), fx[k]), k
    conf = out["conf_matrix"].cpu()
    assert not bool(conf.isnan().any())
    np.testing.assert_allclose(conf.numpy(), fx["conf_matrix"], rtol=1e-4, atol=1e-7)
    valid = m0.flatten(1)[:, :, None] & m1.flatten(1)[:, None, :]
    row_any, col_any = valid.any(2, keepdim=True), valid.any(1, keepdim=True)
    uniform, zero = ~valid & ~row_any & ~col_any, ~valid & (row_any | col_any)
    both = ~m0.flatten(1)[:, :, None] & ~m1.flatten(1)[:, None, :]
    assert bool(both.any()) and bool((uniform | ~both).all())
    assert bool((conf[uniform] == torch.tensor(1.0 / L) * torch.tensor(1.0 / L)).all())   # padded x padded: 1 / (L S)
    assert bool((conf[zero] == 0).all())


def _transformer(dev):
    from pope_amd import synth
    from pope_amd.loftr import LocalFeatureTransformer
    from pope_amd.matcher import default_cfg
    t = LocalFeatureTransformer(default_cfg["coarse"])
    sd = synth.synthetic_matcher_state_dict(seed=0)
    t.load_state_dict({k[len("loftr_coarse."):]: v for k, v in sd.items() if k.startswith("loftr_coarse.")}, strict=True)
    return t.to(dev)


def test_masked_transformer_and_layer_against_the_reference(dev, golden_dir):
    from pope_amd import synth
    fx = np.load(os.path.join(golden_dir, "loftr_xfmr_masked.npz"))
    f0, f1, m0, m1 = synth.masked_xfmr_case()
    assert np.allclose([float(f0.double().sum()), float(f1.double().sum())], fx["feat_digest"], rtol=0, atol=1e-6)
    t = _transformer(dev)
    f0, f1, m0, m1 = f0.to(dev), f1.to(dev), m0.to(dev), m1.to(dev)
    o0, o1 = t(f0, f1, m0, m1)
    layer = t.layers[int(fx["layer_index"])]
    tap = int(fx["tap"])
    errs = {"out0": float(np.abs(o0[:, ::tap].cpu().numpy() - fx["out0"]).max()),
            "out1": float(np.abs(o1[:, ::tap].cpu().numpy() - fx["out1"]).max()),
            "layer_xmask": float(np.abs(layer(f0, f1, m0, None)[:, ::tap].cpu().numpy() - fx["layer_xmask"]).max()),
            "layer_smask": float(np.abs(layer(f0, f1, None, m1)[:, ::tap].cpu().numpy() - fx["layer_smask"]).max()),
            "layer_both": float(np.abs(layer(f0, f1, m0, m1)[:, ::tap].cpu().numpy() - fx["layer_both"]).max())}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= FEAT_ATOL, errs


def test_all_ones_masks_are_bit_identical_to_no_masks(dev):
    """Matcher (the drivers' f16x3 route), dense_match and one layer in both arithmetic routes."""
    from pope_amd.matcher import dense_match
    data, thr = case("loftr_masked_256", dev, keys=("image0", "image1"))
    m = build(thr, dev)
    ones = dict(data, mask0=torch.ones(2, 32, 32, dtype=torch.bool, device=dev), mask1=torch.ones(2, 32, 32, device=dev))
    m(data)
    m(ones)
    for k in ("conf_matrix", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f"):
        assert torch.equal(data[k], ones[k]), k
    g = torch.Generator().manual_seed(3)
    f0, f1 = torch.randn(2, 192, 256, generator=g).to(dev), torch.randn(2, 160, 256, generator=g).to(dev)
    o0, o1 = torch.ones(2, 192, device=dev), torch.ones(2, 160, device=dev)
    for prec in ("f16x3", "f32"):
        a = dense_match(f0, f1, (12, 16), (10, 16), (96, 128), thr=1e-3, precision=prec)
        b = dense_match(f0, f1, (12, 16), (10, 16), (96, 128), thr=1e-3, precision=prec, mask0=o0, mask1=o1,
                        border_mask0=o0.view(2, 12, 16), border_mask1=o1.view(2, 10, 16))
        for k in ("conf_matrix", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c"):
            assert torch.equal(a[k], b[k]), (prec, k)
    layer = _transformer(dev).layers[1]
    nbytes = __import__("pope_amd._lib", fromlist=["lib"]).lib().pope_loftr_layer_workspace_bytes(2, 192, 160, 256, 8)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for prec in ("f16x3", "f32"):
        x, y = f0.clone(), f0.clone()
        layer.update_(x, f1, ws, prec)
        layer.update_(y, f1, ws, prec, o0, o1)
        assert torch.equal(x, y), prec


def test_masked_matcher_is_batch_invariant(dev):
    data, thr = case("loftr_masked_256", dev)
    m = build(thr, dev)
    m(data)
    for k in range(2):
        one = {key: v[k:k + 1] for key, v in case("loftr_masked_256", dev)[0].items()}
        m(one)
        sel = data["b_ids"] == k
        assert torch.equal(one["conf_matrix"][0], data["conf_matrix"][k])
        assert torch.equal(one["i_ids"], data["i_ids"][sel]) and torch.equal(one["j_ids"], data["j_ids"][sel])
        for key in ("mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f"):
            assert torch.equal(one[key], data[key][sel]), (k, key)


def test_masked_range_guard_reruns_in_fp32_with_the_masks(dev):
    from pope_amd import _lib
    from pope_amd.matcher import dense_match
    layer = _transformer(dev).layers[0]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 128, 256, generator=g)
    x[0, 7, 3] = 2.0e4                          # |x| * 8 >= 65504
    x = x.to(dev)
    xm = torch.ones(2, 128, device=dev)
    xm[0, 100:] = 0
    xm[1, :20] = 0
    with pytest.warns(UserWarning, match="LoFTR encoder layer"):
        got = layer(x, x, xm, xm)
    ws = torch.empty(_lib.lib().pope_loftr_layer_workspace_bytes(2, 128, 128, 256, 8), dtype=torch.uint8, device=dev)
    want = x.clone()
    layer.update_(want, want, ws, "f32", xm, xm)
    assert torch.equal(got, want)
    f0, f1 = torch.randn(2, 96, 256, generator=g).to(dev) * 1e4, torch.randn(2, 96, 256, generator=g).to(dev) * 1e4
    mk = torch.ones(2, 8, 12, device=dev)
    mk[0, 6:] = 0
    kw = dict(thr=1e-3, mask0=mk.flatten(1), mask1=mk.flatten(1), border_mask0=mk, border_mask1=mk,
              scale0=torch.full((2, 2), 1.5, device=dev))
    with pytest.warns(UserWarning, match="dense_match"):
        a = dense_match(f0, f1, (8, 12), (8, 12), (64, 96), precision="f16x3", **kw)
    b = dense_match(f0, f1, (8, 12), (8, 12), (64, 96), precision="f32", **kw)
    for k in ("conf_matrix", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c"):
        assert torch.equal(a[k], b[k]), k


def test_masked_call_with_use_graph_runs_eagerly(dev):
    data, thr = case("loftr_masked_256", dev)
    e = build(thr, dev)
    e(data)
    g = build(thr, dev)
    g.use_graph = True
    for _ in range(3):
        d = case("loftr_masked_256", dev)[0]
        g(d)
        for k in ("conf_matrix", "b_ids", "i_ids", "j_ids", "mkpts0_c", "mkpts1_c", "mkpts1_f"):
            assert torch.equal(d[k], data[k]), k
    assert not g._graphs


def test_malformed_masks_and_scales_are_rejected(dev):
    from pope_amd.matcher import CoarseMatching, default_cfg
    data, thr = case("loftr_masked_256", dev)
    m = build(thr, dev)
    bad = [({"mask1": None}, KeyError),
           ({"mask0": data["mask0"][:, :16]}, ValueError),
           ({"mask0": data["mask0"].float() * 0.5}, ValueError),
           ({"mask1": data["mask1"].flatten(-2)}, ValueError),
           ({"scale0": data["scale0"][:, :1]}, ValueError),
           ({"scale1": torch.ones(3, 2, device=dev)}, ValueError)]
    for change, exc in bad:
        d = dict(data, **change)
        if change.get("mask1", 0) is None:
            d.pop("mask1")
        with pytest.raises(exc):
            m(d)
    cm = CoarseMatching(default_cfg["match_coarse"]).eval()
    f = torch.randn(1, 64, 256, device=dev)
    with pytest.raises(ValueError):
        cm(f, f, {"hw0_c": (8, 8), "hw1_c": (8, 8), "hw0_i": (64, 64)}, mask_c0=torch.ones(1, 64, device=dev))
