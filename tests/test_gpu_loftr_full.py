"""GPU: LoFTR with full (softmax) attention on the HIP kernels of pope_amd/csrc/loftr_attention.hip — the attention core
through its op-level entry (pope_loftr_full_attention_f32), layers and transformers against the reference fixture
(tests/golden/loftr_full.npz), and the `Matcher` with both transformers on full attention against loftr_full_128.npz.

"Exact" below is tests/loftr_full_checks.py evaluated in float64; e_ref is the error of the same restatement in float32 (the
reference's own arithmetic) on the same input; the bound on the HIP result is that of tests/test_gpu_loftr.py:
e_hip < 4 e_ref + 2e-5.  Shapes cover both routes (S <= 64: the small-sequence kernel, S > 64: flash tiles), both head widths
on both routes, query-block tails (L not a multiple of 128 / 32), key-tile tails (S not a multiple of 64) and S = 1."""
import copy
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import loftr_full_checks as K
from pope_amd import _lib, synth

pytestmark = pytest.mark.gpu

FEAT_ATOL = 1e-4
PX_ATOL = 5e-4
CLEAR = 1e-3


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def msd():
    return synth.synthetic_matcher_state_dict(seed=0)


@functools.lru_cache(maxsize=None)
def msd64():
    return {k: v.double() for k, v in msd().items()}


def cfg_with(coarse, fine, thr=None):
    from pope_amd.matcher import default_cfg
    cfg = copy.deepcopy(default_cfg)
    cfg["coarse"]["attention"], cfg["fine"]["attention"] = coarse, fine
    if thr is not None:
        cfg["match_coarse"]["thr"] = float(thr)
    return cfg


def hip_transformer(stage, dev, attention="full", layer_names=None):
    from pope_amd.loftr import LocalFeatureTransformer
    from pope_amd.matcher import default_cfg
    cfg = dict(default_cfg[stage], attention=attention)
    if layer_names is not None:
        cfg["layer_names"] = list(layer_names)
    t = LocalFeatureTransformer(cfg).eval()
    prefix = f"loftr_{stage}."
    keys = {k[len(prefix):]: v for k, v in msd().items() if k.startswith(prefix)}
    t.load_state_dict({k: v for k, v in keys.items() if int(k.split(".")[1]) < len(cfg["layer_names"])}, strict=True)
    return t.to(dev)


# ---- 1. the attention core ---------------------------------------------------------------------------------------------
CORE_SHAPES = [(1, 1, 1, 256), (1, 33, 64, 256), (3, 130, 65, 256), (2, 80, 200, 256), (37, 25, 25, 128), (1, 25, 25, 128),
               (2, 70, 130, 128), (2, 40, 25, 256)]


@functools.lru_cache(maxsize=None)
def core_case(n, L, S, Cd, ramp=False):
    """q, kv (fp32) with a score spread of ~9, the exact message (fp64) and the fp32 restatement's error."""
    g = torch.Generator().manual_seed(1000 * n + 10 * L + S + Cd)
    D = Cd // 8
    if ramp:   # scores rise with the key index: a_l * 31 s / (S - 1) (a uniform ramp of range 31 has std 9), every tile a new maximum
        u = torch.nn.functional.normalize(torch.randn(8, D, generator=g), dim=1)
        a = 0.8 + 0.4 * torch.rand(n, L, 1, 1, generator=g)
        q = (a * u * D ** 0.5).reshape(n, L, Cd)
        k = ((31.0 * torch.arange(S) / (S - 1)).view(1, S, 1, 1) * u).reshape(1, S, Cd).repeat(n, 1, 1)
    else:      # q, k ~ 3 randn: q . k / sqrt(D) has std 3 * 3
        q, k = 3.0 * torch.randn(n, L, Cd, generator=g), 3.0 * torch.randn(n, S, Cd, generator=g)
    v = torch.randn(n, S, Cd, generator=g)
    kv = torch.cat([k, v], 2).contiguous()
    h = lambda t: t.double().reshape(n, -1, 8, D)   # noqa: E731
    sc = K.scores(h(q), h(k))
    exact = K.attention_core(q.double(), kv.double())
    e_ref = float((K.attention_core(q, kv).double() - exact).abs().max())
    return q.contiguous(), kv, sc, exact, e_ref


def run_core(q, kv, precision, dev):
    n, L, Cd = q.shape
    qd, kvd = q.to(dev), kv.to(dev)
    out = torch.full((n, L, Cd), float("nan"), device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with _lib.on_device_of(qd):
        _lib.check(_lib.lib().pope_loftr_full_attention_f32(
            C.c_void_p(qd.data_ptr()), C.c_void_p(kvd.data_ptr()), n, L, kv.shape[1], Cd, 8, _lib.PRECISIONS[precision],
            C.c_void_p(out.data_ptr()), C.c_void_p(flag.data_ptr()), _lib.stream_of(dev)), "pope_loftr_full_attention_f32")
    return out.cpu(), int(flag.item())


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("n,L,S,Cd", CORE_SHAPES)
def test_attention_core_against_fp64(dev, n, L, S, Cd, precision):
    q, kv, sc, exact, e_ref = core_case(n, L, S, Cd)
    spread = float(sc.std()) if sc.numel() > 1 else 0.0
    if sc.numel() >= 1000:   # (fewer scores than that do not estimate a standard deviation; S = 1 has no softmax to speak of)
        assert 7.5 < spread < 10.5, spread
    got, bits = run_core(q, kv, precision, dev)
    e_hip = float((got.double() - exact).abs().max())
    print(f"core n={n} L={L} S={S} C={Cd} {precision}: score std {spread:.2f}; max err vs fp64: HIP {e_hip:.2e}, fp32 torch {e_ref:.2e}")
    assert bool(torch.isfinite(got).all()) and bits == 0
    assert e_hip < 4 * e_ref + 2e-5


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("n,L,S,Cd", [(2, 70, 200, 256), (1, 40, 150, 128)])
def test_attention_core_on_a_rising_ramp(dev, n, L, S, Cd, precision):
    """Keys ordered by rising score: every 64-key tile raises the running maximum of the online softmax."""
    q, kv, sc, exact, e_ref = core_case(n, L, S, Cd, True)
    tile_max = torch.stack([sc[:, :, t:t + 64].amax(2) for t in range(0, S, 64)], 0)   # [tiles, n, L, H]
    assert bool((tile_max[1:] > tile_max[:-1] + 0.5).all()) and 7.5 < float(sc.std()) < 10.5
    got, _ = run_core(q, kv, precision, dev)
    e_hip = float((got.double() - exact).abs().max())
    print(f"ramp n={n} L={L} S={S} C={Cd} {precision}: max err vs fp64: HIP {e_hip:.2e}, fp32 torch {e_ref:.2e}")
    assert bool(torch.isfinite(got).all())
    assert e_hip < 4 * e_ref + 2e-5


def test_attention_core_precisions_agree_bitwise_on_the_small_route(dev):
    """S <= 64 runs the same fp32 vector arithmetic under both precisions."""
    for shape in [(37, 25, 25, 128), (2, 40, 25, 256), (1, 33, 64, 256)]:
        q, kv = core_case(*shape)[:2]
        assert torch.equal(run_core(q, kv, "f32", dev)[0], run_core(q, kv, "f16x3", dev)[0]), shape


# ---- 2. layers and transformers of the reference fixture ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_case(name):
    case = synth.loftr_full_case(name)
    exact = K.run_case(msd64(), case)
    ref32 = K.run_case(msd(), case)
    return case, exact, ref32


@pytest.mark.parametrize("name", list(synth.LOFTR_FULL_CASES))
def test_layers_and_transformers_against_the_reference_fixture(dev, golden_dir, name):
    from pope_amd.loftr import LoFTREncoderLayer
    fx = np.load(os.path.join(golden_dir, "loftr_full.npz"))
    case, exact, ref32 = fixture_case(name)
    f0 = case["feat0"].to(dev)
    f1 = None if case["feat1"] is None else case["feat1"].to(dev)
    with torch.no_grad():
        if case["layer_names"] is None:
            layer = LoFTREncoderLayer(256, 8, "full").eval()
            lp = "loftr_coarse.layers.0."
            layer.load_state_dict({k[len(lp):]: v for k, v in msd().items() if k.startswith(lp)}, strict=True)
            got = (layer.to(dev)(f0, f0 if f1 is None else f1), None)
        else:
            got = hip_transformer(case["stage"], dev, "full", case["layer_names"])(f0, f1)
    for i, (g, w, r, tap) in enumerate(zip(got, exact, ref32, case["taps"])):
        if g is None:
            continue
        g = g.cpu()
        assert g.shape == w.shape and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        e_vs_ref = float(np.abs(synth.loftr_full_tap(g, tap).numpy() - fx[f"{name}.out{i}"]).max())
        e_hip, e_ref = float((g.double() - w).abs().max()), float((r.double() - w).abs().max())
        print(f"{name}.out{i}: HIP vs reference fixture {e_vs_ref:.2e}; max err vs fp64: HIP {e_hip:.2e}, fp32 torch {e_ref:.2e}; "
              f"|feat| max {float(w.abs().max()):.2f}")
        assert e_vs_ref <= FEAT_ATOL
        assert e_hip < 4 * e_ref + 2e-5


# ---- 3. determinism and batch invariance -------------------------------------------------------------------------------
@pytest.mark.parametrize("stage,n,L,S", [("coarse", 3, 320, 256), ("fine", 5, 25, 25)])
def test_full_transformer_is_deterministic_and_batch_invariant(dev, stage, n, L, S):
    t = hip_transformer(stage, dev)
    g = torch.Generator().manual_seed(4)
    f0, f1 = torch.randn(n, L, t.d_model, generator=g).to(dev), torch.randn(n, S, t.d_model, generator=g).to(dev)
    with torch.no_grad():
        a0, a1 = t(f0, f1)
        b0, b1 = t(f0, f1)
        c0, c1 = t(f0[1:2], f1[1:2])
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    assert torch.equal(a0[1:2], c0) and torch.equal(a1[1:2], c1)
    assert f0.data_ptr() != a0.data_ptr()


# ---- 4. range guard --------------------------------------------------------------------------------------------------
def test_full_transformer_range_guard_reruns_in_fp32(dev):
    t = hip_transformer("coarse", dev)
    g = torch.Generator().manual_seed(5)
    f0, f1 = torch.randn(1, 128, 256, generator=g), torch.randn(1, 128, 256, generator=g)
    f0[0, 7, 3] = 2.0e4                         # |x| * 8 >= 65504
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a0, a1 = t(f0.to(dev), f1.to(dev))
    ours = [w for w in rec if issubclass(w.category, UserWarning) and "LoFTR transformer" in str(w.message)]
    assert len(ours) == 1 and "re-running" in str(ours[0].message)
    c = t.config
    with torch.no_grad():
        r0, r1 = K.local_feature_transformer(msd64(), "loftr_coarse", f0.double(), f1.double(), c["layer_names"], c["nhead"])
    for a, r in ((a0, r0), (a1, r1)):
        assert bool(torch.isfinite(a).all())
        err = float((a.cpu().double() - r).abs().max()) / max(1.0, float(r.abs().max()))
        print(f"range guard re-run: relative err vs fp64 {err:.2e}")
        assert err < 1e-4, err


# ---- 5. the Matcher with both transformers on full attention -------------------------------------------------------------
def build_matcher(coarse, fine, thr, dev):
    from pope_amd.matcher import Matcher
    m = Matcher(cfg_with(coarse, fine, thr)).eval()
    m.load_state_dict(synth.synthetic_matcher_state_dict(seed=0), strict=True)
    return m.to(dev)


def clear_decisions(conf, thr, border, hw0, hw1):
    """tests/test_gpu_loftr.py:_clear_decisions: what the reference accepts with every margin > CLEAR ("must") and what an
    implementation within CLEAR of it may accept ("may")."""
    n, L, S = conf.shape
    m = torch.ones(n, hw0[0], hw0[1], hw1[0], hw1[1], dtype=torch.bool)
    bd = border
    m[:, :bd] = m[:, -bd:] = False
    m[:, :, :bd] = m[:, :, -bd:] = False
    m[:, :, :, :bd] = m[:, :, :, -bd:] = False
    m[:, :, :, :, :bd] = m[:, :, :, :, -bd:] = False
    inside = m.reshape(n, L, S)
    top2r, top2c = conf.topk(2, dim=2).values, conf.topk(2, dim=1).values
    rmax, rsec = top2r[..., 0:1], top2r[..., 1:2]
    cmax, csec = top2c[:, 0:1, :], top2c[:, 1:2, :]
    must = inside & (conf > thr + CLEAR) & (conf == rmax) & (conf == cmax) & (rmax - rsec > CLEAR) & (cmax - csec > CLEAR)
    may = inside & (conf > thr - CLEAR) & (conf >= rmax - CLEAR) & (conf >= cmax - CLEAR)
    return must, may


@pytest.mark.parametrize("name", ["pairs128", "96x128_vs_128x96"])
def test_matcher_with_full_attention_against_the_reference_fixture(dev, golden_dir, name):
    z = np.load(os.path.join(golden_dir, "loftr_full_128.npz"))
    fx = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}
    thr = float(fx["thr"])
    m = build_matcher("full", "full", thr, dev)
    i0, i1 = synth.loftr_full_matcher_case(name)
    data = {"image0": i0.to(dev), "image1": i1.to(dev)}
    assert m(data) is None
    f0, f1 = m({"image0": i0.to(dev), "image1": i1.to(dev)}, only_att_fea=True)
    assert tuple(data["hw0_c"]) == tuple(fx["hw0_c"]) and tuple(data["hw1_f"]) == tuple(fx["hw1_f"]) and data["W"] == 5
    errs = {"feat_c0": float(np.abs(f0[:, ::8].cpu().numpy() - fx["feat_c0"]).max()),
            "feat_c1": float(np.abs(f1[:, ::8].cpu().numpy() - fx["feat_c1"]).max()),
            "feat_c0_b0": float(np.abs(f0[0, ::2].cpu().numpy() - fx["feat_c0_b0"]).max()),
            "feat_c1_b0": float(np.abs(f1[0, ::2].cpu().numpy() - fx["feat_c1_b0"]).max())}
    print(name, "feature taps", {k: f"{v:.2e}" for k, v in errs.items()}, f"bound {FEAT_ATOL:g}")
    assert max(errs.values()) <= FEAT_ATOL, errs
    # the reference's confidence matrix: the restatement on this host, tied to the fixture by its match list
    with torch.no_grad():
        ref = K.matcher_forward(msd(), cfg_with("full", "full", thr), i0, i1)
    assert np.array_equal(ref["i_ids"].numpy(), fx["i_ids"]) and np.array_equal(ref["j_ids"].numpy(), fx["j_ids"])
    np.testing.assert_allclose(ref["conf_matrix"].max(2)[0].numpy(), fx["conf_rowmax"], rtol=1e-3, atol=1e-9)
    must, may = clear_decisions(ref["conf_matrix"], thr, 2, tuple(fx["hw0_c"]), tuple(fx["hw1_c"]))
    got_ids = torch.stack([data["b_ids"], data["i_ids"], data["j_ids"]], 1).cpu()
    got_mask = torch.zeros_like(must)
    got_mask[got_ids[:, 0], got_ids[:, 1], got_ids[:, 2]] = True
    n_ref, n_must = len(fx["b_ids"]), int(must.sum())
    assert bool((got_mask | ~must).all()), "a clear reference match is missing"
    assert bool((may | ~got_mask).all()), "a match the reference clearly rejects was published"
    identical = len(got_ids) == n_ref and np.array_equal(got_ids[:, 0].numpy(), fx["b_ids"]) \
        and np.array_equal(got_ids[:, 1].numpy(), fx["i_ids"]) and np.array_equal(got_ids[:, 2].numpy(), fx["j_ids"])
    print(f"{name}: {n_ref} reference matches, {n_must} clear by {CLEAR:g}; published {len(got_ids)}; list identical: {identical}")
    assert n_ref > 10 and n_must > 0
    if n_must == n_ref:
        assert identical
    ref_pos = {(int(b), int(i), int(j)): k for k, (b, i, j) in enumerate(zip(fx["b_ids"], fx["i_ids"], fx["j_ids"]))}
    gi = [k for k, t in enumerate(map(tuple, got_ids.tolist())) if t in ref_pos]
    ri = [ref_pos[tuple(got_ids[k].tolist())] for k in gi]
    assert len(gi) >= n_must
    e_conf = float(np.abs(data["mconf"].cpu().numpy()[gi] - fx["mconf"][ri]).max())
    e_px = float(np.abs(data["mkpts1_f"].cpu().numpy()[gi] - fx["mkpts1_f"][ri]).max())
    print(f"{name}: mconf max err {e_conf:.2e}, mkpts1_f max err {e_px:.2e} px")
    assert e_conf <= 2e-4 and e_px <= PX_ATOL
    assert np.array_equal(data["mkpts0_f"].cpu().numpy()[gi], fx["mkpts0_f"][ri])


# ---- 6. mixed configuration ------------------------------------------------------------------------------------------
def test_mixed_config_is_the_composition_of_the_two_transformers(dev):
    """Coarse full + fine linear: the Matcher publishes, bit for bit, what the separately tested full coarse transformer and
    linear fine transformer give when composed by hand around the same stages."""
    thr = 1e-3
    mixed, full = build_matcher("full", "linear", thr, dev), build_matcher("full", "full", thr, dev)
    i0, i1 = (t.to(dev) for t in synth.loftr_full_matcher_case("pairs128"))
    data = {"image0": i0, "image1": i1}
    mixed(data)
    assert len(data["b_ids"]) > 10
    # coarse: the full-attention transformer (the Matcher of test 5)
    c0, c1 = full({"image0": i0, "image1": i1}, only_att_fea=True)
    m0, m1 = mixed({"image0": i0, "image1": i1}, only_att_fea=True)
    assert torch.equal(c0, m0) and torch.equal(c1, m1)
    # fine: a linear-attention transformer of its own on the windows of those features
    feats_c, feats_f = mixed.backbone(torch.cat([i0, i1], 0))
    ff0, ff1 = feats_f.split(i0.size(0))
    comp = {"bs": i0.size(0), "hw0_i": i0.shape[2:], "hw1_i": i1.shape[2:], "hw0_c": feats_c.shape[2:], "hw1_c": feats_c.shape[2:],
            "hw0_f": ff0.shape[2:], "hw1_f": ff1.shape[2:]}
    mixed.coarse_matching(c0, c1, comp)
    w0, w1 = mixed.fine_preprocess(ff0, ff1, c0, c1, comp)
    w0, w1 = hip_transformer("fine", dev, "linear")(w0, w1)
    mixed.fine_matching(w0, w1, comp)
    for k in ("b_ids", "i_ids", "j_ids", "mconf", "expec_f", "mkpts0_f", "mkpts1_f"):
        assert torch.equal(comp[k], data[k]), k
    # and the fine stage of the all-full Matcher differs: the config reaches the fine transformer
    d2 = {"image0": i0, "image1": i1}
    full(d2)
    assert torch.equal(d2["b_ids"], data["b_ids"]) and not torch.equal(d2["expec_f"], data["expec_f"])
