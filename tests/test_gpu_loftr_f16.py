"""GPU: the LoFTR backbone's opt-in plain-f16 mode (ResNetFPN_8_2.precision = "f16") as a whole, and through every call path of
the Matcher.

Accuracy is measured against the arithmetic the mode promises, not against the code under test: per output map,
    got    precision="f16" on the GPU
    ref64  the oracle's fp64 ResNet-FPN (what test_gpu_loftr.py::test_hip_backbone_matches_oracle compares to)
    emul   loftr_f16_checks.backbone_emul on the CPU: the same network in fp64 with every layer input rounded to f16 at scale 8
           and every folded filter to f16 at scale 256
and required, in max-abs and in RMS:  err(got, ref64) <= 1.25 err(emul, ref64) + (1e-5 + 1e-5 max |ref64|).  The 25 % cover f16
roundings that fall the other way under fp32 accumulation-order noise; the additive term is the project's fp32 constant.
The call paths are held to equality: graph replay, encode_reference + indexed call, and the untouched default."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

import loftr_f16_checks as E
from test_gpu_reference_prompt import KEYS, assert_matches_exist, assert_same_outputs, both_indexed_calls, build_matcher, make_case, plain_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def msd():
    from pope_amd import synth
    return synth.synthetic_matcher_state_dict(seed=0)


@pytest.fixture(scope="module")
def peaked_sd(golden_dir):
    from pope_amd import synth
    fx = np.load(os.path.join(golden_dir, "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    return sd


def _bsd(msd):
    return {k[len("backbone."):]: v for k, v in msd.items() if k.startswith("backbone.")}


def _backbone(dev, msd, precision=None):
    from pope_amd.loftr import build_backbone
    from pope_amd.matcher import default_cfg
    b = build_backbone(default_cfg).eval()
    b.load_state_dict(_bsd(msd), strict=True)
    if precision is not None:
        b.precision = precision
    return b.to(dev)


@pytest.mark.parametrize("n,H,W", [(2, 16, 24), (3, 32, 40)])
def test_f16_backbone_against_its_emulation(dev, msd, n, H, W):
    from oracle import loftr_ref
    from pope_amd import synth
    x = synth.synthetic_gray_pairs(n, H, W, seed=n + H)[0]
    with torch.no_grad():
        ref64 = loftr_ref.resnet_fpn_8_2({k: v.double() for k, v in msd.items()}, x.double())
        ec, ef, event = E.backbone_emul(_bsd(msd), x)
        assert not event and bool(torch.isfinite(ec).all()) and bool(torch.isfinite(ef).all()), "the seed must keep the emulation in range"
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*range contract.*")     # a range event would re-run in fp32 and pass trivially
            got = _backbone(dev, msd, "f16")(x.to(dev))
    assert got[0].shape == (n, 256, H // 8, W // 8) and got[1].shape == (n, 128, H // 2, W // 2)
    for name, g, w, e in (("coarse", got[0], ref64[0], ec), ("fine", got[1], ref64[1], ef)):
        g_max, g_rms = E.errors(g.cpu(), w)
        e_max, e_rms = E.errors(e, w)
        slack = 1e-5 + 1e-5 * float(w.abs().max())
        print(f"measured: f16 backbone {name} n={n} {H}x{W}: max |err| {g_max:.3e} (emulation {e_max:.3e}), rms {g_rms:.3e} "
              f"(emulation {e_rms:.3e}), max |ref64| {float(w.abs().max()):.3f}")
        assert bool(torch.isfinite(g).all())
        assert g_max <= 1.25 * e_max + slack, (name, g_max, e_max)
        assert g_rms <= 1.25 * e_rms + slack, (name, g_rms, e_rms)


def _scaled_filter(msd):
    """The weights with layer1.0.conv1 scaled so that its largest folded entry is 200 (inside the weight range, |w| < 255.9): on
    an image of gain 8 the block's activations leave the f16 range at scale 8 and the range flag rises; with the filter as it was
    the same image raises nothing (both shown on the emulation first)."""
    sd = {k: v.clone() for k, v in msd.items()}
    w, g = sd["backbone.layer1.0.conv1.weight"], sd["backbone.layer1.0.bn1.weight"] * torch.rsqrt(sd["backbone.layer1.0.bn1.running_var"] + 1e-5)
    folded = (w * g.view(-1, 1, 1, 1)).abs().max()
    sd["backbone.layer1.0.conv1.weight"] = w * (200.0 / float(folded))
    return sd


def test_f16_overflow_policy(dev, msd):
    from pope_amd import synth
    from pope_amd._lib import PopeRangeError
    sd = _scaled_filter(msd)
    x = 8.0 * synth.synthetic_gray_pairs(2, 32, 40, seed=5)[0]
    with torch.no_grad():
        assert E.backbone_emul(_bsd(sd), x)[2] and not E.backbone_emul(_bsd(msd), x)[2]
    x = x.to(dev)
    b = _backbone(dev, sd, "f16")
    assert b._weights("f16") is not None
    with torch.no_grad():
        want = b._run(x, "f32")[0]
        with pytest.warns(UserWarning, match="LoFTR backbone"):
            got = b(x)
        assert all(torch.equal(g, w) for g, w in zip(got, want)) and all(bool(torch.isfinite(g).all()) for g in got)
        b.on_overflow = "raise"
        with pytest.raises(PopeRangeError):
            b(x)
        # a filter outside the weight range: the same policy before any launch
        sd2 = {k: v.clone() for k, v in msd.items()}
        sd2["backbone.layer1.0.conv1.weight"] = sd["backbone.layer1.0.conv1.weight"] * 4.0
        b2 = _backbone(dev, sd2, "f16")
        assert b2._weights("f16") is None
        assert all(torch.equal(g, w) for g, w in zip(b2(x), b2._run(x, "f32")[0]))
        b2.on_overflow = "raise"
        with pytest.raises(PopeRangeError):
            b2(x)


def _run(m, a, b, **extra):
    d = {"image0": a, "image1": b, **extra}
    m(d)
    return d


def test_default_is_untouched_and_f16_is_another_arithmetic(dev, peaked_sd):
    """A Matcher that never sets the attribute equals one set to "f16x3" bit for bit; "f16" gives other bits and still matches."""
    refs, crops, idx = make_case(dev, 2, (0, 1, 1), (128, 160), (128, 160), seed=11)
    i0 = refs.index_select(0, idx.to(dev))
    plain, x3, h = build_matcher(dev, peaked_sd), build_matcher(dev, peaked_sd), build_matcher(dev, peaked_sd)
    x3.backbone.precision = "f16x3"
    h.backbone.precision = "f16"
    want, same, half = _run(plain, i0, crops), _run(x3, i0, crops), _run(h, i0, crops)
    assert len(want["b_ids"]) > 0
    for k in KEYS:
        assert torch.equal(same[k], want[k]), k
    assert_matches_exist(half, idx, tag="precision f16")
    assert not torch.equal(half["conf_matrix"], want["conf_matrix"])
    assert not any(torch.equal(a, b) for a, b in zip(h.backbone(i0), plain.backbone(i0)))


def test_f16_graph_replay_equals_eager(dev, peaked_sd):
    refs, crops, idx = make_case(dev, 2, (0, 1, 1), (128, 160), (128, 160), seed=11)
    i0 = refs.index_select(0, idx.to(dev))
    m, e = build_matcher(dev, peaked_sd), build_matcher(dev, peaked_sd)
    m.backbone.precision = e.backbone.precision = "f16"
    m.use_graph = True
    want = _run(e, i0, crops)
    assert len(want["b_ids"]) > 0
    for call in range(4):      # eager, capture, replay, replay
        got = _run(m, i0, crops)
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (call, k)
    ents = [v for v in m._graphs.values() if "graph" in v]
    assert len(ents) == 1 and not ents[0].get("retired")
    # the graph belongs to the mode it was captured in
    m.backbone.precision = "f16x3"
    e.backbone.precision = "f16x3"
    want3 = _run(e, i0, crops)
    for call in range(3):
        got3 = _run(m, i0, crops)
        for k in KEYS:
            assert torch.equal(got3[k], want3[k]), ("f16x3 after f16", call, k)


def test_f16_reference_encoding_equals_the_repeated_image_call(dev, peaked_sd):
    """The shapes of test_gpu_reference_prompt.py::test_indexed_call_equals_the_repeated_image_call, with the backbone in "f16"."""
    m = build_matcher(dev, peaked_sd)
    m.backbone.precision = "f16"
    index = (1, 0, 1, 0, 0, 1)
    refs, crops, idx = make_case(dev, 2, index, (128, 160), (128, 160), seed=11)
    want = plain_call(m, refs, crops, idx)
    assert_matches_exist(want, idx, tag="f16, 128x160")
    a, b, ref = both_indexed_calls(m, refs, crops, idx)
    assert_same_outputs(a, want, "f16 / image0 + index")
    assert_same_outputs(b, want, "f16 / kept encoding")
    assert ref.mode == "f16" and "f16" in ref._bb and "f16x3" not in ref._bb
    # L != S: two launch sequences
    refs2, crops2, idx2 = make_case(dev, 2, (0, 1, 1, 0), (128, 160), (96, 96), seed=12)
    want2 = plain_call(m, refs2, crops2, idx2)
    a2, b2, _ = both_indexed_calls(m, refs2, crops2, idx2)
    assert_same_outputs(a2, want2, "f16 / 96x96 crops / image0 + index")
    assert_same_outputs(b2, want2, "f16 / 96x96 crops / kept encoding")
    # the encoding follows the switch: the next call reads it in the mode the backbone has then
    m.backbone.precision = "f16x3"
    want3 = plain_call(m, refs, crops, idx)
    got3 = {"reference": ref, "image0_index": idx, "image1": crops}
    m(got3)
    assert_same_outputs(got3, want3, "f16x3 on an encoding made in f16")
    assert ref.mode == "f16x3"


def test_f16_with_padding_masks_publishes_the_same_keys(dev):
    from pope_amd import synth
    from pope_amd.matcher import Matcher, default_cfg
    inp, thr = synth.masked_loftr_case("loftr_masked_256")
    cfg = copy.deepcopy(default_cfg)
    cfg["match_coarse"]["thr"] = float(thr)
    out = {}
    for mode in ("f16x3", "f16"):
        m = Matcher(cfg).eval()
        m.load_state_dict(synth.synthetic_matcher_state_dict(seed=0), strict=True)
        m = m.to(dev)
        m.backbone.precision = mode
        data = {k: inp[k].to(dev) for k in ("image0", "image1", "mask0", "mask1", "scale0", "scale1")}
        assert m(data) is None
        out[mode] = data
    assert sorted(out["f16"]) == sorted(out["f16x3"])
    for k in ("conf_matrix", "hw0_c", "hw1_c", "hw0_f", "hw1_f"):
        a, b = out["f16"][k], out["f16x3"][k]
        assert tuple(a.shape if isinstance(a, torch.Tensor) else a) == tuple(b.shape if isinstance(b, torch.Tensor) else b), k
    assert len(out["f16"]["b_ids"]) > 0 and bool(torch.isfinite(out["f16"]["conf_matrix"]).all())
    assert bool(torch.isfinite(out["f16"]["mkpts1_f"]).all())
