"""CPU: LoFTR layers with full (softmax) attention — the restatement the GPU tests measure against reproduces the reference
fixture (tests/golden/loftr_full.npz, scripts/gen_golden_loftr_full.py); the modules build with attention = 'full' and keep
the linear layer's parameters; masks are refused with NotImplementedError before any device check; the new C entry points
reject invalid arguments before any HIP call."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import loftr_full_checks as K
from pope_amd import _lib, synth
from pope_amd.loftr import LocalFeatureTransformer, LoFTREncoderLayer
from pope_amd.matcher import Matcher, default_cfg

ERR_ARG = -1


def cfg_with(coarse, fine):
    cfg = copy.deepcopy(default_cfg)
    cfg["coarse"]["attention"], cfg["fine"]["attention"] = coarse, fine
    return cfg


@pytest.mark.parametrize("name", list(synth.LOFTR_FULL_CASES))
def test_restatement_reproduces_the_reference_fixture(golden_dir, golden_threads, name):
    fx = np.load(os.path.join(golden_dir, "loftr_full.npz"))
    case = synth.loftr_full_case(name)
    outs = K.run_case(synth.synthetic_matcher_state_dict(0), case)
    for i, (o, tap) in enumerate(zip(outs, case["taps"])):
        if o is None:
            assert f"{name}.out{i}" not in fx.files
            continue
        want = fx[f"{name}.out{i}"]
        got = synth.loftr_full_tap(o, tap).numpy()
        assert got.shape == want.shape
        err = float(np.abs(got - want).max())
        print(f"{name}.out{i}: restatement vs fixture {err:.2e}")
        assert err <= 1e-5 and np.isfinite(want).all()


def test_full_and_linear_bodies_differ_on_the_fixture_case(golden_dir):
    """The fixture tells the two attention bodies apart by far more than the tests' bounds (1e-4)."""
    case = synth.loftr_full_case("layer_cross")
    sd = synth.synthetic_matcher_state_dict(0)
    with torch.no_grad():
        lin = K.encoder_layer(sd, "loftr_coarse.layers.0", case["feat0"], case["feat1"], attention="linear")
    full = np.load(os.path.join(golden_dir, "loftr_full.npz"))["layer_cross.out0"]
    assert float(np.abs(lin.numpy() - full).max()) > 0.05


def test_full_layer_has_the_linear_layers_state_dict():
    a, b = LoFTREncoderLayer(256, 8, "linear"), LoFTREncoderLayer(256, 8, "full")
    assert list(a.state_dict()) == list(b.state_dict())
    assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]
    sd = synth.synthetic_matcher_state_dict(0)
    m = Matcher(cfg_with("full", "full"))
    m.load_state_dict(dict(sd), strict=True)


@pytest.mark.parametrize("coarse,fine", [("full", "full"), ("full", "linear"), ("linear", "full")])
def test_full_attention_builds(coarse, fine):
    m = Matcher(cfg_with(coarse, fine))
    assert m.loftr_coarse.attention == coarse and m.loftr_fine.attention == fine
    assert all(l.attention == coarse for l in m.loftr_coarse.layers) and all(l.attention == fine for l in m.loftr_fine.layers)
    assert default_cfg["coarse"]["attention"] == default_cfg["fine"]["attention"] == "linear"


@pytest.mark.parametrize("bad", ["softmax", "Full", "", None])
def test_unknown_attention_raises_value_error(bad):
    with pytest.raises(ValueError, match="attention"):
        LoFTREncoderLayer(256, 8, bad)
    with pytest.raises(ValueError, match="attention"):
        LocalFeatureTransformer(dict(default_cfg["fine"], attention=bad))


def test_every_mask_entry_point_refuses_full_attention_on_cpu_tensors():
    x, s = torch.zeros(1, 6, 256), torch.zeros(1, 4, 256)
    mx, ms = torch.ones(1, 6, dtype=torch.bool), torch.ones(1, 4, dtype=torch.bool)
    layer = LoFTREncoderLayer(256, 8, "full").eval()
    t = LocalFeatureTransformer(dict(default_cfg["coarse"], attention="full")).eval()
    m = Matcher(cfg_with("full", "linear")).eval()
    im = torch.zeros(1, 1, 16, 16)
    mc = torch.ones(1, 2, 2, dtype=torch.bool)
    calls = [lambda: layer(x, s, x_mask=mx), lambda: layer(x, s, source_mask=ms), lambda: layer(x, s, mx, ms),
             lambda: t(x, s, mask0=mx), lambda: t(x, s, mask1=ms), lambda: t(x, s, mx, ms),
             lambda: m({"image0": im, "image1": im, "mask0": mc, "mask1": mc})]
    for call in calls:
        with pytest.raises(NotImplementedError, match="padding masks are not supported with attention='full'"):
            call()
    # without masks the CPU tensors reach the device check; the linear modules still take masks as far as that check
    with pytest.raises(_lib.PopeHipError):
        layer(x, s)
    with pytest.raises(_lib.PopeHipError):
        LoFTREncoderLayer(256, 8, "linear").eval()(x, s, x_mask=mx)


def test_new_entry_points_reject_invalid_arguments(hip_lib):
    """No call below passes validation, so none reaches a HIP call (this host has no GPU)."""
    w = _lib.LoftrLayerWeights()
    p = ctypes.c_void_p(16)       # non-null, 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(20)     # not 16-byte aligned
    layer = hip_lib.pope_loftr_encoder_layer_f32
    FULL = _lib.LOFTR_ATTENTIONS["full"]

    def lay(w_=w, x=p, src=p, n=1, L=4, S=4, C=256, H=8, prec=1, ws=p, xm=None, sm=None, attn=FULL):
        return layer(w_, x, src, xm, sm, n, L, S, C, H, 1e-5, attn, prec, ws, 1 << 20, None, None)

    for bad in (dict(w_=None), dict(x=None), dict(src=None), dict(ws=None), dict(n=0), dict(L=0), dict(S=-1), dict(C=64), dict(C=192),
                dict(H=4), dict(prec=2), dict(prec=-1)):
        assert lay(**bad) == ERR_ARG, bad
    # full attention takes no padding masks (the Python layer raises NotImplementedError for them); an unknown attention kind
    for bad in (dict(xm=p), dict(sm=p), dict(xm=p, sm=p), dict(attn=2), dict(attn=-1)):
        assert lay(**bad) == ERR_ARG, bad
    core = hip_lib.pope_loftr_full_attention_f32

    def att(q=p, kv=p, n=1, L=4, S=4, C=128, H=8, prec=0, out=p):
        return core(q, kv, n, L, S, C, H, prec, out, None, None)

    for bad in (dict(q=None), dict(kv=None), dict(out=None), dict(q=odd), dict(n=0), dict(L=-3), dict(S=0), dict(C=512), dict(H=16),
                dict(prec=2), dict(prec=7)):
        assert att(**bad) == ERR_ARG, bad
    assert hip_lib.pope_abi_version() == 10
