"""No GPU: the surface of the LoFTR backbone's precision="f16" mode — the pope_conv_layer_f16 entry and its argument contract, the
Python switch, and the emulation that test_gpu_loftr_f16.py measures the mode against."""
import copy
import ctypes
import os
import re

import pytest
import torch

import conv_checks as K
import loftr_f16_checks as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_prototyped():
    from pope_amd import _lib
    header = open(os.path.join(ROOT, "include", "pope_hip.h")).read()
    assert re.search(r"int\s+pope_conv_layer_f16\s*\(\s*const\s+pope_conv_layer_args\s*\*[^)]*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert "pope_conv_layer_f16" in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["pope_conv_layer_f16"] == _lib.PROTOTYPES["pope_conv_layer_f32"]
    assert _lib.PRECISIONS["f16"] == K.F16


def _args(**kw):
    from pope_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    # CONV3 on [2, 6 + 2, 8 + 2] pixels of two 64-column chunks -> 128 channels as f16 rows (pitch 64 column pairs)
    base = dict(form=K.CONV3, precision=K.F16, n=2, H=6, W=8, cch=2, taps=0, a=p, a_rows=2 * 8 * 10, w=p, bias=p, N=128, ldc=64,
                slope=0.0, out_planes=p, out_f32=None, zero_border=1, res=None, ldres=0, up_src=None, up_lds=0, scratch=None,
                scratch_bytes=0, range_flag=None)
    base.update(kw)
    a = _lib.ConvLayerArgs(**base)
    a._keep = buf
    return a, p


def test_f16_entry_argument_validation_without_gpu(hip_lib):
    """Every rejection of pope_conv_layer_f16's contract comes back before the stream's device is touched (this machine has
    none); the pointers are never dereferenced.  A call inside the contract cannot be made here: it would launch."""
    _, p = _args()
    big = 1 << 40
    s2 = dict(form=K.CONV_S2, taps=9, scratch=p, scratch_bytes=big)
    up = dict(form=K.CONV1_UP, up_src=p, up_lds=128)
    stem = dict(form=K.STEM, cch=0, a_rows=0, scratch=p, scratch_bytes=big)
    f32o = dict(out_planes=None, out_f32=p, zero_border=0, ldc=128)
    bad = {
        "precision f16x3": dict(precision=K.F16X3), "precision f32": dict(precision=K.F32), "precision 3": dict(precision=3),
        "form 4": dict(form=4), "form -1": dict(form=-1),
        "n=0": dict(n=0), "H=0": dict(H=0), "W=-2": dict(W=-2),
        "N=0": dict(N=0, ldc=0), "N=130": dict(N=130, ldc=96), "N=260": dict(N=260, ldc=160),
        "cch=0": dict(cch=0), "CONV3 with taps": dict(taps=9),
        "CONV_S2 taps 3": dict(s2, taps=3), "CONV_S2 taps 1 cch 1": dict(s2, taps=1, cch=1), "CONV1_UP cch 1": dict(up, cch=1),
        "STEM with cch": dict(stem, cch=2), "STEM with taps": dict(stem, taps=9),
        "CONV_S2 odd H": dict(s2, H=7, a_rows=2 * 9 * 10), "CONV1_UP odd W": dict(up, W=1, a_rows=2 * 8 * 3), "STEM odd W": dict(stem, W=9),
        "null a": dict(a=None), "null w": dict(w=None), "misaligned a": dict(a=p + 4), "misaligned w": dict(w=p + 8),
        "misaligned bias": dict(bias=p + 4), "misaligned out": dict(out_planes=p + 2), "misaligned fp32 out": dict(f32o, out_f32=p + 4),
        "a one row short": dict(a_rows=2 * 8 * 10 - 1), "a_rows of the interior only": dict(a_rows=2 * 6 * 8),
        "no output": dict(out_planes=None), "both outputs": dict(out_f32=p),
        "f16 pitch in columns": dict(ldc=128), "f16 pitch 98 for N 196": dict(N=196, ldc=98), "f16 pitch 112 for N 196": dict(N=196, ldc=112),
        "f16 rows without the border pass": dict(zero_border=0), "CONV1_UP without the border pass": dict(up, zero_border=0),
        "STEM without the border pass": dict(stem, zero_border=0),
        "fp32 ldc below N": dict(f32o, ldc=124), "fp32 ldc 130": dict(f32o, ldc=130),
        "CONV_S2 to fp32": dict(s2, **f32o), "CONV1_UP to fp32": dict(up, **f32o), "STEM to fp32": dict(stem, **f32o),
        "res below N": dict(res=p, ldres=32), "res pitch 80": dict(res=p, ldres=80), "res misaligned": dict(res=p + 4, ldres=64),
        "res with CONV_S2": dict(s2, res=p, ldres=64), "res with CONV1_UP": dict(up, res=p, ldres=64), "res with STEM": dict(stem, res=p, ldres=64),
        "CONV1_UP without up_src": dict(up, up_src=None), "up_lds below N": dict(up, up_lds=124), "up_lds 130": dict(up, up_lds=130),
        "up_src misaligned": dict(up, up_src=p + 4), "up_src with CONV3": dict(up_src=p, up_lds=128),
        "CONV_S2 without scratch": dict(s2, scratch=None), "STEM without scratch": dict(stem, scratch=None),
        "scratch misaligned": dict(s2, scratch=p + 4),
        "operand of 4 GiB": dict(n=1, H=4094, W=2046, a_rows=4096 * 2048, cch=4),
    }
    for what, kw in bad.items():
        a, _ = _args(**kw)
        assert hip_lib.pope_conv_layer_f16(ctypes.byref(a), None) == -1, what
    short = {"CONV_S2 scratch one byte short": dict(s2, scratch_bytes=2 * 5 * 6 * 9 * 2 * 128 - 1),
             "STEM scratch one byte short": dict(stem, scratch_bytes=2 * 5 * 6 * 256 - 1)}
    for what, kw in short.items():
        a, _ = _args(**kw)
        assert hip_lib.pope_conv_layer_f16(ctypes.byref(a), None) == -3, what      # POPE_ERR_WORKSPACE
    assert hip_lib.pope_conv_layer_f16(None, None) == -1
    assert hip_lib.pope_abi_version() == 10


def test_precision_attribute_and_config():
    from pope_amd.loftr import ResNetFPN_8_2, build_backbone
    from pope_amd.matcher import Matcher, default_cfg
    before = copy.deepcopy(default_cfg)
    bb = build_backbone(default_cfg)
    assert bb.precision == "f16x3"
    bb.precision = "f16"
    assert bb.precision == "f16"
    for value in ("bf16", "f32", "F16", None, 16):
        with pytest.raises(ValueError, match="precision"):
            bb.precision = value
    assert bb.precision == "f16"
    cfg = copy.deepcopy(default_cfg)
    cfg["resnetfpn"]["precision"] = "f16"
    assert Matcher(cfg).backbone.precision == "f16"
    cfg["resnetfpn"]["precision"] = "bf16"
    with pytest.raises(ValueError, match="precision"):
        ResNetFPN_8_2(cfg["resnetfpn"])
    assert default_cfg == before and "precision" not in default_cfg["resnetfpn"]
    assert Matcher(default_cfg).backbone.precision == "f16x3"


def test_f16_weight_matrices():
    """_matrices(chunk=64): the filters over 64-column chunks — 196 input channels pad to 256 per tap, the stem to 128 columns —
    with zeros in the padding, and the same values as the 32-column form."""
    from pope_amd.loftr import build_backbone
    from pope_amd.matcher import default_cfg
    torch.manual_seed(3)
    bb = build_backbone(default_cfg).eval()
    m32, b32 = bb._matrices()
    m64, b64 = bb._matrices(chunk=64)
    assert [tuple(m.shape) for m in m64] == [(128, 128)] + [(128, 9 * 128)] * 4 + [(196, 9 * 128), (196, 9 * 256), (196, 128)] + \
        [(196, 9 * 256)] * 2 + [(256, 9 * 256), (256, 9 * 256), (256, 256)] + [(256, 9 * 256)] * 2 + \
        [(256, 256), (256, 256), (256, 9 * 256), (196, 9 * 256), (196, 128), (196, 9 * 256), (128, 9 * 256)]
    assert torch.equal(m64[0][:, :49], m32[0][:, :49]) and not bool(m64[0][:, 49:].any())
    a, b = m32[8].reshape(196, 9, 224), m64[8].reshape(196, 9, 256)      # layer2.1.conv1: 196 -> 196
    assert torch.equal(a[:, :, :196], b[:, :, :196]) and not bool(b[:, :, 196:].any())
    assert all((x is None) == (y is None) and (x is None or torch.equal(x, y)) for x, y in zip(b32, b64))


@pytest.mark.parametrize("n,H,W", [(2, 16, 24), (1, 32, 40)])
def test_emulation_without_rounding_is_the_fp64_network(n, H, W):
    """backbone_emul(rounding=False) — folded BatchNorm, the block and FPN wiring, the bilinear x2 — against the oracle's fp64
    ResNet-FPN (separate conv2d and BatchNorm, the reference's op order): fp64 round-off only.  With rounding it moves, by about
    the f16 step, and stays finite: the roundings are really applied."""
    from oracle import loftr_ref
    from pope_amd import synth
    msd = synth.synthetic_matcher_state_dict(seed=0)
    sd64 = {k: v.double() for k, v in msd.items()}
    bsd = {k[len("backbone."):]: v for k, v in msd.items() if k.startswith("backbone.")}
    x = synth.synthetic_gray_pairs(n, H, W, seed=n + H)[0]
    with torch.no_grad():
        wc, wf = loftr_ref.resnet_fpn_8_2(sd64, x.double())
        ec, ef, ev = E.backbone_emul(bsd, x, rounding=False)
        rc, rf, rv = E.backbone_emul(bsd, x, rounding=True)
    assert not ev and not rv
    for want, plain, rounded in ((wc, ec, rc), (wf, ef, rf)):
        scale = float(want.abs().max())
        assert plain.shape == want.shape and E.errors(plain, want)[0] <= 1e-11 * max(1.0, scale)
        e_max, e_rms = E.errors(rounded, want)
        assert 1e-6 * scale < e_max < 2e-2 * max(1.0, scale) and e_rms > 0 and bool(torch.isfinite(rounded).all())


def test_emulation_reports_a_range_event():
    from pope_amd import synth
    msd = synth.synthetic_matcher_state_dict(seed=0)
    bsd = {k[len("backbone."):]: v for k, v in msd.items() if k.startswith("backbone.")}
    x = synth.synthetic_gray_pairs(1, 16, 24, seed=1)[0]
    x[0, 0, 5, 5] = 9000.0
    with torch.no_grad():
        assert E.backbone_emul(bsd, x)[2]
