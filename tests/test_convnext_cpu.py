"""CPU: the host side of the ConvNeXtV2 backbone and the image pose head (pope_amd/convnextv2.py, pose_regressor_cnn.py) —
state-dict layouts against the reference's, the FCMAE checkpoint remapping, and argument checks that need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pope_amd import _lib, convnextv2, pose_regressor_cnn, synth


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "convnext.npz"))


def _layout(sd):
    return [(k, "x".join(str(d) for d in v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("factory", sorted(convnextv2.FACTORIES))
def test_factory_state_dict_is_the_reference_s(gold, factory):
    want = list(zip(gold[f"keys_{factory}.names"].tolist(), gold[f"keys_{factory}.shapes"].tolist()))
    with torch.device("meta"):
        model = convnextv2.FACTORIES[factory]()
    assert _layout(model.state_dict()) == want
    assert [(k, "x".join(str(d) for d in s)) for k, s in synth.convnext_keys(model.depths, model.dims, 1000)] == want
    assert any(k.endswith("grn.gamma") and s.startswith("1x1x1x") for k, s in want)


def test_pose_model_state_dict():
    with torch.device("meta"):
        large = pose_regressor_cnn.Mkpts_Reg_Model(8, "quat")
    keys = list(large.state_dict())
    with torch.device("meta"):
        trunk = list(convnextv2.convnextv2_large(num_classes=32).state_dict())
    assert keys == ["convnextv2.model." + k for k in trunk] + ["translation_head_rot.weight", "translation_head_rot.bias",
                                                                "rotation_head_rot.weight", "rotation_head_rot.bias"]
    assert tuple(large.state_dict()["rotation_head_rot.weight"].shape) == (4, 32)
    assert tuple(large.state_dict()["convnextv2.model.head.weight"].shape) == (32, 1536)
    for mode, width in synth.POSE_REGRESSOR_MODES.items():
        m = pose_regressor_cnn.Mkpts_Reg_Model(8, mode, backbone=convnextv2.ConvNeXtV2(**synth.CONVNEXT_SMALL))
        m.load_state_dict(synth.convnext_pose_state_dict(mode), strict=True)
        assert m.rotation_head_rot.out_features == width
    with pytest.raises(ValueError):
        pose_regressor_cnn.Mkpts_Reg_Model(8, "euler")
    with pytest.raises(ValueError):
        pose_regressor_cnn.Mkpts_Reg_Model(8, "6d", model_type="gigantic")


def test_remap_checkpoint_keys(gold):
    out = convnextv2.remap_checkpoint_keys(synth.fcmae_checkpoint())
    assert list(out) == gold["remap.names"].tolist()
    assert ["x".join(str(d) for d in v.shape) for v in out.values()] == gold["remap.shapes"].tolist()
    for (k, v), want in zip(out.items(), gold["remap.checksums"]):
        f = v.double().reshape(-1)
        got = float((f * torch.arange(1, f.numel() + 1, dtype=torch.float64)).sum())
        assert got == pytest.approx(float(want), rel=1e-12, abs=1e-12), k
    # the result loads into a module of the toy geometry's parameter names
    assert "stages.0.0.dwconv.weight" in out and tuple(out["stages.0.0.grn.gamma"].shape) == (1, 1, 1, 32)
    assert not any(k.startswith("encoder") or ".ln." in k or ".linear." in k or k.endswith("kernel") for k in out)


def test_inference_only_and_no_cpu_path():
    model = convnextv2.ConvNeXtV2(drop_path_rate=0.3, **synth.CONVNEXT_SMALL)     # accepted and unused
    assert not model.training and model.overflow_events == 0
    with pytest.raises(NotImplementedError):
        model.train()
    model.eval()
    with pytest.raises(_lib.PopeHipError):
        model(torch.zeros(1, 3, 32, 32))
    with pytest.raises(_lib.PopeHipError):
        model.forward_features(torch.zeros(1, 3, 32, 32))
    pose = pose_regressor_cnn.Mkpts_Reg_Model(4, "6d", backbone=model)
    with pytest.raises(NotImplementedError):
        pose.train()
    with pytest.raises(_lib.PopeHipError):
        pose(None, None, torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        convnextv2.ConvNeXtV2(precision="bf16")


def _fake_weights(ok, depths=(1, 1, 1, 1), dims=(64, 80, 160, 320)):
    """A weights struct whose every device pointer is the (never dereferenced) address `ok`; blocks_host is a real host array."""
    w = _lib.ConvNextWeights()
    w.depths[:], w.dims[:], w.num_classes = list(depths), list(dims), 32
    for name, kind in _lib.ConvNextWeights._fields_:
        if kind is ctypes.c_void_p:
            setattr(w, name, ok)
        elif kind is ctypes.c_void_p * 3:
            for i in range(3):
                getattr(w, name)[i] = ok
    blocks = (_lib.ConvNextBlockWeights * sum(depths))()
    for b in blocks:
        for name, _ in _lib.ConvNextBlockWeights._fields_:
            setattr(b, name, ok)
    w.blocks_host = ctypes.cast(blocks, ctypes.POINTER(_lib.ConvNextBlockWeights))
    return w, blocks


def test_c_entries_refuse_bad_arguments_without_a_gpu(hip_lib):
    assert hip_lib.pope_abi_version() == 10
    buf = ctypes.create_string_buffer(1024)
    ok = (ctypes.addressof(buf) + 255) & ~255
    w, keep = _fake_weights(ok)
    wp = ctypes.byref(w)
    fwd = hip_lib.pope_convnext_forward_f32
    need = hip_lib.pope_convnext_workspace_bytes(wp, 2, 96, 160)
    assert need > 2 * 24 * 40 * 64 * 4 * (3 + 4)

    def call(w_=wp, img=ok, B=2, H=96, W=160, prec=1, feats=ok, logits=ok, ws=ok, nbytes=None):
        return fwd(w_, img, B, H, W, prec, feats, logits, None, ws, need if nbytes is None else nbytes, None, None)

    # null pointers
    assert call(w_=None) == -1 and call(img=None) == -1 and call(ws=None) == -1
    # H or W not a multiple of 32, non-positive dims
    assert call(H=100) == -1 and call(W=176 - 8) == -1 and call(H=0) == -1 and call(W=-32) == -1 and call(B=0) == -1
    # a short workspace, an unaligned one, an unknown precision
    assert call(nbytes=need - 1) == -1 and call(ws=ok + 16) == -1 and call(prec=2) == -1 and call(prec=-1) == -1
    assert hip_lib.pope_convnext_workspace_bytes(wp, 2, 100, 160) == 0 and hip_lib.pope_convnext_workspace_bytes(None, 2, 96, 160) == 0
    # a null weight pointer, f16x3 without the planes of a K % 32 == 0 GEMM; widths that are no multiple of 8
    keep[2].pw2_wp = None
    assert call() == -1
    keep[2].pw2_wp = ok
    keep[1].pw1_wp = None              # C = 80: K % 32 != 0, its planes are never read
    w.norm_w = None
    assert call() == -1
    w.norm_w = ok
    bad, _k = _fake_weights(ok, dims=(60, 80, 160, 320))
    assert call(w_=ctypes.byref(bad)) == -1
    w.num_classes = 30                 # the head GEMM needs num_classes % 4 == 0; features alone do not
    assert call() == -1

    dw = hip_lib.pope_convnext_dwconv_f32
    assert dw(None, ok, ok, ok, 1, 3, 5, 80, None) == -1 and dw(ok, ok, ok, None, 1, 3, 5, 80, None) == -1
    assert dw(ok, ok, ok, ok, 1, 3, 5, 80, None) == -1          # in place
    assert dw(ok, ok, ok, ok + 256, 0, 3, 5, 80, None) == -1 and dw(ok, ok, ok, ok + 256, 1, 0, 5, 80, None) == -1
    assert dw(ok, ok, ok, ok + 256, 1, 3, 5, 0, None) == -1

    grn = hip_lib.pope_convnext_grn_f32
    gneed = hip_lib.pope_convnext_grn_workspace_bytes(2, 15, 320)
    assert gneed >= (2 * 320 + 2 * 320) * 4 and hip_lib.pope_convnext_grn_workspace_bytes(0, 15, 320) == 0
    assert grn(None, ok, ok, 2, 15, 320, ok, None, ok, gneed, None, None) == -1
    assert grn(ok, ok, ok, 2, 15, 320, None, None, ok, gneed, None, None) == -1      # neither output
    assert grn(ok, ok, ok, 2, 15, 320, ok, ok, ok, gneed, None, None) == -1          # both
    assert grn(ok, ok, ok, 2, 15, 300, ok, None, ok, gneed, None, None) == -1        # C % 32
    assert grn(ok, ok, ok, 2, 0, 320, ok, None, ok, gneed, None, None) == -1
    assert grn(ok, ok, ok, 2, 15, 320, ok, None, ok, gneed - 1, None, None) == -1    # short workspace
    assert grn(ok, ok, ok, 2, 15, 320, ok, None, None, gneed, None, None) == -1

    heads = hip_lib.pope_convnext_pose_heads_f32
    assert heads(None, ok, ok, ok, ok, 0, 1, 32, ok, ok, None) == -1 and heads(ok, ok, ok, ok, ok, 3, 1, 32, ok, ok, None) == -1
    assert heads(ok, ok, ok, ok, ok, 0, 0, 32, ok, ok, None) == -1 and heads(ok, ok, ok, ok, ok, 0, 1, 0, ok, ok, None) == -1
