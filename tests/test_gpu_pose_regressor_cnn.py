"""GPU: the image pose head (pope_amd/pose_regressor_cnn.py; pose/model_cnn.py:Mkpts_Reg_Model) against the composition of the
reference's modules evaluated in fp64 (tests/golden/convnext.npz), with the bound of test_gpu_convnext.py: MARGIN x the fp32
reference's own error."""
import os

import numpy as np
import pytest
import torch

from pope_amd import convnextv2, pose_regressor_cnn, synth

pytestmark = pytest.mark.gpu
MARGIN = 4.0


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "convnext.npz"))


_cache = {}


def run_case(name, precision):
    key = (name, precision)
    if key not in _cache:
        case = synth.convnext_case(name)
        model = pose_regressor_cnn.Mkpts_Reg_Model(16, case["mode"], backbone=convnextv2.ConvNeXtV2(precision=precision, **case["cfg"]))
        model.load_state_dict(case["state_dict"], strict=True)
        model = model.cuda()
        i0, i1 = case["img0"].cuda(), case["img1"].cuda()
        B = i0.shape[0]
        k0, k1 = torch.rand(B, 16, 2, device="cuda"), torch.rand(B, 16, 2, device="cuda")
        t, R = model(k0, k1, i0, i1)
        torch.cuda.synchronize()
        _cache[key] = (model, i0, i1, k0, k1, t, R)
    return _cache[key]


@pytest.mark.parametrize("precision", ("f32", "f16x3"))
@pytest.mark.parametrize("name", list(synth.CONVNEXT_POSE_CASES))
def test_modes_against_fp64(gold, name, precision):
    *_, t, R = run_case(name, precision)
    assert t.shape == (2, 3) and R.shape == (2, 3, 3)
    rt = float((t.cpu().double() - torch.from_numpy(gold[f"{name}.t64"])).abs().max()) / float(gold[f"{name}.e32_t"])
    rR = float((R.cpu().double() - torch.from_numpy(gold[f"{name}.R64"])).abs().max()) / float(gold[f"{name}.e32_R"])
    print(f"{name} {precision}: pred_trans {rt:.2f} x e32, pred_rot {rR:.2f} x e32")
    assert rt <= MARGIN and rR <= MARGIN, (rt, rR)
    if name != "pose_matrix":        # quat / 6d give a rotation
        eye = torch.eye(3, dtype=torch.float64).expand(2, 3, 3)
        assert float((R.cpu().double() @ R.cpu().double().transpose(1, 2) - eye).abs().max()) < 1e-5


@pytest.mark.parametrize("precision", ("f32", "f16x3"))
def test_key_points_are_ignored_and_pairs_are_independent(precision):
    model, i0, i1, k0, k1, t, R = run_case("pose_6d", precision)
    t2, R2 = model(None, None, i0, i1)
    assert torch.equal(t2, t) and torch.equal(R2, R)
    t3, R3 = model(k1 * 100, k0[:, :3], i0, i1)
    assert torch.equal(t3, t) and torch.equal(R3, R)
    for b in range(i0.shape[0]):
        tb, Rb = model(None, None, i0[b:b + 1], i1[b:b + 1])
        assert torch.equal(tb[0], t[b]) and torch.equal(Rb[0], R[b]), b
    with pytest.raises(ValueError):
        model(None, None, i0, i1[:, :, :, :40])
    with pytest.raises(ValueError, match="multiples of 32"):
        model(None, None, i0[:, :, :90], i1[:, :, :90])
