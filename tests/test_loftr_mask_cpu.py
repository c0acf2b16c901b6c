"""CPU: the C-ABI entry points of padded batches and rescaling (pope_loftr_encoder_layer_masked_f32,
pope_dense_match_masked_f32, pope_fine_match_scaled_f32) exist and reject invalid arguments before any HIP call; the
mask / scale validation of the Python layer; and sanity of the padded-batch fixtures (scripts/gen_golden_masked.py)."""
import os

import numpy as np
import pytest
import torch

from pope_amd import _lib

ERR_ARG = -1


def test_masked_entry_points_reject_invalid_arguments(hip_lib):
    for name in ("pope_loftr_encoder_layer_masked_f32", "pope_dense_match_masked_f32", "pope_dense_match_masked_workspace_bytes",
                 "pope_fine_match_scaled_f32"):
        assert hasattr(hip_lib, name), name
    w = _lib.LoftrLayerWeights()
    p = _fake_ptr()
    # layer: null weights / tensors, n <= 0
    assert hip_lib.pope_loftr_encoder_layer_masked_f32(None, p, p, None, None, 1, 4, 4, 256, 8, 1e-5, 1, p, 1 << 20, None, None) == ERR_ARG
    assert hip_lib.pope_loftr_encoder_layer_masked_f32(w, None, p, p, p, 1, 4, 4, 256, 8, 1e-5, 1, p, 1 << 20, None, None) == ERR_ARG
    assert hip_lib.pope_loftr_encoder_layer_masked_f32(w, p, p, p, p, 0, 4, 4, 256, 8, 1e-5, 1, p, 1 << 20, None, None) == ERR_ARG
    # dense match: n <= 0, null outputs
    def dm(n, feat, out):
        return hip_lib.pope_dense_match_masked_f32(feat, 1024, feat, 1024, n, 4, 4, 256, 2, 2, 2, 2, 0.2, 2, 0.1, 8.0,
                                                   p, p, p, p, p, p, p, out, out, out, out, out, out, out, p, 1 << 20, 1, None, None)
    assert dm(1, None, p) == ERR_ARG
    assert dm(0, p, p) == ERR_ARG
    assert dm(1, p, None) == ERR_ARG
    assert hip_lib.pope_dense_match_masked_workspace_bytes(0, 4, 4, 256, 1, 1, 1) == 0
    assert hip_lib.pope_dense_match_masked_workspace_bytes(2, 4, 4, 256, 1, 1, 1) > hip_lib.pope_dense_match_masked_workspace_bytes(
        2, 4, 4, 256, 1, 1, 0) == hip_lib.pope_dense_match_workspace_bytes_prec(2, 4, 4, 256, 1, 1)
    # fine match: M <= 0, scale1 without b_ids, null windows
    assert hip_lib.pope_fine_match_scaled_f32(p, p, 0, 5, 128, p, 2.0, p, p, p, p, None) == ERR_ARG
    assert hip_lib.pope_fine_match_scaled_f32(p, p, 4, 5, 128, p, 2.0, p, None, p, p, None) == ERR_ARG
    assert hip_lib.pope_fine_match_scaled_f32(None, p, 4, 5, 128, p, 2.0, p, p, p, p, None) == ERR_ARG


def _fake_ptr():
    """A non-null pointer the calls above never dereference (every one of them fails argument validation first)."""
    import ctypes
    return ctypes.c_void_p(16)


def test_mask_and_scale_validation():
    m = torch.ones(2, 4, 5, dtype=torch.bool)
    out = _lib.padding_mask(m, (2, 4, 5), "cpu", "m")
    assert out.dtype == torch.float32 and out.is_contiguous() and bool((out == 1).all())
    assert torch.equal(_lib.padding_mask(torch.tensor([[0, 1, 1]]), (1, 3), "cpu", "m"), torch.tensor([[0.0, 1.0, 1.0]]))
    assert _lib.padding_mask(None, (1, 3), "cpu", "m") is None
    with pytest.raises(ValueError):
        _lib.padding_mask(m, (2, 20), "cpu", "m")
    with pytest.raises(ValueError):
        _lib.padding_mask(torch.full((1, 3), 0.5), (1, 3), "cpu", "m")
    with pytest.raises(ValueError):
        _lib.padding_mask(torch.tensor([[2, 1, 0]]), (1, 3), "cpu", "m")
    assert _lib.pair_scale(torch.tensor([[1, 2]]), 1, "cpu", "s").dtype == torch.float32
    with pytest.raises(ValueError):
        _lib.pair_scale(torch.ones(2, 3), 2, "cpu", "s")
    with pytest.raises(ValueError):
        _lib.pair_scale(torch.ones(3, 2), 2, "cpu", "s")


def _padded_limit(e, b, n):
    s = e - b
    if s < 0:
        s += n
    return max(s, 0)


def _inside(m, idx, border=2):
    H, W = m.shape
    y, x = divmod(int(idx), W)
    eh, ew = int(m.sum(0).max()), int(m.sum(1).max())
    return border <= y < _padded_limit(eh, border, H) and border <= x < _padded_limit(ew, border, W)


@pytest.mark.parametrize("name", ["loftr_masked_256", "loftr_masked_192x256_vs_256x192", "coarse_masked", "coarse_masked_1024"])
def test_fixture_matches_obey_the_padded_border_rule(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    assert len(fx["b_ids"]) > 0
    for b, i, j in zip(fx["b_ids"], fx["i_ids"], fx["j_ids"]):
        assert _inside(fx["mask0"][b], i) and _inside(fx["mask1"][b], j), (b, i, j)
        assert fx["mask0"][b].ravel()[i] and fx["mask1"][b].ravel()[j]
    # coarse keypoints are (x, y) * 8 * scale of their pair, as fp32 (coarse_matching.py:243-250)
    for k, s, idx, key in ((0, "scale0", "i_ids", "mask0"), (1, "scale1", "j_ids", "mask1")):
        w = fx[key].shape[2]
        sc = (np.float32(8.0) * fx[s][fx["b_ids"]]).astype(np.float32)
        xy = np.stack([fx[idx] % w, fx[idx] // w], 1).astype(np.float32) * sc
        assert np.array_equal(xy, fx["mkpts%d_c" % k])


def test_fixture_pair1_matches_the_unmasked_fixture(golden_dir):
    """Pair 1 of loftr_masked_256 carries all-ones masks: its match list is pair 1 of loftr_256_lowthr (the floats agree to a
    few ulps only: the batch around it differs)."""
    fx = np.load(os.path.join(golden_dir, "loftr_masked_256.npz"))
    low = np.load(os.path.join(golden_dir, "loftr_256_lowthr.npz"))
    a, b = fx["b_ids"] == 1, low["b_ids"] == 1
    assert a.sum() == b.sum() > 0
    assert np.array_equal(fx["i_ids"][a], low["i_ids"][b]) and np.array_equal(fx["j_ids"][a], low["j_ids"][b])
    assert (fx["b_ids"] == 0).sum() > 0          # the padded pair still matches
