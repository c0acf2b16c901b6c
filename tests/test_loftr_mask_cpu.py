"""CPU: the C-ABI entry points of padded batches and rescaling (the masks of pope_loftr_encoder_layer_f32, the mask and scale
fields of pope_dense_match_args, the scale1 of pope_fine_match_f32) reject invalid arguments before any HIP call; the
mask / scale validation of the Python layer; and sanity of the padded-batch fixtures (scripts/gen_golden_masked.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pope_amd import _lib

ERR_ARG = -1


def match_layout_bytes(n, L, S, C, f16x3, publish_conf, border_masks, sinkhorn=False):
    """The dense matcher's workspace as pope_hip.h's pieces add up (csrc/capi.hip MatchLayout), every piece rounded to 256 bytes."""
    al = lambda v: (v + 255) // 256 * 256   # noqa: E731
    nl, ns, ldp = al(n * L * 4), al(n * S * 4), (S + 3) // 4 * 4
    total = 7 * nl + 3 * ns + al(n * ((L + 31) // 32) * ldp * 4)              # row / column statistics, column-maximum parts
    if f16x3:   # row parts, two column parts, the two feature planes
        total += al(n * L * 2 * ((S + 127) // 128) * 8) + 2 * al(n * 4 * ((L + 127) // 128) * ldp * 4) + al(n * L * C * 4) + al(n * S * C * 4)
    total += 0 if publish_conf else al(n * L * S * 4)
    total += al(n * 16) if border_masks else 0
    total += al(n * (L + 1) * 4) + al(n * (S + 1) * 4) + ns if sinkhorn else 0
    return total


def test_masked_entry_points_reject_invalid_arguments(hip_lib):
    w = _lib.LoftrLayerWeights()
    p = _fake_ptr()
    # layer: null weights / tensors, n <= 0
    assert hip_lib.pope_loftr_encoder_layer_f32(None, p, p, None, None, 1, 4, 4, 256, 8, 1e-5, 0, 1, p, 1 << 20, None, None) == ERR_ARG
    assert hip_lib.pope_loftr_encoder_layer_f32(w, None, p, p, p, 1, 4, 4, 256, 8, 1e-5, 0, 1, p, 1 << 20, None, None) == ERR_ARG
    assert hip_lib.pope_loftr_encoder_layer_f32(w, p, p, p, p, 0, 4, 4, 256, 8, 1e-5, 0, 1, p, 1 << 20, None, None) == ERR_ARG
    # dense match: n <= 0, null outputs
    def args(n, feat, out, border=p):
        v = lambda t: t.value if t is not None else None   # noqa: E731
        return _lib.DenseMatchArgs(
            feat0=v(feat), stride0=1024, feat1=v(feat), stride1=1024, n=n, L=4, S=4, C=256, h0=2, w0=2, h1=2, w1=2, thr=0.2, border_rm=2,
            temperature=0.1, scale=8.0, fill_mask0=v(p), fill_mask1=v(p), border_mask0=v(border), border_mask1=v(border), scale0=v(p),
            scale1=v(p), conf_matrix=v(p), b_ids=v(out), i_ids=v(out), j_ids=v(out), mconf=v(out), mkpts0_c=v(out), mkpts1_c=v(out),
            counts=v(out), workspace=v(p), workspace_bytes=1 << 20, precision=1)

    def dm(n, feat, out):
        return hip_lib.pope_dense_match_f32(ctypes.byref(args(n, feat, out)), None)
    assert dm(1, None, p) == ERR_ARG
    assert dm(0, p, p) == ERR_ARG
    assert dm(1, p, None) == ERR_ARG
    query = lambda a: hip_lib.pope_dense_match_workspace_bytes(ctypes.byref(a))   # noqa: E731
    assert query(args(0, p, p)) == 0
    # the border masks cost the pair extents, and nothing else: both sizes are what the layout formula gives
    assert query(args(2, p, p)) > query(args(2, p, p, border=None)) == match_layout_bytes(2, 4, 4, 256, True, True, False)
    assert query(args(2, p, p)) == match_layout_bytes(2, 4, 4, 256, True, True, True)
    # fine match: M <= 0, scale1 without b_ids, null windows
    assert hip_lib.pope_fine_match_f32(p, p, 0, 5, 128, p, 2.0, p, p, p, p, None) == ERR_ARG
    assert hip_lib.pope_fine_match_f32(p, p, 4, 5, 128, p, 2.0, p, None, p, p, None) == ERR_ARG
    assert hip_lib.pope_fine_match_f32(None, p, 4, 5, 128, p, 2.0, p, p, p, p, None) == ERR_ARG


def _fake_ptr():
    """A non-null pointer the calls above never dereference (every one of them fails argument validation first)."""
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
