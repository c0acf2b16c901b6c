"""CPU: the public surface of "encode the reference once, match many crops" — the argument checks of the Matcher's
`reference` / `image0_index` keys, the `ref0_of_pair` index of `pope_fine_preprocess_f32`, and the driver's `ReferenceSet` /
`ref_index` — everything that is decided before a launch.  What the calls compute is pinned on the card by
tests/test_gpu_reference_prompt.py."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from pope_amd import _lib


@pytest.fixture(scope="module")
def matcher():
    from pope_amd.matcher import Matcher, default_cfg
    return Matcher(default_cfg).eval()


def _gray(n, h=32, w=32):
    return torch.zeros(n, 1, h, w)


# ---- Matcher: data['image0_index'] ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("index, what", [
    ([0, 1, 2], "values"),                                   # 2 outside [0, 2)
    ([0, -1, 1], "values"),
    (torch.tensor([0, 1, 5]), "values"),
    ([0, 1], "one entry per pair"),                          # wrong length
    (torch.zeros(3, 1, dtype=torch.int64), "one entry per pair"),
    (torch.tensor([0.0, 1.0, 1.0]), "integers"),             # float dtype
    ([0.0, 1.0, 0.0], "integers"),
    (torch.tensor([True, False, True]), "integers"),
])
def test_image0_index_is_checked_before_the_device_check(matcher, index, what):
    data = {"image0": _gray(2), "image1": _gray(3), "image0_index": index}
    with pytest.raises(ValueError, match=what):      # CPU tensors: PopeHipError would mean the check came too late
        matcher(data)
    assert "bs" not in data and "hw0_i" not in data


def test_image0_index_helper_accepts_what_it_should():
    from pope_amd.matcher import _image0_index
    assert _image0_index(None, 3, 3).tolist() == [0, 1, 2] and _image0_index(None, 3, 3).dtype == torch.int64
    assert _image0_index([1, 0, 1], 3, 2).tolist() == [1, 0, 1]
    got = _image0_index(torch.tensor([1, 1], dtype=torch.int32), 2, 2)
    assert got.dtype == torch.int64 and got.tolist() == [1, 1] and got.device.type == "cpu"
    assert _image0_index(torch.empty(0, dtype=torch.int64), 0, 4).shape == (0,)
    with pytest.raises(ValueError, match="needs data\\['image0_index'\\]"):
        _image0_index(None, 3, 2)                    # R != n without an index


def test_reference_count_must_match_without_an_index(matcher):
    # reached through a key of the indexed call: an explicit None index with R = 2 references for n = 3 pairs
    with pytest.raises(ValueError, match="needs data\\['image0_index'\\]"):
        matcher({"image0": _gray(2), "image1": _gray(3), "image0_index": None})


def test_reference_together_with_image0_raises(matcher):
    from pope_amd.matcher import ReferenceEncoding
    ref = ReferenceEncoding.__new__(ReferenceEncoding)       # no stage may look at it
    with pytest.raises(ValueError, match="not both"):
        matcher({"reference": ref, "image0": _gray(1), "image1": _gray(1)})
    with pytest.raises(ValueError, match="needs data\\['image0'\\] or data\\['reference'\\]"):
        matcher({"image1": _gray(1), "image0_index": [0]})
    with pytest.raises(ValueError, match="ReferenceEncoding of this matcher"):
        matcher({"reference": "not an encoding", "image1": _gray(1)})


@pytest.mark.parametrize("keys", [("mask0", "mask1"), ("mask0",), ("mask1",)])
def test_masks_with_a_reference_are_refused_before_the_device_check(matcher, keys):
    from pope_amd.matcher import ReferenceEncoding
    masks = {k: torch.ones(2, 4, 4, dtype=torch.bool) for k in keys}
    with pytest.raises(NotImplementedError, match="padding masks"):
        matcher({"image0": _gray(1), "image1": _gray(2), "image0_index": [0, 0], **masks})
    with pytest.raises(NotImplementedError, match="padding masks"):
        matcher({"reference": ReferenceEncoding.__new__(ReferenceEncoding), "image1": _gray(2), **masks})


def test_encode_reference_has_no_cpu_path(matcher):
    from pope_amd._lib import PopeHipError
    with pytest.raises(PopeHipError, match="no CPU fallback"):
        matcher.encode_reference(_gray(1))
    with pytest.raises(ValueError, match=r"\[R, 1, H0, W0\]"):
        matcher.encode_reference(torch.zeros(32, 32))


def test_a_move_invalidates_reference_encodings():
    from pope_amd.matcher import Matcher, default_cfg
    m = Matcher(default_cfg).eval()
    before = m._moves
    m.float()
    assert m._moves == before + 1          # `.to()` / `.cuda()` / `.float()`: every encoding's key goes stale


def test_leading_self_layers():
    from pope_amd.loftr import LocalFeatureTransformer
    from pope_amd.matcher import default_cfg
    cfg = dict(default_cfg["coarse"])
    assert LocalFeatureTransformer(cfg).n_leading_self == 1
    for names, k in ((["self", "self", "cross"], 2), (["cross", "self"], 0), (["self", "self"], 2)):
        assert LocalFeatureTransformer(dict(cfg, layer_names=names)).n_leading_self == k


# ---- the C entry ---------------------------------------------------------------------------------------------------------
def test_indexed_fine_entry_is_exported_and_validates_without_gpu(hip_lib):
    assert hip_lib.pope_abi_version() == 10
    fn = hip_lib.pope_fine_preprocess_f32
    # the index, the pair count and the row count sit between the range flag and the stream
    assert _lib.PROTOTYPES["pope_fine_preprocess_f32"][1][-5:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                   ctypes.c_void_p]
    buf = ctypes.create_string_buffer(256)
    ok = (ctypes.addressof(buf) + 15) & ~15                  # never dereferenced: every call below stops at the checks
    st = (ctypes.c_longlong * 4)(1, 1, 1, 1)

    def call(ptrs=None, index=ok, n=5, n0=2):
        p = dict(f0=ok, f1=ok, c0=ok, c1=ok, b=ok, i=ok, j=ok, dw=ok, db=ok, mw=ok, mb=ok, out=ok, ws=ok)
        p.update(ptrs or {})
        return fn(p["f0"], st, 24, 32, 8, p["f1"], st, 24, 32, 8, p["c0"], p["c1"], 48, 48, 256, 128, p["b"], p["i"], p["j"], 37, 5, 4,
                  p["dw"], p["db"], p["mw"], p["mb"], _lib.PREC_F16X3, p["out"], p["ws"], 1 << 20, None, index, n, n0, None)

    for name in ("f0", "f1", "c0", "c1", "b", "i", "j", "dw", "mw", "out", "ws"):
        assert call({name: None}) == -1, name                # POPE_ERR_ARG
    assert call(n=-1) == -1 and call(n0=-1) == -1
    assert call(index=None, n=-1) == -1                      # a negative n is refused with and without an index
    assert call(n=0) == -1 and call(n0=0) == -1              # an index over no pairs / no rows


# ---- the driver ------------------------------------------------------------------------------------------------------------
class _On(torch.nn.Module):
    """Stands for a model on the CPU: nothing of it is run."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def _refset(R=2):
    from pope_amd.driver import ReferenceSet
    return ReferenceSet(torch.zeros(R, 384), torch.zeros(R, 1, 32, 32), None)


def test_exports_and_keywords():
    from pope_amd import driver, pope_model_api
    assert pope_model_api.encode_references is driver.encode_references and pope_model_api.ReferenceSet is driver.ReferenceSet
    for fn in (driver.locate_and_match_batch_u8, driver.locate_match_pose_batch_u8):
        assert inspect.signature(fn).parameters["ref_index"].default is None


def test_ref_index_validation():
    from pope_amd.driver import _ref_index
    assert _ref_index(None, 3, 3, "t") == [0, 1, 2]
    assert _ref_index([0] * 8, 1, 8, "t") == [0] * 8
    assert _ref_index(torch.tensor([1, 0]), 2, None, "t") == [1, 0]
    with pytest.raises(ValueError, match="needs ref_index"):
        _ref_index(None, 2, 3, "t")
    with pytest.raises(ValueError, match="3 ref_index entries for 4 queries"):
        _ref_index([0, 0, 1], 2, 4, "t")
    for bad in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match=r"\[0, 2\)"):
            _ref_index(bad, 2, 2, "t")
    with pytest.raises(ValueError, match="integers"):
        _ref_index([0.0, 1.0], 2, 2, "t")


def test_reference_set_calls_check_their_counts_before_any_launch():
    from pope_amd.driver import locate_and_match_batch_u8, locate_match_pose_batch_u8, locate_pose_from_frames
    vit, refs = _On(), _refset(2)
    crops = np.zeros((4, 256, 256, 3), np.uint8)
    frames = np.zeros((4, 64, 64, 3), np.uint8)
    boxes = [np.zeros((1, 4), np.int64)] * 4
    K = np.eye(3)
    # wrong Q: three reference rows named for four queries
    with pytest.raises(ValueError, match="3 proposal counts for|for 3 queries"):
        locate_and_match_batch_u8(vit, None, refs, crops, [1, 1, 1, 1], ref_index=[0, 0, 1])
    with pytest.raises(ValueError, match="3 references, 4 frames"):
        locate_match_pose_batch_u8(vit, None, refs, frames, boxes, K, K, ref_index=[0, 0, 1])
    # no index: a set of two stands for two queries
    with pytest.raises(ValueError, match="2 references, 4 frames"):
        locate_match_pose_batch_u8(vit, None, refs, frames, boxes, K, K)
    # a reference row that does not exist
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        locate_and_match_batch_u8(vit, None, refs, crops, [1, 1, 1, 1], ref_index=[0, 0, 2, 0])
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        locate_match_pose_batch_u8(vit, None, refs, frames, boxes, K, K, ref_index=[0, 0, 2, 0])
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        refs.select([0, 5])
    # image references take the keyword too
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        locate_match_pose_batch_u8(vit, None, np.zeros((2, 32, 32, 3), np.uint8), frames, boxes, K, K, ref_index=[0, 0, 2, 0])
    # a selection stands for its length; giving both it and the keyword is ambiguous
    sel = refs.select([0, 0, 1, 0])
    assert len(sel) == 4 and sel.R == 2 and len(refs) == 2 and sel.encoding is refs.encoding and sel.cls is refs.cls
    with pytest.raises(ValueError, match="already carries a selection"):
        locate_match_pose_batch_u8(vit, None, sel, frames, boxes, K, K, ref_index=[0, 0, 1, 0])

    class Gen:
        class predictor:
            device = "cpu"

    matcher = _On()
    with pytest.raises(ValueError, match="2 references, 4 frames"):   # the frame-level call counts a set like images
        locate_pose_from_frames(Gen(), vit, matcher, refs, frames, K, K)
