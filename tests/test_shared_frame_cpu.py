"""CPU: queries that share a frame (`frame_index`) — `driver.share_frames`, the argument checks of the three driver calls (raised
before any model is touched) and of `ops.vote_top3_shared`, and the C ABI of `pope_vote_top3_shared_f32`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pope_amd import _lib
from pope_amd.driver import SharedFrames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoGpu:
    """Stands where the models go: any use of it (parameters(), a call) means a model was touched."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check came after a use of the model ({name})")

    def __call__(self, *a, **k):
        raise AssertionError("the argument check came after a use of the model")


# ---- share_frames ------------------------------------------------------------------------------------------------------
def test_share_frames_groups_by_first_appearance():
    from pope_amd.driver import share_frames
    assert share_frames(["b", "a", "b", "c", "a"]) == ([0, 1, 3], [0, 1, 0, 2, 1])
    assert share_frames([]) == ([], [])
    assert share_frames([(1, 7)] * 3) == ([0], [0, 0, 0])
    keys = [(3, 1), (2, 1), (3, 1), (3, 2), (2, 1), (9, 9)]
    positions, frame_index = share_frames(keys)
    assert all(keys[positions[frame_index[q]]] == keys[q] for q in range(len(keys)))
    assert positions == sorted(positions) and len(set(keys[p] for p in positions)) == len(positions) == len(set(keys))


def test_linemod_list_shares_a_fifth_of_its_frames(golden_dir):
    from pope_amd.driver import share_frames
    from pope_amd.pipeline import load_pair_list
    pairs = load_pair_list(os.path.join(golden_dir, "linemod_pairs.json"))
    keys = [(int(o), int(i1)) for o, _, _, i1 in pairs]           # (object, target frame)
    positions, frame_index = share_frames(keys)
    assert len(keys) == 5796 and len(positions) == 4555 and len(frame_index) == 5796
    assert max(frame_index) == 4554 and all(keys[positions[f]] == k for f, k in zip(frame_index, keys))

    def frames_at(batch):      # a walker that groups within each batch of its walk order
        return sum(len(share_frames(keys[s:s + batch])[0]) for s in range(0, len(keys), batch))
    assert frames_at(128) == 5426 and frames_at(8) == 5772


# ---- the driver's checks -----------------------------------------------------------------------------------------------
REFS = np.zeros((3, 64, 64, 3), np.uint8)                  # Q = 3 queries
FRAMES = np.zeros((2, 48, 64, 3), np.uint8)                # F = 2 frames
BOXES = [np.array([[4, 4, 20, 20]]), np.zeros((0, 4), np.int64)]
K = np.eye(3)
BAD_INDEX = {"short": [0, 1], "long": [0, 1, 0, 1], "float": [0.0, 1.0, 0.0], "negative": [0, -1, 0], "past the frames": [0, 2, 0],
             "two-dimensional": [[0, 1, 0]]}


@pytest.mark.parametrize("why", sorted(BAD_INDEX))
def test_bad_frame_index_is_refused_before_any_model_is_touched(why):
    from pope_amd.driver import locate_and_match_batch_u8, locate_match_pose_batch_u8, locate_pose_from_frames
    bad = BAD_INDEX[why]
    for index in (bad, np.asarray(bad), torch.as_tensor(bad)):
        with pytest.raises(ValueError, match="frame_index"):
            locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), REFS, FRAMES, BOXES, K, K, frame_index=index)
        with pytest.raises(ValueError, match="frame_index"):
            locate_pose_from_frames(_NoGpu(), _NoGpu(), _NoGpu(), REFS, SharedFrames(FRAMES, index), K, K)
        with pytest.raises(ValueError, match="frame_index"):
            locate_and_match_batch_u8(_NoGpu(), _NoGpu(), REFS, np.zeros((5, 256, 256, 3), np.uint8), [5, 0], frame_index=index)


def test_box_lists_and_frame_cameras_are_per_frame():
    from pope_amd.driver import locate_match_pose_batch_u8, locate_pose_from_frames
    index = [0, 1, 0]
    for boxes in (BOXES[:1], BOXES + BOXES[:1]):            # one and three box lists for two frames
        with pytest.raises(ValueError, match="box lists"):
            locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), REFS, FRAMES, boxes, K, K, frame_index=index)
    per_query = np.tile(K, (3, 1, 1))
    with pytest.raises(ValueError, match="K1"):              # K1 is per frame: [3, 3] or [2, 3, 3]
        locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), REFS, FRAMES, BOXES, K, per_query, frame_index=index)
    with pytest.raises(ValueError, match="K1"):
        locate_pose_from_frames(_NoGpu(), _NoGpu(), _NoGpu(), REFS, SharedFrames(FRAMES, index), K, per_query)
    with pytest.raises(ValueError, match="K0"):              # K0 is per query: [3, 3] or [3, 3, 3]
        locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), REFS, FRAMES, BOXES, np.tile(K, (2, 1, 1)), K, frame_index=index)
    with pytest.raises(ValueError, match="frame_index"):     # with ref_index the number of queries is its length
        locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), REFS, FRAMES, BOXES, K, K, ref_index=[0, 0, 1, 2], frame_index=index)


def test_crop_counts_are_per_frame():
    from pope_amd.driver import locate_and_match_batch_u8
    crops = np.zeros((5, 256, 256, 3), np.uint8)
    with pytest.raises(ValueError, match="sum"):
        locate_and_match_batch_u8(_NoGpu(), _NoGpu(), REFS, crops, [4, 0], frame_index=[0, 1, 0])
    with pytest.raises(ValueError, match="sum"):
        locate_and_match_batch_u8(_NoGpu(), _NoGpu(), REFS, crops, [6, -1], frame_index=[0, 1, 0])


def test_one_frame_call_checks_its_references():
    from pope_amd.driver import locate_poses_in_frame
    with pytest.raises(ValueError, match="K1"):              # one frame, one camera
        locate_poses_in_frame(_NoGpu(), _NoGpu(), _NoGpu(), REFS, FRAMES[0], K, np.tile(K, (3, 1, 1)))


# ---- ops.vote_top3_shared and the C entry ------------------------------------------------------------------------------
class _OnDevice:
    """A tensor that says it is on the GPU: `ops` checks the arguments before it reads a pointer."""

    def __init__(self, *shape):
        self.shape, self.dtype, self.is_cuda, self.device = torch.Size(shape), torch.float32, True, torch.device("cuda:0")

    def dim(self):
        return len(self.shape)

    def contiguous(self):
        return self

    def __getattr__(self, name):
        raise AssertionError(f"the argument check came after a use of the tensor ({name})")


@pytest.mark.parametrize("counts, which", [([2, 2], [0, 1, 0]), ([6, -1], [0, 1, 0]), ([5, 0], [0, 1]), ([5, 0], [0, 2, 0]),
                                           ([5, 0], [0, -1, 0]), ([5, 0], [0.0, 1.0, 0.0]), ([5, 0], [[0, 1, 0]])])
def test_vote_shared_checks_counts_and_indices_on_the_host(counts, which):
    from pope_amd import ops
    with pytest.raises(ValueError, match="vote_top3_shared"):
        ops.vote_top3_shared(_OnDevice(3, 16), _OnDevice(5, 16), counts, which)


def test_new_symbol_declared_bound_and_reexported(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pope_hip.h")).read(), flags=re.S)
    name = "pope_vote_top3_shared_f32"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in pope_hip.h"
    assert name in _lib.PROTOTYPES and hasattr(hip_lib, name)
    res, args = _lib.PROTOTYPES[name]
    p, i = ctypes.c_void_p, ctypes.c_int
    assert res is i and args == [p, p, p, i, p, p, i, i, i, ctypes.c_float, p, p, p, p, p, p]
    assert hip_lib.pope_abi_version() == 10
    from pope_amd import pope_model_api as api
    for exported in ("locate_poses_in_frame", "share_frames", "vote_top3_shared", "SharedFrames"):
        assert callable(getattr(api, exported))


def test_shared_frames_stands_for_its_queries_and_leaves_the_signature_alone():
    """`locate_pose_from_frames` keeps the parameter list of the reference's loop body: the index rides on the frames."""
    import inspect
    from pope_amd import driver
    shared = SharedFrames(FRAMES, [0, 1, 0])
    assert len(shared) == 3 and shared.frames is FRAMES and shared.index == [0, 1, 0]
    assert "frame_index" not in inspect.signature(driver.locate_pose_from_frames).parameters
    for fn in (driver.locate_match_pose_batch_u8, driver.locate_and_match_batch_u8):
        assert inspect.signature(fn).parameters["frame_index"].default is None
    from test_frame_query_cpu import _Generator, _On
    with pytest.raises(ValueError, match="3 references, 2 frames"):      # plain frames are still one per query
        driver.locate_pose_from_frames(_Generator("cpu"), _On("cpu"), _On("cpu"), REFS, FRAMES, K, K)


def test_empty_shared_vote_launches_nothing(hip_lib):
    """Q = 0 returns POPE_OK before any HIP call; bad sizes and missing arrays are refused."""
    fn = hip_lib.pope_vote_top3_shared_f32
    nul = [None] * 5
    assert fn(None, None, None, 2, None, None, 0, 0, 384, 1e-8, *nul, None) == 0
    assert fn(None, None, None, 2, None, None, 1, 0, 384, 1e-8, *nul, None) == -1
    assert fn(None, None, None, 2, None, None, -1, 0, 384, 1e-8, *nul, None) == -1
    assert fn(None, None, None, -1, None, None, 0, 0, 384, 1e-8, *nul, None) == -1
    assert fn(None, None, None, 2, None, None, 0, 0, 0, 1e-8, *nul, None) == -1
