"""CPU: the batched driver step's argument checks (raised before any GPU call) and the C ABI of its two kernels."""
import os
import re

import numpy as np
import pytest
import torch

from pope_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pope_vote_top3_batch_f32", "pope_slot_tally_f32")


class _NoGpu:
    """Stands where the models go: any use of it (parameters(), a call) means a GPU step was reached."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check came after a use of the model ({name})")

    def __call__(self, *a, **k):
        raise AssertionError("the argument check came after a use of the model")


def test_proposal_counts_must_sum_to_the_rows():
    from pope_amd.driver import locate_and_match_batch, locate_and_match_batch_u8
    refs, crops = torch.zeros(2, 3, 28, 28), torch.zeros(5, 3, 28, 28)
    g_refs, g_crops = torch.zeros(2, 1, 32, 32), torch.zeros(5, 1, 32, 32)
    with pytest.raises(ValueError, match="sum"):
        locate_and_match_batch(_NoGpu(), _NoGpu(), refs, crops, g_refs, g_crops, [2, 2])
    with pytest.raises(ValueError, match="sum"):
        locate_and_match_batch_u8(_NoGpu(), _NoGpu(), np.zeros((2, 32, 32, 3), np.uint8), np.zeros((5, 256, 256, 3), np.uint8), [4, 2])


def test_query_counts_must_agree():
    from pope_amd.driver import locate_and_match_batch, locate_and_match_batch_u8, locate_match_pose_batch_u8
    refs, crops = torch.zeros(2, 3, 28, 28), torch.zeros(5, 3, 28, 28)
    with pytest.raises(ValueError):     # three counts for two references
        locate_and_match_batch(_NoGpu(), _NoGpu(), refs, crops, torch.zeros(2, 1, 32, 32), torch.zeros(5, 1, 32, 32), [2, 2, 1])
    with pytest.raises(ValueError):     # three gray references for two queries
        locate_and_match_batch(_NoGpu(), _NoGpu(), refs, crops, torch.zeros(3, 1, 32, 32), torch.zeros(5, 1, 32, 32), [2, 3])
    with pytest.raises(ValueError):
        locate_and_match_batch_u8(_NoGpu(), _NoGpu(), np.zeros((2, 32, 32, 3), np.uint8), np.zeros((5, 256, 256, 3), np.uint8), [5])
    refs_u8, frames, K = np.zeros((2, 64, 64, 3), np.uint8), np.zeros((2, 48, 64, 3), np.uint8), np.eye(3)
    boxes = [np.array([[4, 4, 20, 20]]), np.zeros((0, 4), np.int64)]
    with pytest.raises(ValueError):     # three frames for two references
        locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), refs_u8, np.zeros((3, 48, 64, 3), np.uint8), boxes, K, K)
    with pytest.raises(ValueError):     # one box list for two references
        locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), refs_u8, frames, boxes[:1], K, K)
    with pytest.raises(ValueError):     # intrinsics of three queries
        locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), refs_u8, frames, boxes, K, np.tile(np.eye(3), (3, 1, 1)))


def test_frames_of_one_call_have_one_size():
    from pope_amd.driver import locate_match_pose_batch_u8
    refs_u8, K = np.zeros((2, 64, 64, 3), np.uint8), np.eye(3)
    boxes = [np.array([[4, 4, 20, 20]])] * 2
    frames = [np.zeros((48, 64, 3), np.uint8), np.zeros((48, 72, 3), np.uint8)]
    with pytest.raises(ValueError, match="size"):
        locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), refs_u8, frames, boxes, K, K)


def test_new_symbols_declared_bound_and_reexported(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pope_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in pope_hip.h"
        assert name in _lib.PROTOTYPES and hasattr(hip_lib, name)
    assert hip_lib.pope_abi_version() == 10
    from pope_amd import pope_model_api as api
    for name in ("locate_and_match_batch", "locate_and_match_batch_u8", "locate_match_pose_batch_u8"):
        assert callable(getattr(api, name))


def test_empty_calls_launch_nothing(hip_lib):
    """Q = 0 and M = 0 return POPE_OK before any HIP call; bad sizes are refused."""
    assert hip_lib.pope_vote_top3_batch_f32(None, None, None, 0, 0, 384, 1e-8, None, None, None, None, None, None) == 0
    assert hip_lib.pope_vote_top3_batch_f32(None, None, None, 1, 0, 384, 1e-8, None, None, None, None, None, None) == -1
    assert hip_lib.pope_vote_top3_batch_f32(None, None, None, -1, 0, 384, 1e-8, None, None, None, None, None, None) == -1
    nul = [None] * 7
    assert hip_lib.pope_slot_tally_f32(None, None, None, None, None, 0, 10, 0.9, *nul, None) == 0
    assert hip_lib.pope_slot_tally_f32(None, None, None, None, None, 2, 0, 0.9, *nul, None) == 0
    assert hip_lib.pope_slot_tally_f32(None, None, None, None, None, 2, 10, 0.9, *nul, None) == -1
