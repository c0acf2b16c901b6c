"""CPU: the host side of the learned pose regressor (pope_amd/pose_regressor.py) — state-dict layout, the replay of the reference's
collate sampling, the numpy statement of the device sampler, and argument checks that need no GPU."""
import os
import random

import numpy as np
import pytest
import torch

from pope_amd import synth
from pope_amd.pose_regressor import (COLLATE_SEED, Mkpts_Reg_Model, device_sample_indices, reference_sample_indices,
                                     regress_pose_batch)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_regressor.npz"))


@pytest.mark.parametrize("mode", list(synth.POSE_REGRESSOR_MODES))
def test_state_dict_keys_are_the_reference_s(gold, mode):
    want = list(zip(gold[f"keys_S5_{mode}.names"].tolist(), gold[f"keys_S5_{mode}.shapes"].tolist()))
    assert len(want) == 78
    model = Mkpts_Reg_Model(5, mode)
    got = [(k, "x".join(str(d) for d in v.shape)) for k, v in model.state_dict().items()]
    assert got == want
    assert [(k, "x".join(str(d) for d in s)) for k, s in synth.pose_regressor_keys(5, mode)] == want
    model.load_state_dict(synth.pose_regressor_state_dict(5, mode), strict=True)
    assert sum(k.startswith("transformerlayer.") for k, _ in want) == 12      # the unused template layer is part of the file


def _collate_restated(num_sample):
    """pose/utils.py:collate_fn restated: the seed is set once, a pair's mkpts0 and mkpts1 are sampled with a draw each."""
    random.seed(COLLATE_SEED)

    def collate(batch):
        out = []
        for data in batch:
            item = {}
            for key in data:
                item[key] = data[key]
                if key in ("mkpts0", "mkpts1"):
                    if item[key].shape[0] > num_sample:
                        item[key] = item[key][random.sample(range(item[key].shape[0]), num_sample), :]
                    else:
                        item[key] = np.concatenate((item[key], np.zeros((num_sample - item[key].shape[0], 2), np.float32)), axis=0)
            out.append(item)
        return out
    return collate


def test_reference_sample_indices_replays_collate():
    S, counts = 7, [3, 7, 8, 30, 0, 7, 19, 6, 100]
    # rows carry their own number (+ 1, so that padding stays distinguishable) in both columns
    batch = [{"mkpts0": np.repeat(np.arange(1, c + 1, dtype=np.float32)[:, None], 2, 1),
              "mkpts1": np.repeat(np.arange(1, c + 1, dtype=np.float32)[:, None], 2, 1), "other": 1} for c in counts]
    collate = _collate_restated(S)
    want = collate(batch[:4]) + collate(batch[4:])       # two batches: the state carries across calls as across pairs
    got = reference_sample_indices(counts, S)
    assert got.shape == (len(counts), 2, S) and got.dtype == np.int32
    for b, item in enumerate(want):
        for k, key in enumerate(("mkpts0", "mkpts1")):
            assert np.array_equal(got[b, k], item[key][:, 0].astype(np.int32) - 1), (b, key)
    assert np.array_equal(got[1, 0], np.arange(S))        # count == S is not sampled
    assert not np.array_equal(got[2, 0], got[2, 1])       # the two point sets of a pair draw separately
    # continuing from a caller's generator
    rng = random.Random(COLLATE_SEED)
    parts = np.concatenate([reference_sample_indices(counts[:4], S, rng), reference_sample_indices(counts[4:], S, rng)])
    assert np.array_equal(parts, got)


@pytest.mark.parametrize("S", [5, 37, 70])
def test_device_sampler_statement(S):
    for count in (S + 1, 2 * S, 4 * S, 1500):
        for seed in (0, 1, 2 ** 63 + 5):
            idx = device_sample_indices(count, S, seed)
            assert idx.shape == (S,) and idx.dtype == np.int32
            assert len(set(idx.tolist())) == S and idx.min() >= 0 and idx.max() < count
        assert not np.array_equal(device_sample_indices(count, S, 0), device_sample_indices(count, S, 1))
        assert not np.array_equal(device_sample_indices(count, S, 0), np.sort(device_sample_indices(count, S, 0)))   # ordered sample
    for count in (0, 3, S - 1, S):
        idx = device_sample_indices(count, S, 0)
        assert np.array_equal(idx[:count], np.arange(count)) and (idx[count:] == -1).all()
    # one hand-computed key: splitmix64(0 ^ 1 * 0xD1B54A32D192ED03)
    x = (0xD1B54A32D192ED03 + 0x9E3779B97F4A7C15) % 2 ** 64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    x ^= x >> 31
    from pope_amd.pose_regressor import _splitmix64
    with np.errstate(over="ignore"):
        assert int(_splitmix64(np.uint64(0xD1B54A32D192ED03))) == x


def test_uniformity_of_the_device_sampler():
    # every match is equally likely to be kept: 2000 seeds, 10 of 40 -> each index kept 500 +- 5 sigma (sigma = sqrt(2000 * .25 * .75))
    hits = np.zeros(40)
    for seed in range(2000):
        hits[device_sample_indices(40, 10, seed)] += 1
    assert np.abs(hits - 500).max() < 5 * (2000 * 0.25 * 0.75) ** 0.5


def test_inference_only_and_no_cpu_path():
    from pope_amd._lib import PopeHipError
    model = Mkpts_Reg_Model(5)
    assert not model.training
    with pytest.raises(NotImplementedError):
        model.train()
    model.eval()
    with pytest.raises(PopeHipError):
        model(torch.zeros(1, 5, 2), torch.zeros(1, 5, 2))
    with pytest.raises(PopeHipError):
        regress_pose_batch(model, torch.zeros(4, 2), torch.zeros(4, 2), [4])
    with pytest.raises(ValueError):
        Mkpts_Reg_Model(5, "euler")


def test_c_entries_refuse_bad_arguments_without_a_gpu(hip_lib):
    import ctypes
    from pope_amd import _lib
    buf = ctypes.create_string_buffer(1024)
    ok = (ctypes.addressof(buf) + 255) & ~255
    w = _lib.PoseRegressorWeights()
    fwd = hip_lib.pope_pose_regressor_forward_f32
    # null weights / outputs, both or neither input form, B, S
    assert fwd(None, ok, ok, None, None, None, None, None, 1, 5, 1, 0, ok, ok, ok, ok, 1 << 20, None) == -1
    assert hip_lib.pope_pose_regressor_embedding_f32(None, None, None, None, None, None, None, 1, 5, 0, ok, ok, ok, None) == -1
    assert hip_lib.pope_pose_regressor_embedding_f32(ok, ok, None, None, ok, None, None, 1, 5, 0, ok, ok, ok, None) == -1
    assert hip_lib.pope_pose_regressor_embedding_f32(ok, ok, None, None, None, None, None, 0, 5, 0, ok, ok, ok, None) == -1
    assert hip_lib.pope_pose_regressor_embedding_f32(ok, ok, None, None, None, None, None, 1, 0, 0, ok, ok, ok, None) == -1
    assert hip_lib.pope_pose_regressor_embedding_f32(ok, ok, None, None, None, None, None, 1, 5, 0, None, ok, ok, None) == -1
    w.num_sample, w.mode = 5, 0        # every weight pointer null
    assert fwd(ctypes.byref(w), ok, ok, None, None, None, None, None, 1, 5, 1, 0, ok, ok, ok, ok, 1 << 20, None) == -1
    assert hip_lib.pope_pose_regressor_workspace_bytes(0, 5) == 0
    n = hip_lib.pope_pose_regressor_workspace_bytes(3, 37)
    assert n >= 3 * 37 * (76 + 1 + 19 + 1) * 4 and n < 3 * 37 * 97 * 4 + 4 * 256
