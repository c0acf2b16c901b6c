"""`pope_sam_rle_u32` (pope_amd/csrc/sam_rle.hip) on the MI355X against tests/golden/sam_rle.npz (the reference's
`mask_to_rle_pytorch` of edge masks) and against the run lengths tests/golden/sam_generator.npz holds for its NMS survivors.
Run lengths are integers: every comparison is an equality."""
import numpy as np
import pytest
import torch

from pope_amd import _lib, sam_amg, synth
from pope_amd import sam_generator as sg
from pope_amd._lib import ptr, stream_of
from test_sam_generator_cpu import golden
from test_sam_rle_cpu import SHAPES, rle_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_WORKSPACE = -3


def on_device(packed):
    return torch.as_tensor(np.ascontiguousarray(packed).view(np.int32), device=DEV)


def counts_of(rles):
    return [r["counts"] for r in rles]


@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_equals_the_edge_fixture(golden_dir, H, W):
    packed, want = rle_golden(golden_dir, H, W)
    got = sg.rle_from_packed(on_device(packed), W)
    print(f"{H}x{W}: lengths {[len(c) for c in want]}")
    assert all(r["size"] == [H, W] for r in got)
    assert [len(c) for c in counts_of(got)] == [len(c) for c in want]
    assert counts_of(got) == want
    # pad bits are not pixels: set them all and nothing changes
    if W % 32:
        dirty = packed.copy()
        dirty[:, :, -1] |= np.uint32((0xffffffff << (W % 32)) & 0xffffffff)
        assert not np.array_equal(dirty, packed)
        assert counts_of(sg.rle_from_packed(on_device(dirty), W)) == want


@pytest.mark.parametrize("name", list(synth.SAM_GENERATOR_CASES))
def test_kernel_equals_the_generator_fixture(golden_dir, name):
    fx = golden(golden_dir, name)
    H, W = synth.SAM_GENERATOR_CASES[name][1]
    got = counts_of(sg.rle_from_packed(on_device(fx["packed"]), W))
    assert np.array_equal([len(c) for c in got], fx["rle_lengths"])
    assert np.array_equal(np.concatenate(got), fx["rle_counts"])


def test_output_does_not_depend_on_the_batch(golden_dir):
    packed, want = rle_golden(golden_dir, 65, 33)
    order = [8, 3, 5, 0, 7, 1, 6, 2, 4]
    assert counts_of(sg.rle_from_packed(on_device(packed[order]), 33)) == [want[i] for i in order]
    for i in (5, 7):
        assert counts_of(sg.rle_from_packed(on_device(packed[i:i + 1]), 33)) == [want[i]]
    # many more masks than a card runs at once
    many = counts_of(sg.rle_from_packed(on_device(np.tile(packed, (70, 1, 1))), 33))
    assert len(many) == 630 and many == want * 70


def test_wide_mask_spans_several_column_strips():
    # 1100 columns: more than the 1024 one pass of the workgroup covers, and the last word is partial
    rng = np.random.default_rng(7)
    masks = rng.random((3, 70, 1100)) < 0.3
    masks[1, :, 1000:1030] = True                      # a run across the strip boundary
    masks[2, :, 1024:] = False
    got = sg.rle_from_packed(on_device(sam_amg.pack_masks(masks)), 1100)
    assert got == [sam_amg.mask_to_rle(m) for m in masks]


def test_empty_batch_and_capacity(golden_dir):
    assert sg.rle_from_packed(torch.zeros(0, 65, 2, dtype=torch.int32, device=DEV), 33) == []
    lib = _lib.lib()
    stream = stream_of(torch.device(DEV))
    sentinel = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    assert lib.pope_sam_rle_u32(None, 0, 65, 33, ptr(sentinel), None, None, 0, stream) == 0       # n == 0: nothing is written
    torch.cuda.synchronize()
    assert bool((sentinel == -7).all())
    packed, want = rle_golden(golden_dir, 65, 33)
    words = on_device(packed)
    n = words.shape[0]
    lengths = torch.empty(n, dtype=torch.int32, device=DEV)
    assert lib.pope_sam_rle_u32(ptr(words), n, 65, 33, ptr(lengths), None, None, 0, stream) == 0
    assert lengths.cpu().tolist() == [len(c) for c in want]
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    offsets[1:] = torch.cumsum(lengths.to(torch.int64), 0)
    total = int(offsets[-1])
    # one entry short: an error, and the buffer (with room to spare behind the claimed capacity) stays as it was
    out = torch.full((total + 16,), -7, dtype=torch.int32, device=DEV)
    assert lib.pope_sam_rle_u32(ptr(words), n, 65, 33, None, ptr(offsets), ptr(out), total - 1, stream) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    # the exact capacity: everything up to it is written, nothing behind it
    assert lib.pope_sam_rle_u32(ptr(words), n, 65, 33, None, ptr(offsets), ptr(out), total, stream) == 0
    torch.cuda.synchronize()
    assert out[:total].cpu().tolist() == [v for c in want for v in c]
    assert bool((out[total:] == -7).all())
