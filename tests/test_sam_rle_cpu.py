"""CPU: tests/golden/sam_rle.npz (the reference's `mask_to_rle_pytorch` of seeded edge masks, written by
scripts/gen_golden_sam_rle.py) against the CPU definition `sam_amg.mask_to_rle`, and the shape of the new surface: the two C
entries (`pope_sam_rle_u32`, `pope_sam_nms_segments_f32`), their argument checks, which run before any HIP call, and the
Python signatures.  No tolerances."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from pope_amd import _lib, sam_amg
from pope_amd import sam_generator as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 70), (70, 1), (64, 32), (65, 33), (129, 95), (200, 100))
PATTERNS = ("zero", "one", "first", "last", "crossing", "checker", "checker_inv", "bernoulli", "rectangle")
ERR_ARG = -1


def rle_golden(golden_dir, H, W):
    """(packed uint32 [9, H, words], list of the 9 count lists) of one fixture shape."""
    fx = np.load(os.path.join(golden_dir, "sam_rle.npz"))
    key = f"{H}x{W}"
    off = np.concatenate([[0], np.cumsum(fx[key + ".lengths"])])
    return fx[key + ".packed"], [fx[key + ".counts"][off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_fixture_is_reproduced_and_inverted(golden_dir, H, W):
    packed, counts = rle_golden(golden_dir, H, W)
    assert packed.shape == (len(PATTERNS), H, sam_amg.row_words(W)) and packed.dtype == np.uint32
    masks = sam_amg.unpack_masks(packed, W)
    assert np.array_equal(sam_amg.pack_masks(masks), packed)               # pad bits zero in the fixture
    for m, c in zip(masks, counts):
        rle = sam_amg.mask_to_rle(m)
        assert rle == {"size": [H, W], "counts": c}
        assert np.array_equal(sam_amg.rle_to_mask(rle), m)
        assert sum(c) == H * W and len(c) <= H * W + 1 and all(v > 0 for v in c[1:])


@pytest.mark.parametrize("H,W", SHAPES)
def test_fixture_holds_the_edge_rules(golden_dir, H, W):
    packed, counts = rle_golden(golden_dir, H, W)
    by = dict(zip(PATTERNS, counts))
    hw = H * W
    assert by["zero"] == [hw] and by["one"] == [0, hw]
    assert by["first"] == ([0, 1, hw - 1] if hw > 1 else [0, 1])           # a leading 0: the first pixel is set
    assert by["last"] == [hw - 1, 1]
    # the last row of column 0 and the first row of column 1 are neighbours in column-major order: one run of two
    assert by["crossing"] == ([H - 1, 2, hw - H - 1] if W > 1 and hw > H + 1 else ([H - 1, 2] if W > 1 else [H - 1, 1]))
    assert by["checker"][0] == 0 and by["checker_inv"][0] >= 1
    if H % 2 == 1 or W == 1:                                               # odd H: the pattern alternates across columns too
        assert len(by["checker"]) == hw + 1 and len(by["checker_inv"]) == hw
    else:
        assert len(by["checker"]) < hw


def test_python_surface():
    assert list(inspect.signature(sg.SamAutomaticMaskGenerator.generate_batch).parameters) == ["self", "images"]
    assert list(inspect.signature(sg.rle_from_packed).parameters) == ["packed", "W"]
    assert list(inspect.signature(sg.box_nms_segments).parameters) == ["boxes", "scores", "seg_offsets", "iou_threshold"]
    assert list(inspect.signature(sg.SamAutomaticMaskGenerator.generate).parameters) == ["self", "image", "keep_low_res"]
    # the generator's tail has no per-mask host encoding left; the CPU definition itself stays
    assert "mask_to_rle" not in inspect.getsource(sg.SamAutomaticMaskGenerator._finish)
    assert callable(sam_amg.mask_to_rle)


def test_header_declares_the_entries_and_the_binding_covers_them(hip_lib):
    with open(os.path.join(ROOT, "include", "pope_hip.h")) as f:
        header = f.read()
    for name in ("pope_sam_rle_u32", "pope_sam_nms_segments_f32"):
        assert f"int {name}(" in header
        assert name in _lib.PROTOTYPES and hasattr(hip_lib, name)
    assert len(_lib.PROTOTYPES["pope_sam_rle_u32"][1]) == 9 and len(_lib.PROTOTYPES["pope_sam_nms_segments_f32"][1]) == 9
    assert hip_lib.pope_abi_version() == 10


def test_argument_validation_without_gpu(hip_lib):
    buf = ctypes.create_string_buffer(64)
    ok = (ctypes.addressof(buf) + 15) & ~15            # never dereferenced: nothing below gets as far as a launch
    rle = hip_lib.pope_sam_rle_u32
    assert rle(None, 0, 480, 640, None, None, None, 0, None) == 0           # n == 0 is a no-op, whatever the pointers
    assert rle(ok, 0, 480, 640, ok, ok, ok, 0, None) == 0
    assert rle(None, 0, 0, 640, None, None, None, 0, None) == ERR_ARG       # the geometry is still checked
    for H, W in ((0, 8), (8, 0), (-1, 8), ((1 << 14) + 1, 8), (8, (1 << 14) + 1)):
        assert rle(ok, 1, H, W, ok, None, None, 0, None) == ERR_ARG, (H, W)
    assert rle(ok, -1, 8, 8, ok, None, None, 0, None) == ERR_ARG
    assert rle(None, 1, 8, 8, ok, None, None, 0, None) == ERR_ARG           # no masks
    assert rle(ok, 1, 8, 8, None, None, None, 0, None) == ERR_ARG           # lengths call without lengths
    assert rle(ok, 1, 8, 8, None, None, ok, 16, None) == ERR_ARG            # counts call without offsets
    assert rle(ok, 1, 8, 8, None, ok, ok, -1, None) == ERR_ARG              # negative capacity
    nms = hip_lib.pope_sam_nms_segments_f32
    assert nms(None, None, None, 0, 0, 0.35, None, None, None) == 0         # S == 0 is a no-op
    assert nms(ok, ok, None, 1, 4, 0.35, ok, ok, None) == ERR_ARG
    assert nms(ok, ok, ok, 1, 4, 0.35, ok, None, None) == ERR_ARG
    assert nms(None, ok, ok, 1, 4, 0.35, ok, ok, None) == ERR_ARG
    assert nms(ok, ok, ok, -1, 4, 0.35, ok, ok, None) == ERR_ARG and nms(ok, ok, ok, 1, -4, 0.35, ok, ok, None) == ERR_ARG
