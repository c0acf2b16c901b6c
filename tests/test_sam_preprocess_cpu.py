"""SAM's input transform, the parts that need no GPU: the two C entries refuse bad arguments before any HIP call, frames on the
host still take the Pillow path, the torch forms of the coordinate maps are the numpy ones, and frames are dispatched by type.
A tensor on the `meta` device stands in for a CUDA tensor where only the dispatch is under test: it is a tensor that is not on
the CPU, and every check below raises before anything would touch its storage."""
import ctypes as C

import numpy as np
import pytest
import torch

from pope_amd import preprocess as pp
from pope_amd import sam_generator as sg
from test_sam_generator_cpu import small_sam

ERR_ARG, ERR_WORKSPACE = -1, -3            # POPE_ERR_ARG, POPE_ERR_WORKSPACE
FAKE = 1 << 20                             # a non-null, 16-byte aligned address that is never dereferenced
# the arguments of a valid 480 x 640 -> 768 x 1024 call, by name, in the order of pope_resize_u8
VALID = dict(img=FAKE, P=2, Hin=480, Win=640, hstart=FAKE, hcount=FAKE, hk=FAKE, kh=3, vstart=FAKE, vcount=FAKE, vk=FAKE, kv=3,
             OH=768, OW=1024)
SCRATCH = 2 * 480 * 1024 * 3               # P * Hin * OW * 3


def resize(lib, out=FAKE, scratch=FAKE, scratch_bytes=SCRATCH, **kw):
    a = dict(VALID, **kw)
    return lib.pope_resize_u8(*a.values(), out, scratch, scratch_bytes, None)


def sam_pre(lib, S=1024, out=FAKE, scratch=FAKE, scratch_bytes=SCRATCH, mean=True, std=True, **kw):
    a = dict(VALID, **kw)
    three = (C.c_float * 3)(1.0, 2.0, 3.0)
    return lib.pope_sam_preprocess_u8_f32(*a.values(), S, 0, three if mean else None, three if std else None, out, scratch,
                                          scratch_bytes, None)


@pytest.mark.parametrize("call", [resize, sam_pre])
def test_abi_rejects_bad_arguments_without_a_gpu(hip_lib, call):
    for name in ("img", "hstart", "hcount", "hk", "vstart", "vcount", "vk"):
        assert call(hip_lib, **{name: None}) == ERR_ARG, name
    assert call(hip_lib, out=None) == ERR_ARG and call(hip_lib, scratch=None) == ERR_ARG
    for name in ("P", "Hin", "Win", "kh", "kv", "OH", "OW"):
        for bad in (0, -1):
            assert call(hip_lib, **{name: bad}) == ERR_ARG, (name, bad)
    assert call(hip_lib, scratch_bytes=SCRATCH - 1) == ERR_WORKSPACE
    assert call(hip_lib, scratch_bytes=0) == ERR_WORKSPACE
    assert call(hip_lib, P=3) == ERR_WORKSPACE                      # the scratch of two frames for three


def test_fp32_entry_rejects_its_own_arguments_without_a_gpu(hip_lib):
    assert sam_pre(hip_lib, mean=False) == ERR_ARG and sam_pre(hip_lib, std=False) == ERR_ARG
    for S in (0, -4, 1022, 1023, 512, 1020):                        # not positive, no multiple of 4, smaller than OW or OH
        assert sam_pre(hip_lib, S=S) == ERR_ARG, S
    assert sam_pre(hip_lib, OH=1025) == ERR_ARG
    assert sam_pre(hip_lib, out=FAKE + 4) == ERR_ARG                # 16-byte stores
    assert sam_pre(hip_lib, S=1024, scratch_bytes=SCRATCH - 1) == ERR_WORKSPACE


def pillow(frame, hw):
    from PIL import Image
    return np.array(Image.fromarray(frame).resize((hw[1], hw[0]), Image.BILINEAR))


@pytest.mark.parametrize("hw", [(48, 64), (33, 32), (130, 170)])
def test_host_frames_still_take_the_pillow_path(hw):
    frame = np.random.default_rng(hw[0]).integers(0, 256, hw + (3,), dtype=np.uint8)
    t = sg.ResizeLongestSide(96)
    out_hw = t.get_preprocess_shape(*hw, 96)
    want = pillow(frame, out_hw)
    for form in (frame, torch.from_numpy(frame)):
        got = t.apply_image(form)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == out_hw + (3,) and np.array_equal(got, want)
    assert pp.frames_on_device([frame, torch.from_numpy(frame)], "test") is None      # host frames, whatever their type
    assert pp.frames_on_device(np.stack([frame, frame]), "test") is None
    assert pp.frames_on_device(torch.from_numpy(frame)[None], "test") is None


def test_the_tables_reproduce_pillow_for_the_sam_geometries():
    """The arithmetic the two kernels run, restated in numpy from `resize_tables` (horizontal pass of every row, then the
    vertical pass, each rounded to uint8), against Pillow for small frames of the kinds the GPU test uses: an upscale, a
    portrait, a 5-tap downscale, a clipped window, an identity in x and a single output row."""
    def one_pass(a, axis, out):                                     # a [H, W, 3] uint8, resampled along `axis` to `out` samples
        start, count, kk = pp.resize_tables(a.shape[axis], out)
        a = np.moveaxis(a, axis, 0).astype(np.int64)
        rows = [(a[s:s + n] * kk[i, :n, None, None]).sum(0) + (1 << (pp.PRECISION_BITS - 1)) for i, (s, n) in enumerate(zip(start, count))]
        return np.moveaxis(np.clip(np.stack(rows) >> pp.PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)

    for hw, side in (((48, 64), 96), ((33, 32), 100), ((130, 170), 64), ((5, 7), 100), ((9, 64), 64), ((2, 150), 100)):
        frame = np.random.default_rng(sum(hw)).integers(0, 256, hw + (3,), dtype=np.uint8)
        oh, ow = sg.ResizeLongestSide.get_preprocess_shape(*hw, side)
        got = one_pass(one_pass(frame, 1, ow), 0, oh)
        assert np.array_equal(got, pillow(frame, (oh, ow))), (hw, side)


def test_coordinate_maps_in_torch_equal_the_numpy_ones():
    """`apply_coords_torch` works in float32 as the reference's does: float32(x) * float32(factor), one rounding of the factor and
    one of the product, so it is within 2^-23 relative of the float64 `apply_coords` (two roundings of 2^-24 each, and their
    product term) and equal to it bit for bit where the factors are powers of two."""
    rng = np.random.default_rng(2)
    for (H, W), side in (((480, 640), 1024), ((333, 332), 1024), ((1300, 1700), 1024), ((256, 512), 1024)):
        t = sg.ResizeLongestSide(side)
        pts = (rng.random((5, 7, 2)) * [W, H]).astype(np.float32)
        boxes = (rng.random((6, 4)) * [W, H, W, H]).astype(np.float32)
        nh, nw = t.get_preprocess_shape(H, W, side)
        for got, want, src in ((t.apply_coords_torch(torch.from_numpy(pts), (H, W)), t.apply_coords(pts, (H, W)), pts),
                               (t.apply_boxes_torch(torch.from_numpy(boxes), (H, W)), t.apply_boxes(boxes, (H, W)), boxes)):
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
            f = np.array([nw / W, nh / H], np.float32)
            restated = (src.reshape(-1, 2) * f).reshape(want.shape)
            assert np.array_equal(got.numpy(), restated)
            assert np.all(np.abs(got.numpy().astype(np.float64) - want) <= np.abs(want) * 2.0 ** -23)
            if (H, W) == (256, 512):                                # factors 2.0 and 2.0: nothing is rounded
                assert np.array_equal(got.numpy().astype(np.float64), want)
    src = torch.from_numpy(pts)
    keep = src.clone()
    sg.ResizeLongestSide(1024).apply_coords_torch(src, (480, 640))
    assert torch.equal(src, keep)                                   # a copy, as `apply_coords` makes one
    ints = sg.ResizeLongestSide(1024).apply_boxes_torch(torch.tensor([[1, 2, 3, 4]]), (256, 512))
    assert ints.dtype == torch.float32 and ints.tolist() == [[2.0, 4.0, 6.0, 8.0]]


def test_frames_are_dispatched_by_type_and_checked_before_any_work():
    sam, _ = small_sam(depth=1)
    gen = sg.SamAutomaticMaskGenerator(sam, points_per_side=2)
    host = np.zeros((48, 64, 3), np.uint8)
    meta = torch.empty(48, 64, 3, dtype=torch.uint8, device="meta")
    for call in (gen.generate_batch, gen.propose_batch):
        with pytest.raises(ValueError, match="all host arrays or all device tensors"):
            call([host, meta])
        with pytest.raises(ValueError, match="one size"):
            call([meta, torch.empty(48, 32, 3, dtype=torch.uint8, device="meta")])
        with pytest.raises(TypeError):
            call([meta.float(), meta.float()])
        with pytest.raises(TypeError):
            call(torch.empty(2, 48, 64, 4, dtype=torch.uint8, device="meta"))
        with pytest.raises(ValueError, match="the model on cpu"):      # frames on another device than the model
            call(torch.empty(2, 48, 64, 3, dtype=torch.uint8, device="meta"))
    for call in (gen.generate, gen.propose, gen.predictor.set_image, gen.predictor.transform.apply_image):
        with pytest.raises(TypeError):
            call(meta.float())
        with pytest.raises(TypeError):
            call(meta[0])
    with pytest.raises(ValueError, match="the model on cpu"):
        gen.predictor.set_image(meta)
    assert not gen.predictor.is_image_set
    # the two ops themselves: no CPU fallback, and the same dtype / rank rule
    with pytest.raises(pp._lib.PopeHipError):
        pp.resize_u8_batch(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (8, 8))
    with pytest.raises(pp._lib.PopeHipError):
        pp.sam_preprocess_batch(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 1024, [0.0] * 3, [1.0] * 3)


def test_frame_query_checks_device_frames_before_any_work():
    from pope_amd.driver import locate_pose_from_frames
    sam, _ = small_sam(depth=1)
    gen = sg.SamAutomaticMaskGenerator(sam, points_per_side=2)
    lin = torch.nn.Linear(1, 1)
    refs = np.zeros((2, 8, 8, 3), np.uint8)
    meta = torch.empty(48, 64, 3, dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match="all host arrays or all device tensors"):
        locate_pose_from_frames(gen, lin, lin, refs, [np.zeros((48, 64, 3), np.uint8), meta], np.eye(3), np.eye(3))
    with pytest.raises(TypeError):
        locate_pose_from_frames(gen, lin, lin, refs, torch.empty(2, 48, 64, 3, device="meta"), np.eye(3), np.eye(3))
    with pytest.raises(ValueError, match="2 references, 3 frames"):
        locate_pose_from_frames(gen, lin, lin, refs, torch.empty(3, 48, 64, 3, dtype=torch.uint8, device="meta"), np.eye(3), np.eye(3))
