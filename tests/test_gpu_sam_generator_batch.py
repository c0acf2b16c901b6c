"""`SamAutomaticMaskGenerator.generate_batch` on the MI355X: the records of frame q are, key by key and bit for bit, those of
`generate(frames[q])`, in both output modes (`generate` itself is pinned to the CPU reference by
tests/test_gpu_sam_generator.py::test_generate_end_to_end).  Every comparison is an equality."""
import numpy as np
import pytest
import torch

from pope_amd import sam_amg, synth
from pope_amd import sam_generator as sg
from test_sam_generator_cpu import NMS, OFFSET, PRED_IOU, STABILITY, THRESHOLD, small_sam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the thresholds of tests/test_gpu_sam_generator.py::test_generate_end_to_end (its comment says where they come from)
E2E = dict(points_per_side=8, pred_iou_thresh=0.1, stability_score_thresh=0.02, box_nms_thresh=0.9, min_mask_region_area=250)
# (seed, gain) of the three frames.  With the synthetic weights the masks that pass the filters cover one another by more than
# the NMS threshold, so a frame yields one record; a frame at a quarter of the brightness yields none (the CPU reference path of
# the end-to-end test gives 1, 0, 1 for these three and 1 for seeds 5 to 9 at full brightness).
FRAMES = ((5, 1.0), (6, 0.25), (7, 1.0))
KEYS = ["segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"]


def blocky_frame(seed, gain=1.0, H=480, W=640, cell=16):
    """A seeded frame of `cell` x `cell` blocks of one colour each, values in [0, 255 * gain] (the end-to-end test's frame is
    seed 5 at gain 1)."""
    g = torch.Generator().manual_seed(seed)
    small = (torch.rand(H // cell, W // cell, 3, generator=g) * (255 * gain)).to(torch.uint8).numpy()
    return np.ascontiguousarray(np.repeat(np.repeat(small, cell, axis=0), cell, axis=1)[:H, :W])


@pytest.fixture(scope="module")
def sam():
    model, sd = small_sam(depth=2)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


@pytest.fixture(scope="module")
def frames():
    return [blocky_frame(s, g) for s, g in FRAMES]


MODES = ["binary_mask", "uncompressed_rle"]


@pytest.fixture(scope="module")
def runs(sam, frames):
    """output mode -> (generate() per frame, generate_batch of all frames), computed once."""
    out = {}
    for mode in MODES:
        gen = sg.SamAutomaticMaskGenerator(sam, output_mode=mode, **E2E)
        out[mode] = ([gen.generate(f) for f in frames], gen.generate_batch(frames))
    return out


def assert_same_records(got, want, mode):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a) == KEYS and list(b) == KEYS
        if mode == "binary_mask":
            assert a["segmentation"].dtype == bool and a["segmentation"].shape == b["segmentation"].shape
            assert np.array_equal(a["segmentation"], b["segmentation"])
        else:
            assert a["segmentation"] == b["segmentation"]
        for k in KEYS[1:]:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_generate_frame_by_frame(runs, mode):
    single, batch = runs[mode]
    counts = [len(r) for r in single]
    print(f"mode {mode}: records per frame {counts}, batch {[len(r) for r in batch]}")
    assert len(batch) == len(single) == len(FRAMES)
    assert max(counts) >= 1 and len(set(counts)) > 1                  # the frames differ, and something passes
    for got, want in zip(batch, single):
        assert_same_records(got, want, mode)
    for recs in single:                                               # area comes from the device: it is the mask's own
        for r in recs:
            seg = r["segmentation"]
            assert r["area"] == (int(seg.sum()) if mode == "binary_mask" else sam_amg.area_from_rle(seg))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("min_area", [250, 0])
def test_tail_of_several_segments_equals_the_tail_of_each(sam, mode, min_area):
    """The frames above leave one record each; here the tail gets segments with several survivors: the filtered masks of the
    `frame` fixture case at the fork's thresholds, cut into three frames' worth with an empty one in the middle."""
    low, iou, input_size, hw = synth.sam_generator_case("frame")
    d = sg.process_low_res(low.to(DEV), iou.to(DEV), input_size, hw, PRED_IOU, STABILITY, THRESHOLD, OFFSET)
    data = {k: d[k] for k in ("index", "iou_preds", "stability_score", "boxes", "area", "packed")}
    n = data["index"].numel()
    seg = [0, 9, 9, n]
    assert n >= 16
    gen = sg.SamAutomaticMaskGenerator(sam, box_nms_thresh=NMS, min_mask_region_area=min_area, output_mode=mode)
    points = np.repeat(gen.point_grids[0] * np.array([[hw[1], hw[0]]]), 3, axis=0)
    points = np.concatenate([points] * (low.shape[0] // len(points) + 1))
    got = gen._finish(data, seg, points, hw)
    want = [gen._finish({k: v[lo:hi] for k, v in data.items()}, [0, hi - lo], points, hw)[0] for lo, hi in zip(seg[:-1], seg[1:])]
    print(f"mode {mode}, min_area {min_area}: masks {n}, records per segment {[len(r) for r in got]}")
    assert len(got) == 3 and got[1] == [] and len(got[0]) >= 2 and len(got[2]) >= 2
    for g, w in zip(got, want):
        assert_same_records(g, w, mode)


@pytest.mark.parametrize("mode", MODES)
def test_batch_of_one_frame(runs, sam, frames, mode):
    single, _ = runs[mode]
    gen = sg.SamAutomaticMaskGenerator(sam, output_mode=mode, **E2E)
    got = gen.generate_batch(frames[1:2])
    assert len(got) == 1
    assert_same_records(got[0], single[1], mode)


def test_batched_calls_leave_the_predictor_reset(runs, sam, frames):
    """The batched front end takes each frame's features as an argument: the predictor holds no image afterwards, and a
    `generate` after it is that of a generator which ran nothing before."""
    gen = sg.SamAutomaticMaskGenerator(sam, **E2E)
    gen.propose_batch(frames[:1])
    assert gen.predictor.is_image_set is False and gen.predictor.features is None
    assert_same_records(gen.generate(frames[0]), runs["binary_mask"][0][0], "binary_mask")


def test_rle_from_packed_equals_the_cpu_definition(runs):
    single, _ = runs["binary_mask"]
    masks = np.stack([r["segmentation"] for recs in single for r in recs])
    packed = torch.as_tensor(sam_amg.pack_masks(masks).view(np.int32), device=DEV)
    assert sg.rle_from_packed(packed, masks.shape[2]) == [sam_amg.mask_to_rle(m) for m in masks]


@pytest.mark.parametrize("output_mode", MODES)
def test_nothing_passes_gives_empty_lists(sam, frames, output_mode):
    gen = sg.SamAutomaticMaskGenerator(sam, output_mode=output_mode, **dict(E2E, pred_iou_thresh=10.0))
    assert gen.generate_batch(frames) == [[], [], []]
    assert gen.generate(frames[0]) == []
    assert gen.generate_batch([]) == []


def test_mixed_sizes_are_refused(sam, frames):
    gen = sg.SamAutomaticMaskGenerator(sam, **E2E)
    with pytest.raises(ValueError):
        gen.generate_batch([frames[0], np.zeros((333, 332, 3), np.uint8)])
