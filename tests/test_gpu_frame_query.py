"""The frame-to-pose query on the MI355X: `SamAutomaticMaskGenerator.propose` / `propose_batch` return the `bbox` values of the
records of `generate` / `generate_batch`, and `driver.locate_pose_from_frames` returns what `locate_match_pose_batch_u8` returns
when it is handed those boxes by hand, key by key and bit for bit.  Every comparison is an equality."""
import numpy as np
import pytest
import torch

from pope_amd import synth
from pope_amd import sam_generator as sg
from test_gpu_sam_generator_batch import E2E, FRAMES, blocky_frame
from test_sam_generator_cpu import NMS, OFFSET, PRED_IOU, STABILITY, THRESHOLD, small_sam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# The thresholds of the generator's end-to-end test with the box NMS threshold raised to 1: under the synthetic weights the boxes
# of the masks that pass the filters cover one another by more than 0.995, so every threshold from 0.9 to 0.995 leaves the one
# record per frame of that test, which gives the vote nothing to choose from; at 1.0 no IoU exceeds the threshold and every mask
# that passes the filters is a proposal.  Records per frame (seed 5, seed 6 at gain 0.25, seed 7) on the first run on the card:
# 37, 0, 30 with `min_mask_region_area` 250 and with 0 (and 1, 0, 1 at 0.9, 0.93, 0.95, 0.97, 0.98, 0.99 and 0.995).
NMS_RAISED = 1.0
MIN_AREAS = (250, 0)


def generator(sam, min_area=250, **kw):
    return sg.SamAutomaticMaskGenerator(sam, **dict(E2E, box_nms_thresh=NMS_RAISED, min_mask_region_area=min_area, **kw))


@pytest.fixture(scope="module")
def sam():
    model, sd = small_sam(depth=2)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


@pytest.fixture(scope="module")
def frames():
    return [blocky_frame(s, g) for s, g in FRAMES]


@pytest.fixture(scope="module")
def records(sam, frames):
    """min_mask_region_area -> generate_batch(frames), computed once."""
    return {m: generator(sam, m).generate_batch(frames) for m in MIN_AREAS}


def boxes_of(recs):
    return [[r["bbox"] for r in frame] for frame in recs]


@pytest.fixture(scope="module")
def models(sd0, golden_dir):
    """DINOv2 ViT-S/14 and the Matcher under the peaked synthetic weights, as tests/test_gpu_driver_batch.py builds them."""
    import os
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd.matcher import Matcher, default_cfg
    fx = np.load(os.path.join(golden_dir, "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    matcher = Matcher(default_cfg).eval()
    matcher.load_state_dict(sd, strict=True)
    return load_dinov2_model(state_dict=sd0).to(DEV), matcher.to(DEV)


@pytest.fixture(scope="module")
def query():
    """(refs [3, 256, 256, 3] uint8, K0 [3, 3, 3], K1 [3, 3]): one reference crop and camera per frame."""
    cases = [synth.synthetic_frame_case(seed=31 + q) for q in range(len(FRAMES))]
    return np.stack([c[0] for c in cases]), np.stack([c[3] for c in cases]), cases[0][4]


@pytest.fixture(scope="module")
def two_calls(sam, frames, records, models, query):
    """Today's way, once: the boxes of `generate_batch`'s records handed to `locate_match_pose_batch_u8`."""
    from pope_amd.driver import locate_match_pose_batch_u8
    refs, K0, K1 = query
    boxes = boxes_of(records[250])
    return boxes, locate_match_pose_batch_u8(*models, refs, frames, boxes, K0, K1)


def assert_same_value(got, want, tag):
    assert type(got) is type(want), tag
    if isinstance(want, torch.Tensor):
        assert got.dtype == want.dtype and got.device == want.device and torch.equal(got, want), tag
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), tag
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), tag
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same_value(g, w, (tag, i))
    else:
        assert got == want, tag          # ints, and None for None


def assert_same_result(got, want, boxes, tag):
    """One query's dict of the frame-level call against the two-call form's dict and boxes."""
    assert set(got) == set(want) | {"proposals"}, tag
    for k in want:
        assert_same_value(got[k], want[k], (tag, k))
    assert (got["pose"] is None) == (want["pose"] is None) and (want["pose"] is None or len(got["pose"]) == 3), tag
    p = got["proposals"]
    assert isinstance(p, np.ndarray) and p.dtype == np.int64 and p.shape == (len(boxes), 4) and p.tolist() == [list(b) for b in boxes], tag


# ---- 1. the proposals-only tail ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", MIN_AREAS)
def test_propose_batch_equals_the_bboxes_of_generate_batch(sam, frames, records, min_area):
    want = boxes_of(records[min_area])
    counts = [len(b) for b in want]
    print(f"min_mask_region_area {min_area}: records per frame {counts}")
    assert max(counts) >= 4 and min(counts) == 0            # a frame the vote can choose in, and a frame without a proposal
    gen = generator(sam, min_area)
    got = gen.propose_batch(frames)
    assert len(got) == len(frames)
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == np.int64 and g.shape == (len(w), 4) and g.tolist() == w
    rle = generator(sam, min_area, output_mode="uncompressed_rle").propose_batch(frames)      # whatever the output mode
    assert all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(rle, got))
    for f in frames:
        one, recs = gen.propose(f), gen.generate(f)
        assert one.dtype == np.int64 and one.shape == (len(recs), 4) and one.tolist() == [r["bbox"] for r in recs]


def test_propose_batch_of_nothing_and_of_mixed_sizes(sam, frames):
    gen = generator(sam)
    assert gen.propose_batch([]) == []
    with pytest.raises(ValueError):
        gen.propose_batch([frames[0], np.zeros((333, 332, 3), np.uint8)])
    none = generator(sam, pred_iou_thresh=10.0).propose_batch(frames[:2])                     # nothing passes the first filter
    assert [a.shape for a in none] == [(0, 4), (0, 4)] and all(a.dtype == np.int64 for a in none)


@pytest.mark.parametrize("min_area", MIN_AREAS)
def test_box_tail_of_several_segments_equals_the_boxes_of_the_record_tail(sam, min_area):
    """Segments with several survivors each and an empty one between them, as
    tests/test_gpu_sam_generator_batch.py::test_tail_of_several_segments_equals_the_tail_of_each feeds `_finish`: the filtered
    masks of the `frame` fixture case at the fork's thresholds."""
    low, iou, input_size, hw = synth.sam_generator_case("frame")
    d = sg.process_low_res(low.to(DEV), iou.to(DEV), input_size, hw, PRED_IOU, STABILITY, THRESHOLD, OFFSET)
    data = {k: d[k] for k in ("index", "iou_preds", "stability_score", "boxes", "area", "packed")}
    n = data["index"].numel()
    seg = [0, 9, 9, n]
    assert n >= 16
    gen = sg.SamAutomaticMaskGenerator(sam, box_nms_thresh=NMS, min_mask_region_area=min_area)
    points = np.repeat(gen.point_grids[0] * np.array([[hw[1], hw[0]]]), 3, axis=0)
    points = np.concatenate([points] * (low.shape[0] // len(points) + 1))
    want = boxes_of(gen._finish(data, seg, points, hw))
    got = gen._finish_boxes(data, seg, hw)
    print(f"min_area {min_area}: masks {n}, boxes per segment {[len(b) for b in got]}")
    assert len(got) == 3 and len(want[0]) >= 2 and want[1] == [] and len(want[2]) >= 2
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.shape == (len(w), 4) and g.tolist() == w


# ---- 2. the frame-level driver entry -----------------------------------------------------------------------------------
def test_frames_call_equals_generate_batch_then_the_batched_driver(sam, frames, models, query, two_calls):
    from pope_amd.driver import locate_pose_from_frames
    refs, K0, K1 = query
    boxes, want = two_calls
    got = locate_pose_from_frames(generator(sam), *models, refs, frames, K0, K1)
    print(f"proposals per query {[len(b) for b in boxes]}, best proposal {[w['best_proposal'] for w in want]}, "
          f"pose found {[w['pose'] is not None for w in want]}")
    assert len(got) == len(want) == len(frames)
    for q in range(len(frames)):
        assert_same_result(got[q], want[q], boxes[q], f"query {q}")
    # frames as one array and as a tensor are the same call
    for form in (np.stack(frames), torch.from_numpy(np.stack(frames))):
        again = locate_pose_from_frames(generator(sam), *models, refs, form, K0, K1)
        assert_same_result(again[0], want[0], boxes[0], "query 0, stacked frames")


def test_one_query_form(sam, frames, models, query):
    from pope_amd.driver import locate_pose_from_frame, locate_pose_from_frames
    refs, K0, K1 = query
    gen = generator(sam)
    one = locate_pose_from_frame(gen, *models, refs[0], frames[0], K0[0], K1)
    batch = locate_pose_from_frames(gen, *models, refs[:1], frames[:1], K0[:1], K1)
    assert isinstance(one, dict) and len(batch) == 1
    assert_same_result(one, batch[0], batch[0]["proposals"].tolist(), "one query")
    assert np.array_equal(one["proposals"], batch[0]["proposals"])


def test_frame_without_proposals_leaves_its_neighbours_alone(sam, frames, models, query, two_calls):
    from pope_amd.driver import locate_pose_from_frames
    refs, K0, K1 = query
    boxes, want = two_calls
    gen = generator(sam)
    empty = [q for q, b in enumerate(boxes) if not b]
    rest = [q for q, b in enumerate(boxes) if b]
    assert empty and rest
    got = locate_pose_from_frames(gen, *models, refs, frames, K0, K1)
    for q in empty:
        out = got[q]
        assert out["best_proposal"] == -1 and out["pose"] is None and out["pre_bbox"] is None and out["pre_K"] is None
        assert out["proposals"].shape == (0, 4) and out["proposals"].dtype == np.int64 and out["scores"].shape == (0,)
        assert list(out["slot_index"]) == [-1, -1, -1] and list(out["matching_score"]) == [0, 0, 0]
    without = locate_pose_from_frames(gen, *models, refs[rest], [frames[q] for q in rest], K0[rest], K1)
    for q, out in zip(rest, without):
        assert_same_result(out, want[q], boxes[q], f"query {q} without the empty frame")
        assert_same_result(got[q], out, boxes[q], f"query {q} next to the empty frame")


def test_max_proposals_keeps_the_first_boxes_in_record_order(sam, frames, models, query, two_calls):
    from pope_amd.driver import locate_match_pose_batch_u8, locate_pose_from_frames
    refs, K0, K1 = query
    boxes, _ = two_calls
    cut = [b[:2] for b in boxes]
    assert any(len(b) > 2 for b in boxes)
    want = locate_match_pose_batch_u8(*models, refs, frames, cut, K0, K1)
    got = locate_pose_from_frames(generator(sam), *models, refs, frames, K0, K1, max_proposals=2)
    for q in range(len(frames)):
        assert_same_result(got[q], want[q], cut[q], f"query {q}, two proposals")


def test_models_on_two_devices_are_refused(frames, models, query):
    from pope_amd.driver import locate_pose_from_frames
    refs, K0, K1 = query
    on_cpu = sg.SamAutomaticMaskGenerator(small_sam(depth=2)[0], **E2E)
    with pytest.raises(ValueError):
        locate_pose_from_frames(on_cpu, *models, refs, frames, K0, K1)
