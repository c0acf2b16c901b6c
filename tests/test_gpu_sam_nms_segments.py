"""`box_nms_segments` (pope_sam_nms_segments_f32) on the MI355X: greedy box NMS of several independent segments in one launch,
against `box_nms` per segment (the same device function) and against the CPU definition `sam_amg.nms`.  Kept lists are
integers: every comparison is an equality."""
import numpy as np
import pytest
import torch

from pope_amd import sam_amg, synth
from pope_amd import sam_generator as sg
from test_sam_generator_cpu import NMS, OFFSET, PRED_IOU, STABILITY, THRESHOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HAND_BOXES = [[0, 0, 10, 10], [0, 0, 10, 10], [1, 1, 11, 11], [20, 20, 30, 30], [0, 0, 0, 0], [0, 0, 0, 0]]
HAND_SCORES = [0.5, 0.5, 0.9, 0.1, 0.7, 0.7]


@pytest.fixture(scope="module")
def frame_boxes():
    """Boxes and IoU predictions of the `frame` case after the IoU and the stability filter (what the generator's NMS sees)."""
    low, iou, input_size, original_size = synth.sam_generator_case("frame")
    d = sg.process_low_res(low.to(DEV), iou.to(DEV), input_size, original_size, PRED_IOU, STABILITY, THRESHOLD, OFFSET)
    return d["boxes"].to(torch.float32).contiguous(), d["iou_preds"].contiguous()


def kept_lists(keep, counts, seg):
    keep, counts = keep.cpu().numpy(), counts.cpu().numpy()
    return [keep[seg[s]:seg[s] + counts[s]].tolist() for s in range(len(seg) - 1)]


def check_against_both(boxes, scores, seg, thr):
    keep, counts = sg.box_nms_segments(boxes, scores, seg, thr)
    assert keep.dtype == torch.int32 and counts.dtype == torch.int32 and keep.shape == (boxes.shape[0],) and counts.shape == (len(seg) - 1,)
    got = kept_lists(keep, counts, seg)
    b, s = boxes.cpu().numpy(), scores.cpu().numpy()
    for i, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        single = (sg.box_nms(boxes[lo:hi], scores[lo:hi], thr) + lo).cpu().tolist()
        cpu = (sam_amg.nms(b[lo:hi], s[lo:hi], thr) + lo).tolist()
        assert got[i] == single == cpu, i
    return got


def test_three_segments_and_an_empty_one(frame_boxes):
    boxes, scores = frame_boxes
    n = boxes.shape[0]
    assert n >= 16
    seg = [0, n // 3, n // 3, 2 * n // 3 + 1, n]                     # segment 1 is empty
    got = check_against_both(boxes, scores, seg, NMS)
    print("boxes", n, "segments", seg, "kept", [len(g) for g in got])
    assert got[1] == [] and all(len(got[i]) >= 1 for i in (0, 2, 3))
    assert any(len(g) < hi - lo for g, lo, hi in zip(got, seg[:-1], seg[1:]))          # something is suppressed


def test_hand_case_with_ties_and_empty_boxes_in_the_middle(frame_boxes):
    boxes, scores = frame_boxes
    hand_b = torch.tensor(HAND_BOXES, dtype=torch.float32, device=DEV)
    hand_s = torch.tensor(HAND_SCORES, device=DEV)
    all_b = torch.cat([boxes[:7], hand_b, boxes[7:12]])
    all_s = torch.cat([scores[:7], hand_s, scores[7:12]])
    seg = [0, 7, 13, 18]
    for thr, want in ((0.35, [2, 4, 5, 3]), (0.7, [2, 4, 5, 0, 3])):
        got = check_against_both(all_b, all_s, seg, thr)
        assert got[1] == [7 + i for i in want]                          # global indices, ties in index order


def test_one_segment_equals_box_nms(frame_boxes):
    boxes, scores = frame_boxes
    n = boxes.shape[0]
    got = check_against_both(boxes, scores, [0, n], NMS)
    assert got[0] == sg.box_nms(boxes, scores, NMS).cpu().tolist()
    keep, counts = sg.box_nms_segments(boxes[:0], scores[:0], [0], NMS)                # no segment at all
    assert keep.numel() == 0 and counts.numel() == 0
    keep, counts = sg.box_nms_segments(boxes[:0], scores[:0], [0, 0, 0], NMS)          # only empty segments
    assert counts.cpu().tolist() == [0, 0]


def test_a_segment_of_2049_boxes_is_refused():
    n = sg.NMS_MAX + 1
    boxes, scores = torch.zeros(n + 3, 4, device=DEV), torch.zeros(n + 3, device=DEV)
    with pytest.raises(ValueError):
        sg.box_nms_segments(boxes, scores, [0, 3, n + 3], 0.35)
    with pytest.raises(ValueError):
        sg.box_nms_segments(boxes, scores, [0, 5, 3, n + 3], 0.35)                     # not non-decreasing
    with pytest.raises(ValueError):
        sg.box_nms_segments(boxes, scores, [0, 3], 0.35)                               # does not end at n
    keep, counts = sg.box_nms_segments(boxes, scores, [0, 3, sg.NMS_MAX + 3, n + 3], 0.35)   # 2048 is fine
    assert counts.cpu().tolist()[1] >= 1
