"""Times the frame-to-pose query on one GPU, in one process, WALL time (host work included: a device synchronisation before the
clock starts and one before it stops), for Q = 1, 4, 8 queries on 480 x 640 frames:
 (a) ONE call of `driver.locate_pose_from_frames` (the generator's proposals-only tail, `propose_batch`, feeds the batched
     driver step), against
 (b) the same work in two calls: `generate_batch(frames)` in `binary_mask` mode, `bbox` taken from the records, then
     `locate_match_pose_batch_u8`.
Both run the same encoder, decoder, NMS, clean-up, DINOv2, Matcher and pose kernels on the same inputs; (a) leaves out the mask
unpack, its download and the record loop.  SAM ViT-B (`build_sam_vit_b`) under the synthetic weights of
scripts/sam_generator_time.py, 16 x 16 points, IoU and stability filters off as there (all 768 masks of a frame reach NMS), box
NMS 0.35, `min_mask_region_area=250`; DINOv2 ViT-S/14 and the LoFTR Matcher under the peaked synthetic weights of
scripts/driver_batch_time.py.  Before any timing it checks that (a) returns what (b) returns, bit for bit.  After the warm-up
calls of both, (a) and (b) alternate within each repetition, so that drift of the box hits both alike; the spread of each
(max - min over the repetitions) is reported next to the medians, and the verdict compares the difference of the medians with it.
Writes the table to --out (default profiles/frame_query.md); --append adds a further run's section to it, such as one at
`--box-nms-thresh 1.0`, where nothing is suppressed and all 768 masks of a frame are proposals (the synthetic weights leave one
survivor per frame at 0.35).  --cuda-frames hands both forms the frames as one uint8 CUDA tensor, so that SAM's input
transform runs on the device (`pope_sam_preprocess_u8_f32`) instead of Pillow and an upload.
usage: python scripts/frame_query_time.py [--queries 1 4 8] [--reps 7] [--warmup 2] [--box-nms-thresh 0.35] [--out FILE] [--append]
                                          [--cuda-frames]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pope_amd import synth  # noqa: E402
from pope_amd import sam_generator as sg  # noqa: E402
from pope_amd.driver import locate_match_pose_batch_u8, locate_pose_from_frames  # noqa: E402
from driver_batch_time import models, same  # noqa: E402
from sam_generator_time import synthetic_vit_b  # noqa: E402


def wall_pair(fa, fb, reps, warmup):
    """Wall ms of fa() and fb(), alternating: two lists of `reps` times."""
    for _ in range(warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, out in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--box-nms-thresh", type=float, default=0.35)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_query.md"))
    ap.add_argument("--append", action="store_true", help="add this run's section to --out (a run at other thresholds)")
    ap.add_argument("--cuda-frames", action="store_true", help="hand both forms the frames as one uint8 CUDA tensor (no Pillow, no upload)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    H, W, Qmax = 480, 640, max(a.queries)
    sam = synthetic_vit_b(dev)
    vit, matcher = models(dev)
    kw = dict(pred_iou_thresh=0.0, stability_score_thresh=0.0, box_nms_thresh=a.box_nms_thresh, min_mask_region_area=250)
    gen = sg.SamAutomaticMaskGenerator(sam, output_mode="binary_mask", **kw)
    frames = [(torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5 + q)) * 255).to(torch.uint8).numpy() for q in range(Qmax)]
    if a.cuda_frames:
        frames = torch.from_numpy(np.stack(frames)).to(dev)
    cases = [synth.synthetic_frame_case(seed=31 + q) for q in range(Qmax)]
    refs, K0, K1 = np.stack([c[0] for c in cases]), np.stack([c[3] for c in cases]), cases[0][4]

    def one_call(Q):
        return locate_pose_from_frames(gen, vit, matcher, refs[:Q], frames[:Q], K0[:Q], K1)

    def record_boxes(Q):
        return [[r["bbox"] for r in recs] for recs in gen.generate_batch(frames[:Q])]

    def two_calls(Q):
        return locate_match_pose_batch_u8(vit, matcher, refs[:Q], frames[:Q], record_boxes(Q), K0[:Q], K1)

    got, want, boxes = one_call(Qmax), two_calls(Qmax), record_boxes(Qmax)
    counts = [len(g["proposals"]) for g in got]
    diffs = {q: same(g, w) for q, (g, w) in enumerate(zip(got, want)) if same(g, w)}
    diffs.update({q: ["proposals"] for q, (g, b) in enumerate(zip(got, boxes)) if q not in diffs and g["proposals"].tolist() != b})
    equal = not diffs
    head = [f"one call at Q = {Qmax} equals the two-call form bit for bit: {equal}" + (f"  differing: {diffs}" if diffs else ""),
            f"proposals per frame: {counts}   ({sum(w['pose'] is not None for w in want)} of {Qmax} queries yield a pose)"]
    print("\n".join(head), flush=True)
    rows, slower = [], []
    for Q in a.queries:
        ta, tb = wall_pair(lambda: one_call(Q), lambda: two_calls(Q), a.reps, a.warmup)
        ma, mb = statistics.median(ta), statistics.median(tb)
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        rows.append(f"| {Q} | {sum(counts[:Q])} | {sum(counts[:Q]) * H * W / 1e6:.2f} | {ma:.2f} ({min(ta):.2f} .. {max(ta):.2f}) | {mb:.2f} ({min(tb):.2f} .. {max(tb):.2f}) | "
                    f"{mb - ma:+.2f} | {spread:.2f} | {mb / ma:.3f} |")
        print(rows[-1], flush=True)
        if ma - mb > spread:
            slower.append(Q)
    verdict = ("The one-call form is not slower than the two-call form at any Q beyond the run-to-run spread." if not slower else
               f"SLOWER: at Q = {slower} the one-call form's median exceeds the two-call form's by more than the spread.")
    print(verdict)
    argv = [v for i, v in enumerate(sys.argv[1:]) if v != "--out" and (i == 0 or sys.argv[i] != "--out")]
    where = "  The frames are one uint8 CUDA tensor: SAM's input transform runs on the device in both forms." if a.cuda_frames else ""
    title = f"## A further run: box NMS {a.box_nms_thresh}, Q = {a.queries}{', frames on the device' if a.cuda_frames else ''}" if a.append else \
        "# Frame-to-pose query: one call against `generate_batch` + `locate_match_pose_batch_u8`"
    text = f"""{title}

`python scripts/frame_query_time.py{"".join(" " + v for v in argv)}` on one MI355X, one process: WALL time in ms, host work
included, a device synchronisation before the clock starts and one before it stops; {a.warmup} warm-up calls of each form, then
{a.reps} repetitions in which the two forms alternate; median (min .. max).  480 x 640 frames; SAM ViT-B under synthetic weights,
16 x 16 points, IoU and stability filters off (768 masks of a frame reach NMS), box NMS {a.box_nms_thresh},
`min_mask_region_area=250`; DINOv2 ViT-S/14 and the LoFTR Matcher under the peaked synthetic weights.{where}

(a) `locate_pose_from_frames`: `propose_batch` (boxes only) feeds the batched driver step.
(b) `generate_batch` in `binary_mask` mode, `bbox` from the records, then `locate_match_pose_batch_u8`.

{head[0]}
{head[1]}

| Q | proposals | bool masks (b) downloads, MB | (a) one call, ms | (b) two calls, ms | (b) - (a), ms | spread (largest max - min), ms | (b) / (a) |
|---|---|---|---|---|---|---|---|
""" + "\n".join(rows) + f"""

{verdict}

Both forms launch the same kernels up to the second NMS; what (a) leaves out is the unpacking of the survivors' masks to bool
[n, {H}, {W}], their download (third column) and the per-record host loop.  The difference is therefore set by the number of
survivors, not by Q: compare it with the spread before reading anything into it.
"""
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + text)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
