"""Times Q queries asked of ONE frame on one GPU, in one process, WALL time (host work included: a device synchronisation before
the clock starts and one before it stops), for Q = 1, 4, 8 references on a 480 x 640 frame:
 (a) `driver.locate_pose_from_frames(..., SharedFrames([frame], [0] * Q), ...)`, the frame given once (what `locate_poses_in_frame` calls):
     the mask generator, the crops and their DINOv2 forward run once, the vote, the 3 Q Matcher pairs and the pose per query;
 (b) the same queries as they had to be asked before: the frame repeated Q times.
Models and settings are those of scripts/frame_query_time.py: SAM ViT-B (`build_sam_vit_b`) under the synthetic weights of
scripts/sam_generator_time.py, 16 x 16 points, IoU and stability filters off (all 768 masks of a frame reach NMS), box NMS 0.35,
`min_mask_region_area=250`; DINOv2 ViT-S/14 and the LoFTR Matcher under the peaked synthetic weights of
scripts/driver_batch_time.py.  Before any timing it checks that (a) returns what (b) returns, bit for bit.  After the warm-up
calls of both, (a) and (b) alternate within each repetition, so that drift of the box hits both alike.

--repeated-only times form (b) alone, with calls that exist before `frame_index` did, and writes its times to --json: run on the
parent commit it gives the yardstick, whose run-to-run spread (max - min over the repetitions of all its runs) is what the
differences are compared with.  --parent FILE [FILE ...] reads such files (one per process; their repetitions are pooled) and adds
their column and the three verdicts to the table; --alone FILE [FILE ...] reads the same kind of run made on THIS commit, so that
condition 1 compares like with like (form (b) alone in its own process on both commits; without it, form (b) of the alternating
run stands in):
 1. form (b) now stays within the parent's spread of form (b) on the parent;
 2. at Q = 1 the two forms lie within that spread of each other;
 3. at Q >= 4 form (a) is not slower than form (b) beyond that spread.
It also times, at the largest Q, `propose_batch` of the one frame and the shared driver step on its boxes alone: (a) should take
about their sum.  Writes the table to --out (default profiles/shared_frame.md); --append adds a further run's section.
usage: python scripts/shared_frame_time.py [--queries 1 4 8] [--reps 7] [--warmup 2] [--box-nms-thresh 0.35] [--parent FILE ...]
                                           [--alone FILE ...] [--repeated-only --json FILE] [--out FILE] [--append]"""
import argparse
import json
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


def wall_alternating(fns, reps, warmup):
    """Wall ms of every function of `fns`, alternating within each repetition: one list of `reps` times per function."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, out in zip(fns, times):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
    return times


def pooled(files, thresh):
    """The --json files of --repeated-only runs -> {Q: all their times}, and how they were made."""
    ms, made = {}, []
    for name in files:
        with open(name) as f:
            doc = json.load(f)
        assert doc["box_nms_thresh"] == thresh, f"{name} was run at another NMS threshold"
        made.append(f"{doc['reps']} repetitions after {doc['warmup']} warm-ups")
        for Q, t in doc["ms"].items():
            ms.setdefault(Q, []).extend(t)
    return ms, f"{len(files)} process{'es' if len(files) > 1 else ''}, {' / '.join(sorted(set(made)))} each"


def cell(t):
    return f"{statistics.median(t):.2f} ({min(t):.2f} .. {max(t):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--box-nms-thresh", type=float, default=0.35)
    ap.add_argument("--repeated-only", action="store_true", help="time form (b) alone (runs on the commit before frame_index)")
    ap.add_argument("--json", default=None, help="write the raw times here")
    ap.add_argument("--parent", nargs="+", default=None, help="the --json files of --repeated-only runs on the parent commit")
    ap.add_argument("--alone", nargs="+", default=None, help="the --json files of --repeated-only runs on this commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_frame.md"))
    ap.add_argument("--append", action="store_true", help="add this run's section to --out (a run at other thresholds)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    H, W, Qmax = 480, 640, max(a.queries)
    sam = synthetic_vit_b(dev)
    vit, matcher = models(dev)
    kw = dict(pred_iou_thresh=0.0, stability_score_thresh=0.0, box_nms_thresh=a.box_nms_thresh, min_mask_region_area=250)
    gen = sg.SamAutomaticMaskGenerator(sam, output_mode="binary_mask", **kw)
    frame = (torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8).numpy()
    cases = [synth.synthetic_frame_case(seed=31 + q) for q in range(Qmax)]
    refs, K0, K1 = np.stack([c[0] for c in cases]), np.stack([c[3] for c in cases]), cases[0][4]

    def shared(Q):
        from pope_amd.driver import SharedFrames          # not on the parent commit, where only --repeated-only runs
        return locate_pose_from_frames(gen, vit, matcher, refs[:Q], SharedFrames([frame], [0] * Q), K0[:Q], K1)

    def repeated(Q):
        return locate_pose_from_frames(gen, vit, matcher, refs[:Q], [frame] * Q, K0[:Q], K1)

    if a.repeated_only:
        times = {}
        for Q in a.queries:
            (tb,) = wall_alternating([lambda: repeated(Q)], a.reps, a.warmup)
            times[str(Q)] = tb
            print(f"Q = {Q}: (b) {cell(tb)} ms", flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump({"form": "b", "reps": a.reps, "warmup": a.warmup, "box_nms_thresh": a.box_nms_thresh, "ms": times}, f)
            print("wrote", a.json)
        return

    parent, parent_made = pooled(a.parent, a.box_nms_thresh) if a.parent else (None, "not given")
    alone, alone_made = pooled(a.alone, a.box_nms_thresh) if a.alone else ({}, "not given")
    got, want = shared(Qmax), repeated(Qmax)
    diffs = {q: same(g, w) + ([] if np.array_equal(g["proposals"], w["proposals"]) else ["proposals"]) for q, (g, w) in enumerate(zip(got, want))}
    diffs = {q: d for q, d in diffs.items() if d}
    P = len(got[0]["proposals"])
    head = [f"the shared call at Q = {Qmax} equals the repeated-frame call bit for bit: {not diffs}" + (f"  differing: {diffs}" if diffs else ""),
            f"proposals of the frame: {P}   ({sum(w['pose'] is not None for w in want)} of {Qmax} queries yield a pose)"]
    print("\n".join(head), flush=True)
    rows, raw, failed = [], {}, []
    for Q in a.queries:
        ta, tb = wall_alternating([lambda: shared(Q), lambda: repeated(Q)], a.reps, a.warmup)
        raw[str(Q)] = {"a": ta, "b": tb}
        ma, mb = statistics.median(ta), statistics.median(tb)
        own = max(max(ta) - min(ta), max(tb) - min(tb))
        if parent and str(Q) in parent:
            tp, tn = parent[str(Q)], alone.get(str(Q))
            mp, spread = statistics.median(tp), max(tp) - min(tp)
            mn = statistics.median(tn) if tn else mb              # condition 1: like with like where (b) alone was run here too
            checks = [("1", abs(mn - mp) <= spread)]
            checks.append(("2", abs(ma - mb) <= spread) if Q == 1 else ("3", ma - mb <= spread))
            failed += [f"condition {n} at Q = {Q}" for n, ok in checks if not ok]
            tail = (f"{cell(tn) if tn else 'not measured'} | {cell(tp)} | {spread:.2f} | {mn - mp:+.2f} | "
                    + ", ".join(f"{n}: {'met' if ok else 'NOT MET'}" for n, ok in checks))
        else:
            tail = "not measured | not measured | - | - | -"
        rows.append(f"| {Q} | {cell(ta)} | {cell(tb)} | {mb - ma:+.2f} | {mb / ma:.2f} | {own:.2f} | {tail} |")
        print(rows[-1], flush=True)
    # what (a) is made of, at the largest Q: the generator over the one frame, and the shared driver step on its boxes
    boxes = gen.propose_batch([frame])
    tg, td = wall_alternating([lambda: gen.propose_batch([frame]),
                               lambda: locate_match_pose_batch_u8(vit, matcher, refs, frame[None], boxes, K0, K1, frame_index=[0] * Qmax)],
                              a.reps, a.warmup)
    parts = statistics.median(tg) + statistics.median(td)
    ma = statistics.median(raw[str(Qmax)]["a"])
    sum_line = (f"At Q = {Qmax}: `propose_batch` of the one frame alone {cell(tg)} ms, the shared driver step on its boxes alone {cell(td)} ms; "
                f"their medians sum to {parts:.2f} ms, form (a) takes {ma:.2f} ms ({ma - parts:+.2f} ms).")
    print(sum_line)
    if not parent:
        verdict = "No parent run was given (--parent): the three conditions are not judged here."
    elif failed:
        verdict = "NOT MET: " + "; ".join(failed) + "."
    else:
        verdict = ("All three conditions are met: form (b) is where it was on the parent, the two forms agree at Q = 1, and form (a) is not "
                   "slower than form (b) at any Q >= 4, each within the parent's run-to-run spread.")
    print(verdict)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"reps": a.reps, "warmup": a.warmup, "box_nms_thresh": a.box_nms_thresh, "ms": raw, "propose": tg, "step": td}, f)
    argv, words = [], iter(sys.argv[1:])
    for v in words:
        if v in ("--out", "--json"):                   # file names are not part of the recorded command
            next(words, None)
        elif v in ("--parent", "--alone"):
            argv.append(v + " <its times>")
        elif not v.endswith(".json"):
            argv.append(v)
    title = f"## A further run: box NMS {a.box_nms_thresh}, Q = {a.queries}" if a.append else \
        "# Queries that share a frame: `frame_index` against the frame repeated per query"
    text = f"""{title}

`python scripts/shared_frame_time.py{"".join(" " + v for v in argv)}` on one MI355X, one process: WALL time in ms,
host work included, a device synchronisation before the clock starts and one before it stops; {a.warmup} warm-up calls of each form, then
{a.reps} repetitions in which the forms alternate; median (min .. max).  One 480 x 640 frame asked about Q references; SAM ViT-B under
synthetic weights, 16 x 16 points, IoU and stability filters off (768 masks of a frame reach NMS), box NMS {a.box_nms_thresh},
`min_mask_region_area=250`; DINOv2 ViT-S/14 and the LoFTR Matcher under the peaked synthetic weights.

(a) `locate_pose_from_frames(..., SharedFrames([frame], [0] * Q), ...)`: the frame given once; generator, crops and their DINOv2 forward once.
(b) `locate_pose_from_frames` with the frame repeated Q times, as the call had to be made before.
(b) alone: `--repeated-only` runs, form (b) by itself in a process of its own, on this commit ({alone_made}) and on the parent
commit ({parent_made}), the processes of the two commits taking turns.  The parent's spread (max - min over all its repetitions) is
the yardstick of the three conditions: 1. (b) alone now within it of (b) alone on the parent (without a run alone on this commit,
(b) of the alternating run stands in); 2. at Q = 1, (a) and (b) within it of each other; 3. at Q >= 4, (a) not slower than (b)
beyond it.

{head[0]}
{head[1]}

| Q | (a) shared, ms | (b) repeated, ms | (b) - (a), ms | (b) / (a) | spread of this run (largest max - min), ms | (b) alone now, ms | (b) alone on the parent, ms | parent's spread, ms | (b) now - (b) parent, ms | conditions |
|---|---|---|---|---|---|---|---|---|---|---|
""" + "\n".join(rows) + f"""

{verdict}

{sum_line}
Form (b) pays the generator once per query (the encoder, the decoder over 768 prompts, both NMS passes and the clean-up of one
frame each), form (a) once per call; what grows with Q in form (a) is the driver step alone: Q reference rows in the DINOv2
forward, the vote, 3 Q Matcher pairs, Q pose problems.
"""
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + text)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
