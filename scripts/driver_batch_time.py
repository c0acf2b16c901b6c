"""Times the batched driver step against the single-query loop on one GPU, in one process, wall clock around a synchronise
after a warm-up: for Q in 1, 2, 4, 8, 16
 (a) Q calls of `locate_match_pose_u8`, one query each (the per-query loop of the drivers), and
 (b) ONE call of `locate_match_pose_batch_u8` over the same Q queries
(`synth.synthetic_frame_case`, seeds 31 .. 31 + Q - 1, 8 proposals each, DINOv2 ViT-S/14 + the LoFTR Matcher under the peaked
synthetic weights).  Before any timing it checks that (b) returns what (a) returns, bit for bit, and prints the verdict.
With --stages it also times the stages of (b) alone with events (DINOv2 forward, vote kernel, Matcher, tally, pose).
usage: python scripts/driver_batch_time.py [--reps 10] [--warmup 3] [--queries 1 2 4 8 16] [--stages] [--only-batch Q]
(--only-batch Q runs nothing but warmed-up batched calls at Q: the process to put under a kernel trace)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import synth  # noqa: E402
from pope_amd.driver import locate_match_pose_batch_u8, locate_match_pose_u8  # noqa: E402


def models(dev):
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd.matcher import Matcher, default_cfg
    fx = np.load(os.path.join(ROOT, "tests", "golden", "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    matcher = Matcher(default_cfg).eval()
    matcher.load_state_dict(sd, strict=True)
    return load_dinov2_model(state_dict=synth.synthetic_state_dict(seed=0)).to(dev), matcher.to(dev)


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def same(got, want):
    """One query's batched result against its single-query result; returns the list of keys that differ."""
    bad = [k for k in ("slot_index", "slot_scores", "matching_score", "boxes", "K_crops", "pre_bbox", "pre_K")
           if not np.array_equal(got[k], want[k])]
    bad += [k for k in ("best_slot", "best_proposal") if got[k] != want[k]]
    if not torch.equal(got["scores"], want["scores"]):
        bad.append("scores")
    bad += [f"{k}[{s}]" for k in ("mkpts0", "mkpts1", "mconf") for s in range(3) if not np.array_equal(got[k][s], want[k][s])]
    if (got["pose"] is None) != (want["pose"] is None):
        bad.append("pose is None")
    elif want["pose"] is not None:
        bad += [f"pose.{n}" for n, g, w in zip(("R", "t", "inliers"), got["pose"], want["pose"]) if not np.array_equal(g, w)]
    return bad


def stage_times(vit, matcher, dev, cases, reps, warmup):
    """Event times of the stages of one batched call, each stage run alone on the inputs the call would hand it."""
    from pope_amd import ops
    from pope_amd.crops import crop_proposals
    from pope_amd.dinov2_utils import get_cls_token_torch
    from pope_amd.pose import estimate_pose_batch
    from pope_amd.preprocess import gray_batch, set_torch_images
    Q = len(cases)
    refs = torch.from_numpy(np.stack([c[0] for c in cases])).to(dev)
    props = [crop_proposals(torch.from_numpy(c[1]).to(dev), c[2], c[4]) for c in cases]
    crops = torch.cat([p["crops"] for p in props], 0)
    counts = [len(c[2]) for c in cases]
    x = torch.cat([set_torch_images(refs, center_crop=True), set_torch_images(crops, center_crop=True)], 0)
    cls = get_cls_token_torch(vit, x)
    vote = ops.vote_top3_batch(cls[:Q], cls[Q:], counts)
    g1 = gray_batch(crops.index_select(0, vote["pair_row"]))
    batch = {"image0": gray_batch(refs).repeat_interleave(3, dim=0), "image1": g1}
    matcher(batch)
    args = (batch["m_bids"], batch["mconf"], batch["mkpts0_f"], batch["mkpts1_f"], vote["pair_live"])
    tally = ops.slot_tally(*args)
    Kc = torch.from_numpy(np.concatenate([p["K"] for p in props], 0)).to(dev)
    K1 = Kc.index_select(0, vote["pair_row"].view(Q, 3).gather(1, tally["best_slot"].long()[:, None])[:, 0])
    K0 = np.stack([c[3] for c in cases])

    def ev(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return statistics.median(out)

    return {"vit": ev(lambda: get_cls_token_torch(vit, x)), "vote": ev(lambda: ops.vote_top3_batch(cls[:Q], cls[Q:], counts)),
            "matcher": ev(lambda: matcher({"image0": batch["image0"], "image1": g1})), "tally": ev(lambda: ops.slot_tally(*args)),
            "pose": ev(lambda: estimate_pose_batch(tally["best_kpts0"], tally["best_kpts1"], tally["best_count"], K0, K1, 0.5, 0.99)),
            "matches": int(batch["m_bids"].numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--only-batch", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    vit, matcher = models(dev)
    cases = [synth.synthetic_frame_case(seed=31 + q) for q in range(max(a.queries + [a.only_batch]))]

    def batched(Q):
        c = cases[:Q]
        return locate_match_pose_batch_u8(vit, matcher, np.stack([x[0] for x in c]), np.stack([x[1] for x in c]), [x[2] for x in c],
                                          np.stack([x[3] for x in c]), np.stack([x[4] for x in c]))

    if a.only_batch:
        for _ in range(a.warmup + a.reps):
            batched(a.only_batch)
        torch.cuda.synchronize()
        print(f"{a.warmup + a.reps} batched calls at Q = {a.only_batch}")
        return

    def singles(Q):
        return [locate_match_pose_u8(vit, matcher, *c) for c in cases[:Q]]

    Qmax = max(a.queries)
    want, got = singles(Qmax), batched(Qmax)
    diffs = {q: same(g, w) for q, (g, w) in enumerate(zip(got, want)) if same(g, w)}
    poses = sum(w["pose"] is not None for w in want)
    print(f"batched call at Q = {Qmax} equals {Qmax} single-query calls bit for bit: {not diffs}"
          + (f"  differing: {diffs}" if diffs else "") + f"   ({poses} of {Qmax} queries yield a pose)")
    print(f"{'Q':>3} {'single loop ms':>15} {'batched ms':>11} {'speed-up':>9} {'single q/s':>11} {'batched q/s':>12}")
    for Q in a.queries:
        s_med, _ = wall_ms(lambda: singles(Q), a.reps, a.warmup)
        b_med, _ = wall_ms(lambda: batched(Q), a.reps, a.warmup)
        print(f"{Q:3d} {s_med:15.3f} {b_med:11.3f} {s_med / b_med:9.2f} {1e3 * Q / s_med:11.1f} {1e3 * Q / b_med:12.1f}")
    if a.stages:
        for Q in a.queries:
            st = stage_times(vit, matcher, dev, cases[:Q], a.reps, a.warmup)
            print(f"stages at Q = {Q:2d} (events, ms): ViT {st['vit']:.3f}  vote {st['vote']:.4f}  Matcher {st['matcher']:.3f}  "
                  f"tally {st['tally']:.4f}  pose {st['pose']:.3f}   ({st['matches']} matches)")


if __name__ == "__main__":
    main()
