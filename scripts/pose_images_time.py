"""Times the image-conditioned pose head inside the query on one GPU, in one process, for Q = 1, 8, 24 queries (480 x 640 frames,
8 proposals each, `synth.synthetic_frame_case`; DINOv2 ViT-S/14 and the LoFTR Matcher under the peaked synthetic weights of
scripts/driver_batch_time.py; MoCoPE with num_sample S = 500 under `synth.mocope_state_dict`, its backbone the small trunk
`synth.MOCOPE_TRUNK` unless --trunk names a `convnextv2` factory):
 (k) `preprocess.pose_images` alone (event time): Q crops of 256 x 256 gathered by a device index -> [Q, 3, 224, 224];
 (a) `locate_match_pose_batch_u8` without a regressor;
 (b) the same call with `pose_regressor=MoCoPE`: the image pair made on the device, nothing downloaded in between;
 (c) the same result the way it had to be made before: call (a), then per query crop the downloaded best proposal, download the
     crop, resize it and the reference with the host twin `resize_linear_cv_u8`, upload both, and ONE `regress_pose_fused_batch`
     over the re-uploaded best-slot matches;
 (d) call (b) with a `ReferenceSet` encoded with the regressor (reference images and their backbone logits kept).
(a) .. (d) are WALL times (a device synchronisation before the clock starts and one before it stops), alternating within each
repetition after the warm-up calls.  Before any timing it checks that (b), (c) and (d) give the same `pose_regressed`, bit for
bit.  Writes the table to --out (default profiles/pose_images.md).
usage: python scripts/pose_images_time.py [--queries 1 8 24] [--num-sample 500] [--reps 7] [--warmup 2] [--trunk NAME] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pope_amd import convnextv2, synth  # noqa: E402
from pope_amd.crops import crop_proposals  # noqa: E402
from pope_amd.driver import encode_references, locate_match_pose_batch_u8  # noqa: E402
from pope_amd.mocope import MoCoPE, regress_pose_fused_batch  # noqa: E402
from pope_amd.preprocess import pose_images, resize_linear_cv_u8  # noqa: E402
from driver_batch_time import models  # noqa: E402
from shared_frame_time import cell, wall_alternating  # noqa: E402

SIZE = 224


def build_mocope(S, trunk, dev):
    sd = synth.mocope_state_dict(S, "6d")
    if trunk is None:
        backbone = convnextv2.ConvNeXtV2(**synth.MOCOPE_TRUNK)
    else:
        backbone = convnextv2.FACTORIES[trunk](num_classes=1000)
        sd = {k: v for k, v in sd.items() if not k.startswith("convnextv2.model.")}
        sd.update({"convnextv2.model." + k: v for k, v in
                   synth.convnext_state_dict(list(backbone.depths), list(backbone.dims), 1000).items()})
    model = MoCoPE(S, "6d", backbone=backbone)
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8, 24])
    ap.add_argument("--num-sample", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trunk", default=None, help="a convnextv2.FACTORIES name (default: the small trunk of the tests)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_images.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    S, Qmax = a.num_sample, max(a.queries)
    vit, matcher = models(dev)
    model = build_mocope(S, a.trunk, dev)
    cases = [synth.synthetic_frame_case(seed=31 + q) for q in range(Qmax)]
    refs, frames = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    boxes, K0, K1 = [c[2] for c in cases], np.stack([c[3] for c in cases]), cases[0][4]
    seed = 9

    def plain(Q):
        return locate_match_pose_batch_u8(vit, matcher, refs[:Q], frames[:Q], boxes[:Q], K0[:Q], K1)

    def in_call(Q):
        return locate_match_pose_batch_u8(vit, matcher, refs[:Q], frames[:Q], boxes[:Q], K0[:Q], K1, pose_regressor=model, regressor_seed=seed)

    def round_trip(Q):
        outs = plain(Q)
        img0, img1 = [], []
        for q, out in enumerate(outs):
            best = out["best_proposal"]
            if best < 0:
                img0.append(np.zeros((SIZE, SIZE, 3), np.uint8))
                img1.append(img0[-1])
                continue
            crop = crop_proposals(torch.from_numpy(frames[q]).to(dev), boxes[q][best:best + 1], K1)["crops"][0].cpu().numpy()
            img0.append(resize_linear_cv_u8(refs[q], SIZE, SIZE))
            img1.append(resize_linear_cv_u8(crop, SIZE, SIZE))
        up = lambda v: torch.from_numpy(np.stack(v)).to(dev).float().permute(0, 3, 2, 1).contiguous()  # noqa: E731
        counts = [len(o["mkpts0"][o["best_slot"]]) for o in outs]
        k0 = torch.from_numpy(np.concatenate([o["mkpts0"][o["best_slot"]] for o in outs])).to(dev)
        k1 = torch.from_numpy(np.concatenate([o["mkpts1"][o["best_slot"]] for o in outs])).to(dev)
        reg = regress_pose_fused_batch(model, k0, k1, counts, up(img0), up(img1), seed=seed)
        R, t, ok = reg["R"].cpu().numpy(), reg["t"].cpu().numpy(), reg["status"].cpu().numpy() == 0
        for q, out in enumerate(outs):
            out["pose_regressed"] = (R[q], t[q]) if out["best_proposal"] >= 0 and counts[q] >= 5 and ok[q] else None
        return outs

    refset = encode_references(vit, matcher, refs, pose_regressor=model)

    def with_set(Q):
        return locate_match_pose_batch_u8(vit, matcher, refset, frames[:Q], boxes[:Q], K0[:Q], K1, ref_index=list(range(Q)),
                                          pose_regressor=model, regressor_seed=seed)

    def regressed_equal(x, y):
        return all((g["pose_regressed"] is None) == (w["pose_regressed"] is None) and
                   (w["pose_regressed"] is None or all(np.array_equal(u, v) for u, v in zip(g["pose_regressed"], w["pose_regressed"])))
                   for g, w in zip(x, y))

    b, c, d = in_call(Qmax), round_trip(Qmax), with_set(Qmax)
    n_reg = sum(o["pose_regressed"] is not None for o in b)
    head = [f"`pose_regressed` of (b) equals (c) bit for bit at Q = {Qmax}: {regressed_equal(b, c)}; (d) equals (b): {regressed_equal(d, b)}",
            f"{n_reg} of {Qmax} queries are regressed; best-slot matches per query: "
            f"{sorted(len(o['mkpts0'][o['best_slot']]) for o in b)}"]
    print("\n".join(head), flush=True)

    crops = torch.cat([crop_proposals(torch.from_numpy(frames[q]).to(dev), boxes[q], K1)["crops"] for q in range(Qmax)], 0)
    rows_md = []
    for Q in a.queries:
        idx = torch.arange(Q, device=dev, dtype=torch.int64) * int(crops.shape[0] // Qmax)
        tk = event_ms(lambda: pose_images(crops, idx, SIZE), 20, 3)
        ta, tb, tc, td = wall_alternating([lambda: plain(Q), lambda: in_call(Q), lambda: round_trip(Q), lambda: with_set(Q)], a.reps, a.warmup)
        line = (f"| {Q} | {statistics.median(tk) * 1e3:.1f} | {cell(ta)} | {cell(tb)} | {cell(tc)} | {cell(td)} | "
                f"{statistics.median(tc) - statistics.median(tb):+.2f} |")
        print(line, flush=True)
        rows_md.append(line)

    trunk = a.trunk or "the small trunk of the tests (synth.MOCOPE_TRUNK: depths 1-1-2-1, dims 64-80-160-320)"
    doc = ["# The image-conditioned pose head inside the query", "",
           f"`python scripts/pose_images_time.py --queries {' '.join(map(str, a.queries))} --num-sample {S} --reps {a.reps} --warmup {a.warmup}`"
           + (f" --trunk {a.trunk}" if a.trunk else ""),
           f"on {torch.cuda.get_device_name(0)}, one process.  MoCoPE S = {S}, backbone: {trunk}; images {SIZE} x {SIZE}.", "",
           *head, "",
           "(k) `pose_images` alone, event time, median of 20; (a) the query without a regressor; (b) with `pose_regressor=MoCoPE`; "
           "(c) the host round trip after (a); (d) as (b) with a `ReferenceSet` that carries `pose_feat0`.  (a) .. (d): wall ms, median "
           f"(min .. max) of {a.reps} alternating repetitions after {a.warmup} warm-ups.", "",
           "| Q | (k) us | (a) ms | (b) ms | (c) ms | (d) ms | (c) - (b) ms |", "|---|---|---|---|---|---|---|", *rows_md, "",
           "Reading: (k) is the whole op as the query calls it (the index is clamped and narrowed to int32 by two small torch "
           "launches, then the one kernel launch), so it is launch-bound at these Q.  (b) - (a) is what the head costs inside the "
           "query, (c) - (b) what the host round trip adds on top of it.  (d) takes the whole reference side from the set, the "
           "DINOv2 tokens and the Matcher's encoding as well as the head's images and logits, so it can undercut (a), which is "
           "handed raw references.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(doc))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
