"""Times the SAM generator's post-processing on one GPU, in one process, with events after a warm-up:
 (1) the fused HIP pass + filters + NMS for the generator's call (M = 768 masks at 480 x 640, IoU filter off: all 768 processed);
 (2) a torch restatement of the reference's path on the same card and inputs (`Sam.postprocess_masks`, then
     `_process_batch`'s tail: stability score, binarisation, boxes, the transposed diff + nonzero of `mask_to_rle_pytorch`;
     the per-mask Python loop that turns change indices into count lists is host work and is left out of both);
 (3) `generate()` of one frame split into encoder / decoder / post-processing (synthetic ViT-B weights, filters off, so the
     whole batch reaches NMS; min_mask_region_area=0).
With --min-mask-region-area N > 0 additionally, 3 warm-up calls and the median of 10 each:
 (4) the small-region clean-up stage alone (`postprocess_small_regions_segments` with one segment: clean-up and second NMS;
     the survivors stay packed, where the single-frame function these rows timed before also unpacked them) on the NMS
     survivors of `synth.sam_generator_case("frame")`;
 (5) the same stage on 64 random-blob masks of 480 x 640 (a box-blurred noise field cut at a quantile);
 (6) `generate()` of one 480 x 640 frame with `min_mask_region_area=N` (filters off, as in (3)).
With --frames Q[,Q..] only the following, as WALL time (host work included, a device synchronisation before the clock starts
and one at the end; one warm-up, median of 5), synthetic ViT-B weights, 480 x 640 frames, filters off, box NMS 0.35,
`min_mask_region_area=250`, in both output modes:
 (7) Q sequential `generate()` calls against `generate_batch` of the same Q frames (`--sequential-only`: the first alone, which
     is what a commit without `generate_batch` can run);
 (8) the tail alone (`_finish`: NMS through records) on one frame's filtered masks.
Prints medians, minima and the bytes/s of (1) against its floor: the low-res logits read once plus the packed masks written.
usage: python scripts/sam_generator_time.py [--reps 20] [--skip-generate] [--skip-postprocess] [--min-mask-region-area 250]
       python scripts/sam_generator_time.py --frames 1,4,8 [--sequential-only]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pope_amd import sam_amg, synth  # noqa: E402
from pope_amd import sam_generator as sg  # noqa: E402


def timed(fn, reps, warmup=3):
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
    return statistics.median(out), min(out), max(out)


def mask_boxes(masks):
    """`batched_mask_to_box` of bool [n, H, W] in torch on its device: int32 [n, 4] (the reference's path, row (2))."""
    n, H, W = masks.shape
    rows, cols = masks.any(2), masks.any(1)
    ar_h, ar_w = torch.arange(H, device=masks.device), torch.arange(W, device=masks.device)
    y1 = (rows * ar_h).max(1).values
    y0 = (rows * ar_h + H * (~rows)).min(1).values
    x1 = (cols * ar_w).max(1).values
    x0 = (cols * ar_w + W * (~cols)).min(1).values
    empty = (x1 < x0) | (y1 < y0)
    return (torch.stack([x0, y0, x1, y1], 1) * (~empty)[:, None]).to(torch.int32)


def reference_tail(low, input_size, hw, thr=0.0, off=1.0):
    masks = F.interpolate(low[:, None], (1024, 1024), mode="bilinear", align_corners=False)
    masks = masks[..., :input_size[0], :input_size[1]]
    masks = F.interpolate(masks, hw, mode="bilinear", align_corners=False)[:, 0]
    inter = (masks > (thr + off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    union = (masks > (thr - off)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    stability = inter / union
    m = masks > thr
    boxes = mask_boxes(m)
    t = m.permute(0, 2, 1).flatten(1)
    change = (t[:, 1:] ^ t[:, :-1]).nonzero()
    return stability, boxes, change


def box_blur(f, k):
    """Box filter of odd width k along both axes of [H, W] (edges replicated)."""
    r = k // 2
    for ax in (0, 1):
        p = np.concatenate([np.repeat(np.take(f, [0], ax), r + 1, ax), f, np.repeat(np.take(f, [-1], ax), r, ax)], ax)
        c = np.cumsum(p, ax, dtype=np.float64)
        n = f.shape[ax]
        f = (np.take(c, range(k, k + n), ax) - np.take(c, range(0, n), ax)) / k
    return f


def blob_masks(n, H, W, seed=11):
    rng = np.random.default_rng(seed)
    out = np.empty((n, H, W), bool)
    for i in range(n):
        k = (41, 61, 81)[i % 3]
        f = box_blur(box_blur(rng.standard_normal((H, W)), k), k)
        out[i] = f > np.quantile(f, (0.5, 0.8, 0.3, 0.9)[i % 4])
    return out


def time_cleanup(dev, min_area):
    """Rows (4) and (5): `postprocess_small_regions_segments` alone on one segment, device events around the call."""
    low, iou, input_size, hw = synth.sam_generator_case("frame")
    d = sg.process_low_res(low.to(dev), iou.to(dev), input_size, hw, 0.9, 0.95, 0.0, 1.0)
    keep = sg.box_nms(d["boxes"], d["iou_preds"], 0.35)
    frame = {k: d[k][keep].contiguous() for k in ("index", "boxes", "packed")}
    blobs = torch.as_tensor(sam_amg.pack_masks(blob_masks(64, *hw)).view(np.int32), device=dev)
    blob = {"index": torch.arange(64, device=dev), "boxes": mask_boxes(sg.unpack_on_device(blobs, hw[1])), "packed": blobs}
    for name, data in (("(4) clean-up stage, frame survivors", frame), ("(5) clean-up stage, 64 random blobs", blob)):
        seg = [0, data["index"].numel()]
        masks = sg.unpack_on_device(sg.postprocess_small_regions_segments(data, seg, hw[1], min_area, 0.35)[0]["packed"], hw[1])
        med, lo, hi = timed(lambda: sg.postprocess_small_regions_segments(data, seg, hw[1], min_area, 0.35), 10, 3)
        print(f"{name:40s} n = {data['index'].numel():3d} -> {masks.shape[0]:3d} kept, {int(masks.sum())} pixels set   "
              f"median {med:.3f} ms  min {lo:.3f}  max {hi:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--skip-postprocess", action="store_true", help="leave out (1) and (2)")
    ap.add_argument("--min-mask-region-area", type=int, default=0, help="> 0: time the small-region clean-up, rows (4) to (6)")
    ap.add_argument("--frames", default="", help="Q[,Q..]: rows (7) and (8) only, wall time of Q frames")
    ap.add_argument("--sequential-only", action="store_true", help="with --frames: generate() calls only, no generate_batch")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = "cuda:0"
    if a.frames:
        time_frames(dev, [int(q) for q in a.frames.split(",")], a.sequential_only)
        return
    M, (H, W) = 768, (480, 640)
    if a.min_mask_region_area > 0:
        time_cleanup(dev, a.min_mask_region_area)
    if not a.skip_postprocess:
        time_postprocess(dev, a.reps, M, H, W)
    if not a.skip_generate:
        time_generate(dev, H, W, a.min_mask_region_area)


def time_postprocess(dev, reps, M, H, W):
    low, iou, input_size, hw = synth.sam_generator_case("frame", M=M)
    low, iou = low.to(dev), iou.to(dev)
    floor = M * 256 * 256 * 4 + M * H * sam_amg.row_words(W) * 4

    def fused_kernel():
        return sg.postprocess_batch(low, None, input_size, hw, 0.0, 1.0)

    def fused_stage():
        d = sg.process_low_res(low, iou, input_size, hw, 0.0, 0.95, 0.0, 1.0)
        return sg.box_nms(d["boxes"], d["iou_preds"], 0.35)

    stats, _, _ = fused_kernel()
    st_ref, boxes_ref, _ = reference_tail(low, input_size, hw)
    same = bool(torch.equal(stats[:, 3:7], boxes_ref)) and bool(torch.equal(torch.nan_to_num(stats[:, 7].view(torch.float32), -1),
                                                                            torch.nan_to_num(st_ref, -1)))
    print(f"boxes and stability scores of the fused pass equal the torch path on this GPU: {same}")
    k_med, k_min, k_max = timed(fused_kernel, reps)
    s_med, s_min, s_max = timed(fused_stage, reps)
    r_med, r_min, r_max = timed(lambda: reference_tail(low, input_size, hw), max(5, reps // 2))
    print(f"(1) fused kernels only      median {k_med:.3f} ms  min {k_min:.3f}  max {k_max:.3f}   "
          f"{floor / k_med / 1e6:.1f} GB/s of the {floor / 1e6:.1f} MB floor (min: {floor / k_min / 1e6:.1f} GB/s)")
    print(f"(1) fused + filters + NMS   median {s_med:.3f} ms  min {s_min:.3f}  max {s_max:.3f}")
    print(f"(2) torch reference path    median {r_med:.3f} ms  min {r_min:.3f}  max {r_max:.3f}   ratio (2)/(1) = {r_med / s_med:.1f}")


def synthetic_vit_b(dev):
    sam = sg.build_sam_vit_b()
    sd = {"image_encoder." + k: v for k, v in synth.synthetic_sam_encoder_state_dict(seed=0, dim=768, depth=12, heads=12,
                                                                                      global_idx=(2, 5, 8, 11)).items()}
    sd.update(synth.synthetic_sam_decoder_state_dict(seed=0))
    sam.load_state_dict(sd, strict=True)
    return sam.to(dev)


def wall(fn, reps=5, warmup=1):
    """Wall-clock ms of fn(), host work included: synchronised before the clock starts and before it stops."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def time_frames(dev, qs, sequential_only, H=480, W=640, min_area=250):
    """Rows (7) and (8)."""
    sam = synthetic_vit_b(dev)
    frames = [(torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5 + q)) * 255).to(torch.uint8).numpy()
              for q in range(max(qs))]
    for mode in ("uncompressed_rle", "binary_mask"):
        gen = sg.SamAutomaticMaskGenerator(sam, pred_iou_thresh=0.0, stability_score_thresh=0.0, min_mask_region_area=min_area,
                                           output_mode=mode)
        print(f"{mode}: records per frame {[len(gen.generate(f)) for f in frames]}")
        for q in qs:
            seq = wall(lambda: [gen.generate(f) for f in frames[:q]])
            line = f"(7) {mode:16s} Q = {q}: {q} x generate() median {seq[0]:.2f} ms  min {seq[1]:.2f}"
            if not sequential_only:
                bat = wall(lambda: gen.generate_batch(frames[:q]))
                line += f"   generate_batch median {bat[0]:.2f} ms  min {bat[1]:.2f}   sequential / batch = {seq[0] / bat[0]:.2f}"
            print(line)
        # the tail alone, on the filtered masks of one frame
        gen.predictor.set_image(frames[0])
        pr = gen.predictor
        points = gen.point_grids[0] * np.array([[W, H]])
        low, iou = gen._decode(pr.features, points, (H, W))
        d = sg.process_low_res(low, iou, pr.input_size, (H, W), 0.0, 0.0, 0.0, 1.0)
        data = {k: d[k] for k in ("index", "iou_preds", "stability_score", "boxes", "area", "packed")}
        pts = np.repeat(points, 3, axis=0)
        gen.predictor.reset_image()
        if hasattr(gen, "generate_batch"):
            tail = wall(lambda: gen._finish(data, [0, data["index"].numel()], pts, (H, W)))
        else:
            tail = wall(lambda: gen._finish(data, pts, (H, W)))
        print(f"(8) {mode:16s} tail of one frame, {data['index'].numel()} masks in: median {tail[0]:.2f} ms  min {tail[1]:.2f}")


def time_generate(dev, H, W, min_area):
    hw = (H, W)
    sam = synthetic_vit_b(dev)
    gen = sg.SamAutomaticMaskGenerator(sam, pred_iou_thresh=0.0, stability_score_thresh=0.0, min_mask_region_area=0)
    frame = (torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8).numpy()
    pr = gen.predictor
    points = gen.point_grids[0] * np.array([[W, H]])
    pr.set_image(frame)
    lo, io = gen._decode(pr.features, points, (H, W))
    q = torch.quantile(io, torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], device=dev)).cpu().numpy().round(3)
    d = sg.process_low_res(lo, io, pr.input_size, hw, 0.0, 0.0)
    sq = np.nanquantile(d["stability_score"].cpu().numpy(), [0, 0.25, 0.5, 0.75, 1]).round(3)
    print(f"synthetic ViT-B: iou_preds quantiles {q.tolist()}, stability quantiles {sq.tolist()}")
    e = timed(lambda: pr.set_image(frame), 5, 1)
    c = timed(lambda: gen._decode(pr.features, points, (H, W)), 5, 1)

    def post():
        d = sg.process_low_res(lo, io, pr.input_size, hw, 0.0, 0.0)
        return sg.box_nms(d["boxes"], d["iou_preds"], 0.35)
    p = timed(post, 5, 1)
    for name, t in (("encoder (set_image, host resize included)", e), ("decoder (256 prompts x 3)", c), ("post-processing", p)):
        print(f"(3) {name:44s} median {t[0]:.3f} ms  min {t[1]:.3f}")
    if min_area > 0:
        full = sg.SamAutomaticMaskGenerator(sam, pred_iou_thresh=0.0, stability_score_thresh=0.0, min_mask_region_area=min_area)
        off = timed(lambda: gen.generate(frame), 10, 3)
        t0 = time.perf_counter()
        full.generate(frame)                                   # ends in a device-to-host copy
        reps, warm = (10, 3) if time.perf_counter() - t0 < 2.0 else (3, 1)      # a call of seconds: fewer of them
        on = timed(lambda: full.generate(frame), reps, warm)
        print(f"(6) {warm} warm-up, {reps} timed calls")
        print(f"(6) generate(), min_mask_region_area=0: {len(gen.generate(frame))} records   median {off[0]:.3f} ms  min {off[1]:.3f}")
        print(f"(6) generate(), min_mask_region_area={min_area}: {len(full.generate(frame))} records   median {on[0]:.3f} ms  min {on[1]:.3f}")


if __name__ == "__main__":
    main()
