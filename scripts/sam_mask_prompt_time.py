"""Time SAM mask prompts on one GPU: `python scripts/sam_mask_prompt_time.py [iters]`.  One JSON line each:
  - the mask embedding (`pope_sam_mask_embed_f32` through `PromptEncoder.forward`) at P = 1, 16 and 64, next to the same chain
    run by torch on the same card (F.conv2d / LayerNorm2d / F.gelu, the restatement of tests/test_sam_mask_prompt_cpu.py: what
    keeping `mask_downscaling` in torch would cost) and to the traffic floor (256 KiB read + 4 MiB written per prompt);
  - a decoder call at P = 64 with mask prompts (a dense embedding per prompt: layer 0's image projections per prompt) against
    the same prompts without one (the broadcast: layer 0 once per image), in f16x3.
Times are device events around `reps` back-to-back calls (a window of several ms), median and minimum over `iters` windows."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pope_amd import synth  # noqa: E402
from test_sam_decoder_cpu import build_models  # noqa: E402
from test_sam_mask_prompt_cpu import restate_embed  # noqa: E402

FLOOR_BYTES = 256 * 256 * 4 + 256 * 64 * 64 * 4   # per prompt: the mask read once, the embedding written once
PEAK_BYTES_PER_S = 8e12                            # MI355X HBM3E


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = "cuda:0"
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    pe, md = build_models(sd)
    pe, md = pe.to(dev), md.to(dev)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    all_masks = synth.sam_mask_prompt_case(64, 3).to(dev)
    for P in (1, 16, 64):
        masks = all_masks[:P].contiguous()
        reps = max(4, 256 // P)
        with torch.no_grad():
            got, ref = pe(points=None, boxes=None, masks=masks)[1], restate_embed(sdd, masks)
            assert float((got - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
            med, best = timed(lambda: pe(points=None, boxes=None, masks=masks), iters, reps)
            tmed, tbest = timed(lambda: restate_embed(sdd, masks), iters, reps)
        floor_us = P * FLOOR_BYTES / PEAK_BYTES_PER_S * 1e6
        print(json.dumps({"what": "mask embedding", "P": P, "pope_us_median": round(med * 1e3, 2), "pope_us_min": round(best * 1e3, 2),
                          "torch_us_median": round(tmed * 1e3, 2), "torch_us_min": round(tbest * 1e3, 2),
                          "floor_us_at_8TBps": round(floor_us, 2), "pope_TBps": round(P * FLOOR_BYTES / (med * 1e-3) / 1e12, 3)}))
    P = 64
    (coords, labels), _, _ = synth.sam_decoder_case("grid")
    coords, labels = coords[:P].to(dev), labels[:P].to(dev)
    image = synth.synthetic_sam_image_embedding(seed=1).to(dev)
    image_pe = pe.get_dense_pe()
    sparse, dense_mask = pe(points=(coords, labels), boxes=None, masks=all_masks)
    _, dense_none = pe(points=(coords, labels), boxes=None, masks=None)
    for what, dense in (("decoder, mask prompts (layer 0 per prompt)", dense_mask), ("decoder, no mask (layer 0 per image)", dense_none)):
        med, best = timed(lambda: md(image, image_pe, sparse, dense, True), iters, 2)
        print(json.dumps({"what": what, "P": P, "ms_median": round(med, 3), "ms_min": round(best, 3)}))


if __name__ == "__main__":
    main()
