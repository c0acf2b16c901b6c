"""Time `Sam.forward` on one GPU against the per-image loop it replaces (`SamPredictor.set_torch_image` + `predict_torch` per
record): `python scripts/sam_forward_time.py [reps]`.  SAM ViT-B under synthetic weights, N = 1, 4, 8 images of 480 x 640
(768 x 1024 in the input frame) with 1, 2 and 16 box prompts each, `multimask_output=True`.  Per shape: two warm-up calls of
each form, then `reps` (7) alternating repetitions; wall time (host clock around a device synchronisation) as median
(min .. max).  The decoder's share is timed separately with device events on the same embeddings: one
`MaskDecoder.forward_images` call against the loop of `MaskDecoder.forward` calls.  One JSON line per shape."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import synth  # noqa: E402
from pope_amd.sam_generator import SamPredictor, build_sam_vit_b  # noqa: E402

DEV = "cuda:0"


def build():
    sam = build_sam_vit_b()
    sd = {"image_encoder." + k: v for k, v in synth.synthetic_sam_encoder_state_dict(seed=0, dim=768, depth=12, heads=12,
                                                                                      global_idx=(2, 5, 8, 11)).items()}
    sd.update(synth.synthetic_sam_decoder_state_dict(seed=0))
    sam.load_state_dict(sd, strict=True)
    return sam.to(DEV).eval()


def batch(N, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(N):
        lo = torch.rand(B, 2, generator=g) * torch.tensor([600.0, 400.0])
        out.append({"image": (torch.rand(3, 768, 1024, generator=g) * 255).to(DEV), "original_size": (480, 640),
                    "boxes": torch.cat([lo, lo + 100 + torch.rand(B, 2, generator=g) * 250], dim=1).to(DEV)})
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(one, loop, clock, reps):
    for _ in range(2):
        one()
        loop()
    t1, tl = [], []
    for _ in range(reps):
        t1.append(clock(one))
        tl.append(clock(loop))
    return t1, tl


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    sam = build()
    pr = SamPredictor(sam)
    md, pe = sam.mask_decoder, sam.prompt_encoder
    with torch.no_grad():
        for N in (1, 4, 8):
            for B in (1, 2, 16):
                recs = batch(N, B)

                def one():
                    return sam(recs, multimask_output=True)

                def loop():
                    out = []
                    for x in recs:
                        pr.set_torch_image(x["image"][None], x["original_size"])
                        out.append(pr.predict_torch(None, None, x["boxes"], None, True))
                    return out
                got, want = one(), loop()
                same = all(torch.equal(o["masks"], w[0]) and torch.equal(o["low_res_logits"], w[2]) for o, w in zip(got, want))
                t1, tl = alternate(one, loop, wall, reps)
                # the decoder alone, on the embeddings of these records
                emb = sam.image_encoder(torch.stack([sam.preprocess(x["image"]) for x in recs]).contiguous())
                image_pe = pe.get_dense_pe()
                sparse = [pe(points=None, boxes=x["boxes"], masks=None) for x in recs]
                cat, dense = torch.cat([s for s, _ in sparse]), sparse[0][1]
                which = np.repeat(np.arange(N), B)
                d1, dl = alternate(lambda: md.forward_images(emb, image_pe, cat, dense[:1], which, True),
                                   lambda: [md(emb[i:i + 1], image_pe, sparse[i][0], sparse[i][1], True) for i in range(N)],
                                   device_ms, reps)
                print(json.dumps({"N": N, "prompts_per_image": B, "identical": bool(same), "forward_ms": stats(t1),
                                  "loop_ms": stats(tl), "decoder_images_ms": stats(d1), "decoder_loop_ms": stats(dl)}), flush=True)


if __name__ == "__main__":
    main()
