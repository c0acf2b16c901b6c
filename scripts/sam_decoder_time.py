"""Time the SAM mask decoder on one GPU for the automatic mask generator's call: P one-point prompts (the 16 x 16 grid,
multimask_output=True): `python scripts/sam_decoder_time.py [P] [iters]`.  Prints ms per call in f16x3 and f32 and, on the
same card, for the torch fp32 restatement of tests/test_sam_decoder_cpu.py (32 prompts per chunk), one JSON line each."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pope_amd import synth  # noqa: E402
from test_sam_decoder_cpu import build_models, restate  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    P = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    dev = "cuda:0"
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    pe, md = build_models(sd)
    pe, md = pe.to(dev), md.to(dev)
    img = synth.synthetic_sam_image_embedding(seed=1).to(dev)
    (coords, labels), _, _ = synth.sam_decoder_case("grid")
    coords, labels = coords[:P].to(dev), labels[:P].to(dev)
    sparse, dense = pe(points=(coords, labels), boxes=None, masks=None)
    image_pe = pe.get_dense_pe()
    for precision in ("f16x3", "f32"):
        md.precision = precision
        med, best = timed(lambda: md(img, image_pe, sparse, dense, True), iters)
        print(json.dumps({"what": f"pope_amd MaskDecoder {precision}", "P": P, "ms_median": round(med, 3), "ms_min": round(best, 3)}))
    sdd = {k: v.to(dev) for k, v in sd.items()}
    with torch.no_grad():
        med, best = timed(lambda: restate(sdd, img, image_pe, sparse, dense, True), max(3, iters // 3))
    print(json.dumps({"what": "torch fp32 restatement", "P": P, "ms_median": round(med, 3), "ms_min": round(best, 3)}))


if __name__ == "__main__":
    main()
