"""Dev: forward time of ViT-g/14 (SwiGLU FFN) next to ViT-L/14 (the yardstick: its code path has no SwiGLU in it) in f16x3 at
476 x 630 (1 531 tokens), synthetic weights, batches of 64 and of 8.  One process; per batch size both models are warmed
up, then timed ALTERNATELY with device events, median of RUNS forwards each.  Algorithmic FLOPs per image and block:
2 N (4 dim^2 + ffn) + 4 N^2 dim with ffn = 2 dim hidden (MLP) or 3 dim hidden (SwiGLU: w12 is [2 hidden, dim]), plus the
patch embed.  Prints a markdown table and the giant / large ratio of algorithmic TFLOP/s (profiles/vit_giant.md).

Usage:  python scripts/vit_giant_time.py [--runs 10] [--batches 64,8] [--depth-g 40]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pope_amd import synth  # noqa: E402
from pope_amd.dinov2 import DinoVisionTransformer, build_vitg14, vit_large  # noqa: E402

H, W = 476, 630
N = 1 + (H // 14) * (W // 14)


def flops_per_image(dim, depth, hidden, swiglu):
    ffn = (3 if swiglu else 2) * dim * hidden
    return depth * (2 * N * (4 * dim * dim + ffn) + 4 * N * N * dim) + 2 * N * 588 * dim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--depth-g", type=int, default=40, help="blocks of the giant (40 = the real model)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    models = {}
    large = vit_large(patch_size=14, img_size=518, init_values=1e-5, ffn_layer="mlp", block_chunks=0).eval()
    large.load_state_dict(synth.synthetic_state_dict(seed=0, dim=1024, depth=24), strict=True)
    models["ViT-L/14"] = (large.to(dev), flops_per_image(1024, 24, 4096, False))
    giant = DinoVisionTransformer(embed_dim=1536, depth=args.depth_g, num_heads=24, mlp_ratio=4, **build_vitg14.keywords).eval()
    giant.load_state_dict(synth.synthetic_state_dict(seed=0, dim=1536, depth=args.depth_g, ffn="swiglu"), strict=True)
    models["ViT-g/14"] = (giant.to(dev), flops_per_image(1536, args.depth_g, 4096, True))
    print(f"{torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs; "
          f"{H} x {W}, {N} tokens, f16x3, median of {args.runs} forwards, device events\n")
    print("| model | batch | ms / forward (median) | min .. max | images/s | GF / image | algorithmic TFLOP/s |")
    print("|---|---|---|---|---|---|---|")
    ratios = []
    for B in (int(b) for b in args.batches.split(",")):
        x = synth.synthetic_images(B, H, W, seed=3).to(dev)
        times = {k: [] for k in models}
        with torch.no_grad():
            for m, _ in models.values():
                for _ in range(2):
                    m(x)
            torch.cuda.synchronize()
            for _ in range(args.runs):
                for k, (m, _) in models.items():   # alternate: both models see the same clock and neighbour conditions
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    m(x)
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1))
        tf = {}
        for k, (m, fl) in models.items():
            med = statistics.median(times[k])
            tf[k] = B * fl / (med * 1e-3) / 1e12
            print(f"| {k} | {B} | {med:.2f} | {min(times[k]):.2f} .. {max(times[k]):.2f} | {B / med * 1e3:.1f} | {fl / 1e9:.1f} | {tf[k]:.1f} |")
            assert m.overflow_events == 0
        ratios.append((B, tf["ViT-g/14"] / tf["ViT-L/14"]))
    print()
    for B, r in ratios:
        print(f"batch {B}: ViT-g/14 algorithmic TFLOP/s = {r:.3f} x ViT-L/14's")


if __name__ == "__main__":
    main()
