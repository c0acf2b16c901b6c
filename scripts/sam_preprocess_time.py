"""Times SAM's input transform on one GPU, in one process, for Q = 1 and 8 frames of 480 x 640:
 (1) the device time of `pope_sam_preprocess_u8_f32` (both of its launches: the horizontal pass into the uint8 scratch, the
     vertical pass with the normalising, padding fp32 epilogue), with events around --calls back-to-back calls, and the bytes/s
     that is of the entry's floor: the frames read once (Q * H * W * 3 bytes) plus the encoder's input written once
     (Q * 3 * S * S * 4 bytes); the scratch traffic is not part of the floor;
 (2) WALL time from the frames to the encoder's input (a device synchronisation before the clock starts and one before it
     stops), host work included, for
       (a) the host path: numpy frames through `ResizeLongestSide.apply_image` (Pillow, frame by frame), the upload of the
           resized stack and `Sam.preprocess` (three fp32 passes in torch), as `SamAutomaticMaskGenerator._decode_frames` runs it;
       (b) the device path: the same frames as one uint8 CUDA tensor through `SamPredictor.preprocess_frames`.
Before any timing it checks that (a) and (b) give the same bits.  After the warm-up calls (a) and (b) alternate within each
repetition; the spread of each (max - min over the repetitions) is printed next to the medians and the verdict compares the
difference of the medians with it.  Writes the table to --out (default profiles/sam_preprocess.md).
usage: python scripts/sam_preprocess_time.py [--queries 1 8] [--reps 9] [--warmup 3] [--calls 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pope_amd import sam_generator as sg  # noqa: E402
from frame_query_time import wall_pair  # noqa: E402


def device_ms(fn, calls, reps, warmup):
    """Device ms of one fn() between two events around `calls` back-to-back calls: (median, min, max) over `reps`."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_preprocess.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    H, W, Qmax = 480, 640, max(a.queries)
    sam = sg.build_sam_vit_b().to(dev)       # only its pixel buffers and its input size are used: the weights do not matter
    pr = sg.SamPredictor(sam)
    S = sam.image_encoder.img_size
    frames = [(torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5 + q)) * 255).to(torch.uint8).numpy() for q in range(Qmax)]
    stack = torch.from_numpy(np.stack(frames)).to(dev)

    def host_path(Q):
        resized = np.stack([pr.transform.apply_image(im) for im in frames[:Q]])
        x = torch.as_tensor(resized, device=dev).permute(0, 3, 1, 2).contiguous()
        return sam.preprocess(x).contiguous()

    def device_path(Q):
        return pr.preprocess_frames(stack[:Q], "RGB", "sam_preprocess_time")[0]

    xa, xb = host_path(Qmax), device_path(Qmax)
    equal = xa.shape == xb.shape and torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    head = f"device path at Q = {Qmax} equals the host path bit for bit: {equal}"
    print(head, flush=True)
    assert equal
    del xa, xb
    kernel_rows, wall_rows, slower = [], [], []
    for Q in a.queries:
        floor = Q * H * W * 3 + Q * 3 * S * S * 4
        med, lo, hi = device_ms(lambda: device_path(Q), a.calls, a.reps, a.warmup)
        kernel_rows.append(f"| {Q} | {floor / 1e6:.2f} | {med * 1e3:.1f} ({lo * 1e3:.1f} .. {hi * 1e3:.1f}) | {floor / med / 1e6:.0f} | "
                           f"{floor / med / 1e6 / 6300 * 100:.1f} |")
        print(kernel_rows[-1], flush=True)
        ta, tb = wall_pair(lambda: host_path(Q), lambda: device_path(Q), a.reps, a.warmup)
        ma, mb = statistics.median(ta), statistics.median(tb)
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        wall_rows.append(f"| {Q} | {ma:.3f} ({min(ta):.3f} .. {max(ta):.3f}) | {mb:.3f} ({min(tb):.3f} .. {max(tb):.3f}) | {ma - mb:+.3f} | "
                         f"{spread:.3f} | {ma / mb:.1f} |")
        print(wall_rows[-1], flush=True)
        if mb - ma > spread:
            slower.append(Q)
    verdict = ("The device path is not slower than the host path at any Q beyond the run-to-run spread." if not slower else
               f"SLOWER: at Q = {slower} the device path's median exceeds the host path's by more than the spread.")
    print(verdict)
    argv = [v for i, v in enumerate(sys.argv[1:]) if v != "--out" and (i == 0 or sys.argv[i] != "--out")]
    text = f"""# SAM input transform: frames on the device against the host path

`python scripts/sam_preprocess_time.py{"".join(" " + v for v in argv)}` on one MI355X, one process; {H} x {W} uint8 frames to the
encoder's input [Q, 3, {S}, {S}] fp32 (resized to 768 x 1024, normalised, zero rows below).

{head}

## `pope_sam_preprocess_u8_f32`: device time

Events around {a.calls} back-to-back calls of `sam_preprocess_batch` (the horizontal pass into the uint8 scratch and the vertical
pass with the fp32 epilogue; the output and scratch allocations come from torch's caching allocator), {a.warmup} warm-up calls,
median (min .. max) of {a.reps} repetitions.  The events see the larger of the device's work and the rate at which the host issues
the calls: where a call's kernels are shorter than its Python and launch work (Q = 1), the figure is that rate, an upper bound of
the device time.  The floor counts the frames read once and the output written once; 6.3 TB/s is what a streaming kernel reaches
of the 8 TB/s HBM peak on this part.  What lies between the floor and the time is the uint8 scratch between the two passes
(written byte-wide by the horizontal pass, which also reads the frames byte-wide; read as words by the vertical one where OW % 4 == 0) and the integer
arithmetic of the taps; the two launches were not timed separately.

| Q | floor, MB | device time per call, us | GB/s of the floor | % of 6.3 TB/s |
|---|---|---|---|---|
""" + "\n".join(kernel_rows) + f"""

## Frames to the encoder's input: wall time

A device synchronisation before the clock starts and one before it stops; {a.warmup} warm-up calls of each path, then {a.reps}
repetitions in which the two alternate; median (min .. max), ms.

(a) host path, numpy frames: Pillow resize frame by frame, upload of the resized stack, `Sam.preprocess` in torch.
(b) device path, the same frames as one uint8 CUDA tensor: one `pope_sam_preprocess_u8_f32` call.

| Q | (a) host path, ms | (b) device path, ms | (a) - (b), ms | spread (largest max - min), ms | (a) / (b) |
|---|---|---|---|---|---|
""" + "\n".join(wall_rows) + f"""

{verdict}

The host path's time is host work (Pillow is single-threaded) plus a {768 * 1024 * 3 / 1e6:.1f} MB upload per frame, all of it
before the encoder can start; it was counted inside the "encoder" row of profiles/sam_generator.md.
"""
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
