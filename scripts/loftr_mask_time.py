"""Dev: cost of padding masks and rescaling in the drop-in LoFTR Matcher at 24 pairs of 256 x 256 in one process.
Three inputs alternate round by round — no masks, all-ones masks, padded masks (+ scales, the loftr_masked_256 pattern on every
pair) — each timed with device events around one call after a warm-up; prints the median per variant and the ratios to the
unmasked call.  A masked call always runs eagerly (no graph), as the unmasked one does by default."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pope_amd import synth  # noqa: E402
from pope_amd.matcher import Matcher, default_cfg  # noqa: E402

N, ROUNDS, WARM = 24, 20, 3
dev = torch.device("cuda:0")
m = Matcher(default_cfg).eval()
m.load_state_dict(synth.synthetic_matcher_state_dict(0))
m = m.to(dev)
inp, _ = synth.masked_loftr_case("loftr_masked_256")
rep = N // 2
i0, i1 = inp["image0"].repeat(rep, 1, 1, 1).to(dev), inp["image1"].repeat(rep, 1, 1, 1).to(dev)
ones = torch.ones(N, 32, 32, dtype=torch.bool, device=dev)
variants = {
    "none": {"image0": i0, "image1": i1},
    "ones": {"image0": i0, "image1": i1, "mask0": ones, "mask1": ones},
    "padded": {"image0": i0, "image1": i1, **{k: inp[k].repeat(rep, *([1] * (inp[k].dim() - 1))).to(dev)
                                              for k in ("mask0", "mask1", "scale0", "scale1")}},
}
times = {k: [] for k in variants}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for r in range(WARM + ROUNDS):
    for name, d in variants.items():
        data = dict(d)
        torch.cuda.synchronize()
        ev[0].record()
        m(data)
        ev[1].record()
        torch.cuda.synchronize()
        if r >= WARM:
            times[name].append(ev[0].elapsed_time(ev[1]))
med = {k: statistics.median(v) for k, v in times.items()}
for k, v in times.items():
    print(f"Matcher {N} x 256x256, masks {k:>6}: median {med[k]:.3f} ms (min {min(v):.3f}, max {max(v):.3f}, {len(v)} calls)")
print(f"ratio ones / none = {med['ones'] / med['none']:.3f}, padded / none = {med['padded'] / med['none']:.3f}")
