"""Dev: what ResNetFPN_8_2.precision = "f16" buys and costs, written to profiles/loftr_f16.md.

Times (device events, 3 warm-up calls, median (min .. max) of REPS repetitions, the two modes alternating inside one process so
that clocks and neighbours hit both alike):
  - the backbone alone at 6 and 48 images of 256 x 256;
  - the Matcher call at 3 and 24 pairs of 256 x 256 under synth's peaked LoFTR weights.
For the 24-pair call also the matches of each mode, the share of the f16x3 matches that the f16 mode publishes with the same
coarse cell pair, and the largest |mkpts1_f| difference among those.  Accuracy of the backbone against the oracle's fp64 network
next to the CPU emulation of the mode's roundings (tests/loftr_f16_checks.py), at the shapes of tests/test_gpu_loftr_f16.py.

    python scripts/loftr_f16_time.py [--out profiles/loftr_f16.md]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pope_amd import synth  # noqa: E402
from pope_amd.matcher import Matcher, default_cfg  # noqa: E402

REPS = 9
MODES = ("f16x3", "f16")


def timed(fns):
    """fns: {mode: callable}.  Per mode [ms] of REPS calls, the modes alternating call by call."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def cell(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def verdict(ms):
    """Faster beyond the spread: the slowest f16 repetition beats the fastest f16x3 one."""
    a, b = ms["f16x3"], ms["f16"]
    ratio = statistics.median(a) / statistics.median(b)
    if max(b) < min(a):
        return f"f16 faster beyond the spread, x{ratio:.2f} by the medians"
    if max(a) < min(b):
        return f"f16 SLOWER beyond the spread, x{ratio:.2f} by the medians"
    return f"no difference beyond the spread (x{ratio:.2f} by the medians)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loftr_f16.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    ms_ = {}
    for mode in MODES:
        m = Matcher(default_cfg).eval()
        m.load_state_dict(dict(sd), strict=True)
        m = m.to(dev)
        m.backbone.precision = mode
        ms_[mode] = m
    i0, i1 = (t.to(dev) for t in synth.synthetic_gray_pairs(3, 256, 256, seed=21))
    lines = ["# LoFTR backbone: precision=\"f16\" against the default \"f16x3\"", "",
             f"Written by scripts/loftr_f16_time.py on {torch.cuda.get_device_name(0)}.  Times in ms: median (min .. max) of {REPS} "
             "repetitions after 3 warm-up calls, device events, the two modes alternating call by call in one process.  Matcher "
             "weights: synth.peaked_matcher_state_dict (tests/golden/loftr_512_peaked.npz), images synth.synthetic_gray_pairs, 256 x 256.", "",
             "## Times", "", "| what | f16x3 | f16 | verdict |", "|---|---|---|---|"]
    with torch.no_grad():
        for n in (6, 48):
            x = torch.cat([i0, i1], 0).repeat(n // 6, 1, 1, 1)
            ms = timed({mode: (lambda mm=ms_[mode]: mm.backbone(x)) for mode in MODES})
            lines.append(f"| backbone, {n} images | {cell(ms['f16x3'])} | {cell(ms['f16'])} | {verdict(ms)} |")
        last = {}
        for n in (3, 24):
            a, b = i0.repeat(n // 3, 1, 1, 1), i1.repeat(n // 3, 1, 1, 1)

            def call(mm):
                d = {"image0": a, "image1": b}
                mm(d)
                last[mm.backbone.precision] = d
            ms = timed({mode: (lambda mm=ms_[mode]: call(mm)) for mode in MODES})
            lines.append(f"| Matcher call, {n} pairs | {cell(ms['f16x3'])} | {cell(ms['f16'])} | {verdict(ms)} |")
        # match agreement of the 24-pair call
        key = lambda d: {(int(b), int(i), int(j)): k for k, (b, i, j) in enumerate(zip(d["b_ids"].tolist(), d["i_ids"].tolist(), d["j_ids"].tolist()))}
        k3, k1 = key(last["f16x3"]), key(last["f16"])
        common = [t for t in k3 if t in k1]
        p3 = last["f16x3"]["mkpts1_f"][[k3[t] for t in common]]
        p1 = last["f16"]["mkpts1_f"][[k1[t] for t in common]]
        dmax = float((p3 - p1).abs().max()) if common else float("nan")
        lines += ["", "## Match agreement, 24-pair call", "",
                  f"- matches: f16x3 {len(k3)}, f16 {len(k1)}",
                  f"- f16x3 matches that f16 publishes with the same coarse cell pair: {len(common)} of {len(k3)} "
                  f"({100.0 * len(common) / max(1, len(k3)):.2f} %)",
                  f"- largest |mkpts1_f| difference among those: {dmax:.4f} px"]
        # accuracy against fp64 next to the emulation
        import loftr_f16_checks as E
        from oracle import loftr_ref
        msd = synth.synthetic_matcher_state_dict(seed=0)
        bsd = {k[len("backbone."):]: v for k, v in msd.items() if k.startswith("backbone.")}
        acc = Matcher(default_cfg).eval()
        acc.load_state_dict(dict(msd), strict=True)
        acc = acc.to(dev)
        lines += ["", "## Backbone error against the fp64 network (synthetic checkpoint-layout weights)", "",
                  "| images | map | mode | max abs err | rms err | emulation max | emulation rms | max abs ref64 |", "|---|---|---|---|---|---|---|---|"]
        for n, H, W in ((2, 16, 24), (3, 32, 40)):
            x = synth.synthetic_gray_pairs(n, H, W, seed=n + H)[0]
            ref = loftr_ref.resnet_fpn_8_2({k: v.double() for k, v in msd.items()}, x.double())
            emul = E.backbone_emul(bsd, x)
            for mode in MODES:
                acc.backbone.precision = mode
                got = acc.backbone(x.to(dev))
                for name, g, w, e in (("coarse", got[0], ref[0], emul[0]), ("fine", got[1], ref[1], emul[1])):
                    gm, gr = E.errors(g.cpu(), w)
                    em, er = E.errors(e, w)
                    emu = f"{em:.3e} | {er:.3e}" if mode == "f16" else "- | -"
                    lines.append(f"| {n} x {H} x {W} | {name} | {mode} | {gm:.3e} | {gr:.3e} | {emu} | {float(w.abs().max()):.3f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
