"""Times "encode the reference once, match many crops" on one GPU, in one process: wall clock around calls that end in a
synchronise, after a warm-up, the variants of a row taken in turn inside every repetition (so drift of the card hits all of
them alike), median and spread (min .. max) of the repetitions.

Rows
  Matcher, 3 pairs at 256 x 256, one reference:     plain call on the repeated image | image0 [1] + image0_index | kept encoding
  Matcher, 24 pairs at 256 x 256, eight references: the same three
  driver step (`locate_match_pose_batch_u8`) at Q = 1 and Q = 8, 8 proposals each: image references | a `ReferenceSet`
  the one-off cost of `encode_references` for 1 and for 8 references
With --parent DIR (a directory that holds ANOTHER build of the package, e.g. the parent commit's `pope_amd/` with its own
libpope_hip.so) the plain Matcher call and the image-reference driver step of that build are timed in the same turns: that
is the baseline; the new build's plain path is printed next to it only as a cross-check.  Before any timing the script checks
that every variant returns what the plain call returns, bit for bit.
usage: python scripts/reference_prompt_time.py [--parent DIR] [--reps 30] [--warmup 5]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_package(directory, name):
    """The package at `directory`/pope_amd under another module name (its modules import each other relatively, and each
    build loads the libpope_hip.so next to it)."""
    init = os.path.join(directory, "pope_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, init, submodule_search_locations=[os.path.dirname(init)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return name


def models(pkg, dev):
    imp = importlib.import_module
    synth = imp(pkg + ".synth")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    mt = imp(pkg + ".matcher")
    matcher = mt.Matcher(mt.default_cfg).eval()
    matcher.load_state_dict(sd, strict=True)
    vit = imp(pkg + ".dinov2_utils").load_dinov2_model(state_dict=synth.synthetic_state_dict(seed=0)).to(dev)
    return vit, matcher.to(dev), imp(pkg + ".driver")


def turns(variants, reps, warmup):
    """{name: fn} -> {name: (median, min, max)} in ms; every repetition runs each variant once, in order."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            samples[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def report(title, res, base):
    print(title)
    for k, (med, lo, hi) in res.items():
        rel = f"   {med / res[base][0]:.3f} x {base}" if k != base else ""
        print(f"    {k:34s} {med:8.3f} ms   ({lo:.3f} .. {hi:.3f}){rel}")


MATCH_KEYS = ("conf_matrix", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f")


def matcher_rows(new, parent, dev, R, per_ref, reps, warmup):
    from pope_amd import synth
    refs, crops = synth.synthetic_gray_pairs(R, 256, 256, seed=7)
    refs = refs.to(dev)
    index = torch.arange(R).repeat_interleave(per_ref)
    crops = crops.index_select(0, index)
    crops = (crops + 0.01 * torch.randn(crops.shape, generator=torch.Generator().manual_seed(R))).clamp_(0, 1).to(dev)
    repeated = refs.index_select(0, index.to(dev))
    matcher = new[1]
    enc = matcher.encode_reference(refs)

    def plain(m):
        d = {"image0": repeated, "image1": crops}
        m(d)
        return d

    def indexed():
        d = {"image0": refs, "image0_index": index, "image1": crops}
        matcher(d)
        return d

    def kept():
        d = {"reference": enc, "image0_index": index, "image1": crops}
        matcher(d)
        return d

    want = plain(matcher)
    checks = {"image0 + index": indexed(), "kept encoding": kept()}
    if parent:
        checks["parent build, plain"] = plain(parent[1])
    bad = {k: [key for key in MATCH_KEYS if not torch.equal(d[key], want[key])] for k, d in checks.items()}
    print(f"Matcher, {R * per_ref} pairs / {R} references: {int(want['b_ids'].numel())} matches; equal to the plain call bit for bit: "
          + ", ".join(f"{k}: {not v}" + (f" {v}" if v else "") for k, v in bad.items()))
    variants = {}
    if parent:
        variants["parent: repeated image"] = lambda: plain(parent[1])
    variants.update({"new: repeated image": lambda: plain(matcher), "new: image0 [R] + index": indexed, "new: kept encoding": kept})
    res = turns(variants, reps, warmup)
    report(f"Matcher call, {R * per_ref} pairs at 256 x 256, {R} reference(s)", res, next(iter(variants)))
    return res


def driver_rows(new, parent, dev, Q, reps, warmup):
    from pope_amd import synth
    vit, matcher, drv = new
    cases = [synth.synthetic_frame_case(seed=31 + q) for q in range(Q)]
    refs, frames = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    boxes, K0, K1 = [c[2] for c in cases], np.stack([c[3] for c in cases]), np.stack([c[4] for c in cases])
    refset = drv.encode_references(vit, matcher, refs)

    def images(pk):
        return pk[2].locate_match_pose_batch_u8(pk[0], pk[1], refs, frames, boxes, K0, K1)

    def kept():
        return drv.locate_match_pose_batch_u8(vit, matcher, refset, frames, boxes, K0, K1)

    def same(a, b):
        return all(np.array_equal(x["mconf"][s], y["mconf"][s]) and np.array_equal(x["mkpts1"][s], y["mkpts1"][s])
                   for x, y in zip(a, b) for s in range(3)) and all(
            (x["pose"] is None) == (y["pose"] is None) and (x["pose"] is None or all(np.array_equal(u, v) for u, v in zip(x["pose"], y["pose"])))
            for x, y in zip(a, b))

    want = images(new)
    print(f"driver step, Q = {Q}: ReferenceSet equals image references bit for bit: {same(kept(), want)}"
          + (f"; parent build equals: {same(images(parent), want)}" if parent else ""))
    variants = {}
    if parent:
        variants["parent: image references"] = lambda: images(parent)
    variants.update({"new: image references": lambda: images(new), "new: ReferenceSet": kept})
    res = turns(variants, reps, warmup)
    report(f"locate_match_pose_batch_u8, Q = {Q}, 8 proposals each", res, next(iter(variants)))
    enc = turns({f"encode_references, R = {Q}": lambda: drv.encode_references(vit, matcher, refs)}, reps, warmup)
    report("one-off cost", enc, next(iter(enc)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory holding another build's pope_amd/ (the baseline)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}; "
          f"{a.reps} repetitions after {a.warmup} warm-up turns, variants in turn inside each repetition")
    new = models("pope_amd", dev)
    parent = models(load_package(a.parent, "pope_amd_parent"), dev) if a.parent else None
    if not parent:
        print("no --parent build given: NO BASELINE in this run (the new build's plain path is not one)")
    with torch.no_grad():
        matcher_rows(new, parent, dev, 1, 3, a.reps, a.warmup)
        matcher_rows(new, parent, dev, 8, 3, a.reps, a.warmup)
        for Q in (1, 8):
            driver_rows(new, parent, dev, Q, a.reps, a.warmup)


if __name__ == "__main__":
    main()
