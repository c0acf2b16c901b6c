#!/usr/bin/env python
"""Generate the padded-batch fixtures tests/golden/{loftr_masked_256, loftr_masked_192x256_vs_256x192, coarse_masked,
coarse_masked_1024, loftr_xfmr_masked}.npz by running the REFERENCE's own modules on the CPU (mask0 / mask1, scale0 / scale1: matcher.py:62-65,
linear_attention.py:35-41, coarse_matching.py:28-43,115-118,178-184,242-250, fine_matching.py:68-69).

Needs the reference checkout next to the build (see oracle/gen_golden.py, whose loaders it imports; nothing under oracle/ is
changed).  Inputs come from pope_amd.synth (seeded), weights from synth.synthetic_matcher_state_dict(0); the fixtures keep
only outputs (feature taps: every TAP-th row, a stride that meets padded and valid cells of the 32- and 24-wide grids), compressed.
Before writing, it asserts the reference facts the tests rely on: all-ones masks reproduce the unmasked
outputs bit for bit, the all-ones pair of loftr_masked_256 has the match list of pair 1 of loftr_256_lowthr, and the padded
pair still has matches.

Usage:  python scripts/gen_golden_masked.py            (from the repo root)
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import OUT, load_reference_coarse_matching, load_reference_matcher, sd_digest  # noqa: E402
from pope_amd import synth  # noqa: E402

torch.set_num_threads(8)   # the thread count of every fixture (tests/conftest.py GOLDEN_THREADS)

TAP = 31
MATCH_KEYS = ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f")


def reference_matcher(sd, thr):
    ref, _ = load_reference_matcher({"thr": thr})
    ref.load_state_dict({"matcher." + k: v.clone() for k, v in sd.items()}, strict=True)
    return ref


def conf_top2(conf):
    """What the clear-decision rule needs of the reference conf matrix [n, L, S]: top-2 values and indices per row and per
    column (only a row maximum can match, coarse_matching.py:187-196)."""
    r = conf.topk(2, dim=2)
    c = conf.topk(2, dim=1)
    return {"conf_row_top2": r.values.numpy(), "conf_row_top2_idx": r.indices.numpy(),
            "conf_col_top2": c.values.numpy(), "conf_col_top2_idx": c.indices.numpy()}


def gen_matcher(sd, digest):
    for name in synth.MASKED_LOFTR_CASES:
        inp, thr = synth.masked_loftr_case(name)
        ref = reference_matcher(sd, thr)
        data = dict(inp)
        with torch.no_grad():
            ref(data)
            fc0, fc1 = ref(dict(inp), only_att_fea=True)
            # the scale1-only quirk: mkpts1_c scaled, the fine offset not (fine_matching.py:68 keys on 'scale0')
            only1 = {k: v for k, v in inp.items() if k != "scale0"}
            ref(only1)
            # all-ones masks reproduce the unmasked reference bit for bit
            ones = dict(inp, mask0=torch.ones_like(inp["mask0"]), mask1=torch.ones_like(inp["mask1"]))
            ones.pop("scale0"), ones.pop("scale1")
            plain = {"image0": inp["image0"], "image1": inp["image1"]}
            ref(ones), ref(plain)
        for k in ("conf_matrix",) + MATCH_KEYS:
            assert torch.equal(ones[k], plain[k]), f"{name}: all-ones masks change {k}"
        for k in ("b_ids", "i_ids", "j_ids"):
            assert torch.equal(only1[k], data[k]), k
        assert torch.equal(only1["mkpts1_c"], data["mkpts1_c"])
        b = data["b_ids"]
        counts = [int((b == k).sum()) for k in range(inp["image0"].shape[0])]
        assert counts[0] > 0, f"{name}: the padded pair has no matches"
        if name == "loftr_masked_256":
            low = np.load(os.path.join(OUT, "loftr_256_lowthr.npz"))
            sel, lsel = data["b_ids"].numpy() == 1, low["b_ids"] == 1
            assert np.array_equal(data["i_ids"].numpy()[sel], low["i_ids"][lsel])
            assert np.array_equal(data["j_ids"].numpy()[sel], low["j_ids"][lsel])
            print(name, f"pair 1 has the {int(lsel.sum())} matches of loftr_256_lowthr pair 1")
        print(name, "thr", thr, "matches per pair", counts)
        np.savez_compressed(os.path.join(OUT, name + ".npz"),
                 weights_seed=0, weights_digest=digest, thr=np.float64(thr), n=inp["image0"].shape[0],
                 shape0=np.array(inp["image0"].shape[2:]), shape1=np.array(inp["image1"].shape[2:]),
                 image_digest=np.array([float(inp["image0"].double().sum()), float(inp["image1"].double().sum())]),
                 mask0=inp["mask0"].numpy(), mask1=inp["mask1"].numpy(), scale0=inp["scale0"].numpy(), scale1=inp["scale1"].numpy(),
                 feat_c0=fc0[:, ::TAP].numpy(), feat_c1=fc1[:, ::TAP].numpy(),
                 **conf_top2(data["conf_matrix"]), **{k: data[k].numpy() for k in MATCH_KEYS},
                 s1only_mkpts1_c=only1["mkpts1_c"].numpy(), s1only_mkpts1_f=only1["mkpts1_f"].numpy(),
                 s1only_mkpts0_f=only1["mkpts0_f"].numpy(),
                 hw0_c=np.array(data["hw0_c"]), hw1_c=np.array(data["hw1_c"]), tap=TAP)


def filled_entries(m0, m1):
    """(uniform, zero) boolean [n, L, S] for fill masks m0 [n, L], m1 [n, S]: filled entries (m0[i] * m1[j] == 0) whose row
    and column are filled throughout (conf = 1 / (L S)), and those whose row or column is not (conf = 0)."""
    valid = m0[:, :, None] & m1[:, None, :]
    row_any, col_any = valid.any(2, keepdim=True), valid.any(1, keepdim=True)
    return ~valid & ~row_any & ~col_any, ~valid & (row_any | col_any)


def gen_coarse():
    f0, f1, m0, m1, s0, s1, thr = synth.masked_coarse_case()
    cm = load_reference_coarse_matching()
    cm.thr = thr
    h, w = m0.shape[1:]
    data = {"hw0_c": (h, w), "hw1_c": (h, w), "hw0_i": (8 * h, 8 * w), "hw1_i": (8 * h, 8 * w),
            "mask0": m0, "mask1": m1, "scale0": s0, "scale1": s1}
    with torch.no_grad():
        cm(f0, f1, data, mask_c0=m0.flatten(-2), mask_c1=m1.flatten(-2))
        ones = {k: v for k, v in data.items() if k in ("hw0_c", "hw1_c", "hw0_i", "hw1_i")}
        plain = dict(ones)
        o = torch.ones(3, h * w, dtype=torch.bool)
        cm(f0, f1, ones, mask_c0=o, mask_c1=o)   # all-ones fill masks
        cm(f0, f1, plain)
    for k in ("conf_matrix", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c"):
        assert torch.equal(ones[k], plain[k]), f"coarse: all-ones fill masks change {k}"
    conf = data["conf_matrix"]
    L = h * w
    # a filled entry is 0 when its row or its column still holds an unfilled one, else both softmaxes are uniform
    uniform, zero = filled_entries(m0.flatten(1), m1.flatten(1))
    assert bool((conf[uniform] == torch.tensor(1.0 / L) * torch.tensor(1.0 / L)).all())
    assert bool((conf[zero] == 0).all()) and not bool(conf.isnan().any())
    counts = [int((data["b_ids"] == k).sum()) for k in range(3)]
    assert counts[0] > 0 and counts[1] == 0 and counts[2] == 0, counts
    print("coarse_masked thr", thr, "matches per pair", counts)
    f_digest = np.array([float(f0.double().sum()), float(f1.double().sum())])
    np.savez_compressed(os.path.join(OUT, "coarse_masked.npz"), thr=np.float64(thr), feat_digest=f_digest,
             mask0=m0.numpy(), mask1=m1.numpy(), scale0=s0.numpy(), scale1=s1.numpy(), conf_matrix=conf.numpy(),
             **{k: data[k].numpy() for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c")})


def gen_coarse_large():
    """coarse_masked_1024: the reference CoarseMatching at the LoFTR 256 x 256 grid with the loftr_masked_256 masks and scales;
    the conf matrix (8 MB) is kept as its per-row / per-column top 2."""
    f0, f1, m0, m1, s0, s1, thr = synth.masked_coarse_case_large()
    cm = load_reference_coarse_matching()
    cm.thr = thr
    h, w = m0.shape[1:]
    data = {"hw0_c": (h, w), "hw1_c": (h, w), "hw0_i": (8 * h, 8 * w), "hw1_i": (8 * h, 8 * w),
            "mask0": m0, "mask1": m1, "scale0": s0, "scale1": s1}
    with torch.no_grad():
        cm(f0, f1, data, mask_c0=m0.flatten(-2), mask_c1=m1.flatten(-2))
    conf = data["conf_matrix"]
    uniform, zero = filled_entries(m0.flatten(1), m1.flatten(1))
    L = h * w
    assert bool((conf[uniform] == torch.tensor(1.0 / L) * torch.tensor(1.0 / L)).all()) and bool(uniform.any())
    assert bool((conf[zero] == 0).all()) and not bool(conf.isnan().any())
    counts = [int((data["b_ids"] == k).sum()) for k in range(2)]
    assert min(counts) > 100, counts
    print("coarse_masked_1024 thr", thr, "matches per pair", counts)
    np.savez_compressed(os.path.join(OUT, "coarse_masked_1024.npz"), thr=np.float64(thr),
                        feat_digest=np.array([float(f0.double().sum()), float(f1.double().sum())]),
                        mask0=m0.numpy(), mask1=m1.numpy(), scale0=s0.numpy(), scale1=s1.numpy(), **conf_top2(conf),
                        **{k: data[k].numpy() for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c")})


def gen_xfmr(sd):
    ref = reference_matcher(sd, 0.2)
    xf = ref.loftr_coarse
    f0, f1, m0, m1 = synth.masked_xfmr_case()
    with torch.no_grad():
        o0, o1 = xf(f0, f1, m0, m1)
        p0, p1 = xf(f0, f1)
        q0, q1 = xf(f0, f1, torch.ones_like(m0), torch.ones_like(m1))
        layer = xf.layers[1]   # a 'cross' layer
        lx = layer(f0, f1, m0, None)      # x_mask only
        ls = layer(f0, f1, None, m1)      # source_mask only
        lb = layer(f0, f1, m0, m1)
    assert torch.equal(p0, q0) and torch.equal(p1, q1), "all-ones masks change the transformer"
    print("loftr_xfmr_masked: max |masked - unmasked|", float((o0 - p0).abs().max()), float((o1 - p1).abs().max()))
    np.savez_compressed(os.path.join(OUT, "loftr_xfmr_masked.npz"),
                        feat_digest=np.array([float(f0.double().sum()), float(f1.double().sum())]),
                        mask0=m0.numpy(), mask1=m1.numpy(), layer_index=1, tap=TAP,
                        out0=o0[:, ::TAP].numpy(), out1=o1[:, ::TAP].numpy(), layer_xmask=lx[:, ::TAP].numpy(),
                        layer_smask=ls[:, ::TAP].numpy(), layer_both=lb[:, ::TAP].numpy())


def main():
    sd = synth.synthetic_matcher_state_dict(seed=0)
    digest = sd_digest({k: v for k, v in sd.items() if v.dtype.is_floating_point})
    gen_coarse()
    gen_coarse_large()
    gen_xfmr(copy.deepcopy(sd))
    gen_matcher(sd, digest)


if __name__ == "__main__":
    main()
