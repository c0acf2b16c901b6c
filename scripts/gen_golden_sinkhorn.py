"""Writes tests/golden/sinkhorn.npz: the reference's `CoarseMatching(match_type='sinkhorn')` and, end to end, its `Matcher` with
that option, run on the seeded inputs of `pope_amd.synth.sinkhorn_case` (run where the reference checkout exists:
`python scripts/gen_golden_sinkhorn.py /path/to/reference`).

The reference module does the work: the similarity without temperature, the -1e9 fill, exp, the dustbin prefilter and
`get_coarse_match` are its code, loaded from its file under a package of its own.  The one function it imports from a file it
does not ship, `.superglue.log_optimal_transport`, resolves to `pope_amd.sinkhorn_cpu.log_optimal_transport`, registered in
sys.modules beforehand (for the Matcher: as `src.matcher.utils.superglue`).

Stored per case (fp32 results only; the tests regenerate the inputs from the seed): b_ids / i_ids / j_ids, mconf, mkpts0_c /
mkpts1_c and conf_matrix (every 4th row and column for the 32 x 32 case).  For the Matcher case also mkpts0_f / mkpts1_f.

Asserted per case before anything is written, in fp64: the fp32 and fp64 runs of the reference publish identical match lists;
no non-zero confidence lies within 1e-3 of the threshold; in every row and column the dustbin entry and the best real entry of
the assignment differ by more than 1e-3 relative (the prefilter's decision); both prefilters fire; every pair meant to match
has at least 16 matches.  The same margins are asserted for every `synth.SINKHORN_SETTINGS` entry the GPU test sweeps.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import sinkhorn_cpu, synth  # noqa: E402

THR, BORDER, MARGIN = 0.2, 2, 1e-3
CFG = {"thr": THR, "border_rm": BORDER, "match_type": "sinkhorn", "dsmax_temperature": 0.1, "skh_iters": 3,
       "skh_init_bin_score": 1.0, "skh_prefilter": True, "sparse_spvs": False, "train_coarse_percent": 0.4,
       "train_pad_num_gt_min": 200}
# The Matcher case: without a temperature the peaked weights' default gain of 2 leaves sim too flat for any assignment to reach
# thr (no matches at any dustbin score); gain 4 gives sim up to ~23 and ~100 matches per pair with both prefilters deciding; at bin_score 0.5 no confidence lies within 2.9e-3 of thr
MATCHER_BIN_SCORE, MATCHER_GAIN = 0.5, 4.0
CONF_STRIDE = {"32x32": 4}


def load_reference(ref_root):
    """The reference's coarse_matching.py as `ref_skh.coarse_matching`, with `ref_skh.superglue` our statement of the recursion."""
    pkg = types.ModuleType("ref_skh")
    pkg.__path__ = [os.path.join(ref_root, "src", "matcher", "utils")]
    sys.modules["ref_skh"] = pkg
    sys.modules["ref_skh.superglue"] = sinkhorn_cpu
    spec = importlib.util.spec_from_file_location("ref_skh.coarse_matching", os.path.join(pkg.__path__[0], "coarse_matching.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_skh.coarse_matching"] = mod
    spec.loader.exec_module(mod)
    return mod.CoarseMatching


def run_reference(CoarseMatching, case, dtype, **cfg):
    m = CoarseMatching(dict(CFG, **cfg)).eval().to(dtype)
    data = {"hw0_c": case["hw0"], "hw1_c": case["hw1"], "hw0_i": case["hw0_i"]}
    masks = {}
    if "mask0" in case:
        data.update(mask0=case["mask0"], mask1=case["mask1"], scale0=case["scale0"].to(dtype), scale1=case["scale1"].to(dtype))
        masks = {"mask_c0": case["mask0"].flatten(1), "mask_c1": case["mask1"].flatten(1)}
    with torch.no_grad():
        m(case["feat0"].to(dtype), case["feat1"].to(dtype), data, **masks)
    return data


def check_margins(tag, conf64, a64, prefilter, need_filters):
    nz = conf64[conf64 != 0]
    gap = float((nz - THR).abs().min()) if nz.numel() else float("inf")
    assert gap > MARGIN, (tag, "confidence within 1e-3 of thr", gap)
    rows, cols = sinkhorn_cpu.dustbin_margins(a64)
    assert float(rows.min()) > MARGIN and float(cols.min()) > MARGIN, (tag, "dustbin margin", float(rows.min()), float(cols.min()))
    L, S = a64.shape[1] - 1, a64.shape[2] - 1
    f0 = int((a64.max(dim=2)[1] == S)[:, :L].sum())
    f1 = int((a64.max(dim=1)[1] == L)[:, :S].sum())
    if prefilter and need_filters:
        assert f0 > 0 and f1 > 0, (tag, "a prefilter never fires", f0, f1)
    return gap, float(rows.min()), float(cols.min()), f0, f1


def run_case(name, CoarseMatching):
    case = synth.sinkhorn_case(name)
    d32 = run_reference(CoarseMatching, case, torch.float32)
    d64 = run_reference(CoarseMatching, case, torch.float64)
    for k in ("b_ids", "i_ids", "j_ids"):
        assert torch.equal(d32[k], d64[k]), (name, k)
    kw = {"mask0": case["mask0"], "mask1": case["mask1"]} if "mask0" in case else {}
    a64 = sinkhorn_cpu.assignment(case["feat0"].double(), case["feat1"].double(), 1.0, 3, **kw)
    conf64 = sinkhorn_cpu.conf_matrix(case["feat0"].double(), case["feat1"].double(), 1.0, 3, True, **kw)
    assert torch.equal(conf64, d64["conf_matrix"]), name   # the reference's fp64 run is this definition
    gap, rmin, cmin, f0, f1 = check_margins(name, conf64, a64, True, name != "unrelated")
    n = case["feat0"].shape[0]
    counts = torch.bincount(d32["b_ids"], minlength=n).tolist()
    if name == "unrelated":
        assert sum(counts) == 0, counts
    else:
        assert min(counts) >= 16, (name, counts)
    mc = d32["mconf"]
    print(f"{name}: matches per pair {counts}, mconf {float(mc.min()) if len(mc) else 0:.3f}..{float(mc.max()) if len(mc) else 0:.3f}, "
          f"thr gap {gap:.3f}, dustbin margins rows {rmin:.3g} cols {cmin:.3g}, filtered rows {f0} cols {f1}")
    st = CONF_STRIDE.get(name, 1)
    out = {k: d32[k].numpy() for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c")}
    out["conf_matrix"] = d32["conf_matrix"][:, ::st, ::st].contiguous().numpy()
    out["conf_stride"] = np.int64(st)
    return {f"{name}.{k}": v for k, v in out.items()}


def check_settings():
    case = synth.sinkhorn_case("12x16_vs_10x14")
    f0, f1 = case["feat0"].double(), case["feat1"].double()
    for it, b, pre in synth.SINKHORN_SETTINGS:
        a64 = sinkhorn_cpu.assignment(f0, f1, b, it)
        conf64 = sinkhorn_cpu.conf_matrix(f0, f1, b, it, pre)
        print(f"setting iters {it} bin {b} prefilter {pre}:", check_margins((it, b, pre), conf64, a64, pre, False))


def run_matcher():
    """Two pairs of 128 x 128 images through the reference Matcher with match_type='sinkhorn' under the peaked weights."""
    sys.modules["src.matcher.utils.superglue"] = sinkhorn_cpu
    from oracle.gen_golden import load_reference_matcher   # (puts the reference checkout on sys.path)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0, gain=MATCHER_GAIN)
    sd.pop("_calibration_mean")
    sd["coarse_matching.bin_score"] = torch.tensor(MATCHER_BIN_SCORE)
    i0, i1 = synth.synthetic_gray_pairs(2, 128, 128, seed=61)
    outs = {}
    for dtype in (torch.float32, torch.float64):
        m, _ = load_reference_matcher({"match_type": "sinkhorn", "sparse_spvs": False})
        m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        data = {"image0": i0.to(dtype), "image1": i1.to(dtype)}
        with torch.no_grad():
            m.to(dtype)(data)
        outs[dtype] = data
    d32, d64 = outs[torch.float32], outs[torch.float64]
    for k in ("b_ids", "i_ids", "j_ids"):
        assert torch.equal(d32[k], d64[k]), ("matcher", k)
    conf64 = d64["conf_matrix"]
    nz = conf64[conf64 != 0]
    assert float((nz - THR).abs().min()) > MARGIN
    counts = torch.bincount(d32["b_ids"], minlength=2).tolist()
    assert min(counts) >= 16, counts
    print(f"matcher: matches per pair {counts}, thr gap {float((nz - THR).abs().min()):.3f}, "
          f"mkpts1_f fp32 vs fp64 {float((d32['mkpts1_f'].double() - d64['mkpts1_f']).abs().max()):.2e} px")
    out = {k: d32[k].numpy() for k in ("b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f")}
    out["bin_score"] = np.float32(MATCHER_BIN_SCORE)
    out["gain"] = np.float32(MATCHER_GAIN)
    return {f"matcher.{k}": v for k, v in out.items()}


def main():
    CoarseMatching = load_reference(sys.argv[1])
    torch.set_num_threads(8)
    blob = {}
    for name in synth.SINKHORN_CASES:
        blob.update(run_case(name, CoarseMatching))
    check_settings()
    blob.update(run_matcher())
    path = os.path.join(ROOT, "tests", "golden", "sinkhorn.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
