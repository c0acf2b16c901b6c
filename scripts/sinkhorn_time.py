"""Dev: device time of `dense_match` with match_type='sinkhorn' (csrc/sinkhorn.hip) beside the dual-softmax call on the same
inputs, in the same process, and the error of the Sinkhorn confidences against the fp64 definition (pope_amd/sinkhorn_cpu.py).
Writes profiles/sinkhorn.md (`python scripts/sinkhorn_time.py [--out FILE]`).

Method: device events around `calls` back-to-back calls (each call ends in its own read-back of the match counts) after 3
warm-up rounds; median (min .. max) of 9 repetitions, per call; the two matchers alternate inside every repetition.  The cost of
one Sinkhorn iteration (a row pass and a column pass over the matrix) is the slope between skh_iters = 1, 3 and 5."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import sinkhorn_cpu  # noqa: E402
from pope_amd.matcher import dense_match  # noqa: E402

WORKLOADS = [(3, 32, 32), (24, 32, 32), (1, 60, 80)]   # (pairs, grid h, grid w): 1024 x 1024 cells x 3 / x 24, 4800 x 4800 x 1
WARM, REPS = 3, 9


def features(n, L, dev, seed=7):
    """Planted correspondences as in synth.sinkhorn_case: 60 % of the cells copied across a permutation with noise 0.3."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(n, L, 256, generator=g)
    f1 = torch.randn(n, L, 256, generator=g)
    k = int(0.6 * L)
    for b in range(n):
        src, dst = torch.randperm(L, generator=g)[:k], torch.randperm(L, generator=g)[:k]
        f1[b, dst] = f0[b, src] + 0.3 * torch.randn(k, 256, generator=g)
    return (f0 * 12 ** .5).to(dev), (f1 * 12 ** .5).to(dev)


def clock_mhz():
    """The shader clock right now, read only: torch's query, else the `rocm-smi --showclocks` line of device 0."""
    try:
        return f"{torch.cuda.clock_rate()} MHz"
    except Exception:
        pass
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        line = [l for l in out.splitlines() if "sclk" in l]
        return line[0].split(":", 2)[-1].strip() if line else "not measured"
    except Exception:
        return "not measured"


def timed(fns, calls):
    """{name: (median, min, max)} ms per call; the functions alternate inside every repetition."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in fns}
    for rep in range(WARM + REPS):
        for k, fn in fns.items():
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARM:
                ts[k].append(e0.elapsed_time(e1) / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def launches(iters, f16x3=True):
    """(Sinkhorn, dual softmax) kernel launches of one call without masks, and traversals of the L x S matrix."""
    front = 3 if f16x3 else 1                       # two plane conversions + the GEMM | sim_kernel
    skh = front + 1 + 2 * iters + 1 + 4   # row statistics, first rows + iters cols + (iters - 1) rows, conf, tail of 4
    dual = front + 2 + 1 + 4
    skh_pass = 1 + (0 if f16x3 else 2) + iters + (iters - 1) + 3    # write, [row statistics: 2 reads], cols, rows, conf: 2 reads + 1 write
    dual_pass = 1 + (0 if f16x3 else 4) + 1
    return skh, dual, skh_pass, dual_pass


def error_vs_fp64(dev):
    n, h, w = WORKLOADS[0]
    f0, f1 = features(n, h * w, dev)
    want = sinkhorn_cpu.conf_matrix(f0.cpu().double(), f1.cpu().double(), 1.0, 3, True)
    a64 = sinkhorn_cpu.assignment(f0.cpu().double(), f1.cpu().double(), 1.0, 3)
    rows, cols = sinkhorn_cpu.dustbin_margins(a64)
    out = []
    for prec in ("f16x3", "f32"):
        got = dense_match(f0, f1, (h, w), (h, w), (8 * h, 8 * w), match_type="sinkhorn", bin_score=torch.tensor(1.0, device=dev),
                          precision=prec)["conf_matrix"].cpu().double()
        same = (got == 0) == (want == 0)
        d = (got - want).abs()
        big = want > 1e-6
        out.append((prec, float(d.max()), float((d[big] / want[big]).max()), float((d / (1e-3 + want)).max()), int((~same).sum())))
    return out, float(rows.min()), float(cols.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinkhorn.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    bin_score = torch.tensor(1.0, device=dev)
    clock0 = clock_mhz()
    s15, d10, sp, dp = launches(3)
    lines = ["# Sinkhorn coarse matching against the dual softmax", "",
             "`python scripts/sinkhorn_time.py` on one MI355X, one process.  Device events around back-to-back `dense_match` calls",
             f"(each ends in its read-back of the match counts), {WARM} warm-up rounds, median (min .. max) of {REPS} repetitions,",
             "milliseconds per call; the matchers alternate inside every repetition.  C = 256, f16x3 contraction, planted features as in",
             "`synth.sinkhorn_case`; skh_iters = 3, bin_score = 1.0, prefilter on unless stated.", "",
             f"Launches per call (no masks): Sinkhorn {s15}, dual softmax {d10}.  Traversals of the L x S matrix: Sinkhorn {sp} (the",
             "contraction's write, 3 column passes, 2 row passes — iteration 1's row step comes from the contraction's statistics —",
             f"and the confidence pass: 2 reads, 1 write), dual softmax {dp} (+ 1 write when conf_matrix is published).", ""]
    notes = []
    for n, h, w in WORKLOADS:
        L = h * w
        f0, f1 = features(n, L, dev)
        args_ = (f0, f1, (h, w), (h, w), (8 * h, 8 * w))
        calls = 10 if n * L * L <= 4 << 20 else 3
        fns = {}
        for wc in (True, False):
            tag = "conf" if wc else "lists"
            fns[f"dual {tag}"] = lambda wc=wc: dense_match(*args_, want_conf=wc)
            fns[f"skh {tag}"] = lambda wc=wc: dense_match(*args_, want_conf=wc, match_type="sinkhorn", bin_score=bin_score)
        for it in (1, 5):
            fns[f"skh lists iters {it}"] = lambda it=it: dense_match(*args_, want_conf=False, match_type="sinkhorn",
                                                                      bin_score=bin_score, skh_iters=it)
        t = timed(fns, calls)
        m_d = int(dense_match(*args_, want_conf=False)["counts"].sum())
        m_s = int(dense_match(*args_, want_conf=False, match_type="sinkhorn", bin_score=bin_score)["counts"].sum())
        per_iter = (t["skh lists iters 5"][0] - t["skh lists iters 1"][0]) / 4
        mb = n * L * L * 4 / 1e6
        lines += [f"## {n} pair{'s' if n > 1 else ''} of {L} x {L} cells ({mb:.0f} MB of matrix)", "",
                  "| call | ms per call |", "|---|---|",
                  f"| dual softmax, conf_matrix published | {fmt(t['dual conf'])} |",
                  f"| Sinkhorn, conf_matrix published | {fmt(t['skh conf'])} |",
                  f"| dual softmax, match lists only | {fmt(t['dual lists'])} |",
                  f"| Sinkhorn, match lists only | {fmt(t['skh lists'])} |",
                  f"| Sinkhorn, lists only, skh_iters = 1 | {fmt(t['skh lists iters 1'])} |",
                  f"| Sinkhorn, lists only, skh_iters = 5 | {fmt(t['skh lists iters 5'])} |", "",
                  f"Ratio Sinkhorn / dual softmax: {t['skh conf'][0] / t['dual conf'][0]:.2f} published, "
                  f"{t['skh lists'][0] / t['dual lists'][0]:.2f} lists only.  One iteration (row pass + column pass): {per_iter:.3f} ms, "
                  f"{2 * mb / max(per_iter, 1e-9):.0f} GB/s of matrix reads.  Matches: dual softmax {m_d}, Sinkhorn {m_s}.", ""]
        ratio = t["skh lists"][0] / t["dual lists"][0]
        lines += [f"Against the pass counts ({sp} traversals to {dp}, {sp / dp:.1f}x): the measured ratio is {ratio:.2f}, "
                  + ("below it: the contraction that both calls share dominates, and nothing points at a pass that left its cache or at launch overhead."
                     if ratio <= sp / dp else "ABOVE it: a pass left the cache or the launches dominate; see the slope."), ""]
        extra = t["skh lists"][0] - t["dual lists"][0]
        notes.append(f"- {n} x {L}^2: Sinkhorn costs {extra:.3f} ms more than the dual softmax (lists only); its five row / column passes "
                     f"account for {2.5 * per_iter:.3f} ms by the slope above (2.5 iterations), the rest is the confidence pass's second "
                     f"sweep and its write, and {s15 - d10} more launches.")
    errs, rmin, cmin = error_vs_fp64(dev)
    lines += ["## Where the difference goes", ""] + notes + ["",
              "## Error against the fp64 definition", "",
              f"conf_matrix of the {WORKLOADS[0][0]} x 1024^2 workload against `sinkhorn_cpu.conf_matrix` in fp64 (the closest prefilter decision of",
              f"this input is {min(rmin, cmin):.2e} relative away from a tie):", "",
              "| contraction | max abs error | max relative error (conf > 1e-6) | max error / (1e-3 + conf): the tests' bound is 1e-4 | zero pattern mismatches |",
              "|---|---|---|---|---|"]
    lines += [f"| {p} | {a:.2e} | {r:.2e} | {b:.2e} | {z} |" for p, a, r, b, z in errs]
    lines += ["", f"Shader clock: {clock0} before, {clock_mhz()} after the run.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
