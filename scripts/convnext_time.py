"""Dev: device time of the ConvNeXtV2 backbone (`pope_amd.convnextv2`, csrc/convnext.hip) in both precisions, beside the same
parameters evaluated by torch ops on the same GPU (channels-first, restated below: what a user would run today), at
  convnextv2_large, 224 x 448, B = 8   (the shape pose/model_cnn.py runs: pose/dataset.py resizes to 224 x 224, the pair side by side)
  convnextv2_base,  224 x 224, B = 16
Prints markdown (`python scripts/convnext_time.py [--out FILE] [--small]`); the numbers live in profiles/convnext.md.

Method: device events around `calls` back-to-back forwards after 3 warm-up rounds; median (min .. max) of 7 repetitions, per call;
the contenders alternate inside every repetition.  The per-kernel split is one torch.profiler pass over 3 forwards per precision,
kernels grouped by name.  For the kernels of convnext.hip the table sets the group's time against its ALGORITHMIC bytes (every
input element read once, every output element written once, fp32; planes outputs are the same size), summed over the layers:
bytes / time is the rate the kernel achieves against the minimum, whatever it re-reads through the caches (the halo of dwconv7:
3.06 requests per element; the second and third pass of ln_rows over its row).  HBM counters were not read."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import convnextv2, synth  # noqa: E402

WARM, REPS = 3, 7
GROUPS = (("stem_gather", "stem_gather"), ("ln_rows", "ln_rows"), ("dwconv7", "dwconv7"), ("grn_partial", "grn_partial"),
          ("grn_colnorm", "grn_colnorm"), ("grn_finish", "grn_finish"), ("grn_apply", "grn_apply"), ("tail", "tail_kernel"), ("GEMMs", "gemm"), ("range scan", "range"))


def torch_forward(m, x):
    """The reference's forward (convnextv2.py:97-106) with torch ops on the module's own parameters."""
    def ln_cf(x, ln):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        return ln.weight[:, None, None] * ((x - u) / torch.sqrt(s + ln.eps)) + ln.bias[:, None, None]

    for i in range(4):
        a, b = m.downsample_layers[i]
        x = ln_cf(F.conv2d(x, a.weight, a.bias, stride=4), b) if i == 0 else F.conv2d(ln_cf(x, a), b.weight, b.bias, stride=2)
        for blk in m.stages[i]:
            y = F.conv2d(x, blk.dwconv.weight, blk.dwconv.bias, padding=3, groups=x.shape[1]).permute(0, 2, 3, 1)
            y = F.gelu(F.linear(F.layer_norm(y, (y.shape[-1],), blk.norm.weight, blk.norm.bias, 1e-6), blk.pwconv1.weight, blk.pwconv1.bias))
            gx = torch.norm(y, p=2, dim=(1, 2), keepdim=True)
            y = blk.grn.gamma * (y * (gx / (gx.mean(dim=-1, keepdim=True) + 1e-6))) + blk.grn.beta + y
            x = x + F.linear(y, blk.pwconv2.weight, blk.pwconv2.bias).permute(0, 3, 1, 2)
    return m.head(F.layer_norm(x.mean([-2, -1]), (x.shape[1],), m.norm.weight, m.norm.bias, 1e-6))


def timed(fns, calls):
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


def algorithmic_bytes(m, B, H, W):
    """fp32 bytes each kernel group of convnext.hip must move at least, summed over the layers."""
    out = dict.fromkeys(("stem_gather", "ln_rows", "dwconv7", "grn_partial", "grn_colnorm", "grn_finish", "grn_apply", "tail"), 0.0)
    M = B * (H // 4) * (W // 4)
    out["stem_gather"] = 2.0 * 4 * B * 3 * H * W
    out["ln_rows"] += 2.0 * 4 * M * m.dims[0]
    for i in range(4):
        c = m.dims[i]
        if i:
            out["ln_rows"] += 2.0 * 4 * M * m.dims[i - 1]
            M //= 4
        n = m.depths[i]
        out["dwconv7"] += n * 2.0 * 4 * M * c
        out["ln_rows"] += n * 2.0 * 4 * M * c
        out["grn_partial"] += n * 4.0 * M * 4 * c
        out["grn_apply"] += n * 2.0 * 4 * M * 4 * c
        out["grn_colnorm"] += n * 4.0 * B * 4 * c * (1 + -(-(M // B) // 64))
        out["grn_finish"] += n * 2.0 * 4 * B * 4 * c
    out["tail"] = 4.0 * (M + B) * m.dims[3]
    return out


def kernel_split(fn, n=3):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
    split = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if not t or getattr(ev, "device_type", None) is not None and "CPU" in str(ev.device_type):
            continue
        name = next((g for g, pat in GROUPS if pat in ev.key), "other")
        split[name] = split.get(name, 0.0) + t / n / 1e3     # ms per forward
    return split


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="convnextv2_tiny at 64 x 128, B = 2 (a dry run of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    shapes = [("convnextv2_tiny", 2, 64, 128)] if args.small else [("convnextv2_large", 8, 224, 448), ("convnextv2_base", 16, 224, 224)]
    lines = []
    for fac, B, H, W in shapes:
        first = len(lines)
        models = {}
        for prec in ("f32", "f16x3"):
            m = convnextv2.FACTORIES[fac](num_classes=32, precision=prec)
            m.load_state_dict(synth.convnext_state_dict(m.depths, m.dims, 32, seed=3), strict=True)
            models[prec] = m.to(dev)
        x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(5)).to(dev)
        outs = {p: m(x) for p, m in models.items()}
        ref = torch_forward(models["f32"], x)
        calls = 5
        res = timed({"f32": lambda: models["f32"](x), "f16x3": lambda: models["f16x3"](x), "torch": lambda: torch_forward(models["f32"], x)}, calls)
        lines += [f"### {fac}, {H} x {W}, B = {B}", "", "| path | ms per call | images / s | max abs diff of the logits vs torch ops |", "|---|---|---|---|"]
        for k in ("f32", "f16x3", "torch"):
            t = res[k]
            diff = "-" if k == "torch" else f"{float((outs[k] - ref).abs().max()):.2e}"
            lines.append(f"| {k} | {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) | {B / (t[0] * 1e-3):.0f} | {diff} |")
        lines.append(f"\noverflow events: {models['f16x3'].overflow_events}\n")
        alg = algorithmic_bytes(models["f32"], B, H, W)
        for prec in ("f32", "f16x3"):
            try:
                split = kernel_split(lambda: models[prec](x))
            except Exception as e:   # noqa: BLE001
                lines.append(f"per-kernel split ({prec}): not measured ({type(e).__name__}: {e})\n")
                continue
            total = sum(split.values())
            lines += [f"per-kernel split, {prec} (sum {total:.3f} ms of device time per forward):", "",
                      "| group | ms | share | algorithmic MB | algorithmic bytes / time |", "|---|---|---|---|---|"]
            for g, t in sorted(split.items(), key=lambda kv: -kv[1]):
                ab = alg.get(g)
                lines.append(f"| {g} | {t:.3f} | {100 * t / total:.1f} % | " + (f"{ab / 1e6:.1f} | {ab / (t * 1e-3) / 1e12:.2f} TB/s |" if ab else "- | - |"))
            lines.append("")
        print("\n".join(lines[first:]), flush=True)
        del models, x
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
