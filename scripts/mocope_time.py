"""Times the MoCoPE fusion pose model (pope_amd/mocope.py) on the GPU beside a PyTorch-ROCm eager restatement with the same
weights on the same card, and prints the markdown table of profiles/mocope.md:  python scripts/mocope_time.py [--out FILE]

Shapes: num_sample S = 500 (the reference's), the group call at B = 2 (the reference's batch) and the pipeline form (every pair
on its own) at B = 1, 8 and 24.  Per shape: the part after the backbone (the backbone's logits are computed once, outside the
timed region) and the whole forward (small trunk `synth.MOCOPE_TRUNK` on 64 x 64 images: the backbone is not what this measures).
Method: 3 warm-up calls, then REPEATS repeats of ITERS back-to-back calls between two events; reported: the median over the
repeats of the per-call time, and the spread (min .. max).  The eager side is `torch.nn.Transformer` / `nn.Linear` in fp32 with
TF32 off.  Weight traffic: the bytes of every weight the non-backbone part reads once per call, over the time, as a fraction of
the card's copy bandwidth measured here (a 1 GiB device-to-device copy: read + write bytes over the time).
"""
import argparse
import statistics
import sys
import os

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pope_amd import convnextv2, synth  # noqa: E402
from pope_amd import mocope as M  # noqa: E402

S, REPEATS, ITERS = 500, 7, 5


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / ITERS)
    return statistics.median(times), min(times), max(times)


def copy_bandwidth():
    n = 1 << 30
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    ms = timed(lambda: dst.copy_(src))[0]
    return 2 * n / (ms * 1e-3)


class Eager(nn.Module):
    """model0604.py:MoCoPE.forward after the backbone, restated with torch modules that share the HIP model's parameters."""

    def __init__(self, m):
        super().__init__()
        self.m = m
        self.freq = torch.linspace(1, 256, 9)

    def forward(self, k0, k1, f0, f1, grouped):
        m = self.m
        x = torch.cat((k0, k1), dim=-1)
        x = torch.cat([x] + [fn(f * x) for f in self.freq.tolist() for fn in (torch.sin, torch.cos)], dim=-1)      # [B, S, 76]
        if not grouped:          # every pair on its own: the pairs become the batch dimension of a sequence of one
            x = x.reshape(1, -1, 76)
        x = m.transformer_mkpts(x, x).reshape(k0.shape[0], -1)
        xm = m.mlp1(x).reshape(-1, 2, 512)
        xi = torch.stack((m.mlp_img(f0), m.mlp_img(f1)), dim=1)
        if not grouped:
            xm, xi = xm.reshape(1, -1, 512), xi.reshape(1, -1, 512)
        y = torch.cat((m.mkpts_as_q(xi, xm), m.cnn_as_q(xm, xi)), dim=-1).reshape(k0.shape[0], -1)
        y = m.mlp2(y)
        return m.translation_head(y), m.rotation_head(y)


def weight_bytes(m, grouped):
    """fp32 bytes of the parameters one call reads outside the backbone (a group of one skips the q | k thirds of in_proj)"""
    n = 0
    for k, v in m.state_dict().items():
        if k.startswith("convnextv2."):
            continue
        n += v.numel() * 4 // (3 if (not grouped and "in_proj" in k) else 1)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    model = M.MoCoPE(S, "6d", backbone=convnextv2.ConvNeXtV2(**synth.MOCOPE_TRUNK))
    model.load_state_dict(synth.mocope_state_dict(S, "6d"), strict=True)
    model = model.to(dev)
    eager = Eager(model)
    bw = copy_bandwidth()
    lines = [f"copy bandwidth measured here: {bw / 1e12:.2f} TB/s (1 GiB device-to-device copy, read + write)", "",
             "| form | B | HIP after backbone ms (min .. max) | eager after backbone ms (min .. max) | HIP / eager | HIP whole forward ms | "
             "weights read MB | HIP weight traffic, share of copy bandwidth |", "|---|---|---|---|---|---|---|---|"]
    for grouped, B in ((True, 2), (False, 1), (False, 8), (False, 24)):
        counts = [S] * B
        k0, k1 = (t.to(dev) for t in synth.pose_regressor_matches(counts, seed=B))
        d0, d1 = k0.reshape(B, S, 2), k1.reshape(B, S, 2)
        g = torch.Generator().manual_seed(B)
        i0, i1 = (torch.randn(B, 3, 64, 64, generator=g).to(dev) for _ in range(2))
        f0, f1 = model._images(i0, i1, B, "mocope_time")
        cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
        seeds = torch.zeros(B, dtype=torch.int64, device=dev)
        if grouped:
            after = lambda: M._run(model, None, B, B, f0, f1, dense=(d0, d1))  # noqa: E731
            whole = lambda: model(d0, d1, i0, i1)  # noqa: E731
        else:
            after = lambda: M._run(model, None, B, 1, f0, f1, compact=(k0, k1, cnt), seeds=seeds)  # noqa: E731
            whole = lambda: M.regress_pose_fused_batch(model, k0, k1, cnt, i0, i1)  # noqa: E731
        with torch.no_grad():
            ref = lambda: eager(d0, d1, f0, f1, grouped)  # noqa: E731
            # the two sides compute the same thing before they are timed
            t_hip, t_ref = after()["t"], ref()[0]
            assert float((t_hip - t_ref).abs().max()) < 1e-3 * max(1.0, float(t_ref.abs().max())), (B, t_hip, t_ref)
            h, e, w = timed(after), timed(ref), timed(whole)
        nbytes = weight_bytes(model, grouped)
        lines.append(f"| {'group call' if grouped else 'pipeline'} | {B} | {h[0]:.2f} ({h[1]:.2f} .. {h[2]:.2f}) | {e[0]:.2f} ({e[1]:.2f} .. {e[2]:.2f}) | "
                     f"{h[0] / e[0]:.2f} | {w[0]:.2f} | {nbytes / 1e6:.0f} | {nbytes / (h[0] * 1e-3) / bw:.1%} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
