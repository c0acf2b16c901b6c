"""Dev: device time of the learned pose regressor (`regress_pose_batch`, csrc/pose_regressor.hip) at num_sample S in {300, 500} and
B in {1, 8, 16} pairs per call, beside the same state dict evaluated by plain torch.nn modules on the same GPU (a
TransformerEncoder plus a Sequential, restated below: what a user would run today).  Prints a markdown table
(`python scripts/pose_regressor_time.py [--out FILE] [--sizes 300,500]`); the numbers live in profiles/pose_regressor.md.

Method: device events around `calls` back-to-back calls after 3 warm-up rounds; median (min .. max) of 7 repetitions, per call;
the contenders alternate inside every repetition.  Launch groups of the HIP call are differences of its early-stop entries:
embedding = select + embed; encoder = the four layer launches; mlp = the two streamed Linears (mlp.0, mlp.3) + the tail.
The bytes/s figure divides the fp32 bytes of the mlp.0 and mlp.3 weights (each read once per chunk of 8 pairs) by the WHOLE
mlp group's time, so it is a lower bound on what mlp.0 alone achieves.
torch twin, two ways: 'loop' = one `net(x[b:b+1])` call per pair, as the reference notebooks do; 'folded' = all pairs in one
call with the pairs folded into the encoder's batch axis ([1, B S, 76]: every pair on its own, like the HIP call)."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import synth  # noqa: E402
from pope_amd.pose_regressor import ROW_CHUNK, Mkpts_Reg_Model, regress_pose_batch  # noqa: E402

WARM, REPS = 3, 7


class TorchTwin(nn.Module):
    """pose/model.py:Mkpts_Reg_Model restated with torch.nn modules (mode 'matrix'); loads the same state dict."""

    def __init__(self, S):
        super().__init__()
        self.transformerlayer = nn.TransformerEncoderLayer(d_model=76, nhead=2)
        self.transformer = nn.TransformerEncoder(self.transformerlayer, num_layers=4, enable_nested_tensor=False)
        self.translation_head, self.rotation_head = nn.Linear(32, 3), nn.Linear(32, 9)
        widths = [76 * S, 19 * S, S, 256, 128, 64, 32, 32]
        layers = []
        for i in range(7):
            layers += [nn.Linear(widths[i], widths[i + 1]), nn.LeakyReLU(), nn.Dropout(0.1)]
        self.mlp = nn.Sequential(*layers)
        self.register_buffer("freqs", torch.linspace(1, 256, 9), persistent=False)

    def embed(self, x):
        out = [x]
        for f in self.freqs:
            out += [torch.sin(f * x), torch.cos(f * x)]
        return torch.cat(out, dim=-1)

    def head(self, enc, B):
        y = self.mlp(enc.reshape(B, -1))
        return self.translation_head(y), self.rotation_head(y).view(B, 3, 3)

    def loop(self, k0, k1):
        outs = [self.head(self.transformer(self.embed(torch.cat((k0[b:b + 1], k1[b:b + 1]), -1))), 1) for b in range(k0.shape[0])]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])

    def folded(self, k0, k1):
        B, S = k0.shape[:2]
        x = self.embed(torch.cat((k0, k1), -1)).reshape(1, B * S, 76)
        return self.head(self.transformer(x).reshape(B, S, 76), B)


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


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="300,500")
    ap.add_argument("--pairs", default="1,8,16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    lines = ["| S | B | HIP call ms | embedding | encoder | mlp (stream + tail) | mlp.0 + mlp.3 weight bytes / mlp time | torch folded ms | torch loop ms | max abs diff t, R vs torch |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for S in (int(s) for s in args.sizes.split(",")):
        sd = synth.pose_regressor_state_dict(S, "matrix")
        model = Mkpts_Reg_Model(S, "matrix")
        model.load_state_dict(sd, strict=True)
        model = model.to(dev)
        twin = TorchTwin(S).eval()
        twin.load_state_dict(sd, strict=True)
        twin = twin.to(dev)
        del sd
        wbytes = 4.0 * (19 * S * 76 * S + S * 19 * S)
        for B in (int(b) for b in args.pairs.split(",")):
            counts = [S] * B
            k0, k1 = (t.to(dev) for t in synth.pose_regressor_matches(counts, seed=B))
            d0, d1 = k0.view(B, S, 2), k1.view(B, S, 2)
            cdev = torch.tensor(counts, dtype=torch.int32, device=dev)
            out = regress_pose_batch(model, k0, k1, cdev)
            tt, tR = twin.folded(d0, d1)
            diff = (float((out["t"] - tt).abs().max()), float((out["R"] - tR).abs().max()))
            calls = 20
            res = timed({"hip": lambda: regress_pose_batch(model, k0, k1, cdev),
                         "emb": lambda: regress_pose_batch(model, k0, k1, cdev, stage="embedding"),
                         "enc": lambda: regress_pose_batch(model, k0, k1, cdev, stage="encoder"),
                         "folded": lambda: twin.folded(d0, d1), "loop": lambda: twin.loop(d0, d1)}, calls)
            enc = res["enc"][0] - res["emb"][0]
            mlp = res["hip"][0] - res["enc"][0]
            chunks = (B + ROW_CHUNK - 1) // ROW_CHUNK
            lines.append(f"| {S} | {B} | {fmt(res['hip'])} | {res['emb'][0]:.3f} | {enc:.3f} | {mlp:.3f} | "
                         f"{chunks * wbytes / (mlp * 1e-3) / 1e12:.2f} TB/s | {fmt(res['folded'])} | {fmt(res['loop'])} | "
                         f"{diff[0]:.2e}, {diff[1]:.2e} |")
            print(lines[-1], flush=True)
        del model, twin
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
