"""Dev: device time of the LoFTR encoder layer and transformer with linear against full (softmax) attention on the HIP
kernels (loftr.hip, loftr_attention.hip), and of a torch restatement of the reference's full-attention body (einsum, softmax,
einsum, fp32: linear_attention.py:69-81) on the same GPU in the same process.  Writes profiles/loftr_full.md
(`python scripts/loftr_full_time.py [--out FILE]`).

Method: device events around `calls` back-to-back calls after 3 warm-up rounds; median (min .. max) of 9 repetitions, per call.
A layer update is `LoFTREncoderLayer.update_` (one C-ABI call, no synchronisation); a transformer is
`LocalFeatureTransformer.forward` (its range-flag read included)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import _lib, synth  # noqa: E402
from pope_amd.loftr import LocalFeatureTransformer  # noqa: E402
from pope_amd.matcher import default_cfg  # noqa: E402

SHAPES = [("coarse", 6, 1024), ("coarse", 2, 4800), ("fine", 700, 25)]   # (stage, n sequences per stream, L = S)
WARM, REPS = 3, 9


def dev_time(fn, calls, reset=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for rep in range(WARM + REPS):
        if reset is not None:
            reset()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARM:
            ts.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "not measured" if t is None else f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def transformer(stage, attention, dev):
    t = LocalFeatureTransformer(dict(default_cfg[stage], attention=attention)).eval()
    prefix = f"loftr_{stage}."
    sd = synth.synthetic_matcher_state_dict(0)
    t.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    return t.to(dev)


def torch_attention(q, k, v):
    """The reference's FullAttention body."""
    qk = torch.einsum("nlhd,nshd->nlsh", q, k)
    a = torch.softmax((1.0 / q.size(3) ** 0.5) * qk, dim=2)
    return torch.einsum("nlsh,nshd->nlhd", a, v).contiguous()


def torch_layer(layer, x, source):
    """The reference's layer (transformer.py:35-58) with that body, on the layer's own parameters."""
    n, d, h = x.size(0), x.size(2), layer.nhead
    q = layer.q_proj(x).view(n, -1, h, d // h)
    k = layer.k_proj(source).view(n, -1, h, d // h)
    v = layer.v_proj(source).view(n, -1, h, d // h)
    msg = layer.norm1(layer.merge(torch_attention(q, k, v).view(n, -1, d)))
    return x + layer.norm2(layer.mlp(torch.cat([x, msg], dim=2)))


def hip_core(q, kv, out, precision):
    n, L, Cd = q.shape
    _lib.check(_lib.lib().pope_loftr_full_attention_f32(
        C.c_void_p(q.data_ptr()), C.c_void_p(kv.data_ptr()), n, L, kv.shape[1], Cd, 8, _lib.PRECISIONS[precision],
        C.c_void_p(out.data_ptr()), None, _lib.stream_of(q.device)), "pope_loftr_full_attention_f32")


def measure(stage, n, L, dev):
    tl, tf = transformer(stage, "linear", dev), transformer(stage, "full", dev)
    Cd = tl.d_model
    g = torch.Generator().manual_seed(7)
    f0, f1 = torch.randn(n, L, Cd, generator=g).to(dev), torch.randn(n, L, Cd, generator=g).to(dev)
    calls = 10 if L >= 1024 else 20
    rows = {}
    # one layer update ('self' of one stream: n sequences)
    x0 = f0.clone()
    x = x0.clone()
    ws = torch.empty(_lib.lib().pope_loftr_layer_workspace_bytes(n, L, L, Cd, 8), dtype=torch.uint8, device=dev)
    for name, t in (("linear", tl), ("full", tf)):
        for prec in ("f16x3", "f32"):
            layer = t.layers[0]
            with torch.cuda.device(dev):
                rows[f"layer {name} {prec}"] = dev_time(lambda: layer.update_(x, x, ws, prec), calls, lambda: x.copy_(x0))
    with torch.no_grad():
        rows["layer full torch"] = dev_time(lambda: torch_layer(tf.layers[0], x0, x0), calls)
        # the attention core alone
        layer = tf.layers[0]
        q = layer.q_proj(x0).contiguous()
        kv = torch.cat([layer.k_proj(x0), layer.v_proj(x0)], 2).contiguous()
        out = torch.empty_like(q)
        with torch.cuda.device(dev):
            rows["core full hip"] = dev_time(lambda: hip_core(q, kv, out, "f32"), calls)
        h = lambda t: t.reshape(n, L, 8, Cd // 8)   # noqa: E731
        qh, kh, vh = h(q), h(kv[..., :Cd]), h(kv[..., Cd:])
        rows["core full torch"] = dev_time(lambda: torch_attention(qh, kh, vh), calls)
        err = float((out.view_as(qh) - torch_attention(qh, kh, vh)).abs().max())
        # the whole transformer (both streams)
        rows["transformer linear"] = dev_time(lambda: tl(f0, f1), max(2, calls // 4))
        rows["transformer full"] = dev_time(lambda: tf(f0, f1), max(2, calls // 4))
    return rows, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loftr_full.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    lines = ["# LoFTR layers: linear against full (softmax) attention", "",
             "`python scripts/loftr_full_time.py` on one MI355X, one process.  Device events around back-to-back calls (10 at the",
             f"coarse shapes, 20 at the fine one; a quarter of that for whole transformers), {WARM} warm-up rounds, median (min .. max) of",
             f"{REPS} repetitions, milliseconds per call.  Weights: `synth.synthetic_matcher_state_dict(0)`; inputs randn.", "",
             "Routes of the HIP rows: `f16x3` = the five Linears on the f16x3 planes GEMM, `f32` = on the fp32 MFMA (the range",
             "guard's re-run).  The full-attention core itself is the same under both: the fp32-MFMA flash kernel for S > 64 (the",
             "two coarse shapes), the fp32 vector kernel for S <= 64 (the fine windows); there is no f16x3 attention variant.  The",
             "torch rows are the reference's body restated in torch (einsum, softmax, einsum; fp32) on the same card.", ""]
    verdicts = []
    for stage, n, L in SHAPES:
        rows, err = measure(stage, n, L, dev)
        lines += [f"## {stage}: n = {n} sequences, L = S = {L}, C = {256 if stage == 'coarse' else 128}", "",
                  "| what | route | ms per call |", "|---|---|---|",
                  f"| layer update, linear attention | f16x3 | {fmt(rows['layer linear f16x3'])} |",
                  f"| layer update, linear attention | f32 | {fmt(rows['layer linear f32'])} |",
                  f"| layer update, full attention | f16x3 GEMMs + fp32 attention kernel | {fmt(rows['layer full f16x3'])} |",
                  f"| layer update, full attention | f32 GEMMs + fp32 attention kernel | {fmt(rows['layer full f32'])} |",
                  f"| layer, full attention, torch restatement | torch fp32 | {fmt(rows['layer full torch'])} |",
                  f"| attention core alone, HIP | fp32 attention kernel | {fmt(rows['core full hip'])} |",
                  f"| attention core alone, torch restatement | torch fp32 | {fmt(rows['core full torch'])} |",
                  f"| transformer ({len(default_cfg[stage]['layer_names'])} layers, both streams), linear | f16x3 | {fmt(rows['transformer linear'])} |",
                  f"| transformer ({len(default_cfg[stage]['layer_names'])} layers, both streams), full | f16x3 GEMMs + fp32 attention kernel | {fmt(rows['transformer full'])} |",
                  "", f"HIP core against the torch restatement on this input: max abs difference {err:.2e}.", ""]
        if stage == "coarse":
            hip, ref = rows["layer full f16x3"], rows["layer full torch"]
            verdicts.append(f"- n = {n}, L = S = {L}: HIP full layer {hip[0]:.3f} ms (max {hip[2]:.3f}) against the torch restatement "
                            f"{ref[0]:.3f} ms (min {ref[1]:.3f}): {'not slower' if hip[2] <= ref[1] else ('not slower by the medians' if hip[0] <= ref[0] else 'SLOWER')}")
    lines += ["## Yardstick", "", "The HIP full-attention layer against the torch restatement of the reference's layer, same card, same process:", ""]
    lines += verdicts + [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
