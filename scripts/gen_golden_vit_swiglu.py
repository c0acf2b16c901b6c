#!/usr/bin/env python
"""Generate tests/golden/{vits_swiglu_224,vitg_224}.npz by running the REFERENCE's own `DinoVisionTransformer` with
ffn_layer="swiglufused" on the CPU (dinov2/dinov2/models/vision_transformer.py, layers/swiglu_ffn.py; imported read-only through
oracle/gen_golden.py's path set-up, nothing under oracle/ is changed).

Cases:
  vits_swiglu_224   384-d, 6 heads, depth 4, hidden 1 024: the width that takes the LayerNorm-fused residual GEMMs
  vitg_224          vit_giant2 (1536-d, 24 heads, 40 blocks, hidden 4 096; hubconf.py:79 / configs/eval/vitg14_pretrain.yaml)
                    at full depth: ~1.1 G parameters drawn from the seed (pope_amd.synth.synthetic_state_dict(ffn="swiglu")),
                    never stored
one 224 x 224 image each, every 8th token row.  The fixtures hold outputs only, with the fields of oracle/gen_golden.py's
gen_vit_archs() plus
  keys / shapes     the reference module's state-dict keys ('\\n'-joined, sorted) and their shapes (zero-padded to 4 dims)
  ref_fp32_err      max |fp32 - fp64| of the reference module itself (`model.double()` on the same input) over every stored
                    tensor: the noise floor the GPU bounds are read against; ref_fp32_err_fields has it per tensor, in the order
                    x_norm, x_prenorm, blk<tap 0>, blk<tap 1>, blk<tap 2>

Usage:  python scripts/gen_golden_vit_swiglu.py [case ...]            (from the repo root)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import OUT, REF, run_ref_vit, sd_digest  # noqa: E402,F401  (REF: the import path of the reference)
from pope_amd import synth  # noqa: E402

torch.set_num_threads(8)   # the thread count of every fixture (tests/conftest.py GOLDEN_THREADS)

CASES = {
    # name: (dim, depth, heads, row stride)
    "vits_swiglu_224": (384, 4, 6, 8),
    "vitg_224": (1536, 40, 24, 8),
}
EVAL_CFG = dict(patch_size=14, img_size=518, init_values=1e-5, ffn_layer="swiglufused", block_chunks=0)


def build_reference(name, dim, depth, heads):
    from dinov2.dinov2.models import vision_transformer as vits
    if name == "vitg_224":
        model = vits.vit_giant2(**EVAL_CFG)
        assert (model.embed_dim, model.n_blocks, model.num_heads) == (dim, depth, heads)
    else:
        model = vits.DinoVisionTransformer(embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4, **EVAL_CFG)
    return model.eval()


def stored(out, taps, tap_blocks, rows):
    xn = torch.cat([out["x_norm_clstoken"][:, None], out["x_norm_patchtokens"]], 1)
    d = {"x_norm": xn[:, rows], "x_prenorm": out["x_prenorm"][:, rows]}
    for i in tap_blocks:
        d[f"blk{i}"] = taps[f"blk{i}"][:, rows]
    return d


def gen(name):
    dim, depth, heads, stride = CASES[name]
    model = build_reference(name, dim, depth, heads)
    ref_sd = model.state_dict()
    keys = sorted(ref_sd)
    shapes = np.array([list(ref_sd[k].shape) + [0] * (4 - ref_sd[k].dim()) for k in keys], np.int32)
    sd = synth.synthetic_state_dict(seed=0, dim=dim, depth=depth, ffn="swiglu")
    digest = sd_digest(sd)
    model.load_state_dict(sd, strict=True)
    del sd, ref_sd
    H = W = 224
    x = synth.synthetic_images(1, H, W, seed=11)
    tap_blocks = (0, depth // 2, depth - 1)
    out, taps = run_ref_vit(model, x, tap_blocks)
    with torch.no_grad():
        cls = model(x).detach()
    ntok = 1 + (H // 14) * (W // 14)
    rows = torch.arange(0, ntok, stride)
    got = stored(out, taps, tap_blocks, rows)
    # the reference's own fp32 error: the same module in fp64 on the same input
    model.double()
    out64, taps64 = run_ref_vit(model, x.double(), tap_blocks)
    want = stored(out64, taps64, tap_blocks, rows)
    err = np.array([float((got[k].double() - want[k]).abs().max()) for k in got])
    print(name, "reference fp32 vs fp64:", {k: f"{e:.2e}" for k, e in zip(got, err)})
    fx = {"weights_seed": 0, "arch": np.array([dim, depth, heads]), "weights_digest": digest, "input_seed": 11,
          "shape": np.array([1, H, W]), "rows": rows.numpy(), "tap_blocks": np.array(tap_blocks),
          "input_digest": np.array([float(x.double().sum()), float(x.double().abs().sum())]),
          "cls": cls.numpy(), "keys": np.frombuffer("\n".join(keys).encode(), np.uint8), "shapes": shapes,
          "ref_fp32_err": np.float64(err.max()), "ref_fp32_err_fields": err}
    fx.update({k: v.numpy() for k, v in got.items()})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for case in sys.argv[1:] or CASES:
        gen(case)
