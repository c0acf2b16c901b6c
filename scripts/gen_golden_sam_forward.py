"""Writes tests/golden/sam_forward.npz: the reference's own `Sam.forward` (segment_anything/modeling/sam.py:53-131) on
`pope_amd.synth.sam_forward_case()`, on the CPU (run where the reference checkout exists: `python
scripts/gen_golden_sam_forward.py /path/to/reference`).  The reference's `modeling` package is loaded by file path and
does all the work; the model is the reference `Sam` at the geometry of tests/test_sam_generator_cpu.py:small_sam(depth=2)
(ViT-B widths, two blocks, global attention in block 1) under the same synthetic state dict, loaded with strict=True.

Stored per record r (results only; the tests regenerate the inputs from the seed): `r.iou_predictions`, `r.low_res_rows` =
every 8th row of `low_res_logits`, `r.low_res_shape` and `r.masks_shape`; `multimask_output=True`.
"""
import importlib.util
import os
import sys
import types
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import synth  # noqa: E402

ROW_STEP, DEPTH = 8, 2


def load_reference(ref_root):
    base = os.path.join(ref_root, "segment_anything", "segment_anything", "modeling")
    # the modules import their siblings relatively: give them a package of their own (torch only)
    pkg = types.ModuleType("ref_modeling")
    pkg.__path__ = [base]
    sys.modules["ref_modeling"] = pkg
    mods = {}
    for name in ("common", "image_encoder", "prompt_encoder", "transformer", "mask_decoder", "sam"):
        spec = importlib.util.spec_from_file_location("ref_modeling." + name, os.path.join(base, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["ref_modeling." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods


def reference_sam(m):
    enc = m["image_encoder"].ImageEncoderViT(depth=DEPTH, embed_dim=768, img_size=1024, mlp_ratio=4,
                                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_heads=12, patch_size=16,
                                             qkv_bias=True, use_rel_pos=True, global_attn_indexes=[1], window_size=14, out_chans=256)
    pe = m["prompt_encoder"].PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024), mask_in_chans=16)
    md = m["mask_decoder"].MaskDecoder(num_multimask_outputs=3,
                                       transformer=m["transformer"].TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                                       transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    sam = m["sam"].Sam(enc, pe, md)
    sd = {"image_encoder." + k: v for k, v in synth.synthetic_sam_encoder_state_dict(seed=0, dim=768, depth=DEPTH, heads=12,
                                                                                      global_idx=(1,)).items()}
    sd.update(synth.synthetic_sam_decoder_state_dict(seed=0))
    sam.load_state_dict(sd, strict=True)
    return sam.eval()


def main():
    sam = reference_sam(load_reference(sys.argv[1]))
    torch.set_num_threads(8)
    out = sam(synth.sam_forward_case(), multimask_output=True)
    blob = {}
    for r, o in enumerate(out):
        low = o["low_res_logits"]
        blob[f"{r}.iou_predictions"] = o["iou_predictions"].numpy()
        blob[f"{r}.low_res_rows"] = low[:, :, ::ROW_STEP].numpy()
        blob[f"{r}.low_res_shape"] = np.asarray(low.shape, np.int64)
        blob[f"{r}.masks_shape"] = np.asarray(o["masks"].shape, np.int64)
        assert o["masks"].dtype == torch.bool
        print(r, "iou", o["iou_predictions"].flatten().tolist(), "max |logit|", float(low.abs().max()),
              "mask fill", float(o["masks"].float().mean()))
    path = os.path.join(ROOT, "tests", "golden", "sam_forward.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
