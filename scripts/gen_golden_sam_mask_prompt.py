#!/usr/bin/env python
"""Generate tests/golden/sam_mask_prompt.npz by running the REFERENCE's own PromptEncoder and MaskDecoder with mask prompts on
the CPU (the modules `scripts/gen_golden_sam_decoder.py` loads by file path; nothing under oracle/ is changed).

Weights: synth.synthetic_sam_decoder_state_dict(0); image embedding: synth.synthetic_sam_image_embedding(1); prompts and masks:
synth.sam_mask_prompt_inputs(name) for the cases of synth.SAM_MASK_PROMPT_CASES ("box": 6 prompts of two points and a box,
single-mask output; "points": 17 prompts of one positive point, multimask output; one mask prompt each).  The fixture keeps
outputs only, tapped to fit the size budget:
  <case>_dense_prompts  the prompts whose dense embedding is kept ("box": 0, 3, 5; "points": 0, 16: the file stays under 1 MB)
  <case>_dense_tap      the dense (mask) embedding [P, 256, 64, 64] of those prompts tapped as [:, :, ::9, ::7]
  <case>_iou            iou_pred of every prompt
  <case>_logit_rows     mask logits of every prompt on the rows 0, 67, 134, 201
  <case>_maskbits       np.packbits(mask > 0) of every mask of every prompt
  digest                the state dict's digest

Usage:  python scripts/gen_golden_sam_mask_prompt.py            (from the repo root)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from oracle.gen_golden import OUT, sd_digest  # noqa: E402
from pope_amd import synth  # noqa: E402
from gen_golden_sam_decoder import reference_models  # noqa: E402

torch.set_num_threads(8)   # the thread count of every fixture (tests/conftest.py GOLDEN_THREADS)

ROW_TAP, TAP_Y, TAP_X = 67, 9, 7


def run_case(pe, md, img, name):
    points, boxes, masks, multimask = synth.sam_mask_prompt_inputs(name)
    with torch.no_grad():
        sparse, dense = pe(points=points, boxes=boxes, masks=masks)
        low, iou = md(image_embeddings=img, image_pe=pe.get_dense_pe(), sparse_prompt_embeddings=sparse,
                      dense_prompt_embeddings=dense, multimask_output=multimask)
    kept = np.array([0, 3, 5] if name == "box" else [0, dense.shape[0] - 1])
    return {f"{name}_dense_prompts": kept, f"{name}_dense_tap": dense[kept][:, :, ::TAP_Y, ::TAP_X].contiguous().numpy(),
            f"{name}_iou": iou.numpy(),
            f"{name}_logit_rows": low[:, :, ::ROW_TAP, :].contiguous().numpy(),
            f"{name}_maskbits": np.packbits(low.numpy() > 0, axis=-1)}


def main():
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    img = synth.synthetic_sam_image_embedding(seed=1)
    pe, md = reference_models(sd)
    data = {"digest": sd_digest(sd)}
    for name in synth.SAM_MASK_PROMPT_CASES:
        out = run_case(pe, md, img, name)
        data.update(out)
        print(name, {k: v.shape for k, v in out.items()})
    path = os.path.join(OUT, "sam_mask_prompt.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
