#!/usr/bin/env python
"""Generate tests/golden/sam_decoder.npz by running the REFERENCE's own prompt encoder and mask decoder on the CPU
(segment_anything/modeling/{common,transformer,mask_decoder,prompt_encoder}.py, loaded by file path under a synthetic
package as oracle/gen_golden.py loads the image encoder; nothing under oracle/ is changed).

Weights: synth.synthetic_sam_decoder_state_dict(0); image embedding: synth.synthetic_sam_image_embedding(1); prompts:
synth.sam_decoder_case(name).  The fixture keeps outputs only (and the state-dict digest), tapped to fit the size budget:
  <case>_iou            iou_pred of every prompt
  <case>_taps           the tapped prompts ("grid": every 16th from prompt 0, and prompt 255; "box": all)
  <case>_maskbits       np.packbits(mask > 0) of every mask of the tapped prompts
  <case>_logit_rows     mask logits of the tapped prompts on the rows 0, ROW_TAP, 2 ROW_TAP, ... (stride coprime to 256)
  <case>_hs             the transformer's final tokens of the tapped prompts
  <case>_keys           final image tokens of two prompts (<case>_keys_prompts) on the rows 0, KEY_TAP, ...
  <case>_sparse         the reference PromptEncoder's sparse embeddings of every prompt
  dense_value           the dense embedding's value per channel (no_mask_embed)
  dense_pe_tap          get_dense_pe()[0, :, ::PE_TAP, ::PE_TAP]
  keys / shapes         the reference state dict's key list and shapes

Usage:  python scripts/gen_golden_sam_decoder.py            (from the repo root)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import OUT, REF, sd_digest  # noqa: E402
from pope_amd import synth  # noqa: E402

torch.set_num_threads(8)   # the thread count of every fixture (tests/conftest.py GOLDEN_THREADS)

ROW_TAP, KEY_TAP, PE_TAP = 67, 203, 21


def load_reference_decoder():
    base = os.path.join(REF, "segment_anything/segment_anything/modeling")
    pkg = types.ModuleType("ref_sam_modeling")
    pkg.__path__ = [base]
    sys.modules.setdefault("ref_sam_modeling", pkg)
    mods = {}
    for name in ("common", "transformer", "mask_decoder", "prompt_encoder"):
        spec = importlib.util.spec_from_file_location(f"ref_sam_modeling.{name}", os.path.join(base, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def reference_models(sd):
    m = load_reference_decoder()
    pe = m["prompt_encoder"].PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024),
                                           mask_in_chans=16)
    md = m["mask_decoder"].MaskDecoder(num_multimask_outputs=3,
                                       transformer=m["transformer"].TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048,
                                                                                      num_heads=8),
                                       transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256)
    pe.load_state_dict({k[len("prompt_encoder."):]: v for k, v in sd.items() if k.startswith("prompt_encoder.")}, strict=True)
    md.load_state_dict({k[len("mask_decoder."):]: v for k, v in sd.items() if k.startswith("mask_decoder.")}, strict=True)
    return pe.eval(), md.eval()


def run_case(pe, md, img, name):
    points, boxes, multimask = synth.sam_decoder_case(name)
    hs_keys = {}
    hook = md.transformer.register_forward_hook(lambda mod, inp, out: hs_keys.update(hs=out[0], keys=out[1]))
    with torch.no_grad():
        sparse, dense = pe(points=points, boxes=boxes, masks=None)
        masks, iou = md(image_embeddings=img, image_pe=pe.get_dense_pe(), sparse_prompt_embeddings=sparse,
                        dense_prompt_embeddings=dense, multimask_output=multimask)
    hook.remove()
    P = sparse.shape[0]
    taps = np.array(sorted(set(range(0, P, 16)) | {P - 1}) if name == "grid" else np.arange(P))
    kp = np.array([0, P - 1])
    out = {f"{name}_iou": iou.numpy(), f"{name}_taps": taps,
           f"{name}_maskbits": np.packbits(masks[taps].numpy() > 0, axis=-1),
           f"{name}_logit_rows": masks[taps][:, :, ::ROW_TAP, :].numpy(),
           f"{name}_hs": hs_keys["hs"][taps].numpy(), f"{name}_keys_prompts": kp,
           f"{name}_keys": hs_keys["keys"][kp][:, ::KEY_TAP, :].numpy(), f"{name}_sparse": sparse.numpy()}
    return out, dense


def main():
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    img = synth.synthetic_sam_image_embedding(seed=1)
    pe, md = reference_models(sd)
    data = {"digest": sd_digest(sd), "keys": np.array(sorted(sd)), "shapes": np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim())
                                                                                      for k in sorted(sd)])}
    for name in synth.SAM_DECODER_CASES:
        out, dense = run_case(pe, md, img, name)
        data.update(out)
        assert dense.stride(0) == 0   # the broadcast the shared layer-0 path keys on
        data["dense_value"] = dense[0, :, 0, 0].detach().numpy()
        print(name, {k: v.shape for k, v in out.items()})
    with torch.no_grad():
        data["dense_pe_tap"] = pe.get_dense_pe()[0, :, ::PE_TAP, ::PE_TAP].numpy()
    path = os.path.join(OUT, "sam_decoder.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
