"""Writes tests/golden/sam_generator.npz: the reference's post-processing of the seeded synthetic decoder outputs of
`pope_amd.synth.sam_generator_case` (run where the reference checkout exists: `python scripts/gen_golden_sam_generator.py
/path/to/reference`).  The reference's own code does the work: `Sam.postprocess_masks` (called as a plain function on a stub
`self`), `calculate_stability_score`, `batched_mask_to_box` from segment_anything/utils/amg.py.  Box NMS is
`pope_amd.sam_amg.nms` (torchvision, which the reference calls, is not installed; the CPU test checks that no pair's IoU is
within 1e-4 of the threshold and no stability score within 1e-6 of its threshold, the two places a restatement decides).

Stored per case (results only; the tests regenerate the inputs from the seed): n_hi, n_lo, area, boxes and stability scores of
the masks that pass the IoU filter, the kept index lists after the IoU filter, the stability filter and NMS, and the NMS
survivors' masks bit-packed (row-major, 32 pixels per word).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import sam_amg, synth  # noqa: E402

PRED_IOU, STABILITY, OFFSET, NMS, THRESHOLD = 0.9, 0.95, 1.0, 0.35, 0.0


def load_reference(ref_root):
    base = os.path.join(ref_root, "segment_anything", "segment_anything")
    spec = importlib.util.spec_from_file_location("ref_amg", os.path.join(base, "utils", "amg.py"))
    amg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(amg)
    # modeling/sam.py imports its siblings relatively: give it a package of its own (torch only; no torchvision needed)
    pkg = types.ModuleType("ref_modeling")
    pkg.__path__ = [os.path.join(base, "modeling")]
    sys.modules["ref_modeling"] = pkg
    spec = importlib.util.spec_from_file_location("ref_modeling.sam", os.path.join(base, "modeling", "sam.py"))
    sam = importlib.util.module_from_spec(spec)
    sys.modules["ref_modeling.sam"] = sam
    spec.loader.exec_module(sam)
    return amg, sam.Sam


def run_case(name, amg, Sam):
    low, iou, input_size, original_size = synth.sam_generator_case(name)
    stub = types.SimpleNamespace(image_encoder=types.SimpleNamespace(img_size=1024))
    keep_iou = torch.nonzero(iou > PRED_IOU).reshape(-1)
    logits = Sam.postprocess_masks(stub, low[keep_iou][None], input_size, original_size)[0]
    n_hi = (logits > (THRESHOLD + OFFSET)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    n_lo = (logits > (THRESHOLD - OFFSET)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    stability = amg.calculate_stability_score(logits, THRESHOLD, OFFSET)
    assert torch.equal(torch.nan_to_num(stability, nan=-1.0), torch.nan_to_num(n_hi / n_lo, nan=-1.0))
    masks = logits > THRESHOLD
    boxes = amg.batched_mask_to_box(masks)
    area = masks.flatten(1).sum(1, dtype=torch.int32)
    sub = torch.nonzero(stability >= STABILITY).reshape(-1)
    keep_stab = keep_iou[sub]
    order = sam_amg.nms(boxes[sub].float().numpy(), iou[keep_stab].numpy(), NMS)
    keep_nms = keep_stab[torch.as_tensor(order)]
    survivors = masks[sub][torch.as_tensor(order)].numpy()
    rles = amg.mask_to_rle_pytorch(torch.as_tensor(survivors))
    out = {
        "n_hi": n_hi.numpy(), "n_lo": n_lo.numpy(), "area": area.numpy(), "boxes": boxes.numpy().astype(np.int32),
        "stability": stability.numpy().astype(np.float32), "keep_iou": keep_iou.numpy(), "keep_stability": keep_stab.numpy(),
        "keep_nms": keep_nms.numpy(), "packed": sam_amg.pack_masks(survivors),
        "rle_counts": np.concatenate([np.asarray(r["counts"], np.int64) for r in rles]),
        "rle_lengths": np.asarray([len(r["counts"]) for r in rles], np.int64),
    }
    print(name, "M", len(iou), "iou", len(keep_iou), "stability", len(keep_stab), "nms", len(keep_nms),
          "empty", int((area == 0).sum()), "stability range", float(np.nanmin(out["stability"])), float(np.nanmax(out["stability"])))
    return {f"{name}.{k}": v for k, v in out.items()}


def main():
    amg, Sam = load_reference(sys.argv[1])
    torch.set_num_threads(8)
    blob = {}
    for name in synth.SAM_GENERATOR_CASES:
        blob.update(run_case(name, amg, Sam))
    path = os.path.join(ROOT, "tests", "golden", "sam_generator.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
