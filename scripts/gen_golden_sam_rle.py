"""Writes tests/golden/sam_rle.npz: the reference's `mask_to_rle_pytorch` (segment_anything/utils/amg.py, loaded by file path)
of seeded edge masks, for the device RLE (`pope_sam_rle_u32`, pope_amd/csrc/sam_rle.hip).  Run where the reference checkout
exists: `python scripts/gen_golden_sam_rle.py /path/to/reference`.  Needs torch and numpy only.

Shapes (H, W): (1, 1), (1, 70), (70, 1), (64, 32), (65, 33), (129, 95), (200, 100).  Patterns per shape: all-zero, all-one,
only the first pixel, only the last pixel, the last row of column 0 together with the first row of column 1 (a run that
crosses a column boundary; without a second column, the last row alone), a checkerboard and its complement, Bernoulli(0.5)
and a centred rectangle.  Stored per shape `HxW`: `HxW.packed` (uint32 words [9, H, ceil(W / 32)], the layout of
`sam_amg.pack_masks`), `HxW.counts` (int64, the masks' counts one after the other) and `HxW.lengths` (int64 [9]).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import sam_amg  # noqa: E402

SHAPES = ((1, 1), (1, 70), (70, 1), (64, 32), (65, 33), (129, 95), (200, 100))
PATTERNS = ("zero", "one", "first", "last", "crossing", "checker", "checker_inv", "bernoulli", "rectangle")


def edge_masks(H, W, seed):
    """bool [9, H, W] in the order of PATTERNS."""
    rng = np.random.default_rng(seed)
    m = np.zeros((len(PATTERNS), H, W), bool)
    m[1] = True
    m[2, 0, 0] = True
    m[3, H - 1, W - 1] = True
    m[4, H - 1, 0] = True
    if W > 1:
        m[4, 0, 1] = True
    yy, xx = np.mgrid[:H, :W]
    m[5] = (yy + xx) % 2 == 0
    m[6] = ~m[5]
    m[7] = rng.random((H, W)) < 0.5
    m[8, H // 4:H - H // 4, W // 4:W - W // 4] = True
    return m


def main():
    path = os.path.join(sys.argv[1], "segment_anything", "segment_anything", "utils", "amg.py")
    spec = importlib.util.spec_from_file_location("ref_amg", path)
    amg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(amg)
    blob = {}
    for s, (H, W) in enumerate(SHAPES):
        masks = edge_masks(H, W, seed=100 + s)
        rles = amg.mask_to_rle_pytorch(torch.as_tensor(masks))
        assert all(r["size"] == [H, W] for r in rles)
        for r, m in zip(rles, masks):     # the restatement the tests use agrees on these very cases
            assert sam_amg.mask_to_rle(m) == {"size": [H, W], "counts": [int(c) for c in r["counts"]]}
        key = f"{H}x{W}"
        blob[key + ".packed"] = sam_amg.pack_masks(masks)
        blob[key + ".counts"] = np.concatenate([np.asarray(r["counts"], np.int64) for r in rles])
        blob[key + ".lengths"] = np.asarray([len(r["counts"]) for r in rles], np.int64)
        print(key, "lengths", blob[key + ".lengths"].tolist())
    out = os.path.join(ROOT, "tests", "golden", "sam_rle.npz")
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
