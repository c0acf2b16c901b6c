"""CPU: the public surface of `Sam.forward` and of the multi-image decoder entry (`pope_sam_decoder_forward_images_f32`):
prototypes, the arguments the entry rejects before any launch, the errors `Sam.forward` raises without a GPU, and the shape of
tests/golden/sam_forward.npz (the reference's own `Sam.forward` on `synth.sam_forward_case()`, written by
scripts/gen_golden_sam_forward.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pope_amd import _lib, synth
from test_sam_generator_cpu import small_sam

ROW_STEP = 8   # scripts/gen_golden_sam_forward.py


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sam_forward.npz"))


def test_prototypes_and_abi_version(hip_lib):
    assert "pope_sam_decoder_forward_images_f32" in _lib.PROTOTYPES
    assert "pope_sam_decoder_images_workspace_bytes" in _lib.PROTOTYPES
    assert hip_lib.pope_abi_version() == 10


def test_images_entry_rejects_bad_arguments_without_a_gpu(hip_lib):
    # every pointer of the weights is a fake non-NULL one: the only defect of each call below is the argument under test, and
    # every such call returns before a launch (the one call without a defect is never made: it would launch)
    w = _lib.SamDecoderWeights()
    layers = (_lib.SamDecoderLayerWeights * 2)()
    w.dim, w.heads, w.mlp_dim, w.depth, w.grid, w.num_mask_tokens, w.iou_hidden, w.iou_depth = 256, 8, 2048, 2, 64, 4, 256, 3
    w.precision = _lib.PREC_F16X3
    w.layers_host = C.cast(layers, C.POINTER(_lib.SamDecoderLayerWeights))
    fake = C.c_void_p(16)

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def query(N=4, which=ints(0, 3, 1), P=3, ns=2, ds=0, wp=C.byref(w)):
        return hip_lib.pope_sam_decoder_images_workspace_bytes(wp, N, which, P, ns, ds)

    def call(images=fake, N=4, which=ints(0, 3, 1), P=3, ns=2, ds=0, wp=C.byref(w)):
        return hip_lib.pope_sam_decoder_forward_images_f32(wp, images, N, fake, fake, which, P, ns, fake, ds, 1, fake, fake, fake,
                                                           1 << 40, None, None)
    assert query() > 0
    assert call(images=None) == -1                               # NULL images
    for bad in (dict(N=0), dict(N=-2), dict(which=ints(0, 4, 1)), dict(which=ints(0, -1, 1)), dict(which=None),
                dict(ds=256 * 4096), dict(ds=17), dict(P=0), dict(ns=12), dict(wp=None)):
        assert call(**bad) == -1, bad
        assert query(**bad) == 0, bad
    assert query(which=ints(0, 3, 3)) > 0                        # N - 1 is the last image
    # the layer-0 buffers are held once per image: 4 fp32 [4096, 256] and one [4096, 128]
    per_image = (4 * 4096 * 256 + 4096 * 128) * 4
    assert query(N=5) - query(N=4) == per_image and query(N=16) - query(N=4) == 12 * per_image
    # one image: what the single-image entry needs
    assert query(N=1, which=ints(0, 0, 0)) == hip_lib.pope_sam_decoder_workspace_bytes(C.byref(w), 3, 2, 1)
    for field, bad in (("dim", 128), ("depth", 3), ("precision", _lib.PREC_F16)):
        old = getattr(w, field)
        setattr(w, field, bad)
        assert call() == -1 and query() == 0, field
        setattr(w, field, old)


def test_forward_errors_without_a_gpu():
    sam, _ = small_sam()
    assert sam.forward([], True) == [] and sam([], multimask_output=False) == []
    case = synth.sam_forward_case()
    with pytest.raises(NotImplementedError, match="mask prompts"):
        sam([dict(case[0], mask_inputs=torch.zeros(2, 1, 256, 256))], True)
    with pytest.raises(_lib.PopeHipError):   # CPU tensors fail loudly
        sam(case, True)
    with pytest.raises(_lib.PopeHipError):
        sam.mask_decoder.forward_images(torch.zeros(2, 256, 64, 64), torch.zeros(1, 256, 64, 64), torch.zeros(1, 2, 256),
                                        torch.zeros(1, 256, 64, 64), [1], True)


def test_fixture_matches_the_case(golden_dir):
    g = golden(golden_dir)
    case = synth.sam_forward_case()
    assert len(case) == 2
    assert tuple(case[0]["image"].shape) == (3, 768, 1024) and tuple(case[0]["original_size"]) == (480, 640)
    assert tuple(case[1]["image"].shape) == (3, 1024, 683) and tuple(case[1]["original_size"]) == (600, 400)
    assert tuple(case[0]["boxes"].shape) == (2, 4) and "point_coords" not in case[0]
    assert tuple(case[1]["point_coords"].shape) == (3, 2, 2) and tuple(case[1]["point_labels"].shape) == (3, 2) and "boxes" not in case[1]
    for x in case:
        assert x["image"].dtype == torch.float32 and 0.0 <= float(x["image"].min()) and float(x["image"].max()) <= 255.0
    again = synth.sam_forward_case()
    assert all(torch.equal(a[k], b[k]) for a, b in zip(case, again) for k in a if isinstance(a[k], torch.Tensor))
    assert sorted(g.files) == sorted(f"{r}.{k}" for r in range(2) for k in ("iou_predictions", "low_res_rows", "low_res_shape", "masks_shape"))
    for r, x in enumerate(case):
        B = x["boxes"].shape[0] if "boxes" in x else x["point_coords"].shape[0]
        assert g[f"{r}.low_res_shape"].tolist() == [B, 3, 256, 256]
        assert g[f"{r}.masks_shape"].tolist() == [B, 3, *x["original_size"]]
        assert g[f"{r}.iou_predictions"].shape == (B, 3) and g[f"{r}.low_res_rows"].shape == (B, 3, 256 // ROW_STEP, 256)
        assert np.isfinite(g[f"{r}.low_res_rows"]).all() and float(np.abs(g[f"{r}.low_res_rows"]).max()) > 1.0
