"""CPU: the public surface of SAM mask prompts (`pope_sam_mask_embed_f32`, `PromptEncoder.forward(masks=)`, the predictor's
`mask_input`, `Sam.forward` records with `mask_inputs`): the prototype, the arguments the entry rejects before any launch, the
errors raised without a GPU, and the torch restatement of the mask embedding the GPU tests compare against, pinned here to the
reference's own outputs (tests/golden/sam_mask_prompt.npz, scripts/gen_golden_sam_mask_prompt.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pope_amd import _lib, synth
from pope_amd.sam_generator import SamPredictor
from test_sam_decoder_cpu import build_models
from test_sam_generator_cpu import small_sam

ROW_TAP, TAP_Y, TAP_X = 67, 9, 7   # scripts/gen_golden_sam_mask_prompt.py
WEIGHTS = ("conv1_w", "conv1_b", "ln1_w", "ln1_b", "conv2_w", "conv2_b", "ln2_w", "ln2_b", "conv3_w", "conv3_b")


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sam_mask_prompt.npz"))


# ---- torch restatement (prompt_encoder.py:51-59, 102-105; common.py LayerNorm2d) ---------------------------------------
def _ln2d(x, w, b, eps):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + eps)
    return w[:, None, None] * x + b[:, None, None]


def restate_embed(sd, masks, dtype=torch.float32, eps=1e-6):
    """PromptEncoder._embed_masks in torch at `dtype` on the masks' device: [P, 1, 256, 256] -> [P, 256, 64, 64]."""
    w = {k[len("prompt_encoder.mask_downscaling."):]: v.to(device=masks.device, dtype=dtype) for k, v in sd.items()
         if k.startswith("prompt_encoder.mask_downscaling.")}
    x = F.conv2d(masks.to(dtype), w["0.weight"], w["0.bias"], stride=2)
    x = F.gelu(_ln2d(x, w["1.weight"], w["1.bias"], eps))
    x = F.conv2d(x, w["3.weight"], w["3.bias"], stride=2)
    x = F.gelu(_ln2d(x, w["4.weight"], w["4.bias"], eps))
    return F.conv2d(x, w["6.weight"], w["6.bias"])


# ---- the C entry -------------------------------------------------------------------------------------------------------
def test_prototype_and_abi_version(hip_lib):
    assert "pope_sam_mask_embed_f32" in _lib.PROTOTYPES
    assert hip_lib.pope_abi_version() == 10


def test_entry_rejects_bad_arguments_without_a_gpu(hip_lib):
    # every pointer is a fake non-NULL one (16-byte aligned, never dereferenced): the only defect of each call below is the
    # argument under test, and every such call returns before a launch (the one call without a defect is never made)
    fake = C.c_void_p(16)

    def weights(**over):
        w = _lib.SamMaskEmbedWeights()
        w.mask_in_chans, w.embed_dim, w.grid, w.ln1_eps, w.ln2_eps = 16, 256, 64, 1e-6, 1e-6
        for name in WEIGHTS:
            setattr(w, name, fake)
        for k, v in over.items():
            setattr(w, k, v)
        return w

    def call(w=None, wp=True, masks=fake, P=3, dense=fake):
        w = w or weights()
        return hip_lib.pope_sam_mask_embed_f32(C.byref(w) if wp else None, masks, P, dense, None)
    assert call(wp=False) == -1
    assert call(masks=None) == -1 and call(dense=None) == -1
    for name in WEIGHTS:
        assert call(weights(**{name: None})) == -1, name
    for P in (0, -1):
        assert call(P=P) == -1, P
    for field, bad in (("mask_in_chans", 8), ("embed_dim", 128), ("grid", 32)):
        assert call(weights(**{field: bad})) == -1, field
    assert call(masks=C.c_void_p(20)) == -1 and call(dense=C.c_void_p(24)) == -1   # not 16-byte aligned


# ---- errors without a GPU ----------------------------------------------------------------------------------------------
def test_a_cpu_mask_raises_everywhere():
    pe, _ = build_models()
    m = torch.zeros(2, 1, 256, 256)
    with pytest.raises(NotImplementedError, match="mask prompts"):
        pe(points=None, boxes=None, masks=m)
    with pytest.raises(NotImplementedError, match="mask prompts"):   # before any other check: the boxes are on the CPU too
        pe(points=None, boxes=torch.zeros(2, 4), masks=m)
    sam, _ = small_sam()
    predictor = SamPredictor(sam)
    with pytest.raises(NotImplementedError, match="mask prompts"):   # before "an image must be set"
        predictor.predict_torch(None, None, None, mask_input=m)
    with pytest.raises(NotImplementedError, match="mask prompts"):
        predictor.predict(mask_input=np.zeros((1, 256, 256), np.float32))
    case = synth.sam_forward_case()
    with pytest.raises(NotImplementedError, match="mask prompts"):
        sam([case[0], dict(case[1], mask_inputs=torch.zeros(3, 1, 256, 256))], True)


def test_wrong_shape_and_dtype_raise():
    # `forward` looks at the mask's device first (above), so without a GPU the shape and dtype checks are reached through the
    # method `forward` calls for them; tests/test_gpu_sam_mask_prompt.py reaches them through `forward` itself
    pe, _ = build_models()
    with pytest.raises(ValueError, match="masks"):
        pe._check_masks(torch.zeros(2, 256, 256))
    with pytest.raises(ValueError, match="masks"):
        pe._check_masks(torch.zeros(2, 1, 128, 128))
    with pytest.raises(TypeError, match="masks"):
        pe._check_masks(torch.zeros(2, 1, 256, 256, dtype=torch.float64))
    pe._check_masks(torch.zeros(2, 1, 256, 256))
    with pytest.raises(NotImplementedError, match="mask prompts"):   # the order `forward` documents
        pe(points=None, boxes=None, masks=torch.zeros(2, 256, 256))
    with pytest.raises(TypeError, match="mask prompt"):
        pe(points=None, boxes=None, masks=np.zeros((1, 1, 256, 256), np.float32))


# ---- the fixture and the restatement -----------------------------------------------------------------------------------
def test_fixture_matches_the_synthetic_case(golden_dir):
    g = golden(golden_dir)
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    assert np.array_equal(g["digest"], np.array([float(sd[k].double().sum()) for k in sorted(sd)]))
    assert sorted(g.files) == sorted(["digest"] + [f"{n}_{k}" for n in synth.SAM_MASK_PROMPT_CASES
                                                   for k in ("dense_prompts", "dense_tap", "iou", "logit_rows", "maskbits")])
    for name, (P, seed) in synth.SAM_MASK_PROMPT_CASES.items():
        points, boxes, masks, multimask = synth.sam_mask_prompt_inputs(name)
        Cm = 3 if multimask else 1
        assert tuple(masks.shape) == (P, 1, 256, 256) and masks.dtype == torch.float32 and masks.is_contiguous()
        assert torch.equal(masks, synth.sam_mask_prompt_case(P, seed))
        assert points[0].shape[0] == P and (boxes is None or boxes.shape[0] == P)
        kept = g[f"{name}_dense_prompts"]
        assert kept.max() < P and g[f"{name}_dense_tap"].shape == (len(kept), 256, -(-64 // TAP_Y), -(-64 // TAP_X))
        assert g[f"{name}_iou"].shape == (P, Cm) and g[f"{name}_logit_rows"].shape == (P, Cm, -(-256 // ROW_TAP), 256)
        assert g[f"{name}_maskbits"].shape == (P, Cm, 256, 32)
        # logit-like: a floor of -8, blobs of +16 that may overlap, noise of std 0.5
        assert -11.0 < float(masks.min()) < -8.0 and 8.0 < float(masks.max()) < 44.0
        assert 0.02 < float((masks > 0).float().mean()) < 0.6
    assert not torch.equal(synth.sam_mask_prompt_case(2, 0), synth.sam_mask_prompt_case(2, 1))
    assert torch.equal(synth.sam_mask_prompt_case(3, 5)[:2], synth.sam_mask_prompt_case(2, 5))   # a longer batch extends a shorter one


@pytest.mark.parametrize("name", list(synth.SAM_MASK_PROMPT_CASES))
def test_restatement_reproduces_the_fixture(golden_dir, golden_threads, name):
    g = golden(golden_dir)
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    _, _, masks, _ = synth.sam_mask_prompt_inputs(name)
    kept = torch.from_numpy(g[f"{name}_dense_prompts"]).long()
    ref = torch.from_numpy(g[f"{name}_dense_tap"])
    with torch.no_grad():
        mine = restate_embed(sd, masks[kept])[:, :, ::TAP_Y, ::TAP_X]
        mine64 = restate_embed(sd, masks[kept], dtype=torch.float64)[:, :, ::TAP_Y, ::TAP_X]
    bound = 1e-6 * max(1.0, float(ref.abs().max()))
    assert float((mine - ref).abs().max()) <= bound
    assert float((mine64 - ref.double()).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))   # the GPU tests' reference
