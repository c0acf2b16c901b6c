"""SAM mask prompts on the MI355X: the fused mask embedding (`pope_sam_mask_embed_f32`) against the reference fixture
(tests/golden/sam_mask_prompt.npz) and an fp64 restatement, special inputs, batch invariance bit for bit, the decoder's general
(per-prompt dense) path fed with embeddings that vary over pixels, the predictor's `mask_input` loop, `Sam.forward` records
with `mask_inputs`, and weight reloads."""
import warnings

import numpy as np
import pytest
import torch

from pope_amd import synth
from pope_amd.sam_generator import SamPredictor
from test_sam_decoder_cpu import build_models, restate
from test_sam_generator_cpu import small_sam
from test_sam_mask_prompt_cpu import ROW_TAP, TAP_X, TAP_Y, golden, restate_embed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# The project's relative bound, REL * max(1, max |ref|), of tests/test_gpu_sam_decoder.py.  torch's own fp32 error against
# fp64 on these inputs (the restatements on the CPU): embedding 1.1e-6 ("box") and 1.6e-6 ("points") at max |.| 3.8, decoder mask
# logits 6.4e-6 at max 5.5 ("box" masks; |mask| <= 26.4, smallest variance under the first LayerNorm2d 8.9e-4 against eps 1e-6).
# Measured on one MI355X, as |got - ref| / max(1, max |ref|):
#   embedding vs fp64, P = 1 / 3 / 17: 2.7e-7 / 3.3e-7 / 4.2e-7 (max |ref| 3.8); vs the fixture: <= 4.0e-7;
#     special inputs (zeros / constant / binary): 2.0e-7 / 1.4e-7 / 2.1e-7
#   decoder with mask prompts vs fp64, masks / iou: mask only 1.3e-6 / 3.6e-7, "box" 1.5e-6 / 5.2e-7, "points" 1.4e-6 / 9.0e-7
#     (f16x3); 1.2e-6 / 6.1e-7, 1.2e-6 / 2.2e-7, 1.3e-6 / 1.2e-6 (f32); max |ref| 5.0 .. 6.1
#   fixture parity, iou / logit rows: "box" 3.8e-7 / 1.1e-6, "points" 1.2e-6 / 1.4e-6; mask bits excluded 0.43 % / 0.38 %,
#     none differing outside the excluded set
#   a mask prompt moves the "box" logits by 5.7
REL = 1e-5


def bound(ref):
    return REL * max(1.0, float(ref.abs().max()))


def rel(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.fixture(scope="module")
def models():
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    pe, md = build_models(sd)
    return {k: v.to(DEV) for k, v in sd.items()}, pe.to(DEV), md.to(DEV)


@pytest.fixture(scope="module")
def image():
    return synth.synthetic_sam_image_embedding(seed=1).to(DEV)


@pytest.fixture(scope="module")
def masks17():
    return synth.sam_mask_prompt_inputs("points")[2].to(DEV)


@pytest.fixture(scope="module")
def ref17(models, masks17):
    """fp64 restatement of the 17 embeddings, computed once and left unchanged."""
    with torch.no_grad():
        return restate_embed(models[0], masks17, dtype=torch.float64)


def embed(pe, masks):
    sparse, dense = pe(points=None, boxes=None, masks=masks)
    assert tuple(sparse.shape) == (masks.shape[0], 0, 256) and sparse.device == masks.device
    assert tuple(dense.shape) == (masks.shape[0], 256, 64, 64) and dense.is_contiguous() and dense.dtype == torch.float32
    return dense


# ---- the embedding -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 17])
def test_embedding_against_fp64_and_the_fixture(golden_dir, models, masks17, ref17, P):
    _, pe, _ = models
    dense = embed(pe, masks17[:P])
    print(f"P = {P}: vs fp64 {rel(dense, ref17[:P]):.3e} (max |ref| {float(ref17[:P].abs().max()):.3f})")
    assert float((dense.double() - ref17[:P]).abs().max()) <= bound(ref17[:P])
    g = golden(golden_dir)
    kept = [(i, int(p)) for i, p in enumerate(g["points_dense_prompts"]) if p < P]
    assert kept
    for i, p in kept:
        tap = torch.from_numpy(g["points_dense_tap"][i])
        print(f"P = {P}: prompt {p} vs the fixture {rel(dense[p, :, ::TAP_Y, ::TAP_X].cpu(), tap):.3e}")
        assert float((dense[p, :, ::TAP_Y, ::TAP_X].cpu() - tap).abs().max()) <= bound(tap)


def test_special_inputs(models):
    sd, pe, _ = models
    yy, xx = torch.meshgrid(torch.arange(256), torch.arange(256), indexing="ij")
    binary = torch.where(((yy // 24 + xx // 40) % 2 == 0) | ((yy - 128) ** 2 + (xx - 100) ** 2 < 50 ** 2), 10.0, -10.0)
    masks = torch.stack([torch.zeros(256, 256), torch.full((256, 256), -7.5), binary])[:, None].to(DEV)
    dense = embed(pe, masks)
    with torch.no_grad():
        ref = restate_embed(sd, masks, dtype=torch.float64)
    assert bool(torch.isfinite(dense).all())
    for i, name in enumerate(("zeros", "constant -7.5", "binary +-10")):
        print(f"{name}: vs fp64 {rel(dense[i], ref[i]):.3e} (max |ref| {float(ref[i].abs().max()):.3f})")
        assert float((dense[i].double() - ref[i]).abs().max()) <= bound(ref[i]), name
    # a constant mask gives one value per channel
    assert torch.equal(dense[1], dense[1, :, :1, :1].expand(-1, 64, 64))
    assert not torch.equal(dense[0], dense[1])


def test_embedding_is_batch_invariant(models, masks17):
    _, pe, _ = models
    all17 = embed(pe, masks17)
    assert torch.equal(embed(pe, masks17[16:17])[0], all17[16])                            # alone (a view at an offset)
    three = torch.stack([masks17[16], masks17[0], masks17[1]])
    got = embed(pe, three)
    assert torch.equal(got[0], all17[16]) and torch.equal(got[1], all17[0]) and torch.equal(got[2], all17[1])
    wide = torch.zeros(17, 1, 256, 512, device=DEV)
    wide[..., ::2] = masks17
    view = wide[..., ::2]
    assert not view.is_contiguous() and torch.equal(view, masks17)
    assert torch.equal(embed(pe, view), embed(pe, view.contiguous())) and torch.equal(embed(pe, view), all17)
    odd = torch.zeros(3 * 65536 + 1, device=DEV)   # a contiguous view that is not 16-byte aligned
    odd[1:] = masks17[:3].flatten()
    assert torch.equal(embed(pe, odd[1:].view(3, 1, 256, 256)), all17[:3])


def test_argument_errors_on_the_device(models, masks17):
    _, pe, _ = models
    with pytest.raises(ValueError, match="masks"):
        pe(points=None, boxes=None, masks=masks17[:2, 0])                                  # [2, 256, 256]
    with pytest.raises(TypeError, match="masks"):
        pe(points=None, boxes=None, masks=masks17[:2].double())
    with pytest.raises(ValueError, match="masks"):                                         # 2 masks, 3 boxes
        pe(points=None, boxes=torch.zeros(3, 4, device=DEV), masks=masks17[:2])
    assert tuple(pe(points=None, boxes=None, masks=masks17[:0])[1].shape) == (0, 256, 64, 64)
    bad = masks17[:2].clone()
    bad[1, 0, 100, 100] = float("nan")
    dense = embed(pe, bad)                                                                 # non-finite in, non-finite out, no check
    assert bool(torch.isfinite(dense[0]).all()) and bool(torch.isnan(dense[1, :, 25, 25]).all())
    assert bool(torch.isfinite(dense[1, :, 24, 25]).all())


# ---- the decoder's general path --------------------------------------------------------------------------------------------
def case_prompts(name):
    """(points, boxes, masks, multimask) on the device: the two fixture cases and one mask alone."""
    if name == "mask_only":
        return None, None, synth.sam_mask_prompt_case(1, 7).to(DEV), True
    points, boxes, masks, multimask = synth.sam_mask_prompt_inputs(name)
    return (points[0].to(DEV), points[1].to(DEV)), None if boxes is None else boxes.to(DEV), masks.to(DEV), multimask


_decoder_refs = {}


def decoder_ref(name, models, image):
    """fp64 restatement of case `name` (the decoder fed the fp64 embedding), computed once per case."""
    if name not in _decoder_refs:
        sd, pe, _ = models
        points, boxes, masks, multimask = case_prompts(name)
        with torch.no_grad():
            sparse, _ = pe(points=points, boxes=boxes, masks=masks)
            dense64 = restate_embed(sd, masks, dtype=torch.float64)
            rm, ri, _, _ = restate(sd, image, pe.get_dense_pe(), sparse, dense64, multimask, dtype=torch.float64)
        _decoder_refs[name] = (rm, ri)
    return _decoder_refs[name]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", ["mask_only", "box", "points"])
def test_decoder_with_mask_prompts_against_fp64(models, image, name, precision):
    _, pe, md = models
    points, boxes, masks, multimask = case_prompts(name)
    rm, ri = decoder_ref(name, models, image)
    sparse, dense = pe(points=points, boxes=boxes, masks=masks)
    assert sparse.shape[1] == {"mask_only": 0, "box": 4, "points": 2}[name]
    md.precision = precision
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")   # no range-guard re-run on the way
            low, iou = md(image, pe.get_dense_pe(), sparse, dense, multimask)
    finally:
        md.precision = "f16x3"
    assert low.shape == (masks.shape[0], 3 if multimask else 1, 256, 256)
    print(f"{name} {precision}: masks {rel(low, rm):.3e} (max |ref| {float(rm.abs().max()):.3f}), iou {rel(iou, ri):.3e}")
    assert float((iou.double() - ri).abs().max()) <= bound(ri)
    assert float((low.double() - rm).abs().max()) <= bound(rm)


@pytest.mark.parametrize("name", list(synth.SAM_MASK_PROMPT_CASES))
def test_fixture_parity(golden_dir, models, image, name):
    g = golden(golden_dir)
    _, pe, md = models
    points, boxes, masks, multimask = case_prompts(name)
    sparse, dense = pe(points=points, boxes=boxes, masks=masks)
    for i, p in enumerate(g[f"{name}_dense_prompts"]):
        tap = torch.from_numpy(g[f"{name}_dense_tap"][i])
        assert float((dense[int(p), :, ::TAP_Y, ::TAP_X].cpu() - tap).abs().max()) <= bound(tap)
    low, iou = md(image, pe.get_dense_pe(), sparse, dense, multimask)
    low, iou = low.cpu(), iou.cpu()
    ref_iou, ref_rows = torch.from_numpy(g[f"{name}_iou"]), torch.from_numpy(g[f"{name}_logit_rows"])
    print(f"{name}: iou {rel(iou, ref_iou):.3e}, logit rows {rel(low[:, :, ::ROW_TAP], ref_rows):.3e} (max |ref| {float(ref_rows.abs().max()):.3f})")
    assert float((iou - ref_iou).abs().max()) <= bound(ref_iou)
    assert float((low[:, :, ::ROW_TAP] - ref_rows).abs().max()) <= bound(ref_rows)
    bits = torch.from_numpy(np.unpackbits(g[f"{name}_maskbits"], axis=-1).astype(bool))
    near = low.abs() < 1e-3 * float(low.abs().max())
    print(f"{name}: {100.0 * float(near.float().mean()):.2f} % of the mask bits excluded, "
          f"{int(((low > 0) != bits)[~near].sum())} differing outside")
    assert float(near.float().mean()) <= 0.02
    assert bool(((low > 0) == bits)[~near].all())


def test_a_mask_prompt_changes_the_result(models, image):
    _, pe, md = models
    points, boxes, masks, multimask = case_prompts("box")
    sparse, dense = pe(points=points, boxes=boxes, masks=masks)
    sparse0, dense0 = pe(points=points, boxes=boxes, masks=None)
    assert torch.equal(sparse, sparse0) and dense0.stride(0) == 0
    with_mask, _ = md(image, pe.get_dense_pe(), sparse, dense, multimask)
    without, _ = md(image, pe.get_dense_pe(), sparse0, dense0, multimask)
    print(f"a mask prompt moves the logits by {float((with_mask - without).abs().max()):.3f}")
    assert float((with_mask - without).abs().max()) > 1e-2


# ---- predictor and Sam.forward ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sam():
    model, sd = small_sam(depth=2)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


def test_predictor_takes_mask_input(sam):
    x = synth.sam_forward_case(DEV)[1]
    pr = SamPredictor(sam)
    m = synth.sam_mask_prompt_case(3, 11).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no range warning anywhere below
        pr.set_torch_image(x["image"][None], x["original_size"])
        masks, iou, low = pr.predict_torch(x["point_coords"], x["point_labels"], None, mask_input=m, multimask_output=True)
        sparse, dense = sam.prompt_encoder(points=(x["point_coords"], x["point_labels"]), boxes=None, masks=m)
        low_hand, iou_hand = sam.mask_decoder(pr.features, sam.prompt_encoder.get_dense_pe(), sparse, dense, True)
        masks_hand = sam.postprocess_masks(low_hand, pr.input_size, pr.original_size) > sam.mask_threshold
        assert torch.equal(low, low_hand) and torch.equal(iou, iou_hand) and torch.equal(masks, masks_hand)
        _, _, low_plain = pr.predict_torch(x["point_coords"], x["point_labels"], None, None, True)
        assert float((low - low_plain).abs().max()) > 1e-2
        # the documented loop: numpy in and out, the best mask of a call fed back into the next, two rounds
        point, label = x["point_coords"][0].cpu().numpy() * (400 / 683), x["point_labels"][0].cpu().numpy()
        masks_np, iou_np, low_np = pr.predict(point_coords=point, point_labels=label, multimask_output=True)
        for _ in range(2):
            best = int(np.argmax(iou_np))
            masks_np, iou_np, low_np = pr.predict(point_coords=point, point_labels=label, mask_input=low_np[best][None],
                                                  multimask_output=True)
            assert isinstance(masks_np, np.ndarray) and masks_np.dtype == bool and masks_np.shape == (3, 600, 400)
            assert iou_np.shape == (3,) and low_np.shape == (3, 256, 256) and low_np.dtype == np.float32
            assert np.isfinite(low_np).all() and np.isfinite(iou_np).all()


@pytest.mark.parametrize("multimask", [True, False])
def test_forward_with_a_mask_record(sam, multimask):
    case = synth.sam_forward_case(DEV)
    m = synth.sam_mask_prompt_case(3, 12).to(DEV)
    batch = [case[0], dict(case[1], mask_inputs=m)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sam(batch, multimask_output=multimask)
        pr = SamPredictor(sam)
        for r, (x, o) in enumerate(zip(batch, out)):
            pr.set_torch_image(x["image"][None], x["original_size"])
            masks, iou, low = pr.predict_torch(x.get("point_coords"), x.get("point_labels"), x.get("boxes"), x.get("mask_inputs"),
                                               multimask)
            assert torch.equal(o["low_res_logits"], low), r
            assert torch.equal(o["iou_predictions"], iou), r
            assert torch.equal(o["masks"], masks), r
        plain = sam(case, multimask_output=multimask)
    assert all(torch.equal(out[0][k], plain[0][k]) for k in plain[0])           # the record without a mask does not notice
    assert float((out[1]["low_res_logits"] - plain[1]["low_res_logits"]).abs().max()) > 1e-2
    alone = sam(batch[1:], multimask_output=multimask)                           # a single record with a mask
    assert all(torch.equal(alone[0][k], out[1][k]) for k in out[1])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="is on"):
            sam([dict(case[1], mask_inputs=m.to("cuda:1"))], multimask)


# ---- weights ---------------------------------------------------------------------------------------------------------------
def test_weight_changes_take_effect(masks17):
    pe, _ = build_models(synth.synthetic_sam_decoder_state_dict(seed=0))
    pe = pe.to(DEV)
    d0 = embed(pe, masks17[:3])
    sd1 = synth.synthetic_sam_decoder_state_dict(seed=1)
    pe.load_state_dict({k[len("prompt_encoder."):]: v for k, v in sd1.items() if k.startswith("prompt_encoder.")}, strict=True)
    d1 = embed(pe, masks17[:3])
    assert float((d0 - d1).abs().max()) > 1e-2
    with torch.no_grad():
        ref = restate_embed({k: v.to(DEV) for k, v in sd1.items()}, masks17[:3], dtype=torch.float64)
    assert float((d1.double() - ref).abs().max()) <= bound(ref)
    pe.mask_downscaling[6].weight.data.mul_(2)          # in place
    d2 = embed(pe, masks17[:3])
    assert float((d2 - d1).abs().max()) > 1e-2
    bias = pe.mask_downscaling[6].bias.detach().reshape(1, -1, 1, 1)
    assert float((d2 - (2 * (d1 - bias) + bias)).abs().max()) <= bound(d2)
    pe.mask_downscaling[0].weight = torch.nn.Parameter(pe.mask_downscaling[0].weight.detach() * 0.5)   # a replaced Parameter
    sd2 = {"prompt_encoder." + k: v for k, v in pe.state_dict().items()}
    with torch.no_grad():
        ref2 = restate_embed(sd2, masks17[:3], dtype=torch.float64)
    d3 = embed(pe, masks17[:3])
    assert float((d3 - d2).abs().max()) > 1e-3 and float((d3.double() - ref2).abs().max()) <= bound(ref2)
