"""CPU: the definitions the SAM generator's HIP post-processing is held to (pope_amd/sam_amg.py) against the installed torch
and against tests/golden/sam_generator.npz (the reference's own post-processing of `synth.sam_generator_case`, written by
scripts/gen_golden_sam_generator.py), and the shape of the public surface (pope_amd/sam_generator.py).  No tolerances."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pope_amd import sam_amg, synth

PRED_IOU, STABILITY, OFFSET, NMS, THRESHOLD = 0.9, 0.95, 1.0, 0.35, 0.0


def golden(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, "sam_generator.npz"))
    return {k.split(".", 1)[1]: fx[k] for k in fx.files if k.startswith(name + ".")}


def reference_logits(low, input_size, original_size):
    """`Sam.postprocess_masks` written with torch on the CPU."""
    m = F.interpolate(low[None], (1024, 1024), mode="bilinear", align_corners=False)[..., :input_size[0], :input_size[1]]
    return F.interpolate(m, original_size, mode="bilinear", align_corners=False)[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def restated_case(name):
    """The whole CPU restatement for a fixture case: dict with the fixture's keys plus `logits` of the IoU-filtered masks."""
    low, iou, input_size, original_size = synth.sam_generator_case(name)
    keep_iou = np.nonzero(iou.numpy() > np.float32(PRED_IOU))[0]
    logits = sam_amg.postprocess_logits(low.numpy()[keep_iou], input_size, original_size)
    n_hi, n_lo, area = sam_amg.mask_counts(logits, THRESHOLD, OFFSET)
    stability = sam_amg.stability_scores(n_hi, n_lo)
    masks = logits > np.float32(THRESHOLD)
    boxes = sam_amg.mask_to_box(masks)
    sub = np.nonzero(stability >= np.float32(STABILITY))[0]
    order = sam_amg.nms(boxes[sub], iou.numpy()[keep_iou[sub]], NMS)
    return dict(n_hi=n_hi, n_lo=n_lo, area=area, stability=stability, boxes=boxes, keep_iou=keep_iou, keep_stability=keep_iou[sub],
                keep_nms=keep_iou[sub][order], masks=masks[sub][order], logits=logits, sub=sub, iou=iou.numpy())


@pytest.mark.parametrize("name", list(synth.SAM_GENERATOR_CASES))
def test_resampling_recipe_equals_torch_bit_for_bit(name):
    low, _, input_size, original_size = synth.sam_generator_case(name)
    low = low[:6]
    want = reference_logits(low, input_size, original_size).numpy()
    got = sam_amg.postprocess_logits(low.numpy(), input_size, original_size)
    assert got.shape == want.shape == (6, *original_size)
    assert int((bits(got) != bits(want)).sum()) == 0


def test_resampling_recipe_on_other_geometries():
    g = torch.Generator().manual_seed(3)
    for hw in ((600, 400), (1080, 1080), (97, 211)):
        low = torch.randn(2, 256, 256, generator=g) * 5
        isz = sam_amg.preprocess_shape(*hw)
        want = reference_logits(low, isz, hw).numpy()
        assert int((bits(sam_amg.postprocess_logits(low.numpy(), isz, hw)) != bits(want)).sum()) == 0


def test_fmaf_is_a_single_rounding():
    # a * b + c with a tie that double rounding would break the other way: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24, minus 2^-48
    a = np.float32(1 + 2.0 ** -12)
    assert sam_amg.fmaf(a, a, np.float32(-2.0 ** -48)) == np.float32(1 + 2.0 ** -11)
    assert sam_amg.fmaf(a, a, np.float32(2.0 ** -48)) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)


@pytest.mark.parametrize("name", list(synth.SAM_GENERATOR_CASES))
def test_restatement_reproduces_fixture(golden_dir, name):
    fx, got = golden(golden_dir, name), restated_case(name)
    for k in ("n_hi", "n_lo", "area", "boxes", "keep_iou", "keep_stability", "keep_nms"):
        assert np.array_equal(got[k], fx[k]), k
    assert np.array_equal(bits(got["stability"]), bits(fx["stability"]))
    W = synth.SAM_GENERATOR_CASES[name][1][1]
    assert np.array_equal(sam_amg.pack_masks(got["masks"]), fx["packed"])
    assert np.array_equal(sam_amg.unpack_masks(fx["packed"], W), got["masks"])
    rles = [sam_amg.mask_to_rle(m) for m in got["masks"]]
    assert np.array_equal(np.concatenate([r["counts"] for r in rles]), fx["rle_counts"])
    assert np.array_equal([len(r["counts"]) for r in rles], fx["rle_lengths"])
    for r, m in zip(rles, got["masks"]):
        assert r["counts"][0] == 0 or not m[0, 0]
        assert np.array_equal(sam_amg.rle_to_mask(r), m) and sam_amg.area_from_rle(r) == int(m.sum())


def test_fixture_is_not_vacuous(golden_dir):
    name = "frame"
    M, (H, W) = synth.SAM_GENERATOR_CASES[name]
    fx, got = golden(golden_dir, name), restated_case(name)
    assert M >= 96
    assert 16 <= len(fx["keep_iou"]) < M
    assert 16 <= len(fx["keep_stability"]) < len(fx["keep_iou"])
    assert 8 <= len(fx["keep_nms"]) < len(fx["keep_stability"])
    assert int((fx["area"] == 0).sum()) >= 1
    assert np.array_equal(fx["boxes"][fx["area"] == 0], np.zeros((int((fx["area"] == 0).sum()), 4)))
    assert (fx["boxes"][:, 2] == W - 1).any() and (fx["boxes"][:, 3] == H - 1).any()
    # the two places where a restated definition decides: margins around the thresholds
    st = fx["stability"][np.isfinite(fx["stability"])]
    assert np.abs(st.astype(np.float64) - STABILITY).min() > 1e-6
    iou = sam_amg.pairwise_iou(fx["boxes"][got["sub"]])
    iou = iou[np.isfinite(iou)]
    assert np.abs(iou.astype(np.float64) - NMS).min() > 1e-4
    assert len(np.unique(got["iou"])) == M
    # the portrait case has inexact scales
    _, _, (ih, iw), (h, w) = synth.sam_generator_case("portrait")
    assert (ih * 1000) % h and (iw * 1000) % w and h > w
    fp = golden(golden_dir, "portrait")
    assert len(fp["keep_nms"]) < len(fp["keep_stability"]) < len(fp["keep_iou"]) < synth.SAM_GENERATOR_CASES["portrait"][0]


def test_nms_definition_on_hand_cases():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [1, 1, 11, 11], [20, 20, 30, 30], [0, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    scores = np.array([0.5, 0.5, 0.9, 0.1, 0.7, 0.7], np.float32)
    # order 2, 4, 5, 0, 1, 3 (ties keep index order); iou(2, 0) = 81 / 119 > 0.35; empty boxes (0 / 0) suppress nothing
    assert sam_amg.nms(boxes, scores, 0.35).tolist() == [2, 4, 5, 3]
    assert sam_amg.nms(boxes, scores, 0.7).tolist() == [2, 4, 5, 0, 3]
    assert sam_amg.nms(boxes[:0], scores[:0], 0.35).tolist() == []


def test_box_of_masks():
    m = np.zeros((3, 6, 7), bool)
    m[1, 2:4, 3:6] = True
    m[2, 5, 6] = True
    assert sam_amg.mask_to_box(m).tolist() == [[0, 0, 0, 0], [3, 2, 5, 3], [6, 5, 6, 5]]


# ---- remove_small_regions on hand-built masks ------------------------------------------------------------------------------
def _clean(mask, area, mode):
    out, changed = sam_amg.remove_small_regions(torch.as_tensor(mask), area, mode)
    return out.numpy(), changed


def test_holes_of_249_and_250_pixels():
    mask = np.zeros((80, 120), bool)
    mask[5:75, 5:115] = True
    mask[10:20, 10:34] = False      # 240
    mask[20, 10:19] = False         # + 9 = 249, attached below
    mask[40:50, 60:85] = False      # 250
    want = mask.copy()
    want[10:20, 10:34] = True
    want[20, 10:19] = True
    got, changed = _clean(mask, 250, "holes")
    assert changed and np.array_equal(got, want)
    assert not want[40:50, 60:85].any()          # the 250-pixel hole stays: only regions with area < 250 are small
    # the background around the block is itself a "hole" region of the complement; it is large and stays
    assert not got[0, 0]
    got2, changed2 = _clean(want, 250, "holes")
    assert not changed2 and np.array_equal(got2, want)


def test_islands_touching_diagonally_are_one_region():
    mask = np.zeros((40, 40), bool)
    mask[0:10, 0:10] = True          # 100
    mask[10:22, 10:22] = True        # 144, touches the first at a corner only: 8-connectivity joins them (244 < 250)
    mask[30:36, 0:40] = True         # 240, separate
    got, changed = _clean(mask, 250, "islands")
    # every island is small: the largest (244, the diagonal pair) is kept
    want = np.zeros_like(mask)
    want[0:10, 0:10] = True
    want[10:22, 10:22] = True
    assert changed and np.array_equal(got, want)
    mask[22, 22:29] = True           # 7 more pixels on the diagonal chain: 251 >= 250
    got, changed = _clean(mask, 250, "islands")
    want[22, 22:29] = True
    assert changed and np.array_equal(got, want)     # the 240 island goes, the chain stays


def test_all_islands_small_keeps_first_largest_on_a_tie():
    mask = np.zeros((30, 30), bool)
    mask[2:5, 2:6] = True            # 12, first in raster order
    mask[10:14, 10:13] = True        # 12
    mask[20, 20] = True
    got, changed = _clean(mask, 250, "islands")
    want = np.zeros_like(mask)
    want[2:5, 2:6] = True
    assert changed and np.array_equal(got, want)
    empty = np.zeros((8, 8), bool)
    got, changed = _clean(empty, 250, "islands")
    assert not changed and not got.any()


def test_labels_are_in_first_pixel_raster_order():
    m = torch.zeros(1, 6, 9, dtype=torch.bool)
    m[0, 0, 7] = True                 # first pixel (0, 7) -> label 1
    m[0, 1:5, 0] = True               # first pixel (1, 0) -> label 2, a U that closes at the bottom
    m[0, 4, 0:4] = True
    m[0, 2:5, 3] = True
    m[0, 3, 6] = True                 # label 3
    lab, n = sam_amg.label_components(m)
    assert int(n[0]) == 3
    assert lab[0, 0, 7] == 1 and lab[0, 2, 3] == 2 and lab[0, 1, 0] == 2 and lab[0, 3, 6] == 3 and lab[0, 0, 0] == 0


# ---- the public surface ----------------------------------------------------------------------------------------------------
def small_sam(depth=2):
    """A `Sam` with the ViT-B geometry at reduced depth and synthetic weights."""
    from pope_amd.sam_decoder import MaskDecoder, PromptEncoder, TwoWayTransformer
    from pope_amd.sam_encoder import ImageEncoderViT
    from pope_amd.sam_generator import Sam
    from functools import partial
    enc = ImageEncoderViT(depth=depth, embed_dim=768, img_size=1024, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                          num_heads=12, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=[1], window_size=14,
                          out_chans=256)
    sam = Sam(enc, PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024), mask_in_chans=16),
              MaskDecoder(num_multimask_outputs=3, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                          transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256))
    sd = {"image_encoder." + k: v for k, v in synth.synthetic_sam_encoder_state_dict(seed=0, dim=768, depth=depth, heads=12,
                                                                                      global_idx=(1,)).items()}
    sd.update(synth.synthetic_sam_decoder_state_dict(seed=0))
    return sam, sd


def test_sam_loads_a_full_checkpoint_layout_strictly():
    sam, sd = small_sam()
    assert not any(k.startswith("pixel_") for k in sam.state_dict())          # non-persistent, as in a checkpoint
    assert sorted(sam.state_dict()) == sorted(sd)
    sam.load_state_dict(sd, strict=True)
    back = sam.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert sam.mask_threshold == 0.0 and sam.image_format == "RGB"
    assert sam.pixel_mean.shape == (3, 1, 1) and sam.pixel_std.flatten().tolist() == pytest.approx([58.395, 57.12, 57.375])
    x = sam.preprocess(torch.zeros(1, 3, 768, 1024))
    assert x.shape == (1, 3, 1024, 1024) and float(x[0, 0, 800, 0]) == 0.0


def test_generator_defaults_are_the_forks():
    from pope_amd.sam_generator import SamAutomaticMaskGenerator, build_sam_vit_b, sam_model_registry
    want = dict(points_per_side=16, points_per_batch=2048, pred_iou_thresh=0.9, stability_score_thresh=0.95,
                stability_score_offset=1.0, box_nms_thresh=0.35, crop_n_layers=0, crop_nms_thresh=0.35,
                crop_overlap_ratio=512 / 1500, crop_n_points_downscale_factor=1, point_grids=None, min_mask_region_area=250,
                output_mode="binary_mask")
    sig = inspect.signature(SamAutomaticMaskGenerator.__init__)
    assert list(sig.parameters)[2:] == list(want) and {k: sig.parameters[k].default for k in want} == want
    assert set(sam_model_registry) == {"default", "vit_h", "vit_l", "vit_b"}
    sam = build_sam_vit_b()
    assert (sam.image_encoder.embed_dim, sam.image_encoder.depth, sam.image_encoder.global_attn_indexes) == (768, 12, (2, 5, 8, 11))
    gen = SamAutomaticMaskGenerator(sam)
    assert gen.point_grids[0].shape == (256, 2) and gen.min_mask_region_area == 250
    with pytest.raises(NotImplementedError):
        SamAutomaticMaskGenerator(sam, crop_n_layers=1)
    with pytest.raises(NotImplementedError):
        SamAutomaticMaskGenerator(sam, output_mode="coco_rle")
