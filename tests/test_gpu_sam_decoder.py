"""SAM prompt encoder + mask decoder on the MI355X: parity with the reference fixture (tests/golden/sam_decoder.npz) and
with an fp64 restatement, batch invariance, the shared layer-0 path, the range guard, weight reloads, and the chain
from the SAM image encoder."""
import warnings
from functools import partial

import numpy as np
import pytest
import torch

from pope_amd import synth
from pope_amd.dinov2 import PopeRangeError
from test_sam_decoder_cpu import KEY_TAP, ROW_TAP, build_models, golden, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# relative bound, REL * max(1, max |ref|): measured on one MI355X at <= 1.6e-6 (fixture and fp64 cases, f16x3 and f32 alike);
# 1e-5 keeps ~6x headroom (the issue's starting bound was 1e-4)
REL = 1e-5


def bound(ref):
    return REL * max(1.0, float(ref.abs().max()))


@pytest.fixture(scope="module")
def models():
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    pe, md = build_models(sd)
    return sd, pe.to(DEV), md.to(DEV)


@pytest.fixture(scope="module")
def image():
    return synth.synthetic_sam_image_embedding(seed=1).to(DEV)


def prompts(name):
    (coords, labels), boxes, multimask = synth.sam_decoder_case(name)
    return (coords.to(DEV), labels.to(DEV)), None if boxes is None else boxes.to(DEV), multimask


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", synth.SAM_DECODER_CASES)
def test_fixture_parity(golden_dir, models, image, name, precision):
    g = golden(golden_dir)
    _, pe, md = models
    md.precision = precision
    points, boxes, multimask = prompts(name)
    sparse, dense = pe(points=points, boxes=boxes, masks=None)
    assert dense.stride(0) == 0
    assert float((sparse.detach().cpu() - torch.from_numpy(g[f"{name}_sparse"])).abs().max()) <= 1e-6
    assert float((dense[0, :, 0, 0].detach().cpu() - torch.from_numpy(g["dense_value"])).abs().max()) <= 1e-6
    masks, iou, hs, keys = md.forward_with_taps(image, pe.get_dense_pe(), sparse, dense, multimask)
    md.precision = "f16x3"
    masks, iou, hs, keys = masks.cpu(), iou.cpu(), hs.cpu(), keys.cpu()
    taps = torch.from_numpy(g[f"{name}_taps"]).long()
    kp = torch.from_numpy(g[f"{name}_keys_prompts"]).long()
    ref_iou = torch.from_numpy(g[f"{name}_iou"])
    assert masks.shape == (sparse.shape[0], 3 if multimask else 1, 256, 256)
    assert float((iou - ref_iou).abs().max()) <= bound(ref_iou)
    ref_rows = torch.from_numpy(g[f"{name}_logit_rows"])
    assert float((masks[taps][:, :, ::ROW_TAP] - ref_rows).abs().max()) <= bound(ref_rows)
    ref_hs = torch.from_numpy(g[f"{name}_hs"])
    assert float((hs[taps] - ref_hs).abs().max()) <= bound(ref_hs)
    ref_keys = torch.from_numpy(g[f"{name}_keys"])
    assert float((keys[kp][:, ::KEY_TAP] - ref_keys).abs().max()) <= bound(ref_keys)
    bits = torch.from_numpy(np.unpackbits(g[f"{name}_maskbits"], axis=-1).astype(bool))
    near = masks[taps].abs() < 1e-3 * float(masks[taps].abs().max())
    assert bool(((masks[taps] > 0) == bits)[~near].all())


def random_case(P, ns, seed):
    gen = torch.Generator().manual_seed(seed)
    sparse = torch.randn(P, ns, 256, generator=gen).to(DEV)
    dense = (0.5 * torch.randn(256, generator=gen)).to(DEV).reshape(1, -1, 1, 1).expand(P, -1, 64, 64)
    return sparse, dense


@pytest.mark.parametrize("P,ns,multimask,precision", [
    (1, 0, True, "f16x3"), (3, 2, False, "f16x3"), (64, 3, True, "f16x3"), (257, 11, False, "f16x3"),
    (257, 2, True, "f16x3"), (1, 11, True, "f16x3"), (3, 0, False, "f32"), (64, 11, True, "f32")])
def test_against_fp64_restatement(models, image, P, ns, multimask, precision):
    sd, pe, md = models
    sparse, dense = random_case(P, ns, seed=P * 100 + ns)
    image_pe = pe.get_dense_pe()
    md.precision = precision
    masks, iou = md(image, image_pe, sparse, dense, multimask)
    md.precision = "f16x3"
    with torch.no_grad():
        rm, ri, _, _ = restate({k: v.to(DEV) for k, v in sd.items()}, image, image_pe, sparse, dense, multimask, dtype=torch.float64)
    assert float((iou.double() - ri).abs().max()) <= bound(ri)
    assert float((masks.double() - rm).abs().max()) <= bound(rm)


def test_batch_invariance(models, image):
    _, pe, md = models
    points, boxes, multimask = prompts("grid")
    sparse, dense = pe(points=points, boxes=boxes, masks=None)
    m_all, i_all = md(image, pe.get_dense_pe(), sparse, dense, True)
    for i in (0, 17, 100, 255):
        m1, i1 = md(image, pe.get_dense_pe(), sparse[i:i + 1], dense[i:i + 1], True)
        assert torch.equal(m1[0], m_all[i]) and torch.equal(i1[0], i_all[i]), i
        s = min(max(i - 3, 0), 256 - 7)
        m7, i7 = md(image, pe.get_dense_pe(), sparse[s:s + 7], dense[s:s + 7], True)
        assert torch.equal(m7[i - s], m_all[i]) and torch.equal(i7[i - s], i_all[i]), i


def test_shared_layer0_matches_the_general_path(models, image):
    _, pe, md = models
    sparse, dense = random_case(20, 2, seed=5)   # 20 prompts: one chunk seam
    m_s, i_s = md(image, pe.get_dense_pe(), sparse, dense, True)
    m_g, i_g = md(image, pe.get_dense_pe(), sparse, dense.contiguous(), True)
    assert float((m_s - m_g).abs().max()) <= bound(m_s)
    assert float((i_s - i_g).abs().max()) <= bound(i_s)


def test_range_guard(models, image):
    _, pe, md = models
    sparse, dense = random_case(3, 2, seed=9)
    big = image.clone()
    big[0, 5, 10, 20] = 1e6
    md.on_overflow = "raise"
    try:
        with pytest.raises(PopeRangeError):
            md(big, pe.get_dense_pe(), sparse, dense, True)
    finally:
        md.on_overflow = "rerun_f32"
    with pytest.warns(UserWarning, match="f16x3 range"):
        m, i = md(big, pe.get_dense_pe(), sparse, dense, True)
    md.precision = "f32"
    m32, i32 = md(big, pe.get_dense_pe(), sparse, dense, True)
    md.precision = "f16x3"
    assert torch.equal(m, m32) and torch.equal(i, i32)


def test_weight_changes_take_effect(image):
    pe, md = build_models(synth.synthetic_sam_decoder_state_dict(seed=0))
    pe, md = pe.to(DEV), md.to(DEV)
    sparse, dense = random_case(4, 2, seed=3)
    m0, i0 = md(image, pe.get_dense_pe(), sparse, dense, True)
    sd1 = synth.synthetic_sam_decoder_state_dict(seed=1)
    md.load_state_dict({k[len("mask_decoder."):]: v for k, v in sd1.items() if k.startswith("mask_decoder.")}, strict=True)
    pe.load_state_dict({k[len("prompt_encoder."):]: v for k, v in sd1.items() if k.startswith("prompt_encoder.")}, strict=True)
    m1, i1 = md(image, pe.get_dense_pe(), sparse, dense, True)
    assert float((m0 - m1).abs().max()) > 1e-2 and float((i0 - i1).abs().max()) > 1e-2
    with torch.no_grad():
        rm, ri, _, _ = restate({k: v.to(DEV) for k, v in sd1.items()}, image, pe.get_dense_pe(), sparse, dense, True,
                               dtype=torch.float64)
    assert float((m1.double() - rm).abs().max()) <= bound(rm)


def test_image_encoder_to_masks(models):
    from pope_amd.sam_encoder import ImageEncoderViT
    sd, pe, md = models
    dim, depth, heads, gidx = 768, 12, 12, (2, 5, 8, 11)
    enc = ImageEncoderViT(depth=depth, embed_dim=dim, img_size=1024, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                          num_heads=heads, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=list(gidx),
                          window_size=14, out_chans=256)
    enc.load_state_dict(synth.synthetic_sam_encoder_state_dict(seed=0, dim=dim, depth=depth, heads=heads, grid=64, window=14,
                                                               global_idx=gidx), strict=True)
    enc = enc.to(DEV)
    x = torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(4)).to(DEV)
    points, boxes, _ = prompts("grid")
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no range-guard re-run on the way
        emb = enc(x)
        sparse, dense = pe(points=points, boxes=boxes, masks=None)
        masks, iou = md(emb, pe.get_dense_pe(), sparse, dense, True)
    assert emb.is_cuda and masks.is_cuda and masks.shape == (256, 3, 256, 256) and iou.shape == (256, 3)
    assert bool(torch.isfinite(masks).all()) and bool(torch.isfinite(iou).all())
    sel = torch.arange(0, 256, 51, device=DEV)
    with torch.no_grad():
        rm, ri, _, _ = restate({k: v.to(DEV) for k, v in sd.items()}, emb, pe.get_dense_pe(), sparse[sel], dense[sel], True,
                               dtype=torch.float64)
    assert float((masks[sel].double() - rm).abs().max()) <= bound(rm)
    assert float((iou[sel].double() - ri).abs().max()) <= bound(ri)
