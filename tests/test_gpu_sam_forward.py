"""`Sam.forward` and the multi-image mask decoder on the MI355X: the multi-image entry against the single-image decoder bit
for bit (image mixes, the 16-prompt seam, prompt order), its range guard per image, `Sam.forward` against the predictor's
per-record calls bit for bit, and against the reference's own `Sam.forward` (tests/golden/sam_forward.npz)."""
import warnings

import numpy as np
import pytest
import torch

from pope_amd import synth
from pope_amd.dinov2 import PopeRangeError
from pope_amd.sam_generator import SamPredictor
from test_sam_decoder_cpu import build_models
from test_sam_forward_cpu import ROW_STEP, golden
from test_sam_generator_cpu import reference_logits, small_sam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = [5, 0, 14, 1]   # prompts per image: an image without prompts; image 2 straddles the 16-prompt seam; chunk 0 mixes
#                          images 0 and 2, chunk 1 images 2 and 3
# (d): relative bound, REL * max(1, max |ref|), the form of tests/test_gpu_sam_decoder.py.  Measured once on one MI355X: the
# largest deviation from the fixture is 1.998e-6 (record 1's low-res logits, max |ref| 3.64; record 0's 1.444e-6; the IoU
# predictions 9.4e-7 and 6.0e-7), 50 times below the 1e-4 the encoder's embeddings are held to (tests/test_gpu_sam.py).
# REL = 4 x 1.998e-6 = 7.99e-6, rounded up to one significant digit; the margin is for later route changes at other shapes,
# the kernels being deterministic.
REL = 8e-6


@pytest.fixture(scope="module")
def models():
    pe, md = build_models(synth.synthetic_sam_decoder_state_dict(seed=0))
    return pe.to(DEV), md.to(DEV)


@pytest.fixture(scope="module")
def images():
    return torch.cat([synth.synthetic_sam_image_embedding(seed=s) for s in (1, 2, 3, 4)]).to(DEV)


def sparse_prompts(pe, ns, P, seed):
    """P prompts of ns sparse embeddings from the prompt encoder: none; a point + the padding point for the first half and a
    box for the second; a point + a box."""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(P, 1, 2, generator=g) * 1024).to(DEV)
    lab = torch.randint(0, 2, (P, 1), generator=g).to(torch.int).to(DEV)
    lo = torch.rand(P, 2, generator=g) * 600
    box = torch.cat([lo, lo + 50 + torch.rand(P, 2, generator=g) * 300], 1).to(DEV)
    if ns == 0:
        return torch.empty(P, 0, 256, device=DEV), pe(points=None, boxes=None, masks=None)[1]
    if ns == 2:
        h = P // 2
        a, dense = pe(points=(pts[:h], lab[:h]), boxes=None, masks=None)
        b, _ = pe(points=None, boxes=box[h:], masks=None)
        return torch.cat([a, b]), dense[:1]
    return pe(points=(pts, lab), boxes=box, masks=None)


# ---- (a) the multi-image decoder equals the single-image decoder ------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("multimask", [True, False])
@pytest.mark.parametrize("ns", [0, 2, 3])
def test_images_entry_equals_the_single_image_decoder(models, images, ns, multimask, precision):
    pe, md = models
    image_pe = pe.get_dense_pe()
    P = sum(COUNTS)
    sparse, dense = sparse_prompts(pe, ns, P, seed=10 + ns)
    assert sparse.shape == (P, ns, 256)
    which = np.repeat(np.arange(len(COUNTS)), COUNTS)
    md.precision = precision
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")   # no range-guard re-run on the way
            want_m, want_i = [], []
            for n, c in enumerate(COUNTS):    # the reference: each image's prompts with that image alone
                if c == 0:
                    continue
                rows = torch.as_tensor(np.nonzero(which == n)[0], device=DEV)
                m, i = md(images[n:n + 1], image_pe, sparse[rows], dense[:1].expand(c, -1, -1, -1), multimask)
                want_m.append(m)
                want_i.append(i)
            want_m, want_i = torch.cat(want_m), torch.cat(want_i)
            got_m, got_i = md.forward_images(images, image_pe, sparse, dense, which, multimask)
            assert got_m.shape == (P, 3 if multimask else 1, 256, 256) and got_i.shape == (P, 3 if multimask else 1)
            assert torch.equal(got_m, want_m) and torch.equal(got_i, want_i)
            perm = torch.randperm(P, generator=torch.Generator().manual_seed(5))
            assert not torch.equal(perm, torch.arange(P))
            sh_m, sh_i = md.forward_images(images, image_pe, sparse[perm.to(DEV)], dense, which[perm.numpy()], multimask)
            assert torch.equal(sh_m, want_m[perm.to(DEV)]) and torch.equal(sh_i, want_i[perm.to(DEV)])
            # N = 1 is `forward`
            one_m, one_i = md.forward_images(images[2:3], image_pe, sparse[5:19], dense[:1], [0] * 14, multimask)
            assert torch.equal(one_m, want_m[5:19]) and torch.equal(one_i, want_i[5:19])
    finally:
        md.precision = "f16x3"


def test_images_entry_rejects_a_bad_map_and_a_per_prompt_dense(models, images):
    pe, md = models
    sparse, dense = sparse_prompts(pe, 2, 4, seed=1)
    for bad in ([0, 1, 2, 4], [0, -1, 2, 3], [0, 1, 2]):
        with pytest.raises(ValueError, match="prompt_image"):
            md.forward_images(images, pe.get_dense_pe(), sparse, dense, bad, True)
    with pytest.raises(ValueError, match="broadcast"):
        md.forward_images(images, pe.get_dense_pe(), sparse, dense.expand(4, -1, -1, -1).contiguous(), [0, 1, 2, 3], True)


def test_both_entries_reject_the_same_inputs(models, images):
    """Inputs that are bad for both entries raise the same exception with the same message from either; nothing is launched."""
    pe, md = models
    image_pe = pe.get_dense_pe()
    sparse, dense = sparse_prompts(pe, 2, 3, seed=3)
    two, which = images[:2], [0, 1, 1]
    good = dict(image_pe=image_pe, sparse=sparse, dense=dense)
    table = {"a float64 image_pe": dict(image_pe=image_pe.double()),
             "sparse [3, 2, 128]": dict(sparse=sparse[:, :, :128].contiguous()),
             "12 sparse embeddings": dict(sparse=sparse.repeat(1, 6, 1)),
             "a float16 dense": dict(dense=dense.half())}
    for what, bad in table.items():
        a = dict(good, **bad)
        with pytest.raises((TypeError, ValueError)) as one:
            md(two[:1], a["image_pe"], a["sparse"], a["dense"], True)
        with pytest.raises((TypeError, ValueError)) as many:
            md.forward_images(two, a["image_pe"], a["sparse"], a["dense"], which, True)
        print(f"{what}: {one.type.__name__}: {one.value}")
        assert one.type is many.type and str(one.value) == str(many.value), what


def test_one_workspace_serves_both_entries(models, images):
    """The multi-image call's workspace serves the single-image call after it: the buffer is not reallocated, and both
    results are those of a module that has run nothing else."""
    pe, _ = models
    image_pe = pe.get_dense_pe()
    sparse, dense = sparse_prompts(pe, 2, 3, seed=3)
    two, which = images[:2], [0, 1, 1]

    def fresh():
        return build_models(synth.synthetic_sam_decoder_state_dict(seed=0))[1].to(DEV)
    md = fresh()
    got_images = md.forward_images(two, image_pe, sparse, dense, which, True)
    buf = md._ws.data_ptr()
    got_one = md(two[:1], image_pe, sparse[:1], dense[:1], True)
    assert md._ws.data_ptr() == buf
    want_one = fresh()(two[:1], image_pe, sparse[:1], dense[:1], True)
    want_images = fresh().forward_images(two, image_pe, sparse, dense, which, True)
    for got, want in ((got_images, want_images), (got_one, want_one)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- (b) the range guard: one image's overflow stays that image's ----------------------------------------------------------------
def test_range_guard_is_per_image(models, images):
    pe, md = models
    image_pe = pe.get_dense_pe()
    two = images[:2].clone()
    two[1, 5, 10, 20] = 1e6   # past the f16x3 contract
    sparse, dense = sparse_prompts(pe, 2, 5, seed=7)
    which = np.array([1, 0, 1, 0, 1])
    r0, r1 = torch.as_tensor([1, 3], device=DEV), torch.as_tensor([0, 2, 4], device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m0, i0 = md(two[:1], image_pe, sparse[r0], dense[:1].expand(2, -1, -1, -1), True)          # f16x3, no event
    with pytest.warns(UserWarning, match="f16x3 range"):
        m1, i1 = md(two[1:], image_pe, sparse[r1], dense[:1].expand(3, -1, -1, -1), True)          # warned, re-run in f32
    md.on_overflow = "raise"
    try:
        with pytest.raises(PopeRangeError):
            md.forward_images(two, image_pe, sparse, dense, which, True)
    finally:
        md.on_overflow = "rerun_f32"
    events = md.overflow_events
    with pytest.warns(UserWarning, match="f16x3 range") as rec:
        m, i = md.forward_images(two, image_pe, sparse, dense, which, True)
    assert len([w for w in rec if "f16x3 range" in str(w.message)]) == 1
    assert md.overflow_events == events + 1          # what the per-image loop counts: image 1's call alone
    assert torch.equal(m[r0], m0) and torch.equal(i[r0], i0)
    assert torch.equal(m[r1], m1) and torch.equal(i[r1], i1)


# ---- (c), (d): Sam.forward -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sam():
    model, sd = small_sam(depth=2)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


def records():
    case = synth.sam_forward_case(DEV)
    g = torch.Generator().manual_seed(31)
    third = {"image": (torch.rand(3, 768, 1024, generator=g) * 255).to(DEV), "original_size": (480, 640),
             "point_coords": torch.tensor([[[400.0, 300.0]], [[700.0, 500.0]]], device=DEV),
             "point_labels": torch.ones(2, 1, dtype=torch.int, device=DEV),
             "boxes": torch.tensor([[250.0, 150.0, 600.0, 480.0], [500.0, 300.0, 900.0, 700.0]], device=DEV)}
    bare = {"image": (torch.rand(3, 1024, 683, generator=g) * 255).to(DEV), "original_size": (600, 400)}   # no prompt: one empty prompt
    return case + [third, bare]


@pytest.mark.parametrize("multimask", [True, False])
def test_forward_equals_the_predictor_per_record(sam, multimask):
    batch = records()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sam(batch, multimask_output=multimask)
        assert len(out) == len(batch)
        pr = SamPredictor(sam)
        for r, (x, o) in enumerate(zip(batch, out)):
            pr.set_torch_image(x["image"][None], x["original_size"])
            masks, iou, low = pr.predict_torch(x.get("point_coords"), x.get("point_labels"), x.get("boxes"), None, multimask)
            assert sorted(o) == ["iou_predictions", "low_res_logits", "masks"]
            B, Cm = low.shape[0], 3 if multimask else 1
            assert o["masks"].dtype == torch.bool and o["masks"].shape == (B, Cm, *x["original_size"])
            assert o["iou_predictions"].shape == (B, Cm) and o["low_res_logits"].shape == (B, Cm, 256, 256)
            assert torch.equal(o["low_res_logits"], low), r
            assert torch.equal(o["iou_predictions"], iou), r
            assert torch.equal(o["masks"], masks), r
            # torch's own CPU F.interpolate of the low-res logits
            ref = reference_logits(o["low_res_logits"].cpu().flatten(0, 1), tuple(x["image"].shape[-2:]), x["original_size"]) > 0
            assert torch.equal(o["masks"].cpu().flatten(0, 1), ref), r
    assert [o["masks"].shape[0] for o in out] == [2, 3, 2, 1]
    # a single record (the single-image decoder call) gives what it gives inside the batch
    alone = sam(batch[1:2], multimask_output=multimask)
    assert len(alone) == 1 and all(torch.equal(alone[0][k], out[1][k]) for k in out[1])


def test_forward_rejects_other_devices_and_cpu_records(sam):
    from pope_amd import _lib
    case = synth.sam_forward_case(DEV)
    with pytest.raises(_lib.PopeHipError):
        sam([case[0], dict(case[1], image=case[1]["image"].cpu())], True)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="is on"):
            sam([dict(case[0], boxes=case[0]["boxes"].to("cuda:1"))], True)


def test_forward_against_the_reference_fixture(sam, golden_dir):
    g = golden(golden_dir)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sam(synth.sam_forward_case(DEV), multimask_output=True)
    worst = 0.0
    for r, o in enumerate(out):
        for got, key in ((o["iou_predictions"], "iou_predictions"), (o["low_res_logits"][:, :, ::ROW_STEP], "low_res_rows")):
            ref = torch.from_numpy(g[f"{r}.{key}"])
            scale = max(1.0, float(ref.abs().max()))
            dev = float((got.cpu() - ref).abs().max()) / scale
            print(f"record {r} {key}: max |got - ref| / max(1, max |ref|) = {dev:.3e} (max |ref| = {float(ref.abs().max()):.3f})")
            worst = max(worst, dev)
        assert tuple(o["masks"].shape) == tuple(g[f"{r}.masks_shape"]) and tuple(o["low_res_logits"].shape) == tuple(g[f"{r}.low_res_shape"])
    print(f"largest relative deviation from the fixture: {worst:.3e}")
    assert worst <= REL
