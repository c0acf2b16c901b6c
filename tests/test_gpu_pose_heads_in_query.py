"""GPU: the image-conditioned pose heads inside the query.  `locate_match_pose_batch_u8(..., pose_regressor=)` with a
`mocope.MoCoPE` or a `pose_regressor_cnn.Mkpts_Reg_Model` returns, bit for bit, what the head returns when it is fed by hand:
the query's downloaded best-slot matches and an image pair made on the HOST by `resize_linear_cv_u8` from the reference image
and the best proposal's crop.  Every other key of the result is that of the call without a regressor.  The same with shared
frames, with a `ReferenceSet` that carries the reference side of the head (the MoCoPE backbone then sees Q images, not 2 Q), and
from the raw frames (`regress_pose_from_frames`).  Every comparison is an equality."""
import numpy as np
import pytest
import torch

from pope_amd import convnextv2, pose_regressor_cnn, synth
from pope_amd.crops import crop_proposals
from pope_amd.driver import encode_references, locate_match_pose_batch_u8, regress_pose_from_frames
from pope_amd.mocope import MoCoPE, regress_pose_fused_batch
from pope_amd.preprocess import resize_linear_cv_u8
from test_gpu_frame_query import assert_same_value, frames, generator, models, query, sam  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 70
SEED = 9
CNN_SIZE = 96          # the CNN head's test runs at another `pose_image_size` than the default


@pytest.fixture(scope="module")
def mocope(hip_lib):
    m = MoCoPE(S, "6d", backbone=convnextv2.ConvNeXtV2(**synth.MOCOPE_TRUNK))
    m.load_state_dict(synth.mocope_state_dict(S, "6d"), strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def cnn_head(hip_lib):
    m = pose_regressor_cnn.Mkpts_Reg_Model(S, "6d", backbone=convnextv2.ConvNeXtV2(**synth.CONVNEXT_SMALL))
    m.load_state_dict(synth.convnext_pose_state_dict("6d"), strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def case(models):
    """Three queries, the third without a proposal; `plain` is the call without a regressor."""
    cases = [synth.synthetic_frame_case(seed=31), synth.synthetic_frame_case(n_proposals=6, seed=32), synth.synthetic_frame_case(seed=31)]
    c = {"refs": np.stack([k[0] for k in cases]), "frames": np.stack([k[1] for k in cases]),
         "boxes": [cases[0][2], cases[1][2], np.zeros((0, 4), np.int64)], "K0": np.stack([k[3] for k in cases]), "K1": cases[0][4]}
    c["args"] = (*models, c["refs"], c["frames"], c["boxes"], c["K0"], c["K1"])
    c["plain"] = locate_match_pose_batch_u8(*c["args"])
    return c


def host_pairs(refs, frames, boxes, K1, outs, size):
    """The image pair of every query, made the parent commit's way: crops of the query's frame, the downloaded best proposal, the
    host twin of the resize, the fork's permute.  A query without a filled slot gets zeros (its result is dropped)."""
    img0, img1 = [], []
    for q, out in enumerate(outs):
        best = out["best_proposal"]
        if best < 0:
            img0.append(torch.zeros(3, size, size))
            img1.append(torch.zeros(3, size, size))
            continue
        crops = crop_proposals(torch.from_numpy(frames[q]).to(DEV), boxes[q], K1)["crops"].cpu().numpy()
        img0.append(torch.from_numpy(resize_linear_cv_u8(refs[q], size, size)).float().permute(2, 1, 0))
        img1.append(torch.from_numpy(resize_linear_cv_u8(crops[best], size, size)).float().permute(2, 1, 0))
    return torch.stack(img0).contiguous().to(DEV), torch.stack(img1).contiguous().to(DEV)


def best_matches(outs):
    counts = [len(o["mkpts0"][o["best_slot"]]) for o in outs]
    k0 = torch.from_numpy(np.concatenate([o["mkpts0"][o["best_slot"]] for o in outs])).to(DEV)
    k1 = torch.from_numpy(np.concatenate([o["mkpts1"][o["best_slot"]] for o in outs])).to(DEV)
    return k0, k1, counts


def assert_rest_is_plain(outs, plain):
    assert len(outs) == len(plain)
    for q, (got, want) in enumerate(zip(outs, plain)):
        assert "pose_regressed" not in want and set(got) == set(want) | {"pose_regressed"}, q
        for k in want:
            assert_same_value(got[k], want[k], (q, k))


def assert_regressed(outs, R, t, ok):
    for q, out in enumerate(outs):
        if not ok[q]:
            assert out["pose_regressed"] is None, q
            continue
        gR, gt = out["pose_regressed"]
        assert gR.shape == (3, 3) and gt.shape == (3,) and gR.dtype == np.float32 and gt.dtype == np.float32, q
        assert np.array_equal(gR, R[q].cpu().numpy()) and np.array_equal(gt, t[q].cpu().numpy()), q


def mocope_by_hand(model, c, outs, frames=None, boxes=None, refs=None, size=224, seed=SEED):
    k0, k1, counts = best_matches(outs)
    img0, img1 = host_pairs(c["refs"] if refs is None else refs, c["frames"] if frames is None else frames,
                            c["boxes"] if boxes is None else boxes, c["K1"], outs, size)
    want = regress_pose_fused_batch(model, k0, k1, counts, img0, img1, seed=seed)
    ok = [n >= 5 and int(s) == 0 for n, s in zip(counts, want["status"].tolist())]
    return want, ok, counts


def test_mocope_regresses_in_the_query(case, mocope):
    outs = locate_match_pose_batch_u8(*case["args"], pose_regressor=mocope, regressor_seed=SEED)
    assert_rest_is_plain(outs, case["plain"])
    want, ok, counts = mocope_by_hand(mocope, case, outs)
    assert counts[0] > S and counts[2] == 0 and ok[0] and not ok[2]          # the first query is sampled by the device sampler
    assert_regressed(outs, want["R"], want["t"], ok)
    assert outs[2]["pose_regressed"] is None and outs[0]["pose_regressed"] is not None
    assert bool(np.isfinite(outs[0]["pose_regressed"][0]).all())
    other = locate_match_pose_batch_u8(*case["args"], pose_regressor=mocope, regressor_seed=SEED + 1)
    assert not np.array_equal(other[0]["pose_regressed"][1], outs[0]["pose_regressed"][1])
    # the images matter: the reference side swapped between the first two queries moves the result
    swapped = mocope_by_hand(mocope, case, outs, refs=case["refs"][[1, 0, 2]])[0]
    assert not torch.equal(swapped["t"][0], want["t"][0])


def test_cnn_head_regresses_in_the_query(case, cnn_head):
    outs = locate_match_pose_batch_u8(*case["args"], pose_regressor=cnn_head, regressor_seed=SEED, pose_image_size=CNN_SIZE)
    assert_rest_is_plain(outs, case["plain"])
    img0, img1 = host_pairs(case["refs"], case["frames"], case["boxes"], case["K1"], outs, CNN_SIZE)
    t, R = cnn_head(None, None, img0, img1)
    ok = [o["best_proposal"] >= 0 for o in outs]
    assert ok == [True, True, False]
    assert_regressed(outs, R, t, ok)                 # this head reads no key points: None only where no slot was filled
    default = locate_match_pose_batch_u8(*case["args"], pose_regressor=cnn_head)
    assert not np.array_equal(default[0]["pose_regressed"][1], outs[0]["pose_regressed"][1])        # the size is part of the input


def test_shared_frame(case, mocope):
    """Queries 0 and 1 ask two references of frame 0, query 2 its own reference of frame 1."""
    fidx = [0, 0, 1]
    frames, boxes = case["frames"][:2], case["boxes"][:2]
    vit, matcher = case["args"][:2]
    shared = locate_match_pose_batch_u8(vit, matcher, case["refs"], frames, boxes, case["K0"], case["K1"], frame_index=fidx,
                                        pose_regressor=mocope, regressor_seed=SEED)
    repeated = locate_match_pose_batch_u8(vit, matcher, case["refs"], frames[fidx], [boxes[f] for f in fidx], case["K0"], case["K1"],
                                          pose_regressor=mocope, regressor_seed=SEED)
    for q, (got, want) in enumerate(zip(shared, repeated)):
        assert set(got) == set(want)
        for k in want:
            assert_same_value(got[k], want[k], (q, k))
    want, ok, _ = mocope_by_hand(mocope, case, shared, frames=frames[fidx], boxes=[boxes[f] for f in fidx])
    assert ok[0]
    assert_regressed(shared, want["R"], want["t"], ok)


class Counted:
    """Counts the images that pass through a module's forward."""

    def __init__(self, module):
        self.module, self.inner, self.calls, self.images = module, module.forward, 0, 0
        module.forward = self

    def __call__(self, x):
        self.calls += 1
        self.images += int(x.shape[0])
        return self.inner(x)

    def close(self):
        del self.module.forward          # back to the class's method


def test_reference_set_carries_the_reference_side(case, mocope, cnn_head):
    vit, matcher = case["args"][:2]
    rest = (case["frames"], case["boxes"], case["K0"], case["K1"])
    rows = [2, 0, 1]                                         # the set holds the references in another order
    raw = locate_match_pose_batch_u8(vit, matcher, case["refs"], *rest, pose_regressor=mocope, regressor_seed=SEED)
    stored = case["refs"][[1, 2, 0]]
    refset = encode_references(vit, matcher, stored, pose_regressor=mocope)
    assert refset.pose_img0.shape == (3, 3, 224, 224) and refset.pose_feat0.shape == (3, 1000)
    counted = Counted(mocope.convnextv2)
    try:
        got = locate_match_pose_batch_u8(vit, matcher, refset, *rest, ref_index=rows, pose_regressor=mocope, regressor_seed=SEED)
        assert (counted.calls, counted.images) == (1, 3)                       # the crops only
        by_select = locate_match_pose_batch_u8(vit, matcher, refset.select(rows), *rest, pose_regressor=mocope, regressor_seed=SEED)
        counted.calls = counted.images = 0
        locate_match_pose_batch_u8(vit, matcher, case["refs"], *rest, pose_regressor=mocope, regressor_seed=SEED)
        assert (counted.calls, counted.images) == (2, 6)                       # the raw-reference call runs both sides
    finally:
        counted.close()
    for outs in (got, by_select):
        for q, (g, w) in enumerate(zip(outs, raw)):
            assert set(g) == set(w)
            for k in w:
                assert_same_value(g[k], w[k], (q, k))
    assert raw[0]["pose_regressed"] is not None
    # the CNN head keeps the images alone
    cnn_set = encode_references(vit, matcher, stored, pose_regressor=cnn_head, pose_image_size=CNN_SIZE)
    assert cnn_set.pose_img0.shape == (3, 3, CNN_SIZE, CNN_SIZE) and cnn_set.pose_feat0 is None
    a = locate_match_pose_batch_u8(vit, matcher, cnn_set, *rest, ref_index=rows, pose_regressor=cnn_head, pose_image_size=CNN_SIZE)
    b = locate_match_pose_batch_u8(vit, matcher, case["refs"], *rest, pose_regressor=cnn_head, pose_image_size=CNN_SIZE)
    for q in range(3):
        assert_same_value(a[q]["pose_regressed"], b[q]["pose_regressed"], q)
    # a set made without the regressor, for another regressor object or for another size is refused; without a regressor and
    # with the key-point head every set is accepted as before
    plain_set = encode_references(vit, matcher, stored)
    assert plain_set.pose_img0 is None and plain_set.pose_for is None
    for bad, kw in ((plain_set, dict(pose_regressor=mocope)), (cnn_set, dict(pose_regressor=mocope)),
                    (refset, dict(pose_regressor=cnn_head)), (refset, dict(pose_regressor=mocope, pose_image_size=96)),
                    (refset.select(rows), dict(pose_regressor=mocope, pose_image_size=96))):
        with pytest.raises(ValueError, match="not encoded for this pose_regressor"):
            locate_match_pose_batch_u8(vit, matcher, bad, *rest, ref_index=None if bad.index is not None else rows, **kw)
    unchanged = locate_match_pose_batch_u8(vit, matcher, refset, *rest, ref_index=rows)
    for q, (g, w) in enumerate(zip(unchanged, case["plain"])):
        assert set(g) == set(w)
        for k in w:
            assert_same_value(g[k], w[k], (q, k))
    # logits belong to the backbone weights they were computed with
    p = next(mocope.convnextv2.parameters())
    with torch.no_grad():
        p.mul_(1.0)
    with pytest.raises(ValueError, match="backbone changed"):
        locate_match_pose_batch_u8(vit, matcher, refset, *rest, ref_index=rows, pose_regressor=mocope)


def test_logits_in_place_of_an_image(mocope):
    B = 3
    k0, k1 = (t.to(DEV) for t in synth.pose_regressor_matches([S, 90, 12], seed=7))
    g = torch.Generator().manual_seed(5)
    i0, i1 = (torch.rand(B, 3, 64, 64, generator=g).to(DEV) * 255 for _ in range(2))
    want = regress_pose_fused_batch(mocope, k0, k1, [S, 90, 12], i0, i1, seed=SEED)
    f0, f1 = mocope.image_logits(i0), mocope.image_logits(i1)
    for kw in (dict(img1=i1, feat0=f0), dict(img0=i0, feat1=f1), dict(feat0=f0, feat1=f1)):
        got = regress_pose_fused_batch(mocope, k0, k1, [S, 90, 12], seed=SEED, **kw)
        assert torch.equal(got["R"], want["R"]) and torch.equal(got["t"], want["t"]) and torch.equal(got["status"], want["status"])
    with pytest.raises(ValueError):
        regress_pose_fused_batch(mocope, k0, k1, [S, 90, 12], i0, i1, seed=SEED, feat0=f0)
    with pytest.raises(ValueError):
        regress_pose_fused_batch(mocope, k0, k1, [S, 90, 12], None, i1, seed=SEED, feat0=f0[:2])


def test_from_the_raw_frames(sam, frames, models, query, mocope):  # noqa: F811
    refs, K0, K1 = query
    gen = generator(sam)
    got = regress_pose_from_frames(gen, *models, mocope, refs, frames, K0, K1, regressor_seed=SEED)
    proposals = gen.propose_batch(frames)
    want = locate_match_pose_batch_u8(*models, refs, frames, proposals, K0, K1, pose_regressor=mocope, regressor_seed=SEED)
    assert len(got) == len(want) == len(frames)
    for q, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) | {"proposals"} and "pose_regressed" in w, q
        for k in w:
            assert_same_value(g[k], w[k], (q, k))
        assert np.array_equal(g["proposals"], proposals[q])
    print("proposals per frame", [len(p) for p in proposals], "regressed", [o["pose_regressed"] is not None for o in got])
    assert any(len(p) == 0 for p in proposals) and all(o["pose_regressed"] is None for o, p in zip(got, proposals) if len(p) == 0)
