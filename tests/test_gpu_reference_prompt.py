"""GPU: encode the reference once, match many crops (Matcher.encode_reference, data['reference'] / data['image0_index'],
the ref0_of_pair index of pope_fine_preprocess_f32, driver.encode_references / ReferenceSet / ref_index).

The contract is equality: every published output of an indexed call is, bit for bit, that of the plain call on
image0 = refs.index_select(0, image0_index) — no tolerance appears below.  Each test first shows on the PLAIN call that matches
exist (every live pair, and pairs of different references), so an all-empty result cannot pass."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_gpu_driver_batch import _assert_same_step

pytestmark = pytest.mark.gpu

KEYS = ("conf_matrix", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f", "m_bids")
PLAIN_KEYS = ("bs", "hw0_i", "hw1_i", "hw0_c", "hw1_c", "hw0_f", "hw1_f", "W")
SHIFTS = ((8, 16), (16, 8), (0, 8), (8, 0), (8, 8), (16, 16))   # whole coarse cells: the shifted crop matches cell on cell


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def peaked_sd(golden_dir):
    from pope_amd import synth
    fx = np.load(os.path.join(golden_dir, "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    return sd


def build_matcher(dev, sd, attention="linear"):
    from pope_amd.matcher import Matcher, default_cfg
    cfg = copy.deepcopy(default_cfg)
    cfg["coarse"]["attention"] = attention
    m = Matcher(cfg).eval()
    m.load_state_dict(dict(sd), strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def matcher(dev, peaked_sd):
    return build_matcher(dev, peaked_sd)


def make_case(dev, R, index, hw0, hw1, seed, dead=()):
    """R references of size hw0 and one crop of size hw1 per entry of `index`: the top-left hw1 window of that reference
    shifted by whole coarse cells, plus noise; a `dead` crop is all zeros (how the driver pads an unfilled slot)."""
    from pope_amd import synth
    refs = synth.synthetic_gray_pairs(R, hw0[0], hw0[1], seed=seed)[0]
    g = torch.Generator().manual_seed(1000 + seed)
    crops = []
    for b, r in enumerate(index):
        c = torch.roll(refs[r], shifts=SHIFTS[b % len(SHIFTS)], dims=(1, 2))[:, :hw1[0], :hw1[1]]
        c = (c + 0.02 * torch.randn(c.shape, generator=g)).clamp_(0, 1)
        crops.append(torch.zeros_like(c) if b in dead else c)
    return refs.to(dev), torch.stack(crops).contiguous().to(dev), torch.as_tensor(list(index), dtype=torch.int64)


def plain_call(m, refs, crops, index, **extra):
    data = {"image0": refs.index_select(0, index.to(refs.device)), "image1": crops, **extra}
    m(data)
    return data


def assert_matches_exist(plain, index, dead=(), tag=""):
    n = len(index)
    counts = torch.bincount(plain["b_ids"].cpu(), minlength=n).tolist()
    print(f"{tag}: matches per pair {counts} (references {index.tolist()}, dead {list(dead)})")
    assert all(counts[b] > 0 for b in range(n) if b not in dead), (tag, counts)
    used = {int(index[b]) for b in range(n) if b not in dead and counts[b] > 0}
    if len(set(index.tolist())) > 1:
        assert len(used) >= 2, (tag, "pairs of at least two different references must match", counts)


def assert_same_outputs(got, want, tag):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
        assert torch.equal(got[k], want[k]), (tag, k)
    for k in PLAIN_KEYS:
        assert tuple(got[k]) == tuple(want[k]) if hasattr(want[k], "__len__") else got[k] == want[k], (tag, k)
    assert sorted(k for k in got if k not in ("reference", "image0", "image0_index")) == sorted(k for k in want if k != "image0"), tag


def both_indexed_calls(m, refs, crops, index, ref=None, **extra):
    """The two forms of the indexed call: image0 [R] + index (the encoding built inside and dropped), and a kept encoding."""
    a = {"image0": refs, "image0_index": index, "image1": crops, **extra}
    m(a)
    ref = m.encode_reference(refs) if ref is None else ref
    b = {"reference": ref, "image0_index": index, "image1": crops, **extra}
    m(b)
    assert "image0" not in b
    return a, b, ref


def check_equal_to_plain(m, refs, crops, index, dead=(), tag=""):
    want = plain_call(m, refs, crops, index)
    assert_matches_exist(want, index, dead, tag)
    a, b, ref = both_indexed_calls(m, refs, crops, index)
    assert_same_outputs(a, want, tag + " / image0 + index")
    assert_same_outputs(b, want, tag + " / kept encoding")
    # only_att_fea: the coarse transformer's outputs themselves
    f_want = m({"image0": refs.index_select(0, index.to(refs.device)), "image1": crops}, only_att_fea=True)
    f_got = m({"reference": ref, "image0_index": index, "image1": crops}, only_att_fea=True)
    assert all(torch.equal(g, w) for g, w in zip(f_got, f_want)), tag + " / only_att_fea"
    return ref


# ---- 1. the indexed call equals the repeated-image call (L == S: both streams in one buffer) -----------------------------
@pytest.mark.parametrize("index", [(0, 0, 0, 1, 1, 1), (1, 0, 1, 0, 0, 1)])
def test_indexed_call_equals_the_repeated_image_call(dev, matcher, index):
    refs, crops, idx = make_case(dev, 2, index, (128, 160), (128, 160), seed=11)
    ref = check_equal_to_plain(matcher, refs, crops, idx, tag=f"128x160, index {index}")
    assert ref.R == 2 and ref.mode == "f16x3" and tuple(ref.hw_i) == (128, 160)
    lead = ref.leading("f16x3", "f16x3")[0]
    assert lead.shape == (2, 16 * 20, 256) and ref.backbone("f16x3")["fine"].shape == (2, 128, 64, 80)
    # the index as a list, and as a device tensor
    want = plain_call(matcher, refs, crops, idx)
    for form in (list(index), idx.to(dev)):
        got = {"reference": ref, "image0_index": form, "image1": crops}
        matcher(got)
        assert_same_outputs(got, want, f"index given as {type(form).__name__}")


# ---- 2. L != S: two launch sequences, two buffers ------------------------------------------------------------------------
def test_references_and_crops_of_different_sizes(dev, matcher):
    refs, crops, idx = make_case(dev, 2, (0, 1, 1, 0), (128, 160), (96, 96), seed=12)
    check_equal_to_plain(matcher, refs, crops, idx, tag="128x160 vs 96x96")


# ---- 3. a dead pair, one pair, an unused reference ------------------------------------------------------------------------
def test_dead_pair_single_pair_and_unused_reference(dev, matcher):
    refs, crops, idx = make_case(dev, 2, (0, 1, 0, 1), (128, 160), (128, 160), seed=13, dead=(2,))
    check_equal_to_plain(matcher, refs, crops, idx, dead=(2,), tag="pair 2 all zeros")
    refs, crops, idx = make_case(dev, 1, (0,), (128, 160), (128, 160), seed=14)
    check_equal_to_plain(matcher, refs, crops, idx, tag="n = 1, R = 1")
    want = plain_call(matcher, refs, crops, idx)                       # the default index: arange(n), R == n
    got = {"reference": matcher.encode_reference(refs), "image1": crops}
    matcher(got)
    assert_same_outputs(got, want, "no index given")
    refs, crops, idx = make_case(dev, 3, (2, 0, 2), (128, 160), (128, 160), seed=15)
    check_equal_to_plain(matcher, refs, crops, idx, tag="reference 1 unused")


# ---- 4. attention = 'full' on the coarse transformer ------------------------------------------------------------------------
def test_full_attention_coarse_transformer(dev, peaked_sd):
    m = build_matcher(dev, peaked_sd, attention="full")
    assert m.loftr_coarse.attention == "full" and m.loftr_coarse.n_leading_self == 1
    refs, crops, idx = make_case(dev, 2, (0, 1, 1, 0, 0), (64, 64), (64, 64), seed=16)
    check_equal_to_plain(m, refs, crops, idx, tag="full attention, 64x64")


# ---- 5. reuse: across crop batches, and across a change of weights ----------------------------------------------------------
def test_one_encoding_serves_many_calls_and_follows_the_weights(dev, peaked_sd):
    m = build_matcher(dev, peaked_sd)
    refs, crops_a, idx_a = make_case(dev, 2, (0, 0, 1), (128, 160), (128, 160), seed=17)
    _, crops_b, idx_b = make_case(dev, 2, (1, 0, 1, 1), (128, 160), (128, 160), seed=17)
    crops_b = torch.flip(crops_b, dims=(0,)).contiguous()
    idx_b = torch.flip(idx_b, dims=(0,)).contiguous()
    ref = m.encode_reference(refs)
    key = ref.key
    for crops, idx, tag in ((crops_a, idx_a, "first batch"), (crops_b, idx_b, "second batch")):
        want = plain_call(m, refs, crops, idx)
        assert_matches_exist(want, idx, tag=tag)
        got = {"reference": ref, "image0_index": idx, "image1": crops}
        m(got)
        assert_same_outputs(got, want, tag)
    assert ref.key == key                                   # nothing was re-encoded in between
    old = plain_call(m, refs, crops_a, idx_a)
    # other weights: the leading 'self' layer (inside the encoding), a later layer and the fine head of the backbone move
    g = torch.Generator().manual_seed(5)
    other = {k: v.clone() for k, v in peaked_sd.items()}
    for k in other:
        if k.startswith(("loftr_coarse.layers.0.", "loftr_coarse.layers.3.", "backbone.layer1_outconv2.3.")) and other[k].dim() > 1:
            other[k] += 0.05 * other[k].std() * torch.randn(other[k].shape, generator=g)
    m.load_state_dict(other, strict=True)
    want = plain_call(m, refs, crops_a, idx_a)
    assert_matches_exist(want, idx_a, tag="other weights")
    assert not torch.equal(want["conf_matrix"], old["conf_matrix"])        # the weights matter
    got = {"reference": ref, "image0_index": idx_a, "image1": crops_a}
    m(got)                                                                  # the stale-key path: re-encoded from the kept image
    assert ref.key != key
    assert_same_outputs(got, want, "same encoding object under other weights")
    assert not torch.equal(got["conf_matrix"], old["conf_matrix"])


# ---- 6. the range guard: one policy per call -------------------------------------------------------------------------------
def test_range_guard_of_a_crop_reruns_the_call_in_fp32(dev, peaked_sd):
    from pope_amd import loftr
    from pope_amd._lib import PopeRangeError
    m = build_matcher(dev, peaked_sd)
    refs, crops, idx = make_case(dev, 2, (0, 1, 0, 1), (128, 160), (128, 160), seed=18)
    ref = m.encode_reference(refs)
    quiet = plain_call(m, refs, crops, idx)
    crops[1] *= 1.0e4                             # |x| * 8 >= 65504: the stem gather of the crop side raises the flag; a scaled
                                                  # image keeps its structure, where a single huge pixel leaves the pair without matches
    with pytest.warns(UserWarning, match="LoFTR backbone"):
        want = plain_call(m, refs, crops, idx)
    assert_matches_exist(want, idx, tag="one crop outside the f16x3 range")
    assert not torch.equal(want["conf_matrix"][0], quiet["conf_matrix"][0])   # pair 0 too went through the fp32 backbone
    assert "f32" not in ref._bb
    with pytest.warns(UserWarning, match="LoFTR backbone"):
        a, b, _ = both_indexed_calls(m, refs, crops, idx, ref=ref)
    assert_same_outputs(a, want, "range event / image0 + index")
    assert_same_outputs(b, want, "range event / kept encoding")
    assert "f32" in ref._bb and "f16x3" in ref._bb          # the fp32 form was built from the kept image and is kept too
    old = loftr.ON_OVERFLOW
    try:
        loftr.ON_OVERFLOW = "raise"
        with pytest.raises(PopeRangeError):
            plain_call(m, refs, crops, idx)
        with pytest.raises(PopeRangeError):
            m({"reference": ref, "image0_index": idx, "image1": crops})
        with pytest.raises(PopeRangeError):
            m({"image0": refs, "image0_index": idx, "image1": crops})
    finally:
        loftr.ON_OVERFLOW = old


def test_range_guard_of_a_reference_makes_its_encoding_fp32(dev, peaked_sd):
    """The flag rises at encode time: the encoding is fp32, and a call that uses it runs its backbone in fp32 for the crops of
    the same size too — what the plain call does with the flagged image in its batch."""
    m = build_matcher(dev, peaked_sd)
    refs, crops, idx = make_case(dev, 2, (0, 1, 1), (128, 160), (128, 160), seed=19)
    refs[0] *= 1.0e4
    with pytest.warns(UserWarning, match="LoFTR backbone"):
        want = plain_call(m, refs, crops, idx)
    assert_matches_exist(want, idx, tag="one reference outside the f16x3 range")
    ref = m.encode_reference(refs)
    assert ref.mode == "f32"
    with pytest.warns(UserWarning, match="LoFTR backbone"):
        a, b, _ = both_indexed_calls(m, refs, crops, idx, ref=ref)
    assert_same_outputs(a, want, "flagged reference / image0 + index")
    assert_same_outputs(b, want, "flagged reference / kept encoding")


# ---- 7. the ref0_of_pair index of pope_fine_preprocess_f32 at op level -------------------------------------------------------------------------
def _fine_entry(fp, f0, f1, c0, c1, b, i, j, wc, stride, precision, ref0=None):
    from pope_amd import _lib
    lib = _lib.lib()
    dwp, mwp = fp._weights(precision)
    db, mb = fp._hip["biases"]
    M, W, Cf = int(b.shape[0]), fp.W, fp.d_model_f
    out = torch.full((2 * M, W * W, Cf), float("nan"), dtype=torch.float32, device=f0.device)
    nbytes = lib.pope_fine_preprocess_workspace_bytes(M, W, c0.shape[2], Cf)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=f0.device)
    flag = torch.zeros(1, dtype=torch.int32, device=f0.device)
    s0, s1 = (C.c_longlong * 4)(*f0.stride()), (C.c_longlong * 4)(*f1.stride())
    args = [C.c_void_p(f0.data_ptr()), s0, f0.shape[2], f0.shape[3], wc, C.c_void_p(f1.data_ptr()), s1, f1.shape[2], f1.shape[3], wc,
            C.c_void_p(c0.data_ptr()), C.c_void_p(c1.data_ptr()), c0.shape[1], c1.shape[1], c0.shape[2], Cf,
            C.c_void_p(b.data_ptr()), C.c_void_p(i.data_ptr()), C.c_void_p(j.data_ptr()), M, W, stride,
            C.c_void_p(dwp.data_ptr()), C.c_void_p(db.data_ptr()), C.c_void_p(mwp.data_ptr()), C.c_void_p(mb.data_ptr()),
            _lib.PRECISIONS[precision], C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(flag.data_ptr()),
            None if ref0 is None else C.c_void_p(ref0.data_ptr()), int(c0.shape[0]), int(f0.shape[0])]
    with torch.cuda.device(f0.device):
        _lib.check(lib.pope_fine_preprocess_f32(*args, _lib.stream_of(f0.device)), "pope_fine_preprocess_f32")
    assert int(flag.item()) == 0
    return out


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_indexed_fine_preprocess_equals_the_entry_on_the_expanded_map(dev, peaked_sd, precision):
    from pope_amd.loftr import FinePreprocess
    from pope_amd.matcher import default_cfg
    fp = FinePreprocess(default_cfg).eval()
    fp.load_state_dict({k[len("fine_preprocess."):]: v for k, v in peaked_sd.items() if k.startswith("fine_preprocess.")}, strict=True)
    fp = fp.to(dev)
    g = torch.Generator().manual_seed(37)
    M, n, R, hf, wf, s = 37, 5, 2, 24, 32, 4
    hc, wc = hf // s, wf // s
    # map 0 as the backbone hands it over (the interior of a bordered NHWC buffer, permuted), map 1 as a plain NCHW tensor
    f0 = torch.randn(R, hf + 2, wf + 2, 128, generator=g).to(dev)[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)
    f1 = torch.randn(n, 128, hf, wf, generator=g).to(dev)
    c0, c1 = torch.randn(n, hc * wc, 256, generator=g).to(dev), torch.randn(n, hc * wc, 256, generator=g).to(dev)
    b = torch.randint(0, n, (M,), generator=g).sort().values
    b[:n] = torch.arange(n)                                  # every pair has a match
    b = b.sort().values.to(dev)
    i, j = torch.randint(0, hc * wc, (M,), generator=g), torch.randint(0, hc * wc, (M,), generator=g)
    i[0], j[0], i[1], j[1] = 0, hc * wc - 1, hc * wc - 1, 0      # corners: windows reach outside the map
    i, j = i.to(dev), j.to(dev)
    ref0 = torch.tensor([1, 0, 0, 1, 1], dtype=torch.int64, device=dev)
    expanded = f0.index_select(0, ref0)
    assert not torch.equal(f0[0], f0[1]) and set(b.tolist()) == set(range(n))
    tail = (b, i, j, wc, s, precision)
    want = _fine_entry(fp, expanded, f1, c0, c1, *tail)          # no index: one map-0 row per pair
    assert bool(torch.isfinite(want).all())
    got = _fine_entry(fp, f0, f1, c0, c1, *tail, ref0=ref0)
    assert torch.equal(got, want)
    # a NULL index is the identity index on the expanded map
    ident = _fine_entry(fp, expanded, f1, c0, c1, *tail, ref0=torch.arange(n, dtype=torch.int64, device=dev))
    assert torch.equal(ident, want)
    # and through the module, which is how the Matcher reaches it
    data = {"hw0_f": (hf, wf), "hw0_c": (hc, wc), "hw1_c": (hc, wc), "b_ids": b, "i_ids": i, "j_ids": j}
    (w0, w1), _ = fp._run(f0, f1, c0, c1, data, s, precision, ref0)
    assert torch.equal(torch.cat([w0, w1]), want)
    # the index matters: the wrong rows give other windows
    swapped = _fine_entry(fp, f0, f1, c0, c1, *tail, ref0=1 - ref0)
    assert not torch.equal(swapped[:M], want[:M]) and torch.equal(swapped[M:], want[M:])


# ---- 8. the driver: a ReferenceSet and ref_index ---------------------------------------------------------------------------
def test_driver_with_a_reference_set_equals_the_call_with_images(dev, sd0, peaked_sd):
    """`locate_match_pose_batch_u8` level (the frame-level calls hand their references to it unchanged; their counting of a set
    is pinned in tests/test_reference_prompt_cpu.py)."""
    from pope_amd import synth
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd.driver import encode_references, locate_match_pose_batch_u8
    vit, m = load_dinov2_model(state_dict=sd0).to(dev), build_matcher(dev, peaked_sd)
    ca, cb = synth.synthetic_frame_case(seed=31), synth.synthetic_frame_case(seed=32)
    refs_bgr = np.stack([ca[0], cb[0]])
    ref_index = [0, 0, 1, 0]
    frames = np.stack([ca[1], ca[1], cb[1], ca[1]])
    boxes = [ca[2], ca[2][::-1].copy(), cb[2], np.roll(ca[2], 3, axis=0)]       # 8 proposals each, query by query another order
    K0 = np.stack([ca[3], ca[3], cb[3], ca[3]])
    want = locate_match_pose_batch_u8(vit, m, refs_bgr[ref_index], frames, boxes, K0, ca[4])
    assert all(len(b) == 8 for b in boxes) and len(want) == 4
    for q, w in enumerate(want):                              # real pose problems, for both references
        assert w["best_proposal"] >= 0 and len(w["mconf"][w["best_slot"]]) >= 50, q
    assert want[0]["pose"] is not None
    refset = encode_references(vit, m, refs_bgr)
    assert len(refset) == 2 and refset.cls.shape == (2, 384) and refset.gray.shape == (2, 1, 256, 256)
    calls = {"ReferenceSet + ref_index": locate_match_pose_batch_u8(vit, m, refset, frames, boxes, K0, ca[4], ref_index=ref_index),
             "ReferenceSet.select": locate_match_pose_batch_u8(vit, m, refset.select(ref_index), frames, boxes, K0, ca[4]),
             "images + ref_index": locate_match_pose_batch_u8(vit, m, refs_bgr, frames, boxes, K0, ca[4], ref_index=ref_index)}
    for tag, outs in calls.items():
        assert len(outs) == 4
        for q, (got, w) in enumerate(zip(outs, want)):
            for k in ("boxes", "K_crops", "pre_bbox", "pre_K"):
                assert np.array_equal(got[k], w[k]), (tag, q, k)
            _assert_same_step(got, w, f"{tag}, query {q}")
            assert (got["pose"] is None) == (w["pose"] is None), (tag, q)
            for name, a, b in zip(("R", "t", "inliers"), got["pose"] or (), w["pose"] or ()):
                assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (tag, q, name)
