"""GPU: the batched driver step (pope_amd/driver.py:locate_and_match_batch, locate_match_pose_batch_u8) and its two device
kernels (vote.hip) — the vote against `cls_cosine` + the host `streaming_top3` per query, the slot tally against numpy, and the
batched calls against the single-query functions run alone, bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEGMENTS = (0, 1, 3, 8, 70, 200)
# what the rows of each segment look like, per feature width (the second width leaves a tail in the 64-lane stride)
LAYOUTS = {384: ("empty", "positive", "nonpositive", "ties", "ascending", "random_dup"),
           100: ("empty", "nonpositive", "descending", "descending", "random_dup", "ascending")}


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev, sd0):
    from pope_amd import synth
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd.matcher import Matcher, default_cfg
    vit = load_dinov2_model(state_dict=sd0).to(dev)
    matcher = Matcher(default_cfg).eval()
    matcher.load_state_dict(synth.synthetic_matcher_state_dict(seed=0), strict=True)
    return vit, matcher.to(dev)


@pytest.fixture(scope="module")
def peaked_models(dev, sd0, golden_dir):
    from pope_amd import synth
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd.matcher import Matcher, default_cfg
    fx = np.load(os.path.join(golden_dir, "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    matcher = Matcher(default_cfg).eval()
    matcher.load_state_dict(sd, strict=True)
    return load_dinov2_model(state_dict=sd0).to(dev), matcher.to(dev)


# ---- 1. the vote kernel alone ------------------------------------------------------------------------------------------
def _segment_rows(kind, P, ref, rng):
    """P rows a * ref + b * (noise orthogonal to ref, of ref's norm): cosine a / sqrt(a^2 + b^2), in the order `kind` asks for."""
    D = ref.size
    unit = ref / np.linalg.norm(ref)

    def row(cos):
        n = rng.normal(size=D)
        n -= (n @ unit) * unit
        n *= np.linalg.norm(ref) / np.linalg.norm(n)
        return cos * ref + np.sqrt(max(0.0, 1.0 - cos * cos)) * n

    if kind == "empty":
        return np.zeros((0, D))
    if kind == "positive":
        cos = np.full(P, 0.4)
    elif kind == "nonpositive":
        cos = -np.linspace(0.2, 0.8, P)
    elif kind == "ties":
        return np.tile(row(0.6), (P, 1))
    elif kind == "ascending":
        cos = np.linspace(0.05, 0.9, P)
    elif kind == "descending":
        cos = np.linspace(0.9, 0.05, P)
    else:
        cos = rng.uniform(-0.9, 0.9, P)
    rows = np.stack([row(c) for c in cos])
    if kind == "nonpositive" and P >= 3:
        rows[1] = 0.0                      # an all-zero row scores exactly 0: still not strictly greater than an empty slot
    if kind == "random_dup":
        rows[P // 4] = row(0.95)           # the top score of the segment, and its exact duplicate later on
        rows[(3 * P) // 4] = rows[P // 4]
    return rows


@pytest.mark.parametrize("D", sorted(LAYOUTS))
def test_vote_kernel_matches_cosine_and_host_vote_per_query(dev, D):
    from pope_amd import ops
    rng = np.random.default_rng(D)
    refs = rng.normal(size=(len(SEGMENTS), D))
    rows = [_segment_rows(kind, P, refs[q], rng) for q, (kind, P) in enumerate(zip(LAYOUTS[D], SEGMENTS))]
    cls_ref = torch.from_numpy(refs.astype(np.float32)).to(dev)
    cls_prop = torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(dev)
    out = ops.vote_top3_batch(cls_ref, cls_prop, SEGMENTS, eps=1e-8)
    seg = np.concatenate([[0], np.cumsum(SEGMENTS)])
    assert out["seg"].cpu().tolist() == seg.tolist() and out["scores"].shape == (seg[-1],)
    slot_scores, slot_index = out["slot_scores"].cpu().numpy(), out["slot_index"].cpu().numpy()
    pair_row, pair_live = out["pair_row"].cpu().numpy().reshape(-1, 3), out["pair_live"].cpu().numpy().reshape(-1, 3)
    assert slot_index.dtype == np.int64 and pair_row.dtype == np.int32 and pair_live.dtype == np.uint8
    for q, (kind, P) in enumerate(zip(LAYOUTS[D], SEGMENTS)):
        got = out["scores"][seg[q]:seg[q + 1]]
        if P:
            assert torch.equal(got, ops.cls_cosine(cls_ref[q:q + 1], cls_prop[seg[q]:seg[q + 1]], eps=1e-8)), (q, kind)
        want_scores, want_index = ops.streaming_top3(got.cpu().numpy())
        assert np.array_equal(slot_scores[q], want_scores) and np.array_equal(slot_index[q], want_index), (q, kind)
        assert np.array_equal(pair_live[q], (want_index >= 0).astype(np.uint8)), (q, kind)
        live = want_index >= 0
        assert np.array_equal(pair_row[q][live], (seg[q] + want_index)[live]), (q, kind)
        assert ((pair_row[q] >= 0) & (pair_row[q] < seg[-1])).all()
        # the segment is what its name says, so every branch of the vote is met
        s = got.cpu().numpy()
        if kind in ("empty", "nonpositive"):
            assert (s <= 0).all() and (want_index == -1).all()
        elif kind == "ascending":
            assert (np.diff(s) > 0).all() and sorted(want_index) == [P - 3, P - 2, P - 1]
        elif kind == "descending":
            assert (np.diff(s) < 0).all() and list(want_index) == [0, 1, 2][:P] + [-1] * (3 - min(P, 3))
        elif kind == "ties":
            assert (s == s[0]).all() and list(want_index) == [0, 1, 2]
        elif kind == "random_dup":
            assert s[P // 4] == s[(3 * P) // 4] == s.max() and {P // 4, (3 * P) // 4} <= set(want_index)


# ---- 2. the tally kernel alone -----------------------------------------------------------------------------------------
def _tally_numpy(m_bids, mconf, mk0, mk1, live, thr):
    n_pairs = len(live)
    begin = np.searchsorted(m_bids, np.arange(n_pairs), side="left").astype(np.int32)
    count = (np.searchsorted(m_bids, np.arange(n_pairs), side="right") - begin).astype(np.int32)
    score = np.array([int((mconf[begin[b]:begin[b] + count[b]] > np.float32(thr)).sum()) if live[b] else 0 for b in range(n_pairs)],
                     np.int64).reshape(-1, 3)
    best_slot = np.argmax(score, axis=1).astype(np.int32)
    best_pair = 3 * np.arange(len(score)) + best_slot
    best_count = np.where(live[best_pair] != 0, count[best_pair], 0).astype(np.int32)
    rows = np.concatenate([np.arange(begin[b], begin[b] + n) for b, n in zip(best_pair, best_count)]).astype(np.int64)
    return begin, count, score, best_slot, best_count, mk0[rows], mk1[rows]


def test_slot_tally_matches_numpy(dev):
    from pope_amd import ops
    rng = np.random.default_rng(7)
    thr = np.float32(0.9)
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(2))
    #          q0: plain        q1: three-way tie   q2: all zero; live empty, dead empty   q3: dead pair with matches
    counts = [40, 35, 30,       25, 25, 25,         20, 0, 0,                              30, 40, 30]
    live = np.array([1, 1, 1,   1, 1, 1,            1, 1, 0,                               1, 0, 1], np.uint8)
    conf = [rng.uniform(0.2, 1.0, n).astype(np.float32) for n in counts]
    conf[0][:3] = (thr, below, above)                       # only the last of the three counts
    for b in (3, 4, 5):                                      # exactly seven above the threshold in each slot of query 1
        conf[b] = rng.uniform(0.2, 0.89, 25).astype(np.float32)
        conf[b][rng.permutation(25)[:7]] = rng.uniform(0.91, 1.0, 7).astype(np.float32)
    conf[6] = np.concatenate([np.full(10, thr), np.full(5, below), rng.uniform(0.2, 0.89, 5).astype(np.float32)])
    conf[9] = np.minimum(conf[9], np.float32(0.95))
    conf[9][:5] = 0.93                                       # slot 0 of query 3: at least five
    conf[10][:] = 0.99                                       # the dead slot would win if it were counted
    conf[11][:] = 0.2
    conf[11][:29] = 0.97                                     # slot 2 beats slot 0
    mconf = np.concatenate(conf)
    m_bids = np.repeat(np.arange(12), counts).astype(np.int64)
    M = len(m_bids)
    assert M == 300 and (np.diff(m_bids) >= 0).all()
    mk0 = rng.uniform(0, 256, (M, 2)).astype(np.float32)
    mk1 = rng.uniform(0, 256, (M, 2)).astype(np.float32)
    want = _tally_numpy(m_bids, mconf, mk0, mk1, live, thr)
    assert list(want[2][1]) == [7, 7, 7] and want[3][1] == 0            # the tie goes to slot 0
    assert list(want[2][2]) == [0, 0, 0] and want[3][2] == 0 and want[4][2] == 20
    assert want[2][3][1] == 0 and want[3][3] == 2 and want[2][0][0] == int((conf[0] > thr).sum())
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    got = ops.slot_tally(up(m_bids), up(mconf), up(mk0), up(mk1), up(live), conf_thr=0.9)
    names = ("pair_begin", "pair_count", "matching_score", "best_slot", "best_count")
    for name, w in zip(names, want[:5]):
        g = got[name].cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    total = int(want[4].sum())
    assert got["best_kpts0"].shape == (M, 2) and got["best_kpts1"].shape == (M, 2)
    assert np.array_equal(got["best_kpts0"][:total].cpu().numpy(), want[5])
    assert np.array_equal(got["best_kpts1"][:total].cpu().numpy(), want[6])


def test_slot_tally_without_matches(dev):
    from pope_amd import ops
    el = torch.empty(0, dtype=torch.int64, device=dev)
    ef = torch.empty(0, dtype=torch.float32, device=dev)
    got = ops.slot_tally(el, ef, ef.reshape(0, 2), ef.reshape(0, 2), torch.tensor([1, 1, 0, 1, 0, 0], dtype=torch.uint8, device=dev))
    for name, shape in (("pair_begin", (6,)), ("pair_count", (6,)), ("matching_score", (2, 3)), ("best_slot", (2,)), ("best_count", (2,))):
        assert tuple(got[name].shape) == shape and int(got[name].abs().sum()) == 0, name
    assert got["best_kpts0"].shape == (0, 2) and got["best_kpts1"].shape == (0, 2)


# ---- 3. locate_and_match_batch == locate_and_match per query -----------------------------------------------------------
def _assert_same_step(got, want, tag):
    assert torch.equal(got["scores"], want["scores"]), tag
    assert np.array_equal(got["slot_index"], want["slot_index"]) and got["slot_index"].dtype == want["slot_index"].dtype, tag
    assert np.array_equal(got["slot_scores"], want["slot_scores"]) and got["slot_scores"].dtype == want["slot_scores"].dtype, tag
    assert np.array_equal(got["matching_score"], want["matching_score"]) and got["matching_score"].dtype == np.int64, tag
    assert got["best_slot"] == want["best_slot"] and got["best_proposal"] == want["best_proposal"], tag
    for s in range(3):
        for k in ("mkpts0", "mkpts1", "mconf"):
            assert got[k][s].shape == want[k][s].shape, (tag, k, s, got[k][s].shape, want[k][s].shape)
            assert got[k][s].dtype == want[k][s].dtype and np.array_equal(got[k][s], want[k][s]), (tag, k, s)


def _assert_empty_step(out):
    assert out["scores"].shape == (0,) and list(out["slot_index"]) == [-1, -1, -1] and list(out["slot_scores"]) == [0, 0, 0]
    assert list(out["matching_score"]) == [0, 0, 0] and out["best_slot"] == 0 and out["best_proposal"] == -1
    assert all(out["mkpts0"][s].shape == (0, 2) and out["mkpts1"][s].shape == (0, 2) and out["mconf"][s].shape == (0,) for s in range(3))


def test_batched_step_equals_single_query_step(dev, models, golden_dir):
    from pope_amd import synth
    from pope_amd.driver import locate_and_match, locate_and_match_batch
    vit, matcher = models
    a = tuple(t.to(dev) for t in synth.synthetic_driver_case(8, seed=31))
    b = tuple(t.to(dev) for t in synth.synthetic_driver_case(8, seed=32))   # (the generator plants proposals 2, 5 and 6: P >= 7)
    b = (b[0], b[1][:5], b[2], b[3][:5])                                    # seed 32 with 5 proposals
    queries = [a, b, (a[0], a[1][2:3], a[2], a[3][2:3])]
    singles = [locate_and_match(vit, matcher, *q) for q in queries]
    cat = lambda i, qs: torch.cat([q[i] for q in qs], 0)  # noqa: E731
    outs = locate_and_match_batch(vit, matcher, cat(0, queries), cat(1, queries), cat(2, queries), cat(3, queries), [8, 5, 1])
    assert len(outs) == 3
    for q, (got, want) in enumerate(zip(outs, singles)):
        _assert_same_step(got, want, f"query {q}")
    assert list(outs[2]["slot_index"]) == [0, -1, -1] and len(outs[2]["mconf"][0]) > 0 and outs[2]["mconf"][1].shape == (0,)

    # query 0 inside the batch still meets the fixture of the reference's sequential loop (test_driver_step_matches_reference_loop)
    fx, out = np.load(os.path.join(golden_dir, "driver_pair.npz")), outs[0]
    np.testing.assert_allclose(out["scores"].cpu().numpy(), fx["scores"], rtol=0, atol=2e-5)
    assert np.array_equal(out["slot_index"], fx["slot_index"])
    np.testing.assert_allclose(out["slot_scores"], fx["slot_scores"], rtol=0, atol=2e-5)
    for s in range(3):
        ref_c, got_c = fx[f"mconf_{s}"], out["mconf"][s]
        clear = np.abs(ref_c - 0.2) > 1e-3
        assert abs(len(got_c) - len(ref_c)) <= int((~clear).sum())
        if len(got_c) == len(ref_c):
            e_conf = float(np.abs(got_c - ref_c).max()) if len(ref_c) else 0.0
            e_px = float(np.abs(out["mkpts1"][s] - fx[f"mkpts1_{s}"]).max()) if len(ref_c) else 0.0
            assert e_conf <= 2e-4 and e_px <= 5e-4
            assert np.array_equal(out["mkpts0"][s], fx[f"mkpts0_{s}"])
        near = int((np.abs(ref_c - 0.9) < 1e-3).sum())
        assert abs(int(out["matching_score"][s]) - int(fx["matching_score"][s])) <= near
    if all(int((np.abs(fx[f"mconf_{s}"] - 0.9) < 1e-3).sum()) == 0 for s in range(3)):
        assert np.array_equal(out["matching_score"], fx["matching_score"])
        assert out["best_slot"] == int(fx["best_slot"]) and out["best_proposal"] == int(fx["slot_index"][fx["best_slot"]])

    # a fourth query without proposals rides along: the empty result, and its neighbour is unchanged
    outs = locate_and_match_batch(vit, matcher, cat(0, [b, a]), b[1], cat(2, [b, a]), b[3], [5, 0])
    _assert_same_step(outs[0], singles[1], "query 1 next to an empty query")
    _assert_empty_step(outs[1])


# ---- 4. locate_match_pose_batch_u8 == locate_match_pose_u8 per query ----------------------------------------------------
def test_batched_pose_chain_equals_single_query_chain(dev, peaked_models):
    from pope_amd import synth
    from pope_amd.driver import locate_match_pose_batch_u8, locate_match_pose_u8
    vit, matcher = peaked_models
    cases = [synth.synthetic_frame_case(seed=31), synth.synthetic_frame_case(n_proposals=6, seed=32)]
    singles = [locate_match_pose_u8(vit, matcher, *c) for c in cases]
    outs = locate_match_pose_batch_u8(vit, matcher, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]),
                                      [c[2] for c in cases], np.stack([c[3] for c in cases]), cases[0][4])
    assert len(outs) == 2
    for q, (got, want) in enumerate(zip(outs, singles)):
        for k in ("boxes", "K_crops", "pre_bbox", "pre_K"):
            assert np.array_equal(got[k], want[k]), (q, k)
        _assert_same_step(got, want, f"query {q}")
        assert (got["pose"] is None) == (want["pose"] is None), q
        if want["pose"] is not None:
            for name, g, w in zip(("R", "t", "inliers"), got["pose"], want["pose"]):
                assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (q, name)
    assert singles[0]["pose"] is not None and len(singles[0]["mconf"][singles[0]["best_slot"]]) >= 300   # a real pose problem
