"""GPU: the vote of queries that share proposal segments (`ops.vote_top3_shared`, pope_vote_top3_shared_f32 in vote.hip) against
`ops.vote_top3_batch` over the rows gathered per query.  Every comparison is an equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEGMENTS = (0, 1, 2, 3, 5, 261)                    # rows per segment; 261 = 65 rounds of the four waves + 1
QUERY_SEG = (2, 0, 2, 1, 0, 5, 3, 4, 5, 4)         # queries 0 and 2 share segment 2, 5 and 8 the last one, 1 and 4 the empty one
WIDTHS = (384, 70)                                 # 70 leaves a tail in the 64-lane stride


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(D):
    """(refs [Q, D], rows [N, D]) float32: random rows with the planted ones the tests name."""
    rng = np.random.default_rng(D)
    seg = np.concatenate([[0], np.cumsum(SEGMENTS)])
    refs = rng.normal(size=(len(QUERY_SEG), D)).astype(np.float32)
    rows = rng.normal(size=(seg[-1], D)).astype(np.float32)
    rows[seg[1]] = refs[3] + 0.1 * rows[seg[1]]                      # segment 1: its one row points at query 3's reference
    rows[seg[2]:seg[3]] = refs[0] + refs[2]                          # segment 2: two equal rows, positive for queries 0 and 2
    rows[seg[4]:seg[4] + 3] = -refs[7] * np.float32([[1.0], [0.5], [3.0]])   # segment 4: three rows equal to -ref of query 7 ...
    rows[seg[4] + 3:seg[5]] = refs[9] - 2.0 * refs[7]                # ... and two that are negative for query 7, positive for 9
    top = refs[5] + refs[8]                                    # segment 5: the best row of queries 5 and 8, twice
    rows[seg[5] + 10] = rows[seg[5] + 200] = top
    return refs, rows, seg


@pytest.fixture(scope="module", params=WIDTHS)
def voted(request, dev):
    """One width: the shared vote, and the reference — `vote_top3_batch` over each query's rows gathered into a copy."""
    from pope_amd import ops
    refs, rows, seg = _case(request.param)
    cls_ref, cls_prop = torch.from_numpy(refs).to(dev), torch.from_numpy(rows).to(dev)
    own = [SEGMENTS[s] for s in QUERY_SEG]
    gathered = torch.cat([cls_prop[seg[s]:seg[s + 1]] for s in QUERY_SEG])
    want = ops.vote_top3_batch(cls_ref, gathered, own, eps=1e-8)
    got = ops.vote_top3_shared(cls_ref, cls_prop, SEGMENTS, QUERY_SEG, eps=1e-8)
    torch.cuda.synchronize()
    return {"got": got, "want": want, "seg": seg, "own": own, "cls_ref": cls_ref, "cls_prop": cls_prop, "gathered": gathered}


def test_shared_vote_equals_the_batch_vote_on_gathered_rows(voted):
    got, want, seg, own = voted["got"], voted["want"], voted["seg"], voted["own"]
    begin = np.concatenate([[0], np.cumsum(own)])
    assert got["seg"].dtype == torch.int32 and got["seg"].cpu().tolist() == seg.tolist()
    assert got["score_begin"].dtype == torch.int32 and got["score_begin"].cpu().tolist() == begin.tolist()
    assert set(got) == set(want) | {"score_begin"}
    for k in ("scores", "slot_scores", "slot_index", "pair_live"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert got["scores"].shape == (sum(own),)
    # slot_index is local to the segment, pair_row the global row of the SHARED rows: the row the batch vote found in its copy
    index, live = got["slot_index"].cpu().numpy(), got["pair_live"].cpu().numpy().reshape(-1, 3).astype(bool)
    row = got["pair_row"].cpu().numpy().reshape(-1, 3)
    assert got["pair_row"].dtype == torch.int32 and np.array_equal(live, index >= 0)
    first = seg[list(QUERY_SEG)][:, None]
    assert np.array_equal(row, np.where(live, first + index, 0))
    assert np.array_equal(want["pair_row"].cpu().numpy().reshape(-1, 3), np.where(live, begin[:-1, None] + index, 0))
    ours = voted["cls_prop"].index_select(0, got["pair_row"].long())[got["pair_live"].bool()]
    theirs = voted["gathered"].index_select(0, want["pair_row"].long())[want["pair_live"].bool()]
    assert torch.equal(ours, theirs)
    # two queries on one segment name the same rows
    assert row[0].tolist() == row[2].tolist() == [seg[2], seg[2] + 1, 0] and live[0].tolist() == [True, True, False]


def test_every_kind_of_slot_occurs(voted):
    """Tied, dead and partly filled slots are all met, so the equality above covers each branch of the vote."""
    got, seg = voted["got"], voted["seg"]
    scores, index = got["slot_scores"].cpu().numpy(), got["slot_index"].cpu().numpy()
    live = index >= 0
    all_scores = got["scores"].cpu().numpy()
    begin = got["score_begin"].cpu().numpy()
    per_query = [all_scores[begin[q]:begin[q + 1]] for q in range(len(QUERY_SEG))]
    # tied: the duplicated rows score the same, to the bit, and both sit in a slot
    assert scores[0][0] == scores[0][1] > 0 and scores[2][0] == scores[2][1] > 0
    for q in (5, 8):
        assert per_query[q][10] == per_query[q][200] == per_query[q].max() and {10, 200} <= set(index[q].tolist())
    # dead: the empty segment, and a segment whose every row scores <= 0 for this query while its neighbour fills slots from it
    assert not live[1].any() and not live[4].any() and len(per_query[1]) == 0
    assert len(per_query[7]) == 5 and (per_query[7] <= 0).all() and not live[7].any() and (scores[7] == 0).all()
    assert live[9].sum() >= 2 and {3, 4} <= set(index[9].tolist())
    # partly filled: one row, two rows
    assert live[3].tolist() == [True, False, False] and index[3].tolist() == [0, -1, -1]
    assert live[0].sum() == 2 and index[0].tolist() == [0, 1, -1]
    # full, from more rows than slots
    assert live[5].all() and live[8].all()


def _raw(dev, cls_ref, cls_prop, seg, query_seg, score_begin, n_scores):
    """The C entry itself, for index arrays that `ops.vote_top3_shared` refuses.  `scores` is pre-filled with NaN."""
    from pope_amd import _lib
    from pope_amd._lib import check, on_device_of, ptr, stream_of
    q, d = cls_ref.shape
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    seg_d, which, begin = i32(seg), i32(query_seg), i32(score_begin)
    out = {"scores": torch.full((n_scores,), float("nan"), device=dev), "slot_scores": torch.full((q, 3), -7.0, device=dev),
           "slot_index": torch.full((q, 3), 99, dtype=torch.int64, device=dev),
           "pair_row": torch.full((3 * q,), 99, dtype=torch.int32, device=dev),
           "pair_live": torch.full((3 * q,), 9, dtype=torch.uint8, device=dev)}
    with on_device_of(cls_ref):
        check(_lib.lib().pope_vote_top3_shared_f32(ptr(cls_ref), ptr(cls_prop), ptr(seg_d), len(seg) - 1, ptr(which), ptr(begin), q,
                                                   int(cls_prop.shape[0]), d, 1e-8, ptr(out["scores"]), ptr(out["slot_scores"]),
                                                   ptr(out["slot_index"]), ptr(out["pair_row"]), ptr(out["pair_live"]), stream_of(dev)),
              "pope_vote_top3_shared_f32")
    torch.cuda.synchronize()
    return out


def test_out_of_range_segment_and_short_score_range(dev, voted):
    """A `query_seg` outside [0, S) is an empty segment: three dead slots, nothing else touched.  A score range shorter than the
    segment votes over as many rows as it holds."""
    from pope_amd import ops
    seg, cls_prop = voted["seg"], voted["cls_prop"]
    S = len(SEGMENTS)
    # the references of queries 5, 9, 0 and 9 again on: the last segment, segment S, segment -1, segment 4 cut to two rows
    cls_ref = voted["cls_ref"][[5, 9, 0, 9]].contiguous()
    begin = [0, 261, 261, 261, 263]
    out = _raw(dev, cls_ref, cls_prop, seg.tolist(), [5, S, -1, 4], begin, 263 + 4)
    want = ops.vote_top3_batch(cls_ref, torch.cat([cls_prop[seg[5]:seg[6]], cls_prop[seg[4]:seg[4] + 2]]), [261, 0, 0, 2], eps=1e-8)
    assert torch.equal(out["scores"][:263], want["scores"]) and torch.isnan(out["scores"][263:]).all()
    for k in ("slot_scores", "slot_index", "pair_live"):
        assert torch.equal(out[k], want[k]), k
    live = out["pair_live"].cpu().numpy().reshape(-1, 3)
    index, row = out["slot_index"].cpu().numpy(), out["pair_row"].cpu().numpy().reshape(-1, 3)
    assert live[0].all() and not live[1].any() and not live[2].any()
    assert (index[1:3] == -1).all() and (row[1:3] == 0).all() and (out["slot_scores"][1:3] == 0).all()
    assert np.array_equal(row, np.where(live != 0, np.array([seg[5], 0, 0, seg[4]])[:, None] + index, 0))
    assert index[3].max() <= 1                                  # rows 3 and 4 of segment 4, which query 9 prefers, were not seen
    assert {3, 4} <= set(voted["got"]["slot_index"][9].tolist())


def test_identity_mapping_is_the_batch_vote(dev, voted):
    """`vote_top3_batch` is the shared vote with query q on segment q and its scores at the segment's rows."""
    from pope_amd import ops
    seg, cls_prop = voted["seg"], voted["cls_prop"]
    cls_ref = voted["cls_ref"][:len(SEGMENTS)].contiguous()
    want = ops.vote_top3_batch(cls_ref, cls_prop, SEGMENTS, eps=1e-8)
    got = ops.vote_top3_shared(cls_ref, cls_prop, SEGMENTS, list(range(len(SEGMENTS))), eps=1e-8)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["score_begin"], got["seg"])


def test_no_queries_and_no_rows(dev):
    from pope_amd import ops
    none = ops.vote_top3_shared(torch.zeros(0, 16, device=dev), torch.ones(4, 16, device=dev), [4], [], eps=1e-8)
    assert none["scores"].shape == (0,) and none["slot_index"].shape == (0, 3) and none["pair_row"].shape == (0,)
    bare = ops.vote_top3_shared(torch.ones(2, 16, device=dev), torch.zeros(0, 16, device=dev), [0, 0], [1, 0], eps=1e-8)
    assert bare["scores"].shape == (0,) and (bare["slot_index"] == -1).all() and (bare["pair_live"] == 0).all()
    assert (bare["pair_row"] == 0).all() and (bare["slot_scores"] == 0).all()
