"""Queries that share a frame on the MI355X (`frame_index` of `locate_and_match_batch_u8` and `locate_match_pose_batch_u8`,
`SharedFrames` handed to `locate_pose_from_frames`; `locate_poses_in_frame`): each query's dict is, key by key and bit for bit, that of today's call with
the frames and their box lists repeated per query, while the SAM encoder sees every frame once and DINOv2 every crop once.
Every comparison is an equality."""
import numpy as np
import pytest
import torch

from pope_amd import synth
from pope_amd.driver import SharedFrames
from test_gpu_frame_query import assert_same_result, assert_same_value, frames, generator, models, sam  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAME_INDEX = [0, 0, 1, 0]          # Q = 4 queries on F = 2 frames; frame 1 (seed 6 at gain 0.25) has no proposals
REF_INDEX = [2, 0, 3, 1]


@pytest.fixture(scope="module")
def case(sam, frames, models):  # noqa: F811
    """The shared inputs and, computed once, today's calls on the repeated frames."""
    from pope_amd.driver import locate_match_pose_batch_u8, locate_pose_from_frames
    cases = [synth.synthetic_frame_case(seed=31 + q) for q in range(len(FRAME_INDEX))]
    refs, K0, K1 = np.stack([c[0] for c in cases]), np.stack([c[3] for c in cases]), cases[0][4]
    assert len({r.tobytes() for r in refs}) == len(refs)                            # four different references
    gen = generator(sam)
    boxes3 = [b.tolist() for b in gen.propose_batch(frames)]
    assert len(boxes3[0]) >= 4 and len(boxes3[1]) == 0 and len(boxes3[2]) >= 4
    two, boxes = frames[:2], boxes3[:2]
    repeated, repeated_boxes = [two[f] for f in FRAME_INDEX], [boxes[f] for f in FRAME_INDEX]
    events = sam.image_encoder.overflow_events
    c = {"refs": refs, "K0": K0, "K1": K1, "gen": gen, "frames": two, "boxes": boxes, "boxes3": boxes3, "repeated": repeated,
         "repeated_boxes": repeated_boxes,
         "want_pose": locate_match_pose_batch_u8(*models, refs, repeated, repeated_boxes, K0, K1),
         "want_frames": locate_pose_from_frames(gen, *models, refs, repeated, K0, K1),
         "want_reindexed": locate_match_pose_batch_u8(*models, refs[REF_INDEX], repeated, repeated_boxes, K0, K1)}
    assert sam.image_encoder.overflow_events == events                               # no range-guard event: the contract's condition
    assert c["want_pose"][0]["best_proposal"] >= 0 and c["want_pose"][2]["best_proposal"] == -1
    print(f"proposals per frame {[len(b) for b in boxes]}, best proposal {[w['best_proposal'] for w in c['want_pose']]}, "
          f"pose found {[w['pose'] is not None for w in c['want_pose']]}")
    return c


def assert_same_dict(got, want, tag):
    assert set(got) == set(want), tag
    for k in want:
        assert_same_value(got[k], want[k], (tag, k))


# ---- 1. the three forms of the shared call against the repeated-frame call ------------------------------------------------
def test_shared_frames_with_image_references(models, case):  # noqa: F811
    from pope_amd.driver import locate_match_pose_batch_u8, locate_pose_from_frames
    c = case
    got = locate_match_pose_batch_u8(*models, c["refs"], c["frames"], c["boxes"], c["K0"], c["K1"], frame_index=FRAME_INDEX)
    assert len(got) == len(FRAME_INDEX)
    for q, (g, w) in enumerate(zip(got, c["want_pose"])):
        assert_same_dict(g, w, f"query {q}")
    # K1 per frame, frames as one array, the index as an array
    again = locate_match_pose_batch_u8(*models, c["refs"], np.stack(c["frames"]), c["boxes"], c["K0"], np.stack([c["K1"]] * 2),
                                       frame_index=np.asarray(FRAME_INDEX))
    for q, (g, w) in enumerate(zip(again, c["want_pose"])):
        assert_same_dict(g, w, f"query {q}, stacked")
    got = locate_pose_from_frames(c["gen"], *models, c["refs"], SharedFrames(c["frames"], FRAME_INDEX), c["K0"], c["K1"])
    assert len(got) == len(FRAME_INDEX)
    for q, f in enumerate(FRAME_INDEX):
        assert_same_result(got[q], c["want_pose"][q], c["boxes"][f], f"query {q}")
        assert_same_dict(got[q], c["want_frames"][q], f"query {q} against the repeated frames call")
    empty = got[2]
    assert empty["best_proposal"] == -1 and empty["pose"] is None and empty["proposals"].shape == (0, 4) and empty["scores"].shape == (0,)


def test_shared_frames_with_a_reference_set_and_ref_index(models, case):  # noqa: F811
    from pope_amd.driver import encode_references, locate_match_pose_batch_u8, locate_pose_from_frames
    c = case
    refset = encode_references(*models, c["refs"])
    got = locate_match_pose_batch_u8(*models, refset, c["frames"], c["boxes"], c["K0"], c["K1"], ref_index=REF_INDEX, frame_index=FRAME_INDEX)
    for q, (g, w) in enumerate(zip(got, c["want_reindexed"])):
        assert_same_dict(g, w, f"query {q}, reference set")
    got = locate_match_pose_batch_u8(*models, c["refs"], c["frames"], c["boxes"], c["K0"], c["K1"], ref_index=REF_INDEX, frame_index=FRAME_INDEX)
    for q, (g, w) in enumerate(zip(got, c["want_reindexed"])):
        assert_same_dict(g, w, f"query {q}, images with ref_index")
    got = locate_pose_from_frames(c["gen"], *models, refset.select(REF_INDEX), SharedFrames(c["frames"], FRAME_INDEX), c["K0"], c["K1"])
    for q, f in enumerate(FRAME_INDEX):
        assert_same_result(got[q], c["want_reindexed"][q], c["boxes"][f], f"query {q}, selection")
    # one reference asked of both frames, three times of the first
    one = locate_match_pose_batch_u8(*models, refset, c["frames"], c["boxes"], c["K0"][0], c["K1"], ref_index=[0] * 4, frame_index=FRAME_INDEX)
    assert_same_dict(one[0], c["want_pose"][0], "one reference, query 0")
    assert_same_dict(one[3], one[0], "one reference, the same query twice")


def test_shared_frames_as_a_cuda_tensor(models, case):  # noqa: F811
    from pope_amd.driver import locate_pose_from_frames
    c = case
    on_card = torch.from_numpy(np.stack(c["frames"])).to(DEV)
    want = locate_pose_from_frames(c["gen"], *models, c["refs"], on_card[FRAME_INDEX], c["K0"], c["K1"])
    got = locate_pose_from_frames(c["gen"], *models, c["refs"], SharedFrames(on_card, FRAME_INDEX), c["K0"], c["K1"])
    for q in range(len(FRAME_INDEX)):
        assert_same_dict(got[q], want[q], f"query {q}, frames on the device")
    assert want[0]["best_proposal"] >= 0 and len(want[0]["proposals"]) >= 4
    listed = locate_pose_from_frames(c["gen"], *models, c["refs"], SharedFrames([on_card[0], on_card[1]], torch.as_tensor(FRAME_INDEX)),
                                     c["K0"], c["K1"])
    assert_same_dict(listed[3], want[3], "query 3, a list of device frames")


def test_references_asked_of_one_frame(models, case):  # noqa: F811
    from pope_amd.driver import encode_references, locate_pose_from_frames, locate_poses_in_frame
    c = case
    rows = [0, 1, 3]
    refs, K0, frame = c["refs"][rows], c["K0"][rows], c["frames"][0]
    want = locate_pose_from_frames(c["gen"], *models, refs, [frame] * 3, K0, c["K1"])
    got = locate_poses_in_frame(c["gen"], *models, refs, frame, K0, c["K1"])
    assert isinstance(got, list) and len(got) == 3
    for q in range(3):
        assert_same_dict(got[q], want[q], f"reference {q}")
        assert_same_dict(got[q], c["want_frames"][rows[q]], f"reference {q} against the four-query call")
    by_set = locate_poses_in_frame(c["gen"], *models, encode_references(*models, c["refs"]).select(rows), torch.from_numpy(frame), K0, c["K1"])
    for q in range(3):
        assert_same_dict(by_set[q], want[q], f"reference {q} of a set")
    capped = locate_poses_in_frame(c["gen"], *models, refs, frame, K0, c["K1"], max_proposals=2)
    cut = locate_pose_from_frames(c["gen"], *models, refs, [frame] * 3, K0, c["K1"], max_proposals=2)
    for q in range(3):
        assert_same_dict(capped[q], cut[q], f"reference {q}, two proposals per frame")
        assert capped[q]["proposals"].shape == (2, 4)


# ---- 2. the work is done once per frame ----------------------------------------------------------------------------------
class _Rows:
    """Counts the batch rows a module is called with."""

    def __init__(self, module):
        self.rows, self.calls = 0, 0
        self.handle = module.register_forward_pre_hook(self)

    def __call__(self, module, args):
        self.rows += int(args[0].shape[0])
        self.calls += 1

    def take(self):
        rows, self.rows, self.calls = self.rows, 0, 0
        return rows


def test_models_see_every_frame_and_every_crop_once(sam, models, case):  # noqa: F811
    from pope_amd.driver import encode_references, locate_pose_from_frames
    c = case
    F, Q = len(c["frames"]), len(FRAME_INDEX)
    N = sum(len(b) for b in c["boxes"])
    repeated_N = sum(len(b) for b in c["repeated_boxes"])
    assert repeated_N == 3 * N > N
    enc, vit = _Rows(sam.image_encoder), _Rows(models[0])
    events = sam.image_encoder.overflow_events
    try:
        locate_pose_from_frames(c["gen"], *models, c["refs"], c["repeated"], c["K0"], c["K1"])
        assert (enc.take(), vit.take()) == (Q, repeated_N + Q)                        # today's call: every repeat pays
        locate_pose_from_frames(c["gen"], *models, c["refs"], SharedFrames(c["frames"], FRAME_INDEX), c["K0"], c["K1"])
        assert (enc.take(), vit.take()) == (F, N + Q)
        refset = encode_references(*models, c["refs"])
        assert (enc.take(), vit.take()) == (0, Q)
        locate_pose_from_frames(c["gen"], *models, refset.select(REF_INDEX), SharedFrames(c["frames"], FRAME_INDEX), c["K0"], c["K1"])
        assert (enc.take(), vit.take()) == (F, N)
    finally:
        enc.handle.remove()
        vit.handle.remove()
    assert sam.image_encoder.overflow_events == events


# ---- 3. the edges --------------------------------------------------------------------------------------------------------
def test_frame_index_none_is_todays_call(models, case):  # noqa: F811
    from pope_amd.driver import locate_match_pose_batch_u8, locate_pose_from_frames
    c = case
    got = locate_match_pose_batch_u8(*models, c["refs"], c["repeated"], c["repeated_boxes"], c["K0"], c["K1"], frame_index=None)
    for q, (g, w) in enumerate(zip(got, c["want_pose"])):
        assert_same_dict(g, w, f"query {q}")
    got = locate_pose_from_frames(c["gen"], *models, c["refs"], c["repeated"], c["K0"], c["K1"])
    for q, (g, w) in enumerate(zip(got, c["want_frames"])):
        assert_same_dict(g, w, f"query {q}")
    # the identity index is the same call as well
    got = locate_match_pose_batch_u8(*models, c["refs"], c["repeated"], c["repeated_boxes"], c["K0"], c["K1"], frame_index=list(range(4)))
    for q, (g, w) in enumerate(zip(got, c["want_pose"])):
        assert_same_dict(g, w, f"query {q}, identity index")


def test_a_frame_no_query_names_and_queries_on_empty_frames_only(frames, models, case):  # noqa: F811
    from pope_amd.driver import locate_match_pose_batch_u8
    c = case
    three, boxes3 = frames, c["boxes3"]
    refs, K0 = c["refs"][:2], c["K0"][:2]
    want = locate_match_pose_batch_u8(*models, refs, [three[2]] * 2, [boxes3[2]] * 2, K0, c["K1"])
    got = locate_match_pose_batch_u8(*models, refs, three, boxes3, K0, c["K1"], frame_index=[2, 2])     # frames 0 and 1 unnamed
    for q in range(2):
        assert_same_dict(got[q], want[q], f"query {q} on the last frame")
    assert want[0]["best_proposal"] >= 0
    want = locate_match_pose_batch_u8(*models, refs, [three[1]] * 2, [boxes3[1]] * 2, K0, c["K1"])
    got = locate_match_pose_batch_u8(*models, refs, three, boxes3, K0, c["K1"], frame_index=[1, 1])     # only the empty frame is named
    for q in range(2):
        assert_same_dict(got[q], want[q], f"query {q} on the empty frame")
        assert got[q]["best_proposal"] == -1 and got[q]["pose"] is None and got[q]["boxes"].shape == (0, 4)


def test_each_query_owns_its_arrays(models, case):  # noqa: F811
    from pope_amd.driver import locate_pose_from_frames
    c = case
    got = locate_pose_from_frames(c["gen"], *models, c["refs"], SharedFrames(c["frames"], FRAME_INDEX), c["K0"], c["K1"])
    sharing = [q for q, f in enumerate(FRAME_INDEX) if f == 0]
    for k in ("boxes", "K_crops", "proposals"):
        for i, a in enumerate(sharing):
            for b in sharing[i + 1:]:
                assert got[a][k] is not got[b][k] and not np.shares_memory(got[a][k], got[b][k]), (k, a, b)
                assert np.array_equal(got[a][k], got[b][k]), (k, a, b)
    got[0]["boxes"][:] = -1
    got[0]["proposals"][:] = -1
    assert (got[1]["boxes"] >= 0).any() and got[1]["proposals"].tolist() == c["boxes"][0]


def test_shared_frames_with_a_real_pose_problem(models):  # noqa: F811
    """The frames of tests/test_gpu_driver_batch.py, whose planted proposals yield a pose: the best proposal's intrinsics are
    gathered by its row among the SHARED crops."""
    from pope_amd.driver import locate_match_pose_batch_u8
    a, b = synth.synthetic_frame_case(seed=31), synth.synthetic_frame_case(n_proposals=6, seed=32)
    refs, K0 = np.stack([a[0], b[0], a[0], b[0]]), np.stack([a[3], b[3], a[3], b[3]])
    index = [1, 0, 1, 1]                                     # frames [b, a]: the last query asks b's reference of a's frame
    want = locate_match_pose_batch_u8(*models, refs, np.stack([a[1], b[1], a[1], a[1]]), [a[2], b[2], a[2], a[2]], K0, a[4])
    got = locate_match_pose_batch_u8(*models, refs, np.stack([b[1], a[1]]), [b[2], a[2]], K0, a[4], frame_index=index)
    for q in range(4):
        assert_same_dict(got[q], want[q], f"query {q}")
    assert want[0]["pose"] is not None and len(want[0]["mconf"][want[0]["best_slot"]]) >= 300
    assert_same_dict(got[2], got[0], "the same query twice")


def test_crop_level_call_shares_the_crops(models, case):  # noqa: F811
    from pope_amd.crops import crop_proposals
    from pope_amd.driver import locate_and_match_batch_u8
    c = case
    frame = torch.from_numpy(c["frames"][0]).to(DEV)
    crops = crop_proposals(frame, c["boxes"][0][:6], c["K1"])["crops"]
    want = locate_and_match_batch_u8(*models, c["refs"], torch.cat([crops, crops, crops]), [6, 6, 0, 6])
    got = locate_and_match_batch_u8(*models, c["refs"], crops, [6, 0], frame_index=FRAME_INDEX)
    assert len(got) == 4
    for q in range(4):
        assert_same_dict(got[q], want[q], f"query {q}")
    assert want[0]["best_proposal"] >= 0 and want[2]["best_proposal"] == -1
