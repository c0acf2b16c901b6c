"""Per-pair driver step of the reference evaluation loops (eval_linemod_json.py:65-127 and the
identical bodies of eval_onepose_json.py / eval_ycb_json.py), restructured for one
big GPU: what the reference does as P batch-1 DINOv2 forwards, P host round trips for the cosine score
and three batch-1 LoFTR calls becomes one batched extraction, one cosine kernel, one host-side slot
vote (order-dependent by definition) and ONE Matcher call over the occupied slots.

`locate_and_match` takes already-preprocessed tensors; `locate_and_match_u8` starts from the uint8 crops;
`locate_match_pose_u8` is the whole per-pair body of the loop after SAM: frame + proposal boxes in, pose out — proposal
crops and their intrinsics (crops.py), preprocessing (preprocess.py), DINOv2 vote, LoFTR matches and the essential-matrix
RANSAC (pose.py) all on the card.  `locate_pose_from_frames` / `locate_pose_from_frame` start one step earlier, at the raw
frame: the SAM mask generator's proposals (sam_generator.py:propose_batch, boxes only) feed the batched step.

The `*_batch` functions take Q independent queries per call: one DINOv2 forward, the vote on the device (ops.vote_top3_batch),
ONE Matcher call over 3 Q pairs, the per-slot tally and best-slot choice on the device (ops.slot_tally), one pose launch and a
single download; each query's result is what the single-query function returns for it alone.

Prompt once, query many frames: `encode_references` runs everything that depends on the reference images alone (their DINOv2
CLS tokens, their gray images, the Matcher's `ReferenceEncoding`) and the `*_batch_u8` / `locate_pose_from_frame(s)` functions
take the resulting `ReferenceSet` where they take `refs_bgr`, with `ref_index` (or `ReferenceSet.select`) naming each query's
reference ("Reference encodings").

Queries that share a frame: `frame_index` on the `*_batch_u8` calls (`SharedFrames(frames, frame_index)` in place of the frames
of `locate_pose_from_frames`) names each query's frame, the frames are given once, and everything
that depends on the frame alone (the generator's proposals, the crops and their intrinsics, their DINOv2 forward) runs once per
frame; the vote reads the shared CLS rows in place (ops.vote_top3_shared).  `locate_poses_in_frame` asks R references of one
frame, `share_frames` groups a list of queries by frame ("Shared frames").

The learned pose heads run in the same call: `pose_regressor=` takes the key-point head, the image head or MoCoPE; the image
pair of the latter two is made on the device from the reference image and the best slot's crop (`preprocess.pose_images`), and
`regress_pose_from_frames` is the call from the raw frames ("The pose heads inside the query").
"""
import numpy as np
import torch

from .dinov2_utils import get_cls_token_torch
from .ops import cls_cosine, streaming_top3
from .preprocess import frames_on_device, on_device


@torch.no_grad()
def locate_and_match(dinov2_model, matcher, ref_tensor, crop_tensors, gray_ref, gray_crops, conf_thr=0.9):
    """One query/reference pair.

    ref_tensor   [1,3,h,w]  set_torch_image(image0, center_crop=True)          (eval_linemod_json.py:64)
    crop_tensors [P,3,h,w]  set_torch_image(image_crop_p, center_crop=True)     (:89)
    gray_ref     [1,1,H0,W0] image0 as gray / 255                               (:103-105)
    gray_crops   [P,1,H1,W1] proposal crops as gray / 255 (256x256 in the drivers, :86-88,109-111)

    Returns a dict: `scores` [P] cosine of CLS tokens (:93); `slot_scores` [3] / `slot_index` [3] — the
    reference's `similarity_score` / `top_images` after its streaming loop (:94-101; index -1 = slot never
    filled); per slot `mkpts0`, `mkpts1`, `mconf` (numpy, :118-125); `matching_score` [3] = #(mconf >
    conf_thr) (:121-122); `best_slot` = first argmax (:150) and `best_proposal`.
    A slot that was never filled (fewer than three proposals with a positive score) is skipped with
    matching_score 0; the reference raises on it (:109 indexes an empty list)."""
    if ref_tensor.shape[1:] == crop_tensors.shape[1:]:
        # one launch sequence for the reference image and the P proposals (the kernels are batch-invariant bit for bit,
        # tests/test_gpu_vit.py: the tokens are those of the two separate forwards)
        both = get_cls_token_torch(dinov2_model, torch.cat([ref_tensor, crop_tensors], 0))
        ref, fea = both[:1], both[1:]
    else:
        ref = get_cls_token_torch(dinov2_model, ref_tensor)
        fea = get_cls_token_torch(dinov2_model, crop_tensors)
    scores = cls_cosine(ref, fea, eps=1e-8)
    slot_scores, slot_index = streaming_top3(scores.cpu().numpy())
    filled = [s for s in range(3) if slot_index[s] >= 0]
    out = {"scores": scores, "slot_scores": slot_scores, "slot_index": slot_index,
           "mkpts0": [np.zeros((0, 2), np.float32)] * 3, "mkpts1": [np.zeros((0, 2), np.float32)] * 3,
           "mconf": [np.zeros((0,), np.float32)] * 3, "matching_score": np.zeros(3, np.int64)}
    if filled:
        sel = torch.as_tensor([int(slot_index[s]) for s in filled], device=gray_crops.device)
        batch = {"image0": gray_ref.expand(len(filled), -1, -1, -1).contiguous(),
                 "image1": gray_crops.index_select(0, sel)}
        matcher(batch)
        b = batch["m_bids"].cpu().numpy()
        mk0, mk1, mc = (batch[k].cpu().numpy() for k in ("mkpts0_f", "mkpts1_f", "mconf"))
        for k, s in enumerate(filled):
            rows = b == k
            out["mkpts0"][s], out["mkpts1"][s], out["mconf"][s] = mk0[rows], mk1[rows], mc[rows]
            out["matching_score"][s] = int((mc[rows] > conf_thr).sum())
    out["best_slot"] = int(np.argmax(out["matching_score"]))
    out["best_proposal"] = int(slot_index[out["best_slot"]])
    return out


@torch.no_grad()
def locate_and_match_u8(dinov2_model, matcher, ref_bgr, crops_bgr, conf_thr=0.9):
    """The same step from raw uint8 frames, preprocessing included: `ref_bgr` [H0, W0, 3] and
    `crops_bgr` [P, 256, 256, 3] uint8 BGR (numpy or tensors), as the drivers hold them after cropping
    (eval_linemod_json.py:62-64,83-90,103-111).  One upload of the uint8 frames; resize / centre crop / normalisation of
    all P + 1 DINOv2 inputs and the gray / 255 conversion of all matcher inputs run as batched HIP kernels that are
    bit-identical to the reference's per-image PIL + torchvision + cv2 host calls (pope_amd/preprocess.py)."""
    from .preprocess import gray_batch, set_torch_images
    dev = next(dinov2_model.parameters()).device
    ref = torch.as_tensor(ref_bgr)[None].to(dev)
    crops = torch.as_tensor(crops_bgr).to(dev)
    return locate_and_match(dinov2_model, matcher, set_torch_images(ref, center_crop=True), set_torch_images(crops, center_crop=True),
                            gray_batch(ref), gray_batch(crops), conf_thr)


@torch.no_grad()
def locate_match_pose_u8(dinov2_model, matcher, ref_bgr, frame_bgr, bboxes_xywh, K0, K1, conf_thr=0.9, ransac_thr=0.5, ransac_conf=0.99,
                         out_size=256):
    """eval_linemod_json.py:62-127,150-160 for one query: `ref_bgr` [H0, W0, 3] uint8 (the reference crop, `image0`),
    `frame_bgr` [H, W, 3] uint8 (`image1`), `bboxes_xywh` [P, 4] SAM proposal boxes, `K0` / `K1` the two cameras.

    proposals -> expanded boxes, 256 x 256 crops and their K (crops.crop_proposals, one launch) -> `locate_and_match_u8`
    (DINOv2 vote + ONE LoFTR call over the occupied slots) -> `estimate_pose(mkpts0, mkpts1, K0, K_crop[best], 0.5, 0.99)`
    on the best slot's matches (ALL of them: the 0.9 confidence only ranks the slots, :118-119,150-160).
    Adds to `locate_and_match`'s dict: `boxes` [P, 4], `K_crops` [P, 3, 3], `pre_bbox`, `pre_K` (the chosen proposal's) and
    `pose` = (R, t, inliers) or None."""
    from .crops import crop_proposals
    from .pose import estimate_pose
    dev = next(dinov2_model.parameters()).device
    frame = torch.as_tensor(frame_bgr).to(dev)
    prop = crop_proposals(frame, bboxes_xywh, K1, out_size=out_size)
    out = locate_and_match_u8(dinov2_model, matcher, ref_bgr, prop["crops"], conf_thr)
    out["boxes"], out["K_crops"] = prop["boxes"], prop["K"]
    best = out["best_proposal"]
    if best < 0:       # no proposal entered a slot (the reference raises at :109)
        out["pre_bbox"], out["pre_K"], out["pose"] = None, None, None
        return out
    out["pre_bbox"], out["pre_K"] = prop["boxes"][best], prop["K"][best]
    s = out["best_slot"]
    out["pose"] = estimate_pose(out["mkpts0"][s], out["mkpts1"][s], K0, out["pre_K"], ransac_thr, ransac_conf, device=dev)
    return out


# ---- Q queries per call: the same step with the vote, the slot tally and the best-slot choice on the device ------------------
def _counts(proposals_per_query, Q, N, what):
    """The Q per-query proposal counts as ints; ValueError unless there are Q of them, none negative, summing to N."""
    counts = [int(p) for p in proposals_per_query]
    if len(counts) != Q:
        raise ValueError(f"{what}: {len(counts)} proposal counts for {Q} queries")
    if any(c < 0 for c in counts) or sum(counts) != N:
        raise ValueError(f"{what}: proposals_per_query must be non-negative and sum to the {N} proposal rows (got {sum(counts)})")
    return counts


class ReferenceSet:
    """R reference images as the batched step needs them (`encode_references`): `cls` [R, 384] DINOv2 CLS tokens, `gray`
    [R, 1, H0, W0] gray / 255, `encoding` the matcher's `ReferenceEncoding` of `gray`.  Built for one (dinov2_model, matcher)
    pair; the encoding follows later weight changes of the matcher by itself, the CLS tokens are those of the ViT as it was.

    Encoded with an image-conditioned pose head (`encode_references(..., pose_regressor=)`), it also keeps the reference side of
    that head: `pose_img0` [R, 3, s, s] (`preprocess.pose_images` of the references) and, for a MoCoPE whose `train_type` reads
    images, `pose_feat0` [R, 1000], the backbone's logits of those images.  `pose_for` = (the regressor, s, its backbone key when
    logits are kept) names what they were made for; `_pose_side` refuses any other use."""

    def __init__(self, cls, gray, encoding, index=None, pose_img0=None, pose_feat0=None, pose_for=None):
        self.cls, self.gray, self.encoding, self.index = cls, gray, encoding, index
        self.pose_img0, self.pose_feat0, self.pose_for = pose_img0, pose_feat0, pose_for

    @property
    def R(self):
        return int(self.gray.shape[0])

    def select(self, ref_index):
        """The same references (nothing is copied) standing for len(ref_index) queries, query q using row ref_index[q]: what
        the `ref_index` keyword says, for the calls that have no such keyword (`locate_pose_from_frames`, `locate_pose_from_frame`)."""
        return ReferenceSet(self.cls, self.gray, self.encoding, _ref_index(ref_index, self.R, None, "ReferenceSet.select"),
                            self.pose_img0, self.pose_feat0, self.pose_for)

    def __len__(self):
        """The number of queries this stands for: its rows, or the length of its selection."""
        return self.R if self.index is None else len(self.index)


def _regressor_kind(pose_regressor, what):
    """None, "mkpts" (`pose_regressor.Mkpts_Reg_Model`), "mocope" (`mocope.MoCoPE`) or "cnn" (`pose_regressor_cnn.Mkpts_Reg_Model`);
    TypeError for any other object.  Touches no device."""
    if pose_regressor is None:
        return None
    from . import mocope, pose_regressor as kpts, pose_regressor_cnn as cnn
    for kind, cls in (("mkpts", kpts.Mkpts_Reg_Model), ("mocope", mocope.MoCoPE), ("cnn", cnn.Mkpts_Reg_Model)):
        if isinstance(pose_regressor, cls):
            return kind
    raise TypeError(f"{what}: pose_regressor must be a pope_amd pose_regressor.Mkpts_Reg_Model, mocope.MoCoPE or "
                    f"pose_regressor_cnn.Mkpts_Reg_Model, got {type(pose_regressor).__name__}")


def _image_size(pose_image_size, what):
    size = int(pose_image_size)
    if size <= 0:
        raise ValueError(f"{what}: pose_image_size must be positive, got {pose_image_size}")
    return size


def _reads_images(kind, pose_regressor):
    return kind == "cnn" or (kind == "mocope" and pose_regressor.train_type != "mkpts")


@torch.no_grad()
def encode_references(dinov2_model, matcher, refs_bgr, pose_regressor=None, pose_image_size=224):
    """`refs_bgr` [R, H0, W0, 3] uint8 BGR (numpy or tensor; H0, W0 multiples of 8, >= 16) -> `ReferenceSet`: the reference side of
    `locate_and_match_batch_u8`, computed once.  Pass it in place of `refs_bgr`, with `ref_index` naming each query's row.

    With an image-conditioned `pose_regressor` (`mocope.MoCoPE`, `pose_regressor_cnn.Mkpts_Reg_Model`) the set also keeps the
    head's reference images at `pose_image_size` and, for a MoCoPE that reads images, their backbone logits, so a query with
    that regressor and size runs the MoCoPE backbone over its crops only.  The key-point-only head has no reference side."""
    from .preprocess import gray_batch, pose_images, set_torch_images
    kind = _regressor_kind(pose_regressor, "encode_references")
    size = _image_size(pose_image_size, "encode_references")
    dev = next(dinov2_model.parameters()).device
    refs = torch.as_tensor(refs_bgr).to(dev)
    if refs.dim() != 4 or int(refs.shape[0]) == 0:
        raise ValueError("encode_references: refs_bgr is [R >= 1, H0, W0, 3]")
    cls = get_cls_token_torch(dinov2_model, set_torch_images(refs, center_crop=True))
    gray = gray_batch(refs)
    img0 = feat0 = pose_for = None
    if kind in ("mocope", "cnn"):
        img0 = pose_images(refs, None, size)
        feat0 = pose_regressor.image_logits(img0) if kind == "mocope" and _reads_images(kind, pose_regressor) else None
        pose_for = (pose_regressor, size, pose_regressor.backbone_key() if feat0 is not None else None)
    return ReferenceSet(cls, gray, matcher.encode_reference(gray), None, img0, feat0, pose_for)


def _pose_side(refset, rows, pose_regressor, size, what):
    """(img0, feat0) [Q, ...] of a `ReferenceSet` for an image-conditioned regressor, gathered by `rows` on the device; feat0 is
    None where the set keeps no logits.  ValueError unless the set was encoded for this regressor object and size, and (with
    logits) the backbone's tensors are still those the logits were computed with."""
    made = refset.pose_for
    if made is None or made[0] is not pose_regressor or made[1] != size:
        raise ValueError(f"{what}: this ReferenceSet was not encoded for this pose_regressor at pose_image_size {size}: encode it with "
                         "encode_references(..., pose_regressor=, pose_image_size=)")
    if made[2] is not None and made[2] != pose_regressor.backbone_key():
        raise ValueError(f"{what}: the regressor's backbone changed after this ReferenceSet was encoded: encode it again")
    sel = torch.as_tensor(rows, dtype=torch.int64, device=refset.pose_img0.device)
    return refset.pose_img0.index_select(0, sel), None if refset.pose_feat0 is None else refset.pose_feat0.index_select(0, sel)


def _ref_index(ref_index, R, Q, what):
    """The Q reference rows of the queries as ints: None is arange(Q) and needs R == Q; ValueError on a wrong count or a row
    outside [0, R)."""
    if ref_index is None:
        if Q is not None and R != Q:
            raise ValueError(f"{what}: {R} references for {Q} queries needs ref_index (one reference row per query)")
        return list(range(R))
    rows = np.asarray(ref_index.cpu() if torch.is_tensor(ref_index) else ref_index)
    if rows.ndim != 1 or (rows.size and not np.issubdtype(rows.dtype, np.integer)):
        raise ValueError(f"{what}: ref_index is a list of integers, one per query")
    if Q is not None and rows.size != Q:
        raise ValueError(f"{what}: {rows.size} ref_index entries for {Q} queries")
    if rows.size and (rows.min() < 0 or rows.max() >= R):
        raise ValueError(f"{what}: ref_index values must lie in [0, {R}), got [{int(rows.min())}, {int(rows.max())}]")
    return [int(r) for r in rows]


def _select_refs(refs, ref_index, Q, what):
    """(references, rows): a `ReferenceSet` keeps its rows and is indexed on the device; images are selected here, so the
    rest of the call sees one reference per query."""
    if isinstance(refs, ReferenceSet):
        if refs.index is not None:
            if ref_index is not None:
                raise ValueError(f"{what}: this ReferenceSet already carries a selection (ReferenceSet.select); give one of the two")
            return refs, list(refs.index)
        return refs, _ref_index(ref_index, refs.R, Q, what)
    refs = torch.as_tensor(refs)
    if ref_index is None:
        return refs, None
    rows = _ref_index(ref_index, int(refs.shape[0]), Q, what)
    return refs.index_select(0, torch.as_tensor(rows, dtype=torch.int64, device=refs.device)), None


def _frame_index(frame_index, F, Q, what):
    """The frames of the Q queries as ints; ValueError on a wrong count, a non-integer value or a frame outside [0, F)."""
    rows = np.asarray(frame_index.cpu() if torch.is_tensor(frame_index) else frame_index)
    if rows.ndim != 1 or (rows.size and not np.issubdtype(rows.dtype, np.integer)):
        raise ValueError(f"{what}: frame_index is a list of integers, one per query")
    if rows.size != Q:
        raise ValueError(f"{what}: {rows.size} frame_index entries for {Q} queries")
    if rows.size and (rows.min() < 0 or rows.max() >= F):
        raise ValueError(f"{what}: frame_index values must lie in [0, {F}), got [{int(rows.min())}, {int(rows.max())}]")
    return [int(r) for r in rows]


class SharedFrames:
    """F frames standing for len(frame_index) queries, query q asked of frame frame_index[q]: what the `frame_index` keyword of
    the `*_batch_u8` calls says, for `locate_pose_from_frames`, whose signature is that of the reference's loop body and has no
    such keyword.  `frames` is whatever that call takes as `frames_bgr`; nothing is copied, the index is checked by the call."""

    def __init__(self, frames, frame_index):
        self.frames, self.index = frames, frame_index

    def __len__(self):
        """The number of queries this stands for."""
        return len(self.index)


def share_frames(keys):
    """Groups queries by frame for the `frame_index` calls: `keys` holds one hashable key per query (what names its frame, such
    as (object, frame number)).  Returns `(positions, frame_index)`: `positions[f]` is the first query with the f-th distinct
    key, in order of first appearance, and `keys[positions[frame_index[q]]] == keys[q]`.  A walker loads the frames of
    `positions` and hands `frame_index` to the call."""
    first, positions, frame_index = {}, [], []
    for q, key in enumerate(keys):
        if key not in first:
            first[key] = len(positions)
            positions.append(q)
        frame_index.append(first[key])
    return positions, frame_index


def _vote(cls_ref, fea, counts, frame_rows):
    """The vote of the batched step: query q over segment q, or with `frame_rows` over segment frame_rows[q] of shared segments."""
    from .ops import vote_top3_batch, vote_top3_shared
    if frame_rows is None:
        return vote_top3_batch(cls_ref, fea, counts, eps=1e-8)
    return vote_top3_shared(cls_ref, fea, counts, frame_rows, eps=1e-8)


def _batch_refset_on_device(dinov2_model, matcher, refset, rows, crop_tensors, select_gray, counts, conf_thr, frame_rows=None):
    """`_batch_on_device` with the reference side taken from a `ReferenceSet`: the ViT runs over the proposals only, the vote
    reads the kept CLS tokens of rows `rows`, the Matcher gets the kept encoding and pair 3 q + s -> reference rows[q]."""
    from .ops import slot_tally
    Q = len(rows)
    fea = get_cls_token_torch(dinov2_model, crop_tensors)
    rows_h = torch.as_tensor(rows, dtype=torch.int64)
    dv = _vote(refset.cls.index_select(0, rows_h.to(fea.device)), fea, counts, frame_rows)
    live = dv["pair_live"].bool()[:, None, None, None]
    sel = select_gray(dv["pair_row"])
    batch = {"reference": refset.encoding, "image0_index": rows_h.repeat_interleave(3),
             "image1": torch.where(live, sel, torch.zeros_like(sel[:1, :1, :1, :1]))}
    matcher(batch)
    dv.update(slot_tally(batch["m_bids"], batch["mconf"], batch["mkpts0_f"], batch["mkpts1_f"], dv["pair_live"], conf_thr))
    dv.update(mkpts0=batch["mkpts0_f"], mkpts1=batch["mkpts1_f"], mconf=batch["mconf"])
    dv["best_row"] = dv["pair_row"].view(Q, 3).gather(1, dv["best_slot"].long()[:, None])[:, 0]
    return dv


def _batch_on_device(dinov2_model, matcher, ref_tensors, crop_tensors, gray_refs, select_gray, counts, conf_thr, frame_rows=None):
    """Launch sequence of the batched step, nothing read back: one DINOv2 forward over the Q references and the N proposals
    -> `vote_top3_batch` -> ONE Matcher call over 3 Q pairs (pair 3 q + s: reference q against the crop in slot s of query q;
    a dead slot keeps its place with an all-zero image1, so the batch is sized without a host read) -> `slot_tally`.
    `select_gray(pair_row)` -> [3 Q, 1, H1, W1] gray crops of the voted rows.  Returns the device tensors of both ops.
    With `frame_rows` (Q segment numbers) the N proposals are those of F shared frames, `counts` their F counts, and query q votes
    over segment frame_rows[q] (`vote_top3_shared`): a frame's crops pass through the ViT once however many queries name it."""
    from .ops import slot_tally
    Q = int(ref_tensors.shape[0])
    if ref_tensors.shape[1:] == crop_tensors.shape[1:]:
        both = get_cls_token_torch(dinov2_model, torch.cat([ref_tensors, crop_tensors], 0))
        ref, fea = both[:Q], both[Q:]
    else:
        ref = get_cls_token_torch(dinov2_model, ref_tensors)
        fea = get_cls_token_torch(dinov2_model, crop_tensors)
    dv = _vote(ref, fea, counts, frame_rows)
    live = dv["pair_live"].bool()[:, None, None, None]
    sel = select_gray(dv["pair_row"])
    batch = {"image0": gray_refs.repeat_interleave(3, dim=0), "image1": torch.where(live, sel, torch.zeros_like(sel[:1, :1, :1, :1]))}
    matcher(batch)
    dv.update(slot_tally(batch["m_bids"], batch["mconf"], batch["mkpts0_f"], batch["mkpts1_f"], dv["pair_live"], conf_thr))
    dv.update(mkpts0=batch["mkpts0_f"], mkpts1=batch["mkpts1_f"], mconf=batch["mconf"])
    # the best proposal's global row (a dead best slot points at row 0: any valid row, its result is dropped on the host)
    dv["best_row"] = dv["pair_row"].view(Q, 3).gather(1, dv["best_slot"].long()[:, None])[:, 0]
    return dv


def _empty_result(device):
    return {"scores": torch.empty(0, dtype=torch.float32, device=device), "slot_scores": np.zeros(3, np.float32),
            "slot_index": np.full(3, -1, np.int64), "mkpts0": [np.zeros((0, 2), np.float32)] * 3,
            "mkpts1": [np.zeros((0, 2), np.float32)] * 3, "mconf": [np.zeros((0,), np.float32)] * 3,
            "matching_score": np.zeros(3, np.int64), "best_slot": 0, "best_proposal": -1}


def _download(dv, counts):
    """The one download of the batched step: Q dicts with the keys and types of `locate_and_match`.  `counts` are the Q
    per-query proposal counts: with shared frames too, query q's scores lie at the exclusive scan of its own counts."""
    Q = len(counts)
    keys = ("slot_scores", "slot_index", "pair_live", "pair_begin", "pair_count", "matching_score", "best_slot", "mkpts0", "mkpts1", "mconf")
    h = {k: dv[k].cpu().numpy() for k in keys}
    seg = np.concatenate([[0], np.cumsum(counts)])
    outs = []
    for q in range(Q):
        out = _empty_result(dv["scores"].device)
        out["scores"] = dv["scores"][seg[q]:seg[q + 1]]
        out["slot_scores"], out["slot_index"] = h["slot_scores"][q].copy(), h["slot_index"][q].copy()
        out["matching_score"] = h["matching_score"][q].copy()
        out["mkpts0"], out["mkpts1"], out["mconf"] = list(out["mkpts0"]), list(out["mkpts1"]), list(out["mconf"])
        for s in range(3):
            b = 3 * q + s
            if h["pair_live"][b]:
                rows = slice(int(h["pair_begin"][b]), int(h["pair_begin"][b]) + int(h["pair_count"][b]))
                out["mkpts0"][s], out["mkpts1"][s], out["mconf"][s] = h["mkpts0"][rows], h["mkpts1"][rows], h["mconf"][rows]
        out["best_slot"] = int(h["best_slot"][q])
        out["best_proposal"] = int(out["slot_index"][out["best_slot"]])
        outs.append(out)
    return outs


@torch.no_grad()
def locate_and_match_batch(dinov2_model, matcher, ref_tensors, crop_tensors, gray_refs, gray_crops, proposals_per_query, conf_thr=0.9):
    """`locate_and_match` for Q independent queries in one call.

    ref_tensors [Q,3,h,w], gray_refs [Q,1,H0,W0]: one reference per query; crop_tensors [N,3,h,w], gray_crops [N,1,H1,W1]: the
    proposals of all queries, query q owning the next `proposals_per_query[q]` rows (0 is allowed: the empty result, every
    slot -1, best_proposal -1).  Returns a list of Q dicts, each what `locate_and_match` returns for that query alone.
    Nothing is read back between the DINOv2 forward and the Matcher launch, nor between the Matcher and the final download:
    the vote and the slot tally run on the device (ops.vote_top3_batch, ops.slot_tally)."""
    Q, N = int(ref_tensors.shape[0]), int(crop_tensors.shape[0])
    counts = _counts(proposals_per_query, Q, N, "locate_and_match_batch")
    if int(gray_refs.shape[0]) != Q or int(gray_crops.shape[0]) != N:
        raise ValueError(f"locate_and_match_batch: {Q} references / {N} proposals, but {int(gray_refs.shape[0])} / "
                         f"{int(gray_crops.shape[0])} gray images")
    if Q == 0 or N == 0:
        return [_empty_result(ref_tensors.device) for _ in range(Q)]
    dv = _batch_on_device(dinov2_model, matcher, ref_tensors, crop_tensors, gray_refs,
                          lambda rows: gray_crops.index_select(0, rows), counts, conf_thr)
    return _download(dv, counts)


def _batch_u8_on_device(dinov2_model, matcher, refs, crops, counts, conf_thr, rows=None, frame_rows=None):
    from .preprocess import gray_batch, set_torch_images
    if isinstance(refs, ReferenceSet):
        return _batch_refset_on_device(dinov2_model, matcher, refs, rows, set_torch_images(crops, center_crop=True),
                                       lambda r: gray_batch(crops.index_select(0, r)), counts, conf_thr, frame_rows)
    # gray conversion of the 3 Q voted crops only (a per-pixel op: bit-equal to converting all N and selecting)
    return _batch_on_device(dinov2_model, matcher, set_torch_images(refs, center_crop=True), set_torch_images(crops, center_crop=True),
                            gray_batch(refs), lambda rows: gray_batch(crops.index_select(0, rows)), counts, conf_thr, frame_rows)


@torch.no_grad()
def locate_and_match_batch_u8(dinov2_model, matcher, refs_bgr, crops_bgr, proposals_per_query, conf_thr=0.9, ref_index=None,
                              frame_index=None):
    """`locate_and_match_u8` for Q queries: `refs_bgr` [Q, H0, W0, 3] and `crops_bgr` [N, 256, 256, 3] uint8 BGR (numpy or
    tensors), query q owning the next `proposals_per_query[q]` crops.  Preprocessing as there, except that only the 3 Q crops
    the vote selected are converted to gray.

    `refs_bgr` may be a `ReferenceSet` (`encode_references`); `ref_index` (Q integers, default arange(Q), which needs R == Q) names
    the reference row of each query, for a set and for images alike.  Each query's result is, bit for bit, that of the call with
    the images `refs_bgr[ref_index]`.

    `frame_index` (Q integers) lets queries share the crops of a frame: `crops_bgr` then holds the crops of F frames once each,
    `proposals_per_query` their F counts (frame f owning the next count rows), and query q votes over the crops of frame
    `frame_index[q]`.  The crops pass through the ViT once, not once per query that names them; a frame no query names is allowed.
    Each query's result is, bit for bit, that of the call with every frame's crops repeated per query."""
    crops = torch.as_tensor(crops_bgr)
    refs, rows = _select_refs(refs_bgr, ref_index, None, "locate_and_match_batch_u8")
    Q, N = len(rows) if rows is not None else int(refs.shape[0]), int(crops.shape[0])
    fidx = None
    if frame_index is None:
        counts = own = _counts(proposals_per_query, Q, N, "locate_and_match_batch_u8")
    else:
        counts = [int(p) for p in proposals_per_query]
        counts = _counts(counts, len(counts), N, "locate_and_match_batch_u8")
        fidx = _frame_index(frame_index, len(counts), Q, "locate_and_match_batch_u8")
        own = [counts[f] for f in fidx]
    dev = next(dinov2_model.parameters()).device
    if Q == 0 or sum(own) == 0:
        return [_empty_result(dev) for _ in range(Q)]
    if rows is None:
        refs = refs.to(dev)
    return _download(_batch_u8_on_device(dinov2_model, matcher, refs, crops.to(dev), counts, conf_thr, rows, fidx), own)


@torch.no_grad()
def locate_match_pose_batch_u8(dinov2_model, matcher, refs_bgr, frames_bgr, bboxes_xywh, K0, K1, conf_thr=0.9, ransac_thr=0.5,
                               ransac_conf=0.99, out_size=256, ref_index=None, frame_index=None, pose_regressor=None,
                               regressor_seed=0, pose_image_size=224):
    """`locate_match_pose_u8` for Q queries in one call: `refs_bgr` [Q, H0, W0, 3] uint8, `frames_bgr` [Q, H, W, 3] uint8 (an
    array, a tensor or Q frames of one size), `bboxes_xywh` a list of Q arrays [P_q, 4] (P_q = 0 allowed), `K0` / `K1` [3, 3]
    for all queries or [Q, 3, 3].  Returns a list of Q dicts, each what `locate_match_pose_u8` returns for that query alone.

    crop_proposals per frame (asynchronous launches) -> the batched vote + ONE Matcher call over 3 Q pairs + slot tally
    (`locate_and_match_batch_u8`) -> ONE `estimate_pose_batch` over the Q best slots, fed by the tally's compacted matches
    and the crop intrinsics gathered on the device by best proposal row -> one download.  `pose` is None under
    `estimate_pose`'s conditions (fewer than five matches, no inliers) and when no slot was filled.
    `refs_bgr` may be a `ReferenceSet`, and `ref_index` names each query's reference row, as in `locate_and_match_batch_u8`.

    `frame_index` (Q integers in [0, F)) lets queries share frames: `frames_bgr` is then [F, H, W, 3], `bboxes_xywh` F arrays and
    `K1` [3, 3] or [F, 3, 3], all per FRAME, while `refs_bgr` / `ref_index` and `K0` ([3, 3] or [Q, 3, 3]) stay per query; query
    q is asked of frame `frame_index[q]`.  The crops, their intrinsics, their preprocessing and their DINOv2 forward are done
    once per frame; the vote (ops.vote_top3_shared), the 3 Q Matcher pairs, the tally and the pose stay per query.  A frame no
    query names is allowed (its crops are computed and unused).  Each query's dict is, key by key and bit for bit, that of
    the call with `frames_bgr[frame_index]` and the box lists repeated, and its `boxes` / `K_crops` are arrays of its own.

    `pose_regressor` (a `pose_regressor.Mkpts_Reg_Model` on the models' device; default None: nothing changes) sends the same
    best-slot matches through `regress_pose_batch` in this call, every query on its own, the device sampler seeded with
    `regressor_seed`: each dict gains `pose_regressed` = (R [3, 3], t [3]) fp32, or None where the best slot has fewer than five
    matches (the pairs `points_io.save_pair_points` skips) or no slot was filled.  Every other key stays what it was.

    `pose_regressor` may also be one of the image-conditioned heads, `mocope.MoCoPE` or `pose_regressor_cnn.Mkpts_Reg_Model`.  Their
    image pair is made in this call, on the device: img1 = `preprocess.pose_images` of the best slot's 256 x 256 crop, gathered by
    the tally's device-side best row, img0 = the same of the query's reference image, both `pose_image_size` square in the
    layout the fork feeds (linemod.py:129-130, pose/dataset.py:102-106, train0604.py:148-151); nothing is downloaded in between.
    MoCoPE goes through `regress_pose_fused_batch` on the same compacted matches with `seed=regressor_seed`, every query on its
    own, and `pose_regressed` is None under the rule above or on a non-zero status.  The CNN head reads no key points
    (`model(None, None, img0, img1)`): its `pose_regressed` is None only when no slot was filled.  With a `ReferenceSet` encoded
    for the regressor (`encode_references(..., pose_regressor=, pose_image_size=)`) the reference images, and MoCoPE's backbone
    logits of them, are gathered by `ref_index` and the backbone runs over the crops only; a set encoded without them, for
    another regressor object or another size raises ValueError.  Any other object raises TypeError."""
    from .crops import crop_proposals
    from .pose import estimate_pose_batch
    from .pose_regressor import MIN_MATCHES, regress_pose_batch
    kind = _regressor_kind(pose_regressor, "locate_match_pose_batch_u8")       # before any device work
    size = _image_size(pose_image_size, "locate_match_pose_batch_u8")
    refs, rows = _select_refs(refs_bgr, ref_index, None, "locate_match_pose_batch_u8")
    Q = len(rows) if rows is not None else int(refs.shape[0])
    if not isinstance(frames_bgr, (torch.Tensor, np.ndarray)):
        frames_bgr = [torch.as_tensor(f) for f in frames_bgr]
        if len({tuple(f.shape) for f in frames_bgr}) > 1:
            raise ValueError("locate_match_pose_batch_u8: the frames of one call have one size")
        frames_bgr = torch.stack(frames_bgr) if frames_bgr else torch.zeros(0, 1, 1, 3, dtype=torch.uint8)
    frames = torch.as_tensor(frames_bgr)
    if frames.dim() != 4:
        raise ValueError("locate_match_pose_batch_u8: frames_bgr is [Q, H, W, 3] (frames of one size)")
    boxes_in = [np.asarray(b).reshape(-1, 4) for b in bboxes_xywh]

    def per_row(K, name, n):
        K = np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float64)
        if K.shape not in ((3, 3), (n, 3, 3)):
            raise ValueError(f"locate_match_pose_batch_u8: {name} is [3, 3] or [{n}, 3, 3]")
        return np.ascontiguousarray(np.broadcast_to(K, (n, 3, 3)))

    F = Q if frame_index is None else int(frames.shape[0])
    fidx = None if frame_index is None else _frame_index(frame_index, F, Q, "locate_match_pose_batch_u8")
    if int(frames.shape[0]) != F or len(boxes_in) != F:
        raise ValueError(f"locate_match_pose_batch_u8: {Q} references, {int(frames.shape[0])} frames, {len(boxes_in)} box lists"
                         + ("" if fidx is None else " (with frame_index: one box list per frame)"))
    K0q, K1f = per_row(K0, "K0", Q), per_row(K1, "K1", F)
    counts = [len(b) for b in boxes_in]                     # per frame; `own` per query
    frame_of = list(range(Q)) if fidx is None else fidx
    own = [counts[f] for f in frame_of]
    dev = next(dinov2_model.parameters()).device
    frames = frames.to(dev)
    props = [crop_proposals(frames[f], boxes_in[f], K1f[f], out_size=out_size) for f in range(F)]
    if Q == 0 or sum(own) == 0:
        outs = [_empty_result(dev) for _ in range(Q)]
        pose = None
    else:
        crops = torch.cat([p["crops"] for p in props], 0)
        K_crops = torch.from_numpy(np.ascontiguousarray(np.concatenate([p["K"] for p in props], 0))).to(dev)
        if rows is None:
            refs = refs.to(dev)
        elif kind in ("mocope", "cnn"):          # refused before the query runs
            img0, feat0 = _pose_side(refs, rows, pose_regressor, size, "locate_match_pose_batch_u8")
        dv = _batch_u8_on_device(dinov2_model, matcher, refs, crops, counts, conf_thr, rows, fidx)
        pose = estimate_pose_batch(dv["best_kpts0"], dv["best_kpts1"], dv["best_count"], K0q, K_crops.index_select(0, dv["best_row"]),
                                   ransac_thr, ransac_conf)
        if kind == "mkpts":
            reg = regress_pose_batch(pose_regressor, dv["best_kpts0"], dv["best_kpts1"], dv["best_count"], seed=regressor_seed)
        elif kind is not None:
            from .mocope import regress_pose_fused_batch
            from .preprocess import pose_images
            img1 = pose_images(crops, dv["best_row"], size)
            if rows is None:
                img0, feat0 = pose_images(refs, None, size), None
            if kind == "mocope":
                reg = regress_pose_fused_batch(pose_regressor, dv["best_kpts0"], dv["best_kpts1"], dv["best_count"],
                                               None if feat0 is not None else img0, img1, seed=regressor_seed, feat0=feat0)
            else:
                reg_t, reg_R = pose_regressor(None, None, img0, img1)
                reg = {"R": reg_R, "t": reg_t}
        outs = _download(dv, own)
        if kind is not None:
            reg_R, reg_t = reg["R"].cpu().numpy(), reg["t"].cpu().numpy()
            reg_ok = reg["status"].cpu().numpy() == 0 if kind != "cnn" else np.ones(Q, bool)
        R, t, inl, n_inl = (pose[k].cpu().numpy() for k in ("R", "t", "inliers", "n_inliers"))
        off = np.concatenate([[0], np.cumsum(dv["best_count"].cpu().numpy())])
    for q, out in enumerate(outs):
        prop = props[frame_of[q]]
        # queries that share a frame each get arrays of their own
        out["boxes"], out["K_crops"] = (prop["boxes"], prop["K"]) if fidx is None else (prop["boxes"].copy(), prop["K"].copy())
        best = out["best_proposal"]
        if pose_regressor is not None:
            out["pose_regressed"] = None
        if best < 0:
            out["pre_bbox"], out["pre_K"], out["pose"] = None, None, None
            continue
        out["pre_bbox"], out["pre_K"] = out["boxes"][best], out["K_crops"][best]
        n = int(off[q + 1] - off[q])
        out["pose"] = (R[q], t[q], inl[off[q]:off[q + 1]]) if n >= 5 and int(n_inl[q]) > 0 else None
        if kind is not None and (n >= MIN_MATCHES or kind == "cnn") and reg_ok[q]:
            out["pose_regressed"] = (reg_R[q], reg_t[q])
    return outs


# ---- from the raw frames: the mask generator's proposals feed the batched step -------------------------------------------------
@torch.no_grad()
def locate_pose_from_frames(mask_generator, dinov2_model, matcher, refs_bgr, frames_bgr, K0, K1, conf_thr=0.9, ransac_thr=0.5,
                            ransac_conf=0.99, out_size=256, max_proposals=None):
    """The whole per-query body of the loop, eval_linemod_json.py:62-160, for Q queries in one call: `refs_bgr` [Q, H0, W0, 3]
    uint8 (the reference crops), `frames_bgr` [Q, H, W, 3] uint8 (an array, a tensor or Q frames of one size), `K0` / `K1` as in
    `locate_match_pose_batch_u8`.  `mask_generator` is a `sam_generator.SamAutomaticMaskGenerator` on the device of the other
    two models (ValueError otherwise).

    `mask_generator.propose_batch(frames)` -> the XYWH boxes of every frame's records, the only part of a record the loop reads
    (:73; no mask is unpacked, encoded or downloaded) -> `locate_match_pose_batch_u8`.  The frames reach the generator
    unchanged, in BGR channel order: the reference hands the frame of `cv2.imread` to `MASK_GEN.generate` as it is (:66-69),
    and the same proposals come only from the same input.  Frames that already sit in HBM (a uint8 CUDA tensor [Q, H, W, 3] or a
    list of CUDA frames, on the models' device) stay there: the generator resamples them on the device and the driver step reads
    the same tensor, no frame is downloaded or passes through Pillow, and the result is that of the numpy call.  `max_proposals`
    keeps the first `max_proposals` boxes of each frame in record order (None: all of them, as the reference does).

    Returns `locate_match_pose_batch_u8`'s list of Q dicts, each with one more key: `proposals`, the int64 [P_q, 4] XYWH boxes
    of that query.  A frame without a proposal yields the empty result (`best_proposal` -1, `pose` None).
    `refs_bgr` may be a `ReferenceSet` (`encode_references`): one row per frame, or `refs.select(ref_index)` naming each frame's
    row — one reference and eight frames is `refs.select([0] * 8)`.

    `frames_bgr` may be `SharedFrames(frames, frame_index)` (Q integers in [0, F)), which asks several queries of one frame, as
    `ReferenceSet.select` does on the reference side: the frames are then [F, H, W, 3] and `K1` [3, 3] or [F, 3, 3], per frame; the
    references (Q images, or a `ReferenceSet` whose rows or selection number Q) and `K0` stay per query, and `max_proposals`
    applies per frame.  The generator, the crops and their DINOv2 forward run once per frame (a frame no query names is still
    proposed for), the rest per query, and each query's dict is that of the call with `frames[frame_index]`, bit for bit, with a
    `proposals` array of its own."""
    return _pose_from_frames(mask_generator, dinov2_model, matcher, refs_bgr, frames_bgr, K0, K1, conf_thr, ransac_thr, ransac_conf,
                             out_size, max_proposals, None, 0)


def regress_pose_from_frames(mask_generator, dinov2_model, matcher, pose_regressor, refs_bgr, frames_bgr, K0, K1, conf_thr=0.9,
                             ransac_thr=0.5, ransac_conf=0.99, out_size=256, max_proposals=None, regressor_seed=0, pose_image_size=224):
    """`locate_pose_from_frames` with a learned pose head in the same call: every argument as there, plus `pose_regressor` (any
    of the three heads `locate_match_pose_batch_u8` accepts), `regressor_seed` and `pose_image_size` as in that call.  Each dict
    gains `pose_regressed` = (R [3, 3], t [3]) fp32 or None; every other key is that of `locate_pose_from_frames`."""
    if pose_regressor is None:
        raise TypeError("regress_pose_from_frames: pose_regressor is required (locate_pose_from_frames is the call without one)")
    return _pose_from_frames(mask_generator, dinov2_model, matcher, refs_bgr, frames_bgr, K0, K1, conf_thr, ransac_thr, ransac_conf,
                             out_size, max_proposals, pose_regressor, regressor_seed, pose_image_size)


def _pose_from_frames(mask_generator, dinov2_model, matcher, refs_bgr, frames_bgr, K0, K1, conf_thr, ransac_thr, ransac_conf, out_size,
                      max_proposals, pose_regressor, regressor_seed, pose_image_size=224):
    """`locate_pose_from_frames`, with `locate_match_pose_batch_u8`'s `pose_regressor` / `regressor_seed` / `pose_image_size` handed
    through."""
    _regressor_kind(pose_regressor, "locate_pose_from_frames")      # checked before any model is touched
    frame_index = None
    if isinstance(frames_bgr, SharedFrames):
        frames_bgr, frame_index = frames_bgr.frames, frames_bgr.index
    if not isinstance(frames_bgr, (torch.Tensor, np.ndarray)):
        frames_bgr = list(frames_bgr)
    fidx = None
    if frame_index is not None:            # checked before any model is touched
        F = len(frames_bgr)
        fidx = _frame_index(frame_index, F, len(refs_bgr), "locate_pose_from_frames")
        if tuple(np.shape(K1.cpu() if torch.is_tensor(K1) else K1)) not in ((3, 3), (F, 3, 3)):
            raise ValueError(f"locate_pose_from_frames: K1 is [3, 3] or [{F}, 3, 3], per frame")
    dev = next(dinov2_model.parameters()).device
    devices = {"mask_generator": torch.device(mask_generator.predictor.device), "dinov2_model": dev,
               "matcher": next(matcher.parameters()).device}
    if len(set(devices.values())) > 1:
        raise ValueError("locate_pose_from_frames: the models must be on one device, got "
                         + ", ".join(f"{k} on {v}" for k, v in devices.items()))
    if max_proposals is not None and int(max_proposals) < 0:
        raise ValueError(f"locate_pose_from_frames: max_proposals is None or a count, got {max_proposals}")
    frames = stack = frames_on_device(frames_bgr, "locate_pose_from_frames")   # frames in HBM stay there, for both calls below
    if stack is None:
        if isinstance(frames_bgr, torch.Tensor):
            frames_bgr = frames_bgr.cpu().numpy()
        frames = [np.asarray(f.cpu() if torch.is_tensor(f) else f) for f in frames_bgr]
        stack = np.stack(frames) if frames else frames
    if fidx is None and len(frames) != len(refs_bgr):
        raise ValueError(f"locate_pose_from_frames: {len(refs_bgr)} references, {len(frames)} frames")
    proposals = mask_generator.propose_batch(frames)            # mixed frame sizes raise there
    if max_proposals is not None:
        proposals = [p[:int(max_proposals)] for p in proposals]
    outs = locate_match_pose_batch_u8(dinov2_model, matcher, refs_bgr, stack, proposals, K0, K1, conf_thr, ransac_thr, ransac_conf,
                                      out_size, frame_index=fidx, pose_regressor=pose_regressor, regressor_seed=regressor_seed,
                                      pose_image_size=pose_image_size)
    for q, out in enumerate(outs):
        out["proposals"] = proposals[q] if fidx is None else proposals[fidx[q]].copy()
    return outs


def locate_pose_from_frame(mask_generator, dinov2_model, matcher, ref_bgr, frame_bgr, K0, K1, conf_thr=0.9, ransac_thr=0.5,
                           ransac_conf=0.99, out_size=256, max_proposals=None):
    """`locate_pose_from_frames` for one query: `ref_bgr` [H0, W0, 3], `frame_bgr` [H, W, 3], `K0` / `K1` [3, 3]; one dict.
    `ref_bgr` may be a `ReferenceSet` standing for one query: a set of one, or `refs.select([row])`."""
    def batch_of_one(a):
        return a[None] if on_device(a) else np.asarray(a.cpu() if torch.is_tensor(a) else a)[None]
    ref = ref_bgr if isinstance(ref_bgr, ReferenceSet) else batch_of_one(ref_bgr)
    return locate_pose_from_frames(mask_generator, dinov2_model, matcher, ref, batch_of_one(frame_bgr), K0, K1, conf_thr, ransac_thr,
                                   ransac_conf, out_size, max_proposals)[0]


def locate_poses_in_frame(mask_generator, dinov2_model, matcher, refs_bgr, frame_bgr, K0, K1, conf_thr=0.9, ransac_thr=0.5,
                          ransac_conf=0.99, out_size=256, max_proposals=None, pose_regressor=None, regressor_seed=0,
                          pose_image_size=224):
    """R references asked of ONE frame: `refs_bgr` [R, H0, W0, 3] uint8 or a `ReferenceSet` (its R rows, or its selection),
    `frame_bgr` [H, W, 3], `K0` [3, 3] or [R, 3, 3], `K1` [3, 3].  `locate_pose_from_frames` with `SharedFrames([frame], [0] * R)`:
    the frame passes through the mask generator once and its crops through DINOv2 once.  Returns a list of R dicts.
    `pose_regressor` / `regressor_seed` / `pose_image_size`: as in `locate_match_pose_batch_u8` (each dict gains `pose_regressed`;
    all three heads are accepted)."""
    frame = frame_bgr[None] if on_device(frame_bgr) else np.asarray(frame_bgr.cpu() if torch.is_tensor(frame_bgr) else frame_bgr)[None]
    return _pose_from_frames(mask_generator, dinov2_model, matcher, refs_bgr, SharedFrames(frame, [0] * len(refs_bgr)), K0, K1,
                             conf_thr, ransac_thr, ransac_conf, out_size, max_proposals, pose_regressor, regressor_seed, pose_image_size)
