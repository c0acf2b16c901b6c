"""Op-level Python wrappers over the C ABI (one HIP kernel each).  fp32, CUDA(HIP) tensors only."""
import ctypes as C

import torch

from . import _lib
from ._lib import check, on_device_of, ptr, require_cuda, stream_of

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_LS_RES = 0, 1, 2


def _f32c(t, what):
    require_cuda(t, what)
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32, got {t.dtype}")
    return t.contiguous()


def layernorm(x, weight, bias, eps=1e-6):
    """nn.LayerNorm over the last dim (vision_transformer.py:90)."""
    x = _f32c(x, "layernorm")
    dim = x.shape[-1]
    y = torch.empty_like(x)
    with on_device_of(x):
        check(_lib.lib().pope_layernorm_f32(ptr(x), ptr(_f32c(weight, "ln.w")), ptr(_f32c(bias, "ln.b")), ptr(y),
                                            x.numel() // dim, dim, float(eps), stream_of(x.device)), "pope_layernorm_f32")
    return y


def _flag_ptr(range_flag):
    """Device pointer of an optional int32[1] f16x3 range-guard word (pope_hip.h: range_flag)."""
    if range_flag is None:
        return None
    if range_flag.dtype != torch.int32 or range_flag.numel() < 1 or not range_flag.is_cuda:
        raise ValueError("range_flag must be an int32 CUDA tensor")
    return C.c_void_p(range_flag.data_ptr())


def linear(a, weight, bias=None, epilogue=EPI_BIAS, gamma=None, res=None, out=None, precision="f32", range_flag=None):
    """nn.Linear with fused epilogue: bias | bias+GELU(erf) | res + gamma*(.+bias).
    precision: "f32" (exact fp32 MFMA chain) or "f16x3" (error-compensated f16 matrix cores; `range_flag`, an
    int32[1] device tensor, receives POPE_RANGE_INPUT when an operand leaves the f16 range)."""
    a = _f32c(a, "linear")
    weight = _f32c(weight, "linear.w")
    n, k = weight.shape
    assert a.shape[-1] == k
    m = a.numel() // k
    if out is None:
        out = torch.empty(*a.shape[:-1], n, device=a.device, dtype=torch.float32)
    with on_device_of(a):
        check(_lib.lib().pope_linear_f32(ptr(a), ptr(weight), ptr(bias), ptr(out), m, n, k, epilogue, ptr(gamma),
                                         ptr(res), _lib.PRECISIONS[precision], _flag_ptr(range_flag), stream_of(a.device)),
              "pope_linear_f32")
    return out


def patch_embed(img, proj_w, posb, patch, precision="f32", range_flag=None):
    """PatchEmbed + cls + pos (patch_embed.py:69-82, vision_transformer.py:191-200).  precision="f16x3": patches are
    gathered into hi/lo f16 planes and multiplied on the f16 matrix cores (3 MFMAs per product, fp32 accumulate)."""
    img = _f32c(img, "patch_embed")
    b, c, h, w = img.shape
    assert c == 3
    assert h % patch == 0, f"Input image height {h} is not a multiple of patch height {patch}"
    assert w % patch == 0, f"Input image width {w} is not a multiple of patch width: {patch}"
    dim = proj_w.shape[0]
    ntok = 1 + (h // patch) * (w // patch)
    assert posb.shape == (ntok, dim)
    out = torch.empty(b, ntok, dim, device=img.device, dtype=torch.float32)
    pw = _f32c(proj_w.reshape(dim, -1), "pe.w")
    if precision == "f16x3":
        kp = (pw.shape[1] + 31) // 32 * 32
        wp = _lib.to_planes(torch.nn.functional.pad(pw, (0, kp - pw.shape[1])), _lib.PLANES_W_SCALE)
        scratch = torch.empty(b * ntok * kp * 4, dtype=torch.uint8, device=img.device)
        with on_device_of(img):
            check(_lib.lib().pope_patch_embed_planes_f32(ptr(img), ptr(wp), ptr(_f32c(posb, "posb")), ptr(out), b, h, w, patch,
                                                         dim, ptr(scratch), scratch.numel(), _flag_ptr(range_flag),
                                                         stream_of(img.device)),
                  "pope_patch_embed_planes_f32")
        return out
    with on_device_of(img):
        check(_lib.lib().pope_patch_embed_f32(ptr(img), ptr(pw), ptr(_f32c(posb, "posb")),
                                              ptr(out), b, h, w, patch, dim, stream_of(img.device)), "pope_patch_embed_f32")
    return out


def attention(qkv, heads, precision="f32", range_flag=None):
    """softmax((q/8) k^T) v on qkv[B,N,3*heads*64] (attention.py:51-59)."""
    qkv = _f32c(qkv, "attention")
    b, n, d3 = qkv.shape
    assert d3 == 3 * heads * 64
    out = torch.empty(b, n, heads * 64, device=qkv.device, dtype=torch.float32)
    with on_device_of(qkv):
        check(_lib.lib().pope_attention_f32(ptr(qkv), ptr(out), b, n, heads, _lib.PRECISIONS[precision],
                                            _flag_ptr(range_flag), stream_of(qkv.device)), "pope_attention_f32")
    return out


def cls_cosine(ref, fea, eps=1e-8):
    """F.cosine_similarity(ref[1,D], fea[P,D], dim=1, eps) (eval_linemod_json.py:94)."""
    ref = _f32c(ref, "cls_cosine").reshape(-1)
    fea = _f32c(fea, "cls_cosine")
    p, d = fea.shape
    assert ref.numel() == d
    scores = torch.empty(p, device=fea.device, dtype=torch.float32)
    with on_device_of(ref):
        check(_lib.lib().pope_cls_cosine_f32(ptr(ref), ptr(fea), p, d, float(eps), ptr(scores), stream_of(fea.device)),
              "pope_cls_cosine_f32")
    return scores


def streaming_top3(scores):
    """Host-side streaming top-3 vote (eval_linemod_json.py:71,95-101).
    Returns (slot_scores float32[3], slot_index int64[3], -1 = empty slot)."""
    import numpy as np
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).reshape(-1))
    slots = np.zeros(3, np.float32)
    idx = np.zeros(3, np.int64)
    check(_lib.lib().pope_streaming_top3_host(s.ctypes.data_as(_lib.c_float_p), int(s.size),
                                              slots.ctypes.data_as(_lib.c_float_p),
                                              idx.ctypes.data_as(_lib.c_ll_p)), "pope_streaming_top3_host")
    return slots, idx


def vote_top3_batch(cls_ref, cls_prop, proposals_per_query, eps=1e-8):
    """`cls_cosine` + `streaming_top3` for Q queries in one launch, results on the device (pope_vote_top3_batch_f32).
    cls_ref [Q, D], cls_prop [N, D]; `proposals_per_query`: Q counts summing to N (query q owns the next P_q rows), or the
    int32 [Q + 1] row offsets themselves as a tensor.  Returns a dict of device tensors: scores [N], slot_scores [Q, 3],
    slot_index [Q, 3] int64 (-1 = empty slot), pair_row [3 Q] int32 (global row of each slot, 0 when dead), pair_live [3 Q] uint8,
    and `seg`."""
    cls_ref = _f32c(cls_ref, "vote_top3_batch")
    cls_prop = _f32c(cls_prop, "vote_top3_batch")
    dev = cls_ref.device
    q, d = cls_ref.shape
    n = int(cls_prop.shape[0])
    if torch.is_tensor(proposals_per_query):
        seg = proposals_per_query.to(device=dev, dtype=torch.int32).contiguous()
    else:
        counts = [int(p) for p in proposals_per_query]
        if min(counts, default=0) < 0 or sum(counts) != n:
            raise ValueError("vote_top3_batch: proposals_per_query must be non-negative and sum to the number of proposal rows")
        seg = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
    if seg.numel() != q + 1 or (n and cls_prop.shape[1] != d):
        raise ValueError("vote_top3_batch: one segment per reference row, and one feature width")
    out = {"scores": torch.empty(n, device=dev, dtype=torch.float32), "slot_scores": torch.empty(q, 3, device=dev, dtype=torch.float32),
           "slot_index": torch.empty(q, 3, device=dev, dtype=torch.int64), "pair_row": torch.empty(3 * q, device=dev, dtype=torch.int32),
           "pair_live": torch.empty(3 * q, device=dev, dtype=torch.uint8), "seg": seg}
    with on_device_of(cls_ref):
        check(_lib.lib().pope_vote_top3_batch_f32(ptr(cls_ref), ptr(cls_prop), ptr(seg), q, n, d, float(eps), ptr(out["scores"]),
                                                  ptr(out["slot_scores"]), ptr(out["slot_index"]), ptr(out["pair_row"]),
                                                  ptr(out["pair_live"]), stream_of(dev)), "pope_vote_top3_batch_f32")
    return out


def vote_top3_shared(cls_ref, cls_prop, proposals_per_segment, segment_of_query, eps=1e-8):
    """`vote_top3_batch` for Q queries that share proposal segments (pope_vote_top3_shared_f32): cls_ref [Q, D], cls_prop [N, D]
    holding every segment once; `proposals_per_segment`: S counts summing to N (segment s owns the next P_s rows);
    `segment_of_query`: Q integers in [0, S), the segment query q votes over (two queries may name one segment, a segment may
    go unnamed).  The proposals are read in place, no copy per query is made.  Returns the dict of `vote_top3_batch` — scores
    [sum of the queries' P] with query q's at score_begin[q] .. score_begin[q + 1], slot_index local to the segment, pair_row
    the global row in N, `seg` the [S + 1] row offsets — plus `score_begin`, int32 [Q + 1].  ValueError on counts that are
    negative or do not sum to N, and on a segment outside [0, S), before anything is launched."""
    import numpy as np
    cls_ref = _f32c(cls_ref, "vote_top3_shared")
    cls_prop = _f32c(cls_prop, "vote_top3_shared")
    dev = cls_ref.device
    if cls_ref.dim() != 2 or cls_prop.dim() != 2:
        raise ValueError("vote_top3_shared: cls_ref is [Q, D] and cls_prop [N, D]")
    q, d = cls_ref.shape
    n = int(cls_prop.shape[0])
    counts = [int(p) for p in proposals_per_segment]
    if min(counts, default=0) < 0 or sum(counts) != n:
        raise ValueError("vote_top3_shared: proposals_per_segment must be non-negative and sum to the number of proposal rows")
    which = np.asarray(segment_of_query.cpu() if torch.is_tensor(segment_of_query) else segment_of_query)
    if which.ndim != 1 or (which.size and not np.issubdtype(which.dtype, np.integer)):
        raise ValueError("vote_top3_shared: segment_of_query is a list of integers, one per query")
    if which.size != q or (n and cls_prop.shape[1] != d):
        raise ValueError("vote_top3_shared: one segment index per reference row, and one feature width")
    if which.size and (which.min() < 0 or which.max() >= len(counts)):
        raise ValueError(f"vote_top3_shared: segment_of_query values must lie in [0, {len(counts)}), got "
                         f"[{int(which.min())}, {int(which.max())}]")
    which = [int(s) for s in which]
    total = sum(counts[s] for s in which)
    if max(n, total) > 0x7fffffff:
        raise ValueError("vote_top3_shared: the row and score offsets are int32")
    offsets = lambda c: torch.tensor([0] + c, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)  # noqa: E731
    seg, score_begin = offsets(counts), offsets([counts[s] for s in which])
    query_seg = torch.tensor(which, dtype=torch.int32).to(dev)
    out = {"scores": torch.empty(total, device=dev, dtype=torch.float32), "slot_scores": torch.empty(q, 3, device=dev, dtype=torch.float32),
           "slot_index": torch.empty(q, 3, device=dev, dtype=torch.int64), "pair_row": torch.empty(3 * q, device=dev, dtype=torch.int32),
           "pair_live": torch.empty(3 * q, device=dev, dtype=torch.uint8), "seg": seg, "score_begin": score_begin}
    with on_device_of(cls_ref):
        check(_lib.lib().pope_vote_top3_shared_f32(ptr(cls_ref), ptr(cls_prop), ptr(seg), len(counts), ptr(query_seg), ptr(score_begin),
                                                   q, n, d, float(eps), ptr(out["scores"]), ptr(out["slot_scores"]),
                                                   ptr(out["slot_index"]), ptr(out["pair_row"]), ptr(out["pair_live"]), stream_of(dev)),
              "pope_vote_top3_shared_f32")
    return out


def slot_tally(m_bids, mconf, mkpts0_f, mkpts1_f, pair_live, conf_thr=0.9):
    """The matches a `Matcher` call over 3 Q pairs published (pair 3 q + s = slot s of query q) -> per-slot counts, the best
    slot of every query and its matches compacted for `estimate_pose_batch` (pope_slot_tally_f32), all on the device.
    Returns pair_begin / pair_count [3 Q] int32, matching_score [Q, 3] int64, best_slot / best_count [Q] int32 and
    best_kpts0 / best_kpts1 [M, 2] (each query's best-slot matches at the exclusive scan of best_count)."""
    require_cuda(m_bids, "slot_tally")
    if m_bids.dtype != torch.int64 or pair_live.dtype != torch.uint8:
        raise TypeError("slot_tally: m_bids is int64 (as the Matcher publishes it), pair_live uint8")
    dev = m_bids.device
    m_bids, pair_live = m_bids.contiguous(), pair_live.to(dev).contiguous()
    mconf, mk0, mk1 = _f32c(mconf, "slot_tally"), _f32c(mkpts0_f, "slot_tally"), _f32c(mkpts1_f, "slot_tally")
    m = int(m_bids.numel())
    if pair_live.numel() % 3 or mconf.numel() != m or mk0.shape != (m, 2) or mk1.shape != (m, 2):
        raise ValueError("slot_tally: m_bids / mconf [M], mkpts0_f / mkpts1_f [M, 2], pair_live [3 Q]")
    q = pair_live.numel() // 3
    new = torch.zeros if m == 0 else torch.empty      # without matches nothing is launched: the empty tally is all zeros
    out = {"pair_begin": new(3 * q, device=dev, dtype=torch.int32), "pair_count": new(3 * q, device=dev, dtype=torch.int32),
           "matching_score": new(q, 3, device=dev, dtype=torch.int64), "best_slot": new(q, device=dev, dtype=torch.int32),
           "best_count": new(q, device=dev, dtype=torch.int32), "best_kpts0": torch.empty(m, 2, device=dev, dtype=torch.float32),
           "best_kpts1": torch.empty(m, 2, device=dev, dtype=torch.float32)}
    with on_device_of(m_bids):
        check(_lib.lib().pope_slot_tally_f32(ptr(m_bids), ptr(mconf), ptr(mk0), ptr(mk1), ptr(pair_live), q, m, float(conf_thr),
                                             *[ptr(out[k]) for k in ("pair_begin", "pair_count", "matching_score", "best_slot",
                                                                     "best_count", "best_kpts0", "best_kpts1")], stream_of(dev)),
              "pope_slot_tally_f32")
    return out
