"""Dense cross-image matcher on the HIP kernels: mirror of the reference ``CoarseMatching``
(src/matcher/utils/coarse_matching.py:60-261) for the eval path with both of its matchers, ``match_type='dual_softmax'`` and
``match_type='sinkhorn'`` (log-domain optimal transport with the learned dustbin score ``bin_score``, csrc/sinkhorn.hip), plus
a functional ``dense_match`` used directly on DINOv2 patch tokens (BASELINE config 3).
"""
import ctypes as C
import warnings

import torch
import torch.nn as nn

from . import _lib
from ._lib import PopeRangeError, check, on_device_of, ptr, require_cuda, stream_of

# src/matcher/utils/cvpr_ds_config.py:10-50, lower-cased as by lower_config(); plain data.
default_cfg = {
    "backbone_type": "ResNetFPN",
    "resolution": (8, 2),
    "fine_window_size": 5,
    "fine_concat_coarse_feat": True,
    "resnetfpn": {"initial_dim": 128, "block_dims": [128, 196, 256]},
    "coarse": {"d_model": 256, "d_ffn": 256, "nhead": 8, "layer_names": ["self", "cross"] * 4,
               "attention": "linear", "temp_bug_fix": False},
    "match_coarse": {"thr": 0.2, "border_rm": 2, "match_type": "dual_softmax", "dsmax_temperature": 0.1,
                     "skh_iters": 3, "skh_init_bin_score": 1.0, "skh_prefilter": True,
                     "train_coarse_percent": 0.4, "train_pad_num_gt_min": 200},
    "fine": {"d_model": 128, "d_ffn": 128, "nhead": 8, "layer_names": ["self", "cross"], "attention": "linear"},
}


def _rows_contiguous(f):
    """Accept [n, L, C] views whose rows are dense (e.g. x_norm[:, 1:]) without copying."""
    if f.stride(2) == 1 and f.stride(1) == f.shape[2] and f.stride(0) >= f.shape[1] * f.shape[2] \
            and f.stride(0) % 4 == 0 and f.data_ptr() % 16 == 0:
        return f
    return f.contiguous()


DEFAULT_PRECISION = "f16x3"   # arithmetic of the L x S x C contraction ("f32": fp32-in MFMA); see DESIGN.md §2


@torch.no_grad()
def dense_match(feat0, feat1, hw0_c, hw1_c, hw0_i, thr=0.2, border_rm=2, temperature=0.1, precision=None,
                on_overflow="rerun_f32", want_conf=True, mask0=None, mask1=None, border_mask0=None, border_mask1=None,
                scale0=None, scale1=None, match_type="dual_softmax", bin_score=None, skh_iters=3, skh_prefilter=True):
    """All-pairs similarity -> dual softmax (or Sinkhorn) -> threshold/border/mutual-NN -> ordered matches.

    feat0 [n,L,C], feat1 [n,S,C] fp32 on the GPU.  Returns the dict CoarseMatching publishes
    (coarse_matching.py:145-148,239-259): conf_matrix, b_ids, i_ids, j_ids, gt_mask, m_bids,
    mkpts0_c, mkpts1_c, mconf — plus `counts` (matches per pair, int32[n]).  `want_conf=False` (batch pipelines that
    only consume the match lists) does not publish conf_matrix.
    One host synchronisation (to size the outputs), like torch.where in the reference.
    precision "f16x3" (default) keeps feat / sqrt(C) * 256 as f16 pairs: the kernel that converts them guards the
    f16 range with a device flag that travels with the match counts; on a breach the call is repeated with the
    fp32-MFMA contraction (`on_overflow="rerun_f32"`) or raises PopeRangeError ("raise").

    Padded batches and rescaling (coarse_matching.py:115-118,178-184,242-250), all optional and independent of each other:
    mask0 [n, L] / mask1 [n, S] (or [n, h, w]) fill sim with -1e9 where mask0[i] * mask1[j] == 0 (a missing one counts as
    ones); border_mask0 / border_mask1 [n, h, w] put the bottom / right border at each pair's valid extent; scale0 / scale1
    [n, 2] (x, y) rescale mkpts0_c / mkpts1_c.  Masks are bool or 0 / 1; the kernels apply them, torch only converts.

    match_type="sinkhorn" (coarse_matching.py:121-143) replaces the dual softmax by `skh_iters` (>= 1) iterations of log-domain
    optimal transport over the similarity without temperature, bordered by a dustbin row and column of score `bin_score`;
    conf_matrix is the assignment without its dustbins, and `skh_prefilter` zeroes the rows and columns whose largest
    assignment is their dustbin.  `bin_score` is a 0-d or one-element fp32 tensor (the learned parameter): the kernels read it
    from its own storage, the host never does; a tensor on another device is copied over.  `temperature` is not used."""
    if match_type not in ("dual_softmax", "sinkhorn"):
        raise ValueError(f"dense_match: match_type is 'dual_softmax' or 'sinkhorn', got {match_type!r}")
    sinkhorn = match_type == "sinkhorn"
    if sinkhorn:
        if not isinstance(bin_score, torch.Tensor):
            raise TypeError("dense_match: match_type='sinkhorn' needs bin_score as a float32 tensor (0-d or one element)")
        if bin_score.dtype != torch.float32:
            raise TypeError(f"dense_match: bin_score is float32, got {bin_score.dtype}")
        if bin_score.numel() != 1:
            raise ValueError(f"dense_match: bin_score holds one value, got shape {tuple(bin_score.shape)}")
        if int(skh_iters) < 1:
            raise ValueError(f"dense_match: skh_iters >= 1, got {skh_iters}")
    require_cuda(feat0, "dense_match")
    require_cuda(feat1, "dense_match")
    if feat0.dtype != torch.float32 or feat1.dtype != torch.float32:
        raise TypeError("dense_match expects float32 features")
    feat0, feat1 = _rows_contiguous(feat0), _rows_contiguous(feat1)
    n, L, Cc = feat0.shape
    S = feat1.shape[1]
    h0, w0 = int(hw0_c[0]), int(hw0_c[1])
    h1, w1 = int(hw1_c[0]), int(hw1_c[1])
    assert feat1.shape[0] == n and feat1.shape[2] == Cc and L == h0 * w0 and S == h1 * w1
    dev = feat0.device
    if mask0 is not None and mask0.dim() == 3:
        mask0 = mask0.flatten(-2)
    if mask1 is not None and mask1.dim() == 3:
        mask1 = mask1.flatten(-2)
    fill0 = _lib.padding_mask(mask0, (n, L), dev, "dense_match mask0")
    fill1 = _lib.padding_mask(mask1, (n, S), dev, "dense_match mask1")
    bord0 = _lib.padding_mask(border_mask0, (n, h0, w0), dev, "dense_match border_mask0")
    bord1 = _lib.padding_mask(border_mask1, (n, h1, w1), dev, "dense_match border_mask1")
    sc0 = _lib.pair_scale(scale0, n, dev, "dense_match scale0")
    sc1 = _lib.pair_scale(scale1, n, dev, "dense_match scale1")
    extra = (fill0, fill1, bord0, bord1, sc0, sc1)
    if n == 0:   # an empty batch: what torch.where gives the reference on a [0, L, S] mask
        el, ef = torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
        out = {"b_ids": el, "i_ids": el.clone(), "j_ids": el.clone(), "gt_mask": torch.empty(0, dtype=torch.bool, device=dev),
               "m_bids": el.clone(), "mkpts0_c": ef.reshape(0, 2), "mkpts1_c": ef.reshape(0, 2).clone(), "mconf": ef.clone(),
               "counts": torch.empty(0, dtype=torch.int32),
               "conf_matrix": torch.empty(0, L, S, dtype=torch.float32, device=dev) if want_conf else None}
        return out
    lib = _lib.lib()
    precision = precision or DEFAULT_PRECISION
    if Cc % 32 or Cc < 64:
        precision = "f32"   # the planes layout needs whole 32-column chunks
    if sinkhorn:
        bin_score = bin_score.detach()
        if bin_score.device != dev:
            bin_score = bin_score.to(dev)
    conf = torch.empty(n, L, S, dtype=torch.float32, device=dev) if want_conf else None
    cap = n * L
    b_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    i_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    j_ids = torch.empty(cap, dtype=torch.int64, device=dev)
    mconf = torch.empty(cap, dtype=torch.float32, device=dev)
    mk0 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    mk1 = torch.empty(cap, 2, dtype=torch.float32, device=dev)
    counts = torch.zeros(n + 2, dtype=torch.int32, device=dev)   # per-pair counts | total | f16x3 range-guard word
    args = _lib.DenseMatchArgs(
        feat0=feat0.data_ptr(), feat1=feat1.data_ptr(),
        # (the stride of a size-1 dimension is arbitrary in torch: a batch of one has no batch stride to speak of)
        stride0=feat0.stride(0) if n > 1 else L * Cc, stride1=feat1.stride(0) if n > 1 else S * Cc,
        n=n, L=L, S=S, C=Cc, h0=h0, w0=w0, h1=h1, w1=w1, thr=float(thr), border_rm=int(border_rm), temperature=float(temperature),
        scale=float(hw0_i[0] / hw0_c[0]),  # coarse_matching.py:242 (heights only)
        match_type=_lib.MATCH_TYPES[match_type], bin_score=ptr(bin_score) if sinkhorn else None,
        skh_iters=int(skh_iters), skh_prefilter=int(bool(skh_prefilter)),
        fill_mask0=ptr(fill0), fill_mask1=ptr(fill1), border_mask0=ptr(bord0), border_mask1=ptr(bord1), scale0=ptr(sc0),
        scale1=ptr(sc1), conf_matrix=ptr(conf), b_ids=ptr(b_ids), i_ids=ptr(i_ids), j_ids=ptr(j_ids), mconf=ptr(mconf),
        mkpts0_c=ptr(mk0), mkpts1_c=ptr(mk1), counts=ptr(counts), precision=_lib.PRECISIONS[precision],
        range_flag=counts.data_ptr() + 4 * (n + 1) if precision == "f16x3" else None)
    args.workspace_bytes = lib.pope_dense_match_workspace_bytes(C.byref(args))
    ws = torch.empty(args.workspace_bytes, dtype=torch.uint8, device=dev)
    args.workspace = ws.data_ptr()
    with on_device_of(feat0):
        check(lib.pope_dense_match_f32(C.byref(args), stream_of(dev)), "pope_dense_match_f32")
    counts_h = counts.cpu()  # sync point
    if int(counts_h[n + 1]):   # features outside the f16x3 range: nothing of this call is valid
        msg = (f"pope_amd: f16x3 range contract breached in dense_match ({_lib.describe_range_bits(int(counts_h[n + 1]))}: "
               f"|feat| / sqrt(C) * {_lib.PLANES_W_SCALE:g} >= {_lib.F16_MAX:g} or non-finite)")
        if on_overflow == "raise":
            raise PopeRangeError(msg)
        warnings.warn(msg + "; re-running with the fp32-MFMA contraction")
        del conf, ws, b_ids, i_ids, j_ids, mconf, mk0, mk1
        return dense_match(feat0, feat1, hw0_c, hw1_c, hw0_i, thr, border_rm, temperature, "f32", on_overflow, want_conf,
                           *extra, match_type=match_type, bin_score=bin_score, skh_iters=skh_iters, skh_prefilter=skh_prefilter)
    m = int(counts_h[n])
    b_ids, i_ids, j_ids, mconf = b_ids[:m], i_ids[:m], j_ids[:m], mconf[:m]
    return {
        "conf_matrix": conf,
        "b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids,
        "gt_mask": mconf == 0, "m_bids": b_ids,          # eval: mconf > thr, the `!= 0` filter is a no-op
        "mkpts0_c": mk0[:m], "mkpts1_c": mk1[:m], "mconf": mconf,
        "counts": counts_h[:n],
    }


def _loftr():
    from . import loftr
    return loftr


class CoarseMatching(nn.Module):
    """Drop-in for the reference module (eval), match_type 'dual_softmax' or 'sinkhorn'.  The Sinkhorn matcher owns the learned
    dustbin score as the parameter `bin_score` (initialised to config['skh_init_bin_score']; the `coarse_matching.bin_score` of
    the released `*_ot` checkpoints) and hands the parameter itself to the kernels.  config['sparse_spvs'] is accepted and
    ignored: the `conf_matrix_with_bin` it asks for is consumed only by the training loss."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.thr = config["thr"]
        self.border_rm = config["border_rm"]
        self.train_coarse_percent = config["train_coarse_percent"]
        self.train_pad_num_gt_min = config["train_pad_num_gt_min"]
        self.match_type = config["match_type"]
        if self.match_type == "dual_softmax":
            self.temperature = config["dsmax_temperature"]
        elif self.match_type == "sinkhorn":
            self.bin_score = nn.Parameter(torch.tensor(config["skh_init_bin_score"], dtype=torch.float32))
            self.skh_iters = config["skh_iters"]
            self.skh_prefilter = config["skh_prefilter"]
        else:
            raise NotImplementedError(f"pope_amd: match_type is 'dual_softmax' or 'sinkhorn', got {self.match_type!r}")

    def forward(self, feat_c0, feat_c1, data, mask_c0=None, mask_c1=None):
        """mask_c0 [n, L] / mask_c1 [n, S]: the similarity fill (coarse_matching.py:115-118, applied when mask_c0 is given);
        data['mask0'] / data['mask1'] [n, h, w]: the padded border rule (:178-184, keyed on 'mask0' in data);
        data['scale0'] / data['scale1'] [n, 2]: (x, y) factors of mkpts0_c / mkpts1_c (:243-250, each keyed on itself).
        The three come from different places in the reference and are honoured independently."""
        if self.training:
            raise NotImplementedError("pope_amd: inference only (call .eval())")
        if mask_c0 is not None and mask_c1 is None:
            raise ValueError("CoarseMatching: mask_c0 needs mask_c1 (the fill is mask_c0[i] * mask_c1[j])")
        fill0, fill1 = (mask_c0, mask_c1) if mask_c0 is not None else (None, None)
        bord0, bord1 = (data["mask0"], data["mask1"]) if "mask0" in data else (None, None)
        if self.match_type == "sinkhorn":
            how = {"match_type": "sinkhorn", "bin_score": self.bin_score, "skh_iters": self.skh_iters,
                   "skh_prefilter": self.skh_prefilter}
        else:
            how = {"temperature": self.temperature}
        out = dense_match(feat_c0, feat_c1, data["hw0_c"], data["hw1_c"], data["hw0_i"], self.thr, self.border_rm,
                          mask0=fill0, mask1=fill1, border_mask0=bord0, border_mask1=bord1,
                          scale0=data.get("scale0"), scale1=data.get("scale1"), **how)
        out.pop("counts")
        data.update(out)


def _image0_index(index, n, R):
    """data['image0_index'] as a host int64 [n] tensor: pair b uses reference row index[b].  None: arange(n), which needs
    R == n.  ValueError on a float dtype, a wrong length or a value outside [0, R) — on the host, before any launch."""
    if index is None:
        if R != n:
            raise ValueError(f"Matcher: {R} reference images for {n} pairs needs data['image0_index'] (one reference row per pair)")
        return torch.arange(n, dtype=torch.int64)
    idx = torch.as_tensor(index).detach().cpu()
    if idx.dtype in (torch.bool,) or idx.is_floating_point() or idx.is_complex():
        raise ValueError(f"Matcher: image0_index holds integers (int64), got {idx.dtype}")
    if idx.dim() != 1 or idx.shape[0] != n:
        raise ValueError(f"Matcher: image0_index has one entry per pair ([{n}]), got {tuple(idx.shape)}")
    idx = idx.to(torch.int64)
    if n and (int(idx.min()) < 0 or int(idx.max()) >= R):
        raise ValueError(f"Matcher: image0_index values must lie in [0, {R}), got [{int(idx.min())}, {int(idx.max())}]")
    return idx.contiguous()


class ReferenceEncoding:
    """What the Matcher makes of R reference images before stream 0 meets a stream 1 (`Matcher.encode_reference`): the 1/2-
    resolution fine map (the backbone's zero-bordered NHWC buffer, seen as NCHW) and the coarse map after the position code and
    every leading 'self' layer of the coarse transformer ([R, L, 256]); the first 'cross' layer mixes the pair, so nothing
    later can be kept.  The image itself is kept too: the fp32 forms the range guard asks for, and a re-encoding after the
    matcher's weights changed or moved (the encoding carries `_lib.slots_key` of the matcher's parameters and buffers), are built
    from it on the next use.  Forms are held per arithmetic mode of the backbone ("f16x3" / "f16" / "f32") and of the
    transformer ("f16x3" / "f32"), each
    with the range bits it raised; at 256 x 256 a form is ~8.7 MB fine map + 2 x 1 MB coarse map per reference."""

    def __init__(self, matcher, image0):
        if not isinstance(image0, torch.Tensor) or image0.dim() != 4:
            raise ValueError("Matcher.encode_reference: image0 is a [R, 1, H0, W0] tensor")
        self._matcher = matcher
        self.image = matcher.backbone.checked_input(image0)
        if self.image is image0:
            self.image = image0.clone()   # the caller may overwrite theirs
        self.key, self._bb, self._lead = None, {}, {}
        self.mode = None   # the backbone arithmetic a call reads this encoding in (the backbone's `precision` | "f32"), set when it is built
        self._fresh()

    R = property(lambda self: int(self.image.shape[0]))
    hw_i = property(lambda self: self.image.shape[2:])

    def _fresh(self):
        """Drop every form built under other weights, or on another device, than the matcher has now."""
        m = self._matcher
        key = (m._moves, _lib.slots_key(m._ref_slots()))
        if key != self.key:
            self.key, self._bb, self._lead = key, {}, {}
            dev = next(m.parameters()).device
            if self.image.device != dev:
                self.image = self.image.to(dev)

    def _put_backbone(self, precision, maps, bits):
        feat_c, feat_f = maps
        m = self._matcher
        self._bb[precision] = {"fine": feat_f, "hw_c": feat_c.shape[2:], "bits": bits,
                               "cpos": None if bits else m.pos_encoding(feat_c).flatten(2).transpose(1, 2)}

    def backbone(self, precision):
        """{'fine' [R, 128, H/2, W/2], 'cpos' [R, L, 256] (position code added), 'hw_c', 'bits'} of one backbone mode; a form
        whose bits are raised holds nothing usable ('cpos' None)."""
        if precision not in self._bb:
            maps, flag = self._matcher.backbone._run(self.image, precision)
            self._put_backbone(precision, maps, int(flag.item()) if precision != "f32" else 0)
        return self._bb[precision]

    def leading(self, bb_precision, precision):
        """([R, L, 256] after the leading 'self' layers, range bits) for one (backbone mode, transformer mode)."""
        k = (bb_precision, precision)
        if k not in self._lead:
            self._lead[k] = self._matcher.loftr_coarse.encode_leading(self.backbone(bb_precision)["cpos"], precision)
        return self._lead[k]


class Matcher(nn.Module):
    """Drop-in for the reference `Matcher` (src/matcher/matcher.py:12-85): same constructor, same in-place
    `forward(data, only_att_fea=False)` protocol and published keys, same checkpoint layout (`matcher.`
    prefix stripped on load, :81-85).  Every stage — CNN, linear-attention transformers, coarse matching, fine windows and
    sub-pixel refinement — is a call into libpope_hip.so (pope_amd/loftr.py, conv.hip / loftr.hip / match.hip / fine.hip);
    only the position code (a cached table) and tensor views are torch."""

    def __init__(self, config):
        super().__init__()
        from . import loftr
        self.config = config
        self.backbone = loftr.build_backbone(config)
        self.pos_encoding = loftr.PositionEncodingSine(config["coarse"]["d_model"],
                                                       temp_bug_fix=config["coarse"]["temp_bug_fix"])
        self.loftr_coarse = loftr.LocalFeatureTransformer(config["coarse"])
        self.coarse_matching = CoarseMatching(config["match_coarse"])
        self.fine_preprocess = loftr.FinePreprocess(config)
        self.loftr_fine = loftr.LocalFeatureTransformer(config["fine"])
        self.fine_matching = loftr.FineMatching()
        # use_graph = True: the shape-static front of the forward pass (CNN, position code, coarse transformer: ~250 kernel
        # launches at the drivers' batch of three pairs) is replayed from a captured HIP graph from the third call with
        # the same input shapes on.  Same kernels, same order: bit-identical to the eager launches (tests/test_gpu_loftr.py).
        # Off by default because it buys nothing on this path: measured 4.23 -> 4.22 ms per 3-pair call, 17.32 -> 17.27 ms at
        # 24 pairs, driver step 7.34 -> 7.16 ms (scripts/loftr_time.py) — the C-side launch loops already keep the GPU fed,
        # the time is the small-grid kernels themselves.  A call with padding masks (data['mask0'/'mask1'])
        # always runs eagerly: the masks are inputs the captured graph does not have.
        self.use_graph = False
        self._graphs, self._gsrc = {}, None
        self._moves, self._rsrc = 0, None   # ReferenceEncoding keys: .to() count, parameter / buffer slots

    def _features(self, im0, im1, mask_c0=None, mask_c1=None):
        """matcher.py:46-60: (feat_c0, feat_c1) after the coarse transformer [n, L, 256] and the fine maps (feat_f0, feat_f1);
        mask_c0 [n, L] / mask_c1 [n, S]: the coarse transformer's padding masks (:62-65)."""
        n = im0.size(0)
        if im0.shape[2:] == im1.shape[2:]:  # one CNN launch sequence for both images (matcher.py:46-48)
            feats_c, feats_f = self.backbone(torch.cat([im0, im1], 0))
            (feat_c0, feat_c1), (feat_f0, feat_f1) = feats_c.split(n), feats_f.split(n)
        else:
            (feat_c0, feat_f0), (feat_c1, feat_f1) = self.backbone(im0), self.backbone(im1)
        hw_c = (feat_c0.shape[2:], feat_c1.shape[2:])
        feat_c0 = self.pos_encoding(feat_c0).flatten(2).transpose(1, 2)   # 'n c h w -> n (h w) c'
        feat_c1 = self.pos_encoding(feat_c1).flatten(2).transpose(1, 2)
        feat_c0, feat_c1 = self.loftr_coarse(feat_c0, feat_c1, mask_c0, mask_c1)
        return feat_c0, feat_c1, feat_f0, feat_f1, hw_c

    def _features_graphed(self, im0, im1):
        """`_features` through a HIP graph per (shapes, device): call 1 runs eagerly (builds every weight cache, checks
        the range flags), call 2 captures, later calls copy the inputs into the graph's static buffers and replay.
        The f16x3 range flags of the captured launches are read after the replay (one synchronisation, where the eager
        path has two); a raised flag retires the graph and the eager path — with its warnings and fp32 re-runs — takes over."""
        from . import loftr
        # (full attention: always eager — its front end is not captured)
        if not (self.use_graph and self.loftr_coarse.attention == "linear" and im0.size(0) > 0
                and im0.dtype == torch.float32 and im1.dtype == torch.float32 and not torch.cuda.is_current_stream_capturing()):
            return self._features(im0, im1)
        # a captured graph has the device pointers of the weight planes / folded BatchNorm matrices baked in, and any edit of
        # a parameter or buffer makes the eager path rebuild (and free) them: the key carries every tensor's address and
        # in-place version, so a stale graph is simply never looked up again
        if self._gsrc is None:
            self._gsrc = _lib.param_slots(self, buffers=True)
        key = (tuple(im0.shape), tuple(im1.shape), im0.device.index, _lib.slots_key(self._gsrc), self.backbone.precision)
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= 16:   # every graph owns its workspaces: keep the set small
                self._graphs.clear()
            self._graphs[key] = {}
            return self._features(im0, im1)
        if ent.get("retired"):
            return self._features(im0, im1)
        if "graph" not in ent:
            s0, s1 = im0.clone(), im1.clone()
            graph = torch.cuda.CUDAGraph()
            loftr.DEFERRED_FLAGS = []
            try:
                with torch.cuda.graph(graph):
                    outs = self._features(s0, s1)
                flags = loftr.DEFERRED_FLAGS
            except Exception:   # noqa: BLE001 — a capture the runtime refuses is not an error of the forward pass
                ent["retired"] = True
                loftr.DEFERRED_FLAGS = None
                torch.cuda.synchronize(im0.device)
                return self._features(im0, im1)
            finally:
                loftr.DEFERRED_FLAGS = None
            ent.update(graph=graph, s0=s0, s1=s1, outs=outs, flags=flags)
        ent["s0"].copy_(im0)
        ent["s1"].copy_(im1)
        ent["graph"].replay()
        if ent["flags"] and int(torch.stack(ent["flags"]).max()):
            ent["retired"] = True
            return self._features(im0, im1)
        return ent["outs"]

    def _apply(self, fn, *a, **k):
        self._graphs, self._gsrc = {}, None
        self._moves, self._rsrc = self._moves + 1, None   # every ReferenceEncoding re-encodes itself on its next use
        return super()._apply(fn, *a, **k)

    # ---- one reference image, many crops ("Reference encodings") ----
    def _ref_slots(self):
        if self._rsrc is None:
            self._rsrc = _lib.param_slots(self, buffers=True)
        return self._rsrc

    @torch.no_grad()
    def encode_reference(self, image0):
        """image0 [R, 1, H0, W0] fp32 gray in [0, 1] on the matcher's device (H0, W0 multiples of 8, >= 16) -> `ReferenceEncoding`
        for `matcher({"reference": ref, "image0_index": idx, "image1": crops})`: pair b matches reference row idx[b] against
        crops[b], every published key bit for bit that of the plain call with image0 = image0.index_select(0, idx).  The
        backbone, the position code and the leading 'self' layers of the coarse transformer run here, once per reference."""
        ref = ReferenceEncoding(self, image0)
        self._reference_backbone(ref)   # built now, in the mode a call will read it in
        return ref

    def _reference_backbone(self, ref):
        """The backbone mode a call reads `ref` in, by `ResNetFPN_8_2.forward`'s rules for the reference images alone (the
        backbone's `precision`; weights outside the f16 range, or a raised flag: fp32), and its bits.  The leading 'self' layers
        are built with it."""
        ref._fresh()
        bb = self.backbone
        bits = 0
        if bb._weights(bb.precision) is None:
            mode = "f32"
        else:
            bits = ref.backbone(bb.precision)["bits"]
            mode = "f32" if bits else bb.precision
        ref.mode = mode
        if all(l._weights("f16x3") is not None for l in self.loftr_coarse.layers):
            if ref.leading(mode, "f16x3")[1]:
                ref.leading(mode, "f32")
        else:
            ref.leading(mode, "f32")
        return mode, bits

    def _forward_indexed(self, data, only_att_fea):
        """`forward` for data['reference'] (or data['image0'] [R, ...]) + data['image0_index']: stream 0 comes from R reference
        rows, each encoded once.  Stage by stage this makes the decisions the plain call makes on the expanded batch: where the
        plain call runs both images through one launch sequence (equal sizes) one range policy covers both, and the reference's
        bits count; otherwise each side keeps its own."""
        loftr = _loftr()
        if "reference" in data and "image0" in data:
            raise ValueError("Matcher: give data['reference'] or data['image0'], not both")
        if "reference" not in data and "image0" not in data:
            raise ValueError("Matcher: data['image0_index'] needs data['image0'] or data['reference']")
        if "mask0" in data or "mask1" in data:   # before the device check: no stage has run
            raise NotImplementedError("pope_amd: padding masks (data['mask0'] / data['mask1']) are not supported together with "
                                      "data['reference'] / data['image0_index']: expand image0 and make the plain call")
        ref, im1 = data.get("reference"), data["image1"]
        if ref is not None and not (isinstance(ref, ReferenceEncoding) and ref._matcher is self):
            raise ValueError("Matcher: data['reference'] is a ReferenceEncoding of this matcher (matcher.encode_reference)")
        n = int(im1.shape[0])
        R = ref.R if ref is not None else int(data["image0"].shape[0])
        index = _image0_index(data.get("image0_index"), n, R)
        require_cuda(im1, "Matcher")
        if ref is None:
            require_cuda(data["image0"], "Matcher")
        for k in ("scale0", "scale1"):
            if k in data:
                _lib.pair_scale(data[k], n, im1.device, f"Matcher {k}")
        bb = self.backbone
        policy = bb.on_overflow or loftr.ON_OVERFLOW
        x1 = bb.checked_input(im1)
        fast = bb.precision   # "f16x3" | "f16": the reference images and the crops of one call are read in one mode
        fits = bb._weights(fast) is not None
        if not fits and policy == "raise":
            raise PopeRangeError("pope_amd: a folded LoFTR backbone filter is outside the f16x3 weight range (|w| < 255.9)")
        crops = None
        if ref is None:
            ref = ReferenceEncoding(self, data["image0"])
            if ref.hw_i == x1.shape[2:]:   # the encoding is built inside the call: one launch sequence for R + n images
                both = torch.cat([ref.image, x1], 0)
                mode = fast if fits else "f32"
                maps, flag = bb._run(both, mode)
                if fits:
                    bits = loftr._read_flags([flag])
                    if bits:
                        loftr._overflow("LoFTR backbone", bits, policy)
                        mode = "f32"
                        maps, _ = bb._run(both, mode)
                ref._put_backbone(mode, [t[:R] for t in maps], 0)
                ref.mode = mode
                crops = [t[R:] for t in maps]
        same = ref.hw_i == x1.shape[2:]
        if crops is None:
            mode, rbits = self._reference_backbone(ref)
            if same and mode == fast:
                crops, flag = bb._run(x1, fast)
                cbits = loftr._read_flags([flag])
                if cbits:
                    loftr._overflow("LoFTR backbone", cbits, policy)
                    mode = "f32"
                    crops = bb._run(x1, "f32")[0]
            elif same:   # the reference is fp32 (its flag, or the weights): the plain call runs both images in fp32
                if rbits:
                    loftr._overflow("LoFTR backbone", rbits, policy)
                crops = bb._run(x1, "f32")[0]
            else:        # two launch sequences in the plain call: each image's own guard
                if rbits:
                    loftr._overflow("LoFTR backbone", rbits, policy)
                crops = bb(x1)
        rform = ref.backbone(mode)
        feat_c1, feat_f1 = crops
        feat_f0 = rform["fine"]
        hw0_c, hw1_c = rform["hw_c"], feat_c1.shape[2:]
        data.update({"bs": n, "hw0_i": ref.hw_i, "hw1_i": im1.shape[2:]})
        feat_c1 = self.pos_encoding(feat_c1).flatten(2).transpose(1, 2)
        dev_index = index.to(x1.device)
        feat_c0, feat_c1 = self.loftr_coarse.forward_indexed(lambda precision: ref.leading(mode, precision), feat_c1, dev_index)
        data.update({"hw0_c": hw0_c, "hw1_c": hw1_c, "hw0_f": feat_f0.shape[2:], "hw1_f": feat_f1.shape[2:]})
        if only_att_fea:
            return feat_c0.clone(), feat_c1.clone()
        self.coarse_matching(feat_c0, feat_c1, data)
        win0, win1 = self.fine_preprocess(feat_f0, feat_f1, feat_c0, feat_c1, data, ref0_of_pair=dev_index)
        if win0.size(0) != 0:
            win0, win1 = self.loftr_fine(win0, win1)
        self.fine_matching(win0, win1, data)

    @torch.no_grad()
    def forward(self, data, only_att_fea=False):
        if "reference" in data or "image0_index" in data:   # shared references: always eager (no graph is captured for them)
            return self._forward_indexed(data, only_att_fea)
        im0, im1 = data["image0"], data["image1"]
        if "mask0" in data and self.loftr_coarse.attention == "full":   # before the device check: no stage has run
            from . import loftr
            raise NotImplementedError(loftr.FULL_MASK_MSG)
        require_cuda(im0, "Matcher")
        require_cuda(im1, "Matcher")
        n = im0.size(0)
        mask_c0 = mask_c1 = None
        if "mask0" in data:   # matcher.py:62-65: coarse-grid padding masks [n, H/8, W/8]; mask0 without mask1 is a KeyError there too
            hc0, hc1 = (n, im0.shape[2] // 8, im0.shape[3] // 8), (n, im1.shape[2] // 8, im1.shape[3] // 8)
            mask_c0 = _lib.padding_mask(data["mask0"], hc0, im0.device, "Matcher mask0").flatten(-2)
            mask_c1 = _lib.padding_mask(data["mask1"], hc1, im0.device, "Matcher mask1").flatten(-2)
        for k in ("scale0", "scale1"):
            if k in data:
                _lib.pair_scale(data[k], n, im0.device, f"Matcher {k}")
        data.update({"bs": n, "hw0_i": im0.shape[2:], "hw1_i": im1.shape[2:]})
        if mask_c0 is not None:   # eager: the graphs are captured without masks
            feat_c0, feat_c1, feat_f0, feat_f1, (hw0_c, hw1_c) = self._features(im0, im1, mask_c0, mask_c1)
        else:
            feat_c0, feat_c1, feat_f0, feat_f1, (hw0_c, hw1_c) = self._features_graphed(im0, im1)
        data.update({"hw0_c": hw0_c, "hw1_c": hw1_c, "hw0_f": feat_f0.shape[2:], "hw1_f": feat_f1.shape[2:]})
        if only_att_fea:   # the caller keeps these: never hand out a graph's static buffers
            return feat_c0.clone(), feat_c1.clone()
        self.coarse_matching(feat_c0, feat_c1, data, mask_c0=mask_c0, mask_c1=mask_c1)
        win0, win1 = self.fine_preprocess(feat_f0, feat_f1, feat_c0, feat_c1, data)
        if win0.size(0) != 0:
            win0, win1 = self.loftr_fine(win0, win1)
        self.fine_matching(win0, win1, data)

    def load_state_dict(self, state_dict, *args, **kwargs):
        # src/matcher/matcher.py:81-85: the keys are renamed IN THE CALLER'S dict (observable afterwards)
        for old in [k for k in state_dict if k.startswith("matcher.")]:
            state_dict[old[len("matcher."):]] = state_dict.pop(old)
        out = super().load_state_dict(state_dict, *args, **kwargs)
        # parameters were overwritten in place, or (assign=True) replaced: the derived caches (folded BatchNorm, weight
        # planes) and the graph keys notice by themselves — they look the tensors up through their slots on every call and
        # key on address + version (_lib.slots_key); the old graphs would only sit on their workspaces
        self._graphs = {}
        return out
