"""The fork's fusion pose model, `pose/model0604.py:MoCoPE`, on HIP (mocope.hip): matched key points AND the image pair ->
(pred_trans [3], pred_rot [3, 3]).  Inference only, no torch fallback.

`MoCoPE(num_sample, mode, cnn_model_type, train_type)` keeps the reference constructor, its state-dict keys
(`transformer_mkpts.*`, `mlp1.*`, `convnextv2.model.*`, `mlp_img.*`, `mkpts_as_q.*`, `cnn_as_q.*`, `mlp2.*`, `translation_head.*`,
`rotation_head.*`: a reference state dict loads with strict=True) and the semantics of its forward.  The three
`nn.Transformer(nhead=1)` are built with batch_first=False, so [B, S, 76] and [B, 2, 512] are read with the B pairs of a call as
the SEQUENCE: attention runs across the pairs of a call (per sample slot, and per image slot in the fusion), and pair b's
result depends on the other pairs.  That is kept on purpose, as in `pose_regressor.Mkpts_Reg_Model`; `regress_pose_fused_batch`
runs every pair on its own (groups of one), the notebooks' `unsqueeze(0)`.

Unlike the reference constructor, which insists on a ConvNeXtV2 checkpoint file, this one reads none: `backbone=` takes a ready
`pope_amd.convnextv2.ConvNeXtV2` with 1000 classes, else `cnn_model_type` picks a factory.  The backbone runs in its own
`precision` ('f16x3' or 'f32'); everything after its logits is fp32.  The two image sets go through the backbone in two calls,
as in the reference, so an image's logits do not depend on how the sets are batched together.
"""
import ctypes as C
import warnings

import torch
from torch import nn

from . import _lib
from ._lib import check, on_device_of, require_cuda, stream_of
from .pose_regressor import MAX_GROUP, MODES, compact_inputs
from .pose_regressor_cnn import MODEL_TYPES, ConvNeXtV2

TRAIN_TYPES = {"mkpts+cnn": 0, "mkpts": 1, "cnn": 2}       # POPE_MOCOPE_*
# POPE_MOCOPE_TAP_*: stage -> (code, shape of the tap as a function of (B, S))
STAGES = {"embedding": (0, lambda B, S: (B, S, 76)), "memory": (1, lambda B, S: (B, S, 76)), "transformer_mkpts": (2, lambda B, S: (B, S, 76)),
          "x_mkpts": (3, lambda B, S: (B, 2, 512)), "x_img": (4, lambda B, S: (B, 2, 512)), "qmkpts": (5, lambda B, S: (B, 2, 512)),
          "qimg": (6, lambda B, S: (B, 2, 512))}
NUM_CLASSES = 1000


def _mlp(widths, drops):
    layers = []
    for i, p in enumerate(drops):
        layers += [nn.Linear(widths[i], widths[i + 1]), nn.LeakyReLU(), nn.Dropout(p=p)]
    return nn.Sequential(*layers)


class MoCoPE(nn.Module):
    """pose/model0604.py:155-300.  The torch submodules only hold the parameters under the reference's names; forward runs on HIP."""

    def __init__(self, num_sample: int, mode: str = "6d", cnn_model_type: str = "base", train_type: str = "mkpts+cnn", backbone=None,
                 precision="f16x3"):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if train_type not in TRAIN_TYPES:
            raise ValueError(f"train_type must be one of {sorted(TRAIN_TYPES)}")
        if backbone is None and cnn_model_type not in MODEL_TYPES:
            raise ValueError(f"cnn_model_type must be one of {sorted(MODEL_TYPES)}")
        if backbone is not None and backbone.num_classes != NUM_CLASSES:
            raise ValueError("the backbone's head must be 1000 wide")
        self.num_sample, self.mode, self.train_type, self.cnn_model_type = int(num_sample), mode, train_type, cnn_model_type
        self.pts_size, self.N_freqs, self.inner_size = 2, 9, 32
        d, S = 2 * self.pts_size * (2 * self.N_freqs + 1), self.num_sample
        with warnings.catch_warnings():      # torch remarks that batch_first=False rules out its nested-tensor path
            warnings.simplefilter("ignore", UserWarning)
            self.transformer_mkpts = nn.Transformer(d_model=d, nhead=1)
            self.mlp1 = _mlp([d * S, d // 2 * S, 1024], [0.5, 0.2])
            self.convnextv2 = ConvNeXtV2(NUM_CLASSES, cnn_model_type, backbone, precision)
            self.mlp_img = _mlp([NUM_CLASSES, 512], [0.2])
            self.mkpts_as_q = nn.Transformer(d_model=512, nhead=1)
            self.cnn_as_q = nn.Transformer(d_model=512, nhead=1)
        self.mlp2 = _mlp([2048, 1024, 512, 256, 128, 64, self.inner_size, self.inner_size], [0.5, 0.2, 0.2, 0.1, 0.1, 0.1, 0.1])
        self.translation_head = nn.Linear(self.inner_size, 3)
        self.rotation_head = nn.Linear(self.inner_size, MODES[mode][1])
        self.eval()
        self._ws = None
        self._slots = None
        self._backbone_slots = None
        self._struct = None      # (key, struct, keep)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("MoCoPE runs inference only (dropout is not implemented): keep it in eval()")
        return super().train(False)

    def _weights(self):
        if self._slots is None:      # the backbone keeps its own derived data
            self._slots = [s for m in self.children() if m is not self.convnextv2 for s in _lib.param_slots(m)]
        key = _lib.slots_key(self._slots)
        if self._struct is None or self._struct[0] != key:
            keep, w = [], _lib.MocopeWeights()
            p = lambda t: _lib.param_ptr(t, keep, "MoCoPE")  # noqa: E731
            w.num_sample, w.mode = self.num_sample, MODES[self.mode][0]

            def attn(dst, prefix, a):
                for name, t in (("in_proj_w", a.in_proj_weight), ("in_proj_b", a.in_proj_bias), ("out_proj_w", a.out_proj.weight),
                                ("out_proj_b", a.out_proj.bias)):
                    setattr(dst, prefix + name, p(t))

            def rest(dst, layer, norms):
                dst.linear1_w, dst.linear1_b = p(layer.linear1.weight), p(layer.linear1.bias)
                dst.linear2_w, dst.linear2_b = p(layer.linear2.weight), p(layer.linear2.bias)
                for n in norms:
                    norm = getattr(layer, n)
                    setattr(dst, n + "_w", p(norm.weight))
                    setattr(dst, n + "_b", p(norm.bias))

            for name in ("transformer_mkpts", "mkpts_as_q", "cnn_as_q"):
                t, tw = getattr(self, name), getattr(w, name)
                for i in range(6):
                    attn(tw.enc[i], "", t.encoder.layers[i].self_attn)
                    rest(tw.enc[i], t.encoder.layers[i], ("norm1", "norm2"))
                    attn(tw.dec[i], "", t.decoder.layers[i].self_attn)
                    attn(tw.dec[i], "cross_", t.decoder.layers[i].multihead_attn)
                    rest(tw.dec[i], t.decoder.layers[i], ("norm1", "norm2", "norm3"))
                tw.enc_norm_w, tw.enc_norm_b = p(t.encoder.norm.weight), p(t.encoder.norm.bias)
                tw.dec_norm_w, tw.dec_norm_b = p(t.decoder.norm.weight), p(t.decoder.norm.bias)
            for i in range(2):
                w.mlp1_w[i], w.mlp1_b[i] = p(self.mlp1[3 * i].weight), p(self.mlp1[3 * i].bias)
            w.mlp_img_w, w.mlp_img_b = p(self.mlp_img[0].weight), p(self.mlp_img[0].bias)
            for i in range(7):
                w.mlp2_w[i], w.mlp2_b[i] = p(self.mlp2[3 * i].weight), p(self.mlp2[3 * i].bias)
            w.trans_w, w.trans_b = p(self.translation_head.weight), p(self.translation_head.bias)
            w.rot_w, w.rot_b = p(self.rotation_head.weight), p(self.rotation_head.bias)
            self._struct = (key, w, keep)
        return self._struct[1]

    def _images(self, img0, img1, B, who, feat0=None, feat1=None):
        """The backbone's logits [B, 1000] of the two image sets (None under train_type 'mkpts', which reads no image).  `feat0` /
        `feat1`: logits the caller already has (`image_logits`), each in place of its image."""
        for img, feat, n in ((img0, feat0, 0), (img1, feat1, 1)):
            if img is not None and feat is not None:
                raise ValueError(f"{who}: give img{n} or feat{n}, not both")
        if self.train_type == "mkpts":
            return None, None
        for t in (img0 if feat0 is None else feat0, img1 if feat1 is None else feat1):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who} expects torch tensors")
            require_cuda(t, who)
        for f, n in ((feat0, 0), (feat1, 1)):
            if f is not None and (f.dtype != torch.float32 or tuple(f.shape) != (B, NUM_CLASSES)):
                raise ValueError(f"{who}: feat{n} must be the backbone's fp32 logits [B, {NUM_CLASSES}] with the B of the key points")
        imgs = [t for t in (img0 if feat0 is None else None, img1 if feat1 is None else None) if t is not None]
        if any(t.dim() != 4 or t.shape[0] != B for t in imgs) or len({tuple(t.shape) for t in imgs}) > 1:
            raise ValueError(f"{who}: batch_img0 / batch_img1 must both be [B, 3, H, W] with the B of the key points")
        return (self.convnextv2(img0) if feat0 is None else feat0).contiguous(), (self.convnextv2(img1) if feat1 is None else feat1).contiguous()

    @torch.no_grad()
    def image_logits(self, img):
        """The backbone's logits [B, 1000] of [B, 3, H, W] images: what `regress_pose_fused_batch` takes as `feat0` / `feat1`.
        An image's logits do not depend on the other images of the call."""
        return self.convnextv2(img).contiguous()

    def backbone_key(self):
        """Changes whenever a tensor of the backbone is edited in place or replaced (`_lib.slots_key`): logits kept from an
        earlier `image_logits` call belong to the weights of that key."""
        if self._backbone_slots is None:
            self._backbone_slots = _lib.param_slots(self.convnextv2, buffers=True)
        return _lib.slots_key(self._backbone_slots)

    def _dense(self, k0, k1, who):
        for t in (k0, k1):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who} expects torch tensors")
        if k0.dim() != 3 or k0.shape != k1.shape or k0.shape[2] != 2 or k0.shape[1] != self.num_sample:
            raise ValueError(f"{who}: batch_mkpts0 / batch_mkpts1 must both be [B, num_sample = {self.num_sample}, 2]")
        if k0.shape[0] > MAX_GROUP:
            raise NotImplementedError(f"{who}: the B pairs of a call form one attention group; groups above {MAX_GROUP} are not implemented")
        if k0.shape[0] == 0:
            raise ValueError(f"{who}: empty batch")
        for t in (k0, k1):
            require_cuda(t, who)
            if t.dtype != torch.float32:
                raise TypeError(f"{who} expects float32 keypoints")
        return k0.contiguous(), k1.contiguous()

    @torch.no_grad()
    def forward(self, batch_mkpts0, batch_mkpts1, batch_img0, batch_img1):
        """[B, num_sample, 2] x 2, [B, 3, H, W] x 2 -> (pred_trans [B, 3], pred_rot [B, 3, 3]); the B pairs are one attention group
        (B <= 64)."""
        who = "MoCoPE.forward"
        if self.training:
            raise NotImplementedError("MoCoPE runs inference only")
        k0, k1 = self._dense(batch_mkpts0, batch_mkpts1, who)
        B = k0.shape[0]
        f0, f1 = self._images(batch_img0, batch_img1, B, who)
        out = _run(self, None, B, B, f0, f1, dense=(k0, k1))
        return out["t"], out["R"]

    @torch.no_grad()
    def taps(self, batch_mkpts0, batch_mkpts1, batch_img0, batch_img1, stage):
        """Test entry: the tensor after `stage` (one of STAGES)."""
        who = "MoCoPE.taps"
        k0, k1 = self._dense(batch_mkpts0, batch_mkpts1, who)
        B = k0.shape[0]
        f0, f1 = self._images(batch_img0, batch_img1, B, who)
        return _run(self, stage, B, B, f0, f1, dense=(k0, k1))["x"]


def _run(model, stage, B, G, feat0, feat1, dense=None, compact=None, sample_index=None, seeds=None):
    lib = _lib.lib()
    S = model.num_sample
    src = dense[0] if dense else compact[0]
    dev = src.device
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d0, d1 = (p(dense[0]), p(dense[1])) if dense else (None, None)
    k0 = k1 = counts = None
    M = 0
    if compact:
        M = int(compact[0].shape[0])
        if M:
            k0, k1 = p(compact[0]), p(compact[1])
        counts = p(compact[2])
    status = torch.empty(B, dtype=torch.int32, device=dev)
    head = (d0, d1, k0, k1, counts, p(sample_index), p(seeds), p(feat0), p(feat1), B, S, G, M, TRAIN_TYPES[model.train_type])
    with on_device_of(src):
        w = model._weights()
        ws = _lib.grow_workspace(model, lib.pope_mocope_workspace_bytes(B, S), dev)
        if stage is not None:
            code, shape = STAGES[stage]
            x = torch.empty(shape(B, S), dtype=torch.float32, device=dev)
            check(lib.pope_mocope_tap_f32(C.byref(w), *head, code, p(x), p(status), p(ws), ws.numel(), stream_of(dev)), "pope_mocope_tap_f32")
            return {"x": x, "status": status}
        t = torch.empty(B, 3, dtype=torch.float32, device=dev)
        R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
        check(lib.pope_mocope_forward_f32(C.byref(w), *head, p(t), p(R), p(status), p(ws), ws.numel(), stream_of(dev)),
              "pope_mocope_forward_f32")
    return {"R": R, "t": t, "status": status}


@torch.no_grad()
def regress_pose_fused_batch(model, kpts0, kpts1, counts, img0=None, img1=None, seed=0, sample_index=None, feat0=None, feat1=None):
    """The pipeline form: every pair on its own (attention groups of one), from the matcher's compacted device buffers
    (`pose_regressor.regress_pose_batch`: same layout, sampling, padding and status rules) plus the pairs' images
    img0 / img1 [B, 3, H, W] fp32 on the device.  Returns device tensors R [B, 3, 3], t [B, 3], status [B] int32.  The part
    after the backbone makes no host synchronisation; the backbone's f16x3 range guard reads one word per call (none with
    precision='f32').
    `feat0` / `feat1` [B, 1000]: the backbone's logits of an image set computed earlier (`MoCoPE.image_logits`), in place of that
    set: give the image or its logits, never both; the backbone then runs over the other set only.  The result is that of the
    call with the images."""
    who = "regress_pose_fused_batch"
    if not isinstance(model, MoCoPE):
        raise TypeError(f"{who} expects a pope_amd MoCoPE")
    if model.training:
        raise NotImplementedError("MoCoPE runs inference only")
    kpts0, kpts1, counts, sample_index, seeds = compact_inputs(who, model.num_sample, kpts0, kpts1, counts, seed, sample_index)
    B = int(counts.numel())
    f0, f1 = model._images(img0, img1, B, who, feat0, feat1)
    return _run(model, None, B, 1, f0, f1, compact=(kpts0, kpts1, counts), sample_index=sample_index, seeds=seeds)
