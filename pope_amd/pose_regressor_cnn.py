"""The fork's image pose head, `pose/model_cnn.py:Mkpts_Reg_Model`, on HIP: an image pair -> (pred_trans [3], pred_rot [3, 3]).

The pair is concatenated on the width, read by a ConvNeXtV2 backbone with a 32-wide head (`pope_amd.convnextv2`), and the two
Linears `translation_head_rot` / `rotation_head_rot` with `convert2matrix` run in one small kernel that shares the key-point
regressor's conversion code (rot_convert.h).  State-dict keys as in the reference: `convnextv2.model.*`,
`translation_head_rot.*`, `rotation_head_rot.*`.  Unlike the reference constructor, which insists on
`weights/convnextv2_large_22k_384_ema.pt`, this one reads no file: weights come through `load_state_dict`
(`convnextv2.remap_checkpoint_keys` maps an FCMAE checkpoint).  `model_type` picks the backbone ('large' is the reference's).
Inference only, no torch fallback; every pair of a call is computed on its own.
"""
import ctypes as C

import torch
from torch import nn

from . import _lib, convnextv2
from ._lib import check, on_device_of, require_cuda, stream_of
from .pose_regressor import MODES

MODEL_TYPES = {"atto": "convnextv2_atto", "femto": "convnextv2_femto", "pico": "convnext_pico", "nano": "convnextv2_nano",
               "tiny": "convnextv2_tiny", "base": "convnextv2_base", "large": "convnextv2_large", "huge": "convnextv2_huge"}


class ConvNeXtV2(nn.Module):
    """pose/model_cnn.py:11-128 without the checkpoint file: the backbone sits under `.model`."""

    def __init__(self, num_classes, model_type="large", model=None, precision="f16x3"):
        super().__init__()
        self.model = model if model is not None else convnextv2.FACTORIES[MODEL_TYPES[model_type]](num_classes=num_classes, precision=precision)

    def forward(self, x):
        return self.model(x)


class Mkpts_Reg_Model(nn.Module):
    def __init__(self, num_sample: int, mode: str = "6d", model_type: str = "large", backbone=None, precision="f16x3"):
        """`backbone`: a ready `convnextv2.ConvNeXtV2` with num_classes = 32 (tests: a small trunk) instead of `model_type`."""
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if backbone is None and model_type not in MODEL_TYPES:
            raise ValueError(f"model_type must be one of {sorted(MODEL_TYPES)}")
        self.num_sample, self.mode, self.inner_size = int(num_sample), mode, 32
        if backbone is not None and backbone.num_classes != self.inner_size:
            raise ValueError("the backbone's head must be 32 wide")
        self.convnextv2 = ConvNeXtV2(self.inner_size, model_type, backbone, precision)
        self.translation_head_rot = nn.Linear(self.inner_size, 3)
        self.rotation_head_rot = nn.Linear(self.inner_size, MODES[mode][1])
        self.eval()

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("Mkpts_Reg_Model runs inference only: keep it in eval()")
        return super().train(False)

    @torch.no_grad()
    def forward(self, batch_mkpts0, batch_mkpts1, batch_img0, batch_img1):
        """[B, 3, H, W] x 2 -> (pred_trans [B, 3], pred_rot [B, 3, 3]).  The key points are ignored, as in the reference."""
        who = "Mkpts_Reg_Model.forward"
        if self.training:
            raise NotImplementedError("Mkpts_Reg_Model runs inference only")
        for t in (batch_img0, batch_img1):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who} expects torch tensors")
            require_cuda(t, who)
        if batch_img0.dim() != 4 or batch_img0.shape != batch_img1.shape:
            raise ValueError(f"{who}: batch_img0 / batch_img1 must both be [B, 3, H, W]")
        x = self.convnextv2(torch.cat((batch_img0, batch_img1), dim=-1))
        B, dev = x.shape[0], x.device
        t = torch.empty(B, 3, dtype=torch.float32, device=dev)
        R = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
        if B == 0:
            return t, R
        keep = []
        p = lambda v: _lib.param_ptr(v, keep, who)  # noqa: E731
        with on_device_of(x):
            check(_lib.lib().pope_convnext_pose_heads_f32(
                _lib.ptr(x), p(self.translation_head_rot.weight), p(self.translation_head_rot.bias), p(self.rotation_head_rot.weight),
                p(self.rotation_head_rot.bias), MODES[self.mode][0], B, self.inner_size, C.c_void_p(t.data_ptr()), C.c_void_p(R.data_ptr()),
                stream_of(dev)), "pope_convnext_pose_heads_f32")
        return t, R
