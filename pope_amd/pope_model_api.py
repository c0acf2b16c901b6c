"""Hot-path subset of the reference façade `pope_model_api.py` (star-imported by the drivers,
eval_linemod_json.py:1).  Exports, under the reference's names, everything of that namespace that
lies on the accelerated path, including the caller-side geometry either side of it: the proposal crops
and their intrinsics (`get_image_crop_resize`, `get_K_crop_resize`; batched: `crop_proposals`) and the pose solver
(`estimate_pose`, `relative_pose_error`; batched: `estimate_pose_batch`), the fork's learned pose head (`Mkpts_Reg_Model`
of `pose/model.py`; batched from the matcher's buffers: `regress_pose_batch`), the image pose head of `pose/model_cnn.py` with its
ConvNeXtV2 backbone (`Mkpts_Reg_Model_CNN` = `pose_regressor_cnn.Mkpts_Reg_Model`, `ConvNeXtV2`, the `convnextv2_*` factories), the
fusion model of `pose/model0604.py` (`MoCoPE`; batched: `regress_pose_fused_batch`) and the image pair both image heads read
(`pose_images`), the SAM proposal generator the drivers build from it
(`sam_model_registry`, the `build_sam_vit_*` builders, `SamPredictor`, `SamAutomaticMaskGenerator`, `get_model_info`) and the
call that joins the two: `locate_pose_from_frames` / `locate_pose_from_frame`, reference crop and raw frame in, pose out
(`locate_poses_in_frame`: several references asked of one frame; `SharedFrames`: frames that several queries name;
`share_frames` groups a list of queries by frame; `regress_pose_from_frames`: the same call with a learned pose head in it).  Names
that belong to out-of-scope stages (dataset helpers) are not re-implemented here — the reference's own modules keep providing them.

Unlike the reference façade, importing this module has no side effects (the reference builds the
LoFTR `matcher` singleton from weights/matcher.pth at import, pope_model_api.py:177-185).
"""
import json  # noqa: F401  (re-exported like the reference does)
import os  # noqa: F401
import time  # noqa: F401

import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn.functional as F  # noqa: F401

from .crops import crop_proposals, expand_box, get_affine_transform, get_image_crop_resize, get_K_crop_resize  # noqa: F401
from .dinov2_utils import get_cls_token_torch, load_dinov2_model, set_torch_image  # noqa: F401
from .driver import (ReferenceSet, SharedFrames, encode_references, locate_and_match, locate_and_match_batch,  # noqa: F401
                     locate_and_match_batch_u8, locate_match_pose_batch_u8, locate_match_pose_u8, locate_pose_from_frame,
                     locate_pose_from_frames, locate_poses_in_frame, regress_pose_from_frames, share_frames)
from .matcher import CoarseMatching, Matcher, ReferenceEncoding, default_cfg, dense_match  # noqa: F401
from .ops import cls_cosine, slot_tally, streaming_top3, vote_top3_batch, vote_top3_shared  # noqa: F401
from .pipeline import PairPipeline, gather_counts, shard_range  # noqa: F401
from .pose import estimate_pose, estimate_pose_batch, relative_pose_error  # noqa: F401
from .pose_regressor import Mkpts_Reg_Model, reference_sample_indices, regress_pose_batch  # noqa: F401
from . import pose_regressor_cnn  # noqa: F401  (pose/model_cnn.py: its Mkpts_Reg_Model shares the key-point model's name)
from .convnextv2 import (ConvNeXtV2, convnext_pico, convnextv2_atto, convnextv2_base, convnextv2_femto, convnextv2_huge,  # noqa: F401
                         convnextv2_large, convnextv2_nano, convnextv2_tiny, remap_checkpoint_keys)
from .pose_regressor_cnn import Mkpts_Reg_Model as Mkpts_Reg_Model_CNN  # noqa: F401
from .mocope import MoCoPE, regress_pose_fused_batch  # noqa: F401
from .preprocess import pose_images  # noqa: F401
from .sam_generator import (SamAutomaticMaskGenerator, SamPredictor, build_sam, build_sam_vit_b, build_sam_vit_h,  # noqa: F401
                            build_sam_vit_l, sam_model_registry)


def get_model_info(type="b"):
    """(checkpoint path, `sam_model_registry` key) of the SAM size "b", "l" or "h", as the reference façade names them
    (pope_model_api.py:109-121)."""
    info = {"b": ("weights/sam_vit_b_01ec64.pth", "vit_b"), "l": ("weights/sam_vit_l_0b3195.pth", "vit_l"),
            "h": ("weights/sam_vit_h_4b8939.pth", "vit_h")}
    if not isinstance(type, str) or type not in info:
        raise NotImplementedError
    return info[type]


def build_matcher(weights="weights/matcher.pth", device="cuda:0", state_dict=None):
    """The module-level `matcher` singleton of the reference façade (pope_model_api.py:177-185: Matcher(default_cfg),
    `torch.load("weights/matcher.pth")['state_dict']` loaded with strict=False, .eval(), moved to a GPU) as an
    explicit call; `state_dict` overrides the file (synthetic weights in tests)."""
    matcher = Matcher(default_cfg)
    if state_dict is None:
        state_dict = torch.load(weights, map_location="cpu")["state_dict"]
    matcher.load_state_dict(state_dict, strict=False)
    return matcher.eval().to(device)


def vote_top3(model, ref_tensor, crop_tensors):
    """Hot loop #1 of the drivers (eval_linemod_json.py:65,74-101) batched: CLS token of the reference
    crop vs P proposal crops -> cosine scores -> streaming top-3 slots (same slot order as the
    reference's sequential loop).  Returns (scores[P] (cuda), slot_scores[3], slot_index[3])."""
    ref = get_cls_token_torch(model, ref_tensor)
    fea = get_cls_token_torch(model, crop_tensors)
    scores = cls_cosine(ref, fea, eps=1e-8)
    slots, idx = streaming_top3(scores.cpu().numpy())
    return scores, slots, idx
