"""SAM container, predictor and automatic mask generator on the HIP library.

Drop-ins for `segment_anything.{modeling.sam.Sam, predictor.SamPredictor, automatic_mask_generator.SamAutomaticMaskGenerator}`
and `build_sam.py`, for a single crop and point / box / mask prompts.  The generator's post-processing is one fused HIP pass per decoder
call (`pope_sam_postprocess_f32`, pope_amd/csrc/sam_postprocess.hip): from the 256 x 256 low-res logits of the masks that pass
the IoU filter straight to per-mask counts, boxes, stability scores and bit-packed masks, without the 1024 x 1024 or the
frame-sized fp32 tensors of `Sam.postprocess_masks`; the logits are bit-equal to torch's CPU `F.interpolate` (pope_amd/sam_amg.py
restates the arithmetic), so counts, boxes and masks are exact.  Box NMS is `pope_sam_nms_f32`; the small-region clean-up is one
launch over the packed masks of the NMS survivors (`pope_sam_small_regions_u32`, pope_amd/csrc/sam_regions.hip).  `generate_batch` takes the
frames of several queries at once: one encoder call, the decoder per frame, then one tail for all frames (`box_nms_segments` =
`pope_sam_nms_segments_f32`, one workgroup per frame; the clean-up over all survivors; run lengths by `pope_sam_rle_u32`,
pope_amd/csrc/sam_rle.hip, so that `uncompressed_rle` downloads counts instead of masks).  `propose` / `propose_batch` are the
same calls stopped after the second NMS: the records' boxes alone, no mask unpacked, encoded or downloaded (the frame-to-pose
query of pope_amd/driver.py reads nothing else).  There is one tail: `generate` / `propose` are the batched tail with one segment.
`Sam.decode_prompts` is the prompt encoder and the mask decoder of one image, with the image's features as an argument: the
predictor calls it with the features it holds, the generator with each frame's (it never writes the predictor's state).  There
is no torch fallback.

Frames are dispatched by type alone.  A numpy array or a CPU tensor is resized by Pillow on the host, uploaded and normalised
by `Sam.preprocess`.  A uint8 CUDA tensor stays in HBM: `SamPredictor.set_image`, `generate`, `propose` ([H, W, 3]) and
`generate_batch`, `propose_batch` ([Q, H, W, 3] or a list of frames of one size) make one `pope_sam_preprocess_u8_f32` call
(pope_amd/preprocess.py:sam_preprocess_batch: Pillow's resample, the normalisation and the pad in one result, bit-equal to
the host chain), `ResizeLongestSide.apply_image` returns the resized uint8 tensor (`pope_resize_u8`).

Not supported: crop layers (`crop_n_layers > 0`), `output_mode="coco_rle"`.
"""
import ctypes as C
from functools import partial
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, sam_amg
from ._lib import check, on_device_of, params_key, ptr, require_cuda, stream_of
from .preprocess import frames_on_device, on_device, resize_u8_batch, sam_preprocess_batch
from .sam_decoder import MaskDecoder, PromptEncoder, TwoWayTransformer, require_gpu_mask
from .sam_encoder import ImageEncoderViT

NMS_MAX = 2048   # boxes per pope_sam_nms_f32 call
CLEAN_CHUNK = 32  # masks in flight in pope_sam_small_regions_u32: its workspace stops growing there


# ---- device ops ----------------------------------------------------------------------------------------------------------
def postprocess_batch(low_res, selection, input_size, original_size, mask_threshold=0.0, stability_score_offset=1.0,
                      img_size=sam_amg.IMG_SIZE, packed=True, logits=False):
    """One fused pass over low_res [M, h, w] (fp32, CUDA) for the masks listed in `selection` (int32 CUDA tensor, or None for
    all M, in order).  Returns (stats int32 [n, 8], packed int32 [n, H, ceil(W / 32)] or None, logits fp32 [n, H, W] or None);
    stats columns: n_hi, n_lo, area, x0, y0, x1, y1, stability score as fp32 bits (`stats[:, 7].view(torch.float32)`)."""
    require_cuda(low_res, "postprocess_batch")
    if low_res.dtype != torch.float32 or low_res.dim() != 3:
        raise TypeError(f"postprocess_batch: low_res must be float32 [M, h, w], got {low_res.dtype} {tuple(low_res.shape)}")
    low_res = low_res.contiguous()
    M, h, w = low_res.shape
    dev = low_res.device
    if selection is not None:
        require_cuda(selection, "postprocess_batch")
        if selection.dtype != torch.int32 or selection.dim() != 1:
            raise TypeError("postprocess_batch: selection must be an int32 vector")
        selection = selection.contiguous()
    n = M if selection is None else selection.numel()
    (ih, iw), (H, W) = (int(v) for v in input_size), (int(v) for v in original_size)
    need = int(_lib.lib().pope_sam_postprocess_workspace_bytes(img_size, H, W))
    if need <= 0 or not (0 < ih <= img_size and 0 < iw <= img_size):
        raise ValueError(f"postprocess_batch: unsupported geometry (input {ih} x {iw} in {img_size}, frame {H} x {W})")
    stats = torch.empty(n, 8, dtype=torch.int32, device=dev)
    bits = torch.empty(n, H, sam_amg.row_words(W), dtype=torch.int32, device=dev) if packed else None
    dense = torch.empty(n, H, W, dtype=torch.float32, device=dev) if logits else None
    if n == 0 or M == 0:
        return stats, bits, dense
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with on_device_of(low_res):
        check(_lib.lib().pope_sam_postprocess_f32(
            ptr(low_res), M, h, w, ptr(selection), n, img_size, ih, iw, H, W, float(mask_threshold), float(stability_score_offset),
            ptr(stats), ptr(bits), ptr(dense), ptr(ws), ws.numel(), stream_of(dev)), "pope_sam_postprocess_f32")
    return stats, bits, dense


def _nms_args(boxes, scores, who):
    """The arguments of both NMS bindings: (boxes and scores as contiguous fp32 on the boxes' device, an int32 keep buffer)."""
    require_cuda(boxes, who)
    dev = boxes.device
    return (boxes.to(torch.float32).contiguous(), scores.to(device=dev, dtype=torch.float32).contiguous(),
            torch.empty(max(boxes.shape[0], 1), dtype=torch.int32, device=dev))


def _packed_words(packed, W, who):
    """The bit-packed masks of `who`, checked and contiguous: int32 words [n, H, ceil(W / 32)] on a GPU."""
    require_cuda(packed, who)
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != sam_amg.row_words(W):
        raise TypeError(f"{who}: expected int32 words [n, H, {sam_amg.row_words(W)}] for W = {W}, "
                        f"got {packed.dtype} {tuple(packed.shape)}")
    return packed.contiguous()


def box_nms(boxes, scores, iou_threshold):
    """Greedy box NMS on the device (`pope_sam_nms_f32`): `torchvision.ops.batched_nms` with one category restated from its
    definition (torchvision is not a dependency, so it is not pinned against the library itself; `sam_amg.nms` is the same
    definition on the CPU).  boxes [n, 4] XYXY, scores [n]; returns the kept indices in score order (int64, on the device)."""
    boxes, scores, keep = _nms_args(boxes, scores, "box_nms")
    n, dev = boxes.shape[0], boxes.device
    if n > NMS_MAX:
        raise ValueError(f"box_nms: at most {NMS_MAX} boxes per call, got {n}")
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    with on_device_of(boxes):
        check(_lib.lib().pope_sam_nms_f32(ptr(boxes), ptr(scores), n, float(iou_threshold), ptr(keep), ptr(count), stream_of(dev)),
              "pope_sam_nms_f32")
    return keep[:int(count.item())].to(torch.int64)


def box_nms_segments(boxes, scores, seg_offsets, iou_threshold):
    """`box_nms` of S independent segments in one launch (`pope_sam_nms_segments_f32`, one workgroup per segment, the device
    function of `pope_sam_nms_f32`).  boxes [n, 4], scores [n] (device); seg_offsets: S + 1 non-decreasing host integers from 0
    to n, segment s = boxes seg_offsets[s] .. seg_offsets[s + 1] - 1, at most `NMS_MAX` of them.  Returns (keep int32 [n],
    counts int32 [S]), both on the device and without a host read: the kept boxes of segment s are
    keep[seg_offsets[s] : seg_offsets[s] + counts[s]], global indices into n in score order."""
    boxes, scores, keep = _nms_args(boxes, scores, "box_nms_segments")
    n, dev = boxes.shape[0], boxes.device
    seg = np.asarray(seg_offsets.cpu() if isinstance(seg_offsets, torch.Tensor) else seg_offsets, dtype=np.int64).reshape(-1)
    if seg.size < 1 or seg[0] != 0 or seg[-1] != n or (np.diff(seg) < 0).any():
        raise ValueError(f"box_nms_segments: seg_offsets must rise from 0 to n = {n}, got {seg.tolist()}")
    if seg.size > 1 and int(np.diff(seg).max()) > NMS_MAX:
        raise ValueError(f"box_nms_segments: at most {NMS_MAX} boxes per segment, got {int(np.diff(seg).max())}")
    S = seg.size - 1
    counts = torch.zeros(S, dtype=torch.int32, device=dev)
    if S == 0:
        return keep[:n], counts
    seg_dev = torch.as_tensor(seg.astype(np.int32)).to(dev)
    with on_device_of(boxes):
        check(_lib.lib().pope_sam_nms_segments_f32(ptr(boxes), ptr(scores), ptr(seg_dev), S, n, float(iou_threshold), ptr(keep),
                                                   ptr(counts), stream_of(dev)), "pope_sam_nms_segments_f32")
    return keep[:n], counts


def rle_from_packed(packed, W):
    """`mask_to_rle_pytorch` of bit-packed masks on the device (`pope_sam_rle_u32`, pope_amd/csrc/sam_rle.hip): int32 words
    [n, H, ceil(W / 32)] -> list of {"size": [H, W], "counts": [...]}: column-major run lengths, starting with a run of zeros.
    Two calls (lengths, then counts at the scanned offsets); only the lengths and the counts are downloaded."""
    packed = _packed_words(packed, W, "rle_from_packed")
    n, H, _ = packed.shape
    if n == 0:
        return []
    dev = packed.device
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    with on_device_of(packed):
        check(_lib.lib().pope_sam_rle_u32(ptr(packed), n, H, int(W), ptr(lengths), None, None, 0, stream_of(dev)), "pope_sam_rle_u32")
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(lengths.cpu().numpy(), out=offsets[1:])
        total = int(offsets[-1])
        counts = torch.empty(total, dtype=torch.int32, device=dev)
        offsets_dev = torch.as_tensor(offsets).to(dev)
        check(_lib.lib().pope_sam_rle_u32(ptr(packed), n, H, int(W), None, ptr(offsets_dev), ptr(counts), total, stream_of(dev)),
              "pope_sam_rle_u32")
    counts = counts.cpu().numpy()
    return [{"size": [H, int(W)], "counts": counts[offsets[i]:offsets[i + 1]].tolist()} for i in range(n)]


# ---- Sam -----------------------------------------------------------------------------------------------------------------
class Sam(nn.Module):
    """modeling/sam.py: the container a `Sam` checkpoint loads into with strict=True (`pixel_mean` / `pixel_std` are
    non-persistent buffers, as in the reference)."""
    mask_threshold: float = 0.0
    image_format: str = "RGB"

    def __init__(self, image_encoder: ImageEncoderViT, prompt_encoder: PromptEncoder, mask_decoder: MaskDecoder,
                 pixel_mean: List[float] = [123.675, 116.28, 103.53], pixel_std: List[float] = [58.395, 57.12, 57.375]) -> None:
        super().__init__()
        self.image_encoder = image_encoder
        self.prompt_encoder = prompt_encoder
        self.mask_decoder = mask_decoder
        self.register_buffer("pixel_mean", torch.Tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.Tensor(pixel_std).view(-1, 1, 1), False)

    @property
    def device(self) -> Any:
        return self.pixel_mean.device

    @torch.no_grad()
    def forward(self, batched_input: List[Dict[str, Any]], multimask_output: bool) -> List[Dict[str, torch.Tensor]]:
        """modeling/sam.py:53-131, the end-to-end batch call.  One record per image: `image` (3 x h x w, already resized to
        the model's input frame, long side `img_size`), `original_size` (H, W) and the optional prompts `point_coords`
        [B, n, 2] + `point_labels` [B, n] and `boxes` [B, 4], in the input frame, and `mask_inputs` (float32 [B, 1, 256, 256]
        logits, e.g. an earlier call's `low_res_logits` of one mask).  Returns one dict per record: `masks` (bool [B, C, H, W]),
        `iou_predictions` [B, C], `low_res_logits` [B, C, 256, 256]; C = 3 with `multimask_output`, else 1.
        The images run through the encoder in one call and the prompts of the records without a mask prompt through the
        multi-image decoder (`MaskDecoder.forward_images`, one call per distinct number of sparse embeddings); a record with
        `mask_inputs` has a dense embedding per prompt and takes the single-image decoder call.  The masks of records of one
        geometry are resampled together.  Every record's output is bit for bit what `SamPredictor.set_torch_image` +
        `predict_torch` give for that record alone."""
        records = list(batched_input)
        if not records:
            return []
        for x in records:
            require_gpu_mask(x.get("mask_inputs", None), "Sam.forward")
        dev = self.device
        for x in records:
            for k in ("image", "point_coords", "point_labels", "boxes", "mask_inputs"):
                t = x.get(k, None)
                if t is None:
                    continue
                require_cuda(t, "Sam.forward")
                if t.device != dev:
                    raise ValueError(f"Sam.forward: record tensor `{k}` is on {t.device}, the model on {dev}")
        embeddings = self.image_encoder(torch.stack([self.preprocess(x["image"]) for x in records], dim=0).contiguous())
        pe = self.prompt_encoder.get_dense_pe()
        sparse, dense, own_dense = [], None, {}
        for r, x in enumerate(records):
            points = (x["point_coords"], x["point_labels"]) if "point_coords" in x else None
            sp, dn = self.prompt_encoder(points=points, boxes=x.get("boxes", None), masks=x.get("mask_inputs", None))
            sparse.append(sp)
            if x.get("mask_inputs", None) is not None:
                own_dense[r] = dn
            else:
                dense = dn
        low, iou = [None] * len(records), [None] * len(records)
        # a record with a mask prompt has a dense embedding per prompt: the single-image call, as `predict_torch` makes it
        for r, dn in own_dense.items():
            low[r], iou[r] = self.mask_decoder(embeddings[r:r + 1], pe, sparse[r], dn, multimask_output)
        # the others: one decoder call per number of sparse embeddings, over the images that have such prompts (one image alone
        # is the single-image call inside `forward_images`)
        for ns in sorted({sp.shape[1] for r, sp in enumerate(sparse) if r not in own_dense}):
            members = [r for r, sp in enumerate(sparse) if sp.shape[1] == ns and r not in own_dense]
            counts = [sparse[r].shape[0] for r in members]
            emb = embeddings if len(members) == len(records) else embeddings[torch.as_tensor(members, device=dev)]
            which = np.repeat(np.arange(len(members)), counts)
            m, q = self.mask_decoder.forward_images(emb, pe, torch.cat([sparse[r] for r in members]), dense[:1], which,
                                                    multimask_output)
            for r, mr, qr in zip(members, m.split(counts), q.split(counts)):
                low[r], iou[r] = mr, qr
        # postprocess_masks once per geometry
        masks = [None] * len(records)
        geometry = [(tuple(int(v) for v in x["image"].shape[-2:]), tuple(int(v) for v in x["original_size"])) for x in records]
        for geo in dict.fromkeys(geometry):
            members = [r for r, g in enumerate(geometry) if g == geo]
            up = self.postprocess_masks(torch.cat([low[r] for r in members]), *geo) > self.mask_threshold
            for r, ur in zip(members, up.split([low[r].shape[0] for r in members])):
                masks[r] = ur
        return [{"masks": masks[r], "iou_predictions": iou[r], "low_res_logits": low[r]} for r in range(len(records))]

    @torch.no_grad()
    def decode_prompts(self, features, points, boxes, mask_input, multimask_output):
        """The prompt encoder and the mask decoder for one image: features [1, 256, 64, 64], points (coords [B, n, 2], labels
        [B, n]) or None, boxes [B, 4] or None, mask_input [B, 1, 256, 256] or None -> (low_res_masks [B, C, 256, 256],
        iou_predictions [B, C]).  What `SamPredictor.predict_low_res` and the mask generator both run."""
        sparse, dense = self.prompt_encoder(points=points, boxes=boxes, masks=mask_input)
        return self.mask_decoder(image_embeddings=features, image_pe=self.prompt_encoder.get_dense_pe(),
                                 sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=multimask_output)

    def preprocess(self, x: torch.Tensor) -> torch.Tensor:
        """Normalize pixel values and pad to the square input."""
        x = (x - self.pixel_mean) / self.pixel_std
        h, w = x.shape[-2:]
        return F.pad(x, (0, self.image_encoder.img_size - w, 0, self.image_encoder.img_size - h))

    @torch.no_grad()
    def postprocess_masks(self, masks: torch.Tensor, input_size: Tuple[int, ...], original_size: Tuple[int, ...]) -> torch.Tensor:
        """[B, C, h, w] low-res logits -> [B, C, H, W] fp32 logits at the original size: the fused kernel's logit path with a
        dense store, bit-equal to the reference's two `F.interpolate` calls on the CPU."""
        B, Cm = masks.shape[:2]
        _, _, dense = postprocess_batch(masks.reshape(B * Cm, *masks.shape[2:]).float(), None, input_size, original_size,
                                        self.mask_threshold, 1.0, self.image_encoder.img_size, packed=False, logits=True)
        return dense.view(B, Cm, int(original_size[0]), int(original_size[1]))


def _build_sam(encoder_embed_dim, encoder_depth, encoder_num_heads, encoder_global_attn_indexes, checkpoint=None):
    prompt_embed_dim, image_size, vit_patch_size = 256, 1024, 16
    grid = image_size // vit_patch_size
    sam = Sam(
        image_encoder=ImageEncoderViT(depth=encoder_depth, embed_dim=encoder_embed_dim, img_size=image_size, mlp_ratio=4,
                                      norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_heads=encoder_num_heads,
                                      patch_size=vit_patch_size, qkv_bias=True, use_rel_pos=True,
                                      global_attn_indexes=encoder_global_attn_indexes, window_size=14, out_chans=prompt_embed_dim),
        prompt_encoder=PromptEncoder(embed_dim=prompt_embed_dim, image_embedding_size=(grid, grid),
                                     input_image_size=(image_size, image_size), mask_in_chans=16),
        mask_decoder=MaskDecoder(num_multimask_outputs=3,
                                 transformer=TwoWayTransformer(depth=2, embedding_dim=prompt_embed_dim, mlp_dim=2048, num_heads=8),
                                 transformer_dim=prompt_embed_dim, iou_head_depth=3, iou_head_hidden_dim=256),
        pixel_mean=[123.675, 116.28, 103.53], pixel_std=[58.395, 57.12, 57.375])
    sam.eval()
    if checkpoint is not None:
        with open(checkpoint, "rb") as f:
            sam.load_state_dict(torch.load(f))
    return sam


def build_sam_vit_h(checkpoint=None):
    return _build_sam(1280, 32, 16, [7, 15, 23, 31], checkpoint)


def build_sam_vit_l(checkpoint=None):
    return _build_sam(1024, 24, 16, [5, 11, 17, 23], checkpoint)


def build_sam_vit_b(checkpoint=None):
    return _build_sam(768, 12, 12, [2, 5, 8, 11], checkpoint)


build_sam = build_sam_vit_h
sam_model_registry = {"default": build_sam_vit_h, "vit_h": build_sam_vit_h, "vit_l": build_sam_vit_l, "vit_b": build_sam_vit_b}


# ---- predictor -----------------------------------------------------------------------------------------------------------
class ResizeLongestSide:
    """utils/transforms.py: `apply_image` is torchvision's `resize(to_pil_image(image), size)`, i.e. Pillow's 8-bit bilinear
    resample: on the host once per frame for a numpy array or a CPU tensor, `pope_resize_u8` for a uint8 CUDA tensor (the
    same bytes)."""

    def __init__(self, target_length: int) -> None:
        self.target_length = target_length

    @staticmethod
    def get_preprocess_shape(oldh: int, oldw: int, long_side_length: int) -> Tuple[int, int]:
        return sam_amg.preprocess_shape(oldh, oldw, long_side_length)

    def apply_image(self, image):
        """[H, W, 3] uint8 numpy array or CPU tensor -> the resized numpy array; a uint8 CUDA tensor [H, W, 3] or [P, H, W, 3]
        -> the resized CUDA tensor of the same rank (what a caller permutes into a `Sam.forward` record)."""
        if on_device(image):
            if image.dtype != torch.uint8 or image.dim() not in (3, 4) or image.shape[-1] != 3:
                raise TypeError(f"apply_image: a device image is a uint8 [H, W, 3] or [P, H, W, 3] tensor, got {image.dtype} "
                                f"{tuple(image.shape)}")
            stack = image if image.dim() == 4 else image[None]
            out = resize_u8_batch(stack, self.get_preprocess_shape(int(stack.shape[1]), int(stack.shape[2]), self.target_length))
            return out if image.dim() == 4 else out[0]
        from PIL import Image
        h, w = self.get_preprocess_shape(image.shape[0], image.shape[1], self.target_length)
        return np.array(Image.fromarray(np.ascontiguousarray(image)).resize((w, h), Image.BILINEAR))

    def apply_coords_torch(self, coords: torch.Tensor, original_size: Tuple[int, ...]) -> torch.Tensor:
        """`apply_coords` for a tensor [..., 2] on any device: a float32 copy, scaled (the factors are rounded to float32)."""
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(old_h, old_w, self.target_length)
        coords = coords.detach().to(torch.float, copy=True)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes_torch(self, boxes: torch.Tensor, original_size: Tuple[int, ...]) -> torch.Tensor:
        """`apply_boxes` for a tensor [B, 4] on any device."""
        return self.apply_coords_torch(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)

    def apply_coords(self, coords: np.ndarray, original_size: Tuple[int, ...]) -> np.ndarray:
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(old_h, old_w, self.target_length)
        coords = np.array(coords, copy=True).astype(float)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes(self, boxes: np.ndarray, original_size: Tuple[int, ...]) -> np.ndarray:
        return self.apply_coords(np.asarray(boxes).reshape(-1, 2, 2), original_size).reshape(-1, 4)


class SamPredictor:
    """predictor.py: `set_image` / `set_torch_image` run the image encoder once, `predict_torch` the prompt encoder, the mask
    decoder and `Sam.postprocess_masks`."""

    def __init__(self, sam_model: Sam) -> None:
        self.model = sam_model
        self.transform = ResizeLongestSide(sam_model.image_encoder.img_size)
        self._pixel_stats = (None, None, None)   # (params_key, mean, std): host copies of the model's two pixel buffers
        self.reset_image()

    @property
    def device(self) -> torch.device:
        return self.model.device

    def set_image(self, image, image_format: str = "RGB") -> None:
        """`image`: [H, W, 3] uint8, a numpy array or a CPU tensor (Pillow on the host, upload, `Sam.preprocess`) or a CUDA tensor
        on the model's device (one `pope_sam_preprocess_u8_f32` call); the state it leaves is the same, bit for bit."""
        assert image_format in ["RGB", "BGR"], f"image_format must be in ['RGB', 'BGR'], is {image_format}."
        if on_device(image):
            if image.dim() != 3:
                raise TypeError(f"set_image: a device image is a uint8 [H, W, 3] tensor, got {tuple(image.shape)}")
            x, input_size = self.preprocess_frames(frames_on_device(image[None], "set_image"), image_format, "set_image")
            self._set_encoder_input(x, input_size, image.shape[:2])
            return
        if image_format != self.model.image_format:
            image = image[..., ::-1]
        input_image = self.transform.apply_image(image)
        t = torch.as_tensor(input_image, device=self.device).permute(2, 0, 1).contiguous()[None, :, :, :]
        self.set_torch_image(t, image.shape[:2])

    @torch.no_grad()
    def preprocess_frames(self, stack, image_format: str, what: str):
        """The device form of `transform.apply_image` + `model.preprocess` for frames of one size: `stack` is what
        `preprocess.frames_on_device` returns (uint8 [Q, H, W, 3], not on the CPU) -> (the encoder's input
        [Q, 3, img_size, img_size], input_size).  Frames on another device than the model raise ValueError."""
        if stack.device != torch.device(self.device):
            raise ValueError(f"{what}: the frames are on {stack.device}, the model on {self.device}")
        model = self.model
        key = params_key((model.pixel_mean, model.pixel_std))
        if self._pixel_stats[0] != key:   # host copies of the two buffers, read once per value (a download is a synchronisation)
            self._pixel_stats = (key, model.pixel_mean.flatten().tolist(), model.pixel_std.flatten().tolist())
        return sam_preprocess_batch(stack, model.image_encoder.img_size, self._pixel_stats[1], self._pixel_stats[2],
                                    flip=image_format != model.image_format)

    @torch.no_grad()
    def set_torch_image(self, transformed_image: torch.Tensor, original_image_size: Tuple[int, ...]) -> None:
        size = self.model.image_encoder.img_size
        assert (len(transformed_image.shape) == 4 and transformed_image.shape[1] == 3
                and max(*transformed_image.shape[2:]) == size), f"set_torch_image input must be BCHW with long side {size}."
        self._set_encoder_input(self.model.preprocess(transformed_image).contiguous(), transformed_image.shape[-2:],
                                original_image_size)

    # the encoder call both `set_image` paths end in: x [1, 3, img_size, img_size], normalised and padded
    @torch.no_grad()
    def _set_encoder_input(self, x, input_size, original_size) -> None:
        self.reset_image()
        self.original_size = tuple(int(v) for v in original_size)
        self.input_size = tuple(int(v) for v in input_size)
        self.features = self.model.image_encoder(x)
        self.is_image_set = True

    @torch.no_grad()
    def predict_low_res(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output=True):
        """The prompt encoder and the mask decoder of `predict_torch`: (low_res_masks [B, C, 256, 256], iou_predictions [B, C])."""
        require_gpu_mask(mask_input, "SamPredictor")
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        points = (point_coords, point_labels) if point_coords is not None else None
        return self.model.decode_prompts(self.features, points, boxes, mask_input, multimask_output)

    @torch.no_grad()
    def predict_torch(self, point_coords: Optional[torch.Tensor], point_labels: Optional[torch.Tensor],
                      boxes: Optional[torch.Tensor] = None, mask_input: Optional[torch.Tensor] = None,
                      multimask_output: bool = True, return_logits: bool = False):
        low_res_masks, iou_predictions = self.predict_low_res(point_coords, point_labels, boxes, mask_input, multimask_output)
        masks = self.model.postprocess_masks(low_res_masks, self.input_size, self.original_size)
        if not return_logits:
            masks = masks > self.model.mask_threshold
        return masks, iou_predictions, low_res_masks

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output=True, return_logits=False):
        """numpy wrapper of `predict_torch` for one prompt (predictor.py:91-165); `mask_input`: [1, 256, 256] logits, e.g. one
        mask of an earlier call's low-res output."""
        coords = labels = box_t = mask_t = None
        if point_coords is not None:
            assert point_labels is not None, "point_labels must be supplied if point_coords is supplied."
            pc = self.transform.apply_coords(point_coords, self.original_size)
            coords = torch.as_tensor(pc, dtype=torch.float, device=self.device)[None, :, :]
            labels = torch.as_tensor(point_labels, dtype=torch.int, device=self.device)[None, :]
        if box is not None:
            box_t = torch.as_tensor(self.transform.apply_boxes(box, self.original_size), dtype=torch.float, device=self.device)[None, :]
        if mask_input is not None:
            mask_t = torch.as_tensor(mask_input, dtype=torch.float, device=self.device)[None, :, :, :]
        masks, iou, low = self.predict_torch(coords, labels, box_t, mask_t, multimask_output, return_logits=return_logits)
        return masks[0].cpu().numpy(), iou[0].cpu().numpy(), low[0].cpu().numpy()

    def get_image_embedding(self) -> torch.Tensor:
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) to generate an embedding.")
        return self.features

    def reset_image(self) -> None:
        self.is_image_set = False
        self.features = None
        self.original_size = None
        self.input_size = None


# ---- the generator -------------------------------------------------------------------------------------------------------
def process_low_res(low_res, iou_preds, input_size, original_size, pred_iou_thresh, stability_score_thresh, mask_threshold=0.0,
                    stability_score_offset=1.0, img_size=sam_amg.IMG_SIZE):
    """`_process_batch` after the decoder, on the device: low_res [M, h, w], iou_preds [M] -> dict of the masks that pass the
    IoU and the stability filter, in index order: `index` (into M, int64), `iou_preds`, `stability_score`, `boxes` (int32 XYXY),
    `area`, `packed` (int32 words [n, H, ceil(W / 32)]), plus `index_iou` (after the IoU filter only) and its `stats`."""
    iou_preds = iou_preds.reshape(-1)
    if pred_iou_thresh > 0.0:
        sel = torch.nonzero(iou_preds > pred_iou_thresh).reshape(-1).to(torch.int32)   # index order; its length is the one sync
    else:
        sel = torch.arange(iou_preds.numel(), device=iou_preds.device, dtype=torch.int32)
    stats, packed, _ = postprocess_batch(low_res, sel, input_size, original_size, mask_threshold, stability_score_offset, img_size)
    stability = stats[:, 7].view(torch.float32)
    idx = sel.to(torch.int64)
    out = {"index_iou": idx, "stats": stats}
    if stability_score_thresh > 0.0:
        keep = torch.nonzero(stability >= stability_score_thresh).reshape(-1)
        idx, stats, packed, stability = idx[keep], stats[keep], packed[keep], stability[keep]
    out.update(index=idx, iou_preds=iou_preds[idx], stability_score=stability, boxes=stats[:, 3:7], area=stats[:, 2], packed=packed)
    return out


def unpack_on_device(packed, W):
    """int32 words [n, H, ceil(W / 32)] -> bool [n, H, W] (torch, on the words' device)."""
    shifts = torch.arange(32, device=packed.device, dtype=torch.int32)
    bits = (packed.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(*packed.shape[:-1], packed.shape[-1] * 32)[..., :W].to(torch.bool)


class SamAutomaticMaskGenerator:
    """automatic_mask_generator.py with the constructor and defaults of the POPE fork (16 x 16 points, 2048 points per batch,
    IoU 0.9, stability 0.95, box NMS 0.35, min_mask_region_area 250), for a single crop."""

    def __init__(self, model: Sam, points_per_side: Optional[int] = 16, points_per_batch: int = 2048, pred_iou_thresh: float = 0.9,
                 stability_score_thresh: float = 0.95, stability_score_offset: float = 1.0, box_nms_thresh: float = 0.35,
                 crop_n_layers: int = 0, crop_nms_thresh: float = 0.35, crop_overlap_ratio: float = 512 / 1500,
                 crop_n_points_downscale_factor: int = 1, point_grids: Optional[List[np.ndarray]] = None,
                 min_mask_region_area: int = 250, output_mode: str = "binary_mask") -> None:
        assert (points_per_side is None) != (point_grids is None), "Exactly one of points_per_side or point_grid must be provided."
        if crop_n_layers > 0:
            raise NotImplementedError("pope_amd SamAutomaticMaskGenerator: crop layers are not supported (crop_n_layers must be 0)")
        assert output_mode in ["binary_mask", "uncompressed_rle", "coco_rle"], f"Unknown output_mode {output_mode}."
        if output_mode == "coco_rle":
            raise NotImplementedError("pope_amd SamAutomaticMaskGenerator: output_mode='coco_rle' needs pycocotools, which is not a dependency")
        self.point_grids = [sam_amg.build_point_grid(points_per_side)] if points_per_side is not None else point_grids
        self.predictor = SamPredictor(model)
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode
        self.last_low_res = None   # (low_res [M, 256, 256], iou_preds [M]) of the last generate(keep_low_res=True) call

    # the decoder call of one point batch: (low_res [P * 3, 256, 256], iou [P * 3])
    def _decode(self, features, points, im_size):
        pr = self.predictor
        tp = pr.transform.apply_coords(points, im_size)
        in_points = torch.as_tensor(tp, device=pr.device)
        in_labels = torch.ones(in_points.shape[0], dtype=torch.int, device=in_points.device)
        low, iou = pr.model.decode_prompts(features, (in_points[:, None, :], in_labels[:, None]), None, None, True)
        return low.flatten(0, 1), iou.flatten(0, 1)

    # the point-batch loop of one frame, from its features [1, 256, 64, 64] and its size in the input frame: the filtered
    # per-mask data of `process_low_res`
    def _decode_frame(self, features, input_size, hw, keep_low_res=False):
        H, W = hw
        pr = self.predictor
        points_all = self.point_grids[0] * np.array([[W, H]])
        lows, ious, parts, pts, base = [], [], [], [], 0
        for b in range(0, len(points_all), self.points_per_batch):
            points = points_all[b:b + self.points_per_batch]
            low, iou = self._decode(features, points, (H, W))
            if keep_low_res:
                lows.append(low)
                ious.append(iou)
            d = process_low_res(low, iou, input_size, (H, W), self.pred_iou_thresh, self.stability_score_thresh,
                                pr.model.mask_threshold, self.stability_score_offset, pr.model.image_encoder.img_size)
            d["index"] = d["index"] + base
            base += low.shape[0]
            parts.append(d)
            pts.append(np.repeat(points, 3, axis=0))
        if keep_low_res:
            self.last_low_res = (torch.cat(lows), torch.cat(ious))
        data = {k: torch.cat([p[k] for p in parts]) for k in ("index", "iou_preds", "stability_score", "boxes", "area", "packed")}
        return data, np.concatenate(pts)

    @torch.no_grad()
    def generate(self, image, keep_low_res: bool = False) -> List[Dict[str, Any]]:
        """HWC uint8 image (a numpy array, or a CUDA tensor on the model's device) -> list of records (`segmentation`, `area`,
        `bbox` XYWH, `predicted_iou`, `point_coords`, `stability_score`, `crop_box`), in the reference's order."""
        H, W = image.shape[:2]
        pr = self.predictor
        pr.set_image(image)
        data, points = self._decode_frame(pr.features, pr.input_size, (H, W), keep_low_res)
        pr.reset_image()
        return self._finish(data, [0, data["index"].numel()], points, (H, W))[0]

    @torch.no_grad()
    def generate_batch(self, images: List[np.ndarray]) -> List[List[Dict[str, Any]]]:
        """`generate` for a list of HWC uint8 frames of one common size: the image encoder runs over the stacked frames, the
        decoder and the fused post-processing per frame, NMS, small regions and the encoding once for all frames.  The list for
        frame q is record for record what `generate(images[q])` returns.  The frames are numpy arrays or CPU tensors (resized on
        the host), or they sit on the model's device: a uint8 [Q, H, W, 3] CUDA tensor or a list of [H, W, 3] CUDA tensors
        (one `pope_sam_preprocess_u8_f32` call for the stack, the same records).  A list that mixes the two raises ValueError."""
        images = images if on_device(images) else list(images)
        if not len(images):
            return []
        return self._finish(*self._decode_frames(images, "generate_batch"))

    @torch.no_grad()
    def propose(self, image) -> np.ndarray:
        """The `bbox` values of `generate(image)` alone, in record order: int64 [P, 4] XYWH ([0, 4] when nothing survives)."""
        H, W = image.shape[:2]
        pr = self.predictor
        pr.set_image(image)
        data, _ = self._decode_frame(pr.features, pr.input_size, (H, W))
        pr.reset_image()
        return self._finish_boxes(data, [0, data["index"].numel()], (H, W))[0]

    @torch.no_grad()
    def propose_batch(self, images: List[np.ndarray]) -> List[np.ndarray]:
        """The proposals of `generate_batch(images)` without its records: one int64 [P_q, 4] XYWH array per frame, row i the
        `bbox` of record i of that frame, whatever the `output_mode`.  The encoder, the decoder and the tail up to the second
        NMS are those of `generate_batch`; no mask is unpacked, encoded or downloaded, the host reads the survivor counts of
        the NMS calls and the survivors' boxes.  Frames on the device as in `generate_batch`."""
        images = images if on_device(images) else list(images)
        if not len(images):
            return []
        data, seg, _, hw = self._decode_frames(images, "propose_batch")
        return self._finish_boxes(data, seg, hw)

    # the front of the batched calls: one encoder call over the stacked frames, then the decoder frame by frame.  Returns the
    # arguments of `_finish`: (concatenated filtered per-mask data, its seg_offsets, the prompt point of every mask, (H, W))
    def _decode_frames(self, images, what):
        pr = self.predictor
        enc = pr.model.image_encoder
        stack = frames_on_device(images, what)
        if stack is not None:
            # frames in HBM: resample, normalisation and pad of the whole stack in one call
            H, W = (int(v) for v in stack.shape[1:3])
            x, input_size = pr.preprocess_frames(stack, "RGB", what)
        else:
            H, W = images[0].shape[:2]
            if any(im.shape[:2] != (H, W) for im in images):
                raise ValueError(f"{what}: all frames must have one size, got "
                                 + ", ".join(sorted({f"{im.shape[0]} x {im.shape[1]}" for im in images})))
            resized = np.stack([pr.transform.apply_image(im[..., ::-1] if pr.model.image_format != "RGB" else im) for im in images])
            x = torch.as_tensor(resized, device=pr.device).permute(0, 3, 1, 2).contiguous()
            x = pr.model.preprocess(x).contiguous()
            input_size = tuple(resized.shape[1:3])
        events = enc.overflow_events
        features = enc(x)
        if enc.overflow_events != events:
            # the range guard re-ran the whole call on the fp32 MFMA: encode frame by frame, so that a frame's features do not
            # depend on a neighbour's overflow (generate() of that frame alone would not have been re-run)
            features = torch.cat([enc(x[q:q + 1]) for q in range(len(images))])
        pr.reset_image()   # the batched calls leave the predictor as `generate` does: without an image
        parts, seg, points = [], [0], None
        for q in range(len(images)):
            data, points = self._decode_frame(features[q:q + 1], input_size, (H, W))
            parts.append(data)
            seg.append(seg[-1] + data["index"].numel())
        data = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
        return data, seg, points, (H, W)

    def _survivors(self, data, seg, hw, keys):
        """The tail both `_finish` and `_finish_boxes` run, for S frames at once from their concatenated filtered per-mask
        results of `process_low_res` (frame s = rows seg[s] .. seg[s + 1] - 1): segmented NMS, small regions, second NMS.
        Returns (the columns `keys` of the survivors, on the device; their seg_offsets).  The host reads the segments'
        survivor counts, once per NMS.  `packed` is gathered only where the clean-up or the caller needs it."""
        keep, counts = box_nms_segments(data["boxes"], data["iou_preds"], seg, self.box_nms_thresh)
        sel, seg = select_segments(keep, counts, seg)
        clean = self.min_mask_region_area > 0 and sel.numel() > 0
        need = set(keys) | ({"boxes", "packed"} if clean else set())
        data = {k: data[k][sel] for k in need}
        if clean:
            data, seg = postprocess_small_regions_segments(data, seg, hw[1], self.min_mask_region_area,
                                                           max(self.box_nms_thresh, self.crop_nms_thresh))
        return {k: data[k] for k in keys}, seg

    def _finish_boxes(self, data, seg, hw):
        """The proposals-only tail: one int64 [P_s, 4] XYWH array per frame, the `bbox` values of `_finish`'s records.  The only
        downloads are the survivor counts and the survivors' boxes."""
        data, seg = self._survivors(data, seg, hw, ("boxes",))
        xyxy = data["boxes"].cpu().numpy().astype(np.int64).reshape(-1, 4)
        xywh = np.concatenate([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], axis=1)     # `sam_amg.box_xyxy_to_xywh` of every row
        return [xywh[int(seg[s]):int(seg[s + 1])] for s in range(len(seg) - 1)]

    def _finish(self, data, seg, points, hw):
        """NMS, small regions, encoding and the records of S frames at once, from their concatenated filtered per-mask results
        of `process_low_res` (frame s = rows seg[s] .. seg[s + 1] - 1): one list of records per frame.  The host reads the
        segments' survivor counts (once per NMS), the per-mask scalars and either the run lengths or the dense masks."""
        H, W = hw
        data, seg = self._survivors(data, seg, hw, ("index", "iou_preds", "stability_score", "boxes", "area", "packed"))
        host = {k: data[k].cpu().numpy() for k in ("index", "iou_preds", "stability_score", "boxes", "area")}
        if self.output_mode == "binary_mask":
            segm = unpack_on_device(data["packed"], W).cpu().numpy()
        else:
            segm = rle_from_packed(data["packed"], W)
        out = []
        for s in range(len(seg) - 1):
            out.append([{
                "segmentation": segm[i],
                "area": int(host["area"][i]),
                "bbox": sam_amg.box_xyxy_to_xywh(host["boxes"][i]),
                "predicted_iou": float(host["iou_preds"][i]),
                "point_coords": [points[int(host["index"][i])].tolist()],
                "stability_score": float(host["stability_score"][i]),
                "crop_box": [0, 0, W, H],
            } for i in range(int(seg[s]), int(seg[s + 1]))])
        return out


def select_segments(keep, counts, seg):
    """The survivors of `box_nms_segments` as one index list: (rows int64 on the device, segment after segment in score order;
    the survivors' own seg_offsets as host integers).  Reads `counts` (one synchronisation)."""
    counts = counts.cpu().numpy().astype(np.int64)
    if (counts < 0).any():
        raise ValueError("box_nms_segments: a segment holds more boxes than one workgroup takes")
    pos = np.concatenate([np.arange(int(seg[s]), int(seg[s]) + int(c)) for s, c in enumerate(counts)] + [np.zeros(0, np.int64)])
    new_seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return keep[torch.as_tensor(pos.astype(np.int64)).to(keep.device)].to(torch.int64), new_seg


def clean_masks_packed(packed, W, min_area):
    """`remove_small_regions` (holes, then islands, 8-connectivity) of a batch of bit-packed masks in one launch
    (`pope_sam_small_regions_u32`, pope_amd/csrc/sam_regions.hip), without a host read: int32 words [n, H, ceil(W / 32)] ->
    (cleaned words, unchanged bool [n], boxes int32 [n, 4] XYXY of the cleaned masks, area int32 [n])."""
    packed = _packed_words(packed, W, "clean_masks_packed")
    n, H, _ = packed.shape
    dev = packed.device
    out = torch.empty_like(packed)
    unchanged = torch.empty(n, dtype=torch.int32, device=dev)
    boxes = torch.empty(n, 4, dtype=torch.int32, device=dev)
    area = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return out, unchanged.to(torch.bool), boxes, area
    need = int(_lib.lib().pope_sam_small_regions_workspace_bytes(n, H, int(W)))
    if need <= 0 or min_area < 0:
        raise ValueError(f"clean_masks_packed: unsupported geometry or threshold (masks {H} x {W}, min_area {min_area})")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with on_device_of(packed):
        check(_lib.lib().pope_sam_small_regions_u32(ptr(packed), n, H, int(W), int(min_area), ptr(out), ptr(unchanged), ptr(boxes),
                                                    ptr(area), ptr(ws), ws.numel(), stream_of(dev)), "pope_sam_small_regions_u32")
    return out, unchanged.to(torch.bool), boxes, area


def postprocess_small_regions_segments(data, seg, W, min_area, nms_thresh):
    """automatic_mask_generator.py:325-375 on the device, for the concatenated NMS survivors of one or several frames (frame s =
    rows seg[s] .. seg[s + 1] - 1): small holes and islands removed (8-connectivity) from the packed masks by one
    `clean_masks_packed` launch over all of them, then one segmented second NMS on the cleaned masks' boxes in which changed
    masks score 0 and unchanged ones 1; nothing is unpacked.  Returns (data of the survivors with the cleaned `packed` words,
    the cleaned masks' `area` and the boxes of the changed ones replaced; their seg_offsets)."""
    packed, unchanged, boxes, area = clean_masks_packed(data["packed"], W, min_area)
    keep, counts = box_nms_segments(boxes, unchanged.to(torch.float32), seg, nms_thresh)
    sel, seg = select_segments(keep, counts, seg)
    new_boxes = torch.where(unchanged[:, None], data["boxes"], boxes)
    data = dict(data, boxes=new_boxes, area=area, packed=packed)
    return {k: v[sel] for k, v in data.items()}, seg

