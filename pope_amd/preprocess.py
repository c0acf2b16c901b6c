"""Batched GPU preprocessing: `set_torch_image` for P proposal crops at once and the gray / 255
conversion of the matcher's inputs, on HIP kernels (pope_amd/csrc/preprocess.hip) that are bit-identical to the host
path of the reference (segment_anything/segment_anything/dinov2_utils.py:55-78: PIL + torchvision transforms).

The resize is Pillow's 8-bit bilinear resample; its per-output-pixel windows and fixed-point weights depend on the
(input, output) sizes only and are built here on the host in double precision exactly as Pillow's `precompute_coeffs`
builds them (cached per size pair), so the kernels only do the integer arithmetic.

SAM's input transform is the same resample of whole frames: `resize_u8_batch` is `ResizeLongestSide.apply_image` for frames
that already sit in HBM, `sam_preprocess_batch` that resize, `Sam.preprocess` and its zero pad as one result (segment_anything
utils/transforms.py, modeling/sam.py), both bit-identical to the host chain.  `frames_on_device` is how the calls that take
frames as numpy arrays or tensors (pope_amd/sam_generator.py, pope_amd/driver.py) tell the two apart.

`pose_images` makes the image pair of the fork's image-conditioned pose heads (pose/dataset.py:102-106, train0604.py:148-151:
`cv2.resize` to 224 x 224, `.float()`, `.permute(0, 3, 2, 1)`) for Q images gathered by a device index, in one launch.  Its resize
is OpenCV's 8-bit INTER_LINEAR path restated (`resize_linear_cv_tables`, host twin `resize_linear_cv_u8`); cv2 is not installed
here, so parity with the library is unpinned and the twin is the contract.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, on_device_of, require_cuda, stream_of
from .sam_amg import preprocess_shape
from .synth import IMAGENET_MEAN, IMAGENET_STD

PRECISION_BITS = 32 - 8 - 2   # Pillow, 8 bits per channel


def resize_tables(in_size, out_size):
    """Windows and weights of one pass of Pillow's bilinear resample from `in_size` to `out_size` samples:
    (start[out], count[out], weights[out, ksize]) as int32 arrays, weights with 22 fractional bits."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filterscale                      # triangle filter: support 1, stretched when downscaling (antialias)
    ksize = int(math.ceil(support)) * 2 + 1
    start = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    inv = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [max(0.0, 1.0 - abs((x + lo - center + 0.5) * inv)) for x in range(hi - lo)]
        total = 0.0
        for v in w:                            # sequential double-precision sum, as in the C loop
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        start[xx], count[xx] = lo, hi - lo
        kk[xx, :hi - lo] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return start, count, kk


_tables = {}


def _device_tables(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _tables:
        s, c, k = resize_tables(in_size, out_size)
        _tables[key] = (torch.from_numpy(s).to(device), torch.from_numpy(c).to(device), torch.from_numpy(k).to(device),
                        int(k.shape[1]), s, c)
    return _tables[key]


@torch.no_grad()
def preprocess_batch(images, resize, crop=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """[P, H, W, 3] uint8 (CUDA tensor) -> [P, 3, h, w] fp32: Resize(resize) -> CenterCrop(crop) -> /255 -> Normalize,
    bit-identical to the PIL / torchvision host path for every image of the batch."""
    require_cuda(images, "preprocess_batch")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise TypeError("preprocess_batch expects a uint8 [P, H, W, 3] tensor")
    images = images.contiguous()
    P, Hin, Win, _ = images.shape
    OH, OW = int(resize[0]), int(resize[1])
    if crop is None:
        ch, cw, top, left = OH, OW, 0, 0
    else:   # torchvision CenterCrop
        ch, cw = int(crop[0]), int(crop[1])
        top, left = int(round((OH - ch) / 2.0)), int(round((OW - cw) / 2.0))
    dev = images.device
    hs, hc, hk, kh, _, _ = _device_tables(Win, OW, dev)
    vs, vc, vk, kv, vs_h, vc_h = _device_tables(Hin, OH, dev)
    row0 = int(vs_h[top])
    nrows = int(vs_h[top + ch - 1] + vc_h[top + ch - 1]) - row0
    out = torch.empty(P, 3, ch, cw, dtype=torch.float32, device=dev)
    scratch = torch.empty(P * nrows * cw * 3, dtype=torch.uint8, device=dev)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    p = lambda t: C.c_void_p(t.data_ptr())
    with on_device_of(images):
        check(_lib.lib().pope_preprocess_u8_f32(p(images), P, Hin, Win, p(hs), p(hc), p(hk), kh, p(vs), p(vc), p(vk), kv, top, left,
                                                ch, cw, row0, nrows, m, s, p(out), p(scratch), scratch.numel(), stream_of(dev)),
              "pope_preprocess_u8_f32")
    return out


def on_device(x):
    """The dispatch of every call that takes frames as numpy arrays or as tensors: a tensor that is not on the CPU takes the
    device path, numpy arrays and CPU tensors the host path."""
    return isinstance(x, torch.Tensor) and x.device.type != "cpu"


def frames_on_device(images, what):
    """The frames of a call that takes uint8 HWC frames as numpy arrays or as tensors: None when they are host data (numpy
    arrays, CPU tensors: the caller's host path), else one uint8 [Q, H, W, 3] tensor on the frames' device.  `images` is a
    [Q, H, W, 3] tensor or a sequence of [H, W, 3] frames.  A sequence that mixes host and device frames, frames of several
    sizes or on several devices raise ValueError; a device frame of another dtype or rank raises TypeError."""
    def checked(t, shape):
        if t.dtype != torch.uint8 or t.dim() != shape.count(",") + 1 or t.shape[-1] != 3:
            raise TypeError(f"{what}: device frames are uint8 {shape} tensors, got {t.dtype} {tuple(t.shape)}")
        return t

    if isinstance(images, torch.Tensor):
        return checked(images, "[Q, H, W, 3]") if on_device(images) else None
    images = list(images)
    where = [on_device(im) for im in images]
    if not any(where):
        return None
    if not all(where):
        raise ValueError(f"{what}: the frames of one call are all host arrays or all device tensors")
    for im in images:
        checked(im, "[H, W, 3]")
    if len({tuple(im.shape) for im in images}) > 1 or len({im.device for im in images}) > 1:
        raise ValueError(f"{what}: all frames must have one size and one device, got "
                         + ", ".join(sorted({f"{im.shape[0]} x {im.shape[1]} on {im.device}" for im in images})))
    return torch.stack(images)


def _resize_call(images, out_hw_of, who):
    """What both whole-frame resample bindings pass first, for the output size out_hw_of(H, W): (contiguous frames, (OH, OW), the
    table and size arguments of the C entry up to OW, a scratch tensor for the horizontal pass)."""
    require_cuda(images, who)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise TypeError(f"{who} expects a uint8 [P, H, W, 3] tensor")
    images = images.contiguous()
    P, Hin, Win, _ = images.shape
    OH, OW = (int(v) for v in out_hw_of(Hin, Win))
    if P <= 0 or min(Hin, Win, OH, OW) <= 0:
        raise ValueError(f"{who}: empty batch or size ({P} frames of {Hin} x {Win} to {OH} x {OW})")
    dev = images.device
    hs, hc, hk, kh, _, _ = _device_tables(Win, OW, dev)
    vs, vc, vk, kv, _, _ = _device_tables(Hin, OH, dev)
    scratch = torch.empty(P * Hin * OW * 3, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    return images, (OH, OW), (p(images), P, Hin, Win, p(hs), p(hc), p(hk), kh, p(vs), p(vc), p(vk), kv, OH, OW), scratch


@torch.no_grad()
def resize_u8_batch(images, out_hw):
    """[P, H, W, 3] uint8 (CUDA tensor) -> [P, OH, OW, 3] uint8: Pillow's 8-bit bilinear `Image.resize((OW, OH))` of every
    frame (`ResizeLongestSide.apply_image` when `out_hw` is its `get_preprocess_shape`), bit-identical."""
    images, (OH, OW), args, scratch = _resize_call(images, lambda h, w: out_hw, "resize_u8_batch")
    out = torch.empty(images.shape[0], OH, OW, 3, dtype=torch.uint8, device=images.device)
    with on_device_of(images):
        check(_lib.lib().pope_resize_u8(*args, C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                        stream_of(images.device)), "pope_resize_u8")
    return out


@torch.no_grad()
def sam_preprocess_batch(images, img_size, mean, std, flip=False):
    """SAM's input transform for [P, H, W, 3] uint8 frames (CUDA tensor) in one call: `ResizeLongestSide(img_size).apply_image`,
    then `Sam.preprocess` ((x - mean) / std on the 0..255 values, zero pad to the square) -> (x fp32 [P, 3, img_size, img_size],
    input_size = the resized (h, w)).  `mean` / `std`: three floats per model channel; `flip` reads the frame's channels in
    reverse order (a BGR frame for an RGB model).  Bit-identical to the host chain, the pad is +0.0."""
    S = int(img_size)
    images, input_size, args, scratch = _resize_call(images, lambda h, w: preprocess_shape(h, w, S), "sam_preprocess_batch")
    out = torch.empty(images.shape[0], 3, S, S, dtype=torch.float32, device=images.device)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    with on_device_of(images):
        check(_lib.lib().pope_sam_preprocess_u8_f32(*args, S, int(bool(flip)), m, s, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(scratch.data_ptr()), scratch.numel(), stream_of(images.device)),
              "pope_sam_preprocess_u8_f32")
    return out, input_size


def set_torch_images(images, center_crop=False, device="cuda"):
    """Batched `set_torch_image` (dinov2_utils.py:55-78): a list / array of HWC uint8 images of one size (or a uint8
    [P, H, W, 3] tensor) -> [P, 3, 196, 196] (center_crop) or [P, 3, 224, 224] on the GPU."""
    if not isinstance(images, torch.Tensor):
        images = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(i) for i in images])))
    images = images.to(device)
    return preprocess_batch(images, (256, 256), (196, 196)) if center_crop else preprocess_batch(images, (224, 224), None)


@torch.no_grad()
def crop_normalize(images, crop_hw, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """[P, H, W, 3] uint8 (CUDA) -> [P, 3, ch, cw] fp32: the centre crop + ToTensor + Normalize of the dense pair path (640 x 480
    frames -> 476 x 630, no resize), one kernel, bit-equal to torchvision's fp32 arithmetic.  `out` lets a pipeline reuse its
    input buffer."""
    require_cuda(images, "crop_normalize")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise TypeError("crop_normalize expects a uint8 [P, H, W, 3] tensor")
    images = images.contiguous()
    P, H, W, _ = images.shape
    ch, cw = crop_hw
    top, left = (H - ch) // 2, (W - cw) // 2
    if out is None:
        out = torch.empty(P, 3, ch, cw, dtype=torch.float32, device=images.device)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    with on_device_of(images):
        check(_lib.lib().pope_crop_normalize_u8_f32(C.c_void_p(images.data_ptr()), P, H, W, top, left, ch, cw, m, s,
                                                    C.c_void_p(out.data_ptr()), stream_of(images.device)), "pope_crop_normalize_u8_f32")
    return out


# ---- the image pair of the image-conditioned pose heads ---------------------------------------------------------------------------
CV_COEF_BITS = 11   # OpenCV: INTER_RESIZE_COEF_BITS


def resize_linear_cv_tables(n_in, n_out):
    """One axis of OpenCV's 8-bit `INTER_LINEAR` resize from `n_in` to `n_out` samples: (start[n_out], coef[n_out, 2]) int32 —
    the first tap of every output sample (the second is min(start + 1, n_in - 1)) and the two coefficients with 11 fractional
    bits, which sum to 2048.  Restated from OpenCV's public algorithm (cv2 is not in this image: unpinned against the library)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"resize_linear_cv_tables: sizes must be positive, got {n_in} -> {n_out}")
    scale = 1.0 / (np.float64(n_out) / np.float64(n_in))
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= n_in - 1
    s = np.where(low, 0, np.where(high, n_in - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    one = np.float32(1 << CV_COEF_BITS)
    coef = np.stack([np.rint((np.float32(1) - f) * one), np.rint(f * one)], 1).astype(np.int32)   # rint: round half to even
    return s.astype(np.int32), np.ascontiguousarray(coef)


def resize_linear_cv_u8(img_hwc_u8, oh, ow):
    """`cv2.resize(img, (ow, oh))` of a uint8 [H, W, C] image (default INTER_LINEAR) in numpy, the host twin of
    `pose_images`: per channel, the horizontal pass `src[sx] * ax0 + src[sx1] * ax1` in int32, then
    `(((ay0 * (row[sy] >> 4)) >> 16) + ((ay1 * (row[sy1] >> 4)) >> 16) + 2) >> 2`.  Equal sizes are a copy, and an exact 2 x
    shrink of BOTH axes is the rounded mean of the 2 x 2 block (OpenCV switches to its area path there).  Restated from OpenCV's
    public algorithm; cv2 is not in this image, so parity with the library is unpinned."""
    img = np.asarray(img_hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise TypeError("resize_linear_cv_u8 expects a uint8 [H, W, C] image")
    H, W = img.shape[:2]
    oh, ow = int(oh), int(ow)
    if (H, W) == (oh, ow):
        return img.copy()
    src = img.astype(np.int32)
    if H == 2 * oh and W == 2 * ow:
        return ((src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    ys, yc = resize_linear_cv_tables(H, oh)
    xs, xc = resize_linear_cv_tables(W, ow)
    xs1, ys1 = np.minimum(xs + 1, W - 1), np.minimum(ys + 1, H - 1)
    row = (src[:, xs] * xc[None, :, 0, None] + src[:, xs1] * xc[None, :, 1, None]) >> 4          # [H, ow, C]
    out = (((yc[:, 0, None, None] * row[ys]) >> 16) + ((yc[:, 1, None, None] * row[ys1]) >> 16) + 2) >> 2
    return out.astype(np.uint8)


_cv_tables = {}


def _device_cv_tables(n_in, n_out, device):
    key = (n_in, n_out, str(device))
    if key not in _cv_tables:
        _cv_tables[key] = tuple(torch.from_numpy(a).to(device) for a in resize_linear_cv_tables(n_in, n_out))
    return _cv_tables[key]


@torch.no_grad()
def pose_images(src_u8, rows=None, size=224, transposed=True):
    """The images the image-conditioned pose heads read (`pose_regressor_cnn.Mkpts_Reg_Model`, `mocope.MoCoPE`), made on the
    device in one launch: `src_u8` [P, H, W, 3] uint8 (CUDA, BGR as the drivers hold it) -> fp32 [Q, 3, size, size], image q =
    `cv2.resize(src_u8[rows[q]], (size, size))` as floats 0..255 in the stored channel order (linemod.py:129-130,
    pose/dataset.py:102-106).  `transposed` (default, what the fork's train / test loops feed: `.permute(0, 3, 2, 1)`,
    train0604.py:148-151) gives out[q, c, x, y]; False gives out[q, c, y, x].  `rows`: a CUDA int32 / int64 tensor [Q], or None for
    every image in order; a row outside [0, P) gives an all-zero image.  Nothing is read back.  Bit-equal to
    `resize_linear_cv_u8`, the numpy restatement of OpenCV's 8-bit INTER_LINEAR path (unpinned against cv2, which is absent)."""
    require_cuda(src_u8, "pose_images")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise TypeError("pose_images expects a uint8 [P, H, W, 3] tensor")
    src = src_u8.contiguous()
    P, Hin, Win, _ = src.shape
    OH = OW = int(size)
    if min(P, Hin, Win, OH) <= 0:
        raise ValueError(f"pose_images: empty source or size ({P} images of {Hin} x {Win} to {OH} x {OW})")
    dev = src.device
    if rows is not None:
        if not isinstance(rows, torch.Tensor) or rows.dtype not in (torch.int32, torch.int64) or rows.dim() != 1:
            raise TypeError("pose_images: rows is a 1-D int32 / int64 tensor on the images' device, or None")
        if rows.device != dev:
            raise ValueError(f"pose_images: rows on {rows.device}, images on {dev}")
        if rows.dtype == torch.int64:           # rows outside [0, P) stay outside after the narrowing
            rows = rows.clamp(-1, P)
        rows = rows.to(torch.int32).contiguous()
    Q = P if rows is None else int(rows.numel())
    out = torch.empty((Q, 3, OW, OH) if transposed else (Q, 3, OH, OW), dtype=torch.float32, device=dev)
    if Q == 0:          # an empty tensor has no address to hand over
        return out
    xs, xc = _device_cv_tables(Win, OW, dev)
    ys, yc = _device_cv_tables(Hin, OH, dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with on_device_of(src):
        check(_lib.lib().pope_pose_images_u8_f32(p(src), P, Hin, Win, p(rows) if rows is not None else None, Q, p(xs), p(xc), p(ys),
                                                 p(yc), OH, OW, int(bool(transposed)), p(out), stream_of(dev)),
              "pope_pose_images_u8_f32")
    return out


@torch.no_grad()
def gray_batch(images_bgr):
    """[P, H, W, 3] uint8 BGR (CUDA) -> [P, 1, H, W] fp32 in [0, 1]: cv2.cvtColor(BGR2GRAY) (OpenCV's 8-bit fixed-point
    weights) / 255., the matcher's input (eval_linemod_json.py:103-111).  OpenCV is not in this image: the integer
    formula is OpenCV's documented one, unpinned against the library."""
    require_cuda(images_bgr, "gray_batch")
    if images_bgr.dtype != torch.uint8 or images_bgr.dim() != 4 or images_bgr.shape[3] != 3:
        raise TypeError("gray_batch expects a uint8 [P, H, W, 3] tensor")
    images_bgr = images_bgr.contiguous()
    P, H, W, _ = images_bgr.shape
    out = torch.empty(P, 1, H, W, dtype=torch.float32, device=images_bgr.device)
    with on_device_of(images_bgr):
        check(_lib.lib().pope_gray_u8_f32(C.c_void_p(images_bgr.data_ptr()), P, H, W, C.c_void_p(out.data_ptr()),
                                          stream_of(images_bgr.device)), "pope_gray_u8_f32")
    return out
