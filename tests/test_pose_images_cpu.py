"""CPU: the image pair of the image-conditioned pose heads — the numpy twin of `preprocess.pose_images`
(`resize_linear_cv_u8`, OpenCV's 8-bit INTER_LINEAR path restated: cv2 is absent, so parity with it is unpinned), the C entry's
argument checks, and the interface around it (exports, parameter lists, the regressor types the query accepts).

Bound of the twin against float64 bilinear with the same clamps: one grey level.  The final value is a rounding to nearest
(0.5) of a sum whose two products were each floored on the quarter-level scale (together below 0.5 of a level, always
downwards), on top of coefficients rounded to 1 / 2048; measured <= 0.80 on these shapes (printed with -s)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from pope_amd.preprocess import resize_linear_cv_tables, resize_linear_cv_u8

LINEAR = [((5, 7), (9, 12)), ((37, 53), (16, 24)), ((48, 64), (24, 31)), ((2, 3), (224, 224)), ((256, 256), (224, 224)),
          ((480, 640), (224, 224))]
AREA = ((48, 64), (24, 32))
COPY = ((32, 32), (32, 32))
SHAPES = LINEAR + [AREA, COPY]
IDS = [f"{h}x{w}-{oh}x{ow}" for (h, w), (oh, ow) in SHAPES]


def image(h, w, seed=0):
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def bilinear64(img, oh, ow):
    """float64 bilinear with the clamps of the definition: a position below 0 or at / beyond the last sample reads that sample."""
    def axis(n_in, n_out):
        f = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        s = np.floor(f)
        f, s = f - s, s.astype(np.int64)
        low, high = s < 0, s >= n_in - 1
        return np.where(low, 0, np.where(high, n_in - 1, s)), np.where(low | high, 0.0, f)
    (ys, fy), (xs, fx) = axis(img.shape[0], oh), axis(img.shape[1], ow)
    ys1, xs1 = np.minimum(ys + 1, img.shape[0] - 1), np.minimum(xs + 1, img.shape[1] - 1)
    src = img.astype(np.float64)
    row = src[:, xs] * (1 - fx)[None, :, None] + src[:, xs1] * fx[None, :, None]
    return row[ys] * (1 - fy)[:, None, None] + row[ys1] * fy[:, None, None]


@pytest.mark.parametrize("n_in,n_out", sorted({(a, b) for (h, w), (oh, ow) in SHAPES for a, b in ((h, oh), (w, ow))}))
def test_tables(n_in, n_out):
    start, coef = resize_linear_cv_tables(n_in, n_out)
    assert start.dtype == np.int32 and coef.dtype == np.int32 and start.shape == (n_out,) and coef.shape == (n_out, 2)
    assert np.all(coef.sum(1) == 2048) and coef.min() >= 0
    assert start.min() >= 0 and start.max() <= n_in - 1 and np.minimum(start + 1, n_in - 1).max() <= n_in - 1
    assert np.all(np.diff(start) >= 0)
    if n_in == n_out:
        assert start.tolist() == list(range(n_in)) and np.all(coef[:, 0] == 2048)


def test_tables_follow_the_definition_sample_by_sample():
    """The vectorised tables against the issue's rule written as a scalar loop (float32 position, round half to even)."""
    for n_in, n_out in ((256, 224), (640, 224), (3, 224), (7, 12), (53, 24)):
        start, coef = resize_linear_cv_tables(n_in, n_out)
        scale = 1.0 / (np.float64(n_out) / np.float64(n_in))
        for d in range(n_out):
            f = np.float32((d + 0.5) * scale - 0.5)
            s = int(np.floor(f))
            f = np.float32(f - np.float32(s))
            if s < 0:
                s, f = 0, np.float32(0)
            if s >= n_in - 1:
                s, f = n_in - 1, np.float32(0)
            a0 = int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048)))
            a1 = int(np.rint(f * np.float32(2048)))
            assert (int(start[d]), int(coef[d, 0]), int(coef[d, 1])) == (s, a0, a1), (n_in, n_out, d)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_twin(shape):
    (h, w), (oh, ow) = shape
    img = image(h, w)
    out = resize_linear_cv_u8(img, oh, ow)
    assert out.dtype == np.uint8 and out.shape == (oh, ow, 3)
    for v in (0, 1, 127, 255):
        const = np.full((h, w, 3), v, np.uint8)
        assert np.array_equal(resize_linear_cv_u8(const, oh, ow), np.full((oh, ow, 3), v, np.uint8)), v
    err = float(np.abs(out.astype(np.float64) - bilinear64(img, oh, ow)).max())
    print(f"{h}x{w} -> {oh}x{ow}: max |twin - float64 bilinear| = {err:.4f}")
    assert err <= 1.0
    # channels are independent: a channel alone gives that channel
    assert np.array_equal(resize_linear_cv_u8(img[:, :, 1:2], oh, ow), out[:, :, 1:2])


def test_special_paths():
    (h, w), (oh, ow) = AREA
    img = image(h, w, 3)
    a = img.astype(np.int64)
    mean = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    assert np.array_equal(resize_linear_cv_u8(img, oh, ow), mean.astype(np.uint8))
    # 2 x on ONE axis only, and 4 x on both, stay on the linear path: they differ from the block mean somewhere
    one_axis = resize_linear_cv_u8(img, oh, w)
    assert one_axis.shape == (oh, w, 3) and float(np.abs(one_axis.astype(np.float64) - bilinear64(img, oh, w)).max()) <= 1.0
    quarter = resize_linear_cv_u8(img, h // 4, w // 4)
    block = a.reshape(h // 4, 4, w // 4, 4, 3).mean((1, 3))
    assert float(np.abs(quarter - block).max()) > 2.0
    (h, w), _ = COPY
    img = image(h, w, 4)
    out = resize_linear_cv_u8(img, h, w)
    assert np.array_equal(out, img) and out is not img
    with pytest.raises(TypeError):
        resize_linear_cv_u8(img.astype(np.float32), 8, 8)
    with pytest.raises(ValueError):
        resize_linear_cv_tables(0, 4)


def test_permuted_layout_is_the_forks():
    """What `pose_images(..., transposed=True)` returns per image, stated on the host: train0604.py:148-151 per image."""
    img = resize_linear_cv_u8(image(37, 53, 5), 16, 24)
    want = torch.from_numpy(img).float().permute(2, 1, 0)
    got = np.ascontiguousarray(img.astype(np.float32).transpose(2, 1, 0))          # out[c, x, y] = resized[y, x, c]
    assert want.shape == (3, 24, 16) and np.array_equal(want.numpy(), got)
    assert got[2, 5, 7] == float(img[7, 5, 2])


def test_symbol_and_abi(hip_lib):
    from pope_amd import _lib
    assert hip_lib.pope_abi_version() == 10
    assert "pope_pose_images_u8_f32" in _lib.PROTOTYPES and hasattr(hip_lib, "pope_pose_images_u8_f32")
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pope_hip.h")).read()
    assert "int pope_pose_images_u8_f32(" in header


def _call(lib, **over):
    """A valid 48 x 64 -> 24 x 31 call by name (fake non-null addresses: every case returns before any HIP call)."""
    a = dict(src=0x1000, P=4, Hin=48, Win=64, rows=0x2000, Q=6, xstart=0x3000, xcoef=0x4000, ystart=0x5000, ycoef=0x6000, OH=24, OW=31,
             transposed=1, out=0x7000)
    a.update(over)
    return lib.pope_pose_images_u8_f32(*[C.c_void_p(v) if k in ("src", "rows", "xstart", "xcoef", "ystart", "ycoef", "out") else v
                                         for k, v in a.items()], None)


def test_argument_errors_come_before_any_hip_call(hip_lib):
    """No GPU in this process: each of these returns POPE_ERR_ARG from the checks alone."""
    err = _call(hip_lib, src=None)
    assert err != 0 and b"argument" in hip_lib.pope_error_string(err).lower()
    for over in (dict(out=None), dict(xstart=None), dict(xcoef=None), dict(ystart=None), dict(ycoef=None), dict(P=0), dict(Hin=0),
                 dict(Win=-1), dict(OH=0), dict(OW=0), dict(Q=-1), dict(rows=None), dict(out=0x7002), dict(out=0x7001)):
        assert _call(hip_lib, **over) == err, over
    assert _call(hip_lib, Q=0) == 0                         # a no-op
    assert _call(hip_lib, rows=None, Q=4, P=4, out=None) == err


def test_interface():
    from pope_amd import driver, pope_model_api as api
    from pope_amd import mocope, preprocess
    assert api.MoCoPE is mocope.MoCoPE and api.regress_pose_fused_batch is mocope.regress_pose_fused_batch
    assert api.pose_images is preprocess.pose_images and api.regress_pose_from_frames is driver.regress_pose_from_frames
    params = inspect.signature(driver.regress_pose_from_frames).parameters
    lead = ["mask_generator", "dinov2_model", "matcher", "pose_regressor", "refs_bgr", "frames_bgr", "K0", "K1"]
    want = {"conf_thr": 0.9, "ransac_thr": 0.5, "ransac_conf": 0.99, "out_size": 256, "max_proposals": None, "regressor_seed": 0,
            "pose_image_size": 224}
    assert list(params) == lead + list(want)
    assert all(params[k].default is inspect.Parameter.empty for k in lead) and {k: params[k].default for k in want} == want
    for fn in (driver.locate_match_pose_batch_u8, driver.locate_poses_in_frame, driver.encode_references):
        assert inspect.signature(fn).parameters["pose_image_size"].default == 224
        assert inspect.signature(fn).parameters["pose_regressor"].default is None
    assert list(inspect.signature(preprocess.pose_images).parameters) == ["src_u8", "rows", "size", "transposed"]
    fused = inspect.signature(mocope.regress_pose_fused_batch).parameters
    assert fused["feat0"].default is None and fused["feat1"].default is None
    assert list(fused)[:8] == ["model", "kpts0", "kpts1", "counts", "img0", "img1", "seed", "sample_index"]


class _NoGpu:
    """Stands where a model goes: any use fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name})")


def test_wrong_regressor_type_is_refused_before_any_device_work():
    from pope_amd import driver
    refs, frames, K = np.zeros((2, 32, 32, 3), np.uint8), np.zeros((2, 48, 64, 3), np.uint8), np.eye(3)
    boxes = [np.array([[4, 4, 20, 20]])] * 2
    names = "pose_regressor.Mkpts_Reg_Model, mocope.MoCoPE or pose_regressor_cnn.Mkpts_Reg_Model"
    for bad in (torch.nn.Linear(2, 2), "mocope", 3):
        with pytest.raises(TypeError, match=names):
            driver.locate_match_pose_batch_u8(_NoGpu(), _NoGpu(), refs, frames, boxes, K, K, pose_regressor=bad)
        with pytest.raises(TypeError, match=names):
            driver.regress_pose_from_frames(_NoGpu(), _NoGpu(), _NoGpu(), bad, refs, frames, K, K)
        with pytest.raises(TypeError, match=names):
            driver.locate_poses_in_frame(_NoGpu(), _NoGpu(), _NoGpu(), refs, frames[0], K, K, pose_regressor=bad)
        with pytest.raises(TypeError, match=names):
            driver.encode_references(_NoGpu(), _NoGpu(), refs, pose_regressor=bad)
    with pytest.raises(TypeError):
        driver.regress_pose_from_frames(_NoGpu(), _NoGpu(), _NoGpu(), None, refs, frames, K, K)


def test_mocope_takes_logits_in_place_of_an_image():
    """`_images` refuses an image together with its logits and logits of the wrong shape, before the backbone is asked."""
    from pope_amd import convnextv2, synth
    from pope_amd.mocope import MoCoPE
    model = MoCoPE(5, backbone=convnextv2.ConvNeXtV2(**synth.MOCOPE_TRUNK))
    img, feat = torch.zeros(2, 3, 8, 8), torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="img0 or feat0"):
        model._images(img, img, 2, "t", feat0=feat)
    with pytest.raises(ValueError, match="img1 or feat1"):
        model._images(img, img, 2, "t", feat1=feat)
    key = model.backbone_key()
    assert key == model.backbone_key()
    with torch.no_grad():
        next(model.convnextv2.parameters()).add_(1.0)
    assert key != model.backbone_key()
