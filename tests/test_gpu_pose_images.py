"""GPU: `pope_pose_images_u8_f32` (`preprocess.pose_images`) against its numpy twin `resize_linear_cv_u8`, bit for bit: every
shape of tests/test_pose_images_cpu.py (the linear path, the 2 x area path, the copy), gathered rows with two rows out of
range, no rows, both layouts, Q = 0, an image alone against the same image inside the batch, and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from pope_amd.preprocess import pose_images, resize_linear_cv_tables, resize_linear_cv_u8
from test_pose_images_cpu import IDS, SHAPES

pytestmark = pytest.mark.gpu
P = 4
ROWS = [3, 0, 3, -1, 7, 1]


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def images(h, w):
    return np.random.default_rng([11, h, w]).integers(0, 256, (P, h, w, 3), dtype=np.uint8)


def entry(lib, src, rows, oh, ow, transposed, out, Q=None):
    """The C entry with tables of its own (of one sample where a refused call names no valid size); `rows` a device int32 tensor
    or None."""
    dev = src.device
    xs, xc = (torch.from_numpy(a).to(dev) for a in resize_linear_cv_tables(src.shape[2], max(ow, 1)))
    ys, yc = (torch.from_numpy(a).to(dev) for a in resize_linear_cv_tables(src.shape[1], max(oh, 1)))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    Q = (src.shape[0] if rows is None else rows.numel()) if Q is None else Q
    rc = lib.pope_pose_images_u8_f32(p(src), src.shape[0], src.shape[1], src.shape[2], p(rows), Q, p(xs), p(xc), p(ys), p(yc), oh, ow,
                                     int(transposed), p(out), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return rc


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entry_equals_the_twin(hip_lib, dev, shape):
    (h, w), (oh, ow) = shape
    host = images(h, w)
    twin = np.stack([resize_linear_cv_u8(im, oh, ow) for im in host]).astype(np.float32)        # [P, oh, ow, 3]
    zero = np.zeros((oh, ow, 3), np.float32)
    want = np.stack([twin[r] if 0 <= r < P else zero for r in ROWS])
    src = torch.from_numpy(host).to(dev)
    rows = torch.tensor(ROWS, dtype=torch.int32, device=dev)
    for transposed in (1, 0):
        out = torch.full((len(ROWS), 3, ow, oh) if transposed else (len(ROWS), 3, oh, ow), -7.0, device=dev)
        assert entry(hip_lib, src, rows, oh, ow, transposed, out) == 0
        layout = want.transpose(0, 3, 2, 1) if transposed else want.transpose(0, 3, 1, 2)
        assert np.array_equal(out.cpu().numpy(), layout), transposed
        assert float(out[3].abs().max()) == 0 and float(out[4].abs().max()) == 0              # rows -1 and 7
        # no rows: the identity
        out = torch.full((P, 3, ow, oh) if transposed else (P, 3, oh, ow), -7.0, device=dev)
        assert entry(hip_lib, src, None, oh, ow, transposed, out) == 0
        assert np.array_equal(out.cpu().numpy(), twin.transpose(0, 3, 2, 1) if transposed else twin.transpose(0, 3, 1, 2))
    # an image alone is the image inside the batch
    alone = torch.empty(1, 3, ow, oh, device=dev)
    assert entry(hip_lib, src[3:4].contiguous(), None, oh, ow, 1, alone) == 0
    assert np.array_equal(alone.cpu().numpy()[0], want[0].transpose(2, 1, 0))
    # Q = 0 writes nothing
    out = torch.full((1, 3, ow, oh), -7.0, device=dev)
    assert entry(hip_lib, src, rows, oh, ow, 1, out, Q=0) == 0 and float(out.max()) == -7.0


def test_op(dev):
    (h, w), size = (37, 53), 24
    host = images(h, w)
    twin = np.stack([resize_linear_cv_u8(im, size, size) for im in host]).astype(np.float32)
    src = torch.from_numpy(host).to(dev)
    got = pose_images(src, None, size)
    assert got.shape == (P, 3, size, size) and got.dtype == torch.float32 and got.device == src.device
    for b in range(P):           # the fork's own expression, per image
        assert torch.equal(got[b].cpu(), torch.from_numpy(twin[b]).permute(2, 1, 0))
    assert np.array_equal(pose_images(src, None, size, transposed=False).cpu().numpy(), twin.transpose(0, 3, 1, 2))
    for dtype in (torch.int32, torch.int64):
        rows = torch.tensor(ROWS + [2 ** 40 if dtype == torch.int64 else 2 ** 31 - 1], dtype=dtype, device=dev)
        picked = pose_images(src, rows, size)
        for q, r in enumerate(rows.tolist()):
            want = got[r] if 0 <= r < P else torch.zeros_like(got[0])
            assert torch.equal(picked[q], want), (dtype, q)
    assert pose_images(src, rows[:0], size).shape == (0, 3, size, size)
    assert pose_images(src[:, ::2], None, size).shape == (P, 3, size, size)                  # a strided view is made contiguous
    default = pose_images(src[:1])
    assert default.shape == (1, 3, 224, 224)
    assert np.array_equal(default[0].cpu().numpy(), resize_linear_cv_u8(host[0], 224, 224).astype(np.float32).transpose(2, 1, 0))
    with pytest.raises(TypeError):
        pose_images(src.float(), None, size)
    with pytest.raises(TypeError):
        pose_images(src, [0, 1], size)
    with pytest.raises(ValueError):
        pose_images(src, rows.cpu(), size)
    with pytest.raises(Exception):
        pose_images(src.cpu(), None, size)


def test_argument_errors(hip_lib, dev):
    src = torch.zeros(P, 8, 8, 3, dtype=torch.uint8, device=dev)
    rows = torch.zeros(6, dtype=torch.int32, device=dev)
    out = torch.full((6 * 3 * 4 * 4 + 1,), -7.0, device=dev)
    err = entry(hip_lib, src, rows, 4, 4, 1, None)
    assert err != 0 and b"argument" in hip_lib.pope_error_string(err).lower()
    assert entry(hip_lib, src, None, 4, 4, 1, out, Q=6) == err                     # the identity needs Q == P
    assert entry(hip_lib, src, rows, 0, 4, 1, out) == err and entry(hip_lib, src, rows, 4, -1, 1, out) == err
    assert entry(hip_lib, src, rows, 4, 4, 1, out, Q=-1) == err
    misaligned = out.view(torch.uint8)[2:2 + 6 * 3 * 4 * 4 * 4]
    assert entry(hip_lib, src, rows, 4, 4, 1, misaligned) == err
    assert float(out.max()) == -7.0 and float(out.min()) == -7.0                  # nothing was written
