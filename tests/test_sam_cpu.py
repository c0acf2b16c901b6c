"""CPU: the SAM image encoder oracle against the reference-generated fixtures, and the drop-in module's state-dict
layout (BASELINE config 5); the encoder's workspace layout and its contract "every argument is checked
before the first launch" (pope_amd/csrc/sam.hip: SamEncLayout, sam_encoder_check).  No HIP calls."""
import ctypes
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.usefixtures("golden_threads")   # bit-exact against the fixtures (conftest.py)


@pytest.mark.parametrize("name", ["sam_hd80_256", "sam_hd64_224"])
def test_oracle_reproduces_reference_fixture(golden_dir, name):
    from oracle import sam_encoder_ref
    from pope_amd import synth
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    dim, depth, heads, img, window = (int(v) for v in fx["arch"])
    gidx = tuple(int(v) for v in fx["global_idx"])
    sd = synth.synthetic_sam_encoder_state_dict(seed=int(fx["weights_seed"]), dim=dim, depth=depth, heads=heads, grid=img // 16,
                                                window=window, global_idx=gidx)
    assert np.array_equal(np.array([float(sd[k].double().sum()) for k in sorted(sd)]), fx["weights_digest"])
    x = synth.synthetic_images(int(fx["batch"]), img, img, seed=int(fx["input_seed"]))
    taps = {int(i): None for i in fx["tap_blocks"]}
    with torch.no_grad():
        out = sam_encoder_ref.forward(sd, x, heads, window, gidx, taps)
    stride, ts = int(fx["stride"]), max(2, int(fx["stride"]))
    np.testing.assert_allclose(out[:, :, ::stride, ::stride].numpy(), fx["out"], rtol=0, atol=2e-5)
    for i, t in taps.items():
        np.testing.assert_allclose(t[:, ::ts, ::ts, ::2].numpy(), fx[f"blk{i}"], rtol=0, atol=5e-5)


def test_module_has_the_reference_state_dict_layout():
    """Same keys and shapes as segment_anything's ImageEncoderViT (image_encoder.py:53-105): a checkpoint slice
    `image_encoder.*` of build_sam.py:102-105 loads with strict=True."""
    from pope_amd import synth
    from pope_amd.sam_encoder import ImageEncoderViT, get_rel_pos
    from oracle import sam_encoder_ref
    m = ImageEncoderViT(depth=4, embed_dim=640, img_size=256, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                        num_heads=8, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=[1, 3], window_size=14,
                        out_chans=256)
    sd = synth.synthetic_sam_encoder_state_dict(dim=640, depth=4, heads=8, grid=16, window=14, global_idx=(1, 3))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    assert m.blocks[0].window_size == 14 and m.blocks[1].window_size == 0
    # ViT-H key count as build_sam.py:13-21 (32 blocks x 14 + pos + patch 2 + neck 6)
    big = synth.synthetic_sam_encoder_state_dict(dim=128, depth=32, heads=2, grid=4, window=2, global_idx=(7, 15, 23, 31))
    assert len(big) == 32 * 14 + 9
    # the host-side relative-position gather, including the interpolated case (image_encoder.py:299-307)
    for q, L in ((14, 27), (16, 27), (8, 27)):
        rp = torch.randn(L, 80)
        assert torch.equal(get_rel_pos(q, q, rp), sam_encoder_ref.rel_pos_table(q, q, rp))


def test_forward_without_gpu_fails_loudly():
    from pope_amd.sam_encoder import ImageEncoderViT
    m = ImageEncoderViT(depth=1, embed_dim=256, img_size=224, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_heads=4,
                        use_rel_pos=True, window_size=14)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        m(torch.zeros(1, 3, 224, 224))


def _encoder_weights(dim, depth, heads, img, window, precision=0, global_idx=(), pointer=None):
    """A pope_sam_encoder_weights of the given geometry (patch 16, MLP ratio 4, 256 output channels); every pointer = `pointer`."""
    from pope_amd import _lib
    blocks = (_lib.SamBlockWeights * depth)()
    for i, b in enumerate(blocks):
        for name, _ in _lib.SamBlockWeights._fields_[:-1]:
            setattr(b, name, pointer)
        b.global_attn = int(i in global_idx)
    w = _lib.SamEncoderWeights()
    w.img, w.patch, w.dim, w.depth, w.heads, w.hidden, w.out_chans, w.window = img, 16, dim, depth, heads, 4 * dim, 256, window
    w.precision = precision
    for name in ("patch_wp", "patch_b", "pos", "ones", "neck0_wp", "neck1_w", "neck1_b", "neck2_wp", "neck3_w", "neck3_b"):
        setattr(w, name, pointer)
    w.blocks_host = ctypes.cast(blocks, ctypes.POINTER(_lib.SamBlockWeights))
    w._blocks = blocks   # keeps the array alive
    return w


VIT_B, VIT_L, VIT_H = (768, 12, 12, 1024), (1024, 24, 16, 1024), (1280, 32, 16, 1024)


@pytest.mark.parametrize("arch,window,B,want", [
    (VIT_B, 14, 1, 216072192), (VIT_B, 14, 16, 3457155072), (VIT_L, 14, 1, 283713536), (VIT_L, 14, 16, 4539416576),
    (VIT_H, 14, 1, 348594176), (VIT_H, 14, 16, 5577506816),
    ((256, 2, 4, 224), 14, 1, 3651584),      # sam_hd64_224: grid 14, window 14
    ((640, 4, 8, 256), 14, 2, 32133120),     # sam_hd80_256: grid 16, window 14
    (VIT_B, 0, 1, 214474752),                # window 0: both geometries are the grid's
    (VIT_B, 70, 1, 0),                       # no kernel holds 64 + 2 * 70 score columns
])
def test_workspace_bytes_are_those_of_the_three_carvings(hip_lib, arch, window, B, want):
    """The values the size query returned while the layout was written out three times (read from a build of that commit)."""
    w = _encoder_weights(*arch, window)
    assert hip_lib.pope_sam_encoder_workspace_bytes(ctypes.byref(w), B) == want


@pytest.mark.parametrize("precision", ["f16x3", "f16", "f32"])
def test_every_argument_is_checked_before_the_first_launch(hip_lib, precision):
    """With every argument valid a workspace one byte short is the only thing left to refuse: POPE_ERR_WORKSPACE shows that all
    argument checks accepted, and nothing was launched (no GPU here; the fake pointers are never dereferenced).  A fault in the
    LAST block, or an unknown precision with a sufficient workspace, is refused at the same point."""
    from pope_amd import _lib
    ERR_ARG, ERR_WORKSPACE = -1, -3
    buf = ctypes.create_string_buffer(512)
    ok = (ctypes.addressof(buf) + 255) & ~255
    taps, tap_out = (ctypes.c_int * 1)(1), (ctypes.c_void_p * 1)(ok)

    def forward(w, ws_bytes):
        return hip_lib.pope_sam_encoder_forward_f32(ctypes.byref(w), ok, 2, ok, 1, taps, tap_out, ok, ws_bytes, None, None)

    def weights(**kw):
        return _encoder_weights(640, 2, 8, 256, 14, precision=_lib.PRECISIONS[precision], global_idx=(1,), pointer=ok, **kw)

    w = weights()
    need = hip_lib.pope_sam_encoder_workspace_bytes(ctypes.byref(w), 2)
    assert need > 0
    assert forward(w, need - 1) == ERR_WORKSPACE
    for field in ("rel_h", "fc2_b"):
        w = weights()
        setattr(w._blocks[1], field, None)
        assert forward(w, need - 1) == ERR_ARG, field
    w = weights()
    w.precision = 7
    assert forward(w, need) == ERR_ARG


def test_depth_is_not_limited_by_a_copy(hip_lib):
    w = _encoder_weights(256, 65, 4, 224, 14, pointer=1 << 12)
    need = hip_lib.pope_sam_encoder_workspace_bytes(ctypes.byref(w), 1)
    assert need == 3651584      # the workspace does not depend on the depth
    assert hip_lib.pope_sam_encoder_forward_f32(ctypes.byref(w), 1 << 12, 1, 1 << 12, 0, None, None, 1 << 12, need - 1, None, None) == -3


@pytest.mark.parametrize("precision", ["f16x3", "f16", "f32"])
def test_limits_checked_in_the_block_loop_before_are_refused_up_front(hip_lib, precision):
    """One geometry on either side of each limit the launch sequence used to find inside its block loop, with a workspace of one
    byte: POPE_ERR_WORKSPACE = every argument check accepted, POPE_ERR_ARG = refused — both before any launch.  The batch sizes
    follow from the limits: the GEMMs' 32-bit offsets, (B 4096 + 256) max(hidden, 3 dim) 4 < 2^32 - 512, give B <= 51 at ViT-H
    and B <= 85 at ViT-B for every precision; the attention operands' 4 GiB limit binds first where windows pad heavily — dim
    256, 4 heads, grid 64, window 20: Q' = B 16 4 416 2 192 2 bytes >= 2^32 from B = 211, the GEMM limit only from B = 256 —
    and holds for the f16 routes only (the fp32 route keeps no operand planes: the same set as before).  A window side above 64
    has no kernel (workspace size 0).  The relative-position task count (2^31) and the fp32 kernel's LDS size (window side 88)
    lie behind these limits and cannot be reached through the ABI."""
    from pope_amd import _lib
    ERR_ARG, ERR_WORKSPACE = -1, -3
    ok = 1 << 12

    def forward(arch, window, B):
        w = _encoder_weights(*arch, window, precision=_lib.PRECISIONS[precision], pointer=ok)
        return hip_lib.pope_sam_encoder_forward_f32(ctypes.byref(w), ok, B, ok, 0, None, None, ok, 1, None, None)

    assert forward(VIT_H, 14, 51) == ERR_WORKSPACE and forward(VIT_H, 14, 52) == ERR_ARG
    assert forward(VIT_B, 14, 85) == ERR_WORKSPACE and forward(VIT_B, 14, 86) == ERR_ARG
    padded = (256, 1, 4, 1024)
    assert forward(padded, 20, 210) == ERR_WORKSPACE
    assert forward(padded, 20, 211) == (ERR_WORKSPACE if precision == "f32" else ERR_ARG)
    assert forward(padded, 20, 255) == (ERR_WORKSPACE if precision == "f32" else ERR_ARG)
    assert forward(padded, 20, 256) == ERR_ARG
    assert forward(VIT_B, 70, 1) == ERR_ARG
