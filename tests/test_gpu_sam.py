"""GPU: SAM image encoder (BASELINE config 5) through the C ABI vs fixtures captured from the
reference's own ImageEncoderViT (oracle/gen_golden.py:gen_sam_encoder) and vs the CPU oracle.  Tolerance: the north
star's 1e-3 on descriptors; the neck output (LayerNorm2d, O(1)) is held to 1e-4 absolute, the residual stream
(|x| up to 12 after 32 blocks) to 2e-4 (measured at ViT-H / 1024 x 1024: 1.4e-5 and 3.0e-5)."""
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ATOL_OUT, ATOL_X = 1e-4, 2e-4


def build(fx, device="cuda:0"):
    from pope_amd import synth
    from pope_amd.sam_encoder import ImageEncoderViT
    dim, depth, heads, img, window = (int(v) for v in fx["arch"])
    gidx = tuple(int(v) for v in fx["global_idx"])
    m = ImageEncoderViT(depth=depth, embed_dim=dim, img_size=img, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                        num_heads=heads, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=list(gidx),
                        window_size=window, out_chans=256)
    sd = synth.synthetic_sam_encoder_state_dict(seed=int(fx["weights_seed"]), dim=dim, depth=depth, heads=heads, grid=img // 16,
                                                window=window, global_idx=gidx)
    digest = np.array([float(sd[k].double().sum()) for k in sorted(sd)], np.float64)
    # same seeded recipe on this box's CPU: the sums agree up to the last bits of the host's normal sampler
    np.testing.assert_allclose(digest, fx["weights_digest"], rtol=1e-5, atol=1e-3)
    m.load_state_dict(sd, strict=True)
    x = synth.synthetic_images(int(fx["batch"]), img, img, seed=int(fx["input_seed"]))
    np.testing.assert_allclose(float(x.double().sum()), fx["input_digest"][0], rtol=1e-9)
    return m.eval().to(device), x, sd


def check_against_fixture(m, x, fx, name):
    stride = int(fx["stride"])
    taps = [int(t) for t in fx["tap_blocks"]]
    out, blk = m.forward_with_taps(x.cuda(), taps)
    torch.cuda.synchronize()
    got = out[:, :, ::stride, ::stride].cpu().numpy()
    err = float(np.abs(got - fx["out"]).max())
    ts = max(2, stride)
    errs = {i: float(np.abs(t[:, ::ts, ::ts, ::2].cpu().numpy() - fx[f"blk{i}"]).max()) for i, t in zip(taps, blk)}
    print(f"{name}: max |out - reference| = {err:.2e}; residual stream " + ", ".join(f"blk{i} {e:.2e}" for i, e in errs.items()))
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, fx["out"], rtol=0, atol=ATOL_OUT)
    for i, e in errs.items():
        assert e <= ATOL_X, (i, e)
    assert m.overflow_events == 0
    return out


@pytest.mark.parametrize("name", ["sam_hd80_256", "sam_hd64_224"])
def test_small_encoders_match_reference_fixture(hip_lib, golden_dir, name):
    """head_dim 80 with padded windows (grid 16 -> 2 x 2 windows of 14: the pad tokens are keys with k = v = bias) and
    head_dim 64 with one exact window; both with global blocks and O(1) relative-position terms."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    m, x, _ = build(fx)
    out = check_against_fixture(m, x, fx, name)
    # batch invariance and determinism: image k of a larger batch is bit-equal to its own run
    from pope_amd import synth
    img = int(fx["arch"][3])
    x3 = torch.cat([synth.synthetic_images(2, img, img, seed=3), x[:1]]).cuda()
    assert torch.equal(m(x3)[2], out[0])
    assert torch.equal(m(x.cuda()), out)


def test_small_encoder_matches_cpu_oracle_on_fresh_input(hip_lib, golden_dir):
    """A second input (not in any fixture) against the oracle restatement, and a batch that spans two launch sequences."""
    from oracle import sam_encoder_ref
    from pope_amd import synth
    fx = np.load(os.path.join(golden_dir, "sam_hd80_256.npz"))
    m, _, sd = build(fx)
    dim, depth, heads, img, window = (int(v) for v in fx["arch"])
    x = synth.synthetic_images(3, img, img, seed=23)
    with torch.no_grad():
        want = sam_encoder_ref.forward(sd, x, heads, window, tuple(int(v) for v in fx["global_idx"]))
    m.max_batch = 2
    got = m(x.cuda()).cpu()
    err = float((got - want).abs().max())
    print(f"fresh input: max |out - oracle| = {err:.2e}")
    assert err <= ATOL_OUT


def test_vit_h_full_size_matches_reference_fixture(hip_lib, golden_dir):
    """build_sam.py:13-21 at full size: 1280-d, 32 blocks, 16 heads of 80, 1024 x 1024 input (64 x 64 tokens, 25 windows
    of 14 x 14 with padding 64 -> 70), global attention in blocks 7 / 15 / 23 / 31 over 4096 keys."""
    fx = np.load(os.path.join(golden_dir, "sam_vit_h_1024.npz"))
    m, x, _ = build(fx)
    check_against_fixture(m, x, fx, "sam_vit_h_1024")


def test_vit_b_full_size_matches_reference_fixture(hip_lib, golden_dir):
    """build_sam.py:36-45 at full size: 768-d, 12 heads of 64 — the head_dim-64 instantiations of the attention kernel
    with padded windows (score depth 96) and 4096-key global blocks (the bias-table route: score depth 64, the
    relative-position terms start the score accumulators instead of widening Q' / K')."""
    fx = np.load(os.path.join(golden_dir, "sam_vit_b_1024.npz"))
    m, x, _ = build(fx)
    check_against_fixture(m, x, fx, "sam_vit_b_1024")


# precision "f16" (BASELINE config 5's dtype): plain f16 operands, one MFMA per product.  Against the fp32 reference the
# error is f16 rounding through the depth of the model; held to 2e-2 on the O(1) neck output (measured values printed).
ATOL_F16 = 2e-2


@pytest.mark.parametrize("name", ["sam_hd80_256", "sam_hd64_224", "sam_vit_b_1024", "sam_vit_h_1024"])
def test_f16_precision_mode(hip_lib, golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    m, x, _ = build(fx)
    m.precision = "f16"
    stride = int(fx["stride"])
    out = m(x.cuda())
    got = out[:, :, ::stride, ::stride].cpu().numpy()
    err = np.abs(got - fx["out"])
    print(f"{name} [f16]: max |out - reference| = {err.max():.2e}, mean {err.mean():.2e}")
    assert np.isfinite(got).all() and err.max() <= ATOL_F16 and err.mean() <= ATOL_F16 / 10
    assert torch.equal(m(x.cuda()), out)                       # deterministic
    m.precision = "f16x3"                                      # both weight sets stay cached; modes do not leak into each other
    np.testing.assert_allclose(m(x.cuda())[:, :, ::stride, ::stride].cpu().numpy(), fx["out"], rtol=0, atol=ATOL_OUT)
    m.precision = "bf16"
    with pytest.raises(ValueError):
        m(x.cuda())


@pytest.mark.parametrize("variant", ["no_abs_no_rel_all_global", "windows_only"])
def test_constructor_variants_match_oracle(hip_lib, variant):
    """The switches build_sam.py leaves on (image_encoder.py:34-39): without absolute / relative position terms and with
    window_size = 0 (every block global), and with no global block at all — against the CPU oracle on seeded weights."""
    from oracle import sam_encoder_ref
    from pope_amd import synth
    from pope_amd.sam_encoder import ImageEncoderViT
    glob = variant == "no_abs_no_rel_all_global"
    dim, depth, heads, img, window = 256, 2, 4, 224, (0 if glob else 14)
    m = ImageEncoderViT(depth=depth, embed_dim=dim, img_size=img, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                        num_heads=heads, patch_size=16, qkv_bias=True, use_abs_pos=not glob, use_rel_pos=not glob,
                        global_attn_indexes=[], window_size=window, out_chans=256)
    sd = synth.synthetic_sam_encoder_state_dict(seed=3, dim=dim, depth=depth, heads=heads, grid=img // 16, window=window or img // 16,
                                                global_idx=())
    if glob:
        sd = {k: v for k, v in sd.items() if k != "pos_embed" and "rel_pos" not in k}
    m.load_state_dict(sd, strict=True)
    m = m.eval().cuda()
    x = synth.synthetic_images(2, img, img, seed=5)
    with torch.no_grad():
        want = sam_encoder_ref.forward(sd, x, heads, window, ())
    for prec, tol in (("f16x3", ATOL_OUT), ("f16", ATOL_F16)):
        m.precision = prec
        err = float((m(x.cuda()).cpu() - want).abs().max())
        print(f"{variant} [{prec}]: max |out - oracle| = {err:.2e}")
        assert err <= tol


def test_contract_errors(hip_lib, golden_dir):
    from pope_amd.sam_encoder import ImageEncoderViT
    fx = np.load(os.path.join(golden_dir, "sam_hd64_224.npz"))
    m, x, _ = build(fx)
    with pytest.raises(ValueError):
        m(x.cuda()[:, :, :208, :208])
    with pytest.raises(TypeError):
        m(x.cuda().half())
    assert m(x.cuda()[:0]).shape == (0, 256, 14, 14)
    # a weight edited IN PLACE is noticed (the derived planes are keyed by address + version of every parameter) ...
    with torch.no_grad():
        y0 = m(x.cuda()).clone()
        m.blocks[0].mlp.lin1.weight[0, 0] += 0.5
        y1 = m(x.cuda())
    assert not torch.equal(y0, y1)
    # ... and a weight set that leaves the f16x3 range is not silently mangled: it runs on the fp32 MFMA (or raises)
    from pope_amd.dinov2 import PopeRangeError
    with torch.no_grad():
        m.blocks[0].mlp.lin1.weight[0, 0] = 300.0
    with pytest.warns(UserWarning, match="precision='f32'"):
        y2 = m(x.cuda())
    assert bool(torch.isfinite(y2).all())
    m.on_overflow = "raise"
    m._wcache = {}
    with pytest.raises(PopeRangeError):
        m(x.cuda())


@pytest.mark.parametrize("name", ["sam_hd64_224", "sam_hd80_256", "sam_vit_b_1024", "sam_vit_h_1024"])
def test_fp32_mfma_twin_matches_reference_fixture(hip_lib, golden_dir, name):
    """precision = "f32" (sam.hip's sequence on sam_f32.hip's kernels: every contraction on the fp32 MFMA, a plain fp32 window / global attention with the
    decomposed relative-position terms, fp32 LayerNorm2d and convolutions): the reference module's own arithmetic — held to
    the same fixture bounds as f16x3 — and the path a range-guard event is re-run in."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    m, x, _ = build(fx)
    m.precision = "f32"
    with torch.no_grad():
        check_against_fixture(m, x, fx, name + " [f32]")
    # an activation outside the f16 range in the default mode: warning, fp32 re-run, the same answer as the f32 mode
    m.precision = "f16x3"
    xb = x.clone()
    xb[0, 0, 5, 5] = 3.0e4
    with torch.no_grad(), pytest.warns(UserWarning, match="fp32 MFMA"):
        got = m(xb.cuda())
    m.precision = "f32"
    with torch.no_grad():
        want = m(xb.cuda())
    assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and m.overflow_events == 1


def test_odd_window_and_odd_grid_match_oracle(hip_lib):
    """A 7 x 7 window on a 15 x 15 token grid (padded to 21, image_encoder.py:251-254) and a 15 x 15 global block: odd window
    sides put the w-axis relative-position columns on odd offsets (the 2-byte store path of `sam_attn_relpos_kernel`; the
    shipped models have 14 and 64) — against the CPU oracle on seeded weights, both precisions, two images."""
    from oracle import sam_encoder_ref
    from pope_amd import synth
    from pope_amd.sam_encoder import ImageEncoderViT
    dim, depth, heads, img, window, gidx = 256, 2, 4, 240, 7, (1,)
    m = ImageEncoderViT(depth=depth, embed_dim=dim, img_size=img, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                        num_heads=heads, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=list(gidx),
                        window_size=window, out_chans=256)
    sd = synth.synthetic_sam_encoder_state_dict(seed=6, dim=dim, depth=depth, heads=heads, grid=img // 16, window=window, global_idx=gidx)
    m.load_state_dict(sd, strict=True)
    m = m.eval().cuda()
    x = synth.synthetic_images(2, img, img, seed=9)
    with torch.no_grad():
        want = sam_encoder_ref.forward(sd, x, heads, window, gidx)
    for prec, tol in (("f16x3", ATOL_OUT), ("f16", ATOL_F16)):
        m.precision = prec
        err = float((m(x.cuda()).cpu() - want).abs().max())
        print(f"odd window [{prec}]: max |out - oracle| = {err:.2e}")
        assert err <= tol and m.overflow_events == 0


def test_default_norm_layer_eps_1e5(hip_lib):
    """ImageEncoderViT() with the reference constructor's default norm_layer (nn.LayerNorm: eps 1e-5, image_encoder.py:27)
    runs with that eps in the blocks and 1e-6 in the neck's LayerNorm2d (common.py:28) — against the oracle."""
    from oracle import sam_encoder_ref
    from pope_amd import synth
    from pope_amd.sam_encoder import ImageEncoderViT
    kw = dict(img_size=224, patch_size=16, embed_dim=256, depth=2, num_heads=4, out_chans=256, use_rel_pos=True, window_size=14,
              global_attn_indexes=(1,))
    m = ImageEncoderViT(**kw)
    assert m.block_eps == 1e-5 and m.neck_eps == 1e-6
    sd = synth.synthetic_sam_encoder_state_dict(seed=4, dim=256, depth=2, heads=4, grid=14, window=14, global_idx=(1,))
    m.load_state_dict(sd, strict=True)
    m = m.eval().cuda()
    x = synth.synthetic_images(1, 224, 224, seed=8)
    with torch.no_grad():
        got = m(x.cuda()).cpu()
        want = sam_encoder_ref.forward(sd, x, 4, 14, (1,), block_eps=1e-5)
        other = sam_encoder_ref.forward(sd, x, 4, 14, (1,), block_eps=1e-6)
    assert float((got - want).abs().max()) <= 1e-4 and float((got - other).abs().max()) > float((got - want).abs().max())


def test_f16_mode_is_batch_invariant_across_the_gemm_switch(hip_lib, golden_dir):
    """precision "f16": the small encoder (grid 16: 256 token rows per image) alone runs its Linear layers on the 128 x 128 tile
    kernel, a batch of eight (2 048 rows) on gemm_plain.hip's 256-row tiles — including the QKV projection whose epilogue
    writes the attention operand rows through the window row map (EPI_SAM_QKV).  Same accumulation order, same epilogue
    arithmetic: image k of the batch is bit-equal to its own run."""
    from pope_amd import synth
    fx = np.load(os.path.join(golden_dir, "sam_hd80_256.npz"))
    m, _, _ = build(fx)
    m.precision = "f16"
    m.max_batch = 8
    img = int(fx["arch"][3])
    x = synth.synthetic_images(8, img, img, seed=31).cuda()
    big = m(x)
    for k in (0, 3, 7):
        assert torch.equal(m(x[k:k + 1])[0], big[k]), k
    assert bool(torch.isfinite(big).all())
