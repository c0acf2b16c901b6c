"""GPU: the SAM encoder's attention at every window side where `pope_sam_attn_plan` / `pope_sam_attn_block`
(sam_attention.hip) switch kernels, against oracle/sam_encoder_ref.py evaluated in float64 on the CPU.

The shipped models and fixtures run window sides 7, 14, 15, 16 and 64 only, and 64 x 64 global blocks take the bias table, so
the deep score depth (NSTEP 12 / 13), the 8-wave workgroup without the bias table, the second column block of
`sam_attn_relpos_kernel` (MB = 2) without TAB and its dword-tail / 2-byte stores with MB = 2 are reached by nothing else.
Every case is a ONE-block ImageEncoderViT (so the attention output is one projection away from the residual stream read
through `forward_with_taps`), at the smallest grid on either side of each switch:

    g   window  smallest case of
    16  global  last shallow score depth (NSTEP 6 / 7)
    17  global  first deep score depth (NSTEP 12 / 13); odd side (2-byte stores); Nq 289 in Npad 320 (masked keys, dead rows)
    32  global  last 4-wave and last MB = 1 case; Nq = Npad = 1024: no key masked
    33  global  first 8-wave and first MB = 2 case; odd side; Npad 1120
    34  20      deep depth with padded windows (nw = 2, 34 -> 40: pad tokens carry k = v = bias); even side, dword tail
    48  global  MB = 2 with ws % 8 == 0 (16-byte stores in both column blocks); 8 waves, several query blocks per group
    63  global  last case without the bias table: the widened columns reach hd + 126 of 192 / 208; odd side
    64  global  the bias-table route (the neighbour of 63)

(Rows 17, 33, 34 / 20 and 63 are also the only ones with a deep score depth AND a token count that is no multiple of the
QKV GEMM's row tile: there the epilogue's dropped rows once wrote their lo halves into key 0 of the first window — see
EPI_SAM_QKV in gemm_planes.hip — which the f16x3 cases and the batch-of-two test both catch.)

Bounds.  f16x3 and f32 are fp32-level arithmetic: the residual stream must be as close to the float64 result as the
reference's own fp32 chain is (the rule of test_gpu_loftr.py: 4 x its error + 2e-5) and within test_gpu_sam.py's ATOL_X /
ATOL_OUT of the fp32 oracle.  f16 is held on the neck output to test_gpu_sam.py's ATOL_F16 (max) and ATOL_F16 / 10 (mean); its
residual-stream error is printed only (the project has no f16 bound for it).

That these bounds can fail is a property of the INPUTS, checked on the CPU before the GPU runs anything: zeroing one row of
`rel_pos_w` (the last) or of `rel_pos_h` (the first) — one relative offset, the footprint of a single mis-stored or
mis-indexed relative-position column — moves the float64 residual stream by at least 10 x ATOL_X and the float64 neck
output by at least 2 x ATOL_F16 in every case (`reference`)."""
import functools
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu
ATOL_OUT, ATOL_X, ATOL_F16 = 1e-4, 2e-4, 2e-2   # the constants of tests/test_gpu_sam.py
W_SEED, X_SEED, X2_SEED = 1, 2, 12
ARCH = {64: (256, 4), 80: (640, 8)}               # head_dim -> (embed_dim, heads)
GEOMS = [(16, 0), (17, 0), (32, 0), (33, 0), (34, 20), (48, 0), (63, 0), (64, 0)]   # (token grid side, window; 0 = global)
CASES = [pytest.param(hd, g, win, id=f"hd{hd}-g{g}-w{win}") for hd in ARCH for g, win in GEOMS]
ODD_CASES = [pytest.param(hd, g, 0, id=f"hd{hd}-g{g}-w0") for hd in ARCH for g in (17, 33)]
PROBES = (("blocks.0.attn.rel_pos_w", -1), ("blocks.0.attn.rel_pos_h", 0))


def state_dict(hd, g, window):
    from pope_amd import synth
    dim, heads = ARCH[hd]
    return synth.synthetic_sam_encoder_state_dict(seed=W_SEED, dim=dim, depth=1, heads=heads, grid=g, window=window or g, global_idx=())


def oracle(sd, x, hd, window, dtype):
    """(residual stream after block 0, neck output) of the oracle in `dtype`."""
    from oracle import sam_encoder_ref
    taps = {0: None}
    with torch.no_grad():
        out = sam_encoder_ref.forward({k: v.to(dtype) for k, v in sd.items()}, x.to(dtype), ARCH[hd][1], window, (), taps=taps)
    return taps[0], out


@functools.lru_cache(maxsize=None)
def reference(hd, g, window):
    """Weights, one input image and the oracle's answers for one geometry: computed once, shared by every precision, read only.
    Asserts the sensitivity floor (module docstring) on the way."""
    from pope_amd import synth
    sd = state_dict(hd, g, window)
    x = synth.synthetic_images(1, 16 * g, 16 * g, seed=X_SEED)
    w_tap, w_out = oracle(sd, x, hd, window, torch.float64)
    r_tap, r_out = oracle(sd, x, hd, window, torch.float32)
    moved = []
    for key, row in PROBES:
        probe = dict(sd)
        probe[key] = sd[key].clone()
        probe[key][row] = 0.0
        p_tap, p_out = oracle(probe, x, hd, window, torch.float64)
        d_tap, d_out = float((p_tap - w_tap).abs().max()), float((p_out - w_out).abs().max())
        moved.append((d_tap, d_out))
        assert d_tap >= 10 * ATOL_X and d_out >= 2 * ATOL_F16, (hd, g, window, key, row, d_tap, d_out)
    e_ref = float((r_tap.double() - w_tap).abs().max())
    print(f"hd{hd} g{g} w{window}: fp32 oracle vs fp64 {e_ref:.2e}, |tap| max {float(w_tap.abs().max()):.2f}; one rel_pos_w row moves "
          f"tap / out by {moved[0][0]:.3f} / {moved[0][1]:.3f}, one rel_pos_h row by {moved[1][0]:.3f} / {moved[1][1]:.3f}")
    return dict(sd=sd, x=x, w_tap=w_tap, r_tap=r_tap, r_out=r_out, e_ref=e_ref)


def encoder(hd, g, window, sd, precision="f16x3"):
    from pope_amd.sam_encoder import ImageEncoderViT
    dim, heads = ARCH[hd]
    m = ImageEncoderViT(depth=1, embed_dim=dim, img_size=16 * g, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                        num_heads=heads, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=[], window_size=window,
                        out_chans=256)
    m.load_state_dict(sd, strict=True)
    m.precision = precision
    return m.eval().cuda()


def run_case(hd, g, window, precision):
    ref = reference(hd, g, window)   # the CPU side, its sensitivity floor included, before the GPU is touched
    m = encoder(hd, g, window, ref["sd"], precision)
    with torch.no_grad():
        out, (tap,) = m.forward_with_taps(ref["x"].cuda(), [0])
    torch.cuda.synchronize()
    out, tap = out.cpu(), tap.cpu()
    e_hip = float((tap.double() - ref["w_tap"]).abs().max())
    e_vs_ref = float((tap - ref["r_tap"]).abs().max())
    err = (out - ref["r_out"]).abs()
    print(f"hd{hd} g{g} w{window} [{precision}]: tap max err vs fp64 oracle: HIP {e_hip:.2e}, fp32 oracle {ref['e_ref']:.2e}; HIP vs fp32 "
          f"oracle {e_vs_ref:.2e}; out vs fp32 oracle max {float(err.max()):.2e}, mean {float(err.mean()):.2e}")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(tap).all())
    assert m.overflow_events == 0
    return e_hip, e_vs_ref, err, ref["e_ref"]


@pytest.mark.parametrize("hd,g,window", CASES)
def test_f16x3_matches_fp64_oracle(hip_lib, hd, g, window):
    e_hip, e_vs_ref, err, e_ref = run_case(hd, g, window, "f16x3")
    assert e_hip < 4 * e_ref + 2e-5          # as close to the exact result as the reference's own fp32 chain
    assert e_vs_ref <= ATOL_X
    assert float(err.max()) <= ATOL_OUT


@pytest.mark.parametrize("hd,g,window", CASES)
def test_f16_matches_oracle(hip_lib, hd, g, window):
    _, _, err, _ = run_case(hd, g, window, "f16")
    assert float(err.max()) <= ATOL_F16 and float(err.mean()) <= ATOL_F16 / 10


@pytest.mark.parametrize("hd,g,window", ODD_CASES)
def test_f32_twin_matches_fp64_oracle(hip_lib, hd, g, window):
    """The fp32 route (sam.hip's sequence on sam_f32.hip's kernels: what a range-guard event re-runs on) at the first deep-depth and the first 8-wave side."""
    e_hip, e_vs_ref, err, e_ref = run_case(hd, g, window, "f32")
    assert e_hip < 4 * e_ref + 2e-5
    assert e_vs_ref <= ATOL_X
    assert float(err.max()) <= ATOL_OUT


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("hd,g,window", ODD_CASES)
def test_batch_of_two_is_bit_equal_to_single_runs(hip_lib, hd, g, window, precision):
    """B = 2 at the odd sides: the group and row arithmetic of the attention kernels (`grp`, `wb`, `row_of`) with more than one
    image — image 1 of the batch is bit-equal to its own run, residual stream and neck output."""
    from pope_amd import synth
    m = encoder(hd, g, window, state_dict(hd, g, window), precision)
    x = synth.synthetic_images(2, 16 * g, 16 * g, seed=X2_SEED).cuda()
    with torch.no_grad():
        out2, (tap2,) = m.forward_with_taps(x, [0])
        out1, (tap1,) = m.forward_with_taps(x[1:2].contiguous(), [0])
    assert bool(torch.isfinite(out2).all()) and m.overflow_events == 0
    assert not torch.equal(out2[0], out2[1])
    assert torch.equal(tap2[1], tap1[0]) and torch.equal(out2[1], out1[0])


@pytest.mark.parametrize("g", [64, 33])
def test_rel_pos_table_outside_the_f16_range(hip_lib, g):
    """`sam_attn_relpos_kernel` splits the gathered tables times 256 into f16: |rel_pos| < 255.9 is part of the f16x3 range
    contract like every Linear weight.  One entry of 300 (bias-table route at g = 64, widened columns at g = 33): the default
    policy warns and the call gives exactly what precision "f32" gives; "raise" raises."""
    from pope_amd import synth
    from pope_amd.dinov2 import PopeRangeError
    sd = dict(state_dict(64, g, 0))
    sd["blocks.0.attn.rel_pos_h"] = sd["blocks.0.attn.rel_pos_h"].clone()
    sd["blocks.0.attn.rel_pos_h"][g - 1, 3] = 300.0   # offset 0: every query line reads it
    x = synth.synthetic_images(1, 16 * g, 16 * g, seed=X_SEED).cuda()
    m = encoder(64, g, 0, sd)
    with torch.no_grad(), pytest.warns(UserWarning, match="f32|fp32"):
        got = m(x)
    assert m.overflow_events == 1
    m.precision = "f32"
    with torch.no_grad():
        want = m(x)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    m.precision = "f16x3"
    m.on_overflow = "raise"
    m._wcache = {}
    with torch.no_grad(), pytest.raises(PopeRangeError):
        m(x)
