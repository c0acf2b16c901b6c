"""GPU: the launch sequence of the ViT forward (vit_forward.hip), route by route.

The profiled forward records the kind of every launch; the expected sequences below are written out from the design (DESIGN §2,
finding 26), not taken from a run:
  * fused route (dim 384, f16x3, batches past the `small` switch): every residual GEMM emits the LayerNorm that follows it, so
    PATCH_EMBED, then QKV, ATTENTION, PROJ, FC1, FC2 per block, then the close marker: 1 + 5 * depth launches;
  * every other route: PATCH_EMBED, then LAYERNORM, QKV, ATTENTION, PROJ, LAYERNORM, FC1, FC2 per block, the final LAYERNORM, the
    close marker: pope_vit_launch_count(depth) launches.
The unprofiled forward with taps at blocks 0 and 1 must hand out the x_prenorm of the depth-1 and of the depth-2 model, bit for
bit: the block loop has one tap copy, after FC2, on every route.  Depth 2, the smallest shapes that reach each route."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEPTH = 2
NTOK = 257                      # 1 + (224 / 14)^2
PATCH_EMBED, LAYERNORM, QKV, ATTENTION, PROJ, FC1, FC2, CLOSE = 0, 1, 2, 3, 4, 5, 6, -1   # pope_hip.h POPE_K_*
FUSED = [PATCH_EMBED] + [QKV, ATTENTION, PROJ, FC1, FC2] * DEPTH + [CLOSE]
UNFUSED = [PATCH_EMBED] + [LAYERNORM, QKV, ATTENTION, PROJ, LAYERNORM, FC1, FC2] * DEPTH + [LAYERNORM, CLOSE]

# route: (dim, precision, ffn, batch: 1 image, or "fused" = the smallest batch past the `small` switch, expected kinds)
ROUTES = {
    "fp32": (384, "f32", "mlp", 1, UNFUSED),
    "planes-small": (384, "f16x3", "mlp", 1, UNFUSED),
    "planes-fused": (384, "f16x3", "mlp", "fused", FUSED),
    "planes-unfused": (768, "f16x3", "mlp", 1, UNFUSED),
    "plain-f16-384": (384, "f16", "mlp", 1, UNFUSED),
    "plain-f16-768": (768, "f16", "mlp", 1, UNFUSED),
    "swiglu-small": (384, "f16x3", "swiglu", 1, UNFUSED),
    "swiglu-fused": (384, "f16x3", "swiglu", "fused", FUSED),
}


@pytest.fixture(scope="module")
def cu(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cdiv(a, b):
    return -(-a // b)


def _fused_batch(cu):
    """vit_forward.hip `small`: 3 * ceil(rows / 128) <= 2 * CUs keeps the unfused twin; the smallest batch of 224^2 images past it."""
    B = 1
    while 3 * _cdiv(B * NTOK, 128) <= 2 * cu:
        B += 1
    return B


def _model(sd, dim, depth, ffn, prec):
    from pope_amd import dinov2
    m = dinov2.DinoVisionTransformer(embed_dim=dim, depth=depth, num_heads=dim // 64, mlp_ratio=4, patch_size=14, img_size=518,
                                     init_values=1e-5, ffn_layer="swiglufused" if ffn == "swiglu" else "mlp", block_chunks=0)
    m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("blocks.") or int(k.split(".")[1]) < depth}, strict=True)
    m.precision = prec
    return m.eval().to("cuda:0")


@pytest.mark.parametrize("route", list(ROUTES))
def test_launch_sequence_and_taps(hip_lib, cu, route):
    from pope_amd import profiling, synth
    dim, prec, ffn, batch, want = ROUTES[route]
    B = _fused_batch(cu) if batch == "fused" else 1
    assert (3 * _cdiv(B * NTOK, 128) > 2 * cu) == (batch == "fused")
    assert len(UNFUSED) - 1 == hip_lib.pope_vit_launch_count(DEPTH) and len(FUSED) - 1 == 1 + 5 * DEPTH
    sd = synth.synthetic_state_dict(seed=11, dim=dim, depth=DEPTH, ffn=ffn)
    x = synth.synthetic_images(B, 224, 224, seed=5).cuda()
    m = _model(sd, dim, DEPTH, ffn, prec)
    prof = profiling.KernelProfiler(DEPTH, 1)
    try:
        m.profiler = prof
        out = m(x, is_training=True)
        torch.cuda.synchronize()
        (off, n), = prof.launches
        got = list(prof.kinds[off:off + n + 1])
    finally:
        m.profiler = None
        prof.close()
    print(f"{route}: B {B}, {n} launches, kinds {got}")
    assert m.overflow_events == 0
    assert got == want, (route, got)
    # the unprofiled forward with taps: block i's tap is the x_prenorm of the model cut after block i
    pre, _, taps = m._run(x, taps=[0, 1])
    one = _model(sd, dim, 1, ffn, prec)(x, is_training=True)["x_prenorm"]
    assert m.overflow_events == 0 and bool(torch.isfinite(pre).all())
    assert torch.equal(taps[0], one), "tap of block 0"
    assert torch.equal(taps[1], out["x_prenorm"]) and torch.equal(pre, out["x_prenorm"]), "tap of block 1"
