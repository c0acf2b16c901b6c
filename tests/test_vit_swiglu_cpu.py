"""CPU: the SwiGLU FFN surface of the drop-in DinoVisionTransformer (ViT-g/14) — state-dict layout against the reference
module's recorded key list, the hidden-size rule, the w12 row permutation of the fused GEMM, argument checks of the new C
entry points, and an fp64 restatement of the SwiGLU block (`restate`) held to the reference fixtures
(scripts/gen_golden_vit_swiglu.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pope_amd import _lib, dinov2, synth

CASES = ["vits_swiglu_224", "vitg_224"]
EVAL_CFG = dict(patch_size=14, img_size=518, init_values=1e-5, ffn_layer="swiglufused", block_chunks=0)


def build(fx, device=None):
    dim, depth, heads = (int(v) for v in fx["arch"])
    ctx = torch.device(device) if device else torch.device("cpu")
    with ctx:
        if (dim, depth, heads) == (1536, 40, 24):
            return dinov2.build_vitg14()
        return dinov2.DinoVisionTransformer(embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4, **EVAL_CFG)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_layout_equals_the_reference(golden_dir, name):
    """Key names and shapes equal the reference module's own list (recorded by the fixture generator).  The giant is built on
    the meta device: 1.1 G parameters."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    keys = bytes(fx["keys"]).decode().split("\n")
    shapes = {k: tuple(int(v) for v in row[:max(1, int(np.count_nonzero(row)))]) for k, row in zip(keys, fx["shapes"])}
    m = build(fx, "meta")
    sd = m.state_dict()
    assert sorted(sd) == keys
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert any(k.endswith("mlp.w12.weight") for k in keys) and not any(".fc1." in k for k in keys)


def test_strict_loading_of_a_reference_layout_state_dict():
    m = dinov2.DinoVisionTransformer(embed_dim=384, depth=2, num_heads=6, mlp_ratio=4, **EVAL_CFG)
    sd = synth.synthetic_state_dict(seed=0, dim=384, depth=2, ffn="swiglu")
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.blocks[1].mlp.w12.weight, sd["blocks.1.mlp.w12.weight"])
    with pytest.raises(RuntimeError):   # an MLP checkpoint does not fit
        m.load_state_dict(synth.synthetic_state_dict(seed=0, dim=384, depth=2), strict=True)
    for kind in ("swiglu", "swiglufused"):   # vision_transformer.py:112-114: both names select the fused FFN
        assert isinstance(dinov2.DinoVisionTransformer(embed_dim=384, depth=1, num_heads=6, ffn_layer=kind).blocks[0].mlp,
                          dinov2._SwiGLUFFN)
    with pytest.raises(NotImplementedError):
        dinov2.DinoVisionTransformer(embed_dim=384, depth=1, num_heads=6, ffn_layer="identity")
    assert dinov2.vit_giant2.__name__ == "vit_giant2" and dinov2.build_vitg14.keywords["ffn_layer"] == "swiglufused"


def test_hidden_size_rule():
    """swiglu_ffn.py:57 behind block.py:69."""
    for dim, h in ((384, 1024), (768, 2048), (1536, 4096)):
        assert dinov2.swiglu_hidden(dim, 4) == h
        with torch.device("meta"):
            m = dinov2.DinoVisionTransformer(embed_dim=dim, depth=1, num_heads=dim // 64, mlp_ratio=4, ffn_layer="swiglufused")
        assert m.ffn_hidden == h and tuple(m.blocks[0].mlp.w12.weight.shape) == (2 * h, dim)
    with pytest.raises(NotImplementedError, match="2736"):   # no multiple of 64: out of scope, said at construction
        dinov2.DinoVisionTransformer(embed_dim=1024, depth=1, num_heads=16, mlp_ratio=4, ffn_layer="swiglufused")


def test_f16_precision_with_swiglu_raises():
    m = dinov2.DinoVisionTransformer(embed_dim=384, depth=1, num_heads=6, mlp_ratio=4, **EVAL_CFG)
    m.precision = "f16"
    with pytest.raises(NotImplementedError, match="f16.*SwiGLU"):
        m._weights()
    assert m._weights("f32").hidden == 1024   # the other modes build


def test_w12_permutation_is_a_bijection_and_invertible():
    for h in (64, 1024, 4096):
        perm = dinov2.swiglu_permutation(h)
        assert perm.shape == (2 * h,) and torch.equal(perm.sort().values, torch.arange(2 * h))
        blk = perm.view(-1, 2, 32)   # per 64 rows: 32 gates of consecutive hidden columns, then their values
        assert torch.equal(blk[:, 1], blk[:, 0] + h) and torch.equal(blk[:, 0].reshape(-1), torch.arange(h))
    m = dinov2.DinoVisionTransformer(embed_dim=384, depth=1, num_heads=6, mlp_ratio=4, **EVAL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(seed=3, dim=384, depth=1, ffn="swiglu"), strict=True)
    w, b = m._ffn_first(m.blocks[0])
    perm = dinov2.swiglu_permutation(1024)
    back_w, back_b = torch.empty_like(w), torch.empty_like(b)
    back_w[perm], back_b[perm] = w, b
    assert torch.equal(back_w, m.blocks[0].mlp.w12.weight) and torch.equal(back_b, m.blocks[0].mlp.w12.bias)


def test_weight_cache_follows_w12_edits():
    """As tests/test_loader_cpu.py demands of the MLP weights: in-place edits and replaced Parameter objects rebuild the
    derived (permuted) tensors; an unchanged model hits the cache."""
    m = dinov2.DinoVisionTransformer(embed_dim=384, depth=2, num_heads=6, mlp_ratio=4, **EVAL_CFG)
    w0 = m._weights("f32")
    assert m._weights("f32") is w0
    with torch.no_grad():
        m.blocks[1].mlp.w12.weight[5, 7] += 0.5
    w1 = m._weights("f32")
    assert w1 is not w0
    m.blocks[0].mlp.w12.weight = torch.nn.Parameter(m.blocks[0].mlp.w12.weight.detach() * 0.5)
    w2 = m._weights("f32")
    assert w2 is not w1 and m._weights("f32") is w2
    perm = dinov2.swiglu_permutation(1024)
    held = m._wcache["f32"][3]   # the derived tensors the struct points at
    assert any(t.shape == (2048, 384) and torch.equal(t, m.blocks[0].mlp.w12.weight.detach()[perm]) for t in held)


def test_synthetic_state_dict_default_is_unchanged(golden_dir, golden_threads):
    """Nothing moved for the MLP archs: the default recipe still has the digest the ViT-L fixture stores."""
    fx = np.load(os.path.join(golden_dir, "vitl_224.npz"))
    dim, depth, _ = (int(v) for v in fx["arch"])
    sd = synth.synthetic_state_dict(seed=int(fx["weights_seed"]), dim=dim, depth=depth)
    assert np.array_equal(np.array([float(sd[k].double().sum()) for k in sorted(sd)]), fx["weights_digest"])
    sw = synth.synthetic_state_dict(seed=0, dim=384, depth=1, ffn="swiglu")
    assert tuple(sw["blocks.0.mlp.w12.weight"].shape) == (2048, 384) and tuple(sw["blocks.0.mlp.w3.weight"].shape) == (384, 1024)
    assert abs(float(sw["blocks.0.mlp.w3.weight"].std()) * math.sqrt(1024) - 1) < 0.02


# ---- fp64 restatement ---------------------------------------------------------------------------------------------------
def swiglu_block(sd, i, x, heads):
    """block.py:105-106 with SwiGLUFFNFused (swiglu_ffn.py:29-33), eval branch, in x's dtype; weights converted per block."""
    def p(k):
        return sd[f"blocks.{i}.{k}"].to(x.dtype)
    B, N, dim = x.shape
    n1 = F.layer_norm(x, (dim,), p("norm1.weight"), p("norm1.bias"), 1e-6)
    qkv = F.linear(n1, p("attn.qkv.weight"), p("attn.qkv.bias")).reshape(B, N, 3, heads, dim // heads).permute(2, 0, 3, 1, 4)
    a = ((qkv[0] * (dim // heads) ** -0.5) @ qkv[1].transpose(-2, -1)).softmax(-1)
    o = (a @ qkv[2]).transpose(1, 2).reshape(B, N, dim)
    x = x + F.linear(o, p("attn.proj.weight"), p("attn.proj.bias")) * p("ls1.gamma")
    n2 = F.layer_norm(x, (dim,), p("norm2.weight"), p("norm2.bias"), 1e-6)
    x1, x2 = F.linear(n2, p("mlp.w12.weight"), p("mlp.w12.bias")).chunk(2, dim=-1)
    hidden = x1 / (1 + torch.exp(-x1)) * x2
    return x + F.linear(hidden, p("mlp.w3.weight"), p("mlp.w3.bias")) * p("ls2.gamma")


@torch.no_grad()
def restate(sd, x, heads, depth, taps):
    """vision_transformer.py:191-236 in fp64 (the bicubic position table in fp32, as the fp32 reference computes it)."""
    from oracle import dinov2_ref
    B, _, H, W = x.shape
    patch = sd["patch_embed.proj.weight"].shape[-1]
    t = F.conv2d(x.double(), sd["patch_embed.proj.weight"].double(), sd["patch_embed.proj.bias"].double(), stride=patch)
    t = torch.cat((sd["cls_token"].double().expand(B, -1, -1), t.flatten(2).transpose(1, 2)), dim=1)
    t = t + dinov2_ref.interpolate_pos_encoding(sd["pos_embed"], t.shape[1], H, W, patch).double()
    out = {}
    for i in range(depth):
        t = swiglu_block(sd, i, t, heads)
        if i in taps:
            out[f"blk{i}"] = t
    out["x_prenorm"] = t
    out["x_norm"] = F.layer_norm(t, (t.shape[-1],), sd["norm.weight"].double(), sd["norm.bias"].double(), 1e-6)
    return out


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_matches_reference_fixture(golden_dir, golden_threads, name):
    """Bound: max(2e-5, 4 x the reference's own fp32-vs-fp64 error) — 2e-5 is what oracle/gen_golden.py holds the oracle to."""
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    dim, depth, heads = (int(v) for v in fx["arch"])
    sd = synth.synthetic_state_dict(seed=int(fx["weights_seed"]), dim=dim, depth=depth, ffn="swiglu")
    assert np.array_equal(np.array([float(sd[k].double().sum()) for k in sorted(sd)]), fx["weights_digest"])
    B, H, W = (int(v) for v in fx["shape"])
    x = synth.synthetic_images(B, H, W, seed=int(fx["input_seed"]))
    assert float(x.double().sum()) == fx["input_digest"][0]
    taps = [int(t) for t in fx["tap_blocks"]]
    got = restate(sd, x, heads, depth, taps)
    bound = max(2e-5, 4 * float(fx["ref_fp32_err"]))
    rows = torch.from_numpy(fx["rows"])
    for k in ["x_norm", "x_prenorm"] + [f"blk{i}" for i in taps]:
        err = float(np.abs(got[k][:, rows].numpy() - fx[k]).max())
        print(f"{name} {k}: max |restate - reference| = {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (k, err, bound)
    np.testing.assert_allclose(got["x_norm"][:, 0].numpy(), fx["cls"], rtol=0, atol=bound)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_a_gpu(hip_lib):
    assert _lib.EPI_BIAS_SWIGLU == 11 and _lib.FFN_KINDS == {"mlp": 0, "swiglu": 1}
    one = C.c_void_p(256)   # a non-NULL pointer that is never dereferenced: every call below fails its argument check first
    # op level: NULL operands, N no multiple of 64, both / neither output, f16x3 through the on-the-fly entry
    assert hip_lib.pope_linear_planes_f32(None, None, None, None, None, 128, 2048, 384, 11, None, None, None, None) == -1
    assert hip_lib.pope_linear_planes_f32(one, one, None, None, one, 128, 2080, 384, 11, None, None, None, None) == -1
    assert hip_lib.pope_linear_planes_f32(one, one, None, one, one, 128, 2048, 384, 11, None, None, None, None) == -1
    assert hip_lib.pope_linear_planes_f32(one, one, None, None, None, 128, 2048, 384, 11, None, None, None, None) == -1
    assert hip_lib.pope_linear_planes_f32(one, one, None, None, one, 128, 2048, 384, 12, None, None, None, None) == -1
    assert hip_lib.pope_linear_f32(None, None, None, None, 128, 2048, 384, 11, None, None, 0, None, None) == -1
    assert hip_lib.pope_linear_f32(one, one, None, one, 128, 2080, 384, 11, None, None, 0, None, None) == -1
    assert hip_lib.pope_linear_f32(one, one, None, one, 128, 2048, 384, 11, None, None, 1, None, None) == -1
    # whole model
    blocks = (_lib.VitBlockWeights * 1)()
    for n, _ in _lib.VitBlockWeights._fields_:
        setattr(blocks[0], n, 256)

    def weights(hidden=1024, precision=_lib.PREC_F16X3):
        return _lib.VitWeights(384, 1, 6, 14, hidden, one, one, one, blocks, precision, one)

    def call(w, ffn, img=one, ws=one):
        return hip_lib.pope_vit_forward_f32(C.byref(w) if w is not None else None, ffn, img, 1, 224, 224, one, one, one, 0,
                                            None, None, ws, 1 << 30, None, None)
    assert call(None, 1) == -1 and call(weights(), 1, img=None) == -1 and call(weights(), 1, ws=None) == -1
    assert call(weights(), 2) == -1 and call(weights(), -1) == -1                  # unknown FFN kind
    assert call(weights(precision=_lib.PREC_F16), 1) == -1                         # no plain-f16 SwiGLU
    assert call(weights(hidden=1000), 1) == -1                                     # hidden % 32
    blocks[0].fc1_b = None
    assert call(weights(), 1) == -1                                                # w12 bias missing
    blocks[0].fc1_b = 256
    ev = (C.c_void_p * 4)()
    kinds, n = (C.c_int * 4)(), C.c_int()
    assert hip_lib.pope_vit_forward_profiled_f32(C.byref(weights()), 1, one, 1, 224, 224, one, one, one, one, 1 << 30, None,
                                                 None, None, 4, kinds, C.byref(n), 0xffffffff) == -1   # no events
    assert hip_lib.pope_vit_forward_profiled_f32(C.byref(weights()), 3, one, 1, 224, 224, one, one, one, one, 1 << 30, None,
                                                 None, ev, 4, kinds, C.byref(n), 0xffffffff) == -1
