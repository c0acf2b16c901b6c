"""SAM prompt encoder / mask decoder: host-side checks (no GPU), and the torch restatement the GPU tests compare against,
pinned here to the reference's own outputs (tests/golden/sam_decoder.npz, scripts/gen_golden_sam_decoder.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pope_amd import _lib, synth
from pope_amd.sam_decoder import MaskDecoder, PromptEncoder, TwoWayTransformer

ROW_TAP, KEY_TAP, PE_TAP = 67, 203, 21   # scripts/gen_golden_sam_decoder.py


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sam_decoder.npz"))


def build_models(sd=None):
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024), mask_in_chans=16)
    md = MaskDecoder(transformer_dim=256, transformer=TwoWayTransformer(depth=2, embedding_dim=256, num_heads=8, mlp_dim=2048),
                     num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256)
    if sd is not None:
        pe.load_state_dict({k[len("prompt_encoder."):]: v for k, v in sd.items() if k.startswith("prompt_encoder.")}, strict=True)
        md.load_state_dict({k[len("mask_decoder."):]: v for k, v in sd.items() if k.startswith("mask_decoder.")}, strict=True)
    return pe, md


# ---- torch restatement (prompt_encoder.py, mask_decoder.py, transformer.py) ------------------------------------------
def dense_pe(sd, dtype=torch.float32):
    g = sd["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"].to(dtype)
    grid = torch.ones((64, 64), dtype=dtype, device=g.device)
    y = (grid.cumsum(dim=0) - 0.5) / 64
    x = (grid.cumsum(dim=1) - 0.5) / 64
    c = 2 * torch.stack([x, y], dim=-1) - 1
    c = 2 * np.pi * (c @ g)
    return torch.cat([torch.sin(c), torch.cos(c)], dim=-1).permute(2, 0, 1).unsqueeze(0)


def _attention(w, p, q, k, v, heads=8):
    q = F.linear(q, w[p + "q_proj.weight"], w[p + "q_proj.bias"])
    k = F.linear(k, w[p + "k_proj.weight"], w[p + "k_proj.bias"])
    v = F.linear(v, w[p + "v_proj.weight"], w[p + "v_proj.bias"])

    def sep(x):
        b, n, c = x.shape
        return x.reshape(b, n, heads, c // heads).transpose(1, 2)
    q, k, v = sep(q), sep(k), sep(v)
    attn = torch.softmax(q @ k.permute(0, 1, 3, 2) / math.sqrt(q.shape[-1]), dim=-1)
    out = (attn @ v).transpose(1, 2)
    out = out.reshape(out.shape[0], out.shape[1], -1)
    return F.linear(out, w[p + "out_proj.weight"], w[p + "out_proj.bias"])


def _ln(w, p, x, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), w[p + "weight"], w[p + "bias"], eps)


def _mlp(w, p, x, n=3):
    for i in range(n):
        x = F.linear(x, w[f"{p}layers.{i}.weight"], w[f"{p}layers.{i}.bias"])
        x = F.relu(x) if i < n - 1 else x
    return x


def restate(sd, image, image_pe, sparse, dense, multimask, dtype=torch.float32, chunk=32):
    """MaskDecoder.forward in torch at `dtype`, `chunk` prompts at a time: (masks, iou_pred, hs, keys)."""
    dev = image.device
    w = {k[len("mask_decoder."):]: v.to(device=dev, dtype=dtype) for k, v in sd.items() if k.startswith("mask_decoder.")}
    image, image_pe = image.to(dtype), image_pe.to(dtype)
    outs = []
    for s in range(0, sparse.shape[0], chunk):
        sp = sparse[s:s + chunk].to(dtype)
        dn = (dense[s:s + chunk] if dense.shape[0] > 1 else dense).to(dtype)
        P = sp.shape[0]
        out_tok = torch.cat([w["iou_token.weight"], w["mask_tokens.weight"]], 0).unsqueeze(0).expand(P, -1, -1)
        tokens = torch.cat((out_tok, sp), dim=1)
        src = torch.repeat_interleave(image, P, dim=0) + dn
        pos = torch.repeat_interleave(image_pe, P, dim=0).flatten(2).permute(0, 2, 1)
        keys = src.flatten(2).permute(0, 2, 1)
        queries = tokens
        for i in range(2):
            p = f"transformer.layers.{i}."
            if i == 0:
                queries = _attention(w, p + "self_attn.", queries, queries, queries)
            else:
                q = queries + tokens
                queries = queries + _attention(w, p + "self_attn.", q, q, queries)
            queries = _ln(w, p + "norm1.", queries)
            queries = _ln(w, p + "norm2.", queries + _attention(w, p + "cross_attn_token_to_image.", queries + tokens, keys + pos, keys))
            h = F.relu(F.linear(queries, w[p + "mlp.lin1.weight"], w[p + "mlp.lin1.bias"]))
            queries = _ln(w, p + "norm3.", queries + F.linear(h, w[p + "mlp.lin2.weight"], w[p + "mlp.lin2.bias"]))
            keys = _ln(w, p + "norm4.", keys + _attention(w, p + "cross_attn_image_to_token.", keys + pos, queries + tokens, queries))
        queries = queries + _attention(w, "transformer.final_attn_token_to_image.", queries + tokens, keys + pos, keys)
        hs = _ln(w, "transformer.norm_final_attn.", queries)
        x = keys.transpose(1, 2).reshape(P, 256, 64, 64)
        x = F.conv_transpose2d(x, w["output_upscaling.0.weight"], w["output_upscaling.0.bias"], stride=2)
        u = x.mean(1, keepdim=True)
        x = (x - u) / torch.sqrt((x - u).pow(2).mean(1, keepdim=True) + 1e-6)
        x = w["output_upscaling.1.weight"][:, None, None] * x + w["output_upscaling.1.bias"][:, None, None]
        x = F.gelu(x)
        x = F.gelu(F.conv_transpose2d(x, w["output_upscaling.3.weight"], w["output_upscaling.3.bias"], stride=2))
        hyper = torch.stack([_mlp(w, f"output_hypernetworks_mlps.{i}.", hs[:, 1 + i, :]) for i in range(4)], dim=1)
        masks = (hyper @ x.reshape(P, 32, -1)).reshape(P, -1, 256, 256)
        iou = _mlp(w, "iou_prediction_head.", hs[:, 0, :])
        sl = slice(1, None) if multimask else slice(0, 1)
        outs.append((masks[:, sl], iou[:, sl], hs, keys))
    return tuple(torch.cat([o[i] for o in outs]) for i in range(4))


def fixture_inputs(g, name, device="cpu"):
    """(image, image_pe, sparse, dense broadcast) of fixture case `name` from the recorded prompt-encoder outputs."""
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    img = synth.synthetic_sam_image_embedding(seed=1).to(device)
    pe = dense_pe({k: v.to(device) for k, v in sd.items()})
    sparse = torch.from_numpy(g[f"{name}_sparse"]).to(device)
    dense = torch.from_numpy(g["dense_value"]).to(device).reshape(1, -1, 1, 1).expand(sparse.shape[0], -1, 64, 64)
    return sd, img, pe, sparse, dense


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_state_dict_matches_the_reference_keys(golden_dir):
    g = golden(golden_dir)
    pe, md = build_models()
    mine = {"prompt_encoder." + k: tuple(v.shape) for k, v in pe.state_dict().items()}
    mine.update({"mask_decoder." + k: tuple(v.shape) for k, v in md.state_dict().items()})
    ref = {str(k): tuple(int(d) for d in s if d) for k, s in zip(g["keys"], g["shapes"])}
    assert mine == ref
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    assert np.array_equal(g["digest"], np.array([float(sd[k].double().sum()) for k in sorted(sd)]))
    build_models(sd)   # strict=True


def test_unsupported_geometry_and_mask_prompts_raise():
    with pytest.raises(NotImplementedError):
        TwoWayTransformer(depth=3, embedding_dim=256, num_heads=8, mlp_dim=2048)
    with pytest.raises(NotImplementedError):
        TwoWayTransformer(depth=2, embedding_dim=256, num_heads=8, mlp_dim=1024)
    t = TwoWayTransformer(depth=2, embedding_dim=256, num_heads=8, mlp_dim=2048)
    with pytest.raises(NotImplementedError):
        MaskDecoder(transformer_dim=256, transformer=t, num_multimask_outputs=2)
    with pytest.raises(NotImplementedError):
        MaskDecoder(transformer_dim=256, transformer=t, iou_head_hidden_dim=128)
    with pytest.raises(NotImplementedError):
        PromptEncoder(embed_dim=256, image_embedding_size=(32, 32), input_image_size=(512, 512), mask_in_chans=16)
    pe, md = build_models()
    with pytest.raises(NotImplementedError):
        pe(points=None, boxes=None, masks=torch.zeros(1, 1, 256, 256))
    with pytest.raises(ValueError, match="'f16x3' or 'f32'"):
        md._weights("f16")
    with pytest.raises(_lib.PopeHipError):   # CPU tensors fail loudly
        md(torch.zeros(1, 256, 64, 64), torch.zeros(1, 256, 64, 64), torch.zeros(1, 2, 256), torch.zeros(1, 256, 64, 64), True)


def test_abi_rejects_bad_arguments_without_a_gpu(hip_lib):
    w = _lib.SamDecoderWeights()
    layers = (_lib.SamDecoderLayerWeights * 2)()
    w.dim, w.heads, w.mlp_dim, w.depth, w.grid, w.num_mask_tokens, w.iou_hidden, w.iou_depth = 256, 8, 2048, 2, 64, 4, 256, 3
    w.precision = _lib.PREC_F16X3
    w.layers_host = C.cast(layers, C.POINTER(_lib.SamDecoderLayerWeights))
    assert hip_lib.pope_sam_decoder_workspace_bytes(C.byref(w), 256, 2, 1) > 0
    assert hip_lib.pope_sam_decoder_workspace_bytes(C.byref(w), 256, 12, 1) == 0
    assert hip_lib.pope_sam_decoder_workspace_bytes(C.byref(w), 0, 2, 1) == 0
    assert hip_lib.pope_sam_decoder_workspace_bytes(None, 1, 2, 1) == 0
    fake = C.c_void_p(16)

    def call(wp, P=1, ns=2, ds=0, ws=1 << 40):
        return hip_lib.pope_sam_decoder_forward_f32(wp, fake, fake, fake, P, ns, fake, ds, 1, fake, fake, None, None, fake, ws, None, None)
    assert call(None) == -1
    assert call(C.byref(w)) == -1               # null weight pointers
    assert call(C.byref(w), P=0) == -1
    assert call(C.byref(w), ns=12) == -1
    assert call(C.byref(w), ds=17) == -1        # a dense stride that is neither a broadcast nor one prompt
    for field, bad in (("dim", 128), ("heads", 4), ("depth", 3), ("grid", 32), ("precision", _lib.PREC_F16)):
        old = getattr(w, field)
        setattr(w, field, bad)
        assert call(C.byref(w)) == -1, field
        assert hip_lib.pope_sam_decoder_workspace_bytes(C.byref(w), 1, 2, 1) == 0, field
        setattr(w, field, old)


@pytest.mark.parametrize("name", synth.SAM_DECODER_CASES)
def test_restatement_reproduces_the_fixture(golden_dir, golden_threads, name):
    g = golden(golden_dir)
    sd, img, pe, sparse, dense = fixture_inputs(g, name)
    assert float((pe[0, :, ::PE_TAP, ::PE_TAP] - torch.from_numpy(g["dense_pe_tap"])).abs().max()) <= 1e-6
    _, _, multimask = synth.sam_decoder_case(name)
    with torch.no_grad():
        masks, iou, hs, keys = restate(sd, img, pe, sparse, dense, multimask)
    taps = torch.from_numpy(g[f"{name}_taps"]).long()
    kp = torch.from_numpy(g[f"{name}_keys_prompts"]).long()
    assert float((iou - torch.from_numpy(g[f"{name}_iou"])).abs().max()) <= 1e-5
    assert float((masks[taps][:, :, ::ROW_TAP] - torch.from_numpy(g[f"{name}_logit_rows"])).abs().max()) <= 1e-5
    assert float((hs[taps] - torch.from_numpy(g[f"{name}_hs"])).abs().max()) <= 1e-5
    assert float((keys[kp][:, ::KEY_TAP] - torch.from_numpy(g[f"{name}_keys"])).abs().max()) <= 1e-5
    ref = torch.from_numpy(np.unpackbits(g[f"{name}_maskbits"], axis=-1).astype(bool))
    near = masks[taps].abs() < 1e-3 * float(masks[taps].abs().max())
    assert bool(((masks[taps] > 0) == ref)[~near].all())
