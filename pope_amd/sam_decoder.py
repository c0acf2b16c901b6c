"""SAM prompt encoder and mask decoder on the HIP library (point, box and mask prompts).

Drop-ins for `segment_anything.modeling.{prompt_encoder.PromptEncoder, mask_decoder.MaskDecoder, transformer.TwoWayTransformer}`:
same constructor arguments, same parameter and buffer names (a `Sam` checkpoint's `prompt_encoder.*` and `mask_decoder.*` keys
load with strict=True), same forward contracts.  The decoder modules are parameter containers only: `MaskDecoder.forward` is
ONE C-ABI call (`pope_sam_decoder_forward_f32`, pope_amd/csrc/sam_decoder.hip), with no torch fallback, and
`MaskDecoder.forward_images` one (`pope_sam_decoder_forward_images_f32`) for the prompts of up to 16 images.  Both entries share
one input check (`_check`) and one launch method (`_launch`: workspace, launch, range flag); they differ in what follows a
range event (`forward` re-runs in f32, `forward_images` hands the group to `forward` image by image).  The prompt encoder's
point and box embeddings are O(P n 256) work and stay in torch on the device (as LoFTR's position code does); its dense
positional encoding is cached per device.  Its mask embedding (`mask_downscaling`, 4 MiB written per prompt) is ONE C-ABI call
(`pope_sam_mask_embed_f32`, pope_amd/csrc/sam_prompt.hip), with no torch fallback either.

Supported geometry: the decoder every `build_sam` variant builds (dim 256, 8 heads, attention_downsample_rate 2, mlp_dim 2048,
depth 2, a 64 x 64 embedding, 4 mask tokens, IoU head depth 3 / hidden 256), at most 11 sparse embeddings per prompt, and mask
prompts of 256 x 256 with mask_in_chans 16.
"""
import ctypes as C
from typing import Optional, Tuple, Type

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, on_device_of, ptr, require_cuda, stream_of
from .sam_encoder import LayerNorm2d

GRID, DIM, MAX_SPARSE = 64, 256, 11


def _unsupported(what):
    raise NotImplementedError(f"pope_amd SAM decoder: {what} (the build_sam.py decoder geometry only)")


def require_gpu_mask(masks, who):
    """The first check of every entry that takes a mask prompt (None passes): the mask embedding has no torch path, so a mask
    that is not on a GPU is refused before anything else is looked at."""
    if masks is None:
        return
    if not isinstance(masks, torch.Tensor):
        raise TypeError(f"{who}: a mask prompt must be a float32 tensor, got {type(masks).__name__}")
    if not masks.is_cuda:
        raise NotImplementedError(f"pope_amd {who}: mask prompts run on the HIP library only (the mask is on {masks.device})")


class MLPBlock(nn.Module):
    """common.py:13-25 with the decoder's ReLU (parameters only)."""

    def __init__(self, embedding_dim, mlp_dim, act=nn.ReLU):
        super().__init__()
        if act is not nn.ReLU:
            _unsupported("the transformer MLP activation is ReLU (transformer.py:20)")
        self.lin1 = nn.Linear(embedding_dim, mlp_dim)
        self.lin2 = nn.Linear(mlp_dim, embedding_dim)
        self.act = act()


class Attention(nn.Module):
    """transformer.py:185-240 (parameters only)."""

    def __init__(self, embedding_dim, num_heads, downsample_rate=1):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.internal_dim = embedding_dim // downsample_rate
        self.num_heads = num_heads
        assert self.internal_dim % num_heads == 0, "num_heads must divide embedding_dim."
        self.q_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.k_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.v_proj = nn.Linear(embedding_dim, self.internal_dim)
        self.out_proj = nn.Linear(self.internal_dim, embedding_dim)


class TwoWayAttentionBlock(nn.Module):
    """transformer.py:109-182 (parameters only)."""

    def __init__(self, embedding_dim, num_heads, mlp_dim=2048, activation=nn.ReLU, attention_downsample_rate=2,
                 skip_first_layer_pe=False):
        super().__init__()
        self.self_attn = Attention(embedding_dim, num_heads)
        self.norm1 = nn.LayerNorm(embedding_dim)
        self.cross_attn_token_to_image = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate)
        self.norm2 = nn.LayerNorm(embedding_dim)
        self.mlp = MLPBlock(embedding_dim, mlp_dim, activation)
        self.norm3 = nn.LayerNorm(embedding_dim)
        self.norm4 = nn.LayerNorm(embedding_dim)
        self.cross_attn_image_to_token = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate)
        self.skip_first_layer_pe = skip_first_layer_pe


class TwoWayTransformer(nn.Module):
    """transformer.py:16-106 (parameters only; MaskDecoder runs it)."""

    def __init__(self, depth, embedding_dim, num_heads, mlp_dim, activation=nn.ReLU, attention_downsample_rate=2):
        super().__init__()
        if (depth, embedding_dim, num_heads, mlp_dim, attention_downsample_rate) != (2, DIM, 8, 2048, 2):
            _unsupported(f"TwoWayTransformer(depth={depth}, embedding_dim={embedding_dim}, num_heads={num_heads}, "
                         f"mlp_dim={mlp_dim}, attention_downsample_rate={attention_downsample_rate})")
        self.depth = depth
        self.embedding_dim = embedding_dim
        self.num_heads = num_heads
        self.mlp_dim = mlp_dim
        self.layers = nn.ModuleList(
            TwoWayAttentionBlock(embedding_dim=embedding_dim, num_heads=num_heads, mlp_dim=mlp_dim, activation=activation,
                                 attention_downsample_rate=attention_downsample_rate, skip_first_layer_pe=(i == 0))
            for i in range(depth))
        self.final_attn_token_to_image = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate)
        self.norm_final_attn = nn.LayerNorm(embedding_dim)


class MLP(nn.Module):
    """mask_decoder.py:158-182 (parameters only)."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers, sigmoid_output=False):
        super().__init__()
        if sigmoid_output:
            _unsupported("sigmoid_output")
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))
        self.sigmoid_output = sigmoid_output


class MaskDecoder(nn.Module):
    """mask_decoder.py:16-155: forward(image_embeddings [1, 256, 64, 64], image_pe [1, 256, 64, 64], sparse [P, n, 256],
    dense [P, 256, 64, 64], multimask_output) -> (low_res_masks [P, C, 256, 256], iou_pred [P, C]), C = 3 or 1."""

    def __init__(self, *, transformer_dim: int, transformer: nn.Module, num_multimask_outputs: int = 3,
                 activation: Type[nn.Module] = nn.GELU, iou_head_depth: int = 3, iou_head_hidden_dim: int = 256) -> None:
        super().__init__()
        if not isinstance(transformer, TwoWayTransformer):
            _unsupported("the transformer must be pope_amd.sam_decoder.TwoWayTransformer")
        if (transformer_dim, transformer.embedding_dim, num_multimask_outputs, iou_head_depth, iou_head_hidden_dim) != (DIM, DIM, 3, 3, 256):
            _unsupported(f"MaskDecoder(transformer_dim={transformer_dim}, num_multimask_outputs={num_multimask_outputs}, "
                         f"iou_head_depth={iou_head_depth}, iou_head_hidden_dim={iou_head_hidden_dim})")
        if activation is not nn.GELU:
            _unsupported("the upscaling activation is the erf GELU (build_sam.py)")
        self.transformer_dim = transformer_dim
        self.transformer = transformer
        self.num_multimask_outputs = num_multimask_outputs
        self.iou_token = nn.Embedding(1, transformer_dim)
        self.num_mask_tokens = num_multimask_outputs + 1
        self.mask_tokens = nn.Embedding(self.num_mask_tokens, transformer_dim)
        self.output_upscaling = nn.Sequential(
            nn.ConvTranspose2d(transformer_dim, transformer_dim // 4, kernel_size=2, stride=2),
            LayerNorm2d(transformer_dim // 4),
            activation(),
            nn.ConvTranspose2d(transformer_dim // 4, transformer_dim // 8, kernel_size=2, stride=2),
            activation(),
        )
        self.output_hypernetworks_mlps = nn.ModuleList(
            MLP(transformer_dim, transformer_dim, transformer_dim // 8, 3) for _ in range(self.num_mask_tokens))
        self.iou_prediction_head = MLP(transformer_dim, iou_head_hidden_dim, self.num_mask_tokens, iou_head_depth)
        # "f16x3" (default): the image-side Linears on hi + lo f16 planes, three MFMAs per product (fp32-level results);
        # "f32": every image-side Linear on the fp32 GEMM (what a range-guard event re-runs in).  Token side, attention,
        # LayerNorms and the upscaling tail are fp32 in both.
        self.precision = "f16x3"
        self.on_overflow = "rerun_f32"   # "rerun_f32" (warn, re-run the call in f32) | "raise"
        self.overflow_events = 0
        self._wcache = {}
        self._src = None
        self._ws = None

    # ---- host plumbing ---------------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._wcache, self._ws, self._src = {}, None, None
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._wcache = {}
        return out

    def _sources(self):
        if self._src is None:
            self._src = _lib.param_slots(self)
        return self._src

    def _eps(self):
        t = self.transformer
        eps_t = {float(m.eps) for b in t.layers for m in (b.norm1, b.norm2, b.norm3, b.norm4)} | {float(t.norm_final_attn.eps)}
        if len(eps_t) != 1:
            _unsupported("one LayerNorm eps for every token / image-token norm")
        return eps_t.pop(), float(self.output_upscaling[1].eps)

    def _weights(self, precision=None):
        precision = precision or self.precision
        if precision not in ("f16x3", "f32"):
            raise ValueError(f"MaskDecoder.precision must be 'f16x3' or 'f32', not {precision!r}")
        f32 = precision == "f32"
        key = _lib.slots_key(self._sources())
        hit = self._wcache.get(precision)
        if hit is not None and hit[0] == key:
            return hit[1]
        keep = []

        def P(t):
            return _lib.param_ptr(t, keep, "MaskDecoder")

        def cat(*ts):
            return torch.cat([t.detach() for t in ts], 0)

        t = self.transformer
        up0, up1 = self.output_upscaling[0], self.output_upscaling[3]
        image_side = [w for b in t.layers for w in (cat(b.cross_attn_token_to_image.k_proj.weight, b.cross_attn_image_to_token.q_proj.weight),
                                                    b.cross_attn_token_to_image.v_proj.weight, b.cross_attn_image_to_token.out_proj.weight)]
        image_side += [t.final_attn_token_to_image.k_proj.weight, t.final_attn_token_to_image.v_proj.weight,
                       up0.weight.detach().permute(2, 3, 1, 0).reshape(4 * up0.out_channels, up0.in_channels)]
        amax = float(torch.stack([w.detach().abs().max() for w in image_side]).max())
        if not f32 and not amax * _lib.PLANES_W_SCALE < _lib.F16_MAX:
            _lib.range_event(self, f"pope_amd: max |weight| = {amax:g} is outside the f16x3 range contract "
                             f"(|w| < {_lib.F16_MAX / _lib.PLANES_W_SCALE:g})", "; this decoder runs with precision='f32'")
            w = self._weights("f32")
            self._wcache[precision] = self._wcache["f32"]
            return w

        def WP(w2d):
            w2d = w2d.detach().float()
            pl = w2d.contiguous() if f32 else _lib.to_planes(w2d, _lib.PLANES_W_SCALE)
            keep.append(pl)
            return C.c_void_p(pl.data_ptr())

        eps_t, eps_u = self._eps()
        layers = (_lib.SamDecoderLayerWeights * t.depth)()
        for i, b in enumerate(t.layers):
            L, sa, t2i, i2t = layers[i], b.self_attn, b.cross_attn_token_to_image, b.cross_attn_image_to_token
            L.sa_qkv_w = P(cat(sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight))
            L.sa_qkv_b = P(cat(sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias))
            L.sa_o_w, L.sa_o_b = P(sa.out_proj.weight), P(sa.out_proj.bias)
            L.norm1_w, L.norm1_b = P(b.norm1.weight), P(b.norm1.bias)
            L.t2i_q_w, L.t2i_q_b = P(t2i.q_proj.weight), P(t2i.q_proj.bias)
            L.t2i_o_w, L.t2i_o_b = P(t2i.out_proj.weight), P(t2i.out_proj.bias)
            L.norm2_w, L.norm2_b = P(b.norm2.weight), P(b.norm2.bias)
            L.mlp1_w, L.mlp1_b = P(b.mlp.lin1.weight), P(b.mlp.lin1.bias)
            L.mlp2_w, L.mlp2_b = P(b.mlp.lin2.weight), P(b.mlp.lin2.bias)
            L.norm3_w, L.norm3_b = P(b.norm3.weight), P(b.norm3.bias)
            L.i2t_kv_w, L.i2t_kv_b = P(cat(i2t.k_proj.weight, i2t.v_proj.weight)), P(cat(i2t.k_proj.bias, i2t.v_proj.bias))
            L.img_qk_wp, L.img_qk_b = WP(cat(t2i.k_proj.weight, i2t.q_proj.weight)), P(cat(t2i.k_proj.bias, i2t.q_proj.bias))
            L.img_v_wp, L.img_v_b = WP(t2i.v_proj.weight), P(t2i.v_proj.bias)
            L.i2t_o_wp, L.i2t_o_b = WP(i2t.out_proj.weight), P(i2t.out_proj.bias)
            L.norm4_w, L.norm4_b = P(b.norm4.weight), P(b.norm4.bias)
        s = _lib.SamDecoderWeights()
        s.dim, s.heads, s.mlp_dim, s.depth, s.grid = DIM, t.num_heads, t.mlp_dim, t.depth, GRID
        s.num_mask_tokens, s.iou_hidden = self.num_mask_tokens, self.iou_prediction_head.layers[0].out_features
        s.iou_depth = self.iou_prediction_head.num_layers
        s.precision = _lib.PRECISIONS[precision]
        s.token_eps, s.up_eps = eps_t, eps_u
        s.tokens = P(cat(self.iou_token.weight, self.mask_tokens.weight))
        s.layers_host = C.cast(layers, C.POINTER(_lib.SamDecoderLayerWeights))
        fa = t.final_attn_token_to_image
        s.fin_q_w, s.fin_q_b = P(fa.q_proj.weight), P(fa.q_proj.bias)
        s.fin_k_wp, s.fin_k_b = WP(fa.k_proj.weight), P(fa.k_proj.bias)
        s.fin_v_wp, s.fin_v_b = WP(fa.v_proj.weight), P(fa.v_proj.bias)
        s.fin_o_w, s.fin_o_b = P(fa.out_proj.weight), P(fa.out_proj.bias)
        s.norm_final_w, s.norm_final_b = P(t.norm_final_attn.weight), P(t.norm_final_attn.bias)
        # ConvTranspose 2x2 / 2 as GEMMs: row tap * C_out + c_out (tap = 2 dy + dx) of weight[:, c_out, dy, dx]
        s.up1_wp = WP(up0.weight.detach().permute(2, 3, 1, 0).reshape(4 * up0.out_channels, up0.in_channels))
        s.up1_b = P(up0.bias.detach().repeat(4))
        s.up_ln_w, s.up_ln_b = P(self.output_upscaling[1].weight), P(self.output_upscaling[1].bias)
        s.up2_w = P(up1.weight.detach().permute(2, 3, 1, 0).reshape(4 * up1.out_channels, up1.in_channels))
        s.up2_b = P(up1.bias)
        for i, mlp in enumerate(self.output_hypernetworks_mlps):
            for j, lin in enumerate(mlp.layers):
                s.hyper_w[3 * i + j], s.hyper_b[3 * i + j] = P(lin.weight), P(lin.bias)
        for j, lin in enumerate(self.iou_prediction_head.layers):
            s.iou_w[j], s.iou_b[j] = P(lin.weight), P(lin.bias)
        keep.append(layers)
        self._wcache[precision] = (key, s, keep)
        return s

    def _check(self, image_embeddings, image_pe, sparse, dense, images=False):
        """The input check of both entries: device and dtype of the four tensors, the image shapes (one image, N with `images`),
        the sparse shape, then the entry's own dense rule ([1 or P, ...] for `forward`, the stride-0 broadcast for
        `forward_images`).  Returns whether dense is one embedding for every prompt (PromptEncoder's no_mask_embed)."""
        for t, name in ((image_embeddings, "image_embeddings"), (image_pe, "image_pe"), (sparse, "sparse_prompt_embeddings"),
                        (dense, "dense_prompt_embeddings")):
            require_cuda(t, "MaskDecoder")
            if t.dtype != torch.float32:
                raise TypeError(f"MaskDecoder: {name} must be float32, got {t.dtype}")
        one = (1, DIM, GRID, GRID)
        if images:
            if image_embeddings.dim() != 4 or tuple(image_embeddings.shape[1:]) != one[1:] or tuple(image_pe.shape) != one:
                raise ValueError(f"MaskDecoder.forward_images: image_embeddings must be [N, {DIM}, {GRID}, {GRID}] and image_pe "
                                 f"[1, {DIM}, {GRID}, {GRID}], got {tuple(image_embeddings.shape)} and {tuple(image_pe.shape)}")
        elif tuple(image_embeddings.shape) != one or tuple(image_pe.shape) != one:
            raise ValueError(f"MaskDecoder: image_embeddings and image_pe must be {one} (one image), got "
                             f"{tuple(image_embeddings.shape)} and {tuple(image_pe.shape)}")
        if sparse.dim() != 3 or sparse.shape[2] != DIM or sparse.shape[1] > MAX_SPARSE:
            raise ValueError(f"MaskDecoder: sparse_prompt_embeddings must be [P, n <= {MAX_SPARSE}, {DIM}], got {tuple(sparse.shape)}")
        fits = dense.dim() == 4 and tuple(dense.shape[1:]) == one[1:] and dense.shape[0] in (1, sparse.shape[0])
        shared = fits and (dense.shape[0] == 1 or dense.stride(0) == 0)
        if images and not shared:
            raise ValueError("MaskDecoder.forward_images: dense_prompt_embeddings must be the broadcast PromptEncoder returns "
                             f"without a mask ([1 or P, {DIM}, {GRID}, {GRID}], batch stride 0), got {tuple(dense.shape)}")
        if not fits:
            raise ValueError(f"MaskDecoder: dense_prompt_embeddings must be [P, {DIM}, {GRID}, {GRID}], got {tuple(dense.shape)}")
        return shared

    def _launch(self, w, img, pe, sparse, dense, dense_stride, multimask_output, masks, iou, hs=None, keys=None, which=None):
        """The one place that calls the decoder's C entries: `pope_sam_decoder_forward_f32` for one image, with `which` (the
        image of each prompt) `pope_sam_decoder_forward_images_f32` for img [N, ...].  Workspace query, the grow-only workspace,
        the launch and the one read of the range flag (one sync per call: the range guard of every planes producer of the
        call).  Returns the range bits."""
        L = _lib.lib()
        N, P, ns, dev = img.shape[0], sparse.shape[0], sparse.shape[1], img.device
        if which is None:
            need = L.pope_sam_decoder_workspace_bytes(C.byref(w), P, ns, int(dense_stride == 0))
            what = f"n_sparse = {ns}, at most {MAX_SPARSE}"
        else:
            host = (C.c_int * P)(*(int(v) for v in which))
            need = L.pope_sam_decoder_images_workspace_bytes(C.byref(w), N, host, P, ns, dense_stride)
            what = f"N = {N}, P = {P}, n_sparse = {ns}, at most {MAX_SPARSE}"
        if int(need) <= 0:
            raise ValueError(f"pope_amd SAM decoder: unsupported call ({what})")
        ws = _lib.grow_workspace(self, int(need), dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        sp, mm, fl = ptr(sparse) if ns else None, int(bool(multimask_output)), C.c_void_p(flag.data_ptr())
        with on_device_of(img):
            if which is None:
                check(L.pope_sam_decoder_forward_f32(
                    C.byref(w), ptr(img), ptr(pe), sp, P, ns, ptr(dense), dense_stride, mm, ptr(masks), ptr(iou), ptr(hs), ptr(keys),
                    ptr(ws), ws.numel(), fl, stream_of(dev)), "pope_sam_decoder_forward_f32")
            else:
                check(L.pope_sam_decoder_forward_images_f32(
                    C.byref(w), ptr(img), N, ptr(pe), sp, host, P, ns, ptr(dense), dense_stride, mm, ptr(masks), ptr(iou),
                    ptr(ws), ws.numel(), fl, stream_of(dev)), "pope_sam_decoder_forward_images_f32")
        return int(flag.item())

    def _run(self, image_embeddings, image_pe, sparse, dense, multimask_output, taps=False, precision=None):
        shared = self._check(image_embeddings, image_pe, sparse, dense)
        img, pe, sparse = image_embeddings.contiguous(), image_pe.contiguous(), sparse.contiguous()
        dense = dense[:1].contiguous() if shared else dense.contiguous()
        P, ns = sparse.shape[0], sparse.shape[1]
        Cm = self.num_multimask_outputs if multimask_output else 1
        dev = img.device
        masks = torch.empty(P, Cm, 4 * GRID, 4 * GRID, device=dev, dtype=torch.float32)
        iou = torch.empty(P, Cm, device=dev, dtype=torch.float32)
        hs = torch.empty(P, 1 + self.num_mask_tokens + ns, DIM, device=dev, dtype=torch.float32) if taps else None
        keys = torch.empty(P, GRID * GRID, DIM, device=dev, dtype=torch.float32) if taps else None
        if P == 0:
            return masks, iou, hs, keys
        bits = self._launch(self._weights(precision), img, pe, sparse, dense, 0 if shared else DIM * GRID * GRID, multimask_output,
                            masks, iou, hs, keys)
        if bits:
            _lib.range_event(self, f"pope_amd SAM decoder: a value left the f16x3 range ({_lib.describe_range_bits(bits)})",
                             "; re-running the call on the fp32 GEMMs")
            return self._run(image_embeddings, image_pe, sparse, dense, multimask_output, taps, precision="f32")
        return masks, iou, hs, keys

    def forward(self, image_embeddings: torch.Tensor, image_pe: torch.Tensor, sparse_prompt_embeddings: torch.Tensor,
                dense_prompt_embeddings: torch.Tensor, multimask_output: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        masks, iou, _, _ = self._run(image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output)
        return masks, iou

    # ---- several images in one call --------------------------------------------------------------------------------
    IMAGES_PER_CALL = 16   # bounds the workspace: the layer-0 buffers are held once per image of a call (18 MB each)

    def forward_images(self, image_embeddings: torch.Tensor, image_pe: torch.Tensor, sparse_prompt_embeddings: torch.Tensor,
                       dense_prompt_embeddings: torch.Tensor, prompt_image, multimask_output: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """`forward` over the prompts of N images: image_embeddings [N, 256, 64, 64], sparse [P, n, 256], dense the broadcast
        `PromptEncoder` returns without a mask ([1 or P, 256, 64, 64], one value per channel), prompt_image [P] = the image of
        each prompt (host integers, any order) -> (low_res_masks [P, C, 256, 256], iou_pred [P, C]), prompt for prompt
        bit-identical to `forward` with that prompt's image alone.  One image has nothing to share and is `forward` (the same
        bits, less host work: profiles/sam_forward.md).  Otherwise one C call (the multi-image entry, `_launch`) and one
        range-flag read per group of at most 16 images; a flagged group is handled per image by `forward`, so that one
        image's overflow neither changes nor re-runs another image's prompts on other arithmetic than its own call would."""
        sparse, dense = sparse_prompt_embeddings, dense_prompt_embeddings
        self._check(image_embeddings, image_pe, sparse, dense, images=True)
        N, P = image_embeddings.shape[0], sparse.shape[0]
        which = np.asarray(prompt_image.cpu() if isinstance(prompt_image, torch.Tensor) else prompt_image, dtype=np.int64).reshape(-1)
        if which.size != P or (P and (which.min() < 0 or which.max() >= N)):
            raise ValueError(f"MaskDecoder.forward_images: prompt_image must hold {P} image indices in [0, {N})")
        if N == 1:
            return self.forward(image_embeddings, image_pe, sparse, dense[:1], multimask_output)
        Cm = self.num_multimask_outputs if multimask_output else 1
        dev = image_embeddings.device
        masks = torch.empty(P, Cm, 4 * GRID, 4 * GRID, device=dev, dtype=torch.float32)
        iou = torch.empty(P, Cm, device=dev, dtype=torch.float32)
        if P == 0:
            return masks, iou
        img, pe, sparse, dense = image_embeddings.contiguous(), image_pe.contiguous(), sparse.contiguous(), dense[:1].contiguous()
        for i0 in range(0, N, self.IMAGES_PER_CALL):
            i1 = min(N, i0 + self.IMAGES_PER_CALL)
            rows = np.nonzero((which >= i0) & (which < i1))[0]
            if rows.size == 0:
                continue
            if i0 == 0 and i1 == N and rows.size == P:   # one group, every prompt: straight into the outputs
                self._run_images(img, pe, sparse, dense, which, multimask_output, masks, iou)
                continue
            idx = torch.as_tensor(rows, device=dev)
            m, q = masks.new_empty(rows.size, *masks.shape[1:]), iou.new_empty(rows.size, Cm)
            self._run_images(img[i0:i1], pe, sparse[idx].contiguous(), dense, which[rows] - i0, multimask_output, m, q)
            masks[idx], iou[idx] = m, q
        return masks, iou

    def _run_images(self, img, pe, sparse, dense, which, multimask_output, masks, iou):
        """One multi-image call into masks / iou; on a range event the group's images one by one."""
        if not self._launch(self._weights(), img, pe, sparse, dense, 0, multimask_output, masks, iou, which=which):
            return
        # The flag does not say whose value left the range.  Each image's own call does: it counts the event, raises or warns
        # and re-runs in f32 exactly as the per-image loop would, and leaves the other images on the arithmetic they asked for.
        for i in np.unique(which):
            idx = torch.as_tensor(np.nonzero(which == i)[0], device=img.device)
            m, q = self.forward(img[int(i)][None], pe, sparse[idx], dense.expand(idx.numel(), -1, -1, -1), multimask_output)
            masks[idx], iou[idx] = m, q

    def forward_with_taps(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output):
        """(masks, iou_pred, hs [P, T, 256], keys [P, 4096, 256]): the transformer's final tokens and image tokens too."""
        return self._run(image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output, taps=True)


class PositionEmbeddingRandom(nn.Module):
    """prompt_encoder.py:171-214."""

    def __init__(self, num_pos_feats: int = 64, scale: Optional[float] = None) -> None:
        super().__init__()
        if scale is None or scale <= 0.0:
            scale = 1.0
        self.register_buffer("positional_encoding_gaussian_matrix", scale * torch.randn((2, num_pos_feats)))

    def _pe_encoding(self, coords: torch.Tensor) -> torch.Tensor:
        coords = 2 * coords - 1
        coords = coords @ self.positional_encoding_gaussian_matrix
        coords = 2 * np.pi * coords
        return torch.cat([torch.sin(coords), torch.cos(coords)], dim=-1)

    def forward(self, size: Tuple[int, int]) -> torch.Tensor:
        h, w = size
        grid = torch.ones((h, w), device=self.positional_encoding_gaussian_matrix.device, dtype=torch.float32)
        y_embed = (grid.cumsum(dim=0) - 0.5) / h
        x_embed = (grid.cumsum(dim=1) - 0.5) / w
        pe = self._pe_encoding(torch.stack([x_embed, y_embed], dim=-1))
        return pe.permute(2, 0, 1)   # C x H x W

    def forward_with_coords(self, coords_input: torch.Tensor, image_size: Tuple[int, int]) -> torch.Tensor:
        coords = coords_input.clone()
        coords[:, :, 0] = coords[:, :, 0] / image_size[1]
        coords[:, :, 1] = coords[:, :, 1] / image_size[0]
        return self._pe_encoding(coords.to(torch.float))   # B x N x C


class PromptEncoder(nn.Module):
    """prompt_encoder.py:16-168: forward(points, boxes, masks) -> (sparse [P, n, 256], dense [P, 256, 64, 64]);
    get_dense_pe() -> [1, 256, 64, 64], cached per device.  Without a mask, dense is a broadcast of no_mask_embed (batch stride
    0).  masks: float32 [P, 1, 256, 256] on the module's device (made contiguous if it is a view; TypeError for another dtype,
    ValueError for another shape or a P that disagrees with the points / boxes); dense is then a fresh contiguous tensor from one
    C call (`pope_sam_mask_embed_f32`), a prompt's embedding bit-identical whatever P.  Masks alone give sparse [P, 0, 256].
    There is no torch path for the mask embedding: a mask that is not on a GPU raises NotImplementedError."""

    def __init__(self, embed_dim: int, image_embedding_size: Tuple[int, int], input_image_size: Tuple[int, int],
                 mask_in_chans: int, activation: Type[nn.Module] = nn.GELU) -> None:
        super().__init__()
        if embed_dim != DIM or tuple(image_embedding_size) != (GRID, GRID):
            _unsupported(f"PromptEncoder(embed_dim={embed_dim}, image_embedding_size={tuple(image_embedding_size)})")
        self.embed_dim = embed_dim
        self.input_image_size = input_image_size
        self.image_embedding_size = image_embedding_size
        self.pe_layer = PositionEmbeddingRandom(embed_dim // 2)
        self.num_point_embeddings = 4   # pos / neg point + 2 box corners
        self.point_embeddings = nn.ModuleList(nn.Embedding(1, embed_dim) for _ in range(self.num_point_embeddings))
        self.not_a_point_embed = nn.Embedding(1, embed_dim)
        self.mask_input_size = (4 * image_embedding_size[0], 4 * image_embedding_size[1])
        # a parameter container: `_embed_masks` runs the whole chain in one kernel (pope_amd/csrc/sam_prompt.hip)
        self.mask_downscaling = nn.Sequential(
            nn.Conv2d(1, mask_in_chans // 4, kernel_size=2, stride=2),
            LayerNorm2d(mask_in_chans // 4),
            activation(),
            nn.Conv2d(mask_in_chans // 4, mask_in_chans, kernel_size=2, stride=2),
            LayerNorm2d(mask_in_chans),
            activation(),
            nn.Conv2d(mask_in_chans, embed_dim, kernel_size=1),
        )
        self.no_mask_embed = nn.Embedding(1, embed_dim)
        self._pe_cache = {}
        self._mask_src = None   # where mask_downscaling keeps its parameters (_lib.param_slots)
        self._mask_w = None     # (slots key, pope_sam_mask_embed_weights, the tensors it points into)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._pe_cache, self._mask_src, self._mask_w = {}, None, None
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._pe_cache, self._mask_w = {}, None
        return out

    def _get_device(self) -> torch.device:
        return self.point_embeddings[0].weight.device

    def get_dense_pe(self) -> torch.Tensor:
        g = self.pe_layer.positional_encoding_gaussian_matrix
        require_cuda(g, "PromptEncoder")
        key = (g.data_ptr(), g._version)
        hit = self._pe_cache.get(g.device)
        if hit is None or hit[0] != key:
            hit = (key, self.pe_layer(self.image_embedding_size).unsqueeze(0).contiguous())
            self._pe_cache[g.device] = hit
        return hit[1]

    def _embed_points(self, points, labels, pad):
        points = points + 0.5   # shift to the pixel centre
        if pad:
            padding_point = torch.zeros((points.shape[0], 1, 2), device=points.device)
            padding_label = -torch.ones((labels.shape[0], 1), device=labels.device)
            points = torch.cat([points, padding_point], dim=1)
            labels = torch.cat([labels, padding_label], dim=1)
        point_embedding = self.pe_layer.forward_with_coords(points, self.input_image_size)
        point_embedding[labels == -1] = 0.0
        point_embedding[labels == -1] += self.not_a_point_embed.weight
        point_embedding[labels == 0] += self.point_embeddings[0].weight
        point_embedding[labels == 1] += self.point_embeddings[1].weight
        return point_embedding

    def _embed_boxes(self, boxes):
        boxes = boxes + 0.5
        coords = boxes.reshape(-1, 2, 2)
        corner_embedding = self.pe_layer.forward_with_coords(coords, self.input_image_size)
        corner_embedding[:, 0, :] += self.point_embeddings[2].weight
        corner_embedding[:, 1, :] += self.point_embeddings[3].weight
        return corner_embedding

    def _mask_weights(self):
        """The `pope_sam_mask_embed_weights` of `mask_downscaling` (the parameters themselves, torch's layouts), rebuilt when a
        parameter was replaced or edited in place."""
        if self._mask_src is None:
            self._mask_src = _lib.param_slots(self.mask_downscaling)
        key = _lib.slots_key(self._mask_src)
        if self._mask_w is not None and self._mask_w[0] == key:
            return self._mask_w[1]
        conv1, ln1, act1, conv2, ln2, act2, conv3 = self.mask_downscaling
        if conv2.out_channels != 16 or any(not isinstance(a, nn.GELU) or a.approximate != "none" for a in (act1, act2)):
            _unsupported(f"mask prompts with mask_in_chans={conv2.out_channels}, activation {type(act1).__name__} "
                         "(mask_in_chans 16 and the erf GELU)")
        keep = []

        def P(t):
            return _lib.param_ptr(t, keep, "PromptEncoder")

        s = _lib.SamMaskEmbedWeights()
        s.mask_in_chans, s.embed_dim, s.grid = conv2.out_channels, conv3.out_channels, self.image_embedding_size[0]
        s.ln1_eps, s.ln2_eps = float(ln1.eps), float(ln2.eps)
        s.conv1_w, s.conv1_b, s.ln1_w, s.ln1_b = P(conv1.weight), P(conv1.bias), P(ln1.weight), P(ln1.bias)
        s.conv2_w, s.conv2_b, s.ln2_w, s.ln2_b = P(conv2.weight), P(conv2.bias), P(ln2.weight), P(ln2.bias)
        s.conv3_w, s.conv3_b = P(conv3.weight), P(conv3.bias)
        self._mask_w = (key, s, keep)
        return s

    def _check_masks(self, masks):
        """dtype and shape of a mask prompt (its device is `forward`'s first check)."""
        if masks.dtype != torch.float32:
            raise TypeError(f"PromptEncoder: masks must be float32, got {masks.dtype}")
        if masks.dim() != 4 or tuple(masks.shape[1:]) != (1, *self.mask_input_size):
            raise ValueError(f"PromptEncoder: masks must be [B, 1, {self.mask_input_size[0]}, {self.mask_input_size[1]}], "
                             f"got {tuple(masks.shape)}")

    def _embed_masks(self, masks):
        """prompt_encoder.py:102-105 in ONE C call (`pope_sam_mask_embed_f32`): [B, 1, 256, 256] -> a fresh [B, 256, 64, 64]."""
        w = self._mask_weights()
        masks = masks.contiguous()
        if masks.data_ptr() % 16:   # a contiguous view into the middle of a storage: the kernel loads 16 bytes at a time
            masks = masks.clone()
        dense = torch.empty(masks.shape[0], self.embed_dim, *self.image_embedding_size, device=masks.device, dtype=torch.float32)
        if masks.shape[0] == 0:
            return dense
        with on_device_of(masks):
            check(_lib.lib().pope_sam_mask_embed_f32(C.byref(w), ptr(masks), masks.shape[0], ptr(dense), stream_of(masks.device)),
                  "pope_sam_mask_embed_f32")
        return dense

    def forward(self, points: Optional[Tuple[torch.Tensor, torch.Tensor]], boxes: Optional[torch.Tensor],
                masks: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        require_gpu_mask(masks, "PromptEncoder")   # before every other check
        dev = self._get_device()
        require_cuda(self.point_embeddings[0].weight, "PromptEncoder")
        for t in (points[0] if points is not None else None, points[1] if points is not None else None, boxes):
            if t is not None:
                require_cuda(t, "PromptEncoder")
        bs = points[0].shape[0] if points is not None else boxes.shape[0] if boxes is not None else \
            masks.shape[0] if masks is not None else 1
        if masks is not None:
            self._check_masks(masks)
            if masks.shape[0] != bs:
                raise ValueError(f"PromptEncoder: masks holds {masks.shape[0]} prompts, the points / boxes {bs}")
            if masks.device != dev:
                raise ValueError(f"PromptEncoder: masks is on {masks.device}, the module on {dev}")
        sparse_embeddings = torch.empty((bs, 0, self.embed_dim), device=dev)
        if points is not None:
            coords, labels = points
            sparse_embeddings = torch.cat([sparse_embeddings, self._embed_points(coords, labels, pad=(boxes is None))], dim=1)
        if boxes is not None:
            sparse_embeddings = torch.cat([sparse_embeddings, self._embed_boxes(boxes)], dim=1)
        if masks is not None:
            return sparse_embeddings, self._embed_masks(masks)
        dense_embeddings = self.no_mask_embed.weight.reshape(1, -1, 1, 1).expand(bs, -1, self.image_embedding_size[0],
                                                                                 self.image_embedding_size[1])
        return sparse_embeddings, dense_embeddings
