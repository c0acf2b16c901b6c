"""Vision Mamba (`pose/vim/models_mamba.py:VisionMamba`, the image backbone of `pose/model0606.py`) on HIP (vim.hip).  Inference
only, no torch fallback.

`VisionMamba(...)` keeps the reference constructor and its parameter names and shapes (`cls_token`, `pos_embed`,
`patch_embed.proj.*`, `head.*`, `layers.{i}.mixer.{A_log, D, A_b_log, D_b, in_proj, conv1d, x_proj, dt_proj, conv1d_b, x_proj_b,
dt_proj_b, out_proj}.*`, `layers.{i}.norm.weight`, `norm_f.weight`), so a reference checkpoint loads with strict=True.  Served is
the configuration of the four registered factories: RMSNorm, absolute position embedding, the bidirectional "v2" mixer with the
halved sum, one class token in the middle of the sequence, 16 x 16 patches at stride 8 or 16 on a square image; every other
combination raises NotImplementedError at construction, naming the argument.  The torch submodules only hold the parameters.

The mixer is `mamba_ssm.modules.mamba_simple.Mamba` in the Vim authors' fork, which is not part of the reference tree: it is
implemented from the Mamba paper (Algorithm 2) and the Vim paper (Algorithm 1) and is NOT pinned against that package (DESIGN.md
"Vision Mamba").

precision 'f16x3' (default) runs the patch embedding, in_proj and out_proj on f16 hi/lo planes and x_proj / head with their fp32
operands split in the K loop; 'f32' runs every Linear on the fp32 MFMA.  The convolution, dt_proj, the scan and the norms are fp32
in both.  Range guard: a weight outside the f16x3 contract, or a call in which an f16x3 operand left the f16 range, re-runs the
call in 'f32' with a warning (`overflow_events` counts them), or raises PopeRangeError under `on_overflow = "raise"`.
"""
import ctypes as C
import math

import torch
from torch import nn

from . import _lib
from ._lib import check, on_device_of, require_cuda, stream_of

D_STATE, D_CONV = 16, 4


class RMSNorm(nn.Module):
    """mamba_ssm's RMSNorm: holds `weight` (no bias) and `eps`."""

    def __init__(self, hidden_size, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.register_parameter("bias", None)


class Mamba(nn.Module):
    """The parameters of the bidirectional ("v2") mixer, under the names and in the order of the Vim release."""

    def __init__(self, d_model):
        super().__init__()
        e, r = 2 * d_model, math.ceil(d_model / 16)
        self.d_model, self.d_inner, self.dt_rank = d_model, e, r
        a_log = torch.log(torch.arange(1, D_STATE + 1, dtype=torch.float32)).repeat(e, 1)
        self.in_proj = nn.Linear(d_model, 2 * e, bias=False)
        self.conv1d = nn.Conv1d(e, e, D_CONV, groups=e, padding=D_CONV - 1)
        self.x_proj = nn.Linear(e, r + 2 * D_STATE, bias=False)
        self.dt_proj = nn.Linear(r, e)
        self.A_log = nn.Parameter(a_log.clone())
        self.D = nn.Parameter(torch.ones(e))
        self.A_b_log = nn.Parameter(a_log.clone())
        self.conv1d_b = nn.Conv1d(e, e, D_CONV, groups=e, padding=D_CONV - 1)
        self.x_proj_b = nn.Linear(e, r + 2 * D_STATE, bias=False)
        self.dt_proj_b = nn.Linear(r, e)
        self.D_b = nn.Parameter(torch.ones(e))
        self.out_proj = nn.Linear(e, d_model, bias=False)


class Block(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.mixer = Mamba(dim)
        self.norm = RMSNorm(dim, eps=eps)
        self.drop_path = nn.Identity()       # stochastic depth is a training-time term


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, stride, in_chans, embed_dim):
        super().__init__()
        self.img_size, self.patch_size = (img_size, img_size), (patch_size, patch_size)
        g = (img_size - patch_size) // stride + 1
        self.grid_size, self.num_patches = (g, g), g * g
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=stride)
        self.norm = nn.Identity()


class _WeightRange(Exception):
    pass


def _refuse(name, value, why):
    raise NotImplementedError(f"VisionMamba: {name}={value!r} is not served ({why})")


class VisionMamba(nn.Module):
    def __init__(self, img_size=224, patch_size=16, stride=16, depth=24, embed_dim=192, channels=3, num_classes=1000, ssm_cfg=None,
                 drop_rate=0.0, drop_path_rate=0.1, norm_epsilon: float = 1e-5, rms_norm: bool = False, initializer_cfg=None,
                 fused_add_norm=False, residual_in_fp32=False, device=None, dtype=None, ft_seq_len=None, pt_hw_seq_len=14,
                 if_bidirectional=False, final_pool_type="none", if_abs_pos_embed=False, if_rope=False, if_rope_residual=False,
                 flip_img_sequences_ratio=-1.0, if_bimamba=False, bimamba_type="none", if_cls_token=False, if_devide_out=False,
                 init_layer_scale=None, use_double_cls_token=False, use_middle_cls_token=False, precision="f16x3", **kwargs):
        super().__init__()
        if isinstance(img_size, (tuple, list)):
            if len(img_size) != 2 or img_size[0] != img_size[1]:
                _refuse("img_size", img_size, "square images only")
            img_size = img_size[0]
        if not isinstance(img_size, int) or img_size < 16 or img_size % 8:
            _refuse("img_size", img_size, "a square side that is a multiple of 8, at least 16")
        if patch_size != 16:
            _refuse("patch_size", patch_size, "the patch kernel is 16 x 16")
        if stride not in (8, 16):
            _refuse("stride", stride, "8 or 16")
        if channels != 3:
            _refuse("channels", channels, "3-channel images")
        if embed_dim % 64 or not 64 <= embed_dim <= 512:
            _refuse("embed_dim", embed_dim, "a multiple of 64 up to 512")
        if depth < 1:
            _refuse("depth", depth, "at least one layer")
        if ssm_cfg:
            _refuse("ssm_cfg", ssm_cfg, "d_state 16, d_conv 4, expand 2 only")
        if not rms_norm:
            _refuse("rms_norm", rms_norm, "RMSNorm only")
        if if_bidirectional:
            _refuse("if_bidirectional", if_bidirectional, "the layer-pair form is not built")
        if if_rope:
            _refuse("if_rope", if_rope, "no rotary embedding")
        if if_rope_residual:
            _refuse("if_rope_residual", if_rope_residual, "no rotary embedding")
        if flip_img_sequences_ratio > 0:
            _refuse("flip_img_sequences_ratio", flip_img_sequences_ratio, "a training-time augmentation")
        if if_bimamba or bimamba_type != "v2":
            _refuse("bimamba_type" if not if_bimamba else "if_bimamba", "v1" if if_bimamba else bimamba_type, 'bimamba_type="v2" only')
        if not if_abs_pos_embed:
            _refuse("if_abs_pos_embed", if_abs_pos_embed, "the absolute position embedding is part of the token kernel")
        if not if_cls_token:
            _refuse("if_cls_token", if_cls_token, "the class token is the feature")
        if use_double_cls_token:
            _refuse("use_double_cls_token", use_double_cls_token, "one class token")
        if not use_middle_cls_token:
            _refuse("use_middle_cls_token", use_middle_cls_token, "the class token sits in the middle of the sequence")
        if not if_devide_out:
            _refuse("if_devide_out", if_devide_out, "the two directions are averaged")
        if init_layer_scale is not None:
            _refuse("init_layer_scale", init_layer_scale, "no layer scale")
        if num_classes < 1:
            _refuse("num_classes", num_classes, "a Linear head")
        if precision not in ("f16x3", "f32"):
            raise ValueError("precision must be 'f16x3' or 'f32'")
        # fused_add_norm and residual_in_fp32 compute the same thing in fp32: accepted with either value
        self.residual_in_fp32, self.fused_add_norm = residual_in_fp32, fused_add_norm
        self.if_bidirectional, self.final_pool_type, self.if_abs_pos_embed, self.if_rope = False, final_pool_type, True, False
        self.if_rope_residual, self.flip_img_sequences_ratio, self.if_cls_token = False, flip_img_sequences_ratio, True
        self.use_double_cls_token, self.use_middle_cls_token, self.num_tokens = False, True, 1
        self.num_classes, self.stride, self.img_size, self.depth = int(num_classes), stride, img_size, depth
        self.d_model = self.num_features = self.embed_dim = embed_dim
        self.drop_rate, self.drop_path_rate = drop_rate, drop_path_rate    # accepted and unused: inference only
        self.precision = precision
        self.on_overflow = "rerun_f32"
        self.overflow_events = 0
        self.patch_embed = PatchEmbed(img_size, patch_size, stride, channels, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.pos_drop = nn.Identity()
        self.head = nn.Linear(embed_dim, num_classes)
        self.drop_path = nn.Identity()
        self.layers = nn.ModuleList(Block(embed_dim, norm_epsilon) for _ in range(depth))
        self.norm_f = RMSNorm(embed_dim, eps=norm_epsilon)
        if self.cls_token.device.type != "meta":
            nn.init.trunc_normal_(self.head.weight, std=0.02)
            nn.init.zeros_(self.head.bias)
            nn.init.zeros_(self.patch_embed.proj.bias)
            nn.init.trunc_normal_(self.pos_embed, std=0.02)
            nn.init.trunc_normal_(self.cls_token, std=0.02)
        self.eval()
        self._ws = None
        self._slots = None
        self._struct = {}       # precision -> (key, struct, keep)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("VisionMamba runs inference only (no drop path, no backward): keep it in eval()")
        return super().train(False)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token", "dist_token", "cls_token_head", "cls_token_tail"}

    # ---- derived weights, cached per weight version -----------------------------------------------------------------------
    def _weights(self, precision):
        if self._slots is None:
            self._slots = _lib.param_slots(self)
        key = _lib.slots_key(self._slots)
        hit = self._struct.get(precision)
        if hit is not None and hit[0] == key:
            return hit[1]
        self._struct.pop(precision, None)
        lib, keep, w = _lib.lib(), [], _lib.VimWeights()
        who = "VisionMamba"
        x3 = precision == "f16x3"
        P = lambda t: _lib.param_ptr(t, keep, who)  # noqa: E731

        def WP(t):      # [N, K] fp32 -> weight planes (f16x3 only)
            if not x3:
                return None
            n, k = t.shape
            t = t.detach().contiguous()
            require_cuda(t, who)
            pl = torch.empty(n, 2 * k, dtype=torch.float16, device=t.device)
            with on_device_of(t):
                check(lib.pope_split_planes_f32(_lib.ptr(t), C.c_void_p(pl.data_ptr()), n, k, _lib.PLANES_W_SCALE, None, stream_of(t.device)),
                      "pope_split_planes_f32")
            keep.append(pl)
            if not float(t.abs().max()) * _lib.PLANES_W_SCALE < _lib.F16_MAX:
                raise _WeightRange()
            return C.c_void_p(pl.data_ptr())

        d = self.embed_dim
        w.img, w.stride, w.dim, w.depth, w.num_classes, w.eps = self.img_size, self.stride, d, self.depth, self.num_classes, self.norm_f.eps
        pw = self.patch_embed.proj.weight.reshape(d, 768)
        w.patch_w, w.patch_b, w.patch_wp = P(pw), P(self.patch_embed.proj.bias), WP(pw)
        w.cls, w.pos = P(self.cls_token.reshape(-1)), P(self.pos_embed.reshape(-1, d))
        layers = (_lib.VimLayerWeights * self.depth)()
        for k, blk in zip(layers, self.layers):
            m = blk.mixer
            k.norm_w, k.in_proj_w, k.out_proj_w = P(blk.norm.weight), P(m.in_proj.weight), P(m.out_proj.weight)
            k.in_proj_wp, k.out_proj_wp = WP(m.in_proj.weight), WP(m.out_proj.weight)
            for v, (conv, xp, dt, a_log, dd) in zip(k.dir, ((m.conv1d, m.x_proj, m.dt_proj, m.A_log, m.D),
                                                            (m.conv1d_b, m.x_proj_b, m.dt_proj_b, m.A_b_log, m.D_b))):
                v.conv_w, v.conv_b, v.x_proj_w = P(conv.weight.reshape(-1, D_CONV)), P(conv.bias), P(xp.weight)
                v.dt_w, v.dt_b, v.A_log, v.D = P(dt.weight), P(dt.bias), P(a_log), P(dd)
        w.layers_host = C.cast(layers, C.POINTER(_lib.VimLayerWeights))
        keep.append(layers)
        w.norm_f_w, w.head_w, w.head_b = P(self.norm_f.weight), P(self.head.weight), P(self.head.bias)
        self._struct[precision] = (key, w, keep)
        return w

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def _max_images(self):
        """Images per launch sequence: the GEMMs address their rows through 32-bit byte offsets."""
        g = self.patch_embed.grid_size[0]
        per = max((g * g + 1) * 4 * self.embed_dim * 4, g * g * 768 * 4)
        return max(1, ((1 << 32) - 512) // per - 257)

    def _run(self, x, logits=True, taps=False, precision=None):
        who = "VisionMamba"
        if self.training:
            raise NotImplementedError("VisionMamba runs inference only")
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{who} expects a torch tensor")
        require_cuda(x, who)
        if x.dtype != torch.float32:
            raise TypeError(f"{who}: expected float32, got {x.dtype}")
        s = self.img_size
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, s, s):
            raise ValueError(f"{who}: expected [B, 3, {s}, {s}] (the model's img_size), got {tuple(x.shape)}")
        if logits and self.num_classes % 4:
            raise NotImplementedError(f"{who}: the head GEMM needs num_classes % 4 == 0 (forward_features has no such limit)")
        precision = precision or self.precision
        x = x.contiguous()
        dev, b, d = x.device, x.shape[0], self.embed_dim
        L = self.patch_embed.num_patches + 1
        feats = torch.empty(b, d, dtype=torch.float32, device=dev)
        out = torch.empty(b, self.num_classes, dtype=torch.float32, device=dev) if logits else None
        tap_out = [torch.empty(b, L, d, dtype=torch.float32, device=dev) for _ in range(4)] if taps else None
        if b == 0:
            return feats, out, tap_out
        try:
            w = self._weights(precision)
        except _WeightRange:
            _lib.range_event(self, "pope_amd VisionMamba: a weight leaves the f16x3 range contract (|w| * 256 < 65504)",
                             "; running the call on the fp32 MFMA")
            return self._run(x, logits, taps, precision="f32")
        lib = _lib.lib()
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        step = min(self._max_images(), 65535)
        for i in range(0, b, step):
            n = min(step, b - i)
            need = int(lib.pope_vim_workspace_bytes(C.byref(w), n))
            if need <= 0:
                raise ValueError(f"{who}: unsupported geometry ({n} images of side {s})")
            ws = _lib.grow_workspace(self, need, dev)
            tp = (C.c_void_p * 4)(*[t[i:i + n].data_ptr() for t in tap_out]) if taps else None
            with on_device_of(x):
                check(lib.pope_vim_forward_f32(C.byref(w), _lib.ptr(x[i:i + n]), n, _lib.PRECISIONS[precision], _lib.ptr(ws), ws.numel(),
                                               _lib.ptr(feats[i:i + n]), _lib.ptr(out[i:i + n]) if logits else None, tp,
                                               C.c_void_p(flag.data_ptr()), stream_of(dev)),
                      "pope_vim_forward_f32")
        if precision != "f32":
            bits = int(flag.item())   # one sync per call: the range guard of every planes producer of the launch sequence
            if bits:
                _lib.range_event(self, f"pope_amd VisionMamba: a value left the f16x3 range ({_lib.describe_range_bits(bits)})",
                                 "; re-running the call on the fp32 MFMA")
                return self._run(x, logits, taps, precision="f32")
        return feats, out, tap_out

    @torch.no_grad()
    def forward_features(self, x):
        return self._run(x, logits=False)[0]

    @torch.no_grad()
    def forward(self, x, return_features=False):
        return self._run(x, logits=not return_features)[0 if return_features else 1]

    @torch.no_grad()
    def forward_with_taps(self, x):
        """Test entry: (features [B, D], logits [B, num_classes], [tokens, hidden + residual after layers 0, depth / 2 - 1 and
        depth - 1], [B, L, D] each)."""
        return self._run(x, taps=True)


_FACTORY_SETTINGS = dict(patch_size=16, depth=24, rms_norm=True, residual_in_fp32=True, fused_add_norm=True, final_pool_type="mean",
                         if_abs_pos_embed=True, if_rope=False, if_rope_residual=False, bimamba_type="v2", if_cls_token=True,
                         if_devide_out=True, use_middle_cls_token=True)


def _factory(kwargs, **own):
    if kwargs.pop("pretrained", False):
        raise NotImplementedError("the reference's checkpoint URL is a placeholder: load a state dict instead")
    return VisionMamba(**{**_FACTORY_SETTINGS, **own, **kwargs})


def vim_tiny_patch16_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2(**kwargs):
    return _factory(kwargs, embed_dim=192)


def vim_tiny_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2(**kwargs):
    return _factory(kwargs, embed_dim=192, stride=8)


def vim_small_patch16_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2(**kwargs):
    return _factory(kwargs, embed_dim=384)


def vim_small_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2(**kwargs):
    return _factory(kwargs, embed_dim=384, stride=8)


FACTORIES = {f.__name__: f for f in (vim_tiny_patch16_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2,
                                     vim_tiny_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2,
                                     vim_small_patch16_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2,
                                     vim_small_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2)}


def resample_pos_embed(pos_embed_checkpoint, num_patches, num_extra_tokens):
    """pose/model0606.py:116-134: the checkpoint's position grid resampled bicubically to the model's, extra tokens kept in front
    (on the host, in torch)."""
    embedding_size = pos_embed_checkpoint.shape[-1]
    orig_size = int((pos_embed_checkpoint.shape[-2] - num_extra_tokens) ** 0.5)
    new_size = int(num_patches ** 0.5)
    extra_tokens = pos_embed_checkpoint[:, :num_extra_tokens]
    pos_tokens = pos_embed_checkpoint[:, num_extra_tokens:]
    pos_tokens = pos_tokens.reshape(-1, orig_size, orig_size, embedding_size).permute(0, 3, 1, 2)
    pos_tokens = torch.nn.functional.interpolate(pos_tokens, size=(new_size, new_size), mode="bicubic", align_corners=False)
    pos_tokens = pos_tokens.permute(0, 2, 3, 1).flatten(1, 2)
    return torch.cat((extra_tokens, pos_tokens), dim=1)


class Vim(nn.Module):
    """pose/model0606.py:86-144: the stride-8 factory of `model_type` under `self.model`, its checkpoint loaded with the head keys
    of another width dropped and `pos_embed` resampled to the model's grid.  `checkpoint`: a path, a dict with a 'model' key, or
    None (the model keeps its initial weights; the reference's hard-coded paths are not reproduced)."""

    def __init__(self, num_class: int = 1000, model_type: str = "small", img_size: int = 224, checkpoint=None, **kwargs):
        super().__init__()
        names = {"small": "vim_small_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2",
                 "tiny": "vim_tiny_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2"}
        if model_type not in names:
            raise ValueError(f"Vim: model_type must be 'small' or 'tiny', got {model_type!r}")
        self.model = FACTORIES[names[model_type]](num_classes=num_class, drop_rate=0.0, drop_path_rate=0.1, drop_block_rate=None,
                                                  img_size=img_size, **kwargs)
        self.dropped_keys = []
        if checkpoint is not None:
            if not isinstance(checkpoint, dict):
                checkpoint = torch.load(checkpoint, map_location="cpu")
            checkpoint_model = dict(checkpoint["model"])
            state_dict = self.model.state_dict()
            for k in ["head.weight", "head.bias", "head_dist.weight", "head_dist.bias"]:
                if k in checkpoint_model and (k not in state_dict or checkpoint_model[k].shape != state_dict[k].shape):
                    self.dropped_keys.append(k)
                    del checkpoint_model[k]
            num_patches = self.model.patch_embed.num_patches
            checkpoint_model["pos_embed"] = resample_pos_embed(checkpoint_model["pos_embed"], num_patches,
                                                               self.model.pos_embed.shape[-2] - num_patches)
            self.model.load_state_dict(checkpoint_model, strict=False)
        for param in self.model.parameters():
            param.requires_grad = False
        self.eval()

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("Vim runs inference only: keep it in eval()")
        return super().train(False)

    def forward(self, x):
        return self.model(x)
