"""ConvNeXtV2 (`pose/convnextv2/convnextv2.py`: Block + GRN) on HIP (convnext.hip): the image backbone of the fork's later pose
models.  Inference only, no torch fallback.

`ConvNeXtV2(...)` keeps the reference constructor, its parameter names and shapes (`downsample_layers.{i}.{0,1}.*`,
`stages.{i}.{j}.{dwconv,norm,pwconv1,grn,pwconv2}.*`, `norm.*`, `head.*`; GRN `gamma` / `beta` [1, 1, 1, 4C]), so a reference
checkpoint loads with strict=True; `remap_checkpoint_keys` is the FCMAE-checkpoint remapping of `pose/utils.py`.  The torch
submodules only hold the parameters: forward runs channels-last on the device, the convolutions with k = stride as GEMMs over
gathered rows.  H and W must be multiples of 32 (the reference would silently truncate other sizes): ValueError.

precision 'f16x3' (default) runs every GEMM whose K is a multiple of 32 on f16 hi/lo planes, the others (the stem's K = 48, the
C = 40 / 48 / 80 widths of atto / femto / nano) on the fp32 MFMA; 'f32' runs everything there.  Range guard: the flag word is read
once per call, and a call in which an f16x3 operand left the f16 range is re-run in 'f32' (`overflow_events` counts them).
"""
import ctypes as C
import math
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from ._lib import check, on_device_of, require_cuda, stream_of


class LayerNorm(nn.Module):
    """pose/convnextv2/utils.py:79-103: holds weight / bias; both data formats are a per-pixel LayerNorm on the device."""

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps, self.data_format, self.normalized_shape = eps, data_format, (normalized_shape,)


class GRN(nn.Module):
    """pose/convnextv2/utils.py:105-116."""

    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(1, 1, 1, dim))
        self.beta = nn.Parameter(torch.zeros(1, 1, 1, dim))


class Block(nn.Module):
    def __init__(self, dim, drop_path=0.0):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.grn = GRN(4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.drop_path = nn.Identity()       # stochastic depth is a training-time term


class ConvNeXtV2(nn.Module):
    def __init__(self, in_chans=3, num_classes=1000, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], drop_path_rate=0.0,
                 head_init_scale=1.0, precision="f16x3"):
        super().__init__()
        if in_chans != 3:
            raise NotImplementedError("ConvNeXtV2: the stem kernel reads 3-channel images")
        if len(depths) != 4 or len(dims) != 4 or any(d % 8 or d < 8 or d > 8192 for d in dims):
            raise ValueError("ConvNeXtV2: four stages, widths multiples of 8 up to 8192")
        if precision not in ("f16x3", "f32"):
            raise ValueError("precision must be 'f16x3' or 'f32'")
        self.depths, self.dims, self.num_classes = list(depths), list(dims), int(num_classes)
        self.drop_path_rate = drop_path_rate   # accepted and unused: inference only
        self.precision = precision
        self.on_overflow = "rerun_f32"
        self.overflow_events = 0
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4),
                                                    LayerNorm(dims[0], eps=1e-6, data_format="channels_first")))
        for i in range(3):
            self.downsample_layers.append(nn.Sequential(LayerNorm(dims[i], eps=1e-6, data_format="channels_first"),
                                                        nn.Conv2d(dims[i], dims[i + 1], kernel_size=2, stride=2)))
        self.stages = nn.ModuleList(nn.Sequential(*[Block(dims[i]) for _ in range(depths[i])]) for i in range(4))
        self.norm = nn.LayerNorm(dims[-1], eps=1e-6)
        self.head = nn.Linear(dims[-1], num_classes)
        self.apply(self._init_weights)
        self.head.weight.data.mul_(head_init_scale)
        self.head.bias.data.mul_(head_init_scale)
        self.eval()
        self._ws = None
        self._slots = None
        self._struct = {}       # precision -> (key, struct, keep)

    def _init_weights(self, m):
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.trunc_normal_(m.weight, std=0.02)
            nn.init.constant_(m.bias, 0)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("ConvNeXtV2 runs inference only (no drop path, no backward): keep it in eval()")
        return super().train(False)

    # ---- derived weights, cached per weight version -----------------------------------------------------------------------
    def _weights(self, precision):
        if self._slots is None:
            self._slots = _lib.param_slots(self)
        key = _lib.slots_key(self._slots)
        hit = self._struct.get(precision)
        if hit is not None and hit[0] == key:
            return hit[1]
        self._struct.pop(precision, None)
        lib, keep, w = _lib.lib(), [], _lib.ConvNextWeights()
        who = "ConvNeXtV2"
        x3 = precision == "f16x3"
        P = lambda t: _lib.param_ptr(t, keep, who)  # noqa: E731

        def WP(t):      # [N, K] fp32 -> weight planes, or None where the GEMM stays on the fp32 MFMA
            n, k = t.shape
            if not x3 or k % 32 or k < 64:
                return None
            t = t.detach().contiguous()
            require_cuda(t, who)
            pl = torch.empty(n, 2 * k, dtype=torch.float16, device=t.device)
            with on_device_of(t):
                check(lib.pope_split_planes_f32(_lib.ptr(t), C.c_void_p(pl.data_ptr()), n, k, _lib.PLANES_W_SCALE, None, stream_of(t.device)),
                      "pope_split_planes_f32")
            keep.append(pl)
            if float(t.abs().max()) * _lib.PLANES_W_SCALE >= _lib.F16_MAX:
                raise _lib.PopeRangeError(f"{who}: a weight leaves the f16x3 range contract (|w| * 256 < 65504): use precision='f32'")
            return C.c_void_p(pl.data_ptr())

        w.depths[:], w.dims[:], w.num_classes = self.depths, self.dims, self.num_classes
        stem = self.downsample_layers[0]
        w.stem_w, w.stem_b = P(stem[0].weight.reshape(self.dims[0], 48)), P(stem[0].bias)
        w.stem_ln_w, w.stem_ln_b = P(stem[1].weight), P(stem[1].bias)
        for i in range(3):
            ln, conv = self.downsample_layers[i + 1]
            m = conv.weight.detach().permute(0, 2, 3, 1).reshape(self.dims[i + 1], 4 * self.dims[i]).contiguous()   # (kh, kw, C_i)
            w.ds_ln_w[i], w.ds_ln_b[i], w.ds_w[i], w.ds_b[i] = P(ln.weight), P(ln.bias), P(m), P(conv.bias)
            w.ds_wp[i] = WP(m)
        blocks = (_lib.ConvNextBlockWeights * max(1, sum(self.depths)))()
        n = 0
        for stage in self.stages:
            for blk in stage:
                k = blocks[n]
                n += 1
                c = blk.dwconv.weight.shape[0]
                k.dw_w = P(blk.dwconv.weight.detach().reshape(c, 49).t())      # [49, C]
                k.dw_b, k.norm_w, k.norm_b = P(blk.dwconv.bias), P(blk.norm.weight), P(blk.norm.bias)
                k.pw1_w, k.pw1_b, k.pw2_w, k.pw2_b = P(blk.pwconv1.weight), P(blk.pwconv1.bias), P(blk.pwconv2.weight), P(blk.pwconv2.bias)
                k.grn_gamma, k.grn_beta = P(blk.grn.gamma.reshape(-1)), P(blk.grn.beta.reshape(-1))
                k.pw1_wp, k.pw2_wp = WP(blk.pwconv1.weight), WP(blk.pwconv2.weight)
        w.blocks_host = C.cast(blocks, C.POINTER(_lib.ConvNextBlockWeights))
        keep.append(blocks)
        w.norm_w, w.norm_b, w.head_w, w.head_b = P(self.norm.weight), P(self.norm.bias), P(self.head.weight), P(self.head.bias)
        w.ones = P(torch.ones(max(self.dims), dtype=torch.float32, device=self.norm.weight.device))
        self._struct[precision] = (key, w, keep)
        return w

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def _max_images(self, h, w):
        """Images per launch sequence: the GEMMs address their rows through 32-bit byte offsets."""
        worst = max((h // 4 >> i) * (w // 4 >> i) * 16 * self.dims[i] for i in range(4))
        return max(1, ((1 << 32) - 512 - 256 * 16 * max(self.dims)) // worst - 1)

    def _run(self, x, logits=True, taps=False, precision=None):
        who = "ConvNeXtV2"
        if self.training:
            raise NotImplementedError("ConvNeXtV2 runs inference only")
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{who} expects a torch tensor")
        require_cuda(x, who)
        if x.dtype != torch.float32:
            raise TypeError(f"{who}: expected float32, got {x.dtype}")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"{who}: expected [B, 3, H, W], got {tuple(x.shape)}")
        b, _, h, wd = x.shape
        if h % 32 or wd % 32 or h == 0 or wd == 0:
            raise ValueError(f"{who}: H and W must be multiples of 32 (the reference silently truncates {h} x {wd}); resize or pad the input")
        if logits and self.num_classes % 4:
            raise NotImplementedError(f"{who}: the head GEMM needs num_classes % 4 == 0 (forward_features has no such limit)")
        precision = precision or self.precision
        x = x.contiguous()
        dev = x.device
        feats = torch.empty(b, self.dims[3], dtype=torch.float32, device=dev)
        out = torch.empty(b, self.num_classes, dtype=torch.float32, device=dev) if logits else None
        tap_out = [torch.empty(b, h // 4 >> max(i - 1, 0), wd // 4 >> max(i - 1, 0), self.dims[max(i - 1, 0)], dtype=torch.float32, device=dev)
                   for i in range(5)] if taps else None
        if b == 0:
            return feats, out, tap_out
        w = self._weights(precision)
        lib = _lib.lib()
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        step = self._max_images(h, wd)
        for s in range(0, b, step):
            n = min(step, b - s)
            need = int(lib.pope_convnext_workspace_bytes(C.byref(w), n, h, wd))
            if need <= 0:
                raise ValueError(f"{who}: unsupported geometry {n} x {h} x {wd}")
            ws = _lib.grow_workspace(self, need, dev)
            tp = (C.c_void_p * 5)(*[t[s:s + n].data_ptr() for t in tap_out]) if taps else None
            with on_device_of(x):
                check(lib.pope_convnext_forward_f32(C.byref(w), _lib.ptr(x[s:s + n]), n, h, wd, _lib.PRECISIONS[precision],
                                                    _lib.ptr(feats[s:s + n]), _lib.ptr(out[s:s + n]) if logits else None, tp,
                                                    _lib.ptr(ws), ws.numel(), C.c_void_p(flag.data_ptr()), stream_of(dev)),
                      "pope_convnext_forward_f32")
        if precision != "f32":
            bits = int(flag.item())   # one sync per call: the range guard of every planes producer of the launch sequence
            if bits:
                _lib.range_event(self, f"pope_amd ConvNeXtV2: a value left the f16x3 range ({_lib.describe_range_bits(bits)})",
                                 "; re-running the call on the fp32 MFMA")
                return self._run(x, logits, taps, precision="f32")
        return feats, out, tap_out

    @torch.no_grad()
    def forward_features(self, x):
        return self._run(x, logits=False)[0]

    @torch.no_grad()
    def forward(self, x):
        return self._run(x)[1]

    @torch.no_grad()
    def forward_with_taps(self, x):
        """Test entry: (features [B, C3], logits [B, num_classes], [stem output, stage 0 .. 3 outputs] as NCHW views)."""
        f, o, t = self._run(x, taps=True)
        return f, o, [v.permute(0, 3, 1, 2) for v in t]


def convnextv2_atto(**kwargs):
    return ConvNeXtV2(depths=[2, 2, 6, 2], dims=[40, 80, 160, 320], **kwargs)


def convnextv2_femto(**kwargs):
    return ConvNeXtV2(depths=[2, 2, 6, 2], dims=[48, 96, 192, 384], **kwargs)


def convnext_pico(**kwargs):
    return ConvNeXtV2(depths=[2, 2, 6, 2], dims=[64, 128, 256, 512], **kwargs)


def convnextv2_nano(**kwargs):
    return ConvNeXtV2(depths=[2, 2, 8, 2], dims=[80, 160, 320, 640], **kwargs)


def convnextv2_tiny(**kwargs):
    return ConvNeXtV2(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], **kwargs)


def convnextv2_base(**kwargs):
    return ConvNeXtV2(depths=[3, 3, 27, 3], dims=[128, 256, 512, 1024], **kwargs)


def convnextv2_large(**kwargs):
    return ConvNeXtV2(depths=[3, 3, 27, 3], dims=[192, 384, 768, 1536], **kwargs)


def convnextv2_huge(**kwargs):
    return ConvNeXtV2(depths=[3, 3, 27, 3], dims=[352, 704, 1408, 2816], **kwargs)


FACTORIES = {f.__name__: f for f in (convnextv2_atto, convnextv2_femto, convnext_pico, convnextv2_nano, convnextv2_tiny,
                                     convnextv2_base, convnextv2_large, convnextv2_huge)}


def remap_checkpoint_keys(ckpt):
    """pose/utils.py:255-288: an FCMAE (sparse pre-training) checkpoint's names and shapes -> this module's.  Strips the
    `encoder.` prefix, turns `*.kernel` [k k, in, out] / [k k, C] into conv weights, drops the `ln` / `linear` path parts and
    reshapes the GRN parameters to [1, 1, 1, C] and 2-d biases to 1-d."""
    new_ckpt = OrderedDict()
    for k, v in ckpt.items():
        if k.startswith("encoder"):
            k = ".".join(k.split(".")[1:])
        if k.endswith("kernel"):
            new_k = ".".join(k.split(".")[:-1]) + ".weight"
            if v.dim() == 3:
                kv, in_dim, out_dim = v.shape
                ks = int(math.sqrt(kv))
                new_ckpt[new_k] = v.permute(2, 1, 0).reshape(out_dim, in_dim, ks, ks).transpose(3, 2)
            elif v.dim() == 2:
                kv, dim = v.shape
                ks = int(math.sqrt(kv))
                new_ckpt[new_k] = v.permute(1, 0).reshape(dim, 1, ks, ks).transpose(3, 2)
            continue
        if "ln" in k or "linear" in k:
            parts = k.split(".")
            parts.pop(-2)
            k = ".".join(parts)
        new_ckpt[k] = v
    for k, v in new_ckpt.items():
        if k.endswith("bias") and v.dim() != 1:
            new_ckpt[k] = v.reshape(-1)
        elif "grn" in k:
            new_ckpt[k] = v.unsqueeze(0).unsqueeze(1)
    return new_ckpt
