"""Writes tests/golden/vim.npz: the reference's `pose/vim/models_mamba.py:VisionMamba` run on the seeded weights and inputs of
`pope_amd.synth` (run where the reference checkout exists: `python scripts/gen_golden_vim.py /path/to/reference`).

`VisionMamba`, `Block`, `PatchEmbed` and the four factories are the reference's own code, imported by file path.  Its imports
get in-memory stand-ins: `timm` (torch's `trunc_normal_`, a `lecun_normal_`, an identity `DropPath`, `to_2tuple`, a no-op
`register_model`, `_cfg`, `_load_weights`, a `VisionTransformer` placeholder), `pose.vim.rope` (empty) and `mamba_ssm`, which is
not part of the reference tree: `Mamba` below is the bidirectional "v2" mixer written down from the Mamba paper (Algorithm 2) and
the Vim paper (Algorithm 1) as a plain sequential loop over time, `RMSNorm`, `rms_norm_fn` and `layer_norm_fn` are restated with
their `prenorm` / `residual` arguments.  The mixer is therefore NOT pinned against the third-party package.

Per case the file holds results only - the tests regenerate weights and inputs from the seeds: the module's own fp32 values and
an fp64 evaluation of the same module (deep copy, `.double()`) at the taps `synth.VIM_TAPS` (the token matrix, hidden + residual
after layers 0, 11 and 23, forward_features, logits; wide taps at the seeded positions of `synth.vim_tap_index`), and per tap
e32 = max |fp32 - fp64|, the reference's own fp32 error, which is what the GPU tests' bound is made of (MARGIN x e32).

Asserted before anything is written, in fp64, for the logits of the small stride-8 case: swapping the forward and backward
parameter sets, omitting the / 2, shifting the conv taps by one (non-causal), softplus replaced by the identity, the class token
at position 0, and D = 0 each move the result by at least DISCRIMINATION x the bound.  Also stored: the reference's state-dict
keys and shapes of the four factories (built on the meta device), and the `Vim` loader's pos_embed resampling (model0606.py
lines 116-134, restated by `pope_amd.vim.resample_pos_embed` - checked here against torch's interpolate called as the reference
calls it) of a seeded 14 x 14 checkpoint onto the 27 x 27 grid, as checksum and samples.
"""
import copy
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import synth  # noqa: E402

MARGIN, DISCRIMINATION = 4.0, 100.0
FACTORIES = ("vim_tiny_patch16_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2",
             "vim_tiny_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2",
             "vim_small_patch16_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2",
             "vim_small_patch16_stride8_224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2")
TAP_LAYERS = {"layer0": 0, "layer11": 11, "layer23": 23}


# ---- the mamba_ssm stand-in ---------------------------------------------------------------------------------------------------
class Mamba(nn.Module):
    """The mixer of the issue's specification (d_state 16, d_conv 4, expand 2, dt_rank ceil(d_model / 16)), one step at a time.
    `variant` switches the wrong forms of the discrimination checks on."""
    variant = None

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", conv_bias=True, bias=False, layer_idx=None,
                 device=None, dtype=None, bimamba_type="none", if_devide_out=False, init_layer_scale=None, **unused):
        super().__init__()
        assert bimamba_type == "v2" and init_layer_scale is None and d_conv == 4 and not bias and conv_bias
        kw = {"device": device, "dtype": dtype}
        e = expand * d_model
        r = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        self.d_model, self.d_inner, self.d_state, self.d_conv, self.dt_rank, self.if_devide_out = d_model, e, d_state, d_conv, r, if_devide_out
        a_log = torch.log(torch.arange(1, d_state + 1, dtype=torch.float32, device=device)).repeat(e, 1)
        self.in_proj = nn.Linear(d_model, 2 * e, bias=False, **kw)
        self.conv1d = nn.Conv1d(e, e, d_conv, groups=e, padding=d_conv - 1, **kw)
        self.x_proj = nn.Linear(e, r + 2 * d_state, bias=False, **kw)
        self.dt_proj = nn.Linear(r, e, **kw)
        self.A_log = nn.Parameter(a_log.clone())
        self.D = nn.Parameter(torch.ones(e, device=device))
        self.A_b_log = nn.Parameter(a_log.clone())
        self.conv1d_b = nn.Conv1d(e, e, d_conv, groups=e, padding=d_conv - 1, **kw)
        self.x_proj_b = nn.Linear(e, r + 2 * d_state, bias=False, **kw)
        self.dt_proj_b = nn.Linear(r, e, **kw)
        self.D_b = nn.Parameter(torch.ones(e, device=device))
        self.out_proj = nn.Linear(e, d_model, bias=False, **kw)

    def direction(self, x, z, conv, x_proj, dt_proj, A_log, D):
        """x, z [B, L, E] -> o [B, L, E], the sequence as given."""
        B, L, E = x.shape
        n, r = self.d_state, self.dt_rank
        shift = 1 if self.variant == "conv_shift" else 0
        xp = F.pad(x, (0, 0, 3 - shift, shift))                          # zeros before t = 0 (and, shifted, one after the end)
        w = conv.weight[:, 0, :]                                         # [E, 4]
        xc = conv.bias + sum(w[:, k] * xp[:, k:k + L, :] for k in range(4))   # sum_k w[k] x[t - 3 + k]
        xc = F.silu(xc)
        dbc = x_proj(xc)
        dt, Bm, Cm = dbc[..., :r], dbc[..., r:r + n], dbc[..., r + n:]
        delta = dt_proj(dt)
        if self.variant != "no_softplus":
            delta = F.softplus(delta)
        A = -torch.exp(A_log)                                            # [E, N]
        h = x.new_zeros(B, E, n)
        ys = []
        for t in range(L):
            d_t = delta[:, t, :, None]                                   # [B, E, 1]
            h = torch.exp(d_t * A) * h + (d_t * xc[:, t, :, None]) * Bm[:, t, None, :]
            ys.append((h * Cm[:, t, None, :]).sum(-1) + D * xc[:, t])
        return torch.stack(ys, dim=1) * F.silu(z)

    def forward(self, hidden_states, inference_params=None):
        assert inference_params is None
        xz = self.in_proj(hidden_states)
        x, z = xz[..., :self.d_inner], xz[..., self.d_inner:]
        fwd = (self.conv1d, self.x_proj, self.dt_proj, self.A_log, self.D)
        bwd = (self.conv1d_b, self.x_proj_b, self.dt_proj_b, self.A_b_log, self.D_b)
        if self.variant == "swap":
            fwd, bwd = bwd, fwd
        o = self.direction(x, z, *fwd) + self.direction(x.flip(1), z.flip(1), *bwd).flip(1)
        if self.if_devide_out and self.variant != "no_div":
            o = o / 2
        return self.out_proj(o)


class RMSNorm(nn.Module):
    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)

    def forward(self, x):
        return rms_norm_fn(x, self.weight, None, eps=self.eps)


def rms_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, **unused):
    if residual is not None:
        x = x + residual
    out = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * weight
    if bias is not None:
        out = out + bias
    return (out, x) if prenorm else out


def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, **unused):
    if residual is not None:
        x = x + residual
    out = F.layer_norm(x, x.shape[-1:], weight, bias, eps)
    return (out, x) if prenorm else out


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference(ref_root):
    class DropPath(nn.Identity):
        def __init__(self, drop_prob=0.0):
            super().__init__()

    def lecun_normal_(t):
        fan_in = t[0].numel()
        return nn.init.trunc_normal_(t, std=math.sqrt(1.0 / fan_in) / 0.87962566103423978)

    for n in ("timm", "timm.models", "mamba_ssm", "mamba_ssm.modules", "mamba_ssm.utils", "mamba_ssm.ops", "mamba_ssm.ops.triton", "pose",
              "pose.vim"):
        _module(n)
    _module("timm.models.vision_transformer", VisionTransformer=type("VisionTransformer", (nn.Module,), {}), _cfg=lambda **k: dict(k),
            _load_weights=lambda *a, **k: None)
    _module("timm.models.registry", register_model=lambda f: f)
    _module("timm.models.layers", trunc_normal_=nn.init.trunc_normal_, lecun_normal_=lecun_normal_, DropPath=DropPath,
            to_2tuple=lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v))
    _module("mamba_ssm.modules.mamba_simple", Mamba=Mamba)
    _module("mamba_ssm.utils.generation", GenerationMixin=type("GenerationMixin", (), {}))
    _module("mamba_ssm.utils.hf", load_config_hf=lambda *a, **k: None, load_state_dict_hf=lambda *a, **k: None)
    _module("mamba_ssm.ops.triton.layernorm", RMSNorm=RMSNorm, layer_norm_fn=layer_norm_fn, rms_norm_fn=rms_norm_fn)
    _module("pose.vim.rope", __all__=[])
    spec = importlib.util.spec_from_file_location("_ref_models_mamba", os.path.join(ref_root, "pose", "vim", "models_mamba.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["_ref_models_mamba"] = mod
    spec.loader.exec_module(mod)
    return mod


def checksum(v):
    """Order-sensitive fp64 checksum of a tensor in its logical (row-major) order."""
    f = v.detach().double().reshape(-1)
    return float((f * torch.arange(1, f.numel() + 1, dtype=torch.float64)).sum())


def factory_of(cfg):
    size = "tiny" if cfg["embed_dim"] == 192 else "small"
    return f"vim_{size}_patch16_{'stride8_' if cfg['stride'] == 8 else ''}224_bimambav2_final_pool_mean_abs_pos_embed_with_midclstok_div2"


def build(ref, case):
    cfg = case["cfg"]
    m = getattr(ref, factory_of(cfg))(img_size=cfg["img_size"], num_classes=cfg["num_classes"]).eval()
    assert m.layers[0].mixer.d_model == cfg["embed_dim"] and len(m.layers) == cfg["depth"]
    m.load_state_dict(case["state_dict"], strict=True)
    return m


def taps_of(model, x):
    """The reference forward with hooks on its layers: tokens = what layer 0 receives, layer i = hidden + residual behind it."""
    out, hooks = {}, []
    hooks.append(model.layers[0].register_forward_pre_hook(lambda mod, args: out.__setitem__("tokens", args[0].clone())))
    for tap, i in TAP_LAYERS.items():
        hooks.append(model.layers[i].register_forward_hook(lambda mod, args, res, tap=tap: out.__setitem__(tap, res[0] + res[1])))
    out["logits"] = model(x)
    for h in hooks:
        h.remove()
    out["features"] = model(x, return_features=True)
    return out


def run_case(ref, name, blob):
    case = synth.vim_case(name)
    m32 = build(ref, case)
    m64 = copy.deepcopy(m32).double()
    x = case["x"]
    with torch.no_grad():
        t32, t64 = taps_of(m32, x), taps_of(m64, x.double())
        for tap in synth.VIM_TAPS:
            idx = synth.vim_tap_index(name, tap, t32[tap].numel())
            a, b = t32[tap].reshape(-1)[idx], t64[tap].reshape(-1)[idx]
            e = float((a.double() - b).abs().max())
            blob.update({f"{name}.{tap}32": a.numpy(), f"{name}.{tap}64": b.numpy(), f"{name}.e32_{tap}": np.float64(e)})
            print(f"{name} {tap}: shape {tuple(t32[tap].shape)} |x| max {float(b.abs().max()):.3g} rms {float(b.pow(2).mean().sqrt()):.3g} "
                  f"e32 {e:.3g}", flush=True)
        # per-term magnitudes of the first and the last layer (the scaling check of synth.vim_state_dict)
        for i in (0, len(m64.layers) - 1):
            seen = {}
            h = m64.layers[i].mixer.register_forward_hook(lambda mod, args, res: seen.update(u=args[0], out=res))
            m64(x.double())
            h.remove()
            print(f"  {name} layer {i}: mixer input rms {float(seen['u'].pow(2).mean().sqrt()):.3g}, mixer output rms "
                  f"{float(seen['out'].pow(2).mean().sqrt()):.3g}", flush=True)
        if name != "small_s8":
            return
        bound = MARGIN * float(blob[f"{name}.e32_logits"])
        xd = x.double()

        def moved(model, variant=None):
            Mamba.variant = variant
            try:
                return float((model(xd) - t64["logits"]).abs().max())
            finally:
                Mamba.variant = None

        results = {"forward and backward parameter sets swapped": moved(m64, "swap"), "without the / 2": moved(m64, "no_div"),
                   "conv taps shifted by one (non-causal)": moved(m64, "conv_shift"), "softplus replaced by the identity": moved(m64, "no_softplus")}
        v = copy.deepcopy(m64)
        v.use_middle_cls_token = False
        results["class token at position 0"] = moved(v)
        v = copy.deepcopy(m64)
        for layer in v.layers:
            layer.mixer.D.zero_()
            layer.mixer.D_b.zero_()
        results["D = 0"] = moved(v)
        for what, d in results.items():
            if not math.isfinite(d):     # a wrong form that overflows (a negative delta makes the recurrence grow) has moved all the way
                d = math.inf
            print(f"  {name}: {what} moves the logits by {d:.3g} (bound {bound:.3g})", flush=True)
            assert d >= DISCRIMINATION * bound, (name, what, d, bound)


def main():
    ref = load_reference(sys.argv[1])
    torch.set_num_threads(8)
    blob = {}
    linspace = torch.linspace       # the constructor calls .item() on its drop-path schedule: that one tensor stays on the CPU
    for f in FACTORIES:
        torch.linspace = lambda *a, **k: linspace(*a, device="cpu", **k)
        try:
            with torch.device("meta"):
                sd = getattr(ref, f)().state_dict()
        finally:
            torch.linspace = linspace
        blob[f"keys_{f}.names"] = np.array(list(sd))
        blob[f"keys_{f}.shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in sd.values()])
    # the Vim loader's resampling, as model0606.py calls torch: 14 x 14 + class token -> 27 x 27 + class token
    from pope_amd import vim
    ck = synth.vim_pos_embed_checkpoint()["model"]["pos_embed"]
    new = vim.resample_pos_embed(ck, 27 * 27, 1)
    grid = F.interpolate(ck[:, 1:].reshape(-1, 14, 14, 384).permute(0, 3, 1, 2), size=(27, 27), mode="bicubic", align_corners=False)
    assert torch.equal(new, torch.cat((ck[:, :1], grid.permute(0, 2, 3, 1).flatten(1, 2)), dim=1)) and tuple(new.shape) == (1, 730, 384)
    idx = synth.vim_tap_index("pos_embed", "resampled", new.numel())
    blob.update({"pos_embed.orig_size": np.int64(14), "pos_embed.new_size": np.int64(27), "pos_embed.checksum": np.float64(checksum(new)),
                 "pos_embed.samples": new.reshape(-1)[idx].numpy()})
    for name in synth.VIM_CASES:
        run_case(ref, name, blob)
    path = os.path.join(ROOT, "tests", "golden", "vim.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
