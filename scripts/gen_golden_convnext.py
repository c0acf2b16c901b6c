"""Writes tests/golden/convnext.npz: the reference's `pose/convnextv2/convnextv2.py:ConvNeXtV2` and the forward of
`pose/model_cnn.py:Mkpts_Reg_Model` run on the seeded weights and inputs of `pope_amd.synth` (run where the reference checkout
exists: `python scripts/gen_golden_convnext.py /path/to/reference`).

The reference modules do the work.  Their imports that nothing computed here needs get in-memory stand-ins: `timm.models.layers`
(`trunc_normal_` = torch's, an identity `DropPath`), an empty `MinkowskiEngine.SparseTensor`, `loguru`.  `model_cnn.py` itself is
not imported (its constructor insists on a checkpoint file): the pose cases compose the reference's `ConvNeXtV2(num_classes=32)`,
two `nn.Linear` and `qua2mat` / `o6d2mat` exactly as `model_cnn.forward` does.

Per case the file holds results only — the tests regenerate weights and inputs from the seeds: the module's own fp32 results and
an fp64 evaluation of the same module (deep copy, `.double()`) at the taps `synth.CONVNEXT_TAPS` (stem output, the four stage
outputs, forward_features, logits; wide taps at the seeded positions of `synth.convnext_tap_index`), for the pose cases pred_trans
and pred_rot, and per tap e32 = max |fp32 - fp64|, the reference's own fp32 error, which is what the GPU tests' bound is made of
(MARGIN x e32).

Asserted before anything is written, in fp64, for the logits of the backbone cases: zeroing every GRN gamma, keeping only the
centre tap of every depthwise kernel, and transposing the 2 x 2 downsample kernels each move the result by at least
DISCRIMINATION x the bound.  Also stored: the reference's state-dict keys and shapes of the eight factories (built on the meta
device), and names, shapes and an fp64 checksum per tensor of `remap_checkpoint_keys` applied to `synth.fcmae_checkpoint()`.
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import synth  # noqa: E402

MARGIN, DISCRIMINATION = 4.0, 100.0
FACTORIES = ("convnextv2_atto", "convnextv2_femto", "convnext_pico", "convnextv2_nano", "convnextv2_tiny", "convnextv2_base",
             "convnextv2_large", "convnextv2_huge")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    class DropPath(nn.Identity):
        pass

    layers = types.ModuleType("timm.models.layers")
    layers.trunc_normal_, layers.DropPath = nn.init.trunc_normal_, DropPath
    for n in ("timm", "timm.models"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["timm.models.layers"] = layers
    mink = types.ModuleType("MinkowskiEngine")
    mink.SparseTensor = type("SparseTensor", (), {})
    sys.modules.setdefault("MinkowskiEngine", mink)
    sys.modules.setdefault("loguru", types.SimpleNamespace(logger=types.SimpleNamespace(info=print)))
    pkg = types.ModuleType("_ref_convnextv2")
    pkg.__path__ = [os.path.join(ref_root, "pose", "convnextv2")]
    sys.modules["_ref_convnextv2"] = pkg
    _load("_ref_convnextv2.utils", os.path.join(pkg.__path__[0], "utils.py"))
    cnx = _load("_ref_convnextv2.convnextv2", os.path.join(pkg.__path__[0], "convnextv2.py"))
    utils = _load("_ref_pose_utils", os.path.join(ref_root, "pose", "utils.py"))
    if not hasattr(utils, "math"):      # remap_checkpoint_keys calls math.sqrt; the module never imports math
        import math
        utils.math = math
    return cnx, utils


def checksum(v):
    """Order-sensitive fp64 checksum of a tensor in its logical (row-major) order."""
    f = v.detach().double().reshape(-1)
    return float((f * torch.arange(1, f.numel() + 1, dtype=torch.float64)).sum())


def taps_of(model, x):
    out = {}
    for i in range(4):
        x = model.downsample_layers[i](x)
        if i == 0:
            out["stem"] = x
        x = model.stages[i](x)
        out[f"stage{i}"] = x
    out["features"] = model.norm(x.mean([-2, -1]))
    out["logits"] = model.head(out["features"])
    return out


def build(cnx, cfg, sd):
    m = cnx.ConvNeXtV2(depths=cfg["depths"], dims=cfg["dims"], num_classes=cfg["num_classes"]).eval()
    m.load_state_dict(sd, strict=True)
    return m, copy.deepcopy(m).double()


def run_backbone(cnx, name, blob):
    case = synth.convnext_case(name)
    m32, m64 = build(cnx, case["cfg"], case["state_dict"])
    x = case["x"]
    with torch.no_grad():
        t32, t64 = taps_of(m32, x), taps_of(m64, x.double())
        assert torch.equal(t32["logits"], m32(x)) and torch.equal(t32["features"], m32.forward_features(x))
        for tap in synth.CONVNEXT_TAPS:
            idx = synth.convnext_tap_index(name, tap, t32[tap].numel())
            a, b = t32[tap].reshape(-1)[idx], t64[tap].reshape(-1)[idx]
            e = float((a.double() - b).abs().max())
            blob.update({f"{name}.{tap}32": a.numpy(), f"{name}.{tap}64": b.numpy(), f"{name}.e32_{tap}": np.float64(e)})
            print(f"{name} {tap}: shape {tuple(t32[tap].shape)} |x| {float(b.abs().max()):.3g} e32 {e:.3g}")
        bound = MARGIN * float(blob[f"{name}.e32_logits"])
        variants = {}
        v = copy.deepcopy(m64)
        for mod in v.modules():
            if hasattr(mod, "gamma"):
                mod.gamma.zero_()
        variants["GRN gamma zeroed"] = v
        v = copy.deepcopy(m64)
        for st in v.stages:
            for blk in st:
                centre = blk.dwconv.weight[:, :, 3, 3].clone()
                blk.dwconv.weight.zero_()
                blk.dwconv.weight[:, :, 3, 3] = centre
        variants["dwconv centre tap only"] = v
        v = copy.deepcopy(m64)
        for i in range(1, 4):
            v.downsample_layers[i][1].weight.copy_(v.downsample_layers[i][1].weight.transpose(2, 3).clone())
        variants["downsample kernels transposed"] = v
        for what, vm in variants.items():
            d = float((vm(x.double()) - t64["logits"]).abs().max())
            assert d >= DISCRIMINATION * bound, (name, what, d, bound)
            print(f"  {name}: {what} moves the logits by {d:.3g} (bound {bound:.3g})")


def run_pose(cnx, utils, name, blob):
    case = synth.convnext_case(name)
    sd, mode = case["state_dict"], case["mode"]
    pre = "convnextv2.model."
    m32, m64 = build(cnx, case["cfg"], {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
    r = sd["rotation_head_rot.weight"].shape[0]
    th32, rh32 = nn.Linear(32, 3), nn.Linear(32, r)
    th32.load_state_dict({"weight": sd["translation_head_rot.weight"], "bias": sd["translation_head_rot.bias"]})
    rh32.load_state_dict({"weight": sd["rotation_head_rot.weight"], "bias": sd["rotation_head_rot.bias"]})
    th64, rh64 = copy.deepcopy(th32).double(), copy.deepcopy(rh32).double()

    def convert(x):   # model_cnn.py:convert2matrix
        return x.view(x.shape[0], 3, 3) if mode == "matrix" else utils.qua2mat(x) if mode == "quat" else utils.o6d2mat(x)

    with torch.no_grad():
        x = torch.cat((case["img0"], case["img1"]), dim=-1)
        f32, f64 = m32(x), m64(x.double())
        t32, R32, t64, R64 = th32(f32), convert(rh32(f32)), th64(f64), convert(rh64(f64))
    et, eR = float((t32.double() - t64).abs().max()), float((R32.double() - R64).abs().max())
    print(f"{name}: e32 t {et:.3g} R {eR:.3g}; |t| {float(t64.abs().max()):.3g}")
    blob.update({f"{name}.t32": t32.numpy(), f"{name}.t64": t64.numpy(), f"{name}.R32": R32.numpy(), f"{name}.R64": R64.numpy(),
                 f"{name}.e32_t": np.float64(et), f"{name}.e32_R": np.float64(eR)})


def main():
    cnx, utils = load_reference(sys.argv[1])
    torch.set_num_threads(8)
    blob = {}
    linspace = torch.linspace       # the constructor calls .item() on its drop-path schedule: that one tensor stays on the CPU
    for f in FACTORIES:
        torch.linspace = lambda *a, **k: linspace(*a, device="cpu", **k)
        try:
            with torch.device("meta"):
                sd = getattr(cnx, f)().state_dict()
        finally:
            torch.linspace = linspace
        blob[f"keys_{f}.names"] = np.array(list(sd))
        blob[f"keys_{f}.shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in sd.values()])
    out = utils.remap_checkpoint_keys(synth.fcmae_checkpoint())
    blob["remap.names"] = np.array(list(out))
    blob["remap.shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in out.values()])
    blob["remap.checksums"] = np.array([checksum(v) for v in out.values()])
    for name in synth.CONVNEXT_CASES:
        run_backbone(cnx, name, blob)
    for name in synth.CONVNEXT_POSE_CASES:
        run_pose(cnx, utils, name, blob)
    path = os.path.join(ROOT, "tests", "golden", "convnext.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
