"""Writes tests/golden/mocope.npz and mocope_fp32.npz: the reference's `pose/model0604.py:MoCoPE` run on the seeded weights and inputs of
`pope_amd.synth` (run where the reference checkout exists: `python scripts/gen_golden_mocope.py /path/to/reference`).

The reference module does the work.  Its imports that nothing computed here needs get the in-memory stand-ins of
`gen_golden_convnext.py` (`timm.models.layers`, `MinkowskiEngine`, `loguru`); `pose`, `pose.convnextv2` and `pose.utils` are
registered by file path (the package's own `__init__` is not run), `pose.utils.math` is set, and the module's `ConvNeXtV2`
wrapper class, which insists on a checkpoint file, is replaced by one that builds the reference's own `ConvNeXtV2` trunk at the
widths of `synth.MOCOPE_TRUNK` (1000 classes).

Per case (num_sample S, pairs per call B, mode, train_type; the taps in front of the heads once per (S, B, train_type), the
modes share them) the file holds results only — the tests regenerate weights and
inputs from the seeds: the module's own fp32 results and an fp64 evaluation of the same module (deep copy, `.double()`) at the
taps of `synth.MOCOPE_TAPS` plus pred_trans and pred_rot (the three [B, S, 76] taps at the sample slots of
`synth.pose_regressor_tap_slots`, the four [B, 2, 512] taps at the columns `synth.MOCOPE_TAP_COLUMNS`), and per tap e32 = max |fp32 - fp64|, the reference's own fp32 error, which is what the GPU
test's bound is made of (MARGIN x e32).  The fp64 evaluation takes sin and cos of the fp32-ROUNDED product f * x, the convention
of `gen_golden_pose_regressor.py`.

Asserted before anything is written, in fp64, for pred_trans and pred_rot of every fusion case up to S = 70: zeroing the
decoders' `multihead_attn.out_proj` (no cross-attention), swapping src and tgt of `mkpts_as_q`, dropping `encoder.norm` and
`decoder.norm`, and — for B > 1, where a softmax has more than one term — two heads instead of one at d = 76 and evaluating the
pairs one per call each move the result by at least DISCRIMINATION x the bound.  Also stored: the reference's state-dict keys
and shapes outside `convnextv2.model.*` at S = 5 per mode.
"""
import copy
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pope_amd import synth  # noqa: E402
from gen_golden_convnext import _load  # noqa: E402

MARGIN, DISCRIMINATION = 4.0, 100.0


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
    pose = types.ModuleType("pose")
    pose.__path__ = [os.path.join(ref_root, "pose")]
    sys.modules["pose"] = pose
    sub = types.ModuleType("pose.convnextv2")
    sub.__path__ = [os.path.join(ref_root, "pose", "convnextv2")]
    sys.modules["pose.convnextv2"] = sub
    _load("pose.convnextv2.utils", os.path.join(sub.__path__[0], "utils.py"))
    sub.convnextv2 = cnx = _load("pose.convnextv2.convnextv2", os.path.join(sub.__path__[0], "convnextv2.py"))
    utils = _load("pose.utils", os.path.join(ref_root, "pose", "utils.py"))
    if not hasattr(utils, "math"):
        import math
        utils.math = math
    mod = _load("pose.model0604", os.path.join(ref_root, "pose", "model0604.py"))

    class Trunk(nn.Module):     # in place of the wrapper that loads a checkpoint file: same attribute (.model), same forward
        def __init__(self, num_classes=1000, model_type="base"):
            super().__init__()
            cfg = synth.MOCOPE_TRUNK
            self.model = cnx.ConvNeXtV2(depths=cfg["depths"], dims=cfg["dims"], num_classes=cfg["num_classes"])

        def forward(self, x):
            return self.model(x)

    mod.ConvNeXtV2 = Trunk
    return mod.MoCoPE


def embed64(model, x32):
    out = [x32.double()]
    for f in model.embedding.freq_bands:
        p = (f * x32).double()          # the fp32 product, as the module forms it
        out += [torch.sin(p), torch.cos(p)]
    return torch.cat(out, dim=-1)


def evaluate(m, emb, img0, img1, swap_fusion=False):
    """MoCoPE.forward from the embedding on, with the taps; follows model0604.py:253-300 line by line."""
    o, tt = {"embedding": emb}, m.train_type
    if tt != "cnn":
        o["memory"] = m.transformer_mkpts.encoder(emb)
        o["transformer_mkpts"] = m.transformer_mkpts(emb, emb)
        x = m.mlp1(o["transformer_mkpts"].reshape(emb.shape[0], -1))
        o["x_mkpts"] = x.reshape(x.shape[0], 2, -1)
    if tt != "mkpts":
        o["x_img"] = torch.cat((m.mlp_img(m.convnextv2(img0)).unsqueeze(1), m.mlp_img(m.convnextv2(img1)).unsqueeze(1)), dim=1)
    if tt == "mkpts+cnn":
        o["qmkpts"] = m.mkpts_as_q(o["x_mkpts"], o["x_img"]) if swap_fusion else m.mkpts_as_q(o["x_img"], o["x_mkpts"])
        o["qimg"] = m.cnn_as_q(o["x_mkpts"], o["x_img"])
        x = torch.cat((o["qmkpts"], o["qimg"]), dim=-1)
    elif tt == "mkpts":
        o["qmkpts"] = m.mkpts_as_q(o["x_mkpts"], o["x_mkpts"])
        x = torch.cat((o["qmkpts"], o["qmkpts"]), dim=-1)
    else:
        o["qimg"] = m.cnn_as_q(o["x_img"], o["x_img"])
        x = torch.cat((o["qimg"], o["qimg"]), dim=-1)
    y = m.mlp2(x.reshape(x.shape[0], -1))
    o["t"], o["R"] = m.translation_head(y), m.convert2matrix(m.rotation_head(y))
    return o


def variants(m64, emb64, i0, i1, B):
    """name -> (pred_trans, pred_rot) of the fp64 model with one ingredient changed"""
    out = {}
    v = copy.deepcopy(m64)
    for t in (v.transformer_mkpts, v.mkpts_as_q, v.cnn_as_q):
        for layer in t.decoder.layers:
            layer.multihead_attn.out_proj.weight.zero_()
            layer.multihead_attn.out_proj.bias.zero_()
    out["no cross-attention"] = evaluate(v, emb64, i0, i1)
    out["mkpts_as_q src / tgt swapped"] = evaluate(m64, emb64, i0, i1, swap_fusion=True)
    v = copy.deepcopy(m64)
    for t in (v.transformer_mkpts, v.mkpts_as_q, v.cnn_as_q):
        t.encoder.norm = t.decoder.norm = None
    out["closing norms dropped"] = evaluate(v, emb64, i0, i1)
    del v
    if B > 1:       # with one pair per call every softmax has one term: neither of these two can show
        v = copy.deepcopy(m64)
        for mod in v.transformer_mkpts.modules():
            if isinstance(mod, nn.MultiheadAttention):
                mod.num_heads, mod.head_dim = 2, 38
        out["two heads at d = 76"] = evaluate(v, emb64, i0, i1)
        del v
        singles = [evaluate(m64, emb64[b:b + 1], i0[b:b + 1], i1[b:b + 1]) for b in range(B)]
        out["one pair per call"] = {k: torch.cat([s[k] for s in singles]) for k in ("t", "R")}
    return {k: (o["t"], o["R"]) for k, o in out.items()}


def run_case(Model, S, B, mode, train_type, blob, discriminate):
    d0, d1, img0, img1 = synth.mocope_case(S, B)
    x32 = torch.cat((d0, d1), dim=-1)
    slots = synth.pose_regressor_tap_slots(S)
    tag, shared = f"S{S}_B{B}_{mode}_{train_type}", f"S{S}_B{B}_{train_type}"
    m32 = Model(S, mode, "base", train_type).eval()
    m32.load_state_dict(synth.mocope_state_dict(S, mode), strict=True)
    m64 = copy.deepcopy(m32).double()
    with torch.no_grad():
        o32 = evaluate(m32, m32.embedding(x32), img0, img1)
        tf, Rf = m32(d0, d1, img0, img1)
        assert torch.equal(tf, o32["t"]) and torch.equal(Rf, o32["R"])
        emb64 = embed64(m64, x32)
        o64 = evaluate(m64, emb64, img0.double(), img1.double())
        e = {}
        for k in synth.MOCOPE_TAPS_OF[train_type] + ("t", "R"):
            a, b = o32[k], o64[k]
            if k in ("embedding", "memory", "transformer_mkpts"):
                a, b = a[:, slots], b[:, slots]
            elif k not in ("t", "R"):
                a, b = a[..., synth.MOCOPE_TAP_COLUMNS], b[..., synth.MOCOPE_TAP_COLUMNS]
            e[k] = float((a.double() - b).abs().max())
            where = tag if k in ("t", "R") else shared      # the taps in front of the heads do not depend on the mode
            if f"{where}.{k}64" in blob:
                assert np.array_equal(blob[f"{where}.{k}32"], a.numpy())
            blob.update({f"{where}.{k}32": a.numpy(), f"{where}.{k}64": b.numpy(), f"{where}.e32_{k}": np.float64(e[k])})
        print(f"{tag}: e32 " + " ".join(f"{k} {v:.3g}" for k, v in e.items()) + f"; |t| {float(o64['t'].abs().max()):.3g}")
        if discriminate:
            for name, (tv, Rv) in variants(m64, emb64, img0.double(), img1.double(), B).items():
                dt, dR = float((tv - o64["t"]).abs().max()), float((Rv - o64["R"]).abs().max())
                print(f"  {tag}: {name} moves t by {dt:.3g}, R by {dR:.3g}")
                assert dt >= DISCRIMINATION * MARGIN * e["t"] and dR >= DISCRIMINATION * MARGIN * e["R"], (tag, name, dt, dR, e)


def main():
    Model = load_reference(sys.argv[1])
    torch.set_num_threads(8)
    blob = {}
    for mode in synth.POSE_REGRESSOR_MODES:
        sd = {k: v for k, v in Model(5, mode).state_dict().items() if not k.startswith("convnextv2.")}
        blob[f"keys_S5_{mode}.names"] = np.array("\n".join(sd))        # one string each: 576 fixed-width entries are 150 KB a mode
        blob[f"keys_S5_{mode}.shapes"] = np.array("\n".join("x".join(str(d) for d in v.shape) for v in sd.values()))
    for S, B in synth.MOCOPE_CASES:
        for mode in (synth.POSE_REGRESSOR_MODES if S == synth.MOCOPE_MODES_AT else ("6d",)):
            run_case(Model, S, B, mode, "mkpts+cnn", blob, True)
    for tt in ("mkpts", "cnn"):
        run_case(Model, *synth.MOCOPE_REDUCED, "6d", tt, blob, False)
    run_case(Model, *synth.MOCOPE_WIDE, "6d", "mkpts+cnn", blob, False)
    save(blob)


def save(blob):
    """Two files, each under the size limit of a committed file: mocope.npz is what the tests read (fp64 results, e32, key names),
    mocope_fp32.npz the reference's own fp32 results the e32 figures were taken from."""
    fp32 = {k: v for k, v in blob.items() if k.endswith("32") and ".e32_" not in k}
    rest = {k: v for k, v in blob.items() if k not in fp32}
    for name, part in (("mocope.npz", rest), ("mocope_fp32.npz", fp32)):
        path = os.path.join(ROOT, "tests", "golden", name)
        np.savez_compressed(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
