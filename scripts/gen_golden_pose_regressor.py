"""Writes tests/golden/pose_regressor.npz: the reference's `pose/model.py:Mkpts_Reg_Model` run on the seeded weights and inputs of
`pope_amd.synth` (run where the reference checkout exists: `python scripts/gen_golden_pose_regressor.py /path/to/reference`).

The reference module does the work.  `pose/utils.py` imports `loguru`, which is not needed for anything computed here: an empty
stand-in is registered in sys.modules beforehand.

Per case (num_sample S, pairs per call B, mode) the file holds results only — the tests regenerate weights and inputs from the
seeds: the module's own fp32 results and an fp64 evaluation of the same module at four taps (embedding, encoder output,
pred_trans, pred_rot; the two wide taps at the sample slots of `synth.pose_regressor_tap_slots`, and once per (S, B): they do not
depend on the mode), and per tap e32 = max |fp32 - fp64|, the reference's own fp32 error, which is what the GPU test's bound is
made of (4 e32).  The fp64 evaluation takes sin and cos of the fp32-ROUNDED product f * x, as the module does in fp32: at up to
1.6e5 rad the rounding of the product is part of the function, not an error of it.

Asserted before anything is written, in fp64, for pred_trans and pred_rot of every case: zeroing the attention term (out_proj),
swapping sin and cos, and — for B > 1 — evaluating the pairs one per call each move the result by at least 100 x the bound.
Also stored: the reference's 78 state-dict keys and shapes at S = 5 per mode.
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pope_amd import synth  # noqa: E402

MARGIN, DISCRIMINATION = 4.0, 100.0


def load_reference(ref_root):
    sys.modules.setdefault("loguru", types.SimpleNamespace(logger=types.SimpleNamespace(info=print)))
    pkg = types.ModuleType("pose")
    pkg.__path__ = [os.path.join(ref_root, "pose")]
    sys.modules["pose"] = pkg
    for name in ("utils", "model"):
        spec = importlib.util.spec_from_file_location(f"pose.{name}", os.path.join(pkg.__path__[0], f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"pose.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["pose.model"].Mkpts_Reg_Model


def embed64(model, x32, swap=False):
    out = [x32.double()]
    for f in model.embedding.freq_bands:
        p = (f * x32).double()          # the fp32 product, as the module forms it
        out += [torch.cos(p), torch.sin(p)] if swap else [torch.sin(p), torch.cos(p)]
    return torch.cat(out, dim=-1)


def evaluate(model, emb):
    enc = model.transformer(emb)
    y = model.mlp(enc.reshape(enc.shape[0], -1))
    return enc, model.translation_head(y), model.convert2matrix(model.rotation_head(y))


def run_case(Model, S, B, modes, blob):
    d0, d1 = synth.pose_regressor_case(S, B)
    x32 = torch.cat((d0, d1), dim=-1)
    slots = synth.pose_regressor_tap_slots(S)
    tag = f"S{S}_B{B}"
    for mode in modes:
        m32 = Model(S, mode).eval()
        m32.load_state_dict(synth.pose_regressor_state_dict(S, mode), strict=True)
        m64 = copy.deepcopy(m32).double()
        with torch.no_grad():
            emb32 = m32.embedding(x32)
            enc32, t32, R32 = evaluate(m32, emb32)
            tf, Rf = m32(d0, d1)
            assert torch.equal(tf, t32) and torch.equal(Rf, R32)
            emb64 = embed64(m64, x32)
            enc64, t64, R64 = evaluate(m64, emb64)
            e = {"emb": float((emb32[:, slots].double() - emb64[:, slots]).abs().max()),
                 "enc": float((enc32[:, slots].double() - enc64[:, slots]).abs().max()),
                 "t": float((t32.double() - t64).abs().max()), "R": float((R32.double() - R64).abs().max())}
            # discrimination
            noattn = copy.deepcopy(m64)
            for layer in noattn.transformer.layers:
                layer.self_attn.out_proj.weight.zero_()
                layer.self_attn.out_proj.bias.zero_()
            variants = {"no attention": evaluate(noattn, emb64)[1:], "sin / cos swapped": evaluate(m64, embed64(m64, x32, swap=True))[1:]}
            if B > 1:
                singles = [evaluate(m64, emb64[b:b + 1])[1:] for b in range(B)]
                variants["one pair per call"] = (torch.cat([s[0] for s in singles]), torch.cat([s[1] for s in singles]))
            for name, (tv, Rv) in variants.items():
                dt, dR = float((tv - t64).abs().max()), float((Rv - R64).abs().max())
                assert dt >= DISCRIMINATION * MARGIN * e["t"] and dR >= DISCRIMINATION * MARGIN * e["R"], (tag, mode, name, dt, dR, e)
                print(f"  {tag} {mode}: {name} moves t by {dt:.3g}, R by {dR:.3g}")
        print(f"{tag} {mode}: e32 emb {e['emb']:.3g} enc {e['enc']:.3g} t {e['t']:.3g} R {e['R']:.3g}; |t| {float(t64.abs().max()):.3g}")
        if f"{tag}.emb64" not in blob:
            blob.update({f"{tag}.emb32": emb32[:, slots].numpy(), f"{tag}.emb64": emb64[:, slots].numpy(),
                         f"{tag}.enc32": enc32[:, slots].numpy(), f"{tag}.enc64": enc64[:, slots].numpy(),
                         f"{tag}.e32_emb": np.float64(e["emb"]), f"{tag}.e32_enc": np.float64(e["enc"])})
        else:   # the shared part does not depend on the mode
            assert np.array_equal(blob[f"{tag}.enc32"], enc32[:, slots].numpy())
        blob.update({f"{tag}_{mode}.t32": t32.numpy(), f"{tag}_{mode}.R32": R32.numpy(), f"{tag}_{mode}.t64": t64.numpy(),
                     f"{tag}_{mode}.R64": R64.numpy(), f"{tag}_{mode}.e32_t": np.float64(e["t"]), f"{tag}_{mode}.e32_R": np.float64(e["R"])})


def main():
    Model = load_reference(sys.argv[1])
    torch.set_num_threads(8)
    blob = {}
    for mode in synth.POSE_REGRESSOR_MODES:
        sd = Model(5, mode).state_dict()
        assert len(sd) == 78
        blob[f"keys_S5_{mode}.names"] = np.array(list(sd))
        blob[f"keys_S5_{mode}.shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in sd.values()])
    for S, B in synth.POSE_REGRESSOR_CASES:
        run_case(Model, S, B, list(synth.POSE_REGRESSOR_MODES), blob)
    run_case(Model, *synth.POSE_REGRESSOR_LARGE, ["matrix"], blob)
    path = os.path.join(ROOT, "tests", "golden", "pose_regressor.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
