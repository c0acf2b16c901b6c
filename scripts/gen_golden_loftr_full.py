"""Writes tests/golden/loftr_full.npz and tests/golden/loftr_full_128.npz: the reference's LoFTR modules with
attention = 'full' (run where the reference checkout exists: `python scripts/gen_golden_loftr_full.py /path/to/reference`).
The reference's own code does the work:
  * loftr_full.npz: `LoFTREncoderLayer` / `LocalFeatureTransformer` of src/matcher/loftr_module/transformer.py (with
    linear_attention.py beside it), loaded by file path under a synthetic package — torch is the only dependency — on the
    cases of `pope_amd.synth.loftr_full_case` under `synth.synthetic_matcher_state_dict(0)`;
  * loftr_full_128.npz: the reference `Matcher` with coarse.attention = fine.attention = 'full' and thr = 1e-3, built with the
    stand-ins of oracle/gen_golden.py:load_reference_matcher (read, not modified), on `synth.loftr_full_matcher_case`.  Per
    case the keys of loftr_256_lowthr.npz under the prefix '<case>.' (feat_c0_b0 / feat_c1_b0: every second row of pair 0, which
    keeps the file under 1 MB).
Stored: results only (strided taps where `loftr_full_case` says so); the tests regenerate inputs and weights from the seeds.
Before writing, tests/loftr_full_checks.py (the CPU restatement the GPU tests measure against) is checked against the
reference's outputs.
"""
import contextlib
import copy
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from pope_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)   # tests/conftest.py:GOLDEN_THREADS


def load_reference_transformer(ref_root):
    base = os.path.join(ref_root, "src", "matcher", "loftr_module")
    pkg = types.ModuleType("ref_loftr_module")
    pkg.__path__ = [base]
    sys.modules["ref_loftr_module"] = pkg
    mods = {}
    for name in ("linear_attention", "transformer"):
        spec = importlib.util.spec_from_file_location("ref_loftr_module." + name, os.path.join(base, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["ref_loftr_module." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["transformer"]


def maxdiff(a, b):
    return float((a - b).abs().max())


def gen_modules(ref_root, sd):
    import loftr_full_checks as K
    from pope_amd.matcher import default_cfg
    tr = load_reference_transformer(ref_root)
    out = {}
    for name in synth.LOFTR_FULL_CASES:
        case = synth.loftr_full_case(name)
        stage = case["stage"]
        prefix = f"loftr_{stage}."
        cfg = dict(default_cfg[stage], attention="full")
        f0, f1 = case["feat0"], case["feat1"]
        with torch.no_grad():
            if case["layer_names"] is None:
                layer = tr.LoFTREncoderLayer(cfg["d_model"], cfg["nhead"], "full").eval()
                lp = prefix + "layers.0."
                layer.load_state_dict({k[len(lp):]: v for k, v in sd.items() if k.startswith(lp)}, strict=True)
                got = (layer(f0, f0 if f1 is None else f1), None)
            else:
                cfg["layer_names"] = list(case["layer_names"])
                with contextlib.redirect_stdout(io.StringIO()):   # (the reference's constructor prints the layer names)
                    t = tr.LocalFeatureTransformer(cfg).eval()
                keys = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
                t.load_state_dict({k: v for k, v in keys.items() if int(k.split(".")[1]) < len(cfg["layer_names"])}, strict=True)
                got = t(f0, f1)
        mine = K.run_case(sd, case)
        sd64 = {k: v.double() for k, v in sd.items()}
        exact = K.run_case(sd64, case)
        for i, (g, m, e, tap) in enumerate(zip(got, mine, exact, case["taps"])):
            if g is None:
                continue
            print(f"{name}.out{i}: {tuple(g.shape)} |x| max {float(g.abs().max()):.2f}; restatement vs reference {maxdiff(g, m):.1e}; "
                  f"reference fp32 vs fp64 {maxdiff(g.double(), e):.1e}")
            assert maxdiff(g, m) <= 1e-5 and bool(torch.isfinite(g).all())
            out[f"{name}.out{i}"] = synth.loftr_full_tap(g, tap).contiguous().numpy()
    np.savez(os.path.join(OUT, "loftr_full.npz"), weights_seed=0, **out)


def gen_matcher(ref_root, sd):
    import loftr_full_checks as K
    from pope_amd.matcher import default_cfg as my_cfg
    sys.path.insert(1, ref_root)
    from oracle import gen_golden   # the stand-ins for yacs / kornia and the reference's default config
    gen_golden.load_reference_matcher()
    from src.matcher import Matcher, default_cfg
    thr = 1e-3
    out = {}
    for name in ("pairs128", "96x128_vs_128x96"):
        i0, i1 = synth.loftr_full_matcher_case(name)
        cfg = copy.deepcopy(default_cfg)
        cfg["coarse"]["attention"] = cfg["fine"]["attention"] = "full"
        cfg["match_coarse"]["thr"] = thr
        with contextlib.redirect_stdout(io.StringIO()):
            ref = Matcher(cfg).eval()
        ref.load_state_dict({"matcher." + k: v.clone() for k, v in sd.items()}, strict=True)
        data = {"image0": i0, "image1": i1}
        with torch.no_grad():
            ref(data)
            fc0, fc1 = ref({"image0": i0, "image1": i1}, only_att_fea=True)
            bc, bf = ref.backbone(torch.cat([i0, i1], 0) if i0.shape == i1.shape else i0)
        cfg2 = copy.deepcopy(my_cfg)
        cfg2["coarse"]["attention"] = cfg2["fine"]["attention"] = "full"
        cfg2["match_coarse"]["thr"] = thr
        with torch.no_grad():
            mine = K.matcher_forward(sd, cfg2, i0, i1)
        d = {"feat_c0": maxdiff(fc0, mine["feat_c0"]), "feat_c1": maxdiff(fc1, mine["feat_c1"]),
             "conf": maxdiff(data["conf_matrix"], mine["conf_matrix"])}
        for k in ("b_ids", "i_ids", "j_ids"):
            assert torch.equal(data[k], mine[k]), k
        for k in ("mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f"):
            d[k] = maxdiff(data[k], mine[k])
        print(name, "matches", len(data["b_ids"]), "restatement vs reference:", {k: f"{v:.1e}" for k, v in d.items()})
        assert max(d.values()) <= 1e-5 and len(data["b_ids"]) > 10
        conf = data["conf_matrix"]
        n = i0.shape[0]
        fx = dict(feat_c0_b0=fc0[0, ::2].numpy(), feat_c1_b0=fc1[0, ::2].numpy(), weights_seed=0, thr=np.float64(thr), n=n,
                  shape0=np.array(i0.shape[2:]), shape1=np.array(i1.shape[2:]),
                  image_digest=np.array([float(i0.double().sum()), float(i1.double().sum())]),
                  backbone_c=bc[:1, :, ::2, ::2].numpy(), backbone_f=bf[:1, ::4, ::8, ::8].numpy(),
                  feat_c0=fc0[:, ::8].numpy(), feat_c1=fc1[:, ::8].numpy(),
                  conf_rowmax=conf.max(2)[0].numpy(), conf_rowarg=conf.max(2)[1].numpy(),
                  conf_colmax=conf.max(1)[0].numpy(), conf_colarg=conf.max(1)[1].numpy(),
                  conf_sum=np.array([float(conf.double().sum())]),
                  b_ids=data["b_ids"].numpy(), i_ids=data["i_ids"].numpy(), j_ids=data["j_ids"].numpy(),
                  mconf=data["mconf"].numpy(), mkpts0_c=data["mkpts0_c"].numpy(), mkpts1_c=data["mkpts1_c"].numpy(),
                  mkpts0_f=data["mkpts0_f"].numpy(), mkpts1_f=data["mkpts1_f"].numpy(), expec_f=data["expec_f"].numpy(),
                  hw0_c=np.array(data["hw0_c"]), hw1_c=np.array(data["hw1_c"]), hw0_f=np.array(data["hw0_f"]),
                  hw1_f=np.array(data["hw1_f"]))
        out.update({f"{name}.{k}": v for k, v in fx.items()})
    np.savez(os.path.join(OUT, "loftr_full_128.npz"), **out)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_root = sys.argv[1]
    sd = synth.synthetic_matcher_state_dict(seed=0)
    gen_modules(ref_root, sd)
    gen_matcher(ref_root, sd)
    for f in ("loftr_full.npz", "loftr_full_128.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
