"""GPU: the MoCoPE fusion pose model on HIP (mocope.hip, pope_amd/mocope.py) against the reference module.

The checker is tests/golden/mocope.npz (scripts/gen_golden_mocope.py): `pose/model0604.py:MoCoPE` itself, run in fp32 and in
fp64 on the weights and inputs `pope_amd.synth` regenerates here from seeds (the small trunk with a 1000-class head, 64 x 64
images).  Bound per tap and case: the HIP result's error against the fp64 evaluation is at most 4 x e32, the reference's own
CPU fp32 error against that same evaluation (the margin covers a different device sinf and different summation orders: fp32
roundings of the same sums).  The backbone runs in the model's default 'f16x3'; the taps downstream of it take the same bound.
The fixture script asserts that dropping the cross-attention, swapping src and tgt of mkpts_as_q, dropping the closing norms,
two heads at d = 76 and splitting a call into single pairs each move the results by >= 100 x that bound.  Measured ratios are
printed (-s) and recorded in profiles/mocope.md."""
import functools
import os

import numpy as np
import pytest
import torch

from pope_amd import convnextv2, synth
from pope_amd.mocope import MoCoPE, regress_pose_fused_batch
from pope_amd.pose_regressor import ROW_CHUNK, Mkpts_Reg_Model, regress_pose_batch

pytestmark = pytest.mark.gpu
MARGIN = 4.0
WIDE_TAPS = ("embedding", "memory", "transformer_mkpts")      # [B, S, 76]: kept at the fixture's sample slots


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mocope.npz"))


@functools.lru_cache(maxsize=1)
def _state_dict(S):
    return synth.mocope_state_dict(S, "6d")


@functools.lru_cache(maxsize=2)
def _model(S, mode="6d", train_type="mkpts+cnn"):
    m = MoCoPE(S, mode, train_type=train_type, backbone=convnextv2.ConvNeXtV2(**synth.MOCOPE_TRUNK))
    sd = dict(_state_dict(S))
    if mode != "6d":       # the modes share every tensor but the rotation head
        rot = synth.mocope_state_dict(5, mode)
        sd.update({k: rot[k] for k in ("rotation_head.weight", "rotation_head.bias")})
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0")


def _err(got, want64):
    return float((got.double().cpu() - torch.from_numpy(np.asarray(want64))).abs().max())


def _check_case(gold, S, B, mode, train_type="mkpts+cnn"):
    model = _model(S, mode, train_type)
    inputs = [t.cuda() for t in synth.mocope_case(S, B)]
    slots = synth.pose_regressor_tap_slots(S)
    tag = f"S{S}_B{B}_{mode}_{train_type}"
    where = lambda k: tag if k in ("t", "R") else f"S{S}_B{B}_{train_type}"  # noqa: E731  (the modes share the taps in front of the heads)
    t, R = model(*inputs)
    assert R.shape == (B, 3, 3) and t.shape == (B, 3)
    got = {"t": t, "R": R}
    for tap in synth.MOCOPE_TAPS_OF[train_type]:
        x = model.taps(*inputs, tap)
        got[tap] = x[:, slots] if tap in WIDE_TAPS else x[..., synth.MOCOPE_TAP_COLUMNS]
    errs = {k: _err(v, gold[f"{where(k)}.{k}64"]) for k, v in got.items()}
    e32 = {k: float(gold[f"{where(k)}.e32_{k}"]) for k in got}
    print(f"{tag}: " + ", ".join(f"{k} {errs[k]:.3g} (e32 {e32[k]:.3g}, x{errs[k] / e32[k]:.2f})" for k in errs))
    for k in errs:
        assert errs[k] <= MARGIN * e32[k], (tag, k, errs[k], e32[k])


CASES = sorted((S, mode, B) for S, B in synth.MOCOPE_CASES
               for mode in (synth.POSE_REGRESSOR_MODES if S == synth.MOCOPE_MODES_AT else ("6d",)))


@pytest.mark.parametrize("S,mode,B", CASES)
def test_matches_reference_module(dev, gold, S, mode, B):
    _check_case(gold, S, B, mode)


@pytest.mark.parametrize("train_type", ["mkpts", "cnn"])
def test_reduced_train_types(dev, gold, train_type):
    _check_case(gold, *synth.MOCOPE_REDUCED, "6d", train_type)


def test_group_semantics(dev, gold):
    S, B = 37, 3
    model = _model(S)
    d0, d1, i0, i1 = (t.cuda() for t in synth.mocope_case(S, B))
    tag = f"S{S}_B{B}_6d_mkpts+cnn"
    bound_t, bound_R = MARGIN * float(gold[f"{tag}.e32_t"]), MARGIN * float(gold[f"{tag}.e32_R"])
    t, R = model(d0, d1, i0, i1)
    assert _err(t, gold[f"{tag}.t64"]) <= bound_t and _err(R, gold[f"{tag}.R64"]) <= bound_R
    singles = [model(d0[b:b + 1], d1[b:b + 1], i0[b:b + 1], i1[b:b + 1]) for b in range(B)]
    ts, Rs = torch.cat([s[0] for s in singles]), torch.cat([s[1] for s in singles])
    assert float((ts - t).abs().max()) > 100 * bound_t and float((Rs - R).abs().max()) > 100 * bound_R   # the pairs of a call are coupled
    perm = [2, 0, 1]
    tp, Rp = model(*(v[perm].contiguous() for v in (d0, d1, i0, i1)))
    assert _err(tp, gold[f"{tag}.t64"][perm]) <= bound_t and _err(Rp, gold[f"{tag}.R64"][perm]) <= bound_R
    # the largest group: 64 pairs in one call run and stay finite; 65 are refused
    k = torch.rand(64, S, 2, device=dev) * 400
    img = torch.randn(64, 3, 64, 64, device=dev)
    t64, R64 = model(k, k + 3, img, img.flip(0))
    assert bool(torch.isfinite(t64).all()) and bool(torch.isfinite(R64).all())
    with pytest.raises(NotImplementedError):
        z = torch.zeros(65, S, 2, device=dev)
        model(z, z, img, img)


def test_matches_reference_module_at_a_wide_mlp1(dev, gold):
    """S = 220: mlp1.0 is [8360, 16720] (559 MB), its flat weight index passes 2^27 and every 16-byte path is taken."""
    _model.cache_clear()
    torch.cuda.empty_cache()
    _check_case(gold, *synth.MOCOPE_WIDE, "6d")
    _model.cache_clear()
    _state_dict.cache_clear()
    torch.cuda.empty_cache()


def test_pipeline_form_is_batch_invariant(dev, hip_lib):
    S = 37
    model = _model(S)
    B = ROW_CHUNK + 1          # one pair past the row chunk of the streamed Linears
    counts = [S, 50, 12, 200, S + 1, 0, 90, 5, 64]
    assert B == len(counts) == 9
    k0, k1 = (t.to(dev) for t in synth.pose_regressor_matches(counts, seed=7))
    g = torch.Generator().manual_seed(5)
    i0, i1 = torch.randn(B, 3, 64, 64, generator=g).to(dev), torch.randn(B, 3, 64, 64, generator=g).to(dev)
    out = regress_pose_fused_batch(model, k0, k1, counts, i0, i1, seed=11)
    assert out["status"].tolist() == [0] * B and bool(torch.isfinite(out["t"]).all())
    offs = np.concatenate([[0], np.cumsum(counts)])
    for b in range(B):
        one = regress_pose_fused_batch(model, k0[offs[b]:offs[b + 1]], k1[offs[b]:offs[b + 1]], [counts[b]], i0[b:b + 1], i1[b:b + 1], seed=11)
        assert torch.equal(one["R"][0], out["R"][b]) and torch.equal(one["t"][0], out["t"][b]) and int(one["status"][0]) == 0, b
    assert len({tuple(v.tolist()) for v in out["t"]}) == B            # and the pairs do differ
    # status codes are those of regress_pose_batch: a negative device count refuses its pair and every pair after it, counts
    # beyond the buffers refuse the pair they run out in, an index outside [0, count) refuses that pair alone
    plain = Mkpts_Reg_Model(S, "6d").to(dev)
    bad_index = torch.zeros(B, S, dtype=torch.int32)
    bad_index[3, 1] = 200
    for cnt, kw in ((torch.tensor([S, 50, -2, 200, S + 1, 0, 90, 5, 64], dtype=torch.int32, device=dev), {}),
                    (torch.tensor([S, 50, 12, 200, S + 1, 0, 90, 5, 65], dtype=torch.int32, device=dev), {}),
                    (counts, {"sample_index": bad_index})):
        want = regress_pose_batch(plain, k0, k1, cnt, seed=11, stage="embedding", **kw)["status"]
        got = regress_pose_fused_batch(model, k0, k1, cnt, i0, i1, seed=11, **kw)
        assert torch.equal(got["status"], want) and int(want.abs().max()) != 0
        refused = want != 0
        assert float(got["t"][refused].abs().max()) == 0 and float(got["R"][refused].abs().max()) == 0
        assert torch.equal(got["t"][0], out["t"][0])          # count == S: neither sampled nor padded
    # a non-default stream
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        again = regress_pose_fused_batch(model, k0, k1, counts, i0, i1, seed=11)
    side.synchronize()
    assert torch.equal(again["R"], out["R"]) and torch.equal(again["t"], out["t"]) and torch.equal(again["status"], out["status"])
    _model.cache_clear()
    _state_dict.cache_clear()
