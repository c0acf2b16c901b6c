"""GPU: the learned pose regressor on HIP (pose_regressor.hip, pope_amd/pose_regressor.py) against the reference module.

The checker is tests/golden/pose_regressor.npz (scripts/gen_golden_pose_regressor.py): `pose/model.py:Mkpts_Reg_Model` itself, run
in fp32 and in fp64 on the weights and inputs `pope_amd.synth` regenerates here from seeds.  Bound per tap and case: the HIP
result's error against the fp64 evaluation is at most 4 x e32, the reference's own CPU fp32 error against that same evaluation
(the margin covers a different device sinf and different summation orders over K = 2048 and K = 76 S: fp32 roundings of the
same sums).  The fixture script asserts that dropping the attention term, swapping sin and cos and splitting a call into
single pairs each move the results by >= 100 x that bound.  Measured errors are printed (-s) and recorded in
profiles/pose_regressor.md."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from pope_amd import _lib, synth
from pope_amd.pose_regressor import (ROW_CHUNK, Mkpts_Reg_Model, device_sample_indices, reference_sample_indices,
                                     regress_pose_batch)

pytestmark = pytest.mark.gpu
MARGIN = 4.0
MODES = list(synth.POSE_REGRESSOR_MODES)


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_regressor.npz"))


@functools.lru_cache(maxsize=4)
def _model(S, mode):
    m = Mkpts_Reg_Model(S, mode)
    m.load_state_dict(synth.pose_regressor_state_dict(S, mode), strict=True)
    return m.to("cuda:0")


def _err(got, want64):
    return float((got.double().cpu() - torch.from_numpy(np.asarray(want64))).abs().max())


def _check_case(gold, S, B, mode):
    model = _model(S, mode)
    d0, d1 = (t.cuda() for t in synth.pose_regressor_case(S, B))
    slots = synth.pose_regressor_tap_slots(S)
    tag = f"S{S}_B{B}"
    t, R = model(d0, d1)
    got = {"emb": model.taps(d0, d1, "embedding")[:, slots], "enc": model.taps(d0, d1, "encoder")[:, slots], "t": t, "R": R}
    want = {"emb": gold[f"{tag}.emb64"], "enc": gold[f"{tag}.enc64"], "t": gold[f"{tag}_{mode}.t64"], "R": gold[f"{tag}_{mode}.R64"]}
    e32 = {"emb": gold[f"{tag}.e32_emb"], "enc": gold[f"{tag}.e32_enc"], "t": gold[f"{tag}_{mode}.e32_t"], "R": gold[f"{tag}_{mode}.e32_R"]}
    errs = {k: _err(got[k], want[k]) for k in got}
    print(f"{tag} {mode}: " + ", ".join(f"{k} {errs[k]:.3g} (e32 {float(e32[k]):.3g}, x{errs[k] / float(e32[k]):.2f})" for k in errs))
    assert R.shape == (B, 3, 3) and t.shape == (B, 3)
    for k in errs:
        assert errs[k] <= MARGIN * float(e32[k]), (tag, mode, k, errs[k], float(e32[k]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,B", synth.POSE_REGRESSOR_CASES)
def test_matches_reference_module(dev, gold, S, B, mode):
    _check_case(gold, S, B, mode)


def test_matches_reference_module_at_real_width(dev, gold):
    """S = 300: mlp.0 is [5700, 22800] (520 MB), its flat weight index passes 2^27 and every 16-byte path is taken."""
    _check_case(gold, *synth.POSE_REGRESSOR_LARGE, "matrix")
    _model.cache_clear()
    torch.cuda.empty_cache()


def test_group_semantics(dev, gold):
    S, B, mode = 37, 3, "matrix"
    model = _model(S, mode)
    d0, d1 = (t.cuda() for t in synth.pose_regressor_case(S, B))
    tag = f"S{S}_B{B}_{mode}"
    bound_t, bound_R = MARGIN * float(gold[f"{tag}.e32_t"]), MARGIN * float(gold[f"{tag}.e32_R"])
    t, R = model(d0, d1)
    assert _err(t, gold[f"{tag}.t64"]) <= bound_t and _err(R, gold[f"{tag}.R64"]) <= bound_R
    singles = [model(d0[b:b + 1], d1[b:b + 1]) for b in range(B)]
    ts, Rs = torch.cat([s[0] for s in singles]), torch.cat([s[1] for s in singles])
    assert float((ts - t).abs().max()) > 100 * bound_t and float((Rs - R).abs().max()) > 100 * bound_R   # the pairs of a call are coupled
    perm = [2, 0, 1]
    tp, Rp = model(d0[perm].contiguous(), d1[perm].contiguous())
    assert _err(tp, gold[f"{tag}.t64"][perm]) <= bound_t and _err(Rp, gold[f"{tag}.R64"][perm]) <= bound_R
    # the largest group: 64 pairs in one call run (two row blocks per workgroup) and stay finite; 65 are refused
    k = torch.rand(64, S, 2, device=dev) * 400
    t64, R64 = model(k, k + 3)
    assert bool(torch.isfinite(t64).all()) and bool(torch.isfinite(R64).all())
    with pytest.raises(NotImplementedError):
        model(torch.zeros(65, S, 2, device=dev), torch.zeros(65, S, 2, device=dev))


def _compact(counts, seed, dev):
    k0, k1 = synth.pose_regressor_matches(counts, seed=seed)
    return k0.to(dev), k1.to(dev)


def _alone(model, k0, k1, counts, b, **kw):
    off = int(sum(counts[:b]))
    return regress_pose_batch(model, k0[off:off + counts[b]], k1[off:off + counts[b]], [counts[b]], **kw)


def test_pipeline_form_is_batch_invariant(dev, hip_lib):
    S = 37
    model = _model(S, "6d")
    B = ROW_CHUNK + 1          # one pair past the mlp.0 row chunk
    assert B == 9
    counts = [S, 50, 12, 200, S + 1, 0, 90, 5, 64][:B]
    k0, k1 = _compact(counts, 7, dev)
    out = regress_pose_batch(model, k0, k1, counts, seed=11)
    assert int(out["status"].abs().max()) == 0
    for b in range(B):
        one = _alone(model, k0, k1, counts, b, seed=11)
        assert torch.equal(one["R"][0], out["R"][b]) and torch.equal(one["t"][0], out["t"][b]), b
    perm = [8, 3, 0, 5, 1, 7, 2, 6, 4]
    offs = np.concatenate([[0], np.cumsum(counts)])
    rows = torch.cat([torch.arange(offs[b], offs[b + 1]) for b in perm]).to(dev)
    outp = regress_pose_batch(model, k0[rows], k1[rows], [counts[b] for b in perm], seed=11)
    assert torch.equal(outp["R"], out["R"][perm]) and torch.equal(outp["t"], out["t"][perm])
    # two chunks and a remainder, against the same pairs alone
    counts2 = (counts * 3)[:19]
    k0b, k1b = _compact(counts2, 8, dev)
    out2 = regress_pose_batch(model, k0b, k1b, counts2, seed=11)
    for b in (0, 7, 8, 15, 16, 18):
        one = _alone(model, k0b, k1b, counts2, b, seed=11)
        assert torch.equal(one["R"][0], out2["R"][b]) and torch.equal(one["t"][0], out2["t"][b]), b


@pytest.mark.parametrize("S", [5, 37, 70])
def test_sampling(dev, S):
    model = _model(S, "quat")
    counts = [0, 3, S - 1, S, S + 1, 4 * S]
    B = len(counts)
    k0, k1 = _compact(counts, 20 + S, dev)
    offs = np.concatenate([[0], np.cumsum(counts)])
    seed = 5

    def gathered(index):
        """forward on the host-gathered and padded points, one pair per call"""
        ts, Rs = [], []
        for b in range(B):
            d0, d1 = torch.zeros(1, S, 2, device=dev), torch.zeros(1, S, 2, device=dev)
            keep = index[b] >= 0
            rows = torch.from_numpy(offs[b] + index[b][keep]).to(dev)
            d0[0, torch.from_numpy(keep).to(dev)] = k0[rows]
            d1[0, torch.from_numpy(keep).to(dev)] = k1[rows]
            t, R = model(d0, d1)
            ts.append(t), Rs.append(R)
        return torch.cat(ts), torch.cat(Rs)

    want_index = np.stack([device_sample_indices(c, S, seed) for c in counts])
    emb = regress_pose_batch(model, k0, k1, counts, seed=seed, stage="embedding")
    assert np.array_equal(emb["index"].cpu().numpy(), want_index)
    assert np.array_equal(want_index[3], np.arange(S))                     # count == S is not sampled
    out = regress_pose_batch(model, k0, k1, counts, seed=seed)
    assert int(out["status"].abs().max()) == 0
    t, R = gathered(want_index)
    assert torch.equal(out["t"], t) and torch.equal(out["R"], R)
    other = regress_pose_batch(model, k0, k1, counts, seed=seed + 1)
    assert torch.equal(other["t"][:4], out["t"][:4]) and not torch.equal(other["t"][4:], out["t"][4:])
    # the host-supplied index, here the reference's own sample sequence
    ref_index = reference_sample_indices(counts, S)[:, 0]
    out_ref = regress_pose_batch(model, k0, k1, counts, sample_index=torch.from_numpy(ref_index))
    t, R = gathered(ref_index)
    assert torch.equal(out_ref["t"], t) and torch.equal(out_ref["R"], R) and int(out_ref["status"].abs().max()) == 0
    # an index outside [0, count) refuses that pair alone
    bad = ref_index.copy()
    bad[5, S // 2] = counts[5]
    bad[2, 0] = 10 ** 6            # count <= S: the index is not consulted
    out_bad = regress_pose_batch(model, k0, k1, counts, sample_index=torch.from_numpy(bad))
    assert out_bad["status"].tolist() == [0, 0, 0, 0, 0, -2]
    assert torch.equal(out_bad["t"][:5], out_ref["t"][:5]) and torch.equal(out_bad["R"][:5], out_ref["R"][:5])
    assert float(out_bad["t"][5].abs().max()) == 0 and float(out_bad["R"][5].abs().max()) == 0
    bad[5, S // 2] = -1
    assert regress_pose_batch(model, k0, k1, counts, sample_index=torch.from_numpy(bad))["status"].tolist() == [0, 0, 0, 0, 0, -2]


def test_device_counts_that_cannot_be_served(dev):
    S = 5
    model = _model(S, "matrix")
    counts = [4, 9, -2, 6]
    k0, k1 = _compact([4, 9, 0, 6], 3, dev)
    good = regress_pose_batch(model, k0, k1, [4, 9], seed=0)
    out = regress_pose_batch(model, k0, k1, torch.tensor(counts, dtype=torch.int32, device=dev), seed=0)
    assert out["status"].tolist() == [0, 0, -1, -1]          # a negative count refuses its pair and every pair after it
    assert torch.equal(out["t"][:2], good["t"]) and torch.equal(out["R"][:2], good["R"])
    assert float(out["t"][2:].abs().max()) == 0 and float(out["R"][2:].abs().max()) == 0
    out = regress_pose_batch(model, k0[:15], k1[:15], torch.tensor([4, 9, 6], dtype=torch.int32, device=dev), seed=0)
    assert out["status"].tolist() == [0, 0, -1]              # counts beyond the M rows of the buffers


def test_arguments(dev, hip_lib):
    S = 5
    model = _model(S, "matrix")
    z = torch.zeros(2, S, 2, device=dev)
    with pytest.raises(_lib.PopeHipError):
        model(z.cpu(), z.cpu())
    with pytest.raises(TypeError):
        model(z.double(), z.double())
    with pytest.raises(ValueError):
        model(torch.zeros(2, S + 1, 2, device=dev), torch.zeros(2, S + 1, 2, device=dev))
    with pytest.raises(NotImplementedError):
        model(torch.zeros(65, S, 2, device=dev), torch.zeros(65, S, 2, device=dev))
    k = torch.zeros(8, 2, device=dev)
    with pytest.raises(_lib.PopeHipError):
        regress_pose_batch(model, k.cpu(), k.cpu(), [8])
    with pytest.raises(TypeError):
        regress_pose_batch(model, k.half(), k.half(), [8])
    with pytest.raises(ValueError):
        regress_pose_batch(model, k, k, [8, -1])
    with pytest.raises(ValueError):
        regress_pose_batch(model, k, k, [8], sample_index=torch.zeros(1, S + 1, dtype=torch.int32))
    # the C entry called directly: an S the weights were not built for, an undersized / misaligned workspace, a group that does
    # not divide B — refused before any launch (the outputs keep their fill)
    w = model._weights()
    t = torch.full((2, 3), 7.0, device=dev)
    R = torch.full((2, 9), 7.0, device=dev)
    st = torch.full((2,), 7, dtype=torch.int32, device=dev)
    need = hip_lib.pope_pose_regressor_workspace_bytes(2, S)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    stream = _lib.stream_of(dev)

    def call(S_arg=S, G=2, ws_ptr=None, nbytes=need):
        return hip_lib.pope_pose_regressor_forward_f32(C.byref(w), p(z), p(z), None, None, None, None, None, 2, S_arg, G, 0, p(t), p(R), p(st),
                                                       ws_ptr or p(ws), nbytes, stream)
    assert call(S_arg=S + 1, nbytes=1 << 30) == -1
    assert call(nbytes=need - 1) == -3
    assert call(ws_ptr=C.c_void_p(ws.data_ptr() + 16)) == -1
    assert call(G=0) == -1 and call(G=65) == -1
    assert hip_lib.pope_pose_regressor_forward_f32(C.byref(w), p(z), p(z), None, None, None, None, None, 3, S, 2, 0, p(t), p(R), p(st), p(ws),
                                                   1 << 30, stream) == -1
    torch.cuda.synchronize()
    assert float(t.min()) == 7.0 and float(R.min()) == 7.0 and int(st.min()) == 7
    assert call() == 0
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0] and float(t.abs().max()) != 7.0


def test_in_place_weight_edit_is_seen(dev):
    S = 5
    model = _model(S, "matrix")
    d0, d1 = (t.cuda() for t in synth.pose_regressor_case(S, 1))
    t0, _ = model(d0, d1)
    with torch.no_grad():
        model.mlp[0].weight.mul_(1.5)
    t1, _ = model(d0, d1)
    with torch.no_grad():
        model.mlp[0].weight.div_(1.5)
    assert not torch.equal(t0, t1)
    _model.cache_clear()


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def test_driver_regresses_the_best_slot(dev, sd0, golden_dir):
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd.driver import locate_match_pose_batch_u8
    from pope_amd.matcher import Matcher, default_cfg
    fx = np.load(os.path.join(golden_dir, "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    matcher = Matcher(default_cfg).eval()
    matcher.load_state_dict(sd, strict=True)
    vit, matcher = load_dinov2_model(state_dict=sd0).to(dev), matcher.to(dev)
    S = 70
    model = _model(S, "6d")
    cases = [synth.synthetic_frame_case(seed=31), synth.synthetic_frame_case(n_proposals=6, seed=32), synth.synthetic_frame_case(seed=31)]
    boxes = [cases[0][2], cases[1][2], np.zeros((0, 4), np.int64)]       # the third query has no proposal: no slot, no matches
    args = (vit, matcher, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), boxes, np.stack([c[3] for c in cases]),
            cases[0][4])
    plain = locate_match_pose_batch_u8(*args)
    outs = locate_match_pose_batch_u8(*args, pose_regressor=model, regressor_seed=9)
    assert len(outs) == 3
    for q, (got, want) in enumerate(zip(outs, plain)):
        assert "pose_regressed" not in want and set(got) == set(want) | {"pose_regressed"}
        for k in want:
            assert _same(got[k], want[k]), (q, k)
    counts = [len(o["mkpts0"][o["best_slot"]]) for o in outs]
    assert counts[0] > S and counts[2] == 0        # the first query is sampled by the device sampler
    k0 = torch.from_numpy(np.concatenate([o["mkpts0"][o["best_slot"]] for o in outs])).to(dev)
    k1 = torch.from_numpy(np.concatenate([o["mkpts1"][o["best_slot"]] for o in outs])).to(dev)
    want = regress_pose_batch(model, k0, k1, counts, seed=9)
    for q, out in enumerate(outs):
        if counts[q] < 5:
            assert out["pose_regressed"] is None, q
            continue
        R, t = out["pose_regressed"]
        assert R.shape == (3, 3) and t.shape == (3,) and R.dtype == np.float32
        assert np.array_equal(R, want["R"][q].cpu().numpy()) and np.array_equal(t, want["t"][q].cpu().numpy()), q
    assert outs[2]["pose_regressed"] is None and outs[0]["pose_regressed"] is not None
    other = locate_match_pose_batch_u8(*args, pose_regressor=model, regressor_seed=10)
    assert not np.array_equal(other[0]["pose_regressed"][1], outs[0]["pose_regressed"][1])
    _model.cache_clear()
