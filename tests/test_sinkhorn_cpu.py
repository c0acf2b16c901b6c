"""CPU: the torch statement of the Sinkhorn coarse matcher (pope_amd/sinkhorn_cpu.py) against the fixture the reference module
wrote with it (scripts/gen_golden_sinkhorn.py), its marginals in fp64, and the host side of the option: the module owns
`bin_score`, the state-dict keys, the argument checks that need no GPU."""
import os

import numpy as np
import pytest
import torch

UNMASKED = ["12x16_vs_10x14", "32x32", "16x16_vs_12x16", "unrelated"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "sinkhorn.npz"))


@pytest.mark.parametrize("name", UNMASKED + ["masked_16x16"])
def test_cpu_definition_against_the_reference_fixture(fx, name, golden_threads):
    from oracle import coarse_match_ref as cm
    from pope_amd import sinkhorn_cpu, synth
    case = synth.sinkhorn_case(name)
    kw = {"mask0": case["mask0"], "mask1": case["mask1"]} if "mask0" in case else {}
    conf = sinkhorn_cpu.conf_matrix(case["feat0"], case["feat1"], torch.tensor(1.0), 3, True, **kw)
    st = int(fx[f"{name}.conf_stride"])
    np.testing.assert_allclose(conf[:, ::st, ::st].numpy(), fx[f"{name}.conf_matrix"], rtol=1e-4, atol=1e-7)
    if name in UNMASKED:   # (the CPU restatement of get_coarse_match has no padded border)
        out = cm.coarse_match(conf, case["hw0"], case["hw1"], case["hw0_i"], 0.2, 2)
        for k in ("b_ids", "i_ids", "j_ids"):
            assert np.array_equal(out[k].numpy(), fx[f"{name}.{k}"]), k
        assert np.array_equal(out["mkpts1_c"].numpy(), fx[f"{name}.mkpts1_c"])


def test_marginals_in_fp64():
    """After the last column step every column of the assignment (dustbin row included) sums to exp(log_nu - norm) to fp64
    rounding; the rows, one half-step behind, only have to be finite."""
    from pope_amd import sinkhorn_cpu, synth
    case = synth.sinkhorn_case("12x16_vs_10x14")
    sim = torch.einsum("nlc,nsc->nls", case["feat0"].double() / 16, case["feat1"].double() / 16)
    z, u, v, norm, log_mu, log_nu = sinkhorn_cpu.potentials(sim, 1.0, 3)
    a = (z + u.unsqueeze(2) + v.unsqueeze(1) - norm).exp()
    assert torch.equal(a, sinkhorn_cpu.log_optimal_transport(sim, 1.0, 3).exp())
    np.testing.assert_allclose(a.sum(1).numpy(), (log_nu - norm).exp().numpy(), rtol=1e-12, atol=0)
    assert bool(a.sum(2).isfinite().all()) and float(a.sum(2).min()) > 0
    L, S = sim.shape[1:]
    assert abs(float((log_nu - norm).exp()[0, :S].sum()) - S) < 1e-9 and abs(float((log_nu - norm).exp()[0, S]) - L) < 1e-9


def test_module_owns_bin_score_and_state_dict_keys():
    from pope_amd import synth
    from pope_amd.matcher import CoarseMatching, Matcher, default_cfg
    mc = dict(default_cfg["match_coarse"], match_type="sinkhorn", skh_init_bin_score=1.25, sparse_spvs=True)
    m = CoarseMatching(mc)
    assert isinstance(m.bin_score, torch.nn.Parameter) and m.bin_score.dtype == torch.float32 and m.bin_score.dim() == 0
    assert float(m.bin_score.detach()) == 1.25 and list(m.state_dict()) == ["bin_score"]
    assert (m.skh_iters, m.skh_prefilter) == (3, True)
    today = set(synth.synthetic_matcher_state_dict(seed=0))
    ot = Matcher(dict(default_cfg, match_coarse=mc))
    assert set(ot.state_dict()) == today | {"coarse_matching.bin_score"}
    ds = Matcher(default_cfg)
    assert set(ds.state_dict()) == today and list(CoarseMatching(default_cfg["match_coarse"]).state_dict()) == []
    # a checkpoint of the `*_ot` kind loads strictly, `matcher.` prefix included; a dual-softmax Matcher rejects the key
    sd = synth.synthetic_matcher_state_dict(seed=0)
    sd["coarse_matching.bin_score"] = torch.tensor(2.0)
    ot.load_state_dict({"matcher." + k: v for k, v in sd.items()}, strict=True)
    assert float(ot.coarse_matching.bin_score.detach()) == 2.0
    with pytest.raises(RuntimeError, match="bin_score"):
        ds.load_state_dict(dict(sd), strict=True)
    with pytest.raises(NotImplementedError):
        CoarseMatching(dict(default_cfg["match_coarse"], match_type="other"))


def test_host_side_argument_checks(hip_lib):
    """Raised before anything touches a device."""
    from pope_amd.matcher import dense_match
    f = torch.zeros(1, 16, 64)
    args = (f, f, (4, 4), (4, 4), (32, 32))
    with pytest.raises(TypeError):
        dense_match(*args, match_type="sinkhorn")                                  # no bin_score
    with pytest.raises(TypeError):
        dense_match(*args, match_type="sinkhorn", bin_score=1.0)                   # a Python float has no device storage
    with pytest.raises(TypeError):
        dense_match(*args, match_type="sinkhorn", bin_score=torch.tensor(1.0, dtype=torch.float64))
    with pytest.raises(ValueError):
        dense_match(*args, match_type="sinkhorn", bin_score=torch.ones(2))
    with pytest.raises(ValueError):
        dense_match(*args, match_type="sinkhorn", bin_score=torch.tensor(1.0), skh_iters=0)
    with pytest.raises(ValueError):
        dense_match(*args, match_type="other")
    # the C entry: a null dustbin pointer and skh_iters < 1 are argument errors; the workspace holds u, v and the column maxima
    import ctypes
    from pope_amd import _lib
    buf = ctypes.create_string_buffer(64)
    ok = (ctypes.addressof(buf) + 15) & ~15   # never dereferenced

    def args(bin_score, iters, n=1, L=4, S=4, match_type=_lib.MATCH_TYPES["sinkhorn"]):
        return _lib.DenseMatchArgs(
            feat0=ok, stride0=1024, feat1=ok, stride1=1024, n=n, L=L, S=S, C=256, h0=2, w0=2, h1=2, w1=2, thr=0.2, border_rm=2,
            match_type=match_type, bin_score=bin_score, skh_iters=iters, skh_prefilter=1, scale=8.0, b_ids=ok, i_ids=ok, j_ids=ok,
            mconf=ok, mkpts0_c=ok, mkpts1_c=ok, counts=ok, conf_matrix=ok, workspace=ok, workspace_bytes=1 << 20, precision=1)

    def call(bin_score, iters):
        return hip_lib.pope_dense_match_f32(ctypes.byref(args(bin_score, iters)), None)
    assert call(None, 3) == -1 and call(ok, 0) == -1
    query = lambda a: hip_lib.pope_dense_match_workspace_bytes(ctypes.byref(a))   # noqa: E731
    extra = query(args(ok, 3, 2, 192, 140)) - query(args(ok, 3, 2, 192, 140, match_type=_lib.MATCH_TYPES["dual_softmax"]))
    assert extra >= 4 * 2 * (193 + 141 + 140)
    assert query(args(ok, 3, n=0)) == 0
