"""GPU: the SwiGLU FFN (ViT-g/14) — the fused w12 GEMM alone against fp64 on every route, and the whole model against the
reference's own outputs (tests/golden/vits_swiglu_224.npz, vitg_224.npz; scripts/gen_golden_vit_swiglu.py).

Per-op bound: DESIGN §2's per-op 2e-5, scaled by max(1, max |ref|) as tests/test_gpu_sam_decoder.py:bound scales, and tightened
as that file did to about 6x the largest measured figure: 1.5e-5 * max(1, max |ref|).  Measured on the MI355X (256 CUs),
err / max(1, max |ref|): f16x3 planes 5.5e-7 (K 384) and 1.24e-6 (K 1536) on both routes, fp32 MFMA 1.05e-6 and 2.38e-6, the
saturating gates 1.9e-7.
Whole-model bounds: the constants tests/test_gpu_vit.py holds ViT-B/L to (ATOL on x_norm / cls, 5 ATOL on x_prenorm / taps)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ATOL = 2e-4
OP_BOUND = 1.5e-5
EPI_SWIGLU, RANGE_GELU = 11, 8          # pope_hip.h POPE_EPI_BIAS_SWIGLU, POPE_RANGE_GELU
ACT, WSC = 8.0, 256.0                   # _lib.PLANES_ACT_SCALE, _lib.PLANES_W_SCALE
EVAL_CFG = dict(patch_size=14, img_size=518, init_values=1e-5, ffn_layer="swiglufused", block_chunks=0)


def _cdiv(a, b):
    return -(-a // b)


def wide_switch(N, cu):
    """gemm_plain.hip pope_wide_x3_supported: the wide route takes ceil(M / 256) * ceil(N / 256) >= 4 * CUs tiles, N = the GEMM's
    2 * hidden columns.  Returns (largest M on the tile kernel, smallest M on the wide route)."""
    row_tiles = _cdiv(4 * cu, _cdiv(N, 256))
    return (row_tiles - 1) * 256, (row_tiles - 1) * 256 + 1


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cu(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _kernels_of(fn):
    """Device kernel names launched by fn (empty when torch.profiler does not see the library's kernels)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ret = fn()
            torch.cuda.synchronize()
        return ret, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    except Exception:
        return fn(), []


class SwigluOp:
    """One w12 problem: O(1) seeded operands, the permuted weight / bias as the kernels read them, fp64 reference."""

    def __init__(self, M, K, N, dev, seed=0, bias=None, value_rows_zero=False):
        from pope_amd import _lib, dinov2
        g = torch.Generator().manual_seed(seed)
        self.M, self.K, self.N, self.h = M, K, N, N // 2
        self.a = torch.randn(M, K, generator=g).to(dev)
        w = torch.randn(N, K, generator=g) / K ** 0.5
        if value_rows_zero:
            w[self.h:] = 0
        self.w = w.to(dev)
        self.b = (torch.randn(N, generator=g) * 0.1 if bias is None else bias).to(dev)
        perm = dinov2.swiglu_permutation(self.h).to(dev)
        self.wq, self.bq = self.w[perm].contiguous(), self.b[perm].contiguous()
        self.ap, self.wp = _lib.to_planes(self.a, ACT), _lib.to_planes(self.wq, WSC)

    def ref(self, rows=None):
        a = self.a if rows is None else self.a[rows]
        x1, x2 = F.linear(a.double(), self.w.double(), self.b.double()).chunk(2, dim=-1)
        return x1 / (1 + torch.exp(-x1)) * x2

    def planes(self, lib, M=None, fp32_out=False):
        """pope_linear_planes_f32 on the first M rows -> (hidden [M, h] fp32, range word, kernel names)."""
        from pope_amd import _lib
        M = M or self.M
        flag = torch.zeros(1, dtype=torch.int32, device=self.a.device)
        out = torch.full((M, self.h), float("nan"), device=self.a.device) if fp32_out else \
            torch.zeros(M, self.h // 32, 2, 32, dtype=torch.float16, device=self.a.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc, names = _kernels_of(lambda: lib.pope_linear_planes_f32(
            _ptr(self.ap), _ptr(self.wp), _ptr(self.bq), _ptr(out) if fp32_out else None, None if fp32_out else _ptr(out), M, self.N,
            self.K, EPI_SWIGLU, None, None, _ptr(flag), st))
        assert rc == 0, rc
        return (out if fp32_out else _lib.from_planes(out, ACT)), int(flag.item()), names, out

    def f32(self, lib, M=None):
        M = M or self.M
        out = torch.full((M, self.h), float("nan"), device=self.a.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.pope_linear_f32(_ptr(self.a), _ptr(self.wq), _ptr(self.bq), _ptr(out), M, self.N, self.K, EPI_SWIGLU, None, None,
                                 0, None, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return out


def _check(got, want, what):
    scale = max(1.0, float(want.abs().max()))
    err = float((got.double() - want).abs().max())
    print(f"{what}: max |err| = {err:.3e} (max |ref| {scale:.3g}, bound {OP_BOUND * scale:.3e})")
    assert bool(torch.isfinite(got).all()), what
    assert err <= OP_BOUND * scale, (what, err, OP_BOUND * scale)


@pytest.mark.parametrize("K,N", [(384, 2048), (1536, 8192)])
def test_swiglu_gemm_alone_against_fp64_on_every_route(hip_lib, dev, cu, K, N):
    """Both sides of the wide route's switch and a ragged M, f16x3 planes and fp32 MFMA, against fp64; the rows both planes
    routes compute are bit-equal."""
    m_tile, m_wide = wide_switch(N, cu)
    op = SwigluOp(m_wide, K, N, dev, seed=K)
    want = op.ref()
    wide, flag_w, names_w, raw_w = op.planes(hip_lib)
    tile, flag_t, names_t, raw_t = op.planes(hip_lib, M=m_tile)
    if names_w and names_t:   # the profiler saw the kernels: each call ran on the route the rule names
        assert all("gemm_plain256_kernel" in n for n in names_w), names_w
        assert all("gemm_planes16_kernel" in n for n in names_t), names_t
    _check(wide, want, f"K {K} N {N} M {m_wide} wide route")
    _check(tile, want[:m_tile], f"K {K} N {N} M {m_tile} tile route")
    assert flag_w == 0 and flag_t == 0
    assert torch.equal(raw_w[:m_tile], raw_t), "the wide route and the tile kernel differ in bits"
    ragged = 1099   # no multiple of 128 or 256: partial last row tile
    rg, flag_r, _, raw_r = op.planes(hip_lib, M=ragged)
    _check(rg, want[:ragged], f"K {K} N {N} M {ragged} ragged, planes out")
    assert flag_r == 0 and torch.equal(raw_r, raw_t[:ragged])
    rf, flag_f, _, _ = op.planes(hip_lib, M=ragged, fp32_out=True)   # fp32 rows from the same accumulators
    _check(rf, want[:ragged], f"K {K} N {N} M {ragged} ragged, fp32 out")
    assert flag_f == 0
    # hi + lo of the planes output is the fp32 value to 2^-22 relative
    assert float((rf - rg).abs().max()) <= 2.0 ** -20 * max(1.0, float(rf.abs().max()))
    _check(op.f32(hip_lib, M=ragged), want[:ragged], f"K {K} N {N} M {ragged} fp32 MFMA")
    _check(op.f32(hip_lib), want, f"K {K} N {N} M {m_wide} fp32 MFMA")


def test_swiglu_saturating_gates_stay_finite(hip_lib, dev):
    """Gate biases of +-60 and +-5 000 (exp(-x) under- and overflows), |value| <= 1 so that |hidden| stays inside the 8 188
    contract: finite, within the scaled bound, no range flag."""
    K, N, M = 384, 2048, 300
    h = N // 2
    g = torch.Generator().manual_seed(5)
    bias = torch.cat([torch.tensor([60.0, -60.0, 5000.0, -5000.0]).repeat(h // 4), torch.rand(h, generator=g) * 2 - 1])
    op = SwigluOp(M, K, N, dev, seed=9, bias=bias, value_rows_zero=True)
    want = op.ref()
    assert 4000 < float(want.abs().max()) < 8188
    got, flag, _, _ = op.planes(hip_lib)
    _check(got, want, "saturating gates, planes")
    assert flag == 0
    _check(op.f32(hip_lib), want, "saturating gates, fp32 MFMA")
    neg = want[:, 3::4].abs().max()   # gate ~ -5 000: silu = x / inf -> 0, not NaN
    assert float(neg) == 0.0 and float(got[:, 3::4].abs().max()) == 0.0


def test_swiglu_range_flag_on_hidden(hip_lib, dev):
    """|hidden| * 8 >= 65 520 raises the FC1 producer's bit."""
    K, N, M = 384, 2048, 200
    bias = torch.zeros(N)
    bias[:4] = 5000.0        # gates of hidden columns 0-3
    bias[N // 2:N // 2 + 4] = 2.0   # their values: hidden = 10 000
    op = SwigluOp(M, K, N, dev, seed=2, bias=bias)
    _, flag, _, _ = op.planes(hip_lib)
    assert flag == RANGE_GELU


# ---- whole model -----------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name, golden_dir):
    """(model on the GPU, fixture, input) of a case; built once per session (the giant draws 1.1 G parameters)."""
    if name not in _MODELS:
        from pope_amd import dinov2, synth
        fx = np.load(os.path.join(golden_dir, name + ".npz"))
        dim, depth, heads = (int(v) for v in fx["arch"])
        if name == "vitg_224":
            m = dinov2.build_vitg14()
        else:
            m = dinov2.DinoVisionTransformer(embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4, **EVAL_CFG)
        assert (m.embed_dim, m.n_blocks, m.num_heads) == (dim, depth, heads)
        sd = synth.synthetic_state_dict(seed=int(fx["weights_seed"]), dim=dim, depth=depth, ffn="swiglu")
        m.load_state_dict(sd, strict=True)
        del sd
        B, H, W = (int(v) for v in fx["shape"])
        x = synth.synthetic_images(B, H, W, seed=int(fx["input_seed"]))
        assert float(x.double().sum()) == fx["input_digest"][0]
        _MODELS[name] = (m.eval().to("cuda:0"), fx, x.cuda())
    return _MODELS[name]


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("name", ["vits_swiglu_224", "vitg_224"])
def test_swiglu_model_matches_reference_fixture(hip_lib, golden_dir, name, prec):
    from pope_amd import synth
    m, fx, x = _model(name, golden_dir)
    m.precision = prec
    events0 = m.overflow_events
    out = m(x, is_training=True)
    rows = torch.from_numpy(fx["rows"])
    floor = float(fx["ref_fp32_err"])
    got = {"x_norm": torch.cat([out["x_norm_clstoken"][:, None], out["x_norm_patchtokens"]], 1).cpu()[:, rows].numpy(),
           "x_prenorm": out["x_prenorm"].cpu()[:, rows].numpy(), "cls": m(x).cpu().numpy()}
    taps = [int(t) for t in fx["tap_blocks"]]
    inter = m.get_intermediate_layers(x, n=taps, norm=False, return_class_token=True)
    for (patch, cls), i in zip(inter, taps):
        got[f"blk{i}"] = torch.cat([cls[:, None], patch], 1).cpu()[:, rows].numpy()
    errs = {k: float(np.abs(v - fx[k]).max()) for k, v in got.items()}
    print(f"{name} [{prec}]: max |gpu - reference| " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f"; the reference's own fp32 error {floor:.2e}")
    for k, e in errs.items():
        assert np.isfinite(got[k]).all() and e <= (ATOL if k in ("x_norm", "cls") else 5 * ATOL), (k, e)
    assert m.overflow_events == events0
    again = m(x, is_training=True)   # deterministic, bit for bit
    assert all(torch.equal(again[k], out[k]) for k in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"))
    x3 = torch.cat([synth.synthetic_images(2, x.shape[2], x.shape[3], seed=3).cuda(), x])   # batch-invariant, bit for bit
    b3 = m(x3, is_training=True)
    assert all(torch.equal(b3[k][2], out[k][0]) for k in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"))


def _small(depth=4, seed=0):
    from pope_amd import dinov2, synth
    m = dinov2.DinoVisionTransformer(embed_dim=384, depth=depth, num_heads=6, mlp_ratio=4, **EVAL_CFG)
    m.load_state_dict(synth.synthetic_state_dict(seed=seed, dim=384, depth=depth, ffn="swiglu"), strict=True)
    return m.eval().to("cuda:0")


def test_batch_size_routes_give_the_same_bits(hip_lib, dev, cu):
    """w12 takes the wide route at batch size and the tile kernel for one image: image 0 is bit-equal between the two."""
    from pope_amd import synth
    m = _small()
    _, m_wide = wide_switch(2048, cu)
    B = _cdiv(m_wide, 257)
    assert _cdiv(B * 257, 256) * 8 >= 4 * cu > _cdiv(257, 256) * 8
    x = synth.synthetic_images(B, 224, 224, seed=21).cuda()
    big = m(x, is_training=True)
    one = m(x[:1], is_training=True)
    for k in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"):
        assert torch.equal(big[k][0], one[k][0]), k
    assert m.overflow_events == 0 and bool(torch.isfinite(big["x_prenorm"]).all())


def test_range_guard_of_the_swiglu_hidden(hip_lib, dev):
    from pope_amd import synth
    from pope_amd._lib import PopeRangeError
    x = synth.synthetic_images(2, 56, 84, seed=1).cuda()
    m = _small(depth=2)
    with torch.no_grad():
        m.blocks[1].mlp.w12.bias[1024 + 17] = 1e6      # a value-half bias: |hidden| * 8 >= 65 520
    m.on_overflow = "raise"
    with pytest.raises(PopeRangeError):
        m(x, is_training=True)
    assert m.overflow_events == 1
    m = _small(depth=2)   # the default policy: warn once, re-run every such call on the fp32 MFMA
    with torch.no_grad():
        m.blocks[1].mlp.w12.bias[1024 + 17] = 1e6
    assert m.on_overflow == "rerun_f32"
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y = m(x, is_training=True)
        m(x, is_training=True)
    assert len([w for w in rec if "f16x3 range contract" in str(w.message)]) == 1 and m.overflow_events == 2
    ref = _small(depth=2)
    with torch.no_grad():
        ref.blocks[1].mlp.w12.bias[1024 + 17] = 1e6
    ref.precision = "f32"
    want = ref(x, is_training=True)
    for k in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"):
        assert torch.equal(y[k], want[k]), k
    assert ref.overflow_events == 0
    for lin in ("w12", "w3"):   # |w| >= 256 is caught when the planes are built
        bad = _small(depth=2)
        bad.on_overflow = "raise"
        with torch.no_grad():
            getattr(bad.blocks[0].mlp, lin).weight[3, 5] = 300.0
        with pytest.raises(PopeRangeError, match="weight"):
            bad(x, is_training=True)


def test_w12_edits_refresh_the_derived_tensors(hip_lib, dev):
    from pope_amd import synth
    m = _small(depth=2)
    x = synth.synthetic_images(2, 56, 84, seed=1).cuda()
    y0 = m(x, is_training=True)["x_norm_patchtokens"].clone()
    w0 = m._weights()
    assert m._weights() is w0 and torch.equal(m(x, is_training=True)["x_norm_patchtokens"], y0)   # unchanged: cache hit
    with torch.no_grad():
        m.blocks[1].mlp.w12.weight[5, 7] += 0.5
    y1 = m(x, is_training=True)["x_norm_patchtokens"].clone()
    assert m._weights() is not w0 and not torch.equal(y0, y1)
    m.blocks[0].mlp.w12.weight = torch.nn.Parameter(m.blocks[0].mlp.w12.weight.detach() * 0.5, requires_grad=False)
    y2 = m(x, is_training=True)["x_norm_patchtokens"]
    assert not torch.equal(y1, y2)
    fresh = _small(depth=2)
    with torch.no_grad():
        fresh.blocks[1].mlp.w12.weight[5, 7] += 0.5
        fresh.blocks[0].mlp.w12.weight.mul_(0.5)
    assert torch.equal(y2, fresh(x, is_training=True)["x_norm_patchtokens"])


def test_mlp_archs_did_not_move(golden_dir, golden_threads):
    from pope_amd import synth
    fx = np.load(os.path.join(golden_dir, "vitl_224.npz"))
    dim, depth, _ = (int(v) for v in fx["arch"])
    sd = synth.synthetic_state_dict(seed=int(fx["weights_seed"]), dim=dim, depth=depth)
    assert np.array_equal(np.array([float(sd[k].double().sum()) for k in sorted(sd)]), fx["weights_digest"])
