"""GPU: the Vision Mamba backbone (pope_amd/vim.py, vim.hip) against the reference module's fp64 evaluation (tests/golden/vim.npz,
scripts/gen_golden_vim.py), its three arithmetic kernels alone against fp64 restatements on the CPU, batch independence,
determinism, the range guard and the C entries' argument checks.

Bound of every comparison: MARGIN x the fp32 reference's own error against fp64 on the same input (e32 of the fixture for the
taps, the fp32 sequential restatement's error for the op-level checks) — never a figure taken from the code under test."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pope_amd import _lib, synth, vim

pytestmark = pytest.mark.gpu
MARGIN = 4.0
PRECISIONS = ("f16x3", "f32")
N = 16


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "vim.npz"))


def build(name, precision):
    case = synth.vim_case(name)
    cfg = case["cfg"]
    model = vim.VisionMamba(**{**vim._FACTORY_SETTINGS, **cfg}, precision=precision)
    model.load_state_dict(case["state_dict"], strict=True)
    return model.cuda(), case["x"].cuda()


_cache = {}


def run_case(name, precision):
    """(model, x, features, logits, taps) of one fixture case, computed once per precision."""
    key = (name, precision)
    if key not in _cache:
        model, x = build(name, precision)
        f, o, t = model.forward_with_taps(x)
        torch.cuda.synchronize()
        assert model.overflow_events == 0
        _cache[key] = (model, x, f, o, t)
    return _cache[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(synth.VIM_CASES))
def test_taps_against_fp64(gold, name, precision):
    _, _, f, o, t = run_case(name, precision)
    got = dict(zip(synth.VIM_TAPS, t + [f, o]))
    worst = {}
    for tap in synth.VIM_TAPS:
        want = torch.from_numpy(gold[f"{name}.{tap}64"])
        idx = synth.vim_tap_index(name, tap, got[tap].numel())
        g = got[tap].reshape(-1).cpu()[idx].double()
        assert torch.isfinite(g).all()
        e32 = float(gold[f"{name}.e32_{tap}"])
        worst[tap] = float((g - want).abs().max()) / e32
        print(f"{name} {precision} {tap}: max |gpu - fp64| = {worst[tap]:.2f} x e32 ({e32:.3g})")
    assert all(r <= MARGIN for r in worst.values()), worst


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_entries_agree(precision):
    model, x, f, o, _ = run_case("small_s8_64", precision)
    assert torch.equal(model(x), o) and torch.equal(model.forward_features(x), f) and torch.equal(model(x, return_features=True), f)


# ---- the scan ---------------------------------------------------------------------------------------------------------------
def _dirs(tensors, keep):
    """HOST array of 2 pope_vim_dir_weights from dicts of CPU tensors."""
    arr = (_lib.VimDirWeights * 2)()
    for v, d in zip(arr, tensors):
        for k, t in d.items():
            t = t.contiguous().cuda()
            keep.append(t)
            setattr(v, k, t.data_ptr())
    return arr


def _scan_inputs(B, L, E, R, seed, zero_x=False):
    g = torch.Generator().manual_seed(seed)
    M = B * L
    xc = torch.zeros(2, M, E) if zero_x else 0.6 * torch.randn(2, M, E, generator=g)
    xz = torch.randn(M, 2 * E, generator=g)                # z is read in place from the in_proj output: columns E .. 2E - 1
    xdbl = 0.7 * torch.randn(2, M, R + 2 * N, generator=g)
    dirs = []
    for _ in range(2):
        f = torch.exp(torch.rand(E, 1, generator=g) * np.log(4.0) + np.log(0.5))
        dt = torch.exp(torch.rand(E, generator=g) * np.log(100.0) + np.log(1e-3))
        dt_b = dt + torch.log(-torch.expm1(-dt))
        # every 7th channel: delta = about 30 +- 2, past softplus's threshold of 20, and delta A down to -30 * 32 = -960: the decay underflows
        dt_b[3::7] += 30.0
        dirs.append({"dt_w": torch.randn(E, R, generator=g) * (2.0 / R ** 0.5), "dt_b": dt_b,
                     "A_log": torch.log(torch.arange(1, N + 1, dtype=torch.float32)[None, :] * f), "D": 1.0 + 0.3 * torch.randn(E, generator=g)})
    return xc, xz, xdbl, dirs


def _scan_ref(xc, z, xdbl, dirs, B, L, E, R, dtype, which=(0, 1)):
    """The specification as a sequential loop over time in `dtype`: (o_fwd + o_bwd) / 2 [B L, E]; also the largest delta and the
    smallest delta A seen."""
    out = torch.zeros(B, L, E, dtype=dtype)
    gate = F.silu(z.to(dtype)).view(B, L, E)
    dmax, amin = 0.0, 0.0
    for d in which:
        w = {k: v.to(dtype) for k, v in dirs[d].items()}
        x = xc[d].to(dtype).view(B, L, E)
        xd = xdbl[d].to(dtype).view(B, L, R + 2 * N)
        delta = F.softplus(xd[..., :R] @ w["dt_w"].t() + w["dt_b"])
        A = -torch.exp(w["A_log"])
        dmax, amin = max(dmax, float(delta.max())), min(amin, float((delta[..., None] * A).min()))
        h = torch.zeros(B, E, N, dtype=dtype)
        y = torch.zeros(B, L, E, dtype=dtype)
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            dl = delta[:, t, :, None]
            h = torch.exp(dl * A) * h + (dl * x[:, t, :, None]) * xd[:, t, None, R:R + N]
            y[:, t] = (h * xd[:, t, None, R + N:]).sum(-1) + w["D"] * x[:, t]
        out += y * gate
    return (out / 2).view(B * L, E), dmax, amin


def _scan_gpu(hip_lib, xc, xz, xdbl, dirs, B, L, E, R, planes=False):
    keep = []
    arr = _dirs(dirs, keep)
    xcd, xzd, xdd = xc.cuda(), xz.cuda(), xdbl.cuda()
    need = hip_lib.pope_vim_scan_workspace_bytes(B, L, E)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    if planes:
        out = torch.zeros(B * L, 2 * E, dtype=torch.float16, device="cuda")
    else:
        out = torch.full((B * L, E), float("nan"), device="cuda")
    _lib.check(hip_lib.pope_vim_scan_f32(_lib.ptr(xcd), C.c_void_p(xzd.data_ptr() + 4 * E), 2 * E, _lib.ptr(xdd), arr, B, L, E, R,
                                         None if planes else _lib.ptr(out), C.c_void_p(out.data_ptr()) if planes else None, _lib.ptr(ws),
                                         ws.numel(), C.c_void_p(flag.data_ptr()), None), "pope_vim_scan_f32")
    torch.cuda.synchronize()
    return out.cpu(), int(flag.item())


def _seam():
    return _lib.lib().pope_vim_scan_chunk()


# (B, L, E, R): a single step; shorter than the conv width; short odd L at E = D (tiny); the stride-16 length at E = 2 D (tiny);
# the stride-8 length at E = 2 D (small); then, added below, a whole multiple of the kernel's chunk length and that length +- 1
SCAN_SHAPES = [(1, 1, 64, 4), (2, 3, 64, 4), (1, 5, 192, 12), (1, 197, 384, 12), (2, 730, 768, 24)]
SEAM_SHAPES = [(2, -1, 64, 4), (2, 0, 64, 4), (2, 1, 64, 4)]       # L = 2 chunks + the entry


def _check_scan(hip_lib, B, L, E, R, which):
    xc, xz, xdbl, dirs = _scan_inputs(B, L, E, R, seed=L * 1000 + E)
    if which != (0, 1):       # one direction alone: the other direction's x is zero, so its y is exactly zero
        xc[1 - which[0]] = 0.0
    z = xz[:, E:]
    want, dmax, amin = _scan_ref(xc, z, xdbl, dirs, B, L, E, R, torch.float64, which)
    got32, _, _ = _scan_ref(xc, z, xdbl, dirs, B, L, E, R, torch.float32, which)
    e32 = float((got32.double() - want).abs().max())
    assert dmax > 20.0 and amin < -100.0, (dmax, amin)     # the inputs reach past the softplus threshold and into the underflow
    got, _ = _scan_gpu(hip_lib, xc, xz, xdbl, dirs, B, L, E, R)
    assert torch.isfinite(got).all()
    err = float((got.double() - want).abs().max())
    print(f"scan B {B} L {L} E {E} dirs {which}: max |gpu - fp64| = {err:.3g} = {err / e32:.2f} x e32 ({e32:.3g}); delta up to {dmax:.3g}, "
          f"delta A down to {amin:.3g}")
    assert err <= MARGIN * e32
    return xc, xz, xdbl, dirs, got


@pytest.mark.parametrize("B,L,E,R", SCAN_SHAPES)
def test_scan_against_fp64_loop(hip_lib, B, L, E, R):
    _check_scan(hip_lib, B, L, E, R, (0, 1))


@pytest.mark.parametrize("which", [(0, 1), (0,), (1,)], ids=["both", "forward", "backward"])
@pytest.mark.parametrize("B,dL,E,R", SEAM_SHAPES, ids=["2chunks-1", "2chunks", "2chunks+1"])
def test_scan_at_the_chunk_seams(hip_lib, B, dL, E, R, which):
    _check_scan(hip_lib, B, 2 * _seam() + dL, E, R, which)


def test_scan_planes_output_and_determinism(hip_lib):
    B, L, E, R = 2, 2 * _seam() + 1, 192, 12
    xc, xz, xdbl, dirs, got = _check_scan(hip_lib, B, L, E, R, (0, 1))
    again, _ = _scan_gpu(hip_lib, xc, xz, xdbl, dirs, B, L, E, R)
    assert torch.equal(got, again)
    # image 1 alone: the same bits as in the batch
    alone, _ = _scan_gpu(hip_lib, xc[:, L:], xz[L:], xdbl[:, L:], dirs, 1, L, E, R)
    assert torch.equal(alone, got[L:])
    pl, flag = _scan_gpu(hip_lib, xc, xz, xdbl, dirs, B, L, E, R, planes=True)
    assert flag == 0 and torch.equal(pl.view(B * L, E // 32, 2, 32), _lib.to_planes(got, _lib.PLANES_ACT_SCALE))


def test_scan_of_zero_x_is_zero(hip_lib):
    B, L, E, R = 2, _seam() + 3, 64, 4
    xc, xz, xdbl, dirs = _scan_inputs(B, L, E, R, seed=5, zero_x=True)
    got, _ = _scan_gpu(hip_lib, xc, xz, xdbl, dirs, B, L, E, R)
    assert torch.equal(got, torch.zeros_like(got))


# ---- conv1d + SiLU ----------------------------------------------------------------------------------------------------------
def _conv_ref(x, w, b, dtype, anti):
    """x [B, L, E]: silu(b + sum_k w[k] x[t - 3 + k]), or with x[t + 3 - k] (the backward direction in un-reversed time)."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    L = x.shape[1]
    xp = F.pad(x, (0, 0, 3, 3))
    acc = b + sum(w[:, k] * (xp[:, 6 - k:6 - k + L] if anti else xp[:, k:k + L]) for k in range(4))
    return F.silu(acc)


@pytest.mark.parametrize("E", [64, 768])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 730])
def test_conv1d_silu_against_fp64(hip_lib, L, E):
    B = 2
    g = torch.Generator().manual_seed(10 * L + E)
    xz = torch.randn(B * L, 2 * E, generator=g)                  # x = the first E columns of a row of pitch 2 E
    ws = [{"conv_w": 0.5 * torch.randn(E, 4, generator=g), "conv_b": 0.2 * torch.randn(E, generator=g)} for _ in range(2)]
    keep = []
    arr = _dirs(ws, keep)
    xd = xz.cuda()
    out = torch.full((2, B * L, E), float("nan"), device="cuda")
    _lib.check(hip_lib.pope_vim_conv1d_silu_f32(_lib.ptr(xd), 2 * E, arr, B, L, E, _lib.ptr(out), None), "pope_vim_conv1d_silu_f32")
    torch.cuda.synchronize()
    x = xz[:, :E].reshape(B, L, E)
    for d, name in enumerate(("causal", "anti-causal")):
        want = _conv_ref(x, ws[d]["conv_w"], ws[d]["conv_b"], torch.float64, d == 1).reshape(B * L, E)
        e32 = float((_conv_ref(x, ws[d]["conv_w"], ws[d]["conv_b"], torch.float32, d == 1).reshape(B * L, E).double() - want).abs().max())
        err = float((out[d].cpu().double() - want).abs().max())
        print(f"conv1d L {L} E {E} {name}: max |gpu - fp64| = {err:.3g} = {err / e32:.2f} x e32 ({e32:.3g})")
        assert err <= MARGIN * e32


# ---- add + RMSNorm ----------------------------------------------------------------------------------------------------------
def _rms_ref(r, w, eps, dtype):
    r, w = r.to(dtype), w.to(dtype)
    return r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w


def _rms_gpu(hip_lib, hidden, res, w, rows, D, eps, planes=False, stride=1, offset=0, want_res=True):
    hd, wd = hidden.cuda(), w.cuda()
    rd = res.cuda() if res is not None else None
    ro = torch.full_like(hd, float("nan")) if want_res else None
    y = torch.zeros(rows, 2 * D, dtype=torch.float16, device="cuda") if planes else torch.full((rows, D), float("nan"), device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(hip_lib.pope_vim_add_rmsnorm_f32(_lib.ptr(hd), _lib.ptr(rd), _lib.ptr(ro), _lib.ptr(wd), None if planes else _lib.ptr(y),
                                                C.c_void_p(y.data_ptr()) if planes else None, rows, D, eps, stride, offset,
                                                C.c_void_p(flag.data_ptr()), None), "pope_vim_add_rmsnorm_f32")
    torch.cuda.synchronize()
    return y.cpu(), (ro.cpu() if want_res else None), int(flag.item())


@pytest.mark.parametrize("later", [False, True], ids=["first-block", "later-block"])
@pytest.mark.parametrize("rows", [1, 730 * 2])
@pytest.mark.parametrize("D", [192, 384])
def test_add_rmsnorm_against_fp64(hip_lib, D, rows, later):
    g = torch.Generator().manual_seed(D + rows + later)
    hidden = torch.randn(rows, D, generator=g) * 1.3
    res = torch.randn(rows, D, generator=g) * 4.0 if later else None
    w = 1.0 + 0.3 * torch.randn(D, generator=g)
    eps = 1e-5
    r32 = hidden + res if later else hidden
    r64 = hidden.double() + res.double() if later else hidden.double()
    want = _rms_ref(r64, w, eps, torch.float64)
    e32 = float((_rms_ref(r32, w, eps, torch.float32).double() - want).abs().max())
    y, ro, _ = _rms_gpu(hip_lib, hidden, res, w, rows, D, eps)
    assert torch.equal(ro, r32)                                  # one fp32 add: the residual stream is exact
    err = float((y.double() - want).abs().max())
    print(f"add+rmsnorm D {D} rows {rows} later {later}: max |gpu - fp64| = {err:.3g} = {err / e32:.2f} x e32 ({e32:.3g})")
    assert err <= MARGIN * e32
    pl, ro2, flag = _rms_gpu(hip_lib, hidden, res, w, rows, D, eps, planes=True)
    assert flag == 0 and torch.equal(ro2, ro)
    assert torch.equal(pl.view(rows, D // 32, 2, 32), _lib.to_planes(y, _lib.PLANES_ACT_SCALE))
    if rows > 1:       # the final norm's form: only the class-token row of every image, no residual written
        sub, none, _ = _rms_gpu(hip_lib, hidden, res, w, 2, D, eps, stride=730, offset=364, want_res=False)
        assert none is None and torch.equal(sub, y[364::730])


# ---- the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_independence_and_determinism(precision):
    model, x, f, o, t = run_case("tiny_s16", precision)             # L = 197: four scan chunks
    g = torch.Generator().manual_seed(77)
    x3 = torch.cat([x, torch.randn(1, 3, 224, 224, generator=g).cuda()])
    f3, o3, t3 = model.forward_with_taps(x3)
    f3b, o3b, t3b = model.forward_with_taps(x3)
    assert torch.equal(f3, f3b) and torch.equal(o3, o3b) and all(torch.equal(a, b) for a, b in zip(t3, t3b))
    for b in range(3):
        fa, oa, ta = model.forward_with_taps(x3[b:b + 1])
        assert torch.equal(fa[0], f3[b]) and torch.equal(oa[0], o3[b])
        assert all(torch.equal(a[0], c[b]) for a, c in zip(ta, t3))
    assert torch.equal(f3[:2], f) and torch.equal(o3[:2], o)
    assert model.overflow_events == 0


def test_range_guard_weight_and_activation():
    model, x = build("small_s8_64", "f16x3")
    ref, _ = build("small_s8_64", "f32")
    with torch.no_grad():
        for m in (model, ref):
            m.layers[3].mixer.in_proj.weight[5, 7] = 300.0           # 300 * 256 > 65504: outside the weight contract
    want = ref(x)
    with pytest.warns(UserWarning, match="f16x3 range"):
        got = model(x)
    assert model.overflow_events == 1 and torch.equal(got, want)
    model.on_overflow = "raise"
    with pytest.raises(_lib.PopeRangeError):
        model(x)
    # an activation outside the contract: image values past 65504 / 8
    model, x = build("small_s8_64", "f16x3")
    ref, _ = build("small_s8_64", "f32")
    big = x * 1.0e4
    want = ref(big)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model(x)                                                     # in range: no event
    with pytest.warns(UserWarning, match="patch embed input"):
        got = model(big)
    assert model.overflow_events == 1 and torch.equal(got, want) and torch.isfinite(got).all()
    model.on_overflow = "raise"
    with pytest.raises(_lib.PopeRangeError):
        model(big)


def test_c_entries_check_their_arguments(hip_lib):
    """Return codes only: every call below is refused on the host, before any launch."""
    model, x = build("small_s8_64", "f32")
    w = model._weights("f32")
    need = hip_lib.pope_vim_workspace_bytes(C.byref(w), 3)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    feats = torch.empty(3, 384, device="cuda")

    def fwd(wp=C.byref(w), img=_lib.ptr(x), B=3, prec=0, wsp=_lib.ptr(ws), nbytes=need, f=_lib.ptr(feats)):
        return hip_lib.pope_vim_forward_f32(wp, img, B, prec, wsp, nbytes, f, None, None, None, None)

    assert fwd(wp=None) == -1 and fwd(img=None) == -1 and fwd(B=0) == -1 and fwd(B=-2) == -1 and fwd(prec=2) == -1 and fwd(wsp=None) == -1
    assert fwd(nbytes=need - 1) == -3 and fwd(nbytes=0) == -3
    assert fwd(prec=1) == -1                                          # f16x3 without weight planes
    B, L, E, R = 1, 5, 64, 4
    xc, xz, xdbl, dirs = _scan_inputs(B, L, E, R, seed=1)
    keep = []
    arr = _dirs(dirs, keep)
    xcd, xzd, xdd = xc.cuda(), xz.cuda(), xdbl.cuda()
    out = torch.zeros(B * L, E, device="cuda")
    sneed = hip_lib.pope_vim_scan_workspace_bytes(B, L, E)
    sws = torch.empty(sneed, dtype=torch.uint8, device="cuda")

    def scan(xcp=_lib.ptr(xcd), zp=_lib.ptr(xzd), xdp=_lib.ptr(xdd), d=arr, b=B, l=L, e=E, r=R, o=_lib.ptr(out), op=None, wsp=_lib.ptr(sws),
             nbytes=sneed):
        return hip_lib.pope_vim_scan_f32(xcp, zp, 2 * E, xdp, d, b, l, e, r, o, op, wsp, nbytes, None, None)

    assert scan(xcp=None) == -1 and scan(zp=None) == -1 and scan(xdp=None) == -1 and scan(d=None) == -1 and scan(o=None) == -1
    assert scan(b=0) == -1 and scan(l=0) == -1 and scan(e=40) == -1 and scan(r=5) == -1 and scan(r=36) == -1 and scan(wsp=None) == -1
    assert scan(op=_lib.ptr(out)) == -1                               # both outputs at once
    assert scan(nbytes=sneed - 1) == -3
    conv = hip_lib.pope_vim_conv1d_silu_f32
    cw = _dirs([{"conv_w": torch.zeros(E, 4), "conv_b": torch.zeros(E)}] * 2, keep)
    assert conv(None, 2 * E, cw, B, L, E, _lib.ptr(xcd), None) == -1 and conv(_lib.ptr(xzd), 2 * E, None, B, L, E, _lib.ptr(xcd), None) == -1
    assert conv(_lib.ptr(xzd), 2 * E, cw, 0, L, E, _lib.ptr(xcd), None) == -1 and conv(_lib.ptr(xzd), 2 * E, cw, B, 0, E, _lib.ptr(xcd), None) == -1
    assert conv(_lib.ptr(xzd), E - 4, cw, B, L, E, _lib.ptr(xcd), None) == -1 and conv(_lib.ptr(xzd), 2 * E, cw, B, L, E, None, None) == -1
    norm = hip_lib.pope_vim_add_rmsnorm_f32
    h, wv, y = _lib.ptr(out), _lib.ptr(feats), _lib.ptr(xcd)
    assert norm(None, None, None, wv, y, None, 5, 64, 1e-5, 1, 0, None, None) == -1
    assert norm(h, None, None, None, y, None, 5, 64, 1e-5, 1, 0, None, None) == -1
    assert norm(h, None, None, wv, None, None, 5, 64, 1e-5, 1, 0, None, None) == -1
    assert norm(h, None, None, wv, y, y, 5, 64, 1e-5, 1, 0, None, None) == -1
    assert norm(h, None, None, wv, y, None, 0, 64, 1e-5, 1, 0, None, None) == -1
    assert norm(h, None, None, wv, y, None, 5, 62, 1e-5, 1, 0, None, None) == -1
    assert norm(h, None, None, wv, None, y, 5, 48, 1e-5, 1, 0, None, None) == -1          # planes need D % 32 == 0
    assert norm(h, None, None, wv, y, None, 5, 64, 1e-5, 0, 0, None, None) == -1
    torch.cuda.synchronize()
