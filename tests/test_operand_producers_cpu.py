"""Host only: the argument contract of the operand-producer entries (rejected before any HIP call), and the comparison helpers
of test_gpu_operand_producers.py (operand_checks.py) accepting an honest fp32 restatement of each kernel and rejecting
plausible wrong ones: a one-pass variance, a truncated hi plane, swapped planes, an im2col with dy and dx transposed, a
padding column left unzeroed."""
import ctypes as C

import operand_checks as K
import pytest
import torch

FAKE = C.c_void_p(0x1000)   # 16-byte aligned, never dereferenced: every call below is rejected before it reaches the device
ERR_ARG = -1                # POPE_ERR_ARG
EPS = 1e-6
BAD_DIMS = (0, 64, 896, 1152, 2176)   # not a multiple of 128, or a multiple no launcher instantiates (7, 9, 17 x 128)


# ---- argument contract ------------------------------------------------------------------------------------------------------
def test_layernorm_entries_reject_bad_arguments_without_gpu(hip_lib):
    entries = {
        "f32": lambda x, w, b, y, rows, dim: hip_lib.pope_layernorm_f32(x, w, b, y, rows, dim, EPS, None),
        "planes": lambda x, w, b, y, rows, dim: hip_lib.pope_layernorm_planes_f32(x, w, b, y, rows, dim, EPS, None, None),
        "f16": lambda x, w, b, y, rows, dim: hip_lib.pope_layernorm_f16(x, w, b, y, rows, dim, EPS, None, None),
    }
    for name, call in entries.items():
        for nulled in range(4):
            ptrs = [None if i == nulled else FAKE for i in range(4)]
            assert call(*ptrs, 4, 384) == ERR_ARG, (name, "null pointer", nulled)
        for rows in (0, -3):
            assert call(FAKE, FAKE, FAKE, FAKE, rows, 384) == ERR_ARG, (name, rows)
        for dim in BAD_DIMS + (-128,):
            assert call(FAKE, FAKE, FAKE, FAKE, 4, dim) == ERR_ARG, (name, dim)


def test_to_f16_rejects_bad_arguments_without_gpu(hip_lib):
    f = hip_lib.pope_to_f16
    assert f(None, FAKE, 8, None, None) == ERR_ARG and f(FAKE, None, 8, None, None) == ERR_ARG
    for n in (0, -4, 1, 2, 3, 1026, (1 << 33) + 2):
        assert f(FAKE, FAKE, n, None, None) == ERR_ARG, n


def test_div_planes_rejects_bad_arguments_without_gpu(hip_lib):
    def f(src=FAKE, bs=4 * 64, planes=FAKE, n=2, rows=4, cols=64):
        return hip_lib.pope_div_planes_f32(src, bs, planes, n, rows, cols, 8.0, 256.0, None, None)
    rejected = {
        "null src": dict(src=None), "null planes": dict(planes=None), "n = 0": dict(n=0), "n < 0": dict(n=-1),
        "rows = 0": dict(rows=0), "rows < 0": dict(rows=-2), "cols = 0": dict(cols=0), "cols % 32 != 0 (48)": dict(cols=48, bs=4 * 48),
        "cols % 32 != 0 (16)": dict(cols=16), "cols < 0": dict(cols=-32), "odd batch_stride": dict(bs=4 * 64 + 1),
        "batch_stride below one block": dict(bs=4 * 64 - 2),
    }
    for what, kw in rejected.items():
        assert f(**kw) == ERR_ARG, what


# ---- honest and wrong LayerNorms in fp32 torch --------------------------------------------------------------------------------
def ln_wave_fp32(x, w, b, eps, one_pass=False):
    """The wave-per-row kernels' arithmetic in fp32: lane l holds columns i * 128 + 2 l, + 1 and adds them in ascending i, the 64
    lanes combine in a butterfly; mean first, then the centred second moment — or, one_pass, E[x^2] - mean^2."""
    r, d = x.shape
    v = x.view(r, d // 128, 64, 2)

    def wave_sum(t):                      # [r, nv, 64] -> [r, 1]
        s = torch.zeros(r, 64)
        for i in range(t.shape[1]):
            s = s + t[:, i]
        n = 64
        while n > 1:
            s, n = s[:, :n // 2] + s[:, n // 2:n], n // 2
        return s
    inv_d = torch.tensor(1.0 / d, dtype=torch.float32)
    mean = wave_sum(v[..., 0] + v[..., 1]) * inv_d
    if one_pass:
        var = wave_sum(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) * inv_d - mean * mean
    else:
        dv = v - mean.view(r, 1, 1, 1)
        var = wave_sum(dv[..., 0] * dv[..., 0] + dv[..., 1] * dv[..., 1]) * inv_d
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return (x - mean) * rstd * w + b


def _formats(y):
    """An fp32 result in the three output formats, with the checker of each."""
    from pope_amd import _lib
    return {"f32": (y, K.check_ln_f32), "f16": ((y * K.ACT).half(), K.check_ln_f16), "planes": (_lib.to_planes(y, K.ACT), K.check_ln_planes)}


@pytest.mark.parametrize("dim", K.WIDTHS)
def test_ln_checks_accept_two_pass_and_reject_one_pass(dim):
    for family in ("plain", "offset"):
        xs, w, b = K.ln_inputs(family, K.LN_ROWS, dim, seed=dim + len(family))
        ref_all = K.ln_ref64(xs, w, b, EPS)
        bound = K.ln_fp32_bound(xs, w, b, EPS, ref_all)
        for rows in (1, 4, 5, 8, 9, 37):
            x, ref = xs[:rows].contiguous(), ref_all[:rows]
            for fmt, (got, check) in _formats(ln_wave_fp32(x, w, b, EPS)).items():
                err, ratio = check(got, ref, bound, f"two-pass {fmt} {family} dim {dim} rows {rows}")
                assert ratio <= 1.0
            if family == "offset" and rows == 37:
                for fmt, (got, check) in _formats(ln_wave_fp32(x, w, b, EPS, one_pass=True)).items():
                    with pytest.raises(AssertionError, match="allowed"):
                        check(got, ref, bound, f"one-pass {fmt}")
    print(f"dim {dim}: offset family, 37 rows: fp32 bound {bound:.2e}, two-pass {err:.2e}")


def _truncated_half(ts):
    """fp32 -> f16 rounded towards zero."""
    h = ts.half()
    bits = h.view(torch.int16).clone()
    bits[h.float().abs() > ts.abs()] -= 1          # sign-magnitude: one step down in magnitude for either sign
    return bits.view(torch.float16)


def _stack_planes(hi, lo):
    r, c = hi.shape
    return torch.stack([hi.view(r, c // 32, 32), lo.view(r, c // 32, 32)], dim=2).contiguous()


@pytest.mark.parametrize("family", ["plain", "offset"])
def test_planes_check_rejects_truncation_and_swapped_planes(family):
    from pope_amd import _lib
    x, w, b = K.ln_inputs(family, 9, 384, seed=3)
    ref = K.ln_ref64(x, w, b, EPS)
    bound = K.ln_fp32_bound(x, w, b, EPS, ref)
    y = ln_wave_fp32(x, w, b, EPS)
    good = _lib.to_planes(y, K.ACT)
    K.check_ln_planes(good, ref, bound)
    ts = y * K.ACT
    hi = _truncated_half(ts)
    assert bool((hi.float().abs() <= ts.abs()).all()) and not torch.equal(hi, ts.half())
    with pytest.raises(AssertionError, match="RNE"):       # hi + lo still carries y to 22 bits: only the hi check sees it
        K.check_ln_planes(_stack_planes(hi, (ts - hi.float()).half()), ref, bound)
    with pytest.raises(AssertionError):
        K.check_ln_planes(good.flip(2), ref, bound)          # hi and lo swapped
    shifted = good.clone()
    shifted[:, :, 1] = good[:, :, 1].roll(1, dims=-1)      # lo one lane off: each value plausible, the pair wrong
    with pytest.raises(AssertionError):
        K.check_ln_planes(shifted, ref, bound)
    with pytest.raises(AssertionError, match="residual"):  # hi right, lo another chunk's hi
        K.check_ln_planes(_stack_planes(ts.half(), ts.half().roll(32, dims=1)), ref, bound)


# ---- im2col -----------------------------------------------------------------------------------------------------------------
def _im2col_by_reshape(img, patch, transposed=False):
    """The operand without F.unfold: [B, 3, gh, p, gw, p] -> rows (b, py, px), columns (c, dy, dx) — or (c, dx, dy)."""
    from pope_amd import _lib
    B, _, H, W = img.shape
    gh, gw, k = H // patch, W // patch, 3 * patch * patch
    kp = (k + 31) // 32 * 32
    t = img.view(B, 3, gh, patch, gw, patch).permute(0, 2, 4, 1, 5, 3) if transposed else img.view(B, 3, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5)
    rows = torch.zeros(B, 1 + gh * gw, kp)
    rows[:, 1:, :k] = t.reshape(B, gh * gw, k)
    return _lib.to_planes(rows.view(-1, kp), K.ACT)


@pytest.mark.parametrize("B,H,W,patch", [(2, 28, 42, 14), (1, 14, 21, 7), (2, 8, 12, 4), (1, 16, 24, 8)])
def test_im2col_restatement_rejects_transposed_patches_and_dirty_padding(B, H, W, patch):
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(H))
    want = K.im2col_planes_ref(img, patch)
    k, ntok = 3 * patch * patch, 1 + (H // patch) * (W // patch)
    assert want.shape == (B * ntok, (k + 31) // 32, 2, 32)
    K.assert_bits_equal(_im2col_by_reshape(img, patch), want, "reshape restatement")
    with pytest.raises(AssertionError, match="differ"):
        K.assert_bits_equal(_im2col_by_reshape(img, patch, transposed=True), want, "dy / dx transposed")
    dirty_cls = want.clone()
    dirty_cls[ntok * (B - 1), 0, 1, 5] = 2.0 ** -24                 # the CLS row of the last image, a lo half
    with pytest.raises(AssertionError, match="differ"):
        K.assert_bits_equal(dirty_cls, want, "CLS row not zeroed")
    if k % 32:
        dirty = want.clone()
        dirty[-1, -1, 0, 31] = 1.0                                  # the last padding column of the last patch
        with pytest.raises(AssertionError, match="1 of"):
            K.assert_bits_equal(dirty, want, "padding column not zeroed")
        stale = want.clone()
        stale.view(torch.int16)[1, -1, 1, 31] = K.F16_NAN           # never written: the pre-fill pattern, a NaN
        with pytest.raises(AssertionError, match="1 of"):
            K.assert_bits_equal(stale, want, "padding column never written")


def test_guard_rows_catch_stray_and_missing_writes():
    for dt in (torch.float16, torch.float32):
        whole, out = K.guarded(96, dt, "cpu")
        assert out.data_ptr() - whole.data_ptr() == 512 * out.element_size() and bool(out.isnan().all())
        with pytest.raises(AssertionError, match="never written"):
            K.check_guarded(whole, 96, "untouched")
        out.zero_()
        K.check_guarded(whole, 96, "clean")
        for at, msg in ((511, "in front"), (512 + 96, "past the end")):
            whole[at] = 0
            with pytest.raises(AssertionError, match=msg):
                K.check_guarded(whole, 96, "stray")
            whole[at] = K.F16_NAN if dt == torch.float16 else K.F32_NAN
        out[95] = float("nan")                                      # a NaN the kernel computed is not the pre-fill pattern
        K.check_guarded(whole, 96, "computed NaN")


def test_range_bits_come_from_the_header():
    from pope_amd import _lib
    bits = K.range_bits()
    assert bits == {"PATCH": 1, "LAYERNORM": 2, "QKV": 4, "GELU": 8, "MATCH": 16, "INPUT": 32}
    assert sorted(bits.values()) == sorted(_lib.RANGE_BITS)
