"""GPU: the kernels that write the GEMM operands (pope_amd/csrc/layernorm.hip) one by one through the C ABI, against fp64 or
against a bit-exact torch restatement: the three LayerNorm output formats at all ten widths and on both planes routes, the
rowln-order twin, the plane splitters, the f16 converter and the two im2col kernels, each with the threshold of its range
guard.  Every output sits between guard rows, is pre-filled with a NaN pattern (operand_checks.guarded) and is produced twice;
the two runs must agree bit for bit.  The comparison functions live in operand_checks.py (test_operand_producers_cpu.py shows
that they reject wrong kernels)."""
import ctypes as C
import math

import numpy as np
import operand_checks as K
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6
ACT, WSC = 8.0, 256.0                                  # POPE_PLANES_ACT_SCALE, POPE_PLANES_W_SCALE
BITS = K.range_bits()
LIMIT = 65520.0                                        # smallest magnitude that RNE-rounds to f16 infinity
SPARE = 1 << 20                                        # a bit no producer owns: it must survive every call
ROWS_WAVE, ROWS_HALF, ROWS_ROWLN = (1, 4, 5, 37), (1, 8, 9, 37), (1, 16, 17)   # full, partial and many blocks of 4 / 8 / 16 rows
WAVE, HALF = "layernorm_planes_kernel", "layernorm_planes_half_kernel"


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _below(v):
    """The fp32 neighbour of v towards zero."""
    return float(np.nextafter(np.float32(v), np.float32(0)))


def _shifted(t, dev, floats=2):
    """t on the device as a view `floats` floats into a larger buffer: 8-byte but not 16-byte aligned for floats = 2."""
    buf = torch.zeros(t.numel() + 8, device=dev)
    v = buf[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * floats
    return v


def _twice(numel, dtype, dev, call, what):
    """call(out) -> status, run on two fresh guarded buffers: guards intact, every element written, both runs bit-equal."""
    outs = []
    for _ in range(2):
        whole, out = K.guarded(numel, dtype, dev)
        assert out.data_ptr() % 16 == 0
        assert call(out) == 0, what
        torch.cuda.synchronize()
        K.check_guarded(whole, numel, what)
        outs.append(out.cpu())
    K.assert_bits_equal(outs[1], outs[0], what + ": second run against the first")
    return outs[0]


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.fixture(scope="module")
def kernel_names(dev, hip_lib):
    """names(fn) -> the device kernels fn launched, by torch.profiler.  Control: one fp32 LayerNorm launch must be seen by its
    name — the route tests below rest on the names, so a profiler that is blind to the library's kernels fails them here rather
    than letting them pass on numerics alone."""
    x, y = torch.zeros(4, 128, device=dev), torch.empty(4, 128, device=dev)
    seen = _device_kernels(lambda: hip_lib.pope_layernorm_f32(_p(x), _p(x), _p(x), _p(y), 4, 128, EPS, _st()))
    assert any("layernorm_kernel" in n for n in seen), f"torch.profiler does not see the library's kernels: {seen[:5]}"
    return _device_kernels


# ---- LayerNorm: values -------------------------------------------------------------------------------------------------------
ENTRIES = {   # name -> (output dtype, output elements per input element)
    "f32": (torch.float32, 1), "planes": (torch.float16, 2), "f16": (torch.float16, 1),
    "rowln_f32": (torch.float32, 1), "rowln_planes": (torch.float16, 2),
}


def _ln_call(hip_lib, entry, x, w, b, rows, dim, flag=None):
    if entry == "f32":
        return lambda out: hip_lib.pope_layernorm_f32(_p(x), _p(w), _p(b), _p(out), rows, dim, EPS, _st())
    if entry == "planes":
        return lambda out: hip_lib.pope_layernorm_planes_f32(_p(x), _p(w), _p(b), _p(out), rows, dim, EPS, _p(flag), _st())
    if entry == "f16":
        return lambda out: hip_lib.pope_layernorm_f16(_p(x), _p(w), _p(b), _p(out), rows, dim, EPS, _p(flag), _st())
    assert dim == 384
    if entry == "rowln_f32":
        return lambda out: hip_lib.pope_layernorm_rowln_order_f32(_p(x), _p(w), _p(b), None, _p(out), rows, EPS, _p(flag), _st())
    return lambda out: hip_lib.pope_layernorm_rowln_order_f32(_p(x), _p(w), _p(b), _p(out), None, rows, EPS, _p(flag), _st())


def _ln_run(hip_lib, dev, entry, x, w, b, shift=None, flag=None, what=""):
    """One guarded double run of `entry` on host tensors; shift names the operand passed 8-byte-but-not-16-byte aligned."""
    rows, dim = x.shape
    dt, per = ENTRIES[entry]
    xd, wd, bd = (_shifted(t, dev) if shift == n else t.to(dev) for n, t in (("x", x), ("w", w), ("b", b)))
    out = _twice(rows * dim * per, dt, dev, _ln_call(hip_lib, entry, xd, wd, bd, rows, dim, flag), what)
    return out.view(rows, dim // 32, 2, 32) if per == 2 else out.view(rows, dim)


def _ln_check(entry, out, ref, bound, what):
    if ENTRIES[entry][1] == 2:
        return K.check_ln_planes(out, ref, bound, what)
    return (K.check_ln_f16 if out.dtype == torch.float16 else K.check_ln_f32)(out, ref, bound, what)


def _ln_values(hip_lib, dev, entry, dim, row_set, shift=None):
    worst = {}
    for family in ("plain", "offset"):
        xs, w, b = K.ln_inputs(family, K.LN_ROWS, dim, seed=dim + len(family))
        ref_all = K.ln_ref64(xs, w, b, EPS)
        bound = K.ln_fp32_bound(xs, w, b, EPS, ref_all)
        for rows in row_set:
            x, ref = xs[:rows].contiguous(), ref_all[:rows]
            what = f"{entry} dim {dim} rows {rows} {family}" + (f" ({shift} at 8 bytes)" if shift else "")
            out = _ln_run(hip_lib, dev, entry, x, w, b, shift, what=what)
            err = None
            try:
                err = _ln_check(entry, out, ref, bound, what)
            finally:
                print(f"LN {what}: " + ("over the bound" if err is None else f"observed {err[0]:.3e}, {err[1]:.3f} of allowed")
                      + f", fp32 bound {bound:.3e}")
            worst[family] = max(worst.get(family, (0.0, 0.0, 0.0)), (err[1], err[0], bound))
    print(f"LN-SUMMARY {entry} dim {dim}{' shift ' + shift if shift else ''}: "
          + ", ".join(f"{f} worst {r:.3f} of allowed (observed {e:.3e}, fp32 bound {bd:.3e})" for f, (r, e, bd) in worst.items()))


def _planes_rows(dim, shift):
    return ROWS_HALF if dim <= 512 and shift is None else ROWS_WAVE


@pytest.mark.parametrize("dim", K.WIDTHS)
@pytest.mark.parametrize("entry", ["f32", "planes", "f16"])
def test_layernorm_values(hip_lib, dev, entry, dim):
    """fp64 parity of the three output formats at every instantiated width; the planes entry takes its two-rows-per-wave
    kernel up to 512 here (16-byte aligned operands) and the wave-per-row kernel above."""
    _ln_values(hip_lib, dev, entry, dim, _planes_rows(dim, None) if entry == "planes" else ROWS_WAVE)


@pytest.mark.parametrize("shift", ["x", "w", "b"])
@pytest.mark.parametrize("dim", [d for d in K.WIDTHS if d <= 512])
def test_layernorm_planes_wave_route_below_512(hip_lib, dev, dim, shift):
    """One operand at an 8-byte-but-not-16-byte address sends widths <= 512 to the wave-per-row kernel (NV = 1..4)."""
    _ln_values(hip_lib, dev, "planes", dim, ROWS_WAVE, shift)


@pytest.mark.parametrize("entry", ["rowln_f32", "rowln_planes"])
def test_layernorm_rowln_order_values(hip_lib, dev, entry):
    _ln_values(hip_lib, dev, entry, 384, ROWS_ROWLN)


def test_layernorm_planes_route_switch(hip_lib, dev, kernel_names):
    """The kernel behind every width <= 512: the half kernel for aligned operands, the wave-per-row kernel as soon as x, w or b
    alone is not 16-byte aligned; above 512 always wave-per-row."""
    for dim in K.WIDTHS:
        x, w, b = K.ln_inputs("plain", 9, dim, seed=5)
        for shift in (None, "x", "w", "b") if dim <= 512 else (None,):
            xd, wd, bd = (_shifted(t, dev) if shift == n else t.to(dev) for n, t in (("x", x), ("w", w), ("b", b)))
            whole, out = K.guarded(9 * dim * 2, torch.float16, dev)
            names = kernel_names(lambda: hip_lib.pope_layernorm_planes_f32(_p(xd), _p(wd), _p(bd), _p(out), 9, dim, EPS, None, _st()))
            want = HALF if dim <= 512 and shift is None else WAVE
            names = [n for n in names if "layernorm" in n]
            assert len(names) == 1 and want in names[0], (dim, shift, want, names)
            print(f"route confirmed: dim {dim} shift {shift}: {names[0][:90]}")
            K.check_guarded(whole, 9 * dim * 2, f"route dim {dim} shift {shift}")


# ---- LayerNorm: rows whose result is exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", K.WIDTHS)
def test_layernorm_exact_rows(hip_lib, dev, dim):
    """x - mean == 0 exactly on an all-zero row, and on a constant row where the mean is exact (power-of-two widths): the
    output is b, bit for bit, in every format and on both planes routes — element c of the output IS b[c], so a permuted or
    shifted layout shows."""
    from pope_amd import _lib
    _, w, b = K.ln_inputs("plain", 1, dim, seed=77)
    fills = [0.0] + ([7.25] if dim & (dim - 1) == 0 else [])
    runs = [("f32", None, ROWS_WAVE), ("f16", None, ROWS_WAVE), ("planes", None, _planes_rows(dim, None))]
    if dim <= 512:
        runs.append(("planes", "x", ROWS_WAVE))
    if dim == 384:
        runs += [("rowln_f32", None, ROWS_ROWLN), ("rowln_planes", None, ROWS_ROWLN)]
    for entry, shift, row_set in runs:
        rows = row_set[2]                                   # one full block and one row of the next
        if ENTRIES[entry][1] == 2:
            want = _lib.to_planes(b[None], ACT).expand(rows, -1, -1, -1)
        else:
            want = ((b * ACT).half() if entry == "f16" else b)[None].expand(rows, -1)
        for fill in fills:
            out = _ln_run(hip_lib, dev, entry, torch.full((rows, dim), fill), w, b, shift, what=f"exact {entry} dim {dim} fill {fill}")
            K.assert_bits_equal(out, want.contiguous(), f"{entry} dim {dim} shift {shift}: a constant {fill} row must return b")


# ---- pure converters, bit for bit -------------------------------------------------------------------------------------------
def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("rows,ld", [(r, ld) for ld in (32, 64, 96, 384) for r in (1, 3, 1000)] + [(5500, 384)])
def test_split_planes_bits(hip_lib, dev, rows, ld):
    """pope_split_planes_f32 == _lib.to_planes; 5500 x 384 holds more than 4096 * 256 pairs: the grid-stride loop's second trip."""
    from pope_amd import _lib
    assert (rows, ld) != (5500, 384) or rows * ld // 2 > 4096 * 256
    for scale, mag in ((ACT, 3.0), (WSC, 0.05)):
        src = _randn(rows, ld, seed=rows + ld, scale=mag)
        sd = src.to(dev)
        out = _twice(rows * ld * 2, torch.float16, dev,
                     lambda o: hip_lib.pope_split_planes_f32(_p(sd), _p(o), rows, ld, scale, None, _st()), f"split {rows}x{ld} x{scale}")
        K.assert_bits_equal(out.view(rows, ld // 32, 2, 32), _lib.to_planes(src, scale), f"split_planes {rows}x{ld} scale {scale}")


@pytest.mark.parametrize("n", [4, 1028, "past_the_grid"])
def test_to_f16_bits(hip_lib, dev, n):
    """pope_to_f16 == (x * 8).half(); the last n is past 64 blocks per CU x 256 threads x 4 elements: a second grid-stride trip."""
    if n == "past_the_grid":
        n = 64 * torch.cuda.get_device_properties(0).multi_processor_count * 256 * 4 + 1028
    x = _randn(n, seed=n % 1000, scale=3.0)
    xd = x.to(dev)
    out = _twice(n, torch.float16, dev, lambda o: hip_lib.pope_to_f16(_p(xd), _p(o), n, None, _st()), f"to_f16 n {n}")
    K.assert_bits_equal(out, (x * ACT).half(), f"to_f16 n {n}")


@pytest.mark.parametrize("cols", [32, 64, 384])
@pytest.mark.parametrize("rows", [1, 63])
def test_div_planes_bits(hip_lib, dev, rows, cols):
    """pope_div_planes_f32 == to_planes(x / divisor, 256) with torch's fp32 division; three blocks batch_stride apart with NaN
    in the gaps, which must be neither read into the output nor flagged."""
    from pope_amd import _lib
    n, bs = 3, rows * cols + 6
    divisor = float(np.float32(math.sqrt(cols)))
    x = _randn(n, rows * cols, seed=rows + cols)
    src = torch.full((n, bs), float("nan"))
    src[:, :rows * cols] = x
    sd, flag = src.to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out = _twice(n * rows * cols * 2, torch.float16, dev,
                 lambda o: hip_lib.pope_div_planes_f32(_p(sd), bs, _p(o), n, rows, cols, divisor, WSC, _p(flag), _st()),
                 f"div_planes {rows}x{cols}")
    want = _lib.to_planes((x / torch.tensor(divisor, dtype=torch.float32)).view(n * rows, cols), WSC)
    K.assert_bits_equal(out.view(n * rows, cols // 32, 2, 32), want, f"div_planes {rows}x{cols}")
    assert int(flag) == 0, "the NaN between the blocks was read"


# ---- im2col -----------------------------------------------------------------------------------------------------------------
STRIP, ELEMENT = "im2col_planes_strip_kernel", "im2col_planes_kernel"
IM2COL_CASES = [   # (B, H, W, patch, floats the image sits into its buffer, kernel)
    pytest.param(2, 28, 238, 14, 0, STRIP, id="strip-17-patches-last-group-of-one"),
    pytest.param(1, 14, 14, 14, 0, STRIP, id="strip-single-patch"),
    pytest.param(1, 16, 24, 8, 0, STRIP, id="strip-patch8-per_pass-eq-patch"),
    pytest.param(1, 24, 204, 12, 0, STRIP, id="strip-patch12"),
    pytest.param(2, 8, 12, 4, 0, ELEMENT, id="element-patch4"),
    pytest.param(1, 14, 21, 7, 0, ELEMENT, id="element-odd-patch7"),
    pytest.param(1, 32, 48, 16, 0, ELEMENT, id="element-patch16-lds-over-48k"),
    pytest.param(1, 28, 42, 14, 1, ELEMENT, id="element-patch14-image-4-byte-aligned"),
]
DIM = 128


def _patch_operands(B, H, W, patch, dev, seed=3):
    from pope_amd import _lib
    k, ntok = 3 * patch * patch, 1 + (H // patch) * (W // patch)
    kp = (k + 31) // 32 * 32
    pw, posb = _randn(DIM, k, seed=seed, scale=k ** -0.5), _randn(ntok, DIM, seed=seed + 1)
    wp = _lib.to_planes(torch.nn.functional.pad(pw, (0, kp - k)), WSC).to(dev)
    return pw, posb, wp, posb.to(dev), ntok, kp


def _patch_call(hip_lib, img_d, wp, posb_d, tokens, scratch, B, H, W, patch, flag=None):
    return hip_lib.pope_patch_embed_planes_f32(_p(img_d), _p(wp), _p(posb_d), _p(tokens), B, H, W, patch, DIM, _p(scratch),
                                               scratch.numel() * 2, _p(flag), _st())


@pytest.mark.parametrize("B,H,W,patch,offset,kernel", IM2COL_CASES)
def test_im2col_operand_bits(hip_lib, dev, kernel_names, B, H, W, patch, offset, kernel):
    """The A operand pope_patch_embed_planes_f32 leaves in the caller's scratch, whole: [B * ntok, kp / 32, 2, 32] bit for bit
    against the unfold restatement (padding columns and CLS rows included), and the tokens against fp64."""
    pw, posb, wp, posb_d, ntok, kp = _patch_operands(B, H, W, patch, dev)
    img = _randn(B, 3, H, W, seed=H + W)
    img_d = _shifted(img, dev, offset) if offset else img.to(dev)
    assert img_d.data_ptr() % 8 == (4 if offset else 0)
    n_a, n_t = B * ntok * kp * 2, B * ntok * DIM
    got = []
    for run in range(2):
        (wa, scratch), (wt, tokens) = K.guarded(n_a, torch.float16, dev), K.guarded(n_t, torch.float32, dev)
        assert scratch.data_ptr() % 16 == 0                                # the strip route needs it
        def call():
            assert _patch_call(hip_lib, img_d, wp, posb_d, tokens, scratch, B, H, W, patch) == 0
        if run == 0:
            names = [n for n in kernel_names(call) if "im2col" in n]
            assert len(names) == 1 and kernel in names[0], (kernel, names)
            print(f"route confirmed: {names[0][:80]}")
        else:
            call()
        torch.cuda.synchronize()
        K.check_guarded(wa, n_a, "im2col operand")
        K.check_guarded(wt, n_t, "patch-embed tokens")
        got.append((scratch.cpu().view(B * ntok, kp // 32, 2, 32), tokens.cpu().view(B, ntok, DIM)))
    K.assert_bits_equal(got[1][0], got[0][0], "im2col operand: second run against the first")
    K.assert_bits_equal(got[1][1], got[0][1], "tokens: second run against the first")
    K.assert_bits_equal(got[0][0], K.im2col_planes_ref(img, patch), "im2col operand against the unfold restatement")
    err = float((got[0][1].double() - K.patch_tokens_ref64(img, pw, posb, patch)).abs().max())
    print(f"tokens B {B} {H}x{W} patch {patch}: max |err| against fp64 {err:.2e}")
    assert err <= 2e-5                                                     # test_gpu_ops.py test_patch_embed_tokens


# ---- range guards -----------------------------------------------------------------------------------------------------------
def _flag_after(dev, run, preset):
    flag = torch.full((1,), preset, dtype=torch.int32, device=dev)
    assert run(flag) == 0
    torch.cuda.synchronize()
    return int(flag)


def _drive_guard(dev, bit, limit, places, run_with, what):
    """run_with(place, value) -> run(flag): the producer with `value` at `place` of an otherwise harmless input.  At every place
    the word, pre-set to a foreign bit, must gain `bit` exactly from |value| * scale == 65520 on and for NaN and +-inf, and keep
    the foreign bit; below the threshold, and on a clean word, it must not change."""
    assert bit and bit & SPARE == 0
    for place in places:
        for value, sets in ((limit, True), (-limit, True), (_below(limit), False), (-_below(limit), False),
                            (float("nan"), True), (float("inf"), True), (float("-inf"), True)):
            for preset in (SPARE, 0) if not sets else (SPARE,):
                got = _flag_after(dev, run_with(place, value), preset)
                assert got == preset | (bit if sets else 0), f"{what}: value {value!r} at {place}: word {preset:#x} -> {got:#x}"


def _ln_guard_inputs(rows, dim, r, c, value):
    """Row r all zero (its output is b), the other rows random with an outlier against the sign of `value` in column c, w[c] = 1:
    with b[c] = value only row r reaches |value| — the rest stay about 3 below it.  A non-finite value goes into x[r, c] instead."""
    x, w, b = K.ln_inputs("plain", rows, dim, seed=dim + r)
    x[:, c], w[c] = (10.0 if value < 0 else -10.0), 1.0
    x[r] = 0.0
    if math.isfinite(value):
        b[c] = value
    else:
        x[r, c] = value
    return x, w, b


def _ln_guard(hip_lib, dev, entry, dim, rows, shift=None):
    dt, per = ENTRIES[entry]

    def run_with(place, value):
        x, w, b = _ln_guard_inputs(rows, dim, place[0], place[1], value)
        xd, wd, bd = (_shifted(t, dev) if shift == n else t.to(dev) for n, t in (("x", x), ("w", w), ("b", b)))
        whole, out = K.guarded(rows * dim * per, dt, dev)

        def run(flag):
            rc = _ln_call(hip_lib, entry, xd, wd, bd, rows, dim, flag)(out)
            torch.cuda.synchronize()
            K.check_guarded(whole, rows * dim * per, f"guard {entry} dim {dim}")
            return rc
        return run
    # first column of the first row; last column of the last row, which is alone in its block
    _drive_guard(dev, BITS["LAYERNORM"], LIMIT / ACT, [(0, 0), (rows - 1, dim - 1)], run_with, f"{entry} dim {dim} shift {shift}")


@pytest.mark.parametrize("dim", K.WIDTHS)
def test_layernorm_range_guard(hip_lib, dev, dim):
    _ln_guard(hip_lib, dev, "f16", dim, 5)
    _ln_guard(hip_lib, dev, "planes", dim, 9 if dim <= 512 else 5)
    if dim <= 512:
        _ln_guard(hip_lib, dev, "planes", dim, 5, shift="x")


def test_layernorm_rowln_order_range_guard(hip_lib, dev):
    _ln_guard(hip_lib, dev, "rowln_planes", 384, 17)
    # the fp32 output converts nothing: its word stays as it was whatever the values
    x, w, b = _ln_guard_inputs(17, 384, 16, 383, LIMIT / ACT)
    xd, wd, bd, out = x.to(dev), w.to(dev), b.to(dev), torch.empty(17, 384, device=dev)
    run = lambda flag: hip_lib.pope_layernorm_rowln_order_f32(_p(xd), _p(wd), _p(bd), None, _p(out), 17, EPS, _p(flag), _st())
    assert _flag_after(dev, run, SPARE) == SPARE and _flag_after(dev, run, 0) == 0


def _flat_guard(dev, numel, out_numel, places, bit, limit, launch, what):
    """A converter over `numel` floats: zeros but for one value."""
    def run_with(place, value):
        x = torch.zeros(numel)
        x[place] = value
        xd = x.to(dev)
        whole, out = K.guarded(out_numel, torch.float16, dev)

        def run(flag):
            rc = launch(xd, out, flag)
            torch.cuda.synchronize()
            K.check_guarded(whole, out_numel, what)
            return rc
        return run
    _drive_guard(dev, bit, limit, places, run_with, what)


def test_split_planes_range_guard(hip_lib, dev):
    rows, ld = 9, 96                                              # 432 pairs: one full block of 256 threads and a partial one
    for scale in (ACT, WSC):
        _flat_guard(dev, rows * ld, rows * ld * 2, [0, ld - 1, rows * ld - 1], BITS["INPUT"], LIMIT / scale,
                    lambda x, o, f: hip_lib.pope_split_planes_f32(_p(x), _p(o), rows, ld, scale, _p(f), _st()), f"split_planes x{scale}")


def test_to_f16_range_guard(hip_lib, dev):
    n = 1028                                                      # 257 quads: one full block and one thread of the next
    _flat_guard(dev, n, n, [0, 1023, n - 1], BITS["INPUT"], LIMIT / ACT,
                lambda x, o, f: hip_lib.pope_to_f16(_p(x), _p(o), n, _p(f), _st()), "to_f16")


def test_div_planes_range_guard(hip_lib, dev):
    n, rows, cols = 3, 3, 64                                      # divisor 8, exact: the threshold is 65520 / 256 * 8 on the input
    bs = rows * cols + 2
    places = [0, cols - 1, (n - 1) * bs + rows * cols - 1]       # first and last column of block 0, last element of the last block
    _flat_guard(dev, n * bs, n * rows * cols * 2, places, BITS["MATCH"], LIMIT / WSC * 8.0,
                lambda x, o, f: hip_lib.pope_div_planes_f32(_p(x), bs, _p(o), n, rows, cols, 8.0, WSC, _p(f), _st()), "div_planes")


@pytest.mark.parametrize("B,H,W,patch", [(2, 28, 238, 14), (2, 8, 12, 4)], ids=["strip", "element"])
def test_im2col_range_guard(hip_lib, dev, B, H, W, patch):
    """Through one pixel of a black image: the first, the last of the first image row, and the last of all (strip kernel: the
    last group of its patch row, one patch wide)."""
    _, _, wp, posb_d, ntok, kp = _patch_operands(B, H, W, patch, dev)
    n_a = B * ntok * kp * 2

    def run_with(place, value):
        img = torch.zeros(B * 3 * H * W)
        img[place] = value
        img_d = img.to(dev)
        (wa, scratch), tokens = K.guarded(n_a, torch.float16, dev), torch.empty(B * ntok * DIM, device=dev)

        def run(flag):
            rc = _patch_call(hip_lib, img_d, wp, posb_d, tokens, scratch, B, H, W, patch, flag)
            torch.cuda.synchronize()
            K.check_guarded(wa, n_a, "im2col operand")
            return rc
        return run
    _drive_guard(dev, BITS["PATCH"], LIMIT / ACT, [0, W - 1, B * 3 * H * W - 1], run_with, f"im2col patch {patch}")
