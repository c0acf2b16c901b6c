"""Comparison helpers of test_gpu_operand_producers.py (host only; test_operand_producers_cpu.py shows that each of them
rejects a plausible wrong kernel).  The GEMM operand producers write three formats:
  fp32 rows           y
  f16 rows            f16(y * 8)
  activation planes   [rows, cols / 32, 2, 32] f16 with y * 8 = hi + lo, hi = RNE f16 (pope_hip.h)
Every LayerNorm check compares with fp64 computed on the fp32 inputs.  Its bound is not a constant: 4 x the error of torch's own
fp32 LayerNorm on the same inputs (the factor covers the other summation order: a 64-lane butterfly against torch's cascade),
plus the representation error of the output format, which follows from the format alone."""
import torch
import torch.nn.functional as F

ACT = 8.0                      # POPE_PLANES_ACT_SCALE
WIDTHS = (128, 256, 384, 512, 640, 768, 1024, 1280, 1536, 2048)   # what the three LayerNorm launchers instantiate
LN_ROWS = 37                   # rows of a LayerNorm input set: the fp32 bound is taken over all of them (see ln_fp32_bound)
F16_NAN = 0x7E5A               # NaN bit patterns no kernel arithmetic produces (a quiet NaN with a payload): the pre-fill of
F32_NAN = 0x7FC5A5A5           # every output buffer and of its guard rows


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------
def ln_inputs(family, rows, dim, seed):
    """The two input families: `plain` randn * 3 + 0.7, `offset` randn * 0.5 + 50 (mean 100 standard deviations off zero: a
    one-pass E[x^2] - mean^2 variance loses its digits there); w = 1 + 0.1 randn, b = 0.1 randn."""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(rows, dim, generator=g)
    x = {"plain": n * 3.0 + 0.7, "offset": n * 0.5 + 50.0}[family]
    return x, 1.0 + 0.1 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)


def ln_ref64(x, w, b, eps):
    """LayerNorm in fp64 on the fp32 inputs, biased variance, eps inside the sqrt."""
    x, w, b = x.double(), w.double(), b.double()
    mean = x.mean(dim=1, keepdim=True)
    d = x - mean
    return d / torch.sqrt((d * d).mean(dim=1, keepdim=True) + eps) * w + b


def ln_fp32_bound(x, w, b, eps, ref):
    """4 x max |torch fp32 LayerNorm on the CPU - fp64| on these inputs.  Take it over the whole LN_ROWS-row input set that the
    cases of one width and family draw their leading rows from, not over the rows of one case: within a row the error is led
    by ONE rounding, the mean's (offset family: up to half an ulp of 50 against a deviation of 0.5), which a different but
    equally correct summation order rounds the other way — over a single row torch can land 8 x below the butterfly order
    (measured on the CPU restatement at width 2048: 1.1e-6 against 9.4e-6), over 37 rows the two maxima stay within 1.5 x at every width."""
    return 4.0 * float((F.layer_norm(x, (x.shape[1],), w, b, eps).double() - ref).abs().max())


def _assert_within(err, allowed, what):
    over = err - allowed
    i = int(over.argmax())
    assert float(over.flatten()[i]) <= 0.0, (f"{what}: |error| {float(err.flatten()[i]):.3e} > allowed "
                                              f"{float(allowed.flatten()[i]):.3e} at flat index {i}")
    return float(err.max()), float((err / allowed).max())


def check_ln_f32(got, ref, bound, what="layernorm fp32"):
    """fp32 rows against fp64; returns the observed maximum error and the largest error / allowed."""
    return _assert_within((got.double() - ref).abs(), torch.full_like(ref, bound), what)


def check_ln_f16(got_f16, ref, bound, what="layernorm f16"):
    """f16 rows of y * 8: one RNE rounding (2^-11 relative; 2^-25 absolute below the normal range, 2^-28 after the scale)."""
    assert got_f16.dtype == torch.float16
    return _assert_within((got_f16.double() / ACT - ref).abs(), 2.0 ** -11 * ref.abs() + 2.0 ** -28 + bound, what)


def split_hi_lo(planes):
    """[rows, cols / 32, 2, 32] -> hi, lo as [rows, cols] fp64 (still scaled)."""
    assert planes.dtype == torch.float16 and planes.dim() == 4 and planes.shape[2:] == (2, 32)
    r = planes.shape[0]
    return planes[:, :, 0].double().reshape(r, -1), planes[:, :, 1].double().reshape(r, -1)


def check_ln_planes(planes, ref, bound, what="layernorm planes"):
    """Planes of y * 8 against fp64:
      the pair      |(hi + lo) / 8 - ref| <= 2^-23 |ref| + 2^-28 + bound   lo is rounded once more, 12 bits below hi's last
      hi alone      |hi / 8 - ref| <= 2^-11 |ref| + bound                  RNE; truncation is off by up to 2^-10
      lo against hi |lo| <= 2^-11 |hi| + 2^-24                             a residual; swapped or shifted planes break it
    Returns the pair's observed maximum error and its largest error / allowed."""
    hi, lo = split_hi_lo(planes)
    _assert_within((hi / ACT - ref).abs(), 2.0 ** -11 * ref.abs() + bound, what + ": hi is not the RNE f16 of y * 8")
    _assert_within(lo.abs(), 2.0 ** -11 * hi.abs() + 2.0 ** -24, what + ": lo is not a residual of hi")
    return _assert_within(((hi + lo) / ACT - ref).abs(), 2.0 ** -23 * ref.abs() + 2.0 ** -28 + bound, what)


# ---- bit-exact converters ---------------------------------------------------------------------------------------------------
def assert_bits_equal(got, want, what):
    """Equality of two f16 / fp32 tensors as bit patterns (NaN-safe, distinguishes -0), with the first mismatch named."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    it = torch.int16 if got.dtype == torch.float16 else torch.int32
    a, b = got.contiguous().view(it).flatten(), want.contiguous().view(it).flatten()
    bad = (a != b).nonzero()
    if bad.numel():
        i = int(bad[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} elements differ, first at {idx}: got {float(got.flatten()[i])!r} "
                             f"(0x{int(a[i]) & 0xFFFFFFFF:x}), want {float(want.flatten()[i])!r} (0x{int(b[i]) & 0xFFFFFFFF:x})")


def im2col_planes_ref(img, patch):
    """The patch-embed A operand restated: F.unfold's column order k = c p^2 + dy p + dx per patch (row-major patches), zero
    padding up to kp = 3 p^2 rounded up to 32, a zero CLS row in front of every image, then the planes layout at scale 8.
    img [B, 3, H, W] fp32 -> f16 [B * ntok, kp / 32, 2, 32]."""
    from pope_amd import _lib
    B, C, H, W = img.shape
    assert C == 3 and H % patch == 0 and W % patch == 0
    k = 3 * patch * patch
    kp = (k + 31) // 32 * 32
    cols = F.unfold(img, kernel_size=patch, stride=patch).transpose(1, 2)      # [B, L, k]
    rows = F.pad(cols, (0, kp - k, 1, 0))                                      # zero columns behind, a zero row in front
    return _lib.to_planes(rows.reshape(-1, kp), ACT)


def patch_tokens_ref64(img, proj_w, posb, patch):
    """tokens[b, n] = posb[n] + patches[b, n] . proj_w^T in fp64 (n = 0: the CLS row, posb[0] alone)."""
    cols = F.unfold(img.double(), kernel_size=patch, stride=patch).transpose(1, 2)
    return posb.double() + F.pad(cols @ proj_w.double().t(), (0, 0, 1, 0))


# ---- guarded buffers --------------------------------------------------------------------------------------------------------
def guarded(numel, dtype, device, guard=512):
    """An output buffer of `numel` elements between two guards of `guard` elements, all pre-filled with the NaN pattern of
    `dtype` (f16 or fp32).  Returns (whole buffer as integers, payload view in `dtype`); the payload is 1 KiB-aligned at least
    (torch allocates on 512 bytes and the guard is a multiple of that)."""
    it, pat = (torch.int16, F16_NAN) if dtype == torch.float16 else (torch.int32, F32_NAN)
    whole = torch.full((numel + 2 * guard,), pat, dtype=it, device=device)
    return whole, whole[guard:guard + numel].view(dtype)


def check_guarded(whole, numel, what, guard=512, written=True):
    """The guards still hold the pattern; with `written`, no payload element does (every element was written)."""
    pat = F16_NAN if whole.dtype == torch.int16 else F32_NAN
    w = whole.cpu()
    assert bool((w[:guard] == pat).all()), f"{what}: wrote in front of the output"
    assert bool((w[guard + numel:] == pat).all()), f"{what}: wrote past the end of the output"
    if written:
        left = int((w[guard:guard + numel] == pat).sum())
        assert left == 0, f"{what}: {left} of {numel} output elements never written"


def range_bits():
    """The POPE_RANGE_* names and values of include/pope_hip.h."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pope_hip.h")).read()
    return {name: int(value) for name, value in re.findall(r"\bPOPE_RANGE_([A-Z0-9]+)\s*=\s*(\d+)", text)}
