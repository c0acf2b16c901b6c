"""Cases, inputs, fp64 references, planted faults and the comparison of test_gpu_sam_decoder_seams.py (host only: CPU torch;
test_sam_decoder_checks_cpu.py shows that the case lists hold every seam value, that the inputs reach the regime each case is
about, that the comparison accepts fp32 restatements summing in the kernels' order and that it rejects the faults these kernels
are likely to have, on this very data).

The kernels of csrc/sam_decoder.hip, through their op-level entries:
  linear      pope_sam_decoder_token_linear_f32 (sd_lin_kernel): lin_rows rows per workgroup, one column per thread, k in order;
              columns below add_cols read X + ADD, the others X
  self        pope_sam_decoder_self_attention_f32 (sd_self_attn_kernel): 8 heads of 32 over the T tokens of a prompt
  t2i         pope_sam_decoder_t2i_attention_f32 (sd_t2i_attn_kernel): T queries against 4 096 keys, 8 heads of 16; thread tid of
              256 owns the keys tid + 256 i; maximum and sums go 16 keys per thread, then the wave, then the four waves
  i2t         pope_sam_decoder_i2t_attention_f32 (sd_i2t_attn_kernel): 4 096 queries against T tokens, fp32 rows or planes
  norm        pope_sam_decoder_residual_norm_f32 (sd_res_ln_kernel): LayerNorm(res[slot] + y) over 256 columns and its operands
  prep        pope_sam_decoder_prepare_keys_f32 (sd_prep_kernel): (image + dense)^T, image_pe^T: one add, checked bit for bit
  tail        pope_sam_decoder_upscale_tail_f32 (sd_tail_kernel): LayerNorm2d, GELU, ConvTranspose 2x2/2, GELU, hypernetwork dot
chunk (prompts per pass), lin_rows, max_tokens and base_tokens come from pope_sam_decoder_seams (`Seams`), never from literals.

Comparison of one GROUP of outputs (loftr_layer_checks.group_ratio: the project's convention, MARGIN = 4, plus a floor):
    max |gpu - fp64| <= MARGIN * max(e32, 2^-23 * max |fp64|)
e32 = max |fp32 - fp64| of the same torch restatement evaluated in fp32 on the same inputs; a non-finite result has ratio inf.
Groups: one per head for the attentions, one per 256-column block for the linear, one per tensor (keys, operand B) for the norm,
one per selected mask and per (mask, sub-pixel position (oy % 4, ox % 4)) for the tail, one per tensor and prompt chunk for the
whole decoder.  Nothing here is taken from the code under test.

Attention score regimes (asserted in fp64 by the CPU test through `attention_scores`): q and k are sqrt(2) randn, so a score
has a standard deviation of about 2 (`unit`).  `shift_up` / `shift_down` give every q the component A and every k the component
+A / -A along axis 0 of each head, A^2 / sqrt(d) = SHIFT: every score of every row lies within 60 of +SHIFT / -SHIFT, where
exp(s) without a maximum overflows / gives 0 / 0.  `peak`: the keys' axis-0 component is 0 except at the peak keys, whose scores
stand PEAK above the rest; two peaks differ by PEAK_GAP.  v carries a seeded gain per head."""
import collections
import math

import torch
import torch.nn.functional as F

from loftr_layer_checks import MARGIN, ULP, group_ratio, report  # noqa: F401  (one comparison for every pin of the project)

Seams = collections.namedtuple("Seams", "chunk lin_rows max_tokens base_tokens")

NPIX, GRID, D, DI, MLP, HEADS, NMASK = 4096, 64, 256, 128, 2048, 8, 4
THREADS, WAVE = 256, 64                  # of sd_t2i_attn_kernel: key = tid + THREADS * i, wave = tid // WAVE
SENTINEL = -1234.5
PLANES_LIMIT = 65504.0 / 8.0             # |value| from which a planes output must raise the range flag
SHIFT, PEAK, PEAK_GAP, TOKEN_PEAK = 150.0, 130.0, 0.5, 8.0
SLOT_MAP = (2, 0, 1, 1)                  # four prompts over three images: many to one, not the identity
TOKEN_EPS, UP_EPS = 1e-5, 1e-6


def read_seams(lib):
    import ctypes
    v = [ctypes.c_int(0) for _ in range(4)]
    lib.pope_sam_decoder_seams(*(ctypes.byref(x) for x in v))
    return Seams(*(x.value for x in v))


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def token_counts(s):
    return (s.base_tokens, s.base_tokens + 1, s.base_tokens + 2, s.base_tokens + 3, s.max_tokens - 1, s.max_tokens)


def launch_prompts(s):
    return (1, 2, s.chunk)


def head_ratios(got, want64, want32):
    """[..., HEADS * d] -> one ratio per head"""
    def heads(t):
        return t.reshape(-1, HEADS, t.shape[-1] // HEADS).unbind(1)
    return [group_ratio(g.contiguous(), w.contiguous(), s.contiguous()) for g, w, s in zip(heads(got), heads(want64), heads(want32))]


# ---- the three attentions -------------------------------------------------------------------------------------------------------
HEAD_DIM = {"self": 32, "t2i": 16, "i2t": 16}


def peak_keys(w):
    """the two peak keys of wave w: tid + THREADS * i with tid // WAVE == w and different i; over w they cover 0, 255, 256, 4095"""
    tid, (i1, i2) = {0: (0, (0, 1)), 1: (WAVE + 36, (3, 7)), 2: (2 * WAVE + 2, (5, 14)), 3: (THREADS - 1, (0, NPIX // THREADS - 1))}[w]
    assert tid // WAVE == w and i1 != i2
    return tid + THREADS * i1, tid + THREADS * i2


def attention_cases(s):
    Ts, Ps = token_counts(s), launch_prompts(s)
    cases = []

    def add(kernel, regime, T, P, slots=None, ldk=D, peaks=()):
        cid = f"{kernel}-{regime}-T{T}-P{P}" + ("-slots" if slots else "") + (f"-ldk{ldk}" if kernel == "t2i" else "")
        cases.append(dict(id=cid, kernel=kernel, regime=regime, T=T, P=P, slots=slots, ldk=ldk, peaks=tuple(peaks),
                          seed=7000 + 13 * len(cases)))

    for kernel in ("self", "t2i", "i2t"):
        for k, T in enumerate(Ts):
            add(kernel, "unit", T, Ps[k % 3], ldk=(D, DI)[k % 2])
        for k, regime in enumerate(("shift_up", "shift_down")):
            add(kernel, regime, Ts[4], Ps[1], ldk=(D, DI)[k % 2])
            add(kernel, regime, Ts[1], Ps[0], ldk=(DI, D)[k % 2])
        if kernel == "t2i":
            for w in range(THREADS // WAVE):
                add(kernel, f"peak_in_wave_{w}", Ts[2], Ps[1], ldk=(D, DI)[w % 2], peaks=peak_keys(w))
        else:
            for T in (Ts[5], Ts[0]):
                add(kernel, "peak_at_token_0", T, Ps[1], peaks=(0,))
                add(kernel, f"peak_at_token_{T - 1}", T, Ps[1], peaks=(T - 1,))
        if kernel != "self":
            add(kernel, "unit", Ts[2], len(SLOT_MAP), slots=SLOT_MAP)
    return cases


def attention_inputs(case):
    """q [P, Lq, H, d], k, v [n, Lk, H, d] fp32 and the slot of every prompt.  self: n = P, Lq = Lk = T.  t2i: Lq = T, Lk = 4096,
    n = slots of K / V (images).  i2t: Lq = 4096 with n slots of q, Lk = T with P sets of k / v."""
    g = _gen(case["seed"])
    kernel, regime, T, P = case["kernel"], case["regime"], case["T"], case["P"]
    d = HEAD_DIM[kernel]
    slots = list(case["slots"]) if case["slots"] else list(range(P))
    n = max(slots) + 1
    Lq, Lk = (NPIX if kernel == "i2t" else T), (NPIX if kernel == "t2i" else T)
    nq, nk = (n, P) if kernel == "i2t" else (P, n)
    amp = math.sqrt(2.0)
    q = amp * torch.randn(nq, Lq, HEADS, d, generator=g)
    k = amp * torch.randn(nk, Lk, HEADS, d, generator=g)
    v = torch.randn(nk, Lk, HEADS, d, generator=g) * (0.5 + 1.5 * torch.rand(HEADS, generator=g))[None, None, :, None]
    rd = math.sqrt(d)
    if regime in ("shift_up", "shift_down"):
        a = math.sqrt(SHIFT * rd)
        q[..., 0] = a
        k[..., 0] = a if regime == "shift_up" else -a
    elif regime.startswith("peak"):
        height = PEAK if kernel == "t2i" else TOKEN_PEAK
        a = math.sqrt(height * rd)
        q[..., 0] = a
        k[..., 0] = 0.0
        first = case["peaks"][0]
        k[:, first, :, 0] = a
        for other in case["peaks"][1:]:          # the same key but for PEAK_GAP: the peaks' scores differ by exactly that, in every row
            k[:, other] = k[:, first]
            k[:, other, :, 0] = a - PEAK_GAP * rd / a
    return q.contiguous(), k.contiguous(), v.contiguous(), slots


def _gather(case, q, k, v, slots):
    """per prompt: q [P, Lq, H, d], k, v [P, Lk, H, d]"""
    idx = torch.tensor(slots)
    return (q[idx], k, v) if case["kernel"] == "i2t" else (q, k[idx], v[idx])


def attention_scores(case, q, k, v, slots):
    """fp64 scores [P, H, Lq, Lk]"""
    q, k, _ = _gather(case, q, k, v, slots)
    return torch.einsum("plhd,pshd->phls", q.double(), k.double()) / math.sqrt(q.shape[-1])


def attention_ref(case, q, k, v, slots, dtype=torch.float64):
    """softmax(q k^T / sqrt(d)) v per head -> [P, Lq, H d] in `dtype`"""
    q, k, v = (t.to(dtype) for t in _gather(case, q, k, v, slots))
    s = torch.einsum("plhd,pshd->phls", q, k) / math.sqrt(q.shape[-1])
    return torch.einsum("phls,pshd->plhd", torch.softmax(s, -1), v).reshape(q.shape[0], q.shape[1], -1).contiguous()


ATTENTION_FAULTS = ("no_max", "max_missing_wave_0", "max_missing_wave_1", "max_missing_wave_2", "max_missing_wave_3", "scale",
                    "last_256_keys_dropped", "wrong_slot", "last_token_dropped", "kv_swapped")
LOG2E = 1.4426950408889634


def _fast_exp(x):
    """exp as exp2(x log2 e) with the product rounded to the working precision: what a hardware exp2 path computes"""
    return torch.exp2(x * torch.tensor(LOG2E, dtype=x.dtype))


def _scores_in_order(q, k):
    """[P, H, Lq, Lk]: the dot product summed over d ascending, one product at a time"""
    qh, kh = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3)
    a = torch.zeros(qh.shape[0], qh.shape[1], qh.shape[2], kh.shape[2], dtype=q.dtype)
    for i in range(q.shape[-1]):
        a = a + qh[..., i, None] * kh[..., None, :, i]
    return a


def _wave_sum(x, dim):
    """the xor butterfly over the 64 lanes along `dim` (every lane ends with the sum)"""
    lanes = torch.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x.index_select(dim, lanes ^ o)
    return x


def attention_kernel_order(case, q, k, v, slots, fault=None, dtype=torch.float32):
    """An independent restatement in the kernel's order of summation; `fault`: one of ATTENTION_FAULTS planted."""
    kernel = case["kernel"]
    if fault == "wrong_slot":
        slots = slots[1:] + slots[:1]
    if fault == "kv_swapped":
        k, v = v, k
    q, k, v = (t.to(dtype) for t in _gather(case, q, k, v, slots))
    d = q.shape[-1]
    wrong = fault == "scale"
    if fault == "last_token_dropped" and kernel != "t2i":
        k, v = k[:, :-1], v[:, :-1]
    out = []
    for p in range(q.shape[0]):          # a prompt at a time: the 4 096-key accumulators of a whole chunk are half a gigabyte
        s = _scores_in_order(q[p:p + 1], k[p:p + 1])[0]                     # [H, Lq, Lk]
        if kernel == "self":
            s = s / torch.tensor(math.sqrt(16.0 if wrong else d), dtype=dtype)
        else:
            s = s * torch.tensor(1.0 / math.sqrt(32.0) if wrong else 0.25, dtype=dtype)
        vh = v[p].permute(1, 0, 2)                                           # [H, Lk, d]
        if kernel == "t2i":
            out.append(_t2i_order(s, vh, fault))
            continue
        m = torch.zeros_like(s[..., :1]) if fault == "no_max" else s.max(-1, keepdim=True).values
        e = _fast_exp(s - m)
        l = torch.zeros_like(e[..., 0])
        o = torch.zeros(*e.shape[:2], d, dtype=dtype)
        for j in range(e.shape[-1]):
            l = l + e[..., j]
            o = o + e[..., j, None] * vh[:, None, j]
        out.append((o / l[..., None]).permute(1, 0, 2).reshape(s.shape[1], -1))
    return torch.stack(out).contiguous()


def _t2i_order(s, vh, fault):
    """s [H, T, 4096], vh [H, 4096, d] -> [T, H d]: 16 keys per thread in order, the wave's butterfly, then (w0 + w1) + (w2 + w3)"""
    H, T, _ = s.shape
    d, per, waves = vh.shape[-1], NPIX // THREADS, THREADS // WAVE
    s = s.reshape(H, T, per, waves, WAVE)                                    # key = i * 256 + wave * 64 + lane
    vv = vh.reshape(H, 1, per, waves, WAVE, d)
    if fault == "last_256_keys_dropped":
        s, vv, per = s[:, :, :-1], vv[:, :, :-1], per - 1
    mw = s.max(2).values.max(-1).values                                      # [H, T, waves]: a maximum does not depend on its order
    if fault and fault.startswith("max_missing_wave_"):
        keep = [w for w in range(waves) if w != int(fault[-1])]
        mw = mw[..., keep]
    m = torch.zeros_like(mw[..., :1]) if fault == "no_max" else mw.max(-1, keepdim=True).values
    e = _fast_exp(s - m[..., None, None])
    l = torch.zeros(H, T, waves, WAVE, dtype=s.dtype)
    acc = torch.zeros(H, T, waves, WAVE, d, dtype=s.dtype)
    for i in range(per):
        l = l + e[:, :, i]
        acc = acc + e[:, :, i, :, :, None] * vv[:, :, i]
    l, acc = _wave_sum(l, 3)[..., 0], _wave_sum(acc, 3)[..., 0, :]           # [H, T, waves], [H, T, waves, d]
    lt = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
    at = (acc[..., 0, :] + acc[..., 1, :]) + (acc[..., 2, :] + acc[..., 3, :])
    return (at / lt[..., None]).permute(1, 0, 2).reshape(T, -1)


def i2t_flag_case(s):
    """v beyond the planes range: an output is a convex combination of the v rows, so every output passes PLANES_LIMIT"""
    case = dict(id="i2t-flag", kernel="i2t", regime="unit", T=s.base_tokens + 1, P=2, slots=None, ldk=D, peaks=(), seed=7999)
    q, k, v, slots = attention_inputs(case)
    return case, q, k, 2.0 * PLANES_LIMIT + v.abs(), slots


# ---- the token linear -----------------------------------------------------------------------------------------------------------
LIN_SHAPES = ((768, 256, 512), (768, 256, 0), (128, 256, 128), (256, 128, 0), (2048, 256, 0), (256, 2048, 0), (32, 256, 0),
              (3, 256, 0), (1, 256, 0))        # (N, K, add_cols): the decoder's launches
LIN_PAD = 5                                    # columns of sentinel behind each output row: ldy = N + LIN_PAD
LIN_ADD_BLOCK = 128                            # the "off by one block" of the planted add_cols fault


def linear_rows(s):
    return (1, s.lin_rows - 1, s.lin_rows, s.lin_rows + 1, 2 * s.lin_rows + 1)


def linear_cases(s):
    cases = []
    for M in linear_rows(s):
        for N, K, add_cols in LIN_SHAPES:
            for relu in (False, True):
                for res in (False, True):
                    cases.append(dict(id=f"lin-M{M}-N{N}-K{K}-add{add_cols}" + ("-relu" if relu else "") + ("-res" if res else ""),
                                      M=M, N=N, K=K, add_cols=add_cols, relu=relu, res=res, token=None, T=None,
                                      seed=8000 + len(cases)))
    # the hypernetwork / IoU heads: row i of X is token 1 + t of prompt i, ldx = T * 256
    for t, T in ((0, s.base_tokens), (NMASK - 1, s.max_tokens)):
        cases.append(dict(id=f"lin-strided-T{T}-token{1 + t}", M=s.lin_rows + 1, N=D, K=D, add_cols=0, relu=True, res=False,
                          token=1 + t, T=T, seed=8900 + t))
    return cases


# Every input of the linear lies on a binary grid: X and ADD are multiples of 2^-3 with |X + ADD| <= 6.5, W multiples of 2^-7 with
# |W| <= 1 / 8 (rows of about the 1 / sqrt(K) scale of a trained layer), bias and residual multiples of 2^-4.  A product is then
# a multiple of 2^-10 below 1, and a sum of up to 2 048 of them, in any order and with or without fused multiply-adds, stays
# below 2^24 grid steps: fp32 holds every partial sum exactly.  The reason: the kernel adds its K products in one chain, whose
# fp32 rounding error on random data is about four times that of the blocked sum torch's fp32 matmul makes (16 chains of K / 16,
# measured here at 0.46 to 1.11 of the bound for a correct in-order restatement, whatever K), so on random data MARGIN = 4 would
# judge the order of summation; on the grid the order is out of the picture, e32 is 0, the bound is its floor (four ulps of the
# block's largest output), and what remains is what this kernel can get wrong: rows, columns, pitches and the switches.
_LIN_W = {}


def _grid(t, step, limit):
    return (t / step).round().clamp(-limit / step, limit / step) * step


def linear_weights(N, K):
    """W [N, K], bias [N]: one seeded set per shape, shared by its cases"""
    if (N, K) not in _LIN_W:
        g = _gen(8500 + N + K)
        _LIN_W[(N, K)] = (_grid(torch.randn(N, K, generator=g) / 16.0, 2.0 ** -7, 0.125), _grid(torch.randn(N, generator=g), 2.0 ** -4, 4.0))
    return _LIN_W[(N, K)]


def linear_inputs(case):
    """xbuf (the buffer X lives in), X (the [M, K] rows the kernel reads: a view of xbuf with pitch ldx), ldx, add [M, ldx] or
    None (in [0.5, 2.5], different in every column: a v column reading X + ADD is a gross error), W, bias, res [M, N + LIN_PAD]
    or None"""
    g = _gen(case["seed"])
    M, N, K = case["M"], case["N"], case["K"]
    if case["token"] is None:
        xbuf = _grid(torch.randn(M, K, generator=g), 0.125, 4.0)
        X, ldx = xbuf, K
    else:
        xbuf = _grid(torch.randn(M, case["T"], K, generator=g), 0.125, 4.0)
        X, ldx = xbuf[:, case["token"]], case["T"] * K
    add = None
    if case["add_cols"] > 0:
        add = _grid(0.5 + torch.rand(M, ldx, generator=g) + torch.arange(ldx)[None, :] / ldx, 0.125, 2.5)
    W, bias = linear_weights(N, K)
    res = _grid(torch.randn(M, N + LIN_PAD, generator=g), 2.0 ** -4, 4.0) if case["res"] else None
    return xbuf, X, ldx, add, W, bias, res


LINEAR_FAULTS = ("add_cols_off_by_a_block", "no_relu", "res_pitch")


def linear_ref(case, X, add, W, bias, res, dtype=torch.float64, fault=None, in_order=False):
    """[M, N] in `dtype`.  in_order: the products summed over k ascending from 0, then + bias, ReLU, res + v (the kernel's order)"""
    M, N, K = case["M"], case["N"], case["K"]
    add_cols = case["add_cols"] - (LIN_ADD_BLOCK if fault == "add_cols_off_by_a_block" else 0)
    x, w = X.to(dtype), W.to(dtype)

    def product(xx):
        if not in_order:
            return xx @ w.t()
        acc = torch.zeros(M, N, dtype=dtype)
        for kk in range(K):
            acc = acc + xx[:, kk, None] * w[None, :, kk]
        return acc

    y = product(x)
    if add is not None and add_cols > 0:
        y[:, :add_cols] = product(x + add[:, :K].to(dtype))[:, :add_cols]
    y = y + bias.to(dtype)
    if case["relu"] and fault != "no_relu":
        y = torch.relu(y)
    if res is not None:
        r = res[:, :N]
        if fault == "res_pitch":            # rows of pitch N read from a buffer whose pitch is N + LIN_PAD
            r = res.reshape(-1)[:M * N].reshape(M, N)
        y = r.to(dtype) + y
    return y.contiguous()


def column_block_ratios(got, want64, want32):
    """one ratio per block of 256 columns"""
    return [group_ratio(got[:, c:c + 256].contiguous(), want64[:, c:c + 256].contiguous(), want32[:, c:c + 256].contiguous())
            for c in range(0, got.shape[1], 256)]


# ---- residual + LayerNorm (norm4) and its operands ------------------------------------------------------------------------------
NORM_REGIMES = ("unit", "offset", "tiny")
OFFSET, OFFSET_STD, TINY_STD = 100.0, 0.01, 1e-4


def _regime_rows(g, shape, regime, parts=2):
    """one of `parts` summands of a row: unit randn; OFFSET + OFFSET_STD randn; TINY_STD randn (the variance of the sum)"""
    r = torch.randn(*shape, generator=g) / math.sqrt(parts)
    if regime == "unit":
        return r
    if regime == "offset":
        return OFFSET / parts + OFFSET_STD * r
    return TINY_STD * r


def norm_cases(s):
    cases = [dict(id=f"norm-{regime}-P{P}", regime=regime, P=P, slots=None, seed=9000 + 10 * k + P)
             for k, regime in enumerate(NORM_REGIMES) for P in launch_prompts(s)[:2]]
    cases.append(dict(id=f"norm-unit-P{s.chunk}", regime="unit", P=s.chunk, slots=None, seed=9100))
    cases.append(dict(id="norm-offset-slots", regime="offset", P=len(SLOT_MAP), slots=SLOT_MAP, seed=9101))
    return cases


def norm_inputs(case):
    """res [n, 4096, 256], y [P, 4096, 256] (res + y: the regime's rows), w, b [256], pe_t [4096, 256] (every row its own), slots"""
    g = _gen(case["seed"])
    P = case["P"]
    slots = list(case["slots"]) if case["slots"] else list(range(P))
    n = max(slots) + 1
    res = _regime_rows(g, (n, NPIX, D), case["regime"])
    y = _regime_rows(g, (P, NPIX, D), case["regime"])
    w, b = 1.0 + 0.5 * torch.randn(D, generator=g), 0.5 * torch.randn(D, generator=g)
    pe_t = torch.randn(NPIX, D, generator=g)
    return res, y, w, b, pe_t, slots


NORM_FAULTS = ("one_pass_variance", "no_eps", "pe_of_the_wrong_row", "wrong_slot")


def norm_ref(res, y, w, b, pe_t, slots, dtype=torch.float64, fault=None, in_order=False, eps=TOKEN_EPS):
    """(keys, keys + pe_t) [P, 4096, 256] in `dtype`: mean, then the biased variance of the centred values, as LayerNorm states
    it.  in_order: four columns per lane, the wave's butterfly, times 1 / 256 (the kernel's order)"""
    if fault == "wrong_slot":
        slots = slots[1:] + slots[:1]
    res, y, w, b, pe_t = (t.to(dtype) for t in (res, y, w, b, pe_t))
    x = res[torch.tensor(slots)] + y

    def mean(t):
        if not in_order:
            return t.mean(-1, keepdim=True)
        t = t.reshape(*t.shape[:-1], WAVE, 4)
        return _wave_sum((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3]), t.dim() - 2)[..., :1] * torch.tensor(1.0 / D, dtype=dtype)

    mu = mean(x)
    dd = x - mu
    var = mean(x * x) - mu * mu if fault == "one_pass_variance" else mean(dd * dd)
    rstd = 1.0 / torch.sqrt(var + (0.0 if fault == "no_eps" else torch.tensor(eps, dtype=dtype)))
    keys = (dd * rstd) * w + b
    pe = pe_t.roll(1, 0) if fault == "pe_of_the_wrong_row" else pe_t
    return keys.contiguous(), (keys + pe).contiguous()


def norm_flag_weight(w):
    """a weight that takes column 7 of unit rows beyond the planes range (|LayerNorm| reaches 1 in every row of 256 values)"""
    w = w.clone()
    w[7] = 4.0 * PLANES_LIMIT
    return w


# ---- prepare keys ---------------------------------------------------------------------------------------------------------------
def prep_cases():
    """nz blocks; which of image / dense advances with the block (the other has stride 0)"""
    return [dict(id=f"prep-nz{nz}-{walk}", nz=nz, walk=walk, seed=9500 + nz + 10 * k)
            for k, walk in enumerate(("image", "dense")) for nz in (1, 3)]


def prep_inputs(case):
    """image [nz or 1, 256, 4096], image_pe [256, 4096], dense [1 or nz, 256, 4096] (channel-major)"""
    g = _gen(case["seed"])
    nz = case["nz"]
    image = torch.randn(nz if case["walk"] == "image" else 1, D, NPIX, generator=g)
    dense = torch.randn(nz if case["walk"] == "dense" else 1, D, NPIX, generator=g)
    return image, torch.randn(D, NPIX, generator=g), dense


def prep_ref(image, image_pe, dense, nz):
    """(keys [nz, 4096, 256], pe_t [4096, 256], keys + pe_t) in fp32: one add each, so a correct kernel gives these very bits"""
    keys = (image.expand(nz, -1, -1) + dense.expand(nz, -1, -1)).transpose(1, 2).contiguous()
    pe_t = image_pe.t().contiguous()
    return keys, pe_t, keys + pe_t


# ---- the upscaling tail -----------------------------------------------------------------------------------------------------------
HYPER_GAINS = (1.0, 10.0, 0.1, 100.0)       # per mask: one bound over all masks would let the quiet ones off


def tail_cases():
    combos = (("unit", 1, 0), ("unit", 2, 1), ("offset", 1, 1), ("offset", 2, 0), ("tiny", 2, 1), ("tiny", 1, 0))
    return [dict(id=f"tail-{regime}-P{P}-multimask{mm}", regime=regime, P=P, multimask=mm, seed=9700 + k)
            for k, (regime, P, mm) in enumerate(combos)]


def tail_inputs(case):
    """y [P, 4096, 256] (column tap1 * 64 + channel: each 64 columns are one LayerNorm2d group), ln_w, ln_b [64],
    w3 [64, 32, 2, 2] (torch's ConvTranspose2d weight), b2 [32], hyper [P, 4, 32]"""
    g = _gen(case["seed"])
    P = case["P"]
    y = _regime_rows(g, (P, NPIX, D), case["regime"], parts=1)
    ln_w, ln_b = 1.0 + 0.5 * torch.randn(64, generator=g), 0.5 * torch.randn(64, generator=g)
    w3, b2 = torch.randn(64, 32, 2, 2, generator=g) / 8.0, 0.5 * torch.randn(32, generator=g)
    hyper = torch.randn(P, NMASK, 32, generator=g) * torch.tensor(HYPER_GAINS)[None, :, None]
    return y, ln_w, ln_b, w3, b2, hyper


def tail_w2(w3):
    """the kernel's layout [4 * 32, 64]: row tap * 32 + c (tap = 2 dy + dx), column = input channel"""
    return w3.permute(2, 3, 1, 0).reshape(4 * 32, 64).contiguous()


def tail_pixels(y):
    """[P, 4096, 256] -> [P, 64, 128, 128]: the first ConvTranspose's output as an image (pixel (2 gy + dy, 2 gx + dx), tap1 = 2 dy + dx)"""
    P = y.shape[0]
    return y.reshape(P, GRID, GRID, 2, 2, 64).permute(0, 5, 1, 3, 2, 4).reshape(P, 64, 2 * GRID, 2 * GRID)


TAIL_FAULTS = ("tanh_gelu", "taps_transposed", "m0_ignored", "one_pass_variance", "no_eps")


def tail_ref(case, y, ln_w, ln_b, w3, b2, hyper, dtype=torch.float64, fault=None, in_order=False, eps=UP_EPS):
    """masks [P, C, 256, 256] in `dtype`: LayerNorm2d (common.py), erf-GELU, conv_transpose2d, erf-GELU, hyper @ .
    in_order: the channel sums of mean, variance, the ConvTranspose and the hypernetwork dot one term at a time, ascending"""
    y, ln_w, ln_b, w3, b2, hyper = (t.to(dtype) for t in (y, ln_w, ln_b, w3, b2, hyper))
    x = tail_pixels(y)
    P = x.shape[0]
    gelu = (lambda t: F.gelu(t, approximate="tanh")) if fault == "tanh_gelu" else F.gelu

    def csum(t):          # over the channel axis 1
        if not in_order:
            return t.sum(1, keepdim=True)
        acc = torch.zeros_like(t[:, :1])
        for c in range(t.shape[1]):
            acc = acc + t[:, c:c + 1]
        return acc

    u = csum(x) * torch.tensor(1.0 / 64, dtype=dtype)
    dd = x - u
    var = csum(x * x) / 64 - u * u if fault == "one_pass_variance" else csum(dd * dd) * torch.tensor(1.0 / 64, dtype=dtype)
    x = dd / torch.sqrt(var + (0.0 if fault == "no_eps" else torch.tensor(eps, dtype=dtype)))
    x = gelu(ln_w[None, :, None, None] * x + ln_b[None, :, None, None])
    if fault == "taps_transposed":
        w3 = w3.transpose(2, 3)
    if not in_order:
        x = gelu(F.conv_transpose2d(x, w3, b2, stride=2))
        masks = (hyper @ x.reshape(P, 32, -1)).reshape(P, NMASK, 4 * GRID, 4 * GRID)
    else:
        up = torch.zeros(P, 32, 2 * GRID, 2, 2 * GRID, 2, dtype=dtype)
        for ci in range(64):
            up = up + x[:, ci, None, :, None, :, None] * w3[ci][None, :, None, :, None, :]
        x = gelu(up.reshape(P, 32, 4 * GRID, 4 * GRID) + b2[None, :, None, None])
        masks = torch.zeros(P, NMASK, 4 * GRID, 4 * GRID, dtype=dtype)
        for c in range(32):
            masks = masks + hyper[:, :, c, None, None] * x[:, None, c]
    if not case["multimask"]:
        return masks[:, :1].contiguous()
    return (masks[:, :NMASK - 1] if fault == "m0_ignored" else masks[:, 1:]).contiguous()


def tail_ratios(got, want64, want32):
    """per selected mask, then per (mask, sub-pixel position): C * 17 ratios"""
    ratios = [group_ratio(got[:, m].contiguous(), want64[:, m].contiguous(), want32[:, m].contiguous()) for m in range(got.shape[1])]
    for m in range(got.shape[1]):
        for a in range(4):
            for b in range(4):
                ratios.append(group_ratio(got[:, m, a::4, b::4].contiguous(), want64[:, m, a::4, b::4].contiguous(),
                                          want32[:, m, a::4, b::4].contiguous()))
    return ratios


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def assert_refusals(lib, seams):
    """what the op-level entries refuse, by return code: every call below has one bad argument and returns POPE_ERR_ARG on the
    host (null stream, host memory that is never dereferenced, no launch).  The accepting side of a bound cannot be shown here:
    a call that passes the check launches."""
    import ctypes as C
    L = lib

    def _ints(values):
        return (C.c_int * len(values))(*values)

    buf = C.create_string_buffer(1024)
    ok = (C.addressof(buf) + 255) & ~255               # 256-byte aligned, never dereferenced
    odd = ok + 4
    one, big = _ints([0]), _ints([0] * (seams.chunk + 1))
    neg = _ints([-1])
    T, ch = seams.base_tokens, seams.chunk

    def lin(X=ok, ldx=256, add=None, add_cols=0, W=ok, bias=ok, res=None, Y=ok, ldy=256, M=1, N=256, K=256):
        return L.pope_sam_decoder_token_linear_f32(X, ldx, add, add_cols, W, bias, res, Y, ldy, M, N, K, 0, None)
    for bad in (dict(X=None), dict(W=None), dict(bias=None), dict(Y=None), dict(M=0), dict(N=0), dict(N=-3), dict(K=0), dict(K=254),
                dict(ldx=252), dict(ldy=255), dict(add_cols=-1), dict(W=odd)):
        assert lin(**bad) == -1, bad
    assert lin(K=4100, ldx=4100) == -1                 # lin_rows rows of K floats beyond 64 KiB of LDS
    assert lin(K=2052, ldx=2052, add=ok, add_cols=4) == -1          # ... twice with ADD

    def self_(qkv=ok, out=ok, P=1, T_=T):
        return L.pope_sam_decoder_self_attention_f32(qkv, out, P, T_, None)
    for bad in (dict(qkv=None), dict(out=None), dict(P=0), dict(T_=0), dict(T_=seams.max_tokens + 1)):
        assert self_(**bad) == -1, bad

    def t2i(q=ok, K=ok, ldk=256, kps=NPIX * 256, V=ok, vps=NPIX * 128, slot=one, out=ok, T_=T, P=1):
        return L.pope_sam_decoder_t2i_attention_f32(q, K, ldk, kps, V, vps, slot, out, T_, P, None)
    for bad in (dict(q=None), dict(K=None), dict(V=None), dict(slot=None), dict(out=None), dict(T_=0), dict(T_=seams.max_tokens + 1), dict(P=0),
                dict(P=ch + 1, slot=big), dict(ldk=64), dict(ldk=130), dict(kps=-4), dict(kps=6), dict(vps=2), dict(K=odd), dict(V=odd),
                dict(slot=neg)):
        assert t2i(**bad) == -1, bad

    def i2t(Q=ok, qps=NPIX * 256, slot=one, kv=ok, T_=T, P=1, o32=ok, opl=None):
        return L.pope_sam_decoder_i2t_attention_f32(Q, qps, slot, kv, T_, P, o32, opl, None, None)
    for bad in (dict(Q=None), dict(Q=odd), dict(qps=-4), dict(qps=2), dict(slot=None), dict(slot=neg), dict(kv=None), dict(T_=0),
                dict(T_=seams.max_tokens + 1), dict(P=0), dict(P=ch + 1, slot=big), dict(o32=None, opl=None), dict(o32=ok, opl=ok)):
        assert i2t(**bad) == -1, bad

    def norm(res=ok, rps=NPIX * 256, slot=one, y=ok, w=ok, b=ok, eps=1e-5, pe=ok, keys=ok, opA=ok, opB=ok, f32=0, P=1):
        return L.pope_sam_decoder_residual_norm_f32(res, rps, slot, y, w, b, eps, pe, keys, opA, opB, f32, P, None, None)
    for bad in (dict(res=None), dict(y=None), dict(w=None), dict(b=None), dict(pe=None), dict(keys=None), dict(opB=None), dict(opA=None),
                dict(opB=None, f32=1), dict(res=odd), dict(y=odd), dict(keys=odd), dict(rps=2), dict(rps=-4), dict(slot=None), dict(slot=neg),
                dict(P=0), dict(P=ch + 1, slot=big), dict(eps=-1.0), dict(eps=float("nan"))):
        assert norm(**bad) == -1, bad

    def prep(img=ok, ist=0, pe=ok, dense=ok, ds=0, nz=1, keys=ok, opA=ok, opB=ok, f32=0, pe_t=ok):
        return L.pope_sam_decoder_prepare_keys_f32(img, ist, pe, dense, ds, nz, keys, opA, opB, f32, pe_t, None, None)
    for bad in (dict(img=None), dict(pe=None), dict(dense=None), dict(keys=None), dict(pe_t=None), dict(opB=None), dict(opA=None),
                dict(opB=None, f32=1), dict(ist=-1), dict(ds=-1), dict(nz=0), dict(nz=ch + 1)):
        assert prep(**bad) == -1, bad

    def tail(y=ok, lw=ok, lb=ok, eps=1e-6, w2=ok, b2=ok, hyper=ok, P=1, masks=ok):
        return L.pope_sam_decoder_upscale_tail_f32(y, lw, lb, eps, w2, b2, hyper, 1, P, masks, None)
    for bad in (dict(y=None), dict(lw=None), dict(lb=None), dict(w2=None), dict(b2=None), dict(hyper=None), dict(masks=None), dict(y=odd),
                dict(w2=odd), dict(P=0), dict(P=ch + 1), dict(eps=-1.0)):
        assert tail(**bad) == -1, bad


# ---- the whole decoder ------------------------------------------------------------------------------------------------------------
DECODER_PRECISIONS = ("f16x3", "f32")
DECODER_TENSORS = ("masks", "iou", "hs", "keys")


def decoder_cases(s):
    """P around the prompt chunk, every token count of a point / box prompt and the largest, broadcast and per-prompt dense"""
    c = s.chunk
    shapes = ((c - 1, 0, "broadcast", True), (c, 1, "per_prompt", False), (c + 1, 2, "broadcast", False), (2 * c + 1, 3, "per_prompt", True),
              (c + 1, s.max_tokens - s.base_tokens, "broadcast", True), (c - 1, 1, "broadcast", False))
    return [dict(id=f"decoder-{prec}-P{P}-ns{ns}-{dense}-multimask{int(mm)}", precision=prec, P=P, n_sparse=ns, dense=dense, multimask=mm,
                 seed=9900 + k)
            for prec in DECODER_PRECISIONS for k, (P, ns, dense, mm) in enumerate(shapes)]


def decoder_inputs(case):
    """sparse [P, ns, 256], dense [1 or P, 256, 64, 64] (broadcast: one value per channel, as PromptEncoder's no-mask embedding)"""
    g = _gen(case["seed"])
    P = case["P"]
    sparse = torch.randn(P, case["n_sparse"], D, generator=g)
    if case["dense"] == "broadcast":
        dense = (0.5 * torch.randn(D, generator=g)).reshape(1, D, 1, 1).expand(1, D, GRID, GRID).contiguous()
    else:
        dense = 0.5 * torch.randn(P, D, GRID, GRID, generator=g)
    return sparse, dense


def chunk_ratios(got, want64, want32, chunk):
    """one ratio per chunk of prompts (the leading axis)"""
    return [group_ratio(got[p:p + chunk].contiguous(), want64[p:p + chunk].contiguous(), want32[p:p + chunk].contiguous())
            for p in range(0, got.shape[0], chunk)]


def images_case(s):
    """chunk + 1 images (a second pass of the decoder's image loop), one prompt on the even images and two on the odd ones, in an
    order that is not sorted by image -> (prompt_image list, n_sparse)"""
    n = s.chunk + 1
    which = [i for i in range(n)] + [i for i in range(n - 1, -1, -1) if i % 2 == 1]
    return n, which, 2
