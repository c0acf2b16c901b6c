"""Cases, inputs, fp64 references and the comparison of test_gpu_posehead_routes.py (host only: CPU torch;
test_posehead_checks_cpu.py shows that the inputs discriminate, that the comparison accepts a torch fp32 restatement of every op
and that it rejects the faults these kernels are likely to have, on this very data).

The kernels (csrc/mocope.hip, csrc/pose_regressor.hip, csrc/posereg_tile.h), through their op-level entries:
  mocope_linear     pope_mocope_linear_f32: a wave owns RW = 2 (N <= 1024) or 4 output columns and a chunk of 8 rows; lane l sums the
                    16-byte steps l, l + 64, .. of K; launches of at most MAX_GRID_Y = 65 535 row chunks, A and Y re-based between them
  mocope_attention  pope_mocope_attention_f32: one wave per query row, score g in lane g, p broadcast by a shuffle; G <= 64
  mocope_add_ln     pope_mocope_add_ln_f32: residual + LayerNorm (+ the closing norm) per row by one wave, four rows per workgroup
  mocope_ffn76      pope_mocope_ffn76_f32: the d = 76 FFN + residual + LayerNorm (+ closing norm) of a 32-row tile on the fp32 MFMA
  layer             pope_pose_regressor_layer_f32: one nhead = 2 encoder layer; a workgroup owns T = 32 / G sample slots and all G
                    members of their groups (T G of 32 rows live), from G = 33 one slot on 64-row tiles
  stream_linear     pope_pose_regressor_stream_linear_f32: Linear + LeakyReLU; chunks of 8 rows, a remainder instantiation per
                    1 .. 7 rows, 16-byte loads (K % 4 == 0, aligned operands) or single floats; a wave owns 4 columns, 16 per workgroup
  tail              pope_pose_regressor_tail_f32: mlp.6 .. 18, the heads and convert2matrix, one workgroup per pair

Bound of every comparison (the project's convention): the error against the fp64 reference is at most MARGIN = 4 times the error
of the SAME torch op run in fp32 on the CPU on the same input, max |.| over the output; nothing is taken from the code under
test.  Linears with K <= 4 are the exception: torch's fp32 error can be exactly 0 there, so they are held to ULP_BOUND = 2 ulp of
the fp64 result rounded to fp32.  Their inputs are built so that this is what correct fp32 arithmetic delivers: A in [0.25, 1],
|W| in [0.01, 0.05] with one sign per output column, bias of that sign in [1, 2].  Every term has the column's sign (no
cancellation) and a partial sum stays below 0.2 while 1 <= |result|, so the K roundings of the accumulation cost at most K / 16
ulp of the result and the bias addition half an ulp: 0.75 ulp of the pre-activation.  LeakyReLU's product carries that over at up
to 1.28 times (just above 0.01 an ulp is relatively finer than just above 1), adds half an ulp of its own, and the fp32 value of
0.01 another 0.24: 1.7 ulp from the exact value, which a comparison against the rounded fp64 result (itself within half an ulp)
shows as at most 2.  The pre-activation's sign is the column's: half of them negative.

Attention inputs: q, k, v ~ N(0, 1), then every query row is scaled by the gain at which its largest softmax weight over its group
equals a target drawn from [max(0.2, 1 / G + 0.1), 0.8] (bisection on the fp64 scores; the largest weight grows with the gain), so
no softmax is uniform and none is one-hot, at G = 2 as at G = 64.  The encoder layer gets the same control through its weights:
q of head h reads columns [20 h, 20 h + 20) of x alone (no bias), k reads columns [40, 76), v, out_proj and the FFN are dense; the
gain of row r for head h scales x[r, 20 h : 20 h + 20], which moves that row's scores of that head and nothing else of the
attention.  Elsewhere weights are N(0, 2 / fan_in), biases 0.3 N(0, 1), LayerNorm gains 1 + 0.3 N(0, 1), so pre-activations are
symmetric about 0.

Plants (the reference alone, fp64): the last member of each group dropped from the softmax; members g = (G - 1) // 2 and g + 1
swapped in V; one head instead of two (layer).  Each must move the result by at least PLANT = 100 bounds."""
import functools
import math
import warnings

import torch
import torch.nn.functional as F
from torch import nn

MARGIN = 4.0
ULP_BOUND = 2.0
PLANT = 100.0
SPREAD = (0.15, 0.9)          # the largest softmax weight of every row
SIGN_SHARE = 0.25             # of the pre-activations in front of a ReLU / LeakyReLU, each sign
SIGN_MIN_COUNT = 32           # asserted per case from this many pre-activations on, per family below it
SENTINEL = -1234.5
EPS = 1e-5
D76, HID = 76, 2048
NB, MAX_GRID_Y = 8, 65535     # mocope.hip: rows per chunk, chunks per launch
SEAM_ROW = NB * MAX_GRID_Y    # first row of the second launch
ACT_NONE, ACT_RELU = 0, 1


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _norm_params(g, d):
    return 1.0 + 0.3 * _randn(g, d), 0.3 * _randn(g, d)


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def max_err(got, want64):
    return float((got.detach().cpu().double() - want64).abs().max())


def _spacing(w32):
    a = w32.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def measure(got, want64, want32=None):
    """(error, bound) of a result against the fp64 reference.  want32 is the same torch op in fp32: error = max |got - want64|,
    bound = MARGIN max |want32 - want64|.  want32 None (K <= 4): error in ulp of the fp64 result rounded to fp32, bound ULP_BOUND."""
    got = got.detach().cpu()
    assert got.shape == want64.shape and got.dtype == torch.float32, (got.shape, want64.shape, got.dtype)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), 0.0
    if want32 is None:
        w = want64.float()
        return float(((got.double() - w.double()).abs() / _spacing(w)).max()), ULP_BOUND
    return max_err(got, want64), MARGIN * max_err(want32, want64)


def report(tag, err, bound, own=None):
    """One line per comparison: the measured ratio, beside it the ratio of the fp32 torch op itself (1 / MARGIN by definition
    where the bound comes from it)."""
    ratio = err / bound if bound > 0 else float("inf")
    print(f"{tag}: err {err:.3g} bound {bound:.3g} ratio {ratio:.3f}" + (f" (torch fp32 {own:.3f})" if own is not None else ""))
    return ratio


def moved(a64, b64, want32):
    """By how many bounds two fp64 results differ (plants)."""
    return max_err(a64, b64) / (MARGIN * max_err(want32, a64))


def sign_shares(pre):
    n = pre.numel()
    return float((pre < 0).sum()) / n, float((pre > 0).sum()) / n


# ---- Linears (mocope_linear, stream_linear) -----------------------------------------------------------------------------------
def _lin(name, R, K, N, act, offset=0, seed=None):
    return dict(id=f"{name}-R{R}-K{K}-N{N}-act{act}" + (f"-off{offset}" if offset else ""), R=R, K=K, N=N, act=act, offset=offset, seed=seed)


LINEAR_N = (1, 2, 3, 76, 228, 1023, 1024, 1025, 1027, 2048)
LINEAR_R = (1, 7, 8, 9, 17)
LINEAR_K = (4, 76, 256, 260, 512, 2048)       # 1, 19, 64, 65, 128, 512 16-byte steps over the 64 lanes
LINEAR_CASES = [_lin("lin", R, K, N, act) for N, R, K, act in (
    (1, 1, 4, 0), (2, 7, 76, 1), (3, 8, 256, 0), (76, 9, 260, 1), (228, 17, 512, 0), (1023, 9, 2048, 1), (1024, 9, 256, 0),
    (1025, 9, 260, 1), (1027, 9, 76, 0), (2048, 17, 4, 1), (1, 17, 2048, 1), (2, 8, 512, 0), (3, 9, 4, 1), (76, 1, 76, 0),
    (228, 7, 256, 1), (1023, 9, 4, 0), (1024, 8, 2048, 1), (1025, 9, 512, 0), (1027, 9, 256, 1), (2048, 1, 260, 0),
    (2048, 9, 76, 1), (1024, 17, 260, 0), (1025, 9, 2048, 1), (76, 8, 512, 1))]
SEAM_CASE = _lin("lin-seam", SEAM_ROW + 3, 4, 2, 1)      # 8 MB of input; the second launch serves the last three rows
SEAM_ROWS = (SEAM_ROW - 1, SEAM_ROW, SEAM_ROW + 1, SEAM_ROW + 2)

STREAM_B = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)
STREAM_N = (1, 3, 15, 16, 17, 33)
STREAM_K = (1, 3, 4, 255, 256, 260, 1000)
ACT_LEAKY = 2
STREAM_CASES = [_lin("stream", B, K, N, ACT_LEAKY) for B, K, N in (
    (1, 1, 1), (2, 3, 3), (3, 4, 15), (4, 255, 16), (5, 256, 17), (6, 260, 33), (7, 1000, 1), (8, 1, 3), (9, 3, 15), (16, 4, 16),
    (17, 255, 17), (1, 256, 33), (2, 260, 1), (3, 1000, 3), (4, 1, 15), (5, 3, 16), (6, 4, 17), (7, 255, 33), (8, 256, 1),
    (9, 260, 3), (16, 1000, 15), (17, 1, 16), (1, 3, 17), (2, 4, 33), (9, 256, 17), (9, 1000, 33), (17, 260, 17), (5, 1000, 16),
    (7, 4, 3), (6, 3, 33), (4, 256, 15), (3, 255, 3))]
STREAM_CASES.append(_lin("stream", 9, 256, 17, ACT_LEAKY, offset=1))     # A one float off 16 bytes: the scalar route at a vector-friendly K
STREAM_TWIN = (9, 256, 17)       # served by both routes: aligned A and A one float off


def stream_route(c):
    """pope_launch_posereg_stream_linear restated: (V, full chunks, remainder rows)"""
    return (4 if c["K"] % 4 == 0 and not c["offset"] else 1), c["R"] // 8, c["R"] % 8


def _seed_of(c, cases, base):
    return c["seed"] if c["seed"] is not None else base + [k["id"] for k in cases].index(c["id"])


def linear_inputs(c, seed):
    """A [R, K], W [N, K], bias [N] fp32 (module docstring: K <= 4 without cancellation, else N(0, 1) against N(0, 1 / K))"""
    g = _gen(seed)
    R, K, N = c["R"], c["K"], c["N"]
    if K <= 4:
        sign = torch.where(torch.arange(N) % 2 == 0, -1.0, 1.0)
        A = 0.25 + 0.75 * torch.rand(R, K, generator=g)
        W = sign[:, None] * (0.01 + 0.04 * torch.rand(N, K, generator=g))
        bias = sign * (1.0 + torch.rand(N, generator=g))
    else:
        A, W, bias = _randn(g, R, K), _randn(g, N, K) / math.sqrt(K), 0.3 * _randn(g, N)
    return dict(A=A, W=W, bias=bias)


def activation(pre, act):
    return pre if act == ACT_NONE else F.relu(pre) if act == ACT_RELU else F.leaky_relu(pre, 0.01)


def linear_reference(c, x):
    """dict(want64, want32 (None for K <= 4: the ulp rule), pre: the fp64 pre-activations)"""
    pre = F.linear(x["A"].double(), x["W"].double(), x["bias"].double())
    want32 = None if c["K"] <= 4 else activation(F.linear(x["A"], x["W"], x["bias"]), c["act"])
    return dict(want64=activation(pre, c["act"]), want32=want32, pre=pre)


@functools.lru_cache(maxsize=None)
def _linear_case(cid):
    for cases, base in ((LINEAR_CASES + [SEAM_CASE], 2000), (STREAM_CASES, 3000)):
        for c in cases:
            if c["id"] == cid:
                x = linear_inputs(c, _seed_of(c, cases, base))
                return x, linear_reference(c, x)
    raise KeyError(cid)


def linear_case(c):
    """(inputs, reference) of a mocope_linear / stream_linear case, computed once"""
    return _linear_case(c["id"])


def linear_restated(c, x):
    """fp32 restatement with the kernels' own order for K <= 4 (one lane: the K products in order by fused multiply-add, then
    the bias; fp64 products of fp32 values are exact, so each step is one rounding), torch's fp32 op otherwise"""
    if c["K"] > 4:
        return activation(F.linear(x["A"], x["W"], x["bias"]), c["act"])
    acc = torch.zeros(c["R"], c["N"])
    for k in range(c["K"]):
        acc = (acc.double() + x["A"][:, k, None].double() * x["W"][None, :, k].double()).float()
    pre = acc + x["bias"]
    if c["act"] == ACT_LEAKY:
        return torch.where(pre >= 0, pre, torch.tensor(0.01, dtype=torch.float32) * pre)
    return activation(pre, c["act"])


# ---- attention ------------------------------------------------------------------------------------------------------------------
ATT_D = (76, 512)
ATT_G = (2, 3, 5, 31, 32, 33, 63, 64)
ATT_LAYOUTS = ("self", "cross")


def _att(d, G, q, layout):
    S = 1 if (G + q) % 2 == 0 else 3
    return dict(id=f"att-d{d}-G{G}-q{q}-S{S}-{layout}", d=d, G=G, q=q, S=S, R=q * G * S, layout=layout)


ATTENTION_CASES = [_att(d, G, q, layout) for d in ATT_D for G in ATT_G for q in ((1,) if G >= 63 else (1, 2, 3)) for layout in ATT_LAYOUTS]


def row_gain(base, target):
    """base [.., G] fp64 scores of a row at gain 1, target [..]: the gain at which the row's largest softmax weight is the target"""
    peak = lambda a: torch.softmax(a[..., None] * base, -1).amax(-1)  # noqa: E731
    lo, hi = torch.zeros_like(target), torch.ones_like(target)
    for _ in range(40):
        if bool((peak(hi) >= target).all()):
            break
        hi = hi * 2
    assert bool((peak(hi) >= target).all())
    for _ in range(60):
        mid = (lo + hi) / 2
        under = peak(mid) < target
        lo, hi = torch.where(under, mid, lo), torch.where(under, hi, mid)
    return (lo + hi) / 2


def _targets(g, shape, G):
    lo = max(0.2, 1.0 / G + 0.1)
    return (lo + (0.8 - lo) * torch.rand(*shape, generator=g)).double()


def grouped(t, S, G):
    """[R, c] rows b * S + s -> [Q, S, G, c]: the G members of a group side by side"""
    R, c = t.shape
    return t.view(R // (S * G), G, S, c).permute(0, 2, 1, 3)


def ungrouped(t):
    Q, S, G, c = t.shape
    return t.permute(0, 2, 1, 3).reshape(Q * G * S, c)


def swap_perm(G):
    g = (G - 1) // 2
    perm = list(range(G))
    perm[g], perm[g + 1] = perm[g + 1], perm[g]
    return perm


def attention_ref(q, k, v, S, G, drop_last=False, swap=False):
    """softmax(q k^T / sqrt(d)) v over the members of a group, in the dtype of the inputs: (out [R, d], weights [Q, S, G, G])"""
    d = q.shape[1]
    sc = grouped(q, S, G) @ grouped(k, S, G).transpose(-1, -2) / math.sqrt(d)
    if drop_last:
        sc = sc.clone()
        sc[..., -1] = -math.inf
    p = torch.softmax(sc, -1)
    vv = grouped(v, S, G)
    if swap:
        vv = vv[:, :, swap_perm(G)]
    return ungrouped(p @ vv), p


def attention_inputs(c, seed):
    g = _gen(seed)
    R, d, S, G = c["R"], c["d"], c["S"], c["G"]
    q, k, v = _randn(g, R, d), _randn(g, R, d), _randn(g, R, d)
    base = grouped(q.double(), S, G) @ grouped(k.double(), S, G).transpose(-1, -2) / math.sqrt(d)
    gain = row_gain(base, _targets(g, base.shape[:-1], G))          # [Q, S, G]
    q = (q.double() * ungrouped(gain[..., None])).float()
    return dict(q=q, k=k, v=v)


def attention_buffers(c, x):
    """The op's operands as the two callers lay them out: ((Q, ldq), (K, ldk), (V, ldv)) as views of the buffers to upload.
    self: q | k | v are the thirds of one [R, 3 d] buffer; cross: q [R, d], k | v the halves of a separate memory buffer [R, 2 d]"""
    d = c["d"]
    if c["layout"] == "self":
        buf = torch.cat([x["q"], x["k"], x["v"]], 1).contiguous()
        return [buf], ((0, 0, 3 * d), (0, d, 3 * d), (0, 2 * d, 3 * d))
    return [x["q"].contiguous(), torch.cat([x["k"], x["v"]], 1).contiguous()], ((0, 0, d), (1, 0, 2 * d), (1, d, 2 * d))


@functools.lru_cache(maxsize=None)
def _attention_case(d, G, q, S):
    c = dict(d=d, G=G, q=q, S=S, R=q * G * S)
    x = attention_inputs(c, 4000 + 7 * d + 100 * G + q)
    dbl = [x[n].double() for n in "qkv"]
    want64, p = attention_ref(*dbl, S, G)
    return x, dict(want64=want64, want32=attention_ref(x["q"], x["k"], x["v"], S, G)[0], weights=p,
                   drop64=attention_ref(*dbl, S, G, drop_last=True)[0], swap64=attention_ref(*dbl, S, G, swap=True)[0])


def attention_case(c):
    """(inputs, reference) — the two layouts of a shape share both"""
    return _attention_case(c["d"], c["G"], c["q"], c["S"])


# ---- add_ln, ffn76 --------------------------------------------------------------------------------------------------------------
ADD_LN_CASES = [dict(id=f"addln-d{d}-R{R}-{'closing' if closing else 'plain'}", d=d, R=R, closing=closing)
                for d in (76, 512) for R in (1, 3, 4, 5, 130) for closing in (False, True)]
FFN76_CASES = [dict(id=f"ffn76-R{R}-{'closing' if closing else 'plain'}", R=R, closing=closing)
               for R in (1, 31, 32, 33, 65) for closing in (False, True)]


def add_ln_ref(x, closing=True):
    """LayerNorm(X + Y) (+ the closing norm) in the dtype of x"""
    d = x["X"].shape[1]
    out = F.layer_norm(x["X"] + x["Y"], (d,), x["w1"], x["b1"], EPS)
    return F.layer_norm(out, (d,), x["w2"], x["b2"], EPS) if closing else out


@functools.lru_cache(maxsize=None)
def _add_ln_case(d, R, closing):
    g = _gen(5000 + d + 10 * R)
    x = dict(X=_randn(g, R, d), Y=_randn(g, R, d))
    x["w1"], x["b1"] = _norm_params(g, d)
    x["w2"], x["b2"] = _norm_params(g, d)
    x64 = {k: v.double() for k, v in x.items()}
    return x, dict(want64=add_ln_ref(x64, closing), want32=add_ln_ref(x, closing))


def add_ln_case(c):
    return _add_ln_case(c["d"], c["R"], c["closing"])


def ffn_weights(g, d=D76):
    w = dict(l1w=_randn(g, HID, d) * math.sqrt(2.0 / d), l1b=0.3 * _randn(g, HID), l2w=_randn(g, d, HID) * math.sqrt(2.0 / HID),
             l2b=0.3 * _randn(g, d))
    w["nw"], w["nb"] = _norm_params(g, d)
    w["fw"], w["fb"] = _norm_params(g, d)
    return w


def ffn76_ref(x, closing=True, relu=True):
    """(LayerNorm(X + linear2(relu(linear1(X)))) (+ the closing norm), the pre-activations) in the dtype of x"""
    pre = F.linear(x["X"], x["l1w"], x["l1b"])
    out = F.layer_norm(x["X"] + F.linear(F.relu(pre) if relu else pre, x["l2w"], x["l2b"]), (D76,), x["nw"], x["nb"], EPS)
    return (F.layer_norm(out, (D76,), x["fw"], x["fb"], EPS) if closing else out), pre


@functools.lru_cache(maxsize=None)
def _ffn76_case(R, closing):
    g = _gen(6000 + R)
    x = dict(X=_randn(g, R, D76), **ffn_weights(g))
    x64 = {k: v.double() for k, v in x.items()}
    want64, pre = ffn76_ref(x64, closing)
    return x, dict(want64=want64, want32=ffn76_ref(x, closing)[0], pre=pre)


def ffn76_case(c):
    return _ffn76_case(c["R"], c["closing"])


# ---- the nhead = 2 encoder layer ----------------------------------------------------------------------------------------------
LAYER_GBS = ((1, 3, 5), (2, 4, 9), (3, 6, 7), (5, 10, 7), (7, 7, 5), (16, 32, 3), (31, 31, 2), (32, 64, 2), (33, 33, 2), (64, 64, 3),
             (33, 66, 1))
LAYER_CASES = [dict(id=f"layer-G{G}-B{B}-S{S}", G=G, B=B, S=S) for G, B, S in LAYER_GBS]
HD, QBLK, KCOL = 38, 20, 40      # head width; columns of x a head's q reads; first column k reads
LAYER_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
              "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
              "norm2.bias")


def layer_route(c):
    """pope_launch_posereg_layer restated: (row blocks RB, slots per tile T, live rows of a full tile, tiles, slots in the last)"""
    NU = c["B"] // c["G"] * c["S"]
    if c["G"] > 32:
        return 2, 1, c["G"], NU, 1
    T = 32 // c["G"]
    return 1, T, T * c["G"], -(-NU // T), NU - (NU - 1) // T * T


def layer_weights(g):
    """State dict of nn.TransformerEncoderLayer(76, 2, 2048) with the q / k column blocks of the module docstring"""
    wq = torch.zeros(D76, D76)
    for h in range(2):
        wq[h * HD:(h + 1) * HD, h * QBLK:(h + 1) * QBLK] = _randn(g, HD, QBLK) / math.sqrt(QBLK)
    wk = torch.zeros(D76, D76)
    wk[:, KCOL:] = _randn(g, D76, D76 - KCOL) / math.sqrt(D76 - KCOL)
    wv = _randn(g, D76, D76) * math.sqrt(2.0 / D76)
    f = ffn_weights(g)
    sd = {"self_attn.in_proj_weight": torch.cat([wq, wk, wv]),
          "self_attn.in_proj_bias": torch.cat([torch.zeros(D76), 0.3 * _randn(g, 2 * D76)]),
          "self_attn.out_proj.weight": _randn(g, D76, D76) * math.sqrt(2.0 / D76), "self_attn.out_proj.bias": 0.3 * _randn(g, D76),
          "linear1.weight": f["l1w"], "linear1.bias": f["l1b"], "linear2.weight": f["l2w"], "linear2.bias": f["l2b"],
          "norm1.weight": f["nw"], "norm1.bias": f["nb"], "norm2.weight": f["fw"], "norm2.bias": f["fb"]}
    return {k: sd[k].contiguous() for k in LAYER_KEYS}


def to_seq(X, G):
    """[B, S, d] -> [G, Q S, d]: batch_first=False input with the groups of a call as batch entries"""
    B, S, d = X.shape
    return X.view(B // G, G, S, d).permute(1, 0, 2, 3).reshape(G, B // G * S, d)


def from_seq(Y, B, S):
    G, _, d = Y.shape
    return Y.view(G, B // G, S, d).permute(1, 0, 2, 3).reshape(B, S, d)


def layer_module(sd, dtype, nhead=2):
    m = nn.TransformerEncoderLayer(D76, nhead, HID, dropout=0.0, batch_first=False)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype).eval()


def layer_restated(sd, x, nhead=2, drop_last=False, swap=False, relu=True):
    """The layer written out (post-norm, ReLU, eps 1e-5) on x [G, N, 76] in the dtype of sd: (out, softmax weights [N, nhead, G, G],
    FFN pre-activations)"""
    G, N, D = x.shape
    hd = D // nhead
    q, k, v = F.linear(x, sd["self_attn.in_proj_weight"], sd["self_attn.in_proj_bias"]).split(D, -1)
    heads = lambda t: t.reshape(G, N, nhead, hd).permute(1, 2, 0, 3)  # noqa: E731
    sc = heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(hd)
    if drop_last:
        sc = sc.clone()
        sc[..., -1] = -math.inf
    p = torch.softmax(sc, -1)
    vv = heads(v)
    if swap:
        vv = vv[:, :, swap_perm(G)]
    o = (p @ vv).permute(2, 0, 1, 3).reshape(G, N, D)
    x = F.layer_norm(x + F.linear(o, sd["self_attn.out_proj.weight"], sd["self_attn.out_proj.bias"]), (D,), sd["norm1.weight"],
                     sd["norm1.bias"], EPS)
    pre = F.linear(x, sd["linear1.weight"], sd["linear1.bias"])
    h = F.linear(F.relu(pre) if relu else pre, sd["linear2.weight"], sd["linear2.bias"])
    return F.layer_norm(x + h, (D,), sd["norm2.weight"], sd["norm2.bias"], EPS), p, pre


def layer_inputs(c, seed):
    g = _gen(seed)
    G, B, S = c["G"], c["B"], c["S"]
    sd = layer_weights(g)
    X = _randn(g, B, S, D76)
    if G > 1:
        xs = to_seq(X.double(), G)                       # [G, N, 76]
        w, b = sd["self_attn.in_proj_weight"].double(), sd["self_attn.in_proj_bias"].double()
        k = F.linear(xs, w[D76:2 * D76], b[D76:2 * D76])
        for h in range(2):
            cols = slice(h * QBLK, (h + 1) * QBLK)
            qh = F.linear(xs[..., cols], w[h * HD:(h + 1) * HD, cols])              # [G, N, 38]
            base = qh.permute(1, 0, 2) @ k[..., h * HD:(h + 1) * HD].permute(1, 2, 0) / math.sqrt(HD)      # [N, G, G]
            gain = row_gain(base, _targets(g, base.shape[:-1], G))                  # [N, G]
            xs[..., cols] = xs[..., cols] * gain.t()[..., None]
        X = from_seq(xs, B, S).float()
    return dict(X=X.contiguous(), sd=sd)


@functools.lru_cache(maxsize=None)
def _layer_case(G, B, S):
    c = dict(G=G, B=B, S=S)
    x = layer_inputs(c, 7000 + 100 * G + B)
    sd64 = {k: v.double() for k, v in x["sd"].items()}
    with torch.no_grad():
        xs = to_seq(x["X"], G)
        want64 = from_seq(layer_module(x["sd"], torch.float64)(xs.double()), B, S)
        want32 = from_seq(layer_module(x["sd"], torch.float32)(xs), B, S)
        again, p, pre = layer_restated(sd64, xs.double())
        ref = dict(want64=want64, want32=want32, weights=p, pre=pre, restated64=from_seq(again, B, S))
        if G > 1:
            ref["drop64"] = from_seq(layer_restated(sd64, xs.double(), drop_last=True)[0], B, S)
            ref["swap64"] = from_seq(layer_restated(sd64, xs.double(), swap=True)[0], B, S)
            ref["head64"] = from_seq(layer_module(x["sd"], torch.float64, nhead=1)(xs.double()), B, S)
    return x, ref


def layer_case(c):
    return _layer_case(c["G"], c["B"], c["S"])


# ---- tail ---------------------------------------------------------------------------------------------------------------------
MODES = {"matrix": (0, 9), "quat": (1, 4), "6d": (2, 6)}       # POPE_ROT_*: (code, width of the rotation head)
TAIL_B = 3
TAIL_CASES = [dict(id=f"tail-S{S}-{mode}", S=S, mode=mode, status=(0, 0, 0)) for S, mode in
              ((1, "6d"), (63, "6d"), (64, "6d"), (65, "6d"), (512, "6d"), (64, "matrix"), (64, "quat"))]
TAIL_STATUS_CASE = dict(id="tail-S64-6d-refused", S=64, mode="6d", status=(0, -2, 0))
TAIL_WIDTHS = (256, 128, 64, 32, 32)      # mlp.6 .. mlp.18


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-8)


def rot_to_matrix(mode, r):
    """csrc/rot_convert.h (the fork's convert2matrix) restated on [B, 9 | 4 | 6] in the dtype of r -> [B, 9] row-major"""
    if mode == "matrix":
        return r
    if mode == "quat":
        qw, qx, qy, qz = _unit(r).unbind(-1)
        xx, yy, zz, xy, xz, yz, xw, yw, zw = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qx * qw, qy * qw, qz * qw
        return torch.stack([1 - 2 * yy - 2 * zz, 2 * xy - 2 * zw, 2 * xz + 2 * yw, 2 * xy + 2 * zw, 1 - 2 * xx - 2 * zz, 2 * yz - 2 * xw,
                            2 * xz - 2 * yw, 2 * yz + 2 * xw, 1 - 2 * xx - 2 * yy], -1)
    x = _unit(r[:, :3])
    z = _unit(torch.linalg.cross(x, r[:, 3:]))
    y = torch.linalg.cross(z, x)
    return torch.stack([x, y, z], -1).reshape(-1, 9)           # x, y, z are the columns


def tail_ref(x, mode, leaky=True):
    """(trans [B, 3], rot [B, 9], pre-activations) of the chain in the dtype of x"""
    h, pres = x["Y2"], []
    for i in range(5):
        pre = F.linear(h, x[f"w{i}"], x[f"b{i}"])
        pres.append(pre.flatten())
        h = F.leaky_relu(pre, 0.01) if leaky else pre
    return F.linear(h, x["trans_w"], x["trans_b"]), rot_to_matrix(mode, F.linear(h, x["rot_w"], x["rot_b"])), torch.cat(pres)


@functools.lru_cache(maxsize=None)
def _tail_case(S, mode):
    g = _gen(8000 + S + 1000 * MODES[mode][0])
    x = dict(Y2=_randn(g, TAIL_B, S))
    widths = (S,) + TAIL_WIDTHS
    for i in range(5):
        x[f"w{i}"], x[f"b{i}"] = _randn(g, widths[i + 1], widths[i]) * math.sqrt(2.0 / widths[i]), 0.3 * _randn(g, widths[i + 1])
    x["trans_w"], x["trans_b"] = _randn(g, 3, 32) * math.sqrt(2.0 / 32), 0.3 * _randn(g, 3)
    x["rot_w"], x["rot_b"] = _randn(g, MODES[mode][1], 32) * math.sqrt(2.0 / 32), 0.3 * _randn(g, MODES[mode][1])
    t64, r64, pre = tail_ref({k: v.double() for k, v in x.items()}, mode)
    t32, r32, _ = tail_ref(x, mode)
    return x, dict(t64=t64, r64=r64, t32=t32, r32=r32, pre=pre)


def tail_case(c):
    return _tail_case(c["S"], c["mode"])


# ---- the whole nn.Transformer under groupings the callers never use -----------------------------------------------------------
XFMR_S = 5
XFMR_BG = ((6, 3), (6, 1), (64, 32))
# tap under test -> (transformer, d, the taps that feed it as (src, tgt), what of the result the tap is)
XFMR_TAPS = {"memory": ("transformer_mkpts", 76, ("embedding", "embedding"), "memory"),
             "transformer_mkpts": ("transformer_mkpts", 76, ("embedding", "embedding"), "out"),
             "qmkpts": ("mkpts_as_q", 512, ("x_img", "x_mkpts"), "out"),
             "qimg": ("cnn_as_q", 512, ("x_mkpts", "x_img"), "out")}


def load_transformer(sd, prefix, d, dtype):
    """nn.Transformer(d, 1, 6, 6, 2048) with the model's own tensors `prefix.*`, eval, dropout 0, batch_first=False"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        t = nn.Transformer(d_model=d, nhead=1, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=HID, dropout=0.0)
    t.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}, strict=True)
    return t.to(dtype).eval()


@torch.no_grad()
def run_grouped(t, src, tgt, G):
    """src, tgt [B, S, d] in the dtype of t, groups of G consecutive b: (memory, out) [B, S, d].  The groups ride the batch
    dimension of one call: batch entries do not meet anywhere in nn.Transformer, so this is the run group by group."""
    B, S, _ = src.shape
    mem = t.encoder(to_seq(src, G))
    out = t.decoder(to_seq(tgt, G), mem)
    return dict(memory=from_seq(mem, B, S), out=from_seq(out, B, S))


# ---- argument refusals of the op-level entries ----------------------------------------------------------------------------------
def argument_refusals(lib):
    """[(what, status)] of calls every one of which must come back POPE_ERR_ARG (-1) before any HIP call: the pointers are
    16-byte aligned host addresses that are never dereferenced"""
    import ctypes as C

    from pope_amd import _lib
    buf = C.create_string_buffer(64)
    ok = (C.addressof(buf) + 15) & ~15
    out = []
    lin = lambda **kw: lib.pope_mocope_linear_f32(*[kw.get(k, v) for k, v in (("A", ok), ("W", ok), ("bias", ok), ("Y", ok), ("R", 8), ("K", 76),  # noqa: E731
                                                                              ("N", 4), ("act", 0))], None)
    for kw in (dict(A=None), dict(W=None), dict(bias=None), dict(Y=None), dict(R=0), dict(K=0), dict(K=3), dict(K=78), dict(K=-4), dict(N=0),
               dict(act=2), dict(act=-1), dict(A=ok + 4), dict(W=ok + 8)):
        out.append((f"mocope_linear {kw}", lin(**kw)))
    att = lambda **kw: lib.pope_mocope_attention_f32(*[kw.get(k, v) for k, v in (("Q", ok), ("ldq", 76), ("K", ok), ("ldk", 152), ("V", ok),  # noqa: E731
                                                                                 ("ldv", 152), ("O", ok), ("R", 12), ("S", 2), ("G", 3), ("d", 76))], None)
    for kw in (dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(d=64), dict(d=0), dict(d=1024), dict(G=0), dict(G=65), dict(G=-1),
               dict(R=0), dict(S=0), dict(R=13), dict(G=4), dict(ldq=75), dict(ldk=0), dict(ldv=-76), dict(d=512)):
        out.append((f"mocope_attention {kw}", att(**kw)))
    aln = lambda **kw: lib.pope_mocope_add_ln_f32(*[kw.get(k, v) for k, v in (("X", ok), ("Y", ok), ("w1", ok), ("b1", ok), ("w2", None),  # noqa: E731
                                                                              ("b2", None), ("R", 3), ("d", 76))], None)
    for kw in (dict(X=None), dict(Y=None), dict(w1=None), dict(b1=None), dict(w2=ok), dict(b2=ok), dict(R=0), dict(d=77), dict(d=256)):
        out.append((f"mocope_add_ln {kw}", aln(**kw)))
    names = ("X", "l1w", "l1b", "l2w", "l2b", "nw", "nb")
    ffn = lambda **kw: lib.pope_mocope_ffn76_f32(*[kw.get(k, ok) for k in names], kw.get("fw"), kw.get("fb"), kw.get("R", 5), None)  # noqa: E731
    for kw in [{n: None} for n in names] + [dict(fw=ok), dict(fb=ok), dict(R=0), dict(l1w=ok + 4), dict(l2w=ok + 8), dict(l1b=ok + 4)]:
        out.append((f"mocope_ffn76 {kw}", ffn(**kw)))
    layer = _lib.PoseRegressorLayer(*([ok] * 12))
    lay = lambda w=layer, X=ok, B=6, S=2, G=3: lib.pope_pose_regressor_layer_f32(C.byref(w) if w is not None else None, X, B, S, G, None)  # noqa: E731
    holed, skewed = _lib.PoseRegressorLayer(*([ok] * 12)), _lib.PoseRegressorLayer(*([ok] * 12))
    holed.norm2_b, skewed.linear2_w = None, ok + 4
    for what, st in (("w", lay(w=None)), ("X", lay(X=None)), ("B 0", lay(B=0)), ("S 0", lay(S=0)), ("G 0", lay(G=0)), ("G 65", lay(B=65, G=65)),
                     ("B % G", lay(B=7)), ("null weight", lay(w=holed)), ("misaligned weight", lay(w=skewed))):
        out.append((f"layer {what}", st))
    stl = lambda A=ok, W=ok, bias=ok, Y=ok, B=2, K=8, N=3: lib.pope_pose_regressor_stream_linear_f32(A, W, bias, Y, B, K, N, None)  # noqa: E731
    for what, st in (("A", stl(A=None)), ("W", stl(W=None)), ("bias", stl(bias=None)), ("Y", stl(Y=None)), ("B", stl(B=0)), ("K", stl(K=0)),
                     ("N", stl(N=-1))):
        out.append((f"stream_linear {what}", st))

    def tail(edit=None, **kw):
        w = _lib.PoseRegressorWeights()
        w.num_sample, w.mode = 64, 2
        for i in range(2, 7):
            w.mlp_w[i], w.mlp_b[i] = ok, ok
        w.trans_w = w.trans_b = w.rot_w = w.rot_b = ok
        if edit:
            edit(w)
        args = dict(dict(Y2=ok, status=ok, B=3, trans=ok, rot=ok), **kw)
        return lib.pope_pose_regressor_tail_f32(C.byref(w), args["Y2"], args["status"], args["B"], args["trans"], args["rot"], None)

    out.append(("tail w", lib.pope_pose_regressor_tail_f32(None, ok, ok, 3, ok, ok, None)))
    for what, st in (("Y2", tail(Y2=None)), ("status", tail(status=None)), ("trans", tail(trans=None)), ("rot", tail(rot=None)), ("B", tail(B=0)),
                     ("num_sample", tail(lambda w: setattr(w, "num_sample", 0))), ("mode", tail(lambda w: setattr(w, "mode", 3))),
                     ("mlp_w", tail(lambda w: w.mlp_w.__setitem__(4, None))), ("rot_b", tail(lambda w: setattr(w, "rot_b", None)))):
        out.append((f"tail {what}", st))
    return out
