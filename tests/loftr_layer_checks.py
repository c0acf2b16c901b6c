"""Cases, inputs, fp64 references and the comparison of test_gpu_loftr_layer_routes.py (host only: CPU torch;
test_loftr_layer_checks_cpu.py shows that the case lists hold every seam value, that the inputs reach the regime each case is
about, that the comparison accepts a torch fp32 restatement summing in the kernels' order and that it rejects the faults these
kernels are likely to have, on this very data).

The kernels, through their entries:
  attention   pope_loftr_linear_attention_f32 (csrc/loftr.hip: linattn_reduce_kernel, linattn_finish_kernel,
              linattn_apply_kernel): the per-head D x D state is summed over the source rows in chunks of c rows, the chunk
              partials in chunk order, and a workgroup of the message kernel serves r query rows, 256 / C of them per pass;
              c and r are read from pope_loftr_linear_attention_seams, never written here as literals
  layer       pope_loftr_encoder_layer_f32 (with and without masks) through LoFTREncoderLayer.update_: the same attention between five
              GEMMs, ln_cat_planes_kernel and ln_add_kernel
  fine match  pope_fine_match_f32 without and with scale1 (csrc/fine.hip: fine_match_kernel, four matches per workgroup)
  fine pre    pope_fine_preprocess_f32 (fine_gather_coarse_kernel, fine_gather_windows_kernel, two GEMMs)

Comparison of one GROUP of outputs (the project's convention, MARGIN = 4, plus a floor):
    max |gpu - fp64| <= MARGIN * max(e32, 2^-23 * max |fp64|)
e32 = max |fp32 - fp64| of the same torch restatement evaluated in fp32 on the same inputs; the floor, one fp32 ulp of the
group's largest value, keeps a group whose fp32 restatement happens to round luckily from demanding more than fp32 can give.
Groups: one per head for the attention entry (the strongly negative head's e32 is a hundred times that of the others: one
bound over all heads would let seven of them off), one per output tensor for the layer and the fine preprocess, one per
published column (x, y, spread, both axes of mkpts1_f) for the fine matching.  Nothing here is taken from the code under test.

References: oracle/loftr_ref.py (linear_attention, encoder_layer, fine_matching, fine_preprocess) evaluated in fp64, and the
masked restatements below, which multiply Q by the query mask and K and V by the source mask before the sums
(linear_attention.py:35-41) and equal the oracle's functions without masks (asserted by the CPU test).

Attention inputs: head h of q and k is scale_h randn + shift_h with seeded scale_h in [0.5, 2] and shift_h in [-1, 1]; head
NEG_HEAD is -10 + 0.5 randn in both: there elu's negative branch carries the value (exp(x) - 1 + 1 keeps three digits) and the
denominator Q . Ksum is comparable with eps = 1e-6.  v is randn times a seeded per-head gain.

A fine-match case is one (window side, C, heatmap kind, entry); it is LAUNCHED once per M in FINE_M (1, 4 and 5 matches: four
per workgroup) on different data, and the columns of the three launches form the case's groups: a group of the single value that
M = 1 publishes per column would be judged against the luck of one fp32 rounding."""
import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import loftr_ref

MARGIN = 4.0
ULP = 2.0 ** -23
EPS = 1e-6
NHEAD = 8
NEG_HEAD = 5
SENTINEL = -1234.5
PLANES_LIMIT = 65504.0 / 8.0       # |message| from which the planes output must raise the range flag
VAR_FLOOR = 1e-3                   # fp64 variance per axis of every case that checks the spread
SPREAD_CLAMP = 2e-5 * (1 - 1e-3)   # sqrt(1e-10) per axis: the reference's clamp, less a thousandth


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def group_ratio(got, want64, want32, scale=None):
    """error / bound of one group.  scale: the magnitude the floor's ulp refers to (default: max |want64|)."""
    got = got.detach().cpu()
    assert got.shape == want64.shape == want32.shape, (got.shape, want64.shape, want32.shape)
    assert got.dtype == torch.float32 and want32.dtype == torch.float32 and want64.dtype == torch.float64
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = float((got.double() - want64).abs().max())
    e32 = float((want32.double() - want64).abs().max())
    bound = MARGIN * max(e32, ULP * (float(want64.abs().max()) if scale is None else scale))
    if err == 0.0:
        return 0.0
    return err / bound if bound > 0 else float("inf")


def head_groups(t, nhead=NHEAD):
    """[n, L, C] -> nhead tensors [n, L, D]"""
    n, L, Cd = t.shape
    return list(t.reshape(n, L, nhead, Cd // nhead).unbind(2))


def head_ratios(got, want64, want32):
    return [group_ratio(g, w, s) for g, w, s in zip(head_groups(got), head_groups(want64), head_groups(want32))]


def report(tag, ratios):
    worst = max(ratios)
    print(f"{tag}: ratio " + " ".join(f"{r:.3f}" for r in ratios) + f" worst {worst:.3f}")
    return worst


# ---- linear attention -------------------------------------------------------------------------------------------------------
def attention_lengths(c, r):
    """(S values, L values) at the seams c (reduction chunk) and r (rows per message workgroup)"""
    return (1, c - 1, c, c + 1, 2 * c + 1, 3 * c + 8), (1, r - 1, r, r + 1, 2 * r + 1)


def attention_cases(c, r):
    """The smallest L and S paired with each other, a diagonal over the rest, the two extremes; every pair at n = 1 and 3 and at
    both widths.  Masked variants at (r + 1, 2 c + 1), n = 3."""
    Ss, Ls = attention_lengths(c, r)
    pairs = [(Ls[0], Ss[0]), (Ls[1], Ss[1]), (Ls[2], Ss[2]), (Ls[3], Ss[3]), (Ls[4], Ss[4]), (Ls[3], Ss[5]),
             (Ls[0], Ss[5]), (Ls[4], Ss[0])]
    cases = []
    for Cd in (256, 128):
        for k, (L, S) in enumerate(pairs):
            for n in (1, 3):
                cases.append(dict(id=f"attn-C{Cd}-n{n}-L{L}-S{S}", C=Cd, n=n, L=L, S=S, mask=None, seed=1000 + 10 * k + n + Cd))
        for k, mask in enumerate(MASK_KINDS):
            cases.append(dict(id=f"attn-C{Cd}-n3-L{r + 1}-S{2 * c + 1}-{mask}", C=Cd, n=3, L=r + 1, S=2 * c + 1, mask=mask,
                              seed=2000 + k + Cd))
    return cases


MASK_KINDS = ("qmask", "kvmask", "both", "kvtail", "image")
MASKED_IMAGE = 1      # "image": the whole source of this image is masked


def attention_inputs(case, c):
    """q [n, L, C], kv [n, S, 2C] (k | v), q_mask [n, L] or None, kv_mask [n, S] or None (fp32 0 / 1)"""
    g = _gen(case["seed"])
    n, L, S, Cd = case["n"], case["L"], case["S"], case["C"]
    D = Cd // NHEAD
    scale = 0.5 + 1.5 * torch.rand(NHEAD, generator=g)
    shift = 2.0 * torch.rand(NHEAD, generator=g) - 1.0
    scale[NEG_HEAD], shift[NEG_HEAD] = 0.5, -10.0
    vgain = 0.5 + 1.5 * torch.rand(NHEAD, generator=g)

    def heads(rows, sc, sh):
        return (torch.randn(n, rows, NHEAD, D, generator=g) * sc[None, None, :, None] + sh[None, None, :, None]).reshape(n, rows, Cd)

    q = heads(L, scale, shift)
    k = heads(S, scale, shift)
    v = heads(S, vgain, torch.zeros(NHEAD))
    kv = torch.cat([k, v], 2).contiguous()
    qm = km = None
    mask = case["mask"]
    if mask in ("qmask", "both"):
        qm = (torch.rand(n, L, generator=g) > 0.3).float()
        qm[0, 0], qm[0, L - 1], qm[n - 1, 0], qm[n - 1, L - 1] = 0.0, 1.0, 1.0, 0.0
    if mask in ("kvmask", "both"):
        km = (torch.rand(n, S, generator=g) > 0.3).float()
        km[0, 0], km[0, S - 1], km[n - 1, 0], km[n - 1, S - 1] = 0.0, 1.0, 1.0, 0.0
    if mask == "kvtail":        # the last, partial chunk holds masked rows only
        km = (torch.rand(n, S, generator=g) > 0.3).float()
        km[:, ((S - 1) // c) * c:] = 0.0
        km[:, 0] = 1.0
    if mask == "image":
        km = (torch.rand(n, S, generator=g) > 0.3).float()
        km[:, 0] = 1.0
        km[MASKED_IMAGE] = 0.0
    return q, kv, qm, km


def _split(q, kv):
    n, L, Cd = q.shape
    S, D = kv.shape[1], Cd // NHEAD
    return q.view(n, L, NHEAD, D), kv[..., :Cd].reshape(n, S, NHEAD, D), kv[..., Cd:].reshape(n, S, NHEAD, D)


def masked_linear_attention(q, k, v, q_mask=None, kv_mask=None, eps=EPS):
    """linear_attention.py:20-47 with its masks (:35-41): Q = (elu(q) + 1) * q_mask, K = (elu(k) + 1) * kv_mask,
    V = v * kv_mask / S with the full length S.  q, k, v: [n, rows, H, D]; no masks: loftr_ref.linear_attention."""
    Q, K = F.elu(q) + 1, F.elu(k) + 1
    if q_mask is not None:
        Q = Q * q_mask[:, :, None, None].to(Q.dtype)
    if kv_mask is not None:
        K = K * kv_mask[:, :, None, None].to(K.dtype)
        v = v * kv_mask[:, :, None, None].to(v.dtype)
    S = v.size(1)
    v = v / S
    KV = torch.einsum("nshd,nshv->nhdv", K, v)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, K.sum(dim=1)) + eps)
    return (torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * S).contiguous()


def attention_ref(q, kv, q_mask=None, kv_mask=None, dtype=torch.float64):
    """the message [n, L, C] in `dtype`"""
    Q, K, V = _split(q.to(dtype), kv.to(dtype))
    if q_mask is None and kv_mask is None:
        out = loftr_ref.linear_attention(Q, K, V)
    else:
        out = masked_linear_attention(Q, K, V, q_mask, kv_mask)
    return out.reshape(q.shape)


def attention_denominator(q, kv, q_mask=None, kv_mask=None):
    """fp64 Q . Ksum [n, L, H] (without eps)"""
    Q, K, _ = _split(q.double(), kv.double())
    Q, K = F.elu(Q) + 1, F.elu(K) + 1
    if q_mask is not None:
        Q = Q * q_mask[:, :, None, None].double()
    if kv_mask is not None:
        K = K * kv_mask[:, :, None, None].double()
    return torch.einsum("nlhd,nhd->nlh", Q, K.sum(dim=1))


ATTENTION_FAULTS = ("ragged_dropped", "chunk_length", "no_eps", "qmask_ignored", "kvmask_ignored", "wrong_image", "doubled")


def attention_kernel_order(q, kv, q_mask, kv_mask, c, fault=None, dtype=torch.float32):
    """An independent restatement in the kernels' order of summation: per chunk of c source rows the partial K^T V and Ksum, row
    after row; the chunk partials in chunk order; per query row numerator and denominator over d ascending, then
    num * (1 / (den + eps)) * S.  dtype fp32: what a correct kernel may compute; `fault`: one of ATTENTION_FAULTS planted."""
    Q, K, V = _split(q.to(dtype), kv.to(dtype))
    n, L, H, D = Q.shape
    S = K.shape[1]
    Q, K = F.elu(Q) + 1, F.elu(K) + 1
    if q_mask is not None and fault != "qmask_ignored":
        Q = Q * q_mask[:, :, None, None].to(dtype)
    if kv_mask is not None and fault != "kvmask_ignored":
        K = K * kv_mask[:, :, None, None].to(dtype)
        V = V * kv_mask[:, :, None, None].to(dtype)
    kvs = torch.zeros(n, H, D, D, dtype=dtype)
    ksum = torch.zeros(n, H, D, dtype=dtype)
    for s0 in range(0, S, c):
        ns = min(c, S - s0)
        if fault == "ragged_dropped" and ns < c:
            break
        length = torch.tensor(float(ns if fault == "chunk_length" else S), dtype=dtype)
        pkv = torch.zeros(n, H, D, D, dtype=dtype)
        pk = torch.zeros(n, H, D, dtype=dtype)
        for s in range(s0, s0 + ns):
            ks = K[:, s]
            pk = pk + ks
            pkv = pkv + ks[..., :, None] * (V[:, s] / length)[..., None, :]
        kvs, ksum = kvs + pkv, ksum + pk
    if fault == "wrong_image":
        kvs, ksum = kvs.roll(1, 0), ksum.roll(1, 0)
    num = torch.zeros(n, L, H, D, dtype=dtype)
    den = torch.zeros(n, L, H, dtype=dtype)
    for d in range(D):
        num = num + Q[..., d, None] * kvs[:, None, :, d, :]
        den = den + Q[..., d] * ksum[:, None, :, d]
    eps = 0.0 if fault == "no_eps" else EPS
    out = num * (1.0 / (den + torch.tensor(eps, dtype=dtype)))[..., None] * torch.tensor(float(S), dtype=dtype)
    if fault == "doubled":
        out = out * 2
    return out.reshape(n, L, H * D)


def flag_case(c, r):
    """A message beyond the planes range: v of head 2 is scaled so that its convex combinations (which is all a message is:
    num / den * S is a weighted mean of the v rows, whatever q) exceed PLANES_LIMIT; q of that head is large as well."""
    case = dict(id="attn-flag", C=256, n=2, L=r + 1, S=c + 1, mask=None, seed=31)
    q, kv, _, _ = attention_inputs(case, c)
    D = 256 // NHEAD
    q[:, :, 2 * D:3 * D] = q[:, :, 2 * D:3 * D].abs() * 100.0
    kv[:, :, 256 + 2 * D:256 + 3 * D] = 4.0 * PLANES_LIMIT + kv[:, :, 256 + 2 * D:256 + 3 * D].abs()
    return case, q, kv


def assert_attention_refusals(lib):
    """what pope_loftr_linear_attention_f32 refuses, by return code; no call gets as far as a HIP call (null stream, host memory)"""
    import ctypes
    buf = ctypes.create_string_buffer(1024)
    ok = (ctypes.addressof(buf) + 255) & ~255             # 256-byte aligned, never dereferenced
    big = 1 << 40

    def call(q=ok, kv=ok, n=1, L=4, S=4, Cd=256, H=NHEAD, o32=ok, opl=None, ws=ok, nbytes=big):
        return lib.pope_loftr_linear_attention_f32(q, kv, None, None, n, L, S, Cd, H, o32, opl, ws, nbytes, None, None)

    assert call(q=None) == -1 and call(kv=None) == -1 and call(ws=None) == -1
    assert call(n=0) == -1 and call(L=0) == -1 and call(S=-1) == -1
    assert call(Cd=64) == -1 and call(Cd=192) == -1 and call(H=4) == -1
    assert call(o32=ok, opl=ok) == -1 and call(o32=None, opl=None) == -1
    assert call(ws=ok + 128) == -1
    assert call(L=(0x7fffffff // 512) + 1) == -1 and call(S=(0x7fffffff // 512) + 1) == -1      # the layer's index range: 2^31 / 2C rows
    assert call(Cd=128, n=2, L=(0x7fffffff // 256) // 2 + 1) == -1
    need = lib.pope_loftr_linear_attention_workspace_bytes(1, 4, 256, NHEAD)
    assert need > 0 and need % 256 == 0
    assert call(nbytes=need - 1) == -3 and call(nbytes=0) == -3
    for bad in ((0, 4, 256, 8), (1, 0, 256, 8), (1, 4, 64, 8), (1, 4, 256, 4)):
        assert lib.pope_loftr_linear_attention_workspace_bytes(*bad) == 0


# ---- the encoder layer --------------------------------------------------------------------------------------------------------
LAYER_PRECISIONS = ("f16x3", "f32")
COARSE, FINE = "loftr_coarse.layers.0", "loftr_fine.layers.0"


def layer_cases(c, r):
    shapes = [("cross", COARSE, 256, 1, 1, 1, False), ("cross", COARSE, 256, 2, r + 1, c + 1, False),
              ("cross", COARSE, 256, 3, c, 2 * c + 1, False), ("self", COARSE, 256, 2, c + 1, c + 1, False),
              ("self", FINE, 128, 2, 25, 25, False), ("cross", FINE, 128, 5, 25, 25, False),
              ("cross", COARSE, 256, 2, r + 1, c + 1, True)]
    return [dict(id=f"layer-{prec}-{kind}-C{Cd}-n{n}-L{L}-S{S}" + ("-masked" if masked else ""), kind=kind, prefix=prefix, C=Cd, n=n,
                 L=L, S=S, masked=masked, precision=prec, seed=3000 + k)
            for prec in LAYER_PRECISIONS for k, (kind, prefix, Cd, n, L, S, masked) in enumerate(shapes)]


def layer_inputs(case):
    """x [n, L, C], source [n, S, C] (x itself for a self layer), x_mask, source_mask"""
    g = _gen(case["seed"])
    n, L, S, Cd = case["n"], case["L"], case["S"], case["C"]
    x = torch.randn(n, L, Cd, generator=g)
    source = x if case["kind"] == "self" else torch.randn(n, S, Cd, generator=g)
    xm = sm = None
    if case["masked"]:
        xm = (torch.rand(n, L, generator=g) > 0.3).float()
        sm = (torch.rand(n, S, generator=g) > 0.3).float()
        xm[:, 0], sm[:, 0], xm[0, L - 1], sm[0, S - 1] = 1.0, 1.0, 0.0, 0.0
    return x, source, xm, sm


def layer_state(sd, prefix):
    """the layer's parameters without the prefix (LoFTREncoderLayer.load_state_dict)"""
    return {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}


def masked_encoder_layer(sd, p, x, source, nhead, x_mask=None, source_mask=None):
    """loftr_ref.encoder_layer (transformer.py:35-58) with the padding masks handed to the attention"""
    n, d = x.size(0), x.size(2)
    q = F.linear(x, sd[p + ".q_proj.weight"]).view(n, -1, nhead, d // nhead)
    k = F.linear(source, sd[p + ".k_proj.weight"]).view(n, -1, nhead, d // nhead)
    v = F.linear(source, sd[p + ".v_proj.weight"]).view(n, -1, nhead, d // nhead)
    msg = F.linear(masked_linear_attention(q, k, v, x_mask, source_mask).view(n, -1, d), sd[p + ".merge.weight"])
    msg = F.layer_norm(msg, (d,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5)
    msg = F.linear(F.relu(F.linear(torch.cat([x, msg], dim=2), sd[p + ".mlp.0.weight"])), sd[p + ".mlp.2.weight"])
    msg = F.layer_norm(msg, (d,), sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5)
    return x + msg


def as_dtype(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def layer_ref(sd, case, x, source, xm, sm, dtype=torch.float64):
    sdd = as_dtype(layer_state_full(sd, case["prefix"]), dtype)
    x, source = x.to(dtype), source.to(dtype)
    if xm is None and sm is None:
        return loftr_ref.encoder_layer(sdd, case["prefix"], x, source, NHEAD)
    return masked_encoder_layer(sdd, case["prefix"], x, source, NHEAD, xm, sm)


def layer_state_full(sd, prefix):
    return {k: v for k, v in sd.items() if k.startswith(prefix + ".")}


# ---- fine matching ------------------------------------------------------------------------------------------------------------
FINE_W, FINE_C, FINE_M = (3, 5, 8), (32, 128), (1, 4, 5)
FINE_KINDS = ("random", "peak_first", "peak_last", "flat")
FINE_ENTRIES = ("plain", "scaled")
FINE_IMAGES = 3
SCALE_PX = 2.0
PEAK_LOGIT = 3.4       # what the planted peak adds to its position's logit: the largest weight, far from one-hot
COLUMNS = ("x", "y", "spread", "mkpts1_f.x", "mkpts1_f.y")


def fine_match_cases():
    cases = []
    for entry in FINE_ENTRIES:
        for W in FINE_W:
            for Cd in FINE_C:
                for kind in FINE_KINDS:
                    cases.append(dict(id=f"fine-{entry}-W{W}-C{Cd}-{kind}", entry=entry, W=W, C=Cd, kind=kind,
                                      seed=4000 + 100 * W + Cd + FINE_KINDS.index(kind)))
        for W, Cd in ((5, 128), (8, 32)):
            cases.append(dict(id=f"fine-{entry}-W{W}-C{Cd}-saturated", entry=entry, W=W, C=Cd, kind="saturated", seed=4900 + W))
    return cases


def fine_match_inputs(case, M):
    """win0, win1 [M, WW, C], mkpts1_c [M, 2], b_ids [M] (int64), scale1 [FINE_IMAGES, 2] or None"""
    g = _gen(case["seed"] * 10 + M)
    W, Cd, kind = case["W"], case["C"], case["kind"]
    WW = W * W
    w0, w1 = torch.randn(M, WW, Cd, generator=g), torch.randn(M, WW, Cd, generator=g)
    centre = w0[:, WW // 2]
    if kind in ("peak_first", "peak_last"):
        # <centre, a centre> / sqrt(C) = PEAK_LOGIT for a = PEAK_LOGIT sqrt(C) / |centre|^2; the other logits are about N(0, 1 / 4)
        w1 = w1 * 0.5
        w1[:, 0 if kind == "peak_first" else WW - 1] = centre * (PEAK_LOGIT * math.sqrt(Cd) / (centre * centre).sum(1, keepdim=True))
    elif kind == "flat":
        w1 = w1[:, :1].expand(M, WW, Cd).contiguous()
    elif kind == "saturated":
        k0 = torch.randint(0, WW, (M,), generator=g)
        w1[torch.arange(M), k0] = centre * 50.0
    mk = torch.rand(M, 2, generator=g) * 200.0
    b_ids = (torch.arange(M) * 2) % FINE_IMAGES
    scale1 = None
    if case["entry"] == "scaled":
        scale1 = torch.tensor([[1.25, 0.75], [0.6, 1.7], [2.0, 0.9]])[:FINE_IMAGES]
    return w0, w1, mk, b_ids.long(), scale1


@contextlib.contextmanager
def _default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def fine_match_ref(w0, w1, mk, b_ids, scale1, dtype=torch.float64):
    """loftr_ref.fine_matching in `dtype` (its grid included: the oracle builds it in torch's default dtype) -> [M, 5]:
    x, y, spread, mkpts1_f.  The scaled entry's factor scale_px * scale1[b_ids] (fine_matching.py:68) goes in as `scale`."""
    scale = SCALE_PX
    if scale1 is not None:
        scale = torch.tensor(SCALE_PX, dtype=dtype) * scale1.to(dtype)[b_ids]
    with _default_dtype(dtype):
        expec, _, mk1f = loftr_ref.fine_matching(w0.to(dtype), w1.to(dtype), mk.to(dtype), mk.to(dtype), scale)
    return torch.cat([expec, mk1f], 1)


def fine_match_variances(w0, w1):
    """fp64 variance per axis [M, 2] and heat [M, WW]"""
    M, WW, Cd = w0.shape
    W = int(math.sqrt(WW))
    w0, w1 = w0.double(), w1.double()
    heat = torch.softmax(torch.einsum("mc,mrc->mr", w0[:, WW // 2], w1) / Cd ** 0.5, 1)
    lin = torch.linspace(-1, 1, W, dtype=torch.float64)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    grid = torch.stack([gx, gy], -1).reshape(1, WW, 2)
    coords = (heat[:, :, None] * grid).sum(1)
    return (grid ** 2 * heat[:, :, None]).sum(1) - coords ** 2, heat


FINE_FAULTS = ("centre_row0", "xy_swapped", "scale_axes_swapped")


def fine_match_fault(fault, w0, w1, mk, b_ids, scale1):
    """fp64 result [M, 5] of a kernel with `fault`"""
    W = int(math.sqrt(w0.shape[1]))
    if fault == "centre_row0":
        w0 = w0.clone()
        w0[:, w0.shape[1] // 2] = w0[:, 0]
        return fine_match_ref(w0, w1, mk, b_ids, scale1)
    ref = fine_match_ref(w0, w1, mk, b_ids, scale1)
    scale = torch.full((w0.shape[0], 2), SCALE_PX, dtype=torch.float64)
    if scale1 is not None:
        scale = SCALE_PX * scale1.double()[b_ids]
    coords = ref[:, :2]
    if fault == "xy_swapped":
        coords = coords[:, [1, 0]]
    if fault == "scale_axes_swapped":
        scale = scale[:, [1, 0]]
    return torch.cat([coords, ref[:, 2:3], mk.double() + coords * (W // 2) * scale], 1)


def fine_match_checked_columns(kind):
    return (0, 1, 3, 4) if kind == "saturated" else (0, 1, 2, 3, 4)


def fine_match_ratios(case, got, want64, want32):
    """one ratio per checked column of the case's launches taken together ([sum of FINE_M, 5]).  Flat heatmap: the expectation
    is a sum of WW terms of magnitude up to 1 / WW that cancels to 0, so its floor is an ulp of the grid's extent 1, not of 0."""
    scale = 1.0 if case["kind"] == "flat" else None
    return [group_ratio(got[:, j].contiguous(), want64[:, j].contiguous(), want32[:, j].contiguous(), scale if j < 2 else None)
            for j in fine_match_checked_columns(case["kind"])]


# ---- fine preprocess ----------------------------------------------------------------------------------------------------------
PRE_STRIDE, PRE_W, PRE_CC, PRE_CF, PRE_N = 4, 5, 256, 128, 2
PRE_GRID0, PRE_GRID1 = (12, 16), (10, 20)        # coarse cells (rows, columns) of the two maps: nothing in common
PRE_LAYOUTS = ("nchw", "nhwc_view")


def fine_pre_cases():
    return [dict(id=f"pre-{prec}-{layout}-M{M}", precision=prec, layout=layout, M=M, seed=5000 + M)
            for prec in LAYER_PRECISIONS for layout in PRE_LAYOUTS for M in (9, 1)]


def _cell(grid, y, x):
    return y * grid[1] + x


def fine_pre_matches(M):
    """b, i, j.  M = 9: the four corners of each map (map 1's in another order), a cell on each edge of each map, an interior one"""
    (h0, w0), (h1, w1) = PRE_GRID0, PRE_GRID1
    if M == 1:
        return torch.tensor([1]), torch.tensor([_cell(PRE_GRID0, 5, 7)]), torch.tensor([_cell(PRE_GRID1, 0, w1 - 1)])
    i = [_cell(PRE_GRID0, 0, 0), _cell(PRE_GRID0, 0, w0 - 1), _cell(PRE_GRID0, h0 - 1, 0), _cell(PRE_GRID0, h0 - 1, w0 - 1),
         _cell(PRE_GRID0, 0, 6), _cell(PRE_GRID0, h0 - 1, 9), _cell(PRE_GRID0, 4, 0), _cell(PRE_GRID0, 7, w0 - 1), _cell(PRE_GRID0, 5, 7)]
    j = [_cell(PRE_GRID1, h1 - 1, w1 - 1), _cell(PRE_GRID1, h1 - 1, 0), _cell(PRE_GRID1, 0, w1 - 1), _cell(PRE_GRID1, 0, 0),
         _cell(PRE_GRID1, h1 - 1, 13), _cell(PRE_GRID1, 0, 3), _cell(PRE_GRID1, 6, w1 - 1), _cell(PRE_GRID1, 2, 0), _cell(PRE_GRID1, 4, 11)]
    return torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 1]), torch.tensor(i), torch.tensor(j)


def fine_pre_inputs(case):
    """f0 [n, Cf, H0, W0], f1 [n, Cf, H1, W1] (NCHW values; the layout is the GPU test's business), c0 [n, L, Cc], c1 [n, S, Cc],
    b, i, j"""
    g = _gen(case["seed"])
    (h0, w0), (h1, w1), s = PRE_GRID0, PRE_GRID1, PRE_STRIDE
    f0 = torch.randn(PRE_N, PRE_CF, h0 * s, w0 * s, generator=g)
    f1 = torch.randn(PRE_N, PRE_CF, h1 * s, w1 * s, generator=g)
    c0 = torch.randn(PRE_N, h0 * w0, PRE_CC, generator=g)
    c1 = torch.randn(PRE_N, h1 * w1, PRE_CC, generator=g)
    return (f0, f1, c0, c1) + fine_pre_matches(case["M"])


def fine_pre_ref(sd, f0, f1, c0, c1, b, i, j, dtype=torch.float64, fault=None):
    """(out0, out1) [M, WW, Cf].  fault "wc_of_stream0": stream 1's cell index decoded with stream 0's grid width"""
    if fault == "wc_of_stream0":
        j = ((j // PRE_GRID0[1]) % PRE_GRID1[0]) * PRE_GRID1[1] + j % PRE_GRID0[1]
    sdd = as_dtype({k: v for k, v in sd.items() if k.startswith("fine_preprocess.")}, dtype)
    out0, out1 = loftr_ref.fine_preprocess(sdd, f0.to(dtype), f1.to(dtype), c0.to(dtype), c1.to(dtype), b, i, j, PRE_W, PRE_STRIDE)
    return out0.contiguous(), out1.contiguous()
