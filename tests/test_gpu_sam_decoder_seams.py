"""GPU: the SAM mask decoder's kernels (csrc/sam_decoder.hip) one at a time, through their op-level entries, against fp64 at their
seams: the token counts base .. max, 1 / 2 / chunk prompts per launch, score regimes in which a softmax without (or with a partly
missing) maximum cannot pass, slot maps and strides of layer 0, the row tails and switches of the token linear, LayerNorm rows
with a large offset or a tiny variance; then the whole decoder around the prompt chunk and the second pass of its image loop.

Cases, inputs, references and the comparison are tests/sam_decoder_checks.py (proven on the CPU by
test_sam_decoder_checks_cpu.py): per group, max |gpu - fp64| <= 4 max(e32, 2^-23 max |fp64|) with e32 the error of the same torch
restatement in fp32.  Every output buffer carries a guard row (the linear: guard columns too) that must stay bit-unchanged.
Measured ratios are printed (-s) and recorded in profiles/sam_decoder_seams.md.  The image side is 4 096 tokens throughout, the
smallest (and only) shape these kernels have."""
import ctypes as C

import pytest
import torch

import sam_decoder_checks as sc
from pope_amd import _lib, synth
from test_sam_decoder_cpu import build_models, restate

pytestmark = pytest.mark.gpu
NPIX, D, DI = sc.NPIX, sc.D, sc.DI


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def seams(hip_lib):
    return sc.read_seams(hip_lib)


def _p(t, offset=0):
    return C.c_void_p(t.data_ptr() + 4 * offset) if t is not None else None


def _ints(values):
    return (C.c_int * len(values))(*values)


def _ok(status, what):
    """A launch that fails ends the session: nothing more is started on a device that may have faulted"""
    if status != 0:
        pytest.exit(f"{what}: status {status} ({_lib.lib().pope_error_string(status).decode()})", returncode=3)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _guarded(rows, cols, dev):
    """[rows + 1, cols] of the sentinel: the last row is the guard"""
    return torch.full((rows + 1, cols), sc.SENTINEL, dtype=torch.float32, device=dev)


def _result(buf, rows, what):
    _sync(what)
    host = buf.cpu()
    assert bool((host[rows:] == sc.SENTINEL).all()), f"{what}: the guard row was written"
    return host[:rows]


def _planes(rows_f32, cols):
    """the bytes of `rows` fp32 rows read as planes [rows, cols / 32, 2, 32]"""
    return rows_f32.contiguous().view(torch.float16).view(rows_f32.shape[0], cols // 32, 2, 32)


# ---- the entries ------------------------------------------------------------------------------------------------------------------
def op_self(lib, dev, qkv, P, T, what="self"):
    qkv = qkv.to(dev).contiguous()
    out = _guarded(P * T, D, dev)
    _ok(lib.pope_sam_decoder_self_attention_f32(_p(qkv), _p(out), P, T, _lib.stream_of(dev)), what)
    return _result(out, P * T, what)


def op_t2i(lib, dev, q, Kb, Vb, slots, T, P, what="t2i"):
    """Kb [n, 4096, ldk] (k in the first 128 columns), Vb [n, 4096, 128]"""
    q, Kb, Vb = q.to(dev).contiguous(), Kb.to(dev).contiguous(), Vb.to(dev).contiguous()
    ldk = Kb.shape[-1]
    out = _guarded(P * T, DI, dev)
    _ok(lib.pope_sam_decoder_t2i_attention_f32(_p(q), _p(Kb), ldk, NPIX * ldk, _p(Vb), NPIX * DI, _ints(slots), _p(out), T, P,
                                               _lib.stream_of(dev)), what)
    return _result(out, P * T, what)


def op_i2t(lib, dev, Qb, slots, kv, T, P, planes=False, what="i2t"):
    """Qb [n, 4096, 256] (q in the LAST 128 columns: the [k | q] layout).  -> (fp32 rows or planes, the range-flag word)"""
    Qb, kv = Qb.to(dev).contiguous(), kv.to(dev).contiguous()
    out = _guarded(P * NPIX, DI, dev)          # planes: the same bytes per row
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _ok(lib.pope_sam_decoder_i2t_attention_f32(_p(Qb, DI), NPIX * D, _ints(slots), _p(kv), T, P, None if planes else _p(out),
                                               _p(out) if planes else None, _p(flag), _lib.stream_of(dev)), what)
    rows = _result(out, P * NPIX, what)
    return (_planes(rows, DI) if planes else rows), int(flag.item())


def op_norm(lib, dev, res, slots, y, w, b, pe_t, P, f32=True, what="norm"):
    """-> (keys, operand A (planes; None with f32), operand B (fp32 rows or planes), the range-flag word)"""
    res, y, w, b, pe_t = (t.to(dev).contiguous() for t in (res, y, w, b, pe_t))
    rows = P * NPIX
    keys, opB = _guarded(rows, D, dev), _guarded(rows, D, dev)
    opA = None if f32 else _guarded(rows, D, dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _ok(lib.pope_sam_decoder_residual_norm_f32(_p(res), NPIX * D, _ints(slots), _p(y), _p(w), _p(b), sc.TOKEN_EPS, _p(pe_t), _p(keys),
                                               _p(opA), _p(opB), int(f32), P, _p(flag), _lib.stream_of(dev)), what)
    k, B = _result(keys, rows, what), _result(opB, rows, what)
    if f32:
        return k, None, B, int(flag.item())
    return k, _planes(_result(opA, rows, what), D), _planes(B, D), int(flag.item())


def op_prep(lib, dev, image, image_pe, dense, nz, f32=True, what="prep"):
    image, image_pe, dense = (t.to(dev).contiguous() for t in (image, image_pe, dense))
    rows = nz * NPIX
    keys, opB, pe_t = _guarded(rows, D, dev), _guarded(rows, D, dev), _guarded(NPIX, D, dev)
    opA = None if f32 else _guarded(rows, D, dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _ok(lib.pope_sam_decoder_prepare_keys_f32(_p(image), D * NPIX if image.shape[0] > 1 else 0, _p(image_pe), _p(dense),
                                              D * NPIX if dense.shape[0] > 1 else 0, nz, _p(keys), _p(opA), _p(opB), int(f32), _p(pe_t),
                                              _p(flag), _lib.stream_of(dev)), what)
    k, B, pt = _result(keys, rows, what), _result(opB, rows, what), _result(pe_t, NPIX, what)
    if f32:
        return k, None, B, pt, int(flag.item())
    return k, _planes(_result(opA, rows, what), D), _planes(B, D), pt, int(flag.item())


def op_tail(lib, dev, y, ln_w, ln_b, w2, b2, hyper, multimask, P, what="tail"):
    y, ln_w, ln_b, w2, b2, hyper = (t.to(dev).contiguous() for t in (y, ln_w, ln_b, w2, b2, hyper))
    Cm = sc.NMASK - 1 if multimask else 1
    out = _guarded(P * Cm, 256 * 256, dev)
    _ok(lib.pope_sam_decoder_upscale_tail_f32(_p(y), _p(ln_w), _p(ln_b), sc.UP_EPS, _p(w2), _p(b2), _p(hyper), int(multimask), P,
                                              _p(out), _lib.stream_of(dev)), what)
    return _result(out, P * Cm, what).view(P, Cm, 256, 256)


def op_lin(lib, dev, xbuf, x_offset, ldx, add, add_cols, W, bias, res, M, N, K, relu, what="lin"):
    """Y [M, N]; rows of pitch N + LIN_PAD in a buffer of M + 1 rows: the pad columns and the last row are guards"""
    xbuf, W, bias = xbuf.to(dev).contiguous(), W.to(dev).contiguous(), bias.to(dev).contiguous()
    add = None if add is None else add.to(dev).contiguous()
    res = None if res is None else res.to(dev).contiguous()
    ldy = N + sc.LIN_PAD
    out = _guarded(M, ldy, dev)
    _ok(lib.pope_sam_decoder_token_linear_f32(_p(xbuf, x_offset), ldx, _p(add), add_cols, _p(W), _p(bias), _p(res), _p(out), ldy, M, N, K,
                                              int(relu), _lib.stream_of(dev)), what)
    rows = _result(out, M, what)
    assert bool((rows[:, N:] == sc.SENTINEL).all()), f"{what}: a column past N was written"
    return rows[:, :N].contiguous()


# ---- the attentions -----------------------------------------------------------------------------------------------------------------
def _garbage(shape, seed):
    return 50.0 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _attention(lib, dev, case, q, k, v, slots, planes=False):
    kernel, T, P = case["kernel"], case["T"], case["P"]
    if kernel == "self":
        qkv = torch.cat([q.reshape(P * T, D), k.reshape(P * T, D), v.reshape(P * T, D)], 1)
        return op_self(lib, dev, qkv, P, T, case["id"]).view(P, T, D)
    if kernel == "t2i":
        n, ldk = k.shape[0], case["ldk"]
        Kb = _garbage((n, NPIX, ldk), case["seed"] + 1)              # ldk 256: the other half of the [k | q] rows is not k
        Kb[..., :DI] = k.reshape(n, NPIX, DI)
        return op_t2i(lib, dev, q.reshape(P * T, DI), Kb, v.reshape(n, NPIX, DI), slots, T, P, case["id"]).view(P, T, DI)
    n = q.shape[0]
    Qb = _garbage((n, NPIX, D), case["seed"] + 1)
    Qb[..., DI:] = q.reshape(n, NPIX, DI)
    kv = torch.cat([k.reshape(P * T, DI), v.reshape(P * T, DI)], 1)
    out, bits = op_i2t(lib, dev, Qb, slots, kv, T, P, planes, case["id"])
    return (out, bits) if planes else (out.view(P, NPIX, DI), bits)


@pytest.mark.parametrize("kernel", ["self", "t2i", "i2t"])
def test_attention_matches_fp64_in_every_regime(dev, hip_lib, seams, kernel):
    worst = {}
    for case in (k for k in sc.attention_cases(seams) if k["kernel"] == kernel):
        x = sc.attention_inputs(case)
        want64, want32 = sc.attention_ref(case, *x), sc.attention_ref(case, *x, dtype=torch.float32)
        got = _attention(hip_lib, dev, case, *x)
        if kernel == "i2t":
            got, bits = got
            assert bits == 0, case["id"]                             # fp32 rows: no range contract
        ratios = sc.head_ratios(got, want64, want32)
        regime = case["regime"].rstrip("0123456789")
        worst[regime] = max(worst.get(regime, (-1.0, "")), (sc.report(case["id"], ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
    for regime, (ratio, cid) in worst.items():
        print(f"{kernel} attention, {regime}: worst ratio {ratio:.3f} at {cid}")


def test_i2t_planes_are_the_planes_of_the_rows_and_raise_the_range_flag(dev, hip_lib, seams):
    case = next(k for k in sc.attention_cases(seams) if k["kernel"] == "i2t" and k["slots"])
    x = sc.attention_inputs(case)
    rows, bits = _attention(hip_lib, dev, case, *x)
    planes, pbits = _attention(hip_lib, dev, case, *x, planes=True)
    assert bits == 0 and pbits == 0
    assert torch.equal(planes, _lib.to_planes(rows.reshape(-1, DI), _lib.PLANES_ACT_SCALE))
    case, q, k, v, slots = sc.i2t_flag_case(seams)
    rows, bits = _attention(hip_lib, dev, case, q, k, v, slots)
    assert bits == 0 and float(rows.abs().min()) > sc.PLANES_LIMIT
    ratios = sc.head_ratios(rows, sc.attention_ref(case, q, k, v, slots), sc.attention_ref(case, q, k, v, slots, dtype=torch.float32))
    sc.report(case["id"], ratios)
    assert max(ratios) <= 1.0, ratios
    _, bits = _attention(hip_lib, dev, case, q, k, v, slots, planes=True)
    assert bits != 0


# ---- the token linear ---------------------------------------------------------------------------------------------------------------
def test_token_linear_matches_fp64_at_every_tail_and_switch(dev, hip_lib, seams):
    worst = (-1.0, "")
    for case in sc.linear_cases(seams):
        xbuf, X, ldx, add, W, bias, res = sc.linear_inputs(case)
        want64, want32 = sc.linear_ref(case, X, add, W, bias, res), sc.linear_ref(case, X, add, W, bias, res, torch.float32)
        offset = 0 if case["token"] is None else case["token"] * case["K"]
        got = op_lin(hip_lib, dev, xbuf, offset, ldx, add, case["add_cols"], W, bias, res, case["M"], case["N"], case["K"], case["relu"],
                     case["id"])
        ratios = sc.column_block_ratios(got, want64, want32)
        worst = max(worst, (max(ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
    print(f"token linear: worst ratio {worst[0]:.3f} at {worst[1]} ({len(sc.linear_cases(seams))} cases)")


# ---- residual + LayerNorm, prepare keys ---------------------------------------------------------------------------------------------
def test_residual_norm_matches_fp64_and_its_operands_are_exact(dev, hip_lib, seams):
    worst = {}
    for case in sc.norm_cases(seams):
        res, y, w, b, pe_t, slots = sc.norm_inputs(case)
        want64, want32 = sc.norm_ref(res, y, w, b, pe_t, slots), sc.norm_ref(res, y, w, b, pe_t, slots, dtype=torch.float32)
        P = case["P"]
        keys, _, opB, bits = op_norm(hip_lib, dev, res, slots, y, w, b, pe_t, P, True, case["id"])
        assert bits == 0, case["id"]
        ratios = [sc.group_ratio(keys.view(P, NPIX, D), want64[0], want32[0]), sc.group_ratio(opB.view(P, NPIX, D), want64[1], want32[1])]
        worst[case["regime"]] = max(worst.get(case["regime"], (-1.0, "")), (sc.report(case["id"], ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
        assert torch.equal(opB, keys + pe_t.repeat(P, 1))           # one fp32 add of the published keys
        if P > 2:
            continue
        pkeys, opA, opBp, bits = op_norm(hip_lib, dev, res, slots, y, w, b, pe_t, P, False, case["id"] + "-planes")
        assert bits == 0 and torch.equal(pkeys, keys)
        assert torch.equal(opA, _lib.to_planes(keys, _lib.PLANES_ACT_SCALE)) and torch.equal(opBp, _lib.to_planes(opB, _lib.PLANES_ACT_SCALE))
    for regime, (ratio, cid) in worst.items():
        print(f"residual norm, {regime}: worst ratio {ratio:.3f} at {cid}")
    # the range flag: raised by planes beyond the f16 range, left alone by fp32 operands
    case = sc.norm_cases(seams)[0]
    res, y, w, b, pe_t, slots = sc.norm_inputs(case)
    big = sc.norm_flag_weight(w)
    keys, _, _, bits = op_norm(hip_lib, dev, res, slots, y, big, b, pe_t, case["P"], True)
    assert bits == 0 and float(keys.abs().max()) > sc.PLANES_LIMIT
    _, _, _, bits = op_norm(hip_lib, dev, res, slots, y, big, b, pe_t, case["P"], False)
    assert bits != 0


def test_prepare_keys_is_exact(dev, hip_lib):
    for case in sc.prep_cases():
        image, image_pe, dense = sc.prep_inputs(case)
        nz = case["nz"]
        want_keys, want_pe, want_B = sc.prep_ref(image, image_pe, dense, nz)
        keys, _, opB, pe_t, bits = op_prep(hip_lib, dev, image, image_pe, dense, nz, True, case["id"])
        assert bits == 0
        assert torch.equal(keys.view(nz, NPIX, D), want_keys) and torch.equal(pe_t, want_pe), case["id"]
        assert torch.equal(opB.view(nz, NPIX, D), want_B), case["id"]
        keys, opA, opB, pe_t, bits = op_prep(hip_lib, dev, image, image_pe, dense, nz, False, case["id"] + "-planes")
        assert bits == 0
        assert torch.equal(keys.view(nz, NPIX, D), want_keys) and torch.equal(pe_t, want_pe), case["id"]
        assert torch.equal(opA, _lib.to_planes(want_keys.view(-1, D), _lib.PLANES_ACT_SCALE)), case["id"]
        assert torch.equal(opB, _lib.to_planes(want_B.view(-1, D), _lib.PLANES_ACT_SCALE)), case["id"]


# ---- the upscaling tail -------------------------------------------------------------------------------------------------------------
def test_upscale_tail_matches_fp64_per_mask_and_sub_pixel(dev, hip_lib):
    worst = {}
    for case in sc.tail_cases():
        y, ln_w, ln_b, w3, b2, hyper = sc.tail_inputs(case)
        want64 = sc.tail_ref(case, y, ln_w, ln_b, w3, b2, hyper)
        want32 = sc.tail_ref(case, y, ln_w, ln_b, w3, b2, hyper, dtype=torch.float32)
        got = op_tail(hip_lib, dev, y, ln_w, ln_b, sc.tail_w2(w3), b2, hyper, case["multimask"], case["P"], case["id"])
        ratios = sc.tail_ratios(got, want64, want32)
        print(f"{case['id']}: per mask " + " ".join(f"{r:.3f}" for r in ratios[:got.shape[1]]) + f", worst sub-pixel group {max(ratios):.3f}")
        worst[case["regime"]] = max(worst.get(case["regime"], (-1.0, "")), (max(ratios), case["id"]))
        assert max(ratios) <= 1.0, (case["id"], ratios)
    for regime, (ratio, cid) in worst.items():
        print(f"upscale tail, {regime}: worst ratio {ratio:.3f} at {cid}")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_op_entries_refuse_bad_arguments(hip_lib, seams):
    """return codes only: every refused call returns on the host, before any launch (the CPU suite runs the same list)"""
    sc.assert_refusals(hip_lib, seams)


# ---- the whole decoder --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev):
    sd = synth.synthetic_sam_decoder_state_dict(seed=0)
    pe, md = build_models(sd)
    return {k: v.to(dev) for k, v in sd.items()}, pe.to(dev), md.to(dev)


@pytest.fixture(scope="module")
def image(dev):
    return synth.synthetic_sam_image_embedding(seed=1).to(dev)


_RESTATED = {}


def _restated(sd, image, image_pe, sparse, dense, multimask, key):
    """(fp64, fp32) restatements (masks, iou, hs, keys), torch on the device, once per case and shared by both precisions"""
    if key not in _RESTATED:
        with torch.no_grad():
            _RESTATED[key] = tuple(tuple(t.cpu() for t in restate(sd, image, image_pe, sparse, dense, multimask, dtype=dt))
                                   for dt in (torch.float64, torch.float32))
    return _RESTATED[key]


DECODER_SHAPES = 6          # cases per precision (asserted below): one test each, so that no test takes more than a second or two


@pytest.mark.parametrize("precision", sc.DECODER_PRECISIONS)
@pytest.mark.parametrize("k", range(DECODER_SHAPES))
def test_decoder_matches_fp64_around_the_prompt_chunk(dev, seams, models, image, k, precision):
    sd, pe, md = models
    image_pe = pe.get_dense_pe()
    mine = [c for c in sc.decoder_cases(seams) if c["precision"] == precision]
    assert len(mine) == DECODER_SHAPES
    case = mine[k]
    sparse, dense = (t.to(dev) for t in sc.decoder_inputs(case))
    P = case["P"]
    md.precision = precision
    try:
        got = md.forward_with_taps(image, image_pe, sparse, dense.expand(P, -1, -1, -1) if dense.shape[0] == 1 else dense, case["multimask"])
    except _lib.PopeHipError as e:
        pytest.exit(f"{case['id']}: {e}", returncode=3)
    finally:
        md.precision = "f16x3"
    _sync(case["id"])
    key = case["id"].replace(precision, "")
    want64, want32 = _restated(sd, image, image_pe, sparse, dense, case["multimask"], key)
    if precision == sc.DECODER_PRECISIONS[-1]:
        del _RESTATED[key]                 # the last precision to need it: up to 400 MB per case
    for name, g, w64, w32 in zip(sc.DECODER_TENSORS, got, want64, want32):
        ratios = sc.chunk_ratios(g.cpu(), w64, w32, seams.chunk)
        sc.report(f"{case['id']} {name}", ratios)
        assert max(ratios) <= 1.0, (case["id"], name, ratios)


def test_second_pass_of_the_image_loop_equals_each_image_alone(dev, seams, models):
    """chunk + 1 images in ONE call of the multi-image entry (MaskDecoder.forward_images splits its calls at 16 images, so the
    call is made through _run_images): bit for bit each image decoded alone, and within the fp64 bound"""
    sd, pe, md = models
    image_pe = pe.get_dense_pe()
    n, which, ns = sc.images_case(seams)
    P = len(which)
    g = torch.Generator().manual_seed(9950)
    images = torch.cat([synth.synthetic_sam_image_embedding(seed=100 + i) for i in range(n)]).to(dev)
    sparse = torch.randn(P, ns, D, generator=g).to(dev)
    dense = (0.5 * torch.randn(D, generator=g)).reshape(1, D, 1, 1).expand(1, D, 64, 64).contiguous().to(dev)
    masks = torch.empty(P, 3, 256, 256, device=dev)
    iou = torch.empty(P, 3, device=dev)
    try:
        md._run_images(images, image_pe.contiguous(), sparse, dense, which, True, masks, iou)
        split_m, split_i = md.forward_images(images, image_pe, sparse, dense, which, True)
    except _lib.PopeHipError as e:
        pytest.exit(f"forward_images: {e}", returncode=3)
    _sync("forward_images")
    assert torch.equal(split_m, masks) and torch.equal(split_i, iou)
    want = [[torch.empty(P, *t.shape[1:], dtype=dt) for t in (masks, iou)] for dt in (torch.float64, torch.float32)]
    for i in range(n):
        idx = torch.tensor([p for p in range(P) if which[p] == i], device=dev)
        m1, i1 = md(images[i:i + 1], image_pe, sparse[idx], dense.expand(idx.numel(), -1, -1, -1), True)
        assert torch.equal(m1, masks[idx]) and torch.equal(i1, iou[idx]), i
        with torch.no_grad():
            for k, dt in enumerate((torch.float64, torch.float32)):
                rm, ri, _, _ = restate(sd, images[i:i + 1], image_pe, sparse[idx], dense, True, dtype=dt)
                want[k][0][idx.cpu()], want[k][1][idx.cpu()] = rm.cpu(), ri.cpu()
    for name, got, w64, w32 in (("masks", masks, want[0][0], want[1][0]), ("iou", iou, want[0][1], want[1][1])):
        ratios = sc.chunk_ratios(got.cpu(), w64, w32, seams.chunk)
        sc.report(f"forward_images N={n} P={P} {name}", ratios)
        assert max(ratios) <= 1.0, (name, ratios)


# ---- bit identities -----------------------------------------------------------------------------------------------------------------
def test_op_entries_are_reproducible_and_batch_invariant_on_the_decoders_own_tensors(dev, hip_lib, seams, models, image):
    """each entry on the decoder's own intermediates (its final tokens hs and image tokens keys): the same bits twice, and prompt
    p of a chunk-wide launch equals the same prompt launched alone"""
    sd, pe, md = models
    P, ns = seams.chunk, 2
    T = seams.base_tokens + ns
    sparse = torch.randn(P, ns, D, generator=torch.Generator().manual_seed(9960)).to(dev)
    dense = (0.5 * torch.randn(D, generator=torch.Generator().manual_seed(9961))).reshape(1, D, 1, 1).expand(P, D, 64, 64).to(dev)
    _, _, hs, keys = md.forward_with_taps(image, pe.get_dense_pe(), sparse, dense, True)
    _sync("taps")
    own = list(range(P))
    g = torch.Generator().manual_seed(9962)
    w, b, pe_t = 1.0 + 0.5 * torch.randn(D, generator=g), 0.5 * torch.randn(D, generator=g), torch.randn(NPIX, D, generator=g)
    ln_w, ln_b, w3, b2 = torch.ones(64), torch.zeros(64), torch.randn(64, 32, 2, 2, generator=g) / 8.0, torch.zeros(32)
    hyper = hs[:, 1:1 + sc.NMASK, :32].contiguous()
    vrows = keys[..., :DI].contiguous()
    tokens = hs.reshape(P * T, D)
    W = sd["mask_decoder.output_hypernetworks_mlps.0.layers.0.weight"]
    bias = sd["mask_decoder.output_hypernetworks_mlps.0.layers.0.bias"]

    def rows(t, p, per):                      # prompt p's rows of a [P * per, ...] tensor
        return t[p * per:(p + 1) * per]

    ops = {
        "self": (lambda: op_self(hip_lib, dev, torch.cat([tokens] * 3, 1), P, T),
                 lambda p: op_self(hip_lib, dev, torch.cat([rows(tokens, p, T)] * 3, 1), 1, T), T),
        "t2i": (lambda: op_t2i(hip_lib, dev, tokens[:, :DI], keys, vrows, own, T, P),
                lambda p: op_t2i(hip_lib, dev, rows(tokens, p, T)[:, :DI], keys[p:p + 1], vrows[p:p + 1], [0], T, 1), T),
        "i2t": (lambda: op_i2t(hip_lib, dev, keys, own, tokens, T, P)[0],
                lambda p: op_i2t(hip_lib, dev, keys[p:p + 1], [0], rows(tokens, p, T), T, 1)[0], NPIX),
        "norm": (lambda: op_norm(hip_lib, dev, keys, own, keys, w, b, pe_t, P)[0],
                 lambda p: op_norm(hip_lib, dev, keys[p:p + 1], [0], keys[p:p + 1], w, b, pe_t, 1)[0], NPIX),
        "tail": (lambda: op_tail(hip_lib, dev, keys, ln_w, ln_b, sc.tail_w2(w3), b2, hyper, 1, P).reshape(P * 3, -1),
                 lambda p: op_tail(hip_lib, dev, keys[p:p + 1], ln_w, ln_b, sc.tail_w2(w3), b2, hyper[p:p + 1], 1, 1).reshape(3, -1), 3),
        # the hypernetwork's first layer as the decoder launches it: row i = mask token 0 of prompt i, ldx = T * 256
        "linear": (lambda: op_lin(hip_lib, dev, hs, D, T * D, None, 0, W, bias, None, P, D, D, True),
                   lambda p: op_lin(hip_lib, dev, hs[p:p + 1], D, T * D, None, 0, W, bias, None, 1, D, D, True), 1),
    }
    for name, (whole, alone, per) in ops.items():
        first, again = whole(), whole()
        assert torch.equal(first, again), name
        assert bool(torch.isfinite(first).all()), name
        for p in (0, P - 1):
            assert torch.equal(alone(p), rows(first, p, per)), (name, p)
    want = torch.relu(torch.nn.functional.linear(hs[:, 1].double(), W.double(), bias.double())).cpu()
    got = ops["linear"][0]()
    assert float((got.double() - want).abs().max()) <= 1e-4 * float(want.abs().max())        # the right token of every prompt
