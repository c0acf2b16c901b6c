"""CPU: the rig of test_gpu_sam_decoder_seams.py (tests/sam_decoder_checks.py) is sound — the case lists hold every seam value of
the mask decoder's kernels, the inputs reach the regime each case is about (asserted in fp64), the comparison accepts fp32
restatements that sum in the kernels' order and rejects every planted fault, on the same data, in at least the case built for it.

Worst ratio of the kernel-order fp32 restatements (this file, -s): self 0.54, token -> image 0.53, image -> token 0.41, residual
norm 0.26, tail 0.97 (offset rows: 64 channels summed in one chain) of the bound; the linear's inputs lie on a grid where every
order of summation gives the same bits (sam_decoder_checks.py), ratio 0."""
import functools

import pytest
import torch

import sam_decoder_checks as sc


@pytest.fixture(scope="module")
def seams(hip_lib):
    s = sc.read_seams(hip_lib)
    assert s.chunk > 2 and s.lin_rows > 1 and s.max_tokens > s.base_tokens + 3 > 3
    return s


@functools.lru_cache(maxsize=None)
def _attention(case_id, s):
    case = next(k for k in sc.attention_cases(s) if k["id"] == case_id)
    x = sc.attention_inputs(case)
    return case, x, sc.attention_ref(case, *x), sc.attention_ref(case, *x, dtype=torch.float32)


def _case(cases, **want):
    """the first case with these fields"""
    return next(k for k in cases if all(k[f] == v for f, v in want.items()))


# ---- the case lists -------------------------------------------------------------------------------------------------------------
def test_case_lists_hold_every_seam(seams):
    s = seams
    Ts, Ps = sc.token_counts(s), sc.launch_prompts(s)
    assert Ts == (s.base_tokens, s.base_tokens + 1, s.base_tokens + 2, s.base_tokens + 3, s.max_tokens - 1, s.max_tokens)
    assert Ps == (1, 2, s.chunk)
    att = sc.attention_cases(s)
    assert len({k["id"] for k in att}) == len(att)
    for kernel in ("self", "t2i", "i2t"):
        mine = [k for k in att if k["kernel"] == kernel]
        unit = [k for k in mine if k["regime"] == "unit" and not k["slots"]]
        assert {k["T"] for k in unit} == set(Ts) and {k["P"] for k in unit} == set(Ps)
        assert {"shift_up", "shift_down"} <= {k["regime"] for k in mine}
        if kernel == "t2i":
            assert {k["ldk"] for k in unit} == {sc.D, sc.DI}
            peaks = [k for k in mine if k["regime"].startswith("peak_in_wave_")]
            assert [k["regime"] for k in peaks] == [f"peak_in_wave_{w}" for w in range(4)]
            covered = set()
            for w, k in enumerate(peaks):
                a, b = k["peaks"]
                assert a % sc.THREADS == b % sc.THREADS and a // sc.THREADS != b // sc.THREADS      # one thread's keys, different i
                assert (a % sc.THREADS) // sc.WAVE == w
                covered |= {a, b}
            assert covered >= {0, 255, 256, 4095}
        else:
            for T in (Ts[0], Ts[-1]):
                assert {k["peaks"] for k in mine if k["regime"].startswith("peak_at_token") and k["T"] == T} == {(0,), (T - 1,)}
        if kernel != "self":
            slotted = [k for k in mine if k["slots"]]
            assert slotted and all(k["slots"] == (2, 0, 1, 1) and k["P"] == 4 for k in slotted)
    lin = sc.linear_cases(s)
    assert len({k["id"] for k in lin}) == len(lin)
    plain = [k for k in lin if k["token"] is None]
    L = s.lin_rows
    assert {k["M"] for k in plain} == {1, L - 1, L, L + 1, 2 * L + 1}
    assert {(k["N"], k["K"], k["add_cols"]) for k in plain} == {(768, 256, 512), (768, 256, 0), (128, 256, 128), (256, 128, 0), (2048, 256, 0),
                                                              (256, 2048, 0), (32, 256, 0), (3, 256, 0), (1, 256, 0)}
    for M in sc.linear_rows(s):
        for shape in sc.LIN_SHAPES:
            assert {(k["relu"], k["res"]) for k in plain if k["M"] == M and (k["N"], k["K"], k["add_cols"]) == shape} == \
                {(False, False), (False, True), (True, False), (True, True)}
    strided = [k for k in lin if k["token"] is not None]
    assert strided and all(k["token"] >= 1 and k["T"] in Ts for k in strided)
    norm = sc.norm_cases(s)
    assert {k["regime"] for k in norm} == set(sc.NORM_REGIMES) and {k["P"] for k in norm if not k["slots"]} == set(Ps)
    assert any(k["slots"] == (2, 0, 1, 1) for k in norm)
    assert {(k["nz"], k["walk"]) for k in sc.prep_cases()} == {(1, "image"), (3, "image"), (1, "dense"), (3, "dense")}
    tail = sc.tail_cases()
    assert {k["regime"] for k in tail} == set(sc.NORM_REGIMES)
    assert {(k["P"], k["multimask"]) for k in tail} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    dec = sc.decoder_cases(s)
    for prec in sc.DECODER_PRECISIONS:
        mine = [k for k in dec if k["precision"] == prec]
        assert {k["P"] for k in mine} == {s.chunk - 1, s.chunk, s.chunk + 1, 2 * s.chunk + 1}
        assert {k["n_sparse"] for k in mine} == {0, 1, 2, 3, s.max_tokens - s.base_tokens}
        assert {k["dense"] for k in mine} == {"broadcast", "per_prompt"} and {k["multimask"] for k in mine} == {True, False}
    n, which, ns = sc.images_case(s)
    assert n == s.chunk + 1 and set(which) == set(range(n)) and len(which) > s.chunk and which != sorted(which)
    assert {which.count(i) for i in range(n)} == {1, 2}


def test_op_entries_refuse_bad_arguments_without_a_gpu(hip_lib, seams):
    sc.assert_refusals(hip_lib, seams)


# ---- the regimes ----------------------------------------------------------------------------------------------------------------
def test_attention_inputs_reach_their_regimes(seams):
    for k in sc.attention_cases(seams):
        case, x, _, _ = _attention(k["id"], seams)
        s = sc.attention_scores(case, *x)
        regime = case["regime"]
        if regime == "unit":
            assert 1.5 < float(s.std()) < 2.5, (case["id"], float(s.std()))
        elif regime == "shift_up":
            assert 90 < float(s.min()) and float(s.max()) < 210, case["id"]
        elif regime == "shift_down":
            assert -210 < float(s.min()) and float(s.max()) < -90, case["id"]
        else:
            peaks = list(case["peaks"])
            rest = [j for j in range(s.shape[-1]) if j not in peaks]
            top, others = s[..., peaks], s[..., rest].max(-1).values
            if case["kernel"] == "t2i":
                assert float((top[..., 0] - top[..., 1]).abs().max()) <= 1.0 and float((top[..., 0] - top[..., 1]).abs().min()) > 0.1
                assert float((top.min(-1).values - others).min()) >= 100.0, case["id"]
            else:                       # one token well above the others, far from one-hot
                gap = top[..., 0] - others
                assert float(gap.median()) > 3.0 and float(gap.median()) < sc.TOKEN_PEAK, (case["id"], float(gap.median()))
    _, q, k, v, slots = sc.i2t_flag_case(seams)
    assert float(v.abs().min()) > sc.PLANES_LIMIT


def test_norm_and_tail_inputs_reach_their_regimes(seams):
    for case in sc.norm_cases(seams)[:6:2] + sc.norm_cases(seams)[-1:]:
        res, y, w, b, pe_t, slots = sc.norm_inputs(case)
        x = res.double()[torch.tensor(slots)] + y.double()
        _check_rows(case, x, sc.TOKEN_EPS)
        assert float((pe_t[1:] - pe_t[:-1]).abs().max(1).values.min()) > 0.5          # no two neighbouring rows of pe alike
    for case in sc.tail_cases():
        y, ln_w, ln_b, w3, b2, hyper = sc.tail_inputs(case)
        _check_rows(case, y.double().reshape(-1, 64), sc.UP_EPS)
        gains = hyper.abs().amax((0, 2))
        assert gains[1] > 3 * gains[0] > 9 * gains[2] and gains[3] > 3 * gains[1]
        assert torch.equal(sc.tail_w2(w3)[2 * 32 + 5, 9], w3[9, 5, 1, 0])            # row tap * 32 + c, tap = 2 dy + dx
    norm = sc.norm_cases(seams)[0]
    res, y, w, b, pe_t, slots = sc.norm_inputs(norm)
    keys, _ = sc.norm_ref(res, y, sc.norm_flag_weight(w), b, pe_t, slots)
    assert float(keys.abs().max()) > sc.PLANES_LIMIT
    assert float(sc.norm_ref(res, y, w, b, pe_t, slots)[1].abs().max()) < sc.PLANES_LIMIT


def _check_rows(case, x, eps):
    mean, var = x.mean(-1), x.var(-1, unbiased=False)
    if case["regime"] == "unit":
        assert float(mean.abs().max()) < 1.0 and 0.4 < float(var.min()) and float(var.max()) < 2.5, case["id"]
    elif case["regime"] == "offset":    # mean^2 / var ~ 1e8: beyond what a one-pass fp32 variance resolves
        assert float((mean - sc.OFFSET).abs().max()) < 0.01 and float(var.max()) < 4 * sc.OFFSET_STD ** 2, case["id"]
        assert float(var.min()) > sc.OFFSET_STD ** 2 / 4
    else:
        assert float(var.max()) < eps / 25, (case["id"], float(var.max()))


# ---- accepted: fp32 in the kernels' order -----------------------------------------------------------------------------------------
def test_comparison_accepts_the_kernel_order_in_fp32(seams):
    worst = {}

    def note(kind, cid, ratios):
        assert max(ratios) <= 1.0, (cid, ratios)
        worst[kind] = max(worst.get(kind, (-1.0, "")), (max(ratios), cid))

    for k in sc.attention_cases(seams):
        if k["P"] == seams.chunk and k["T"] != seams.max_tokens:
            continue                    # the order within a prompt is that of the smaller launches: one chunk-wide case per kernel
        case, x, want64, want32 = _attention(k["id"], seams)
        note(case["kernel"], case["id"], sc.head_ratios(sc.attention_kernel_order(case, *x), want64, want32))
    for case in sc.linear_cases(seams):
        if case["M"] != 2 * seams.lin_rows + 1 or not (case["relu"] and case["res"]):
            continue
        _, X, _, add, W, bias, res = sc.linear_inputs(case)
        got = sc.linear_ref(case, X, add, W, bias, res, torch.float32, in_order=True)
        note("linear", case["id"], sc.column_block_ratios(got, sc.linear_ref(case, X, add, W, bias, res),
                                                          sc.linear_ref(case, X, add, W, bias, res, torch.float32)))
    for case in sc.norm_cases(seams):
        if case["P"] == seams.chunk:
            continue
        x = sc.norm_inputs(case)
        got, w64, w32 = (sc.norm_ref(*x, dtype=torch.float32, in_order=True), sc.norm_ref(*x), sc.norm_ref(*x, dtype=torch.float32))
        note("norm", case["id"], [sc.group_ratio(g, a, b) for g, a, b in zip(got, w64, w32)])
    for case in sc.tail_cases():
        if case["P"] != 1:
            continue
        x = sc.tail_inputs(case)
        got = sc.tail_ref(case, *x, dtype=torch.float32, in_order=True)
        note("tail", case["id"], sc.tail_ratios(got, sc.tail_ref(case, *x), sc.tail_ref(case, *x, dtype=torch.float32)))
    for kind, (ratio, cid) in worst.items():
        print(f"kernel-order fp32 restatement, {kind}: worst ratio {ratio:.3f} at {cid}")


# ---- rejected: the planted faults ---------------------------------------------------------------------------------------------------
def _attention_rejects(seams, fault, **want):
    k = _case(sc.attention_cases(seams), **want)
    case, x, want64, want32 = _attention(k["id"], seams)
    ok = sc.head_ratios(sc.attention_kernel_order(case, *x), want64, want32)
    bad = sc.head_ratios(sc.attention_kernel_order(case, *x, fault=fault), want64, want32)
    assert max(ok) <= 1.0 and max(bad) > 1.0, (case["id"], fault, max(ok), max(bad))
    return max(bad)


@pytest.mark.parametrize("kernel", ["self", "t2i", "i2t"])
def test_attention_faults_are_rejected(seams, kernel):
    Ts = sc.token_counts(seams)
    for regime in ("shift_up", "shift_down"):
        assert _attention_rejects(seams, "no_max", kernel=kernel, regime=regime) == float("inf")
    _attention_rejects(seams, "scale", kernel=kernel, regime="unit", T=Ts[1])
    if kernel == "t2i":
        for w in range(4):              # a maximum that misses the wave of the only peaks: exp overflows
            assert _attention_rejects(seams, f"max_missing_wave_{w}", kernel=kernel, regime=f"peak_in_wave_{w}") == float("inf")
        _attention_rejects(seams, "last_256_keys_dropped", kernel=kernel, regime="unit", T=Ts[0])
        _attention_rejects(seams, "last_256_keys_dropped", kernel=kernel, regime="peak_in_wave_3")
    else:
        for T in (Ts[0], Ts[-1]):
            _attention_rejects(seams, "last_token_dropped", kernel=kernel, regime=f"peak_at_token_{T - 1}", T=T)
            _attention_rejects(seams, "last_token_dropped", kernel=kernel, regime="unit", T=T)
        _attention_rejects(seams, "kv_swapped", kernel=kernel, regime="unit", T=Ts[2])
    if kernel != "self":
        _attention_rejects(seams, "wrong_slot", kernel=kernel, slots=sc.SLOT_MAP)


def test_linear_faults_are_rejected(seams):
    cases = sc.linear_cases(seams)
    M = seams.lin_rows + 1

    def rejects(fault, **want):
        case = _case(cases, M=M, **want)
        _, X, _, add, W, bias, res = sc.linear_inputs(case)
        w64, w32 = sc.linear_ref(case, X, add, W, bias, res), sc.linear_ref(case, X, add, W, bias, res, torch.float32)
        bad = sc.linear_ref(case, X, add, W, bias, res, torch.float32, fault=fault)
        assert max(sc.column_block_ratios(bad, w64, w32)) > 1.0, (case["id"], fault)

    rejects("add_cols_off_by_a_block", N=768, add_cols=512, relu=False, res=False)
    rejects("add_cols_off_by_a_block", N=128, add_cols=128, relu=False, res=False)
    rejects("no_relu", N=2048, relu=True, res=False)
    rejects("no_relu", N=1, relu=True, res=True)
    rejects("res_pitch", N=256, K=2048, relu=False, res=True)
    rejects("res_pitch", N=3, relu=True, res=True)


def test_norm_faults_are_rejected(seams):
    cases = sc.norm_cases(seams)

    def rejects(fault, **want):
        case = _case(cases, **want)
        x = sc.norm_inputs(case)
        w64, w32 = sc.norm_ref(*x), sc.norm_ref(*x, dtype=torch.float32)
        bad = sc.norm_ref(*x, dtype=torch.float32, fault=fault)
        ratios = [sc.group_ratio(g, a, b) for g, a, b in zip(bad, w64, w32)]
        return case, ratios

    case, ratios = rejects("one_pass_variance", regime="offset", P=1)
    assert min(ratios) > 1.0, ratios
    case, ratios = rejects("no_eps", regime="tiny", P=1)
    assert min(ratios) > 1.0, ratios
    case, ratios = rejects("pe_of_the_wrong_row", regime="unit", P=2)
    assert ratios[0] <= 1.0 < ratios[1], ratios                      # the keys are right, operand B is not
    case, ratios = rejects("wrong_slot", slots=sc.SLOT_MAP)
    assert min(ratios) > 1.0, ratios


def test_tail_faults_are_rejected():
    cases = sc.tail_cases()

    def rejects(fault, **want):
        case = _case(cases, **want)
        x = sc.tail_inputs(case)
        w64, w32 = sc.tail_ref(case, *x), sc.tail_ref(case, *x, dtype=torch.float32)
        ratios = sc.tail_ratios(sc.tail_ref(case, *x, dtype=torch.float32, fault=fault), w64, w32)
        assert max(ratios) > 1.0, (case["id"], fault, max(ratios))
        return ratios, case

    rejects("tanh_gelu", regime="unit", P=1)
    ratios, case = rejects("taps_transposed", regime="unit", P=1)
    C = 3 if case["multimask"] else 1
    sub = torch.tensor(ratios[C:C + 16]).reshape(4, 4)               # mask 0's sub-pixel groups [oy % 4, ox % 4]
    assert bool((sub[0, 0] <= 1.0) and (sub[0, 1] > 1.0) and (sub[1, 0] > 1.0) and (sub[3, 3] <= 1.0))      # only dy != dx moves
    rejects("m0_ignored", regime="unit", P=2, multimask=1)
    rejects("one_pass_variance", regime="offset", P=1)
    rejects("no_eps", regime="tiny", P=1)


def test_the_quiet_mask_is_judged_by_its_own_bound():
    """an error a loud mask's bound would hide: 1e-3 of the quiet mask's scale on the quiet mask alone"""
    case = _case(sc.tail_cases(), regime="unit", P=2, multimask=1)
    x = sc.tail_inputs(case)
    w64, w32 = sc.tail_ref(case, *x), sc.tail_ref(case, *x, dtype=torch.float32)
    quiet = 1                                                         # selected masks 1, 2, 3 carry the gains 10, 0.1, 100
    bad = w32.clone()
    bad[:, quiet] *= 1.0 + 1e-3
    ratios = sc.tail_ratios(bad, w64, w32)
    assert ratios[quiet] > 1.0 and ratios[0] <= 1.0 and ratios[2] <= 1.0
    pooled = sc.group_ratio(bad, w64, w32)
    assert pooled <= 1.0                                              # one bound over all masks lets it pass
