"""The comparisons of test_gpu_gemm_f16_routes.py (gemm_f16_checks.py) accept an fp64 result stored in each output format and
reject it with the faults a plain-f16 GEMM epilogue is likely to have, on the operands and at the shapes the GPU test uses; and
pope_linear_f16 rejects every call outside its contract before any HIP call.  Host only."""
import ctypes

import pytest
import torch

import gemm_f16_checks as K

FAULTS = ("q_scale_one_group_more", "q_scale_one_group_less", "q_rounded_before_scaling", "last_k_step_dropped",
          "bias_shifted_in_ragged_column_tile", "row_tile_shifted")


def _ref(op, epi, rows, bias=True, a16=None, w16=None, b=None):
    a16 = op["a16"] if a16 is None else a16
    return K.ref64(a16[rows], op["w16"] if w16 is None else w16, (op["bias"] if b is None else b) if bias else None, epi,
                   op["gamma"], op["res"][rows])


def _faulty(fault, op, epi, M, N, K_, rows, route):
    """The stored output of a kernel with `fault` and no other error, at `rows`."""
    if fault in ("q_scale_one_group_more", "q_scale_one_group_less"):
        lin = _ref(op, K.EPI_BIAS, rows)
        edge = N // 3 + (4 if fault.endswith("more") else -4)
        return K.stored(lin * torch.where(torch.arange(N) < edge, K.QSCALE, 1.0).double(), epi)
    if fault == "q_rounded_before_scaling":
        lin = _ref(op, K.EPI_BIAS, rows)
        q = (lin[:, :N // 3].half().float() * torch.tensor(K.QSCALE, dtype=torch.float32)).half()   # two roundings, as a kernel would
        return torch.cat([q, lin[:, N // 3:].half()], dim=1)
    if fault == "last_k_step_dropped":
        return K.stored(_ref(op, epi, rows, a16=op["a16"][:, :K_ - 64], w16=op["w16"][:, :K_ - 64]), epi)
    if fault == "bias_shifted_in_ragged_column_tile":
        c0 = (N - 1) // 128 * 128      # the last, partial 128 columns: ragged under 128- and 256-column tiles alike
        b = op["bias"].clone()
        b[c0:N - 1] = op["bias"][c0 + 1:]
        return K.stored(_ref(op, epi, rows, b=b), epi)
    if fault == "row_tile_shifted":
        t = K.TILE_ROWS[route]
        last0 = (M - 1) // t * t
        src = rows.clone()
        sel = (rows >= last0 + 1) if M - last0 > 1 else (rows >= 1) & (rows < t)      # a one-row last tile: shift the first
        src[sel] -= 1
        a = op["a16"][src]
        return K.stored(K.ref64(a, op["w16"], op["bias"], epi, op["gamma"], op["res"][rows]), epi)
    raise ValueError(fault)


def _applies(fault, epi, N):
    if fault.startswith("q_"):
        return epi == K.EPI_QKV
    if fault == "bias_shifted_in_ragged_column_tile":
        return N % 128 != 0
    return True


CPU_CASES = [(epi, M, N, K_) for (epi, M, N, K_) in K.CASES if M in (2047, 2049, 129)]


@pytest.mark.parametrize("case", CPU_CASES, ids=K.case_id)
def test_checks_accept_the_stored_reference_and_reject_each_fault(case):
    epi, M, N, K_ = case
    op = K.operands(M, N, K_)
    route = K.plain_route(M, N, K_, epi)
    rows = K.check_rows_of(M, route)
    want = _ref(op, epi, rows)
    err, frac = K.check_out(K.stored(want, epi), want, epi, "stored reference")
    assert frac <= 1.0
    for fault in FAULTS:
        if not _applies(fault, epi, N):
            continue
        with pytest.raises(AssertionError) as e:
            K.check_out(_faulty(fault, op, epi, M, N, K_, rows, route), want, epi, fault)
        print(f"{K.case_id(case)} {fault}: {str(e.value)[:150]}")


@pytest.mark.parametrize("M,N,K_", K.RES_MOD_CASES)
def test_checks_reject_the_wrong_table_row(M, N, K_):
    """res_mod: the residual row taken as row % 288 instead of row % 289."""
    op = K.operands(M, N, K_)
    rows = K.check_rows_of(M, K.plain_route(M, N, K_, K.EPI_LS_RES))
    ones = torch.ones(N)
    want = K.ref64(op["a16"][rows], op["w16"], op["bias"], K.EPI_LS_RES, ones, op["table"][rows % K.RES_MOD])
    K.check_f32(want.float(), want, "stored reference")
    wrong = K.ref64(op["a16"][rows], op["w16"], op["bias"], K.EPI_LS_RES, ones, op["table"][rows % (K.RES_MOD - 1)])
    with pytest.raises(AssertionError):
        K.check_f32(wrong.float(), want, "row % 288")
    # rows below 288 are the same under both moduli: the compared rows must reach past them
    assert int((rows >= K.RES_MOD - 1).sum()) > 0


def test_ulp_f16_is_the_spacing_of_torch_half():
    v = torch.tensor([1.0, 1.5, 2.0, 0.999, 1023.0, 1024.0, 65472.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 0.0, -3.0, 11818.0])
    want = []
    for x in v.half():
        b = x.abs().view(torch.int16)
        want.append(float((b + 1).view(torch.float16)) - float(b.view(torch.float16)))
    assert K.ulp_f16(v).tolist() == want


def test_route_mirror_straddles_the_switch():
    for epi in K.NK:
        for N, K_ in K.NK[epi]:
            wide = N >= 256 and N % 64 == 0
            assert K.plain_route(2047, N, K_, epi) == "tile16"
            assert K.plain_route(2048, N, K_, epi) == ("plain256" if wide else "tile16")
    assert {K.plain_route(M, N, K_, K.EPI_LS_RES) for M, N, K_ in K.RES_MOD_CASES} == {"plain256", "tile16"}
    assert max(M * N * K_ for M, N, K_ in K.RES_MOD_CASES) == 2312 * 1152 * 1536      # the largest case


def test_linear_f16_argument_validation_without_gpu(hip_lib):
    """Every rejection of pope_linear_f16's contract returns POPE_ERR_ARG before the stream's device is touched (this machine
    has none); the pointers are never dereferenced."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    M, N, K_ = 300, 384, 128

    def call(a=p, w=p, bias=p, C=None, c16=None, M=M, N=N, K_=K_, epi=K.EPI_BIAS, gamma=None, res=None, res_mod=0):
        return hip_lib.pope_linear_f16(a, w, bias, C, c16, M, N, K_, epi, gamma, res, res_mod, None, None)

    bad = {
        "null A": call(a=None, C=p), "null W": call(w=None, C=p),
        "epilogue 3": call(C=p, epi=3), "epilogue -1": call(C=p, epi=-1), "epilogue 11 (SwiGLU)": call(C=p, epi=11),
        "epilogue 6": call(c16=p, epi=6),
        "BIAS without C": call(), "BIAS to f16": call(c16=p), "BIAS with both": call(C=p, c16=p),
        "GELU to fp32": call(C=p, epi=K.EPI_GELU), "GELU with both": call(C=p, c16=p, epi=K.EPI_GELU),
        "QKV to fp32": call(C=p, epi=K.EPI_QKV), "QKV without output": call(epi=K.EPI_QKV),
        "LS_RES to f16": call(c16=p, epi=K.EPI_LS_RES, gamma=p, res=p),
        "K=64": call(C=p, K_=64), "K=0": call(C=p, K_=0), "K=160": call(C=p, K_=160), "K=96": call(C=p, K_=96),
        "N=386 fp32": call(C=p, N=386), "N=0": call(C=p, N=0), "N=352 GELU": call(c16=p, N=352, epi=K.EPI_GELU),
        "N=324 GELU": call(c16=p, N=324, epi=K.EPI_GELU),
        "N=320 QKV": call(c16=p, N=320, epi=K.EPI_QKV), "N=256 QKV": call(c16=p, N=256, epi=K.EPI_QKV),
        "LS_RES without res": call(C=p, epi=K.EPI_LS_RES, gamma=p),
        "LS_RES without gamma or table": call(C=p, epi=K.EPI_LS_RES, res=p),
        "LS_RES res_mod -1 without gamma": call(C=p, epi=K.EPI_LS_RES, res=p, res_mod=-1),
        "M=0": call(C=p, M=0), "M=-3": call(c16=p, M=-3, epi=K.EPI_GELU),
    }
    for what, rc in bad.items():
        assert rc == -1, what
