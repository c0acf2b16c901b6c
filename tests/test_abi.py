"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/pope_hip.h
declares (no compute calls without a GPU); host-only helpers behave like the oracle."""
import os
import re
import subprocess

import numpy as np
import pytest

from pope_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "pope_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pope_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(hip_lib):
    declared = _declared_symbols()
    assert len(declared) >= 12
    for name in declared:
        assert hasattr(hip_lib, name), f"{name} declared in pope_hip.h but not exported"
    assert sorted(_lib.PROTOTYPES) == declared  # the ctypes table covers the whole header


def test_header_is_plain_c():
    # the boundary must be consumable from C (no torch / C++ types in signatures)
    src = "#include \"pope_hip.h\"\nint main(void){return pope_abi_version()==POPE_ABI_VERSION?0:1;}\n"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_code_object_is_gfx950():
    assert _lib.code_object_archs() == ["gfx950"]


def test_abi_version_and_errors(hip_lib):
    assert hip_lib.pope_abi_version() == 10
    assert hip_lib.pope_error_string(0) == b"ok"
    assert b"workspace" in hip_lib.pope_error_string(-3)


def test_workspace_queries(hip_lib):
    # B=64 images of 1531 tokens: xn + max(qkv+attn, fc1) = 5*dim floats per token
    n = hip_lib.pope_vit_workspace_bytes(64, 1531, 384, 1536)
    assert n >= 64 * 1531 * 5 * 384 * 4 and n < 64 * 1531 * 5 * 384 * 4 + 1024
    assert hip_lib.pope_vit_workspace_bytes(0, 1, 1, 1) == 0
    import ctypes
    args = _lib.DenseMatchArgs(n=2, L=1530, S=1530, C=4, precision=_lib.PREC_F32_MFMA, conf_matrix=64)   # conf published
    assert hip_lib.pope_dense_match_workspace_bytes(ctypes.byref(args)) >= 8 * 2 * 1530 * 4
    assert hip_lib.pope_dense_match_workspace_bytes(None) == 0


def test_argument_validation_without_gpu(hip_lib):
    # invalid arguments are rejected before any HIP call is made
    assert hip_lib.pope_layernorm_f32(None, None, None, None, 4, 384, 1e-6, None) == -1
    assert hip_lib.pope_linear_f32(None, None, None, None, 1, 1, 4, 0, None, None, _lib.PREC_F32_MFMA, None, None) == -1
    assert hip_lib.pope_attention_f32(None, None, 1, 1, 6, _lib.PREC_F32_MFMA, None, None) == -1
    # every attention entry shares one argument check; nothing below gets as far as a launch (a null range flag: no scan).
    # The accepting side of a bound cannot be shown here: a call that passes the check launches.
    import ctypes
    buf = ctypes.create_string_buffer(64)
    ok = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, never dereferenced
    count = ctypes.c_longlong(0)
    entries = {
        "f32": lambda q, o, B, N, H: hip_lib.pope_attention_f32(q, o, B, N, H, _lib.PREC_F32_MFMA, None, None),
        "f16x3": lambda q, o, B, N, H: hip_lib.pope_attention_f32(q, o, B, N, H, _lib.PREC_F16X3, None, None),
        "planes": lambda q, o, B, N, H: hip_lib.pope_attention_planes_f32(q, o, B, N, H, None),
        "planes diag": lambda q, o, B, N, H: hip_lib.pope_attention_planes_diag_f32(q, o, B, N, H, ctypes.byref(count), None),
        "f16": lambda q, o, B, N, H: hip_lib.pope_attention_f16(q, o, B, N, H, None),
    }
    for name, call in entries.items():
        for q, o in ((None, ok), (ok, None), (ok + 8, ok), (ok, ok + 8)):      # null, not 16-byte aligned
            assert call(q, o, 1, 64, 6) == -1, (name, q, o)
        for B, N, H in ((0, 64, 6), (-1, 64, 6), (1, 0, 6), (1, -5, 6), (1, 64, 0), (1, 64, -2)):
            assert call(ok, ok, B, N, H) == -1, (name, B, N, H)
        # the qkv image reaches the 32-bit extent of the kernels' buffer descriptor: fp32 and planes rows of 3 * heads * 64 * 4
        # bytes, N * 12288 >= 2^32 from N = 349526 at 16 heads; f16 rows of half that, N + 64 of them, 512 bytes of margin:
        # (N + 64) * 6144 >= 2^32 - 512 from N = 698987
        assert call(ok, ok, 1, 698987 if name == "f16" else 349526, 16) == -1, name
    assert hip_lib.pope_attention_planes_diag_f32(ok, ok, 1, 64, 6, None, None) == -1    # the diagnostic entry needs its counter


def _header_struct_fields(name):
    """Field names of `typedef struct <name> { ... }` in pope_hip.h, in declaration order."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pope_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", d).group(1) for stmt in body.split(";") for d in stmt.split(",") if d.strip()]


def test_dense_match_args_layout(tmp_path):
    """The ctypes mirror of pope_dense_match_args has the C struct's size, field names, field order and offsets (the check the
    positional signatures never had)."""
    import ctypes
    names = _header_struct_fields("pope_dense_match_args")
    assert names == [n for n, _ in _lib.DenseMatchArgs._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"pope_hip.h\"\nint main(void){\n"
    src += "printf(\"%zu\\n\", sizeof(pope_dense_match_args));\n"
    src += "".join("printf(\"%%zu\\n\", offsetof(pope_dense_match_args, %s));\n" % n for n in names) + "return 0;}\n"
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert len(out) == 1 + len(names)
    assert out[0] == ctypes.sizeof(_lib.DenseMatchArgs)
    for n, off in zip(names, out[1:]):
        assert getattr(_lib.DenseMatchArgs, n).offset == off, n


def test_dense_match_refuses_before_any_hip_call(hip_lib):
    """Every refusal of pope_dense_match_f32 is decided on the host: fake aligned pointers that are never dereferenced, no GPU.
    (The accepting side launches; the GPU suites cover it.)"""
    import ctypes
    import itertools
    buf = ctypes.create_string_buffer(64)
    ok = (ctypes.addressof(buf) + 15) & ~15
    ERR_ARG, ERR_WORKSPACE = -1, -3
    required = ("feat0", "feat1", "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "counts", "workspace")
    n, L, S, Cd = 2, 192, 140, 256
    for sinkhorn, border, publish in itertools.product((False, True), repeat=3):
        def make(**over):
            a = _lib.DenseMatchArgs(
                feat0=ok, stride0=L * Cd, feat1=ok, stride1=S * Cd, n=n, L=L, S=S, C=Cd, h0=12, w0=16, h1=10, w1=14, thr=0.2,
                border_rm=2, temperature=0.1, scale=8.0, match_type=_lib.MATCH_TYPES["sinkhorn" if sinkhorn else "dual_softmax"],
                bin_score=ok if sinkhorn else None, skh_iters=3, skh_prefilter=1, border_mask0=ok if border else None,
                border_mask1=ok if border else None, conf_matrix=ok if publish else None, b_ids=ok, i_ids=ok, j_ids=ok,
                mconf=ok, mkpts0_c=ok, mkpts1_c=ok, counts=ok, workspace=ok, precision=_lib.PREC_F16X3)
            a.workspace_bytes = hip_lib.pope_dense_match_workspace_bytes(ctypes.byref(a))
            for k, v in over.items():
                setattr(a, k, v)
            return a
        call = lambda a: hip_lib.pope_dense_match_f32(ctypes.byref(a), None)   # noqa: E731
        case = (sinkhorn, border, publish)
        need = make().workspace_bytes
        assert need > 0, case
        assert call(make(workspace_bytes=need - 1)) == ERR_WORKSPACE, case
        for name in required:
            assert call(make(**{name: None})) == ERR_ARG, (case, name)
        assert call(make(n=0)) == ERR_ARG, case
        assert call(make(match_type=2)) == ERR_ARG, case
        assert call(make(match_type=-1)) == ERR_ARG, case
        if sinkhorn:
            assert call(make(bin_score=None)) == ERR_ARG, case
            assert call(make(skh_iters=0)) == ERR_ARG, case
    assert hip_lib.pope_dense_match_f32(None, None) == ERR_ARG


def test_streaming_top3_host_matches_oracle(golden_dir):
    from oracle import coarse_match_ref as cm
    from pope_amd import ops
    fx = np.load(os.path.join(golden_dir, "top3.npz"))
    slots, idx = ops.streaming_top3(fx["scores"])
    assert np.array_equal(slots, fx["slot_scores"]) and np.array_equal(idx, fx["slot_index"])
    rng = np.random.default_rng(0)
    for _ in range(50):
        s = rng.uniform(-0.2, 1.0, size=rng.integers(0, 12)).astype(np.float32)
        s[rng.random(s.size) < 0.3] = 0.5  # ties
        a, b = ops.streaming_top3(s)
        c, d = cm.streaming_top3(s)
        assert np.array_equal(a, c) and np.array_equal(b, d)


def test_product_fails_loudly_on_cpu(sd0):
    import torch
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd._lib import PopeHipError
    model = load_dinov2_model(state_dict=sd0)
    assert len(model.state_dict()) == 175
    with pytest.raises(PopeHipError):
        model(torch.zeros(1, 3, 28, 28))


def test_product_never_imports_oracle():
    import pathlib
    for p in pathlib.Path(ROOT, "pope_amd").rglob("*.py"):
        assert "oracle" not in p.read_text().replace("no CPU oracle", ""), p


def test_library_has_no_environment_switches(hip_lib):
    """`pope_hip.h` promises no global state: the shipped library must not read the environment (round 3 carried seven
    `getenv("POPE_...")` dev switches that selected kernels no test ran) and its kernel sources must not carry timing
    ablations ("wrong results" builds) — lab variants are compiled from scripts/ with their own flags."""
    import glob
    import os
    import re
    from pope_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    assert not re.search(rb"POPE_[A-Z0-9_]{3,}", blob), "an environment / macro name survives in the binary"
    csrc = os.path.dirname(_lib.LIB_PATH)
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        text = open(path).read()
        assert "getenv" not in text, path
        assert not re.search(r"#\s*if(n?def)?\b[^\n]*(_ABL_|_LAB\b|NO_EPILOGUE|NOSTORE|L1ONLY)", text), path
