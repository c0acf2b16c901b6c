"""CPU: the host side of the MoCoPE fusion pose model (pope_amd/mocope.py, mocope.hip's C entries) — exported prototypes, the
state-dict layout against the names the fixture recorded from the reference, and argument checks that need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pope_amd import _lib, convnextv2, synth
from pope_amd.mocope import MoCoPE, regress_pose_fused_batch


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mocope.npz"))


def _model(S, mode="6d", **kw):
    return MoCoPE(S, mode, backbone=convnextv2.ConvNeXtV2(**synth.MOCOPE_TRUNK), **kw)


def test_library_exports_the_entries(hip_lib):
    assert hip_lib.pope_abi_version() == 10
    for name in ("pope_mocope_workspace_bytes", "pope_mocope_forward_f32", "pope_mocope_tap_f32"):
        fn = getattr(hip_lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args
    assert len(_lib.PROTOTYPES["pope_mocope_forward_f32"][1]) == 21 and len(_lib.PROTOTYPES["pope_mocope_tap_f32"][1]) == 21
    # the struct is what the header declares: 2 ints, three transformers of 6 x 12 + 2 + 6 x 18 + 2 pointers, 24 more pointers
    assert ctypes.sizeof(_lib.MocopeWeights) == 8 + 8 * (3 * (72 + 2 + 108 + 2) + 24)


@pytest.mark.parametrize("mode", list(synth.POSE_REGRESSOR_MODES))
def test_state_dict_keys_are_the_reference_s(gold, mode):
    want = list(zip(str(gold[f"keys_S5_{mode}.names"]).split("\n"), str(gold[f"keys_S5_{mode}.shapes"]).split("\n")))
    assert len(want) == 576
    model = _model(5, mode)
    sd = model.state_dict()
    got = [(k, "x".join(str(d) for d in v.shape)) for k, v in sd.items() if not k.startswith("convnextv2.")]
    assert got == want
    assert [(k, "x".join(str(d) for d in s)) for k, s in synth.mocope_keys(5, mode)] == want
    # the backbone sits where the reference keeps it, between mlp1 and mlp_img
    names = list(sd)
    trunk = [k for k in names if k.startswith("convnextv2.")]
    assert trunk == ["convnextv2.model." + k for k, _ in synth.convnext_keys(**synth.MOCOPE_TRUNK)]
    assert names.index(trunk[0]) == names.index("mlp1.3.bias") + 1 and names.index(trunk[-1]) + 1 == names.index("mlp_img.0.weight")
    model.load_state_dict(synth.mocope_state_dict(5, mode), strict=True)


def test_inference_only_and_no_cpu_path():
    model = _model(5)
    assert not model.training
    with pytest.raises(NotImplementedError):
        model.train()
    model.eval()
    z, img = torch.zeros(1, 5, 2), torch.zeros(1, 3, 64, 64)
    with pytest.raises(_lib.PopeHipError):
        model(z, z, img, img)
    with pytest.raises(_lib.PopeHipError):
        regress_pose_fused_batch(model, torch.zeros(4, 2), torch.zeros(4, 2), [4], img, img)
    with pytest.raises(ValueError):
        MoCoPE(5, "euler")
    with pytest.raises(ValueError):
        MoCoPE(5, train_type="imgs")
    with pytest.raises(ValueError):
        MoCoPE(5, backbone=convnextv2.ConvNeXtV2(**synth.CONVNEXT_SMALL))     # a 32-class head


def test_a_call_of_65_pairs_is_refused():
    z = torch.zeros(65, 5, 2)      # the group check comes before the device check: no launch is attempted
    with pytest.raises(NotImplementedError):
        _model(5)(z, z, None, None)


def test_c_entries_refuse_bad_arguments_without_a_gpu(hip_lib):
    buf = ctypes.create_string_buffer(1 << 16)
    ok = (ctypes.addressof(buf) + 255) & ~255
    fwd, tap = hip_lib.pope_mocope_forward_f32, hip_lib.pope_mocope_tap_f32
    S = 5
    w = _lib.MocopeWeights()
    w.num_sample, w.mode = S, 2

    def fill(struct):      # every pointer of the weights struct non-null and 16-byte aligned
        for name, typ in struct._fields_:
            v = getattr(struct, name)
            if typ is ctypes.c_void_p:
                setattr(struct, name, ok)
            elif isinstance(v, ctypes.Array):
                for i in range(len(v)):
                    if isinstance(v[i], ctypes.Structure):
                        fill(v[i])
                    else:
                        v[i] = ok
            elif isinstance(v, ctypes.Structure):
                fill(v)
    big = 1 << 40

    def call(weights=w, d0=ok, d1=ok, counts=None, f0=ok, f1=ok, B=2, S_arg=S, G=2, tt=0, t=ok, R=ok, st=ok, ws=ok, nbytes=big):
        return fwd(ctypes.byref(weights) if weights is not None else None, d0, d1, None, None, counts, None, None, f0, f1, B, S_arg, G, 0, tt,
                   t, R, st, ws, nbytes, None)
    assert call() == -1                                   # every weight pointer null
    fill(w)
    w.num_sample, w.mode = S, 2
    # from here on only the named argument is wrong: each call would reach the device if it were accepted, so each is paired
    # with the check that it was not (-1 / -3, and the process is still alive without a GPU)
    assert call(weights=None) == -1
    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(S_arg=0) == -1 and call(S_arg=S + 1) == -1
    assert call(G=0) == -1 and call(G=65) == -1 and call(B=3, G=2) == -1
    assert call(tt=3) == -1 and call(tt=-1) == -1
    assert call(d0=None) == -1 and call(counts=ok) == -1        # neither / both input forms
    assert call(f0=None) == -1 and call(f1=None) == -1
    assert call(t=None) == -1 and call(R=None) == -1 and call(st=None) == -1
    assert call(ws=None) == -1 and call(ws=ok + 16) == -1
    need = hip_lib.pope_mocope_workspace_bytes(2, S)
    assert call(nbytes=need - 1) == -3
    w.mode = 3
    assert call() == -1
    w.mode = 2
    w.mkpts_as_q.dec[5].cross_out_proj_b = None
    assert call() == -1
    w.mkpts_as_q.dec[5].cross_out_proj_b = ok + 4                # misaligned
    assert call() == -1
    w.mkpts_as_q.dec[5].cross_out_proj_b = ok

    def call_tap(stage, tt=0, out=ok):
        return tap(ctypes.byref(w), ok, ok, None, None, None, None, None, ok, ok, 2, S, 2, 0, tt, stage, out, ok, ok, need - 1, None)
    # a stage the entry knows and the route computes gets as far as the workspace size (-3); the others stop at -1
    assert [call_tap(s) for s in range(7)] == [-3] * 7
    assert call_tap(-1) == -1 and call_tap(7) == -1 and call_tap(0, out=None) == -1
    assert [call_tap(s, tt=1) for s in range(7)] == [-3, -3, -3, -3, -1, -3, -1]
    assert [call_tap(s, tt=2) for s in range(7)] == [-1, -1, -1, -1, -3, -1, -3]


def test_workspace_bytes(hip_lib):
    ws = hip_lib.pope_mocope_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(-1, 5) == 0
    sizes = {(B, S): ws(B, S) for B in (1, 2, 3, 8, 9, 64, 200) for S in (1, 5, 37, 70, 220, 500)}
    assert all(n > 0 and n % 256 == 0 for n in sizes.values())
    for (B, S), n in sizes.items():
        assert n >= B * S * (2 * 76 + 1 + 3 * 76 + 2 * 76 + 38) * 4       # the [B, S, .] buffers alone
        for (B2, S2), n2 in sizes.items():
            if B2 >= B and S2 >= S:
                assert n2 >= n, ((B, S), (B2, S2))
