"""CPU: the host side of the Vision Mamba backbone (pope_amd/vim.py) — state-dict layouts against the reference's, the
constructor's refusals, the `Vim` loader (head keys, pos_embed resampling) against tests/golden/vim.npz, the seeded weights, and
argument checks that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pope_amd import _lib, synth, vim


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "vim.npz"))


def _layout(sd):
    return [(k, "x".join(str(d) for d in v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("factory", sorted(vim.FACTORIES))
def test_factory_state_dict_is_the_reference_s(gold, factory):
    want = list(zip(gold[f"keys_{factory}.names"].tolist(), gold[f"keys_{factory}.shapes"].tolist()))
    with torch.device("meta"):
        model = vim.FACTORIES[factory]()
    assert _layout(model.state_dict()) == want
    keys = synth.vim_keys(model.embed_dim, model.depth, 1000, 224, model.stride)
    assert [(k, "x".join(str(d) for d in s)) for k, s in keys] == want
    L = 730 if "stride8" in factory else 197
    assert ("pos_embed", f"1x{L}x{model.embed_dim}") in want and len(want) == 6 + 24 * 17 + 1


SERVED = dict(vim._FACTORY_SETTINGS, embed_dim=192)
REFUSED = [("if_rope", True), ("if_rope_residual", True), ("if_bidirectional", True), ("bimamba_type", "v1"), ("bimamba_type", "none"),
           ("if_bimamba", True), ("rms_norm", False), ("if_cls_token", False), ("use_double_cls_token", True),
           ("use_middle_cls_token", False), ("if_abs_pos_embed", False), ("if_devide_out", False), ("img_size", 220),
           ("img_size", (224, 192)), ("patch_size", 14), ("stride", 4), ("channels", 1), ("embed_dim", 200), ("init_layer_scale", 1e-2),
           ("ssm_cfg", {"d_state": 8}), ("flip_img_sequences_ratio", 0.5)]


@pytest.mark.parametrize("arg,value", REFUSED, ids=[f"{a}={v}" for a, v in REFUSED])
def test_constructor_refuses(arg, value):
    with torch.device("meta"):
        with pytest.raises(NotImplementedError, match=arg):
            vim.VisionMamba(**{**SERVED, arg: value})


def test_constructor_accepts_the_equivalent_settings():
    with torch.device("meta"):
        for fused in (True, False):
            for res32 in (True, False):
                m = vim.VisionMamba(**{**SERVED, "fused_add_norm": fused, "residual_in_fp32": res32, "img_size": 64, "stride": 8})
                assert m.patch_embed.grid_size == (7, 7) and tuple(m.pos_embed.shape) == (1, 50, 192)
        with pytest.raises(ValueError):
            vim.VisionMamba(**SERVED, precision="bf16")
        m = vim.VisionMamba(**SERVED)
    assert not m.training
    with pytest.raises(NotImplementedError):
        m.train()
    assert m.eval() is m


def test_vim_loader_resamples_pos_embed_and_drops_head(gold):
    ck = synth.vim_pos_embed_checkpoint()
    assert int(gold["pos_embed.orig_size"]) == 14 and int(gold["pos_embed.new_size"]) == 27
    # the released checkpoints carry a 1000-class head: another width drops it, the same width loads it
    m = vim.Vim(num_class=32, model_type="small", checkpoint=ck)
    assert m.dropped_keys == ["head.weight", "head.bias"] and tuple(m.model.head.weight.shape) == (32, 384)
    assert "pos_embed" in ck["model"] and tuple(ck["model"]["pos_embed"].shape) == (1, 197, 384)     # the caller's dict is not edited
    pe = m.model.pos_embed.detach()
    assert tuple(pe.shape) == (1, 730, 384)
    f = pe.double().reshape(-1)
    assert float((f * torch.arange(1, f.numel() + 1, dtype=torch.float64)).sum()) == pytest.approx(float(gold["pos_embed.checksum"]), rel=1e-9)
    idx = synth.vim_tap_index("pos_embed", "resampled", pe.numel())
    assert np.allclose(pe.reshape(-1)[idx].numpy(), gold["pos_embed.samples"], rtol=1e-5, atol=1e-6)
    assert torch.equal(pe[:, 0], ck["model"]["pos_embed"][:, 0])         # the extra token's row is kept as it is
    assert not any(p.requires_grad for p in m.parameters())
    m = vim.Vim(num_class=1000, model_type="small", checkpoint=ck)
    assert m.dropped_keys == [] and torch.equal(m.model.head.weight, ck["model"]["head.weight"])
    with pytest.raises(ValueError):
        vim.Vim(model_type="base")
    with pytest.raises(NotImplementedError):
        m.train()


def test_vim_loader_from_a_file_and_without_checkpoint(tmp_path):
    ck = synth.vim_pos_embed_checkpoint(embed_dim=192, num_classes=8)
    path = tmp_path / "vim_t.pth"
    torch.save(ck, path)
    a = vim.Vim(num_class=8, model_type="tiny", img_size=64, checkpoint=str(path))
    b = vim.Vim(num_class=8, model_type="tiny", img_size=64, checkpoint=ck)
    assert tuple(a.model.pos_embed.shape) == (1, 50, 192) and torch.equal(a.model.pos_embed, b.model.pos_embed)
    assert torch.equal(a.model.head.bias, ck["model"]["head.bias"])
    c = vim.Vim(num_class=8, model_type="tiny", img_size=64)
    assert c.dropped_keys == [] and 0.015 < float(c.model.pos_embed.std()) < 0.025          # trunc_normal_(std=0.02) as initialised


def test_synth_vim_state_dict():
    a = synth.vim_state_dict(192, 2, 40, 64, 8, seed=3)
    b = synth.vim_state_dict(192, 2, 40, 64, 8, seed=3)
    c = synth.vim_state_dict(192, 2, 40, 64, 8, seed=4)
    assert list(a) == [k for k, _ in synth.vim_keys(192, 2, 40, 64, 8)]
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["cls_token"], c["cls_token"])
    m = vim.VisionMamba(**{**SERVED, "depth": 2, "num_classes": 40, "img_size": 64, "stride": 8})
    m.load_state_dict(a, strict=True)
    p = "layers.1.mixer."
    A = torch.exp(a[p + "A_log"])
    ratio = A / torch.arange(1, 17)
    assert torch.allclose(ratio, ratio[:, :1].expand(-1, 16), rtol=1e-5) and 0.5 <= float(ratio.min()) and float(ratio.max()) <= 2.0
    dt = torch.nn.functional.softplus(a[p + "dt_proj.bias"])
    assert 1e-3 * 0.999 <= float(dt.min()) and float(dt.max()) <= 1e-1 * 1.001
    assert not torch.equal(a[p + "conv1d.weight"], a[p + "conv1d_b.weight"]) and not torch.equal(a[p + "D"], a[p + "D_b"])
    assert 0.3 < float(a[p + "conv1d.weight"].std()) < 0.7 and 0.7 < float(a["pos_embed"].std()) < 1.3
    case = synth.vim_case("small_s8_64")
    assert tuple(case["x"].shape) == (3, 3, 64, 64) and synth.vim_geometry(64, 8) == (7, 50, 24)
    assert synth.vim_geometry(224, 8) == (27, 730, 364) and synth.vim_geometry(224, 16) == (14, 197, 98)


def test_workspace_query_refuses_bad_arguments(hip_lib):
    assert hip_lib.pope_abi_version() == 10
    w = _lib.VimWeights()
    w.img, w.stride, w.dim, w.depth, w.num_classes, w.eps = 224, 8, 384, 24, 1000, 1e-5
    layers = (_lib.VimLayerWeights * 24)()
    w.layers_host = C.cast(layers, C.POINTER(_lib.VimLayerWeights))
    need = hip_lib.pope_vim_workspace_bytes(C.byref(w), 2)
    assert need > 2 * 730 * 384 * 4 * 10 and need % 256 == 0
    assert hip_lib.pope_vim_workspace_bytes(C.byref(w), 4) > need
    assert hip_lib.pope_vim_workspace_bytes(None, 2) == 0
    for b in (0, -1, 1 << 20):
        assert hip_lib.pope_vim_workspace_bytes(C.byref(w), b) == 0
    for field, bad in (("img", 220), ("img", 8), ("stride", 4), ("dim", 200), ("dim", 1024), ("depth", 0), ("eps", 0.0)):
        keep = getattr(w, field)
        setattr(w, field, bad)
        assert hip_lib.pope_vim_workspace_bytes(C.byref(w), 2) == 0, (field, bad)
        setattr(w, field, keep)
    assert hip_lib.pope_vim_scan_chunk() >= 16
    assert hip_lib.pope_vim_scan_workspace_bytes(2, 730, 768) > 0 and hip_lib.pope_vim_scan_workspace_bytes(0, 730, 768) == 0
