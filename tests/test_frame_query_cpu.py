"""CPU: the public surface of the frame-to-pose query — the façade's SAM exports (`pope_amd/pope_model_api.py`), the signatures of
`SamAutomaticMaskGenerator.propose` / `propose_batch` and `driver.locate_pose_from_frames` / `locate_pose_from_frame`, and the
checks of the frame-level call that come before any launch.  What they compute is pinned on the card by
tests/test_gpu_frame_query.py."""
import inspect
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

FACADE_NAMES = ("SamAutomaticMaskGenerator", "SamPredictor", "build_sam_vit_h", "build_sam_vit_l", "build_sam_vit_b",
                "sam_model_registry", "get_model_info", "locate_pose_from_frames", "locate_pose_from_frame")


def test_facade_exports_the_generator_and_the_frame_level_calls():
    from pope_amd import driver, pope_model_api as api, sam_generator as sg
    for name in FACADE_NAMES:
        assert hasattr(api, name), name
    ns = {}
    exec("from pope_amd.pope_model_api import *", ns)             # what the drivers do (eval_linemod_json.py:1)
    assert not [name for name in FACADE_NAMES if name not in ns]
    assert api.SamAutomaticMaskGenerator is sg.SamAutomaticMaskGenerator and api.SamPredictor is sg.SamPredictor
    assert api.locate_pose_from_frames is driver.locate_pose_from_frames
    assert api.locate_pose_from_frame is driver.locate_pose_from_frame
    assert "out-of-scope stages (the SAM" not in " ".join(api.__doc__.split())


def test_sam_model_registry_maps_to_the_builders():
    from pope_amd import pope_model_api as api
    assert api.sam_model_registry == {"default": api.build_sam_vit_h, "vit_h": api.build_sam_vit_h, "vit_l": api.build_sam_vit_l,
                                      "vit_b": api.build_sam_vit_b}
    assert len({api.build_sam_vit_h, api.build_sam_vit_l, api.build_sam_vit_b}) == 3


def test_get_model_info_names_the_reference_checkpoints():
    from pope_amd.pope_model_api import get_model_info, sam_model_registry
    assert get_model_info("b") == ("weights/sam_vit_b_01ec64.pth", "vit_b")
    assert get_model_info("l") == ("weights/sam_vit_l_0b3195.pth", "vit_l")
    assert get_model_info("h") == ("weights/sam_vit_h_4b8939.pth", "vit_h")
    assert get_model_info() == get_model_info("b")
    assert all(get_model_info(t)[1] in sam_model_registry for t in "blh")
    for other in ("vit_b", "B", "", None, 0):
        with pytest.raises(NotImplementedError):
            get_model_info(other)


# run in a fresh interpreter: torch and numpy are imported first, then every file the import of the façade opens and every
# module it constructs is recorded (the reference façade loads weights/matcher.pth and builds the matcher at that point)
IMPORT_PROBE = """
import sys
import numpy, torch, torch.nn.functional, PIL.Image
opened, built = [], []
sys.addaudithook(lambda event, args: opened.append(str(args[0])) if event == "open" else None)
init = torch.nn.Module.__init__
def counting_init(self, *a, **k):
    built.append(type(self).__name__)
    init(self, *a, **k)
torch.nn.Module.__init__ = counting_init
import pope_amd.pope_model_api as api
code = (".py", ".pyc")
print("OPENED", [p for p in opened if not p.endswith(code) and "__pycache__" not in p])
print("BUILT", built)
print("CUDA", torch.cuda.is_initialized())
"""


def test_importing_the_facade_builds_no_model_and_touches_no_file():
    out = subprocess.run([sys.executable, "-c", IMPORT_PROBE], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = dict(line.split(" ", 1) for line in out.stdout.splitlines() if line.split(" ", 1)[0] in ("OPENED", "BUILT", "CUDA"))
    assert lines == {"OPENED": "[]", "BUILT": "[]", "CUDA": "False"}, out.stdout


def test_signatures():
    from pope_amd import driver
    from pope_amd.sam_generator import SamAutomaticMaskGenerator as Gen
    assert list(inspect.signature(Gen.propose_batch).parameters) == ["self", "images"]
    assert list(inspect.signature(Gen.propose).parameters) == ["self", "image"]
    want = {"conf_thr": 0.9, "ransac_thr": 0.5, "ransac_conf": 0.99, "out_size": 256, "max_proposals": None}
    for fn, lead in ((driver.locate_pose_from_frames, ["mask_generator", "dinov2_model", "matcher", "refs_bgr", "frames_bgr", "K0", "K1"]),
                     (driver.locate_pose_from_frame, ["mask_generator", "dinov2_model", "matcher", "ref_bgr", "frame_bgr", "K0", "K1"])):
        params = inspect.signature(fn).parameters
        assert list(params) == lead + list(want)
        assert all(params[k].default is inspect.Parameter.empty for k in lead)
        assert {k: params[k].default for k in want} == want
    batch = inspect.signature(driver.locate_match_pose_batch_u8).parameters           # the call it hands over to
    assert {k: batch[k].default for k in want if k in batch} == {k: v for k, v in want.items() if k != "max_proposals"}


class _On(torch.nn.Module):
    """Stands for a model that lives on `device`: nothing of it is run."""

    def __init__(self, device):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=device), requires_grad=False)


class _Generator:
    def __init__(self, device):
        self.predictor = type("P", (), {"device": torch.device(device)})()

    def propose_batch(self, images):
        raise AssertionError("the generator must not run")


def test_refusals_before_any_launch():
    from pope_amd.driver import locate_pose_from_frames
    refs, K = np.zeros((2, 64, 64, 3), np.uint8), np.eye(3)
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="one device"):
        locate_pose_from_frames(_Generator("cpu"), _On("meta"), _On("meta"), refs, frames, K, K)
    with pytest.raises(ValueError, match="one device"):
        locate_pose_from_frames(_Generator("meta"), _On("meta"), _On("cpu"), refs, frames, K, K)
    with pytest.raises(ValueError, match="2 references, 1 frames"):
        locate_pose_from_frames(_Generator("cpu"), _On("cpu"), _On("cpu"), refs, frames[:1], K, K)
    with pytest.raises(ValueError, match="max_proposals"):
        locate_pose_from_frames(_Generator("cpu"), _On("cpu"), _On("cpu"), refs, frames, K, K, max_proposals=-1)


def test_mixed_frame_sizes_are_refused_by_the_generator_front():
    from pope_amd import sam_generator as sg
    from test_sam_generator_cpu import small_sam
    gen = sg.SamAutomaticMaskGenerator(small_sam(depth=2)[0], points_per_side=2)
    assert gen.propose_batch([]) == []
    for call in (gen.propose_batch, gen.generate_batch):
        with pytest.raises(ValueError, match="one size"):
            call([np.zeros((48, 64, 3), np.uint8), np.zeros((48, 72, 3), np.uint8)])
