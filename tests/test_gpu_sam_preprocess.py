"""SAM's input transform on the MI355X: `pope_resize_u8` against Pillow, `pope_sam_preprocess_u8_f32` against the host chain
(Pillow, `(x - mean) / std` in fp32 on the CPU, `F.pad`), and the public calls with frames that sit on the device against the
same calls with numpy frames.  Every comparison is an equality of bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pope_amd import preprocess as pp
from pope_amd import sam_generator as sg
from pope_amd import synth
from test_gpu_frame_query import assert_same_value, generator
from test_gpu_sam_generator_batch import E2E, FRAMES, MODES, assert_same_records, blocky_frame
from test_sam_generator_cpu import small_sam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 1024
# 480 x 640: the drivers' frames; 333 x 332: portrait, OW = 1021, a store quad straddles the edge; 1300 x 1700: a downscale with
# 5 taps; 5 x 7: the windows clip at both borders; 97 x 1024: identity in x, pad rows below; 2 x 1500: one output row
SIZES = [(480, 640), (333, 332), (1300, 1700), (5, 7), (97, 1024), (2, 1500)]
SAM_MEAN, SAM_STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def pillow(frame, hw):
    from PIL import Image
    return np.array(Image.fromarray(np.ascontiguousarray(frame)).resize((hw[1], hw[0]), Image.BILINEAR))


@pytest.fixture(scope="module")
def cases(hip_lib):
    """size -> (frame uint8 [H, W, 3], the frame on the device, (oh, ow), Pillow's resize of it), computed once."""
    assert torch.cuda.is_available()
    out = {}
    for hw in SIZES:
        frame = np.random.default_rng(hw[0] * 7 + hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)
        out_hw = sg.ResizeLongestSide.get_preprocess_shape(*hw, S)
        out[hw] = (frame, torch.from_numpy(frame).to(DEV), out_hw, pillow(frame, out_hw))
    return out


def host_chain(resized, mean, std):
    """`Sam.preprocess` of one resized uint8 HWC image on the CPU: fp32 [3, S, S]."""
    x = torch.as_tensor(resized).permute(2, 0, 1)
    x = (x - torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)
    return F.pad(x, (0, S - x.shape[-1], 0, S - x.shape[-2]))


def same_bits(got, want):
    """Equal as fp32 bit patterns: `torch.equal` alone takes -0.0 for +0.0."""
    got = got.cpu()
    return got.dtype == want.dtype == torch.float32 and got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES)
def test_resize_equals_pillow(cases, hw):
    frame, on_dev, out_hw, want = cases[hw]
    assert want.shape == out_hw + (3,) and max(out_hw) == S
    got = pp.resize_u8_batch(on_dev[None], out_hw)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1,) + want.shape
    assert np.array_equal(got[0].cpu().numpy(), want)
    t = sg.ResizeLongestSide(S)
    one, four = t.apply_image(on_dev), t.apply_image(on_dev[None])
    assert one.is_cuda and one.dtype == torch.uint8 and tuple(one.shape) == want.shape and np.array_equal(one.cpu().numpy(), want)
    assert tuple(four.shape) == (1,) + want.shape and torch.equal(four[0], one)


@pytest.mark.parametrize("hw", SIZES)
def test_fused_output_equals_the_host_chain(cases, hw):
    frame, on_dev, out_hw, resized = cases[hw]
    rng = np.random.default_rng(17)
    other_mean, other_std = rng.uniform(0, 255, 3).tolist(), rng.uniform(0.5, 90, 3).tolist()
    for mean, std in ((SAM_MEAN, SAM_STD), (other_mean, other_std)):
        got, input_size = pp.sam_preprocess_batch(on_dev[None], S, mean, std)
        want = host_chain(resized, mean, std)
        assert input_size == out_hw and got.is_cuda and same_bits(got[0], want), (hw, mean)
        pad = torch.ones(S, S, dtype=torch.bool)
        pad[:out_hw[0], :out_hw[1]] = False
        assert not got[0].cpu().view(torch.int32)[:, pad].any()                     # every pad element is +0.0
    got, _ = pp.sam_preprocess_batch(on_dev[None], S, SAM_MEAN, SAM_STD, flip=True)
    assert same_bits(got[0], host_chain(pillow(frame[..., ::-1], out_hw), SAM_MEAN, SAM_STD)), hw


def test_a_frame_of_a_batch_has_the_bits_of_that_frame_alone():
    hw = (333, 332)
    rng = np.random.default_rng(23)
    stack = torch.from_numpy(rng.integers(0, 256, (3,) + hw + (3,), dtype=np.uint8)).to(DEV)
    out_hw = sg.ResizeLongestSide.get_preprocess_shape(*hw, S)
    x, _ = pp.sam_preprocess_batch(stack, S, SAM_MEAN, SAM_STD)
    u8 = pp.resize_u8_batch(stack, out_hw)
    assert tuple(x.shape) == (3, 3, S, S) and tuple(u8.shape) == (3,) + out_hw + (3,)
    for q in range(3):
        alone, _ = pp.sam_preprocess_batch(stack[q:q + 1], S, SAM_MEAN, SAM_STD)
        assert same_bits(x[q], alone[0].cpu()), q
        assert torch.equal(u8[q], pp.resize_u8_batch(stack[q:q + 1], out_hw)[0]), q
    assert not torch.equal(x[0], x[1])


# ---- 2. the public calls -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sam():
    model, sd = small_sam(depth=2)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV)


@pytest.mark.parametrize("image_format", ["RGB", "BGR"])
def test_predictor_state_from_a_device_frame(cases, sam, image_format):
    frame, on_dev, out_hw, _ = cases[(480, 640)]
    host, dev = sg.SamPredictor(sam), sg.SamPredictor(sam)
    host.set_image(frame, image_format)
    dev.set_image(on_dev, image_format)
    assert dev.is_image_set and dev.input_size == host.input_size == out_hw and dev.original_size == host.original_size == (480, 640)
    assert type(dev.input_size) is type(host.input_size) and all(type(v) is int for v in dev.input_size + dev.original_size)
    assert torch.equal(dev.features, host.features)
    with pytest.raises(TypeError):
        dev.set_image(on_dev.float(), image_format)


@pytest.mark.parametrize("mode", MODES)
def test_generate_from_a_device_frame(sam, mode):
    frame = blocky_frame(5)
    gen = sg.SamAutomaticMaskGenerator(sam, output_mode=mode, **E2E)
    want = gen.generate(frame)
    got = gen.generate(torch.from_numpy(frame).to(DEV))
    assert len(want) >= 1
    assert_same_records(got, want, mode)


def test_propose_batch_from_device_frames(sam):
    frames = [blocky_frame(5), blocky_frame(7)]
    gen = sg.SamAutomaticMaskGenerator(sam, **E2E)
    want = gen.propose_batch(frames)
    stack = torch.from_numpy(np.stack(frames)).to(DEV)
    assert sum(len(w) for w in want) >= 1
    for form in (stack, [stack[0], stack[1]]):
        got = gen.propose_batch(form)
        assert len(got) == 2 and not gen.predictor.is_image_set
        for g, w in zip(got, want):
            assert g.dtype == w.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w)
    assert np.array_equal(gen.propose(stack[1]), want[1])
    with pytest.raises(ValueError):
        gen.propose_batch([frames[0], stack[1]])
    with pytest.raises(TypeError):
        gen.propose_batch(stack.float())


def test_frame_query_from_device_frames_never_reaches_pillow(sam, sd0, golden_dir, monkeypatch):
    """The set-up of tests/test_gpu_frame_query.py: three frames, the box NMS threshold raised so that the vote has proposals to
    choose from, DINOv2 ViT-S/14 and the Matcher under the peaked synthetic weights."""
    import os
    from PIL import Image
    from pope_amd.dinov2_utils import load_dinov2_model
    from pope_amd.driver import locate_pose_from_frame, locate_pose_from_frames
    from pope_amd.matcher import Matcher, default_cfg
    fx = np.load(os.path.join(golden_dir, "loftr_512_peaked.npz"))
    sd = synth.peaked_matcher_state_dict(torch.from_numpy(fx["outconv_mean"]), seed=0)
    sd.pop("_calibration_mean")
    matcher = Matcher(default_cfg).eval()
    matcher.load_state_dict(sd, strict=True)
    models = load_dinov2_model(state_dict=sd0).to(DEV), matcher.to(DEV)
    frames = [blocky_frame(s, g) for s, g in FRAMES]
    qs = [synth.synthetic_frame_case(seed=31 + q) for q in range(len(FRAMES))]
    refs, K0, K1 = np.stack([c[0] for c in qs]), np.stack([c[3] for c in qs]), qs[0][4]
    want = locate_pose_from_frames(generator(sam), *models, refs, frames, K0, K1)
    want_one = locate_pose_from_frame(generator(sam), *models, refs[0], frames[0], K0[0], K1)
    want_two = locate_pose_from_frames(generator(sam), *models, refs[:2], frames[:2], K0[:2], K1)
    assert max(len(w["proposals"]) for w in want) >= 4 and max(w["best_proposal"] for w in want) >= 0   # the vote had a choice
    stack = torch.from_numpy(np.stack(frames)).to(DEV)

    def no_pillow(*a, **k):
        raise AssertionError("the device path reached PIL.Image.Image.resize")

    with monkeypatch.context() as m:
        m.setattr(Image.Image, "resize", no_pillow)
        got = locate_pose_from_frames(generator(sam), *models, refs, stack, K0, K1)
        as_list = locate_pose_from_frames(generator(sam), *models, refs[:2], [stack[0], stack[1]], K0[:2], K1)
        one = locate_pose_from_frame(generator(sam), *models, refs[0], stack[0], K0[0], K1)
    assert len(got) == len(want) == len(frames)
    for q, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w)
        for k in w:
            assert_same_value(g[k], w[k], (q, k))
    for k in want_one:
        assert_same_value(one[k], want_one[k], ("one query", k))
        for q in range(2):
            assert_same_value(as_list[q][k], want_two[q][k], ("list of device frames", q, k))
