"""CPU: the C ABI of the SAM generator's small-region clean-up (pope_sam_small_regions_u32, pope_amd/csrc/sam_regions.hip) as far
as it goes without a GPU: the symbols, the workspace query and the argument check, which runs before any HIP call."""
import ctypes
import inspect

from pope_amd import _lib
from pope_amd import sam_generator as sg

ERR_ARG = -1


def test_symbols_are_bound(hip_lib):
    for name in ("pope_sam_small_regions_workspace_bytes", "pope_sam_small_regions_u32"):
        assert name in _lib.PROTOTYPES and hasattr(hip_lib, name)
    assert hip_lib.pope_abi_version() == 10
    assert list(inspect.signature(sg.clean_masks_packed).parameters) == ["packed", "W", "min_area"]
    assert list(inspect.signature(sg.postprocess_small_regions_segments).parameters) == ["data", "seg", "W", "min_area", "nms_thresh"]


def test_workspace_query(hip_lib):
    ws = hip_lib.pope_sam_small_regions_workspace_bytes
    assert ws(1, 4096, 4096) == 0 and ws(1, 1 << 12, (1 << 12) + 1) == 0         # H * W >= 2^24
    assert ws(1, 4096, 4095) > 0                                                  # just below
    assert ws(1, 0, 640) == 0 and ws(1, 480, 0) == 0 and ws(1, -1, 640) == 0 and ws(-1, 480, 640) == 0 and ws(0, 480, 640) == 0
    one = ws(1, 480, 640)
    # per mask: a label and a counter (int32 each) per two pixels of the padded rows
    assert 480 * 640 * 4 <= one <= 480 * 640 * 4 + 512
    full = ws(768, 480, 640)
    assert 0 < full <= sg.CLEAN_CHUNK * one                                        # bounded by the chunk, not by n
    assert ws(sg.CLEAN_CHUNK, 480, 640) == full == ws(sg.CLEAN_CHUNK + 1, 480, 640) == ws(1 << 20, 480, 640)
    assert ws(sg.CLEAN_CHUNK - 1, 480, 640) < full
    assert ws(3, 37, 70) > 0 and ws(1, 1, 1) > 0


def test_argument_validation_without_gpu(hip_lib):
    call = hip_lib.pope_sam_small_regions_u32
    buf = ctypes.create_string_buffer(64)
    ok = (ctypes.addressof(buf) + 15) & ~15          # never dereferenced: nothing below gets as far as a launch
    big = 1 << 30
    good = dict(packed=ok, n=2, H=8, W=8, min_area=250, packed_out=ok, unchanged=ok, boxes=ok, area=ok, workspace=ok, workspace_bytes=big)

    def run(**kw):
        a = dict(good, **kw)
        return call(a["packed"], a["n"], a["H"], a["W"], a["min_area"], a["packed_out"], a["unchanged"], a["boxes"], a["area"],
                    a["workspace"], a["workspace_bytes"], None)
    for name in ("packed", "packed_out", "unchanged", "boxes", "area", "workspace"):
        assert run(**{name: None}) == ERR_ARG, name
    for kw in (dict(n=-1), dict(H=0), dict(H=-4), dict(W=0), dict(W=-4), dict(min_area=-1), dict(H=4096, W=4096)):
        assert run(**kw) == ERR_ARG, kw
    assert run(packed_out=ok + 4) == ERR_ARG          # overlapping without being the same buffer
    assert run(workspace_bytes=0) == -3               # POPE_ERR_WORKSPACE
    # an empty batch is a no-op, whatever the pointers
    assert run(n=0) == 0
    assert call(None, 0, 480, 640, 250, None, None, None, None, None, 0, None) == 0
    assert run(n=0, H=0) == ERR_ARG                   # the geometry is still checked

