"""`clean_masks_packed` (pope_sam_small_regions_u32, pope_amd/csrc/sam_regions.hip) on the MI355X against the CPU definition:
`sam_amg.remove_small_regions` for holes, then for islands, then `sam_amg.mask_to_box`, the oracle of `cpu_clean` in
test_gpu_sam_generator.py.  Connected components of a bit mask are exact, so every comparison is an equality: the packed
words (pad bits zero), `unchanged`, the boxes and the areas."""
import functools

import numpy as np
import pytest
import torch

from pope_amd import sam_amg, synth
from pope_amd import sam_generator as sg
from test_sam_generator_cpu import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = sg.CLEAN_CHUNK


def oracle(masks, min_area):
    """(cleaned bool [n, H, W], unchanged bool [n], boxes int32 [n, 4], area int32 [n]) by the CPU definition."""
    out, same = [], []
    for m in masks:
        m = torch.as_tensor(np.ascontiguousarray(m))
        m, c0 = sam_amg.remove_small_regions(m, min_area, "holes")
        m, c1 = sam_amg.remove_small_regions(m, min_area, "islands")
        out.append(m.numpy())
        same.append(not (c0 or c1))
    out = np.stack(out)
    return out, np.asarray(same), sam_amg.mask_to_box(out), out.reshape(len(out), -1).sum(1).astype(np.int32)


def device_clean(masks, min_area):
    """The four outputs of `clean_masks_packed` for bool [n, H, W], as numpy (words as uint32)."""
    masks = np.asarray(masks, bool)
    packed = torch.as_tensor(sam_amg.pack_masks(masks).view(np.int32), device=DEV)
    out, same, boxes, area = sg.clean_masks_packed(packed, masks.shape[2], min_area)
    assert out.dtype == torch.int32 and same.dtype == torch.bool and boxes.dtype == torch.int32 and area.dtype == torch.int32
    return out.cpu().numpy().view(np.uint32), same.cpu().numpy(), boxes.cpu().numpy(), area.cpu().numpy()


def assert_equals_oracle(got, want, W):
    words, same, boxes, area = got
    want_masks, want_same, want_boxes, want_area = want
    print(f"masks={len(want_masks)} changed={int((~want_same).sum())} word_diff={int((words != sam_amg.pack_masks(want_masks)).sum())} "
          f"unchanged_diff={int((same != want_same).sum())} box_diff={int((boxes != want_boxes).sum())} area_diff={int((area != want_area).sum())}")
    assert np.array_equal(words, sam_amg.pack_masks(want_masks))            # pack_masks leaves the pad bits zero
    if W % 32:
        assert not (words[:, :, -1] >> np.uint32(W % 32)).any()
    assert np.array_equal(same, want_same)
    assert np.array_equal(boxes, want_boxes)
    assert np.array_equal(area, want_area)


# ---- hand-built masks --------------------------------------------------------------------------------------------------
def _random(H, W, seed, p=0.5):
    return np.random.default_rng(seed).random((H, W)) < p


def _threshold_edge():
    m = np.zeros((96, 200), bool)
    m[4:60, 4:110] = True
    m[8:18, 8:32] = False; m[18, 8:17] = False          # hole of 249
    m[8:18, 40:65] = False                              # hole of 250
    m[8:18, 72:97] = False; m[18, 72] = False           # hole of 251
    m[66:76, 4:28] = True; m[76, 4:13] = True           # island of 249
    m[66:76, 40:65] = True                              # island of 250
    m[66:76, 72:97] = True; m[76, 72] = True            # island of 251
    m[30:50, 120:190] = True                            # a second large island
    return m


def _hole_at_the_border():
    m = np.zeros((64, 96), bool)
    m[10:50, 10:80] = True
    m[10:16, 30:38] = False      # a bay of 48 pixels, open to the outer background through the block's edge
    m[30:36, 40:48] = False      # an enclosed hole of 48
    m[44:50, 60:66] = False      # a bay whose only opening is diagonal: (50, 66) is background, (49, 66) and (50, 65) are not
    m[50, 58:66] = True
    m[44:51, 66] = True
    m[50, 66] = False
    m[0:8, 84:96] = True         # a block in the image corner with a hole on the image border: enclosed, so it is small
    m[0:3, 88:92] = False
    return m


def _diagonals():
    m = np.zeros((48, 100), bool)
    for t in range(40):
        m[t, 12 + t] = True          # crosses x = 31 / 32
        m[t + 4, 84 - t] = True      # crosses x = 63 / 64 the other way
    return m


def _spiral(H=64, W=96):
    m = np.zeros((H, W), bool)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    m[top, left:right + 1] = True
    while True:
        if bottom - top < 2 or right - left < 2:
            break
        m[top:bottom + 1, right] = True
        m[bottom, left:right + 1] = True
        m[top + 2:bottom + 1, left] = True
        top += 2
        m[top, left:right - 1] = True
        left += 2; bottom -= 2; right -= 2
        if left > right or top > bottom:
            break
    return m


def _comb():
    m = np.zeros((64, 96), bool)
    m[:, ::2] = True
    m[-2, :] = False
    m[-1, :] = True
    m[-2, ::2] = True
    return m


def _nested():
    m = np.zeros((64, 200), bool)

    def ring(y0, y1, x0, x1, t=2, open_top=False):
        m[y0:y1, x0:x0 + t] = True
        m[y0:y1, x1 - t:x1] = True
        m[y1 - t:y1, x0:x1] = True
        if not open_top:
            m[y0:y0 + t, x0:x1] = True
    ring(2, 62, 2, 60)                   # O around ..
    ring(20, 39, 14, 34)                 # .. an O whose inside (15 x 16 = 240) is a small hole
    ring(2, 62, 70, 130, open_top=True)  # U around ..
    ring(30, 50, 90, 110, open_top=True)  # .. a U of 20 + 20 + 16 + .. pixels: below 250, an island that goes
    ring(2, 62, 140, 198)                # O around an O around a dot
    ring(12, 52, 150, 188)
    m[30:33, 166:170] = True
    return m


def _lattice():
    m = np.zeros((64, 96), bool)
    m[::2, ::2] = True
    return m


def _two_equal_islands():
    m = np.zeros((40, 70), bool)
    m[20:23, 2:6] = True
    m[5:9, 60:63] = True          # same size, first in raster order although it lies to the right
    return m


def _single_small_island():
    m = np.zeros((40, 70), bool)
    m[10:14, 30:40] = True
    return m


def _checkerboard():
    y, x = np.mgrid[0:64, 0:96]
    return ((x + y) & 1).astype(bool)


HAND = {
    "1x1 set": (np.ones((1, 1), bool), 250),
    "1x1 clear": (np.zeros((1, 1), bool), 250),
    "8x8 background": (np.zeros((8, 8), bool), 250),
    "8x8 foreground": (np.ones((8, 8), bool), 250),
    "5x33": (_random(5, 33, 1), 250),
    "5x33 area 3": (_random(5, 33, 1), 3),
    "37x70": (_random(37, 70, 2, 0.45), 250),
    "37x70 area 6": (_random(37, 70, 2, 0.45), 6),
    "64x96": (_random(64, 96, 3, 0.4), 250),
    "64x96 area 6": (_random(64, 96, 3, 0.4), 6),
    "threshold edge": (_threshold_edge(), 250),
    "hole at the border": (_hole_at_the_border(), 250),
    "diagonals": (_diagonals(), 30),
    "checkerboard": (_checkerboard(), 250),
    "lattice": (_lattice(), 250),
    "spiral": (_spiral(), 250),
    "comb": (_comb(), 50),        # the gaps between the teeth are 62 pixels each: they stay, and so does the comb
    "nested": (_nested(), 250),
    "two equal islands": (_two_equal_islands(), 250),
    "single small island": (_single_small_island(), 250),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_masks(name):
    mask, min_area = HAND[name]
    want = oracle(mask[None], min_area)
    assert_equals_oracle(device_clean(mask[None], min_area), want, mask.shape[1])


def test_hand_built_masks_say_what_they_claim():
    """The oracle's verdict on the cases whose names promise one (so that a case cannot quietly stop exercising its rule)."""
    cleaned = {k: oracle(HAND[k][0][None], HAND[k][1]) for k in ("8x8 background", "threshold edge", "diagonals", "checkerboard",
                                                                 "lattice", "two equal islands", "single small island", "spiral")}
    assert cleaned["8x8 background"][0].all()
    m, t = HAND["threshold edge"][0], cleaned["threshold edge"][0][0]
    assert t[8:18, 8:32].all() and not t[8:18, 40:65].any() and not t[8:18, 72:97].any()         # holes: 249 filled, 250 / 251 stay
    assert not t[66:77, 4:28].any() and t[66:76, 40:65].all() and t[66:76, 72:97].all()         # islands: 249 gone, 250 / 251 stay
    assert np.array_equal(cleaned["diagonals"][0][0], HAND["diagonals"][0]) and cleaned["diagonals"][1][0]
    assert cleaned["checkerboard"][1][0]
    lat = cleaned["lattice"][0][0]
    assert lat.sum() == 1 and lat[0, 0] and not cleaned["lattice"][1][0]
    two = cleaned["two equal islands"][0][0]
    assert two[5:9, 60:63].all() and two.sum() == 12 and not cleaned["two equal islands"][1][0]
    one = cleaned["single small island"]
    assert np.array_equal(one[0][0], HAND["single small island"][0]) and not one[1][0]
    assert cleaned["spiral"][1][0] and m.any()


# ---- random blobs at 480 x 640 -----------------------------------------------------------------------------------------
def box_blur(f, k):
    """Box filter of odd width k along both axes of [H, W] (edges replicated), by differences of running sums."""
    r = k // 2
    for ax in (0, 1):
        p = np.concatenate([np.repeat(np.take(f, [0], ax), r + 1, ax), f, np.repeat(np.take(f, [-1], ax), r, ax)], ax)
        c = np.cumsum(p, ax, dtype=np.float64)
        n = f.shape[ax]
        f = (np.take(c, range(k, k + n), ax) - np.take(c, range(0, n), ax)) / k
    return f


@functools.lru_cache(maxsize=None)
def blob_case():
    """CHUNK + 1 masks of 480 x 640 (a noise field box-blurred twice, cut at a quantile; widths and quantiles cycle so that
    clean and speckled masks alternate) and their oracle result, computed once for every test below (which only read them)."""
    rng = np.random.default_rng(11)
    masks = np.empty((CHUNK + 1, 480, 640), bool)
    for i in range(len(masks)):
        k = (41, 61, 81)[i % 3]
        f = box_blur(box_blur(rng.standard_normal((480, 640)), k), k)
        masks[i] = f > np.quantile(f, (0.5, 0.8, 0.3, 0.9)[i % 4])
    return masks, oracle(masks, 250)


@pytest.mark.parametrize("n", [1, 3, CHUNK + 1])
def test_random_blobs(n):
    masks, want = blob_case()
    # masks 0 .. 2 hold both kinds (checked here on the oracle; seed 11 was chosen on the CPU for it), so n = 3 and
    # n = CHUNK + 1 see changed and unchanged masks in one batch; n = 1 takes an unchanged one
    assert want[1][:3].any() and not want[1][:3].all()
    pick = np.arange(n) if n > 1 else np.nonzero(want[1])[0][:1]
    assert_equals_oracle(device_clean(masks[pick], 250), tuple(w[pick] for w in want), 640)


def test_batch_invariance():
    masks, _ = blob_case()
    hand = np.zeros((2, 480, 640), bool)
    hand[0, :64, :96] = HAND["spiral"][0]
    hand[1, 100:164, 200:296] = HAND["lattice"][0]
    batch = np.concatenate([masks[:CHUNK + 1], hand])
    full = device_clean(batch, 250)
    again = device_clean(batch, 250)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))                       # two runs of the same call
    rev = device_clean(batch[::-1], 250)
    assert all(np.array_equal(a[::-1], b) for a, b in zip(rev, full))                   # reversed within the batch
    for i in (0, 2, CHUNK, len(batch) - 1):                                             # alone; CHUNK sits behind the seam
        alone = device_clean(batch[i:i + 1], 250)
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(alone, full)), i
    pick = np.array([len(batch) - 1, 5, 0, CHUNK, 5])                                   # next to other masks, one of them twice
    some = device_clean(batch[pick], 250)
    assert all(np.array_equal(a, b[pick]) for a, b in zip(some, full))


def test_in_place_and_empty_batch():
    masks, want = blob_case()
    packed = torch.as_tensor(sam_amg.pack_masks(masks[:3]).view(np.int32), device=DEV)
    out, same, boxes, area = sg.clean_masks_packed(packed, 640, 250)
    # the C entry with packed_out == packed
    from pope_amd import _lib
    lib = _lib.lib()
    buf = packed.clone()
    un, bx, ar = (torch.empty(s, dtype=torch.int32, device=DEV) for s in ((3,), (3, 4), (3,)))
    ws = torch.empty(int(lib.pope_sam_small_regions_workspace_bytes(3, 480, 640)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.pope_sam_small_regions_u32(_lib.ptr(buf), 3, 480, 640, 250, _lib.ptr(buf), _lib.ptr(un), _lib.ptr(bx), _lib.ptr(ar),
                                              _lib.ptr(ws), ws.numel(), _lib.stream_of(torch.device(DEV))), "in place")
    assert torch.equal(buf, out) and torch.equal(un.bool(), same) and torch.equal(bx, boxes) and torch.equal(ar, area)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), sam_amg.pack_masks(want[0][:3]))
    # overlapping, but not identical, buffers are refused; a short workspace too
    two = torch.cat([packed, packed])
    assert lib.pope_sam_small_regions_u32(_lib.ptr(two), 3, 480, 640, 250, _lib.ptr(two[1:]), _lib.ptr(un), _lib.ptr(bx), _lib.ptr(ar),
                                          _lib.ptr(ws), ws.numel(), None) == -1
    assert lib.pope_sam_small_regions_u32(_lib.ptr(packed), 3, 480, 640, 250, _lib.ptr(buf), _lib.ptr(un), _lib.ptr(bx), _lib.ptr(ar),
                                          _lib.ptr(ws), ws.numel() - 1, None) == -3
    e = sg.clean_masks_packed(packed[:0], 640, 250)
    assert [tuple(t.shape) for t in e] == [(0, 480, 20), (0,), (0, 4), (0,)]
    m, s, _, _ = sg.clean_masks_packed(torch.zeros(0, 480, 20, dtype=torch.int32, device=DEV), 640, 250)
    assert tuple(sg.unpack_on_device(m, 640).shape) == (0, 480, 640) and tuple(s.shape) == (0,)


# ---- the generator's own survivors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(synth.SAM_GENERATOR_CASES))
def test_fixture_survivors(golden_dir, name):
    fx = golden(golden_dir, name)
    W = synth.SAM_GENERATOR_CASES[name][1][1]
    masks = sam_amg.unpack_masks(fx["packed"], W)
    want = oracle(masks, 250)
    assert (~want[1]).any()
    assert_equals_oracle(device_clean(masks, 250), want, W)


# ---- an independent labelling ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,min_area", [("64x96", 6), ("37x70", 6), ("64x96", 250), ("37x70", 250)])
def test_component_sizes_against_scipy(name, min_area):
    ndimage = pytest.importorskip("scipy.ndimage")
    mask = HAND[name][0]
    words, _, _, _ = device_clean(mask[None], min_area)
    got = sam_amg.unpack_masks(words, mask.shape[1])[0]
    want = oracle(mask[None], min_area)[0][0]

    def sizes(m):
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        return n, sorted(np.bincount(lab.reshape(-1), minlength=n + 1)[1:].tolist())
    for polarity in (False, True):
        assert sizes(got ^ polarity) == sizes(want ^ polarity)
    # the cleaned mask by scipy's components alone: no background component below min_area is left, and either no island
    # below it or exactly one island in all
    n_bg, bg = sizes(~got)
    n_fg, fg = sizes(got)
    assert all(s >= min_area for s in bg)
    assert all(s >= min_area for s in fg) or n_fg == 1
