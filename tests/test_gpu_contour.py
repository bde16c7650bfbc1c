"""GPU: the contours of all regions of a region map (include/dq_hip.h, "region
contours").

The reference is the numpy model of tests/contour_model.py, written from the
rules and using none of the code under test (test_contour_model.py pins it to
OpenCV's loop on one region's mask at a time and to hand-checked literals).
Equality is exact everywhere: array_equal on every array asked for, == on M.

The mechanisms whose edges the shapes sit on: waves of 64 and workgroups of 256
pixels in raster order, scan chunks of 1024 pixels, states or regions with a
second block of the top scan past 2^20 of them; pointer jumping that resolves a
contour of len points after ceil(log2(len - 1)) rounds, sent 4, 4, then 8 at a
time, the round after the last one needed being the one that stops them."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import contour_model as cm
import region_inputs as ri
from region_dev import to_dev

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ARRAYS = ("offsets", "points", "codes", "len", "visits")
GUARD = 0x5A
SIDES = (1, 2, 63, 64, 65, 255, 257, 1023, 1025)
SHAPES = [(s, o) for s in SIDES for o in (5, 67)] + [(o, s) for s in SIDES for o in (5, 67)]   # (height, width)
DTYPES = {"codes": np.uint8, "visits": np.uint8}


def _host(name, t):
    return t.cpu().numpy().view(DTYPES.get(name, np.uint32))


def contours(gpu, reg, nreg, orientation=0, outputs=None, point_capacity=None, stream=None):
    h, w = reg.shape
    total, out = gpu.region_contours_device(to_dev(reg.astype(np.uint32)), w, h, nreg, orientation=orientation,
                                            outputs=outputs, point_capacity=point_capacity, stream=stream)
    got = {k: _host(k, v) for k, v in out.items()}
    got["total"] = total
    return got


def same(got, want, names=ARRAYS + ("total",)):
    for k in names:
        if k == "total":
            assert got[k] == want[k], (k, got[k], want[k])
            continue
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:6].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def check(gpu, reg, nreg, orientation=0):
    want = cm.region_contours(reg, nreg, orientation)
    same(contours(gpu, reg, nreg, orientation), want)
    return want


def blocky(rng, h, w, block, ids, background=None):
    cells = rng.integers(0, ids, ((h + block - 1) // block, (w + block - 1) // block))
    reg = np.kron(cells, np.ones((block, block), np.int64))[:h, :w].astype(np.uint32)
    if background is not None:
        holes = rng.random((h, w)) < 0.05
        reg[holes] = rng.choice(np.array(background, np.uint32), int(holes.sum()))
    return reg


def stripes(h, w, width, along_x):
    line = (np.arange(w if along_x else h, dtype=np.uint32) // width) % 2
    return np.tile(line, (h, 1)) if along_x else np.tile(line[:, None], (1, w))


def shape_maps(h, w):
    """(name, map, R, orientation) of every map a shape is run with."""
    rng = np.random.default_rng(h * 65537 + w)
    yield "whole", np.zeros((h, w), np.uint32), 1, 1
    yield "stripes_x1", stripes(h, w, 1, True), 2, 0
    yield "stripes_y1", stripes(h, w, 1, False), 2, 1
    yield "stripes_x3", stripes(h, w, 3, True), 2, 1
    yield "stripes_y2", stripes(h, w, 2, False), 2, 0
    for block, orientation in ((1, 0), (3, 1), (16, 0)):
        ids = int(rng.integers(2, 6))
        reg = blocky(rng, h, w, block, ids)
        yield "blocks%d" % block, reg, ids, orientation
        yield "blocks%d_background" % block, blocky(rng, h, w, block, ids, background=(ids, ids + 9, NONE)), ids, \
            1 - orientation
        yield "blocks%d_low_r" % block, reg, ids - 1, orientation   # the highest id is background


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % (w, h) for h, w in SHAPES])
def test_every_map_of_a_shape(gpu, shape):
    h, w = shape
    for name, reg, nreg, orientation in shape_maps(h, w):
        try:
            check(gpu, reg, nreg, orientation)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None


# Every contact is diagonal: each id is one component, its contour runs along the frame in a zigzag and
# passes the pixels next to the frame's edge more than once.
@pytest.mark.parametrize("orientation", [0, 1])
def test_the_two_id_checkerboard(gpu, orientation):
    reg = ri.regions_base("checker", 130, 70).astype(np.uint32)
    want = check(gpu, reg, 2, orientation)
    assert want["visits"].max() >= 2 and want["len"].min() > 2 * (130 + 70) - 8


@pytest.mark.parametrize("orientation", [0, 1])
def test_the_spiral(gpu, orientation):
    reg = ri.spiral(67, 65).astype(np.uint32)
    want = check(gpu, reg, 2, orientation)
    # one pixel wide: out along one side and back along the other, a corner cut on its inner side
    assert want["len"].tolist() == [4160, 4420] and want["visits"].max() == 2 and want["visits"].min() == 1


def test_one_region_that_touches_all_four_frame_edges(gpu):
    want = check(gpu, np.zeros((257, 257), np.uint32), 1, 1)
    assert want["len"][0] == 1024 and want["visits"][1:-1, 1:-1].sum() == 0


# ---- the last pointer-jumping round is needed, and is not ---------------------------
def bar(length):
    """A (2, n) map whose one region has a contour of `length` points: a bar 1 high (2 n - 2 points), with a
    pixel under its first one (2 n - 1 points) for an odd length."""
    n = (length + 2) // 2
    reg = np.full((2, n), 3, np.uint32)
    reg[0, :] = 0
    if length % 2:
        reg[1, 0] = 0
    return reg


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6, 8, 12])
def test_contour_lengths_around_a_power_of_two(gpu, k):
    for length in (2 ** k - 1, 2 ** k, 2 ** k + 1, 2 ** k + 2):
        if length < 2:
            continue
        for orientation in (0, 1):
            want = check(gpu, bar(length), 1, orientation)
            assert want["len"][0] == length, (length, want["len"][0])


# ---- many regions, absent ids, background, two components ---------------------------
def test_70000_single_pixel_regions(gpu):
    reg = np.arange(280 * 250, dtype=np.uint32).reshape(250, 280)
    got = contours(gpu, reg, reg.size)
    assert got["total"] == reg.size and (got["len"] == 1).all() and (got["visits"] == 1).all()
    assert np.array_equal(got["offsets"], np.arange(reg.size + 1, dtype=np.uint32))
    yy, xx = np.mgrid[0:250, 0:280]
    assert np.array_equal(got["points"], (xx | yy << 16).astype(np.uint32).reshape(-1)) and (got["codes"] == 8).all()


def test_absent_ids_and_background(gpu):
    reg = blocky(np.random.default_rng(3), 70, 90, 8, 3, background=(12, 40, NONE)) * 3 + 1   # ids 1, 4, 7 of R = 12
    reg[reg > 12] = NONE
    want = check(gpu, reg, 12, 1)
    for r in (0, 2, 3, 5, 6, 8, 11):
        assert want["len"][r] == 0 and want["offsets"][r] == want["offsets"][r + 1]
    assert want["visits"][reg >= 12].sum() == 0


def test_only_the_first_component_of_an_id_is_traced(gpu):
    reg = np.full((40, 150), 9, np.uint32)
    reg[3:6, 100:104] = 0          # the first in raster order: 3 x 4
    reg[10:35, 5:90] = 0           # the larger one
    reg[4, 140:145] = 1
    reg[20:30, 120:140] = 1
    want = check(gpu, reg, 2)
    assert want["len"].tolist() == [10, 8] and want["visits"][10:].sum() == 0


def test_a_ring_and_a_one_pixel_thick_ring(gpu):
    reg = np.full((90, 200), NONE, np.uint32)
    yy, xx = np.mgrid[0:90, 0:200]
    d2 = (yy - 44) ** 2 + (xx - 50) ** 2
    reg[(d2 <= 40 * 40) & (d2 >= 20 * 20)] = 0
    reg[10:80, 110:190] = 1
    reg[11:79, 111:189] = NONE     # one pixel thick: the hole's border is not followed
    want = check(gpu, reg, 2)
    assert want["len"][1] == 2 * (70 + 80) - 4 and want["visits"][reg == 1].max() == 1
    assert want["visits"][(d2 < 30 * 30) & (reg == 0)].sum() == 0    # nothing at the hole of the thick ring


# ---- output handling --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def three_shapes(orientation=0):
    reg = np.full((80, 150), 50, np.uint32)
    reg[4:30, 5:70] = 0
    reg[35:75, 60:70] = 1
    reg[10:70, 90:140] = 2
    reg[30:40, 100:120] = 50   # a hole
    reg[33, 75:88] = 3         # a bar: pixels passed twice
    return reg, cm.region_contours(reg, 5, orientation)


def _guarded(nbytes):   # (bytes, not region_dev's words: the outputs here are u8 and u32)
    import torch
    return torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")


def _raw(gpu, reg, nreg, orientation, cap, skip=(), room=None):
    """The device entry on guarded arrays: `room` entries in the lists (default cap); the arrays as
    flat numpy, the guards checked."""
    import torch
    h, w = reg.shape
    room = cap if room is None else room
    size = {"offsets": 4 * (nreg + 1), "points": 4 * room, "codes": room, "len": 4 * nreg, "visits": h * w}
    t_reg = to_dev(reg)
    t = {k: _guarded(size[k]) for k in ARRAYS if k not in skip}
    p = lambda k: ctypes.c_void_p(t[k].data_ptr()) if k in t else None  # noqa: E731
    torch.cuda.synchronize()
    r = gpu.lib().dq_hip_region_contours_dev(0, ctypes.c_void_p(t_reg.data_ptr()), w, h, nreg, orientation, cap,
                                             *[p(k) for k in ARRAYS], None)
    got = {"total": r}
    for k, v in t.items():
        a = v.cpu().numpy()
        assert (a[size[k]:] == GUARD).all(), k
        got[k] = a[:size[k]].view(DTYPES.get(k, np.uint32))
    if "visits" in got:
        got["visits"] = got["visits"].reshape(h, w)
    return got


@pytest.mark.parametrize("skip", ARRAYS + ("all_but_points", "all_but_codes", "all_but_visits", "all_but_len"))
def test_outputs_null_in_turn(gpu, skip):
    reg, want = three_shapes(1)
    skip = tuple(k for k in ARRAYS if k != skip[8:]) if skip.startswith("all_but_") else (skip,)
    lists = "points" not in skip or "codes" not in skip   # (room without a list is refused)
    got = _raw(gpu, reg, 5, 1, want["total"] if lists else 0, skip)
    assert set(got) == set(ARRAYS + ("total",)) - set(skip)
    same(got, want, tuple(got))


def test_count_only(gpu):
    reg, want = three_shapes()
    got = _raw(gpu, reg, 5, 0, 0, skip=("points", "codes"))
    same(got, want, ("total", "offsets", "len", "visits"))
    got = _raw(gpu, reg, 5, 0, 0, skip=("points", "codes", "offsets", "visits"))
    same(got, want, ("total", "len"))


def test_lists_that_do_not_fit_stay_untouched(gpu):
    reg, want = three_shapes()
    m = want["total"]
    got = _raw(gpu, reg, 5, 0, m - 1, room=m)
    assert (got["points"].view(np.uint8) == GUARD).all() and (got["codes"] == GUARD).all()
    same(got, want, ("total", "offsets", "len", "visits"))
    same(_raw(gpu, reg, 5, 0, m), want)
    same(_raw(gpu, reg, 5, 0, m + 5, room=m), want)    # room to spare: nothing behind entry M is written
    same(_raw(gpu, reg, 5, 0, 1 << 40, room=m), want)


def test_the_wrapper_counts_then_fills(gpu):
    reg, want = three_shapes(1)
    same(contours(gpu, reg, 5, 1), want)
    got = contours(gpu, reg, 5, 1, outputs=("codes", "len"))
    assert set(got) == {"codes", "len", "total"}
    same(got, want, ("codes", "len", "total"))
    got = contours(gpu, reg, 5, 1, outputs=("visits",))
    same(got, want, ("visits", "total"))
    got = contours(gpu, reg, 5, 1, point_capacity=want["total"] + 3)
    assert got["points"].size == want["total"] + 3
    assert np.array_equal(got["points"][:want["total"]], want["points"])


def test_the_host_entry(gpu):
    for orientation in (0, 1):
        reg, want = three_shapes(orientation)
        same(gpu.region_contours(reg, 5, orientation=orientation), want)
    reg, want = three_shapes()
    same(gpu.region_contours(reg.astype(np.uint8), 5), want)
    none = np.full((3, 4), 7, np.uint32)              # no region pixel at all: M = 0
    got = gpu.region_contours(none, 2)
    same(got, cm.region_contours(none, 2))
    assert got["total"] == 0 and got["points"].size == 0


def test_two_calls_overlap_on_two_streams(gpu):
    import torch
    rng = np.random.default_rng(8)
    maps = [(blocky(rng, 257, 300, 16, 4), 4, 0), (blocky(rng, 130, 513, 48, 3, background=(3, NONE)), 3, 1)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in maps]
    got, errors = [None] * 2, []

    def work(i):
        try:
            torch.cuda.set_device(0)
            for _ in range(3):
                got[i] = contours(gpu, *maps[i], stream=streams[i])
        except BaseException as e:   # noqa: B036 (reported by the test's thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i in range(2):
        same(got[i], cm.region_contours(*maps[i]))


# ---- at size ----------------------------------------------------------------------
# The checkerboard: every pixel off the frame's edge is a border pixel with four states.
def test_past_2_to_the_20_border_states(gpu):
    reg = ri.regions_base("checker", 520, 520).astype(np.uint32)
    bits = cm.neighbour_bits(reg, 2)
    assert sum(int((bits >> d & 1).sum()) for d in range(8)) > 1 << 20
    check(gpu, reg, 2)


def test_past_2_to_the_20_pixels(gpu):
    reg = blocky(np.random.default_rng(1025), 1025, 1025, 8, 6, background=(6, NONE))
    assert reg.size > 1 << 20
    want = check(gpu, reg, 6, 1)
    assert want["total"] > 6 * 32
