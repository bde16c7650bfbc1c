"""GPU: the distance transform, the centres and the cores of a region map
(include/dq_hip.h, "region distance").

The reference is the numpy model of tests/distance_model.py, written from the
definition and using none of the code under test (test_distance_model.py pins
it to brute force, scipy and hand-worked literals).  Equality is exact
everywhere: array_equal on every output array, == on the return.

Shapes: one side from {1, 2, 63, 64, 65, 255, 257, 1023, 1025, 2049, 4097},
the other 5 or 67, both orientations: every power-of-two band and chunk up to
4096 is crossed, with one and with two row chunks beside it.  Each case is a
few hundred thousand pixels at most."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import distance_model as dm
from region_dev import to_dev

pytestmark = pytest.mark.gpu

NONE = dm.NONE
DISTANCE = ("dist", "dmax", "bbox", "thresh", "count", "centre")
CORES = ("core", "cored", "centre", "core_area", "dist")
GUARD = 0x5A
SIDES = (1, 2, 63, 64, 65, 255, 257, 1023, 1025, 2049, 4097)
SHAPES = [(s, o) for s in SIDES for o in (5, 67)] + [(o, s) for s in SIDES for o in (5, 67)]   # (height, width)


def coord(x, y):
    return x | y << 16


def _host(name, t):
    a = t.cpu().numpy()
    return a.view({"dist": np.uint16, "core": np.uint8}.get(name, np.uint32))


def distance(gpu, reg, nreg, rule=0, outputs=None, stream=None):
    h, w = reg.shape
    out = gpu.region_distance_device(to_dev(reg.astype(np.uint32)), w, h, nreg, rule=rule, outputs=outputs,
                                     stream=stream)
    return {k: _host(k, v) for k, v in out.items()}


def cores(gpu, reg, nreg, rule=0, connectivity=8, outputs=None):
    h, w = reg.shape
    kept, out = gpu.region_cores_device(to_dev(reg.astype(np.uint32)), w, h, nreg, rule=rule, connectivity=connectivity,
                                        outputs=outputs)
    got = {k: _host(k, v) for k, v in out.items()}
    got["kept"] = kept
    return got


def same(got, want, names):
    for k in names:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:6].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def check_distance(gpu, reg, nreg, rule=0):
    want = dm.region_values(reg, nreg, rule)
    same(distance(gpu, reg, nreg, rule), want, DISTANCE)
    return want


def check_cores(gpu, reg, nreg, rule=0, connectivity=8):
    v = dm.region_values(reg, nreg, rule)
    want = dict(dm.region_cores(reg, nreg, v["centre"], connectivity), centre=v["centre"], dist=v["dist"])
    got = cores(gpu, reg, nreg, rule, connectivity)
    same(got, want, CORES)
    assert got["kept"] == want["kept"] == int(want["core_area"].sum())
    return want


def blocky(rng, h, w, block, ids, background=False):
    cells = rng.integers(0, ids, ((h + block - 1) // block, (w + block - 1) // block))
    reg = np.kron(cells, np.ones((block, block), np.int64))[:h, :w].astype(np.uint32)
    if background:
        reg[rng.random((h, w)) < 0.05] = 77
    return reg


def shape_maps(h, w):
    """(name, map, R) of every map a shape is run with."""
    rng = np.random.default_rng(h * 65537 + w)
    yield "whole", np.zeros((h, w), np.uint32), 1
    yield "stripes_x", np.tile(np.arange(w, dtype=np.uint32) % 2, (h, 1)), 2
    yield "stripes_y", np.tile((np.arange(h, dtype=np.uint32) % 2)[:, None], (1, w)), 2
    three = np.zeros((h, w), np.uint32)   # the middle one spans the long side but for a pixel at either end
    if w >= h:
        three[:, :1], three[:, w - 1:] = 1, 2
    else:
        three[:1, :], three[h - 1:, :] = 1, 2
    yield "three", three, 3
    for block in (1, 3, 16):
        ids = int(rng.integers(2, 6))
        reg = blocky(rng, h, w, block, ids)
        yield "blocks%d" % block, reg, ids
        yield "blocks%d_background" % block, blocky(rng, h, w, block, ids, background=True), ids
        yield "blocks%d_low_r" % block, reg, ids - 1   # the highest id is background


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % (w, h) for h, w in SHAPES])
def test_every_map_of_a_shape(gpu, shape):
    h, w = shape
    for name, reg, nreg in shape_maps(h, w):
        try:
            check_distance(gpu, reg, nreg)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None


@pytest.mark.parametrize("shape", [(5, 63), (67, 65), (257, 5), (64, 67)], ids=str)
@pytest.mark.parametrize("connectivity", [4, 8])
def test_cores_of_the_random_maps(gpu, shape, connectivity):
    h, w = shape
    for name, reg, nreg in shape_maps(h, w):
        try:
            check_cores(gpu, reg, nreg, connectivity=connectivity)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None


# A pixel whose nearest other-id pixel is the foot of a tall notch in the next
# row chunk (column 64) or the next row band (row 32): reached only through g.
@pytest.mark.parametrize("turned", [False, True])
def test_a_tall_notch_beside_a_chunk_edge(gpu, turned):
    reg = np.zeros((400, 130), np.uint32)
    reg[:151, 64] = 1
    reg[:300, 32] = 1
    want_at = dm.region_values(reg, 2)["dist"]
    assert want_at[160, 60] == 4 + 10 and want_at[160, 68] == 4 + 10   # through g(64, 160) = 10, from either chunk
    check_distance(gpu, reg.T.copy() if turned else reg, 2)
    check_distance(gpu, reg.T.copy() if turned else reg, 1)


def test_70000_single_pixel_regions(gpu):
    reg = np.arange(280 * 250, dtype=np.uint32).reshape(250, 280)
    want = check_distance(gpu, reg, reg.size)
    assert (want["dmax"] == 1).all() and (want["count"] == 1).all()
    got = cores(gpu, reg, reg.size, outputs=("cored", "core_area"))
    assert got["kept"] == reg.size and np.array_equal(got["cored"], reg) and (got["core_area"] == 1).all()


def test_absent_ids(gpu):
    reg = blocky(np.random.default_rng(3), 70, 90, 8, 3) * 3 + 1   # ids 1, 4, 7 of R = 12
    want = check_distance(gpu, reg, 12)
    for r in (0, 2, 3, 5, 6, 8, 11):
        assert want["dmax"][r] == want["count"][r] == want["thresh"][r] == 0 and want["centre"][r] == NONE
        assert want["bbox"][r].tolist() == [NONE, NONE, 0, 0]
    assert check_cores(gpu, reg, 12)["core_area"][[0, 2, 3]].tolist() == [0, 0, 0]


@functools.lru_cache(maxsize=None)
def centre_literals():
    """One map holding the shapes of the model test's literals and a C, each its own id, on background 99."""
    reg = np.full((40, 60), 99, np.uint32)
    reg[1, 1] = 0                    # one pixel
    reg[1, 4:6] = 1                  # two in a row: the left one
    reg[4:6, 1] = 2                  # two in a column: the lower one
    reg[4:8, 4:8] = 3                # 4 x 4: four maxima, the centroid is one of them
    reg[10:17, 1:8] = 4              # a ring 2 wide: the centroid lies in the hole
    reg[12:15, 3:6] = 99
    reg[20:35, 10:25] = 5            # a C 3 wide: the centroid lies in the opening
    reg[23:32, 13:25] = 99
    want = {0: coord(1, 1), 1: coord(4, 1), 2: coord(1, 5), 3: coord(5, 5), 4: coord(2, 11)}
    return reg, want


def test_the_centre_literals(gpu):
    reg, centres = centre_literals()
    want = check_distance(gpu, reg, 6)
    for r, c in centres.items():
        assert want["centre"][r] == c, (r, hex(int(want["centre"][r])), hex(c))
    c = int(want["centre"][5])
    assert want["count"][5] > 2 and reg[c >> 16, c & 0xFFFF] == 5   # the C: searched, on the C
    check_cores(gpu, reg, 6)
    check_distance(gpu, reg, 6, rule=1)


def _strip(sizes):
    """Rectangles (w, h) of own ids on background, shelf-packed 1 pixel apart into a frame about 1200 wide."""
    x = y = shelf = 0
    at = []
    for w, h in sizes:
        if x and x + w > 1200:
            x, y, shelf = 0, y + shelf + 1, 0
        at.append((x, y))
        x, shelf = x + w + 1, max(shelf, h)
    reg = np.full((y + shelf, max(px + w for (px, _), (w, _) in zip(at, sizes))), len(sizes) + 5, np.uint32)
    for r, ((px, py), (w, h)) in enumerate(zip(at, sizes)):
        reg[py:py + h, px:px + w] = r
    return reg


SWEEPS = {
    "squares_1_90": [(s, s) for s in range(1, 91)],
    "squares_91_120": [(s, s) for s in range(91, 121)],
    "squares_121_132": [(s, s) for s in range(121, 133)],
    "squares_133_142": [(s, s) for s in range(133, 143)],
    "squares_143_150": [(s, s) for s in range(143, 151)],
    "wide_1_150": [(s, 3) for s in range(1, 151)],
    "tall_1_150": [(3, s) for s in range(1, 151)],
}


# The check of the device's FP64 sqrt and /: the thresholds of the 8-bit scale.
@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_the_threshold_sweep(gpu, name):
    sizes = SWEEPS[name]
    reg = _strip(sizes)
    assert reg.size < 450000
    want = dm.region_values(reg, len(sizes), rule=1)
    for r, (w, h) in enumerate(sizes):
        assert want["bbox"][r].tolist()[2] - want["bbox"][r].tolist()[0] + 1 == w
        assert want["thresh"][r] == dm.thresh_by_walk(int(want["dmax"][r]), w, h)
    got = distance(gpu, reg, len(sizes), rule=1)
    same(got, want, ("thresh", "count"))
    same(got, want, DISTANCE)


def _two_blobs(gap_id):
    reg = np.full((30, 50), gap_id, np.uint32)
    reg[2:12, 2:12] = 0      # two separate blobs of equal dmax
    reg[15:25, 30:40] = 0
    reg[2:6, 20:24] = 1      # two blobs joined only by a corner
    reg[6:12, 24:30] = 1
    return reg


@pytest.mark.parametrize("gap", ["region", "background"])
def test_cores_of_blobs(gpu, gap):
    reg = _two_blobs(2 if gap == "region" else 50)
    nreg = 3 if gap == "region" else 2
    want8 = check_cores(gpu, reg, nreg, connectivity=8)
    want4 = check_cores(gpu, reg, nreg, connectivity=4)
    assert want8["core_area"][:2].tolist() == [100, 16 + 36] and want4["core_area"][:2].tolist() == [100, 36]
    assert want8["kept"] - want4["kept"] == 16


# Every output NULL in turn; 64 guard bytes behind every output given.
def _guarded(nbytes):   # (bytes, not region_dev's words: the outputs here are u8, u16 and u32)
    import torch
    t = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    return t


def _raw(gpu, call, reg, nreg, names, skip, extra, stream=None):
    h, w = reg.shape
    size = {"dist": 2 * h * w, "core": h * w, "cored": 4 * h * w, "bbox": 16 * nreg}
    t_reg = to_dev(reg)
    t = {k: _guarded(size.get(k, 4 * nreg)) for k in names if k not in skip}
    p = lambda k: ctypes.c_void_p(t[k].data_ptr()) if k in t else None  # noqa: E731
    import torch
    torch.cuda.synchronize()
    r = getattr(gpu.lib(), call)(0, ctypes.c_void_p(t_reg.data_ptr()), w, h, nreg, *extra, *[p(k) for k in names], stream)
    got = {}
    for k, v in t.items():
        a = v.cpu().numpy()
        assert (a[-64:] == GUARD).all(), k
        a = a[:-64].view({"dist": np.uint16, "core": np.uint8}.get(k, np.uint32))
        got[k] = a.reshape({"dist": (h, w), "core": (h, w), "cored": (h, w), "bbox": (nreg, 4)}.get(k, (nreg,)))
    return r, got


@pytest.mark.parametrize("skip", DISTANCE + ("all_but_centre",))
def test_distance_outputs_null_in_turn(gpu, skip):
    reg, _ = centre_literals()
    want = dm.region_values(reg, 6)
    skip = tuple(k for k in DISTANCE if k != "centre") if skip == "all_but_centre" else (skip,)
    r, got = _raw(gpu, "dq_hip_region_distance_dev", reg, 6, DISTANCE, skip, (0,))
    assert r == 0 and set(got) == set(DISTANCE) - set(skip)
    same(got, want, tuple(got))


@pytest.mark.parametrize("skip", CORES + ("all_but_core_area",))
def test_cores_outputs_null_in_turn(gpu, skip):
    reg, _ = centre_literals()
    v = dm.region_values(reg, 6)
    want = dict(dm.region_cores(reg, 6, v["centre"]), centre=v["centre"], dist=v["dist"])
    skip = tuple(k for k in CORES if k != "core_area") if skip == "all_but_core_area" else (skip,)
    r, got = _raw(gpu, "dq_hip_region_cores_dev", reg, 6, CORES, skip, (0, 8))
    assert r == want["kept"] and set(got) == set(CORES) - set(skip)
    same(got, want, tuple(got))


def test_cored_in_place(gpu):
    reg = _two_blobs(50)
    v = dm.region_values(reg, 2)
    want = dm.region_cores(reg, 2, v["centre"], 4)
    t_reg = to_dev(reg)
    kept, out = gpu.region_cores_device(t_reg, reg.shape[1], reg.shape[0], 2, connectivity=4, outputs=("cored",),
                                        t_cored=t_reg)
    assert kept == want["kept"] and np.array_equal(_host("cored", t_reg), want["cored"])


def test_the_host_entries(gpu):
    reg, _ = centre_literals()
    for rule in (0, 1):
        want = dm.region_values(reg, 6, rule)
        same(gpu.region_distance(reg, 6, rule=rule), want, DISTANCE)
        same(gpu.region_distance(reg.astype(np.uint8), 6, rule=rule), want, DISTANCE)
    v = dm.region_values(reg, 6)
    want = dict(dm.region_cores(reg, 6, v["centre"], 4), centre=v["centre"], dist=v["dist"])
    got = gpu.region_cores(reg, 6, connectivity=4)
    same(got, want, CORES)
    assert got["kept"] == want["kept"]


def test_two_calls_overlap_on_two_streams(gpu):
    import torch
    rng = np.random.default_rng(8)
    maps = [(blocky(rng, 257, 300, 16, 4), 4), (blocky(rng, 130, 513, 3, 5, background=True), 5)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in maps]
    got, errors = [None] * 2, []

    def work(i):
        try:
            torch.cuda.set_device(0)
            reg, nreg = maps[i]
            for _ in range(3):
                if i == 0:
                    got[i] = distance(gpu, reg, nreg, stream=streams[i])
                else:
                    h, w = reg.shape
                    kept, out = gpu.region_cores_device(to_dev(reg), w, h, nreg, stream=streams[i])
                    got[i] = dict({k: _host(k, v) for k, v in out.items()}, kept=kept)
        except BaseException as e:   # noqa: B036 (reported by the test's thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    same(got[0], dm.region_values(*maps[0]), DISTANCE)
    v = dm.region_values(*maps[1])
    want = dict(dm.region_cores(*maps[1], v["centre"]), centre=v["centre"], dist=v["dist"])
    same(got[1], want, CORES)
    assert got[1]["kept"] == want["kept"]
