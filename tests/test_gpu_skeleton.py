"""GPU: the skeletons of all regions of a region map (include/dq_hip.h, "region
skeleton").

The reference is the numpy model of tests/skeleton_model.py, written from the
rules and using none of the code under test (test_skeleton_model.py pins it to
scalar loops over one region's mask at a time and to hand-checked literals).
Equality is exact everywhere: array_equal on every array asked for, == on the
return, on `iterations` and on `converged`.

The mechanisms whose edges the shapes sit on: words of 64 pixels along x; tiles
of 384 x 64 pixels (6 words x 64 rows) with a halo of 32 rows above and below and
one word to either side, 32 pixels of which 16 iterations use up; 16 iterations
per launch; launches sent 2, 4, then 8 at a time."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import skeleton_model as sm
from region_dev import to_dev

pytestmark = pytest.mark.gpu

NONE = sm.NONE
ARRAYS = ("skel", "skeled", "when", "skel_area", "thick")
WORDS = ("kept", "iterations", "converged")
GUARD = 0x5A
K = 16                      # iterations per launch
TILE_W, TILE_H, HALO = 384, 64, 32
SIDES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 257, HALO - 1, HALO + 1, TILE_W - 1, TILE_W + 1)
SHAPES = [(s, o) for s in SIDES for o in (5, 67)] + [(o, s) for s in SIDES for o in (5, 67)]   # (height, width)
DTYPES = {"skel": np.uint8, "when": np.uint16}


def _host(name, t):
    return t.cpu().numpy().view(DTYPES.get(name, np.uint32))


def skeleton(gpu, reg, nreg, max_iters=0, outputs=None, stream=None):
    h, w = reg.shape
    kept, out = gpu.region_skeleton_device(to_dev(reg.astype(np.uint32)), w, h, nreg, max_iters=max_iters,
                                           outputs=outputs, stream=stream)
    got = {k: (_host(k, v) if k in ARRAYS else v) for k, v in out.items()}
    got["kept"] = kept
    return got


def same(got, want, names=ARRAYS + WORDS):
    for k in names:
        if k in WORDS:
            assert got[k] == want[k], (k, got[k], want[k])
            continue
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:6].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def check(gpu, reg, nreg, max_iters=0):
    want = sm.region_skeleton(reg, nreg, max_iters)
    same(skeleton(gpu, reg, nreg, max_iters), want)
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
    """(name, map, R) of every map a shape is run with."""
    rng = np.random.default_rng(h * 65537 + w)
    yield "whole", np.zeros((h, w), np.uint32), 1
    for width in (1, 2, 3):
        yield "stripes_x%d" % width, stripes(h, w, width, True), 2
        yield "stripes_y%d" % width, stripes(h, w, width, False), 2
    for block in (1, 3, 16):
        ids = int(rng.integers(2, 6))
        reg = blocky(rng, h, w, block, ids)
        yield "blocks%d" % block, reg, ids
        yield "blocks%d_background" % block, blocky(rng, h, w, block, ids, background=(ids, ids + 9, NONE)), ids
        yield "blocks%d_low_r" % block, reg, ids - 1   # the highest id is background


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % (w, h) for h, w in SHAPES])
def test_every_map_of_a_shape(gpu, shape):
    h, w = shape
    for name, reg, nreg in shape_maps(h, w):
        try:
            check(gpu, reg, nreg)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None


# Two 8 x 8 blocks that touch by one corner only, the contact lying exactly on a
# word boundary (x = 63 | 64) or on a tile corner (x = 383 | 384), and on a tile
# row boundary (y = 63 | 64 for the NW-SE contacts, y = 127 | 128 for the NE-SW
# ones).  With the same id the pair is one region joined through the corner.
@pytest.mark.parametrize("ids", ["same_id", "different_ids"])
def test_diagonal_contacts_on_word_and_tile_borders(gpu, ids):
    reg = np.full((200, 460), 7, np.uint32)
    other = 0 if ids == "same_id" else 1
    for x in (64, TILE_W):
        reg[56:64, x - 8:x], reg[64:72, x:x + 8] = 0, other          # (x - 1, 63) meets (x, 64)
        reg[120:128, x:x + 8], reg[128:136, x - 8:x] = 0, other      # (x, 127) meets (x - 1, 128)
    want = check(gpu, reg, 2)
    assert want["kept"] == (38 if ids == "same_id" else 8), want["kept"]   # (a block alone keeps one pixel)
    check(gpu, reg.T.copy(), 2)


def test_the_two_id_checkerboard(gpu):
    yy, xx = np.mgrid[0:70, 0:130]
    want = check(gpu, ((yy + xx) % 2).astype(np.uint32), 2)
    assert want["kept"] == 70 * 130 and want["iterations"] == 0 and want["converged"] == 1


# ---- the front crosses many tiles at different times ----------------------------
@functools.lru_cache(maxsize=None)
def square_257():
    reg = np.zeros((257, 257), np.uint32)
    return reg, sm.region_skeleton(reg, 1)


def test_the_257_square(gpu):
    reg, want = square_257()
    assert want["iterations"] == 128 and want["kept"] == 1 and want["skel"][128, 128] == 1
    same(skeleton(gpu, reg, 1), want)


def test_a_right_triangle(gpu):
    yy, xx = np.mgrid[0:300, 0:301]
    check(gpu, np.where(xx <= yy, 0, 5).astype(np.uint32), 1)


def test_a_ring_a_bar_and_a_block(gpu):
    reg = np.full((150, 420), NONE, np.uint32)
    yy, xx = np.mgrid[0:150, 0:420]
    d2 = (yy - 74) ** 2 + (xx - 72) ** 2
    reg[(d2 <= 70 * 70) & (d2 >= 30 * 30)] = 0
    reg[5:145, 150:155] = 1            # a bar 5 wide beside the ring
    reg[40:100, 300:400] = 2           # a 100 x 60 block that straddles x = 384
    want = check(gpu, reg, 3)
    assert want["thick"].tolist() == [26, 2, 30]


# One region around a whole tile (x 384..767, y 64..127), `margin` pixels to every side of it: no
# launch deletes in that tile until the front has eaten the margin (launch 1 for 20, launch 2 for 36).
# Its eight neighbours delete in every launch, so the tile must run in every launch although its own
# flag is clear: a skip rule that looks at the tile alone leaves it asleep.  A frame under 384 wide
# has one column of tiles, and each of them holds the region's left and right edge: this is the
# smallest frame with a tile that is quiet before the front arrives.
@pytest.mark.parametrize("margin", [20, 36])
def test_a_quiet_tile_runs_while_its_neighbours_delete(gpu, margin):
    assert K < margin
    reg = np.full((2 * TILE_H + margin + 6, 2 * TILE_W + margin + 6), 4, np.uint32)
    reg[TILE_H - margin:2 * TILE_H + margin, TILE_W - margin:2 * TILE_W + margin] = 0
    want = check(gpu, reg, 1)
    inside = want["when"][TILE_H:2 * TILE_H, TILE_W:2 * TILE_W]
    assert inside[inside > 0].min() == margin + 1 and want["iterations"] == TILE_H // 2 + margin   # (0: the skeleton)


# The same around a 3 x 3 block of tiles (x 384..1535, y 64..255).  In the first launch the front
# eats 16 of the 20 pixels of margin and no tile of the block deletes, so in the second launch the
# middle tile really is skipped: its flag is cleared and its core is not written.  The eight around
# it delete in that launch, so it is woken in the third, reads the plane it did not write, runs
# without deleting until the front has crossed the tile above or below, and deletes from
# iteration 85 on.
def test_a_skipped_tile_is_woken_by_its_neighbours(gpu):
    margin = 20
    assert K < margin < 2 * K
    reg = np.full((4 * TILE_H + margin + 6, 4 * TILE_W + margin + 6), 4, np.uint32)
    reg[TILE_H - margin:4 * TILE_H + margin, TILE_W - margin:4 * TILE_W + margin] = 0
    want = check(gpu, reg, 1)
    block = want["when"][TILE_H:4 * TILE_H, TILE_W:4 * TILE_W]
    middle = want["when"][2 * TILE_H:3 * TILE_H, 2 * TILE_W:3 * TILE_W]
    assert block[block > 0].min() == margin + 1 and middle[middle > 0].min() == margin + TILE_H + 1
    assert want["iterations"] == 3 * TILE_H // 2 + margin
    check(gpu, reg, 1, max_iters=2 * K + 8)   # (ends in the launch that wakes the tile)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_blocks_of_48(gpu, seed):
    rng = np.random.default_rng(480 + seed)
    check(gpu, blocky(rng, 290, 300 + 40 * seed, 48, 2 + seed), 2 + seed)


# ---- max_iters ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slab():
    reg = np.full((70, 100), 3, np.uint32)
    reg[:, :97] = 0
    return reg, sm.region_skeleton(reg, 1)


@pytest.mark.parametrize("m", [1, 2, K - 1, K, K + 1])
def test_max_iters(gpu, m):
    reg, full = slab()
    assert full["iterations"] > K + 1
    got = skeleton(gpu, reg, 1, max_iters=m)
    want = sm.region_skeleton(reg, 1, m)
    assert want["iterations"] == m and want["converged"] == 0
    assert np.array_equal(want["when"], np.where(full["when"] <= m, full["when"], 0))   # the unbounded run, cut
    same(got, want)


def test_max_iters_2k_plus_1_on_the_257_square(gpu):
    reg, full = square_257()
    got = skeleton(gpu, reg, 1, max_iters=2 * K + 1)
    assert got["iterations"] == 2 * K + 1 and got["converged"] == 0
    assert np.array_equal(got["when"], np.where(full["when"] <= 2 * K + 1, full["when"], 0))
    assert np.array_equal(got["skel"], ((full["when"] == 0) | (full["when"] > 2 * K + 1)).astype(np.uint8))


def test_max_iters_where_the_run_ends_by_itself(gpu):
    reg, full = slab()
    for m in (full["iterations"], full["iterations"] + 1):
        want = sm.region_skeleton(reg, 1, m)
        assert want["converged"] == (0 if m == full["iterations"] else 1)
        same(skeleton(gpu, reg, 1, max_iters=m), want)


def test_a_map_that_is_a_skeleton_already(gpu):
    reg = np.full((90, 140), 9, np.uint32)
    reg[10, 5:130], reg[10:80, 64], reg[40, 64:135] = 0, 0, 1
    want = check(gpu, reg, 2)
    assert want["iterations"] == 0 and want["converged"] == 1 and want["kept"] == int((reg < 2).sum())


# ---- many regions, absent ids -----------------------------------------------------
def test_70000_single_pixel_regions(gpu):
    reg = np.arange(280 * 250, dtype=np.uint32).reshape(250, 280)
    got = skeleton(gpu, reg, reg.size)
    assert got["kept"] == reg.size and got["iterations"] == 0 and got["converged"] == 1
    assert np.array_equal(got["skeled"], reg) and got["skel"].all() and not got["when"].any()
    assert (got["skel_area"] == 1).all() and not got["thick"].any()


def test_absent_ids(gpu):
    reg = blocky(np.random.default_rng(3), 70, 90, 8, 3) * 3 + 1   # ids 1, 4, 7 of R = 12
    want = check(gpu, reg, 12)
    for r in (0, 2, 3, 5, 6, 8, 11):
        assert want["skel_area"][r] == 0 and want["thick"][r] == 0


# ---- output handling --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def three_shapes():
    reg = np.full((80, 150), 50, np.uint32)
    reg[4:30, 5:70] = 0
    reg[35:75, 60:70] = 1
    reg[10:70, 90:140] = 2
    reg[30:40, 100:120] = 50   # a hole
    return reg, sm.region_skeleton(reg, 4)


def _guarded(nbytes):   # (bytes, not region_dev's words: the outputs here are u8, u16 and u32)
    import torch
    return torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")


def _raw(gpu, reg, nreg, skip, words=True):
    import torch
    h, w = reg.shape
    size = {"skel": h * w, "skeled": 4 * h * w, "when": 2 * h * w}
    t_reg = to_dev(reg)
    t = {k: _guarded(size.get(k, 4 * nreg)) for k in ARRAYS if k not in skip}
    p = lambda k: ctypes.c_void_p(t[k].data_ptr()) if k in t else None  # noqa: E731
    its, conv = ctypes.c_uint32(77), ctypes.c_uint32(77)
    tail = (ctypes.byref(its), ctypes.byref(conv)) if words else (None, None)
    torch.cuda.synchronize()
    r = gpu.lib().dq_hip_region_skeleton_dev(0, ctypes.c_void_p(t_reg.data_ptr()), w, h, nreg, 0, *[p(k) for k in ARRAYS],
                                             *tail, None)
    got = {"kept": r, "iterations": its.value, "converged": conv.value}
    for k, v in t.items():
        a = v.cpu().numpy()
        assert (a[-64:] == GUARD).all(), k
        a = a[:-64].view(DTYPES.get(k, np.uint32))
        got[k] = a.reshape((h, w) if k in size else (nreg,))
    return got


@pytest.mark.parametrize("skip", ARRAYS + ("all_but_thick", "all_but_skel"))
def test_outputs_null_in_turn(gpu, skip):
    reg, want = three_shapes()
    skip = tuple(k for k in ARRAYS if k != skip[8:]) if skip.startswith("all_but_") else (skip,)
    got = _raw(gpu, reg, 4, skip)
    assert set(got) == set(ARRAYS + WORDS) - set(skip)
    same(got, want, tuple(got))


def test_the_host_words_may_be_null(gpu):
    reg, want = three_shapes()
    got = _raw(gpu, reg, 4, (), words=False)
    assert got["iterations"] == 77 and got["converged"] == 77
    same(got, want, ARRAYS + ("kept",))


def test_skeled_in_place(gpu):
    reg, want = three_shapes()
    t_reg = to_dev(reg)
    kept, out = gpu.region_skeleton_device(t_reg, reg.shape[1], reg.shape[0], 4, outputs=("skeled", "thick"),
                                           t_skeled=t_reg)
    assert kept == want["kept"] and out["skeled"] is t_reg
    assert np.array_equal(_host("skeled", t_reg), want["skeled"])
    assert np.array_equal(_host("thick", out["thick"]), want["thick"])


def test_the_host_entry(gpu):
    reg, want = three_shapes()
    same(gpu.region_skeleton(reg, 4), want)
    same(gpu.region_skeleton(reg.astype(np.uint8), 4), want)
    m = 5
    same(gpu.region_skeleton(reg, 4, max_iters=m), sm.region_skeleton(reg, 4, m))


def test_two_calls_overlap_on_two_streams(gpu):
    import torch
    rng = np.random.default_rng(8)
    maps = [(blocky(rng, 257, 300, 16, 4), 4), (blocky(rng, 130, 513, 48, 3, background=(3, NONE)), 3)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in maps]
    got, errors = [None] * 2, []

    def work(i):
        try:
            torch.cuda.set_device(0)
            for _ in range(3):
                got[i] = skeleton(gpu, *maps[i], stream=streams[i])
        except BaseException as e:   # noqa: B036 (reported by the test's thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i in range(2):
        same(got[i], sm.region_skeleton(*maps[i]))


# ---- at size ----------------------------------------------------------------------
# Just past 2^20 pixels: 17 rows of tiles and 3 columns, 17425 words per plane.
def test_past_2_to_the_20_pixels(gpu):
    reg = blocky(np.random.default_rng(1025), 1025, 1025, 8, 6, background=(6, NONE))
    assert reg.size > 1 << 20
    want = check(gpu, reg, 6)
    assert 2 <= want["iterations"] < 40
