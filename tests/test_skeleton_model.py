"""CPU: the numpy model of the skeleton stage (tests/skeleton_model.py) against
an independent statement of rules 1-4 of include/dq_hip.h, "region skeleton":
scalar loops, pixel by pixel, over ONE region's zero-padded 0/1 mask at a time,
the way the reference thins a mask.  Then hand-checked literals."""
import numpy as np
import pytest

import skeleton_model as sm


def thin_one_mask(mask, max_iters=0):
    """(kept mask, when, iterations) of one 0/1 mask by scalar loops."""
    h, w = mask.shape
    cur = [[0] * (w + 2) for _ in range(h + 2)]
    for y in range(h):
        for x in range(w):
            cur[y + 1][x + 1] = int(mask[y, x])
    when = np.zeros((h, w), np.uint16)

    def sub(src, second):
        dst = [row[:] for row in src]
        for y in range(1, h + 1):
            for x in range(1, w + 1):
                if not src[y][x]:
                    continue
                n0, n1, n2 = src[y - 1][x - 1], src[y - 1][x], src[y - 1][x + 1]
                n3, n4, n5 = src[y][x + 1], src[y + 1][x + 1], src[y + 1][x]
                n6, n7 = src[y + 1][x - 1], src[y][x - 1]
                c = ((not n1) and (n2 or n3)) + ((not n3) and (n4 or n5)) + ((not n5) and (n6 or n7)) + \
                    ((not n7) and (n0 or n1))
                if c != 1:
                    continue
                na = (n0 or n1) + (n2 or n3) + (n4 or n5) + (n6 or n7)
                nb = (n1 or n2) + (n3 or n4) + (n5 or n6) + (n7 or n0)
                if min(na, nb) not in (2, 3):
                    continue
                side = ((n5 or n6 or not n0) and n7) if second else ((n1 or n2 or not n4) and n3)
                if not side:
                    dst[y][x] = 0
        return dst

    iterations = 0
    it = 0
    while max_iters == 0 or it < max_iters:
        it += 1
        nxt = sub(sub(cur, False), True)
        deleted = False
        for y in range(h):
            for x in range(w):
                if cur[y + 1][x + 1] and not nxt[y + 1][x + 1]:
                    when[y, x] = it
                    deleted = True
        cur = nxt
        if not deleted:
            break
        iterations = it
    kept = np.array([row[1:w + 1] for row in cur[1:h + 1]], np.uint8).reshape(h, w)
    return kept, when, iterations


def region_by_region(reg, nreg, max_iters=0):
    skel = np.zeros(reg.shape, np.uint8)
    when = np.zeros(reg.shape, np.uint16)
    thick = np.zeros(nreg, np.uint32)
    for r in range(nreg):
        kept, w, its = thin_one_mask(reg == r, max_iters)
        skel |= kept
        when = np.maximum(when, w)
        thick[r] = its
    return skel, when, thick


def random_map(rng):
    h, w = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    block = int(rng.choice([1, 2, 3, 5]))
    ids = int(rng.integers(1, 5))
    background = [ids, ids + 3, 0xFFFFFFFF][int(rng.integers(0, 3))]
    cells = rng.integers(0, ids + 1, ((h + block - 1) // block, (w + block - 1) // block))
    reg = np.kron(cells, np.ones((block, block), np.int64))[:h, :w]
    return np.where(reg == ids, background, reg).astype(np.uint32), ids


@pytest.mark.parametrize("seed", range(6))
def test_the_model_equals_scalar_loops_region_by_region(seed):
    rng = np.random.default_rng(1000 + seed)
    for _ in range(20):   # 120 maps in all
        reg, nreg = random_map(rng)
        got = sm.region_skeleton(reg, nreg)
        skel, when, thick = region_by_region(reg, nreg)
        assert np.array_equal(got["skel"], skel), (reg.tolist(), nreg)
        assert np.array_equal(got["when"], when), (reg.tolist(), nreg)
        assert np.array_equal(got["thick"], thick), (reg.tolist(), nreg)   # the per-region iteration counts
        assert got["iterations"] == int(thick.max()) and got["converged"] == 1
        assert got["kept"] == int(skel.sum()) == int(got["skel_area"].sum())
        assert np.array_equal(got["skeled"], np.where(skel == 1, reg, sm.NONE))


def _box(w, h):
    return sm.region_skeleton(np.zeros((h, w), np.uint32), 1)


def _kept(got):
    ys, xs = np.nonzero(got["skel"])
    return sorted(zip(xs.tolist(), ys.tolist()))


@pytest.mark.parametrize("w,h,kept,iterations", [
    (1, 1, [(0, 0)], 0),
    (1, 50, [(0, y) for y in range(50)], 0),
    (2, 2, [(0, 1)], 1),
    (3, 3, [(1, 1)], 1),
    (4, 4, [(1, 2)], 2),
    (5, 5, [(2, 2)], 2),
    (64, 64, [(31, 32)], 32),
    (257, 257, [(128, 128)], 128),
    (50, 2, [(x, 1) for x in range(0, 49)], 1),
    (50, 3, [(x, 1) for x in range(1, 49)], 1),
    (130, 65, [(x, 32) for x in range(32, 98)], 32),
])
def test_the_literals(w, h, kept, iterations):
    got = _box(w, h)
    assert _kept(got) == sorted(kept)
    assert got["iterations"] == iterations and got["converged"] == 1
    assert got["kept"] == len(kept) == int(got["skel_area"][0]) and got["thick"][0] == iterations


def test_a_two_id_checkerboard_keeps_every_pixel():
    yy, xx = np.mgrid[0:9, 0:11]
    got = sm.region_skeleton(((yy + xx) % 2).astype(np.uint32), 2)
    assert got["skel"].all() and got["iterations"] == 0 and got["converged"] == 1 and not got["when"].any()


@pytest.mark.parametrize("m", [1, 2, 7])
def test_max_iters_cuts_the_unbounded_run(m):
    reg = np.zeros((64, 64), np.uint32)
    full = sm.region_skeleton(reg, 1)
    got = sm.region_skeleton(reg, 1, max_iters=m)
    cut = (full["when"] == 0) | (full["when"] > m)       # alive after m iterations
    assert np.array_equal(got["skel"], cut.astype(np.uint8))
    assert np.array_equal(got["when"], np.where(full["when"] <= m, full["when"], 0))
    assert got["iterations"] == m and got["converged"] == 0 and got["thick"][0] == m


def test_max_iters_past_the_end_converges():
    reg = np.zeros((5, 5), np.uint32)
    assert sm.region_skeleton(reg, 1, max_iters=2)["converged"] == 0    # the second iteration still deleted
    got = sm.region_skeleton(reg, 1, max_iters=3)
    assert got["iterations"] == 2 and got["converged"] == 1
