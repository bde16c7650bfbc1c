"""CPU: the model of the region-contour stage (tests/contour_model.py) against
an independent scalar statement of rules 2-4, against the facts the kernels
lean on, and against hand-checked literals.

The scalar statement is OpenCV 3.1's border-following loop for an outer border,
literally, on one region's mask inside a 1-pixel border of zeros: the clockwise
search from 4 for the first neighbour, then ++s until a non-zero neighbour,
stopping when the next point is the start and the current one is the first
neighbour found; (1, 1) is subtracted from every point.  It shares no code with
the model: its own deltas, no neighbour bytes, no table.

The facts (observed on random masks up to 9 x 9, not proven; every map here is
at most 9 x 9, where the length bound was observed -- a 1 x 11 bar has 20 > 19.8
points): `step` is a bijection on the states of a mask; every pixel of a traced
contour has a 4-neighbour that is off; a pixel is visited at most 4 times;
len <= 1.8 x the area of the component traced."""
import numpy as np
import pytest

import contour_model as cm

# OpenCV's CV_INIT_3X3_DELTAS, as (dx, dy): 0 = E, then counter-clockwise on the screen
DELTAS = [(1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1)]


def opencv_outer_border(mask):
    """(points (x, y) in frame coordinates, in the order followed) of the first outer border a
    raster scan of the mask meets; [] for an empty mask."""
    h, w = mask.shape
    img = np.zeros((h + 2, w + 2), np.int64)
    img[1:-1, 1:-1] = mask != 0
    found = np.argwhere(img)
    if len(found) == 0:
        return []
    y0, x0 = found[0]
    i0 = (int(x0), int(y0))
    at = lambda p, s: (p[0] + DELTAS[s][0], p[1] + DELTAS[s][1])  # noqa: E731
    s_end = s = 4
    while True:
        s = (s - 1) & 7
        i1 = at(i0, s)
        if img[i1[1], i1[0]]:
            break
        if s == s_end:
            return [(i0[0] - 1, i0[1] - 1)]   # a single pixel
    i3, points = i0, []
    while True:
        while True:
            s = (s + 1) & 7
            i4 = at(i3, s)
            if img[i4[1], i4[0]]:
                break
        points.append((i3[0] - 1, i3[1] - 1))
        if i4 == i0 and i3 == i1:
            return points
        i3, s = i4, (s + 4) & 7


def scalar_contours(reg, nreg, orientation):
    h, w = reg.shape
    length = np.zeros(nreg, np.uint32)
    points, codes = [], []
    visits = np.zeros((h, w), np.uint8)
    for r in range(nreg):
        pts = opencv_outer_border(reg == r)
        if orientation == 1:
            pts = pts[::-1]
        length[r] = len(pts)
        for i, (x, y) in enumerate(pts):
            nx, ny = pts[(i + 1) % len(pts)]
            points.append(x | y << 16)
            codes.append(8 if len(pts) == 1 else DELTAS.index((nx - x, ny - y)))
            visits[y, x] += 1
    offsets = np.concatenate([[0], np.cumsum(length)]).astype(np.uint32)
    return {"offsets": offsets, "len": length, "points": np.array(points, np.uint32).reshape(-1),
            "codes": np.array(codes, np.uint8).reshape(-1), "visits": visits, "total": len(points)}


KEYS = ("offsets", "len", "points", "codes", "visits")


def same(got, want):
    assert got["total"] == want["total"]
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def random_map(seed):
    """((H, W) map, R): blocks of 1, 2, 3 or 5, ids 0 .. ids - 1 of which some are background (>= R),
    and some ids below R absent."""
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 10)), int(rng.integers(1, 10))
    block = (1, 2, 3, 5)[seed % 4]
    ids = int(rng.integers(1, 5))
    cells = rng.integers(0, ids, ((h + block - 1) // block, (w + block - 1) // block))
    reg = np.kron(cells, np.ones((block, block), np.int64))[:h, :w].astype(np.uint32)
    reg = reg * 2 + 1                                  # ids 1, 3, ..: the even ones are absent
    nreg = 2 * ids + int(rng.integers(0, 3))
    if seed % 3 == 0:                                  # background: ids at and above R, 0xFFFFFFFF among them
        holes = rng.random((h, w)) < 0.2
        reg[holes] = rng.choice(np.array([nreg, nreg + 7, 0xFFFFFFFF], np.uint32), int(holes.sum()))
    if seed % 5 == 0:                                  # the highest id is background
        nreg = max(1, 2 * ids - 1)
    return reg, nreg


SEEDS = range(160)


@pytest.mark.parametrize("orientation", [0, 1])
def test_the_model_is_the_opencv_loop(orientation):
    for seed in SEEDS:
        reg, nreg = random_map(seed)
        try:
            same(cm.region_contours(reg, nreg, orientation), scalar_contours(reg, nreg, orientation))
        except AssertionError as e:
            raise AssertionError("seed %d: %s" % (seed, e)) from None


def component_area(mask, x, y):
    h, w = mask.shape
    seen, todo = {(x, y)}, [(x, y)]
    while todo:
        px, py = todo.pop()
        for dx, dy in DELTAS:
            q = (px + dx, py + dy)
            if 0 <= q[0] < w and 0 <= q[1] < h and mask[q[1], q[0]] and q not in seen:
                seen.add(q)
                todo.append(q)
    return len(seen)


def test_the_observed_facts_hold_on_every_map():
    states = 0
    for seed in SEEDS:
        reg, nreg = random_map(seed)
        h, w = reg.shape
        bits = cm.neighbour_bits(reg, nreg)
        # step is a bijection on the states (p, d) of the map: no two states share a successor
        successors = set()
        for y in range(h):
            for x in range(w):
                for d in range(8):
                    if bits[y, x] >> d & 1:
                        s = cm.NEXT[int(bits[y, x])][d]
                        successors.add((x + cm.DX[s], y + cm.DY[s], (s + 4) & 7))
                        states += 1
        assert len(successors) == sum(bin(int(b)).count("1") for b in bits.reshape(-1)), seed
        got = cm.region_contours(reg, nreg)
        assert got["visits"].max(initial=0) <= 4, seed
        on_contour = got["visits"] > 0
        assert ((bits[on_contour] & 0x55) != 0x55).all(), seed   # one of E, N, W, S is off
        for r in range(nreg):
            if got["len"][r]:
                p0 = int(got["points"][got["offsets"][r]])
                assert 10 * int(got["len"][r]) <= 18 * component_area(reg == r, p0 & 0xFFFF, p0 >> 16), (seed, r)
    assert states > 5000


# ---- hand-checked literals -----------------------------------------------------------
def contour(mask, orientation=0):
    """([(x, y)], [code], visits) of the one region of a 0/1 mask (0: the region)."""
    got = cm.region_contours(np.where(np.asarray(mask) != 0, 0, 9).astype(np.uint32), 1, orientation)
    assert got["total"] == got["len"][0] == got["offsets"][1] and got["offsets"][0] == 0
    return [(int(p) & 0xFFFF, int(p) >> 16) for p in got["points"]], got["codes"].tolist(), got["visits"]


def test_a_single_pixel():
    mask = np.zeros((3, 4), int)
    mask[1, 2] = 1
    pts, codes, visits = contour(mask)
    assert pts == [(2, 1)] and codes == [8] and visits.sum() == 1 and visits[1, 2] == 1
    assert contour(mask, 1)[:2] == ([(2, 1)], [8])


@pytest.mark.parametrize("n", [2, 3, 7])
def test_a_bar(n):
    pts, codes, visits = contour(np.ones((1, n), int))
    # out along the bar and back: E n - 1 times, then W n - 1 times
    assert pts == [(x, 0) for x in range(n)] + [(x, 0) for x in range(n - 2, 0, -1)] and len(pts) == 2 * n - 2
    assert codes == [0] * (n - 1) + [4] * (n - 1)
    assert visits[0].tolist() == [1] + [2] * (n - 2) + [1]
    pts, codes, _ = contour(np.ones((n, 1), int))
    assert pts == [(0, y) for y in range(n)] + [(0, y) for y in range(n - 2, 0, -1)] and len(pts) == 2 * n - 2
    assert codes == [6] * (n - 1) + [2] * (n - 1)


def test_the_4x4_square():
    pts, codes, visits = contour(np.ones((4, 4), int))
    assert pts == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 3), (3, 3), (3, 2), (3, 1), (3, 0), (2, 0), (1, 0)]
    assert codes == [6, 6, 6, 0, 0, 0, 2, 2, 2, 4, 4, 4]          # down, right, up, left: counter-clockwise, y down
    assert visits.sum() == 12 and visits[1:3, 1:3].sum() == 0
    pts, codes, _ = contour(np.ones((4, 4), int), 1)
    assert len(pts) == 12 and pts[0] == (1, 0) and pts[-1] == (0, 0)
    assert pts == [(1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3), (2, 3), (1, 3), (0, 3), (0, 2), (0, 1), (0, 0)]
    assert codes == [0, 0, 6, 6, 6, 4, 4, 4, 2, 2, 2, 0]          # clockwise; the last one closes the list


# The arms of an upright plus touch by their corners, and border following on 8-neighbours turns from
# one arm into the next over that diagonal: under rules 3 and 4 its centre is never visited (traced by
# hand below).  The cross whose centre IS passed four times is the diagonal one.
def test_an_upright_plus_sign():
    mask = np.zeros((5, 5), int)
    mask[2, :] = mask[:, 2] = 1
    pts, codes, visits = contour(mask)
    assert pts == [(2, 0), (2, 1), (1, 2), (0, 2), (1, 2), (2, 3), (2, 4), (2, 3), (3, 2), (4, 2), (3, 2), (2, 1)]
    assert codes == [6, 5, 4, 0, 7, 6, 2, 1, 0, 4, 3, 2]
    assert visits[2, 2] == 0 and visits[1, 2] == visits[2, 1] == visits[2, 3] == visits[3, 2] == 2


def test_a_diagonal_cross_passes_its_centre_four_times():
    mask = np.zeros((3, 3), int)
    mask[0, 0] = mask[0, 2] = mask[1, 1] = mask[2, 0] = mask[2, 2] = 1
    pts, codes, visits = contour(mask)
    assert pts == [(0, 0), (1, 1), (0, 2), (1, 1), (2, 2), (1, 1), (2, 0), (1, 1)]
    assert codes == [7, 5, 1, 7, 3, 1, 5, 3]
    assert visits[1, 1] == 4 and visits.sum() == 8


def test_a_ring_gives_its_outer_border_only():
    mask = np.ones((7, 7), int)
    mask[2:5, 2:5] = 0            # two pixels thick
    pts, _, visits = contour(mask)
    assert len(pts) == 24 and visits[1:6, 1:6].sum() == 0 and (visits[0] == 1).all() and (visits[:, 6] == 1).all()
    mask = np.ones((5, 5), int)
    mask[1:4, 1:4] = 0            # one pixel thick: the hole's border is the same pixels, and is not followed
    pts, _, visits = contour(mask)
    assert len(pts) == 16 and visits.sum() == 16 and visits.max() == 1


def test_two_diagonal_pixels():
    pts, codes, _ = contour(np.eye(2, dtype=int))
    assert pts == [(0, 0), (1, 1)] and codes == [7, 3]
    pts, codes, _ = contour(np.eye(2, dtype=int)[::-1])
    assert pts == [(1, 0), (0, 1)] and codes == [5, 1]


def test_only_the_component_of_the_first_pixel_is_traced():
    reg = np.full((4, 9), 5, np.uint32)
    reg[0, 0:2] = 0
    reg[2:4, 4:8] = 0             # a second, larger component of id 0
    got = cm.region_contours(reg, 3)
    assert got["len"].tolist() == [2, 0, 0] and got["offsets"].tolist() == [0, 2, 2, 2]
    assert got["points"].tolist() == [0, 1] and got["visits"][2:].sum() == 0
