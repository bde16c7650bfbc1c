"""CPU: the numpy model of the "region distance" block (tests/distance_model.py)
against brute force, against scipy's taxicab transform where scipy imports, and
against hand-worked literals of every rule."""
import numpy as np
import pytest

import distance_model as dm

NONE = dm.NONE


def coord(x, y):
    return x | y << 16


def blocky(rng, h, w, block, ids, background=False):
    cells = rng.integers(0, ids, ((h + block - 1) // block, (w + block - 1) // block))
    reg = np.kron(cells, np.ones((block, block), np.int64))[:h, :w].astype(np.uint32)
    if background:
        reg[rng.random((h, w)) < 0.1] = 1000
    return reg


def random_maps():
    rng = np.random.default_rng(11)
    for i in range(60):
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        yield blocky(rng, h, w, int(rng.choice([1, 2, 3])), int(rng.integers(1, 5)), background=bool(i % 3 == 0))


def test_the_scan_form_equals_brute_force():
    for reg in random_maps():
        for nreg in (int(reg.max()) + 1, 2):   # (2: the higher ids are background)
            assert np.array_equal(dm.scan_distance(reg, nreg), dm.brute_distance(reg, nreg)), (reg, nreg)


def test_the_scan_form_equals_scipy_per_region():
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    maps = list(random_maps())[:20] + [blocky(rng, 70, 90, 16, 4), blocky(rng, 33, 129, 3, 3, background=True)]
    for reg in maps:
        nreg = min(int(reg.max()) + 1, 5)
        assert np.array_equal(dm.scan_distance(reg, nreg), dm.scipy_distance(reg, nreg))


def test_one_and_two_pixel_regions():
    reg = np.array([[9, 0, 9, 1, 1, 9]], np.uint32)
    v = dm.region_values(reg, 2)
    assert v["dist"].tolist() == [[0, 1, 0, 1, 1, 0]]
    assert v["dmax"].tolist() == [1, 1] and v["thresh"].tolist() == [1, 1] and v["count"].tolist() == [1, 2]
    assert v["bbox"].tolist() == [[1, 0, 1, 0], [3, 0, 4, 0]]
    assert v["centre"].tolist() == [coord(1, 0), coord(3, 0)]   # two in a row: the leftmost


def test_two_pixels_in_a_column_take_the_lower():
    reg = np.full((4, 3), 7, np.uint32)
    reg[1:3, 1] = 0
    v = dm.region_values(reg, 1)
    assert v["count"].tolist() == [2] and v["centre"].tolist() == [coord(1, 2)]


def test_a_4x4_square_has_four_maxima_and_the_centroid_is_one():
    reg = np.full((6, 7), 5, np.uint32)
    reg[1:5, 2:6] = 0
    v = dm.region_values(reg, 1)
    assert v["dist"][1:5, 2:6].tolist() == [[1, 1, 1, 1], [1, 2, 2, 1], [1, 2, 2, 1], [1, 1, 1, 1]]
    assert v["dmax"].tolist() == [2] and v["count"].tolist() == [4]
    assert v["centre"].tolist() == [coord(2 + 1, 1 + 1)]   # (1, 1) in region coordinates


def test_a_ring_takes_the_lowest_raster_index_of_a_four_way_tie():
    reg = np.zeros((7, 7), np.uint32)
    reg[2:5, 2:5] = 3   # the hole: background
    v = dm.region_values(reg, 1)
    # the ring is 2 wide: D = 2 only where both the frame and the hole are 2 away, the four inner corners
    assert v["dmax"].tolist() == [2] and v["count"].tolist() == [4]
    assert np.argwhere(v["dist"] == 2).tolist() == [[1, 1], [1, 5], [5, 1], [5, 5]]
    # c = (3, 3) lies in the hole; the four tie at dx^2 + dy^2 = 8
    assert v["centre"].tolist() == [coord(1, 1)]
    cores = dm.region_cores(reg, 1, v["centre"])
    assert cores["kept"] == 49 - 9 and cores["core_area"].tolist() == [40]


def test_the_8_bit_scale_of_a_400_square():
    assert dm.radius_of(400, 400) == 285
    # sqrt(d) / 285 * 255 + 0.5 is 12.994 at d = 195 and 13.026 at d = 196: the bytes of 196 .. 200 are all 13
    assert [dm.scale_byte(d, 285) for d in range(194, 201)] == [12, 12, 13, 13, 13, 13, 13]
    assert dm.thresh_of(200, 400, 400, 1) == dm.thresh_by_walk(200, 400, 400)
    reg = np.zeros((400, 400), np.uint32)
    v = dm.region_values(reg, 1, rule=1)
    assert v["dmax"].tolist() == [200]
    t = int(v["thresh"][0])
    assert t == 196 and t == dm.thresh_by_walk(200, 400, 400) and dm.scale_byte(t, 285) == 13 and dm.scale_byte(t - 1, 285) == 12
    assert v["count"][0] == (400 - 2 * (t - 1)) ** 2
    assert v["centre"].tolist() == [coord(199, 199)]


def test_the_radius_and_the_search_equal_their_reference_forms():
    for bw in list(range(1, 300)) + [1023, 4096, 65535]:
        for bh in (1, 2, 3, 7, bw, bw + 1, 65535):
            assert dm.radius_of(bw, bh) == dm.radius_reference(bw, bh), (bw, bh)
    for side in range(1, 151):
        for bh in (side, 3):
            dmax = (min(side, bh) + 1) // 2
            assert dm.thresh_of(dmax, side, bh, 1) == dm.thresh_by_walk(dmax, side, bh), (side, bh)
            radius = dm.radius_of(side, bh)
            scale = [dm.scale_byte(d, radius) for d in range(1, dmax + 1)]
            assert scale == sorted(scale)


def test_cores_follow_the_connectivity():
    reg = np.full((5, 6), 9, np.uint32)
    reg[0:2, 0:2] = 0
    reg[2:5, 2:5] = 0   # joined to the first blob by a corner only; the larger: it holds the centre
    v = dm.region_values(reg, 1)
    assert v["centre"].tolist() == [coord(3, 3)]
    assert dm.region_cores(reg, 1, v["centre"], 8)["kept"] == 13
    assert dm.region_cores(reg, 1, v["centre"], 4)["kept"] == 9
    assert dm.region_cores(reg, 2, np.array([coord(3, 3), NONE]), 4)["core_area"].tolist() == [9, 0]
