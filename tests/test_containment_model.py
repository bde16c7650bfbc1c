"""CPU: the host model of the containment tree (tests/containment_model.py)
gives the literals Test/ContainmentTest.mm asserts (ids = tag - 1, typed out
as the XCTest states them), and on nested maps its parents and roots equal a
sequential restatement of the reference's depth-first claim.  The GPU tests
compare the library with this model; this file pins the model itself."""
import numpy as np
import pytest

import containment_model as cm


def _run(reg, connectivity=4, area=None):
    R = int(reg.max()) + 1
    area = cm.areas_of(reg, R) if area is None else area
    return cm.model(reg, area, cm.edges_of(reg, connectivity), R), R


def _children(m, p):
    return m["children"][m["child_offsets"][p]:m["child_offsets"][p + 1]].tolist()


def test_xctest_one_pixel():
    m, R = _run(cm.XCTEST_MAPS["1x1"])
    assert m["roots"].tolist() == [0]
    assert _children(m, 0) == [] and m["child_offsets"].tolist() == [0, 0]
    assert m["order"].tolist() == [0] and (m["levels"], m["reached"], m["nroots"]) == (1, 1, 1)


def test_xctest_two_rows():
    m, _ = _run(cm.XCTEST_MAPS["2x2_rows"])
    assert m["roots"].tolist() == [0, 1]
    assert _children(m, 0) == [] and _children(m, 1) == []


def test_xctest_corner():
    m, _ = _run(cm.XCTEST_MAPS["2x2_corner"])
    assert m["roots"].tolist() == [1, 0]      # the three-pixel tag first
    assert _children(m, 0) == [] and _children(m, 1) == []


def test_xctest_two_bars_in_a_frame():
    m, _ = _run(cm.XCTEST_MAPS["4x4_bars"])
    assert m["roots"].tolist() == [0]
    assert _children(m, 0) == [1, 2]
    assert _children(m, 1) == [] and _children(m, 2) == []
    assert m["parent"].tolist() == [cm.NONE, 0, 0] and m["depth"].tolist() == [0, 1, 1]
    assert m["subtree"].tolist() == [3, 1, 1] and m["enclosed"].tolist() == [16, 2, 2]
    assert m["order"].tolist() == [1, 2, 0] and m["pos"].tolist() == [2, 0, 1]


NESTED = {
    "rings_9": cm.rings(9),
    "rings_12": cm.rings(12),
    "islands_10": cm.islands(10),
    "islands_14_mixed": cm.islands(14, two_pixel_every=3),
    "islands_in_islands": cm.islands_in_islands(),
    "4x4_bars": cm.XCTEST_MAPS["4x4_bars"],
}


@pytest.mark.parametrize("name", sorted(NESTED))
@pytest.mark.parametrize("connectivity", [4, 8])
def test_nested_maps_agree_with_the_reference_rule(name, connectivity):
    reg = NESTED[name]
    R = int(reg.max()) + 1
    area, edges = cm.areas_of(reg, R), cm.edges_of(reg, connectivity)
    assert cm.is_nested(reg, area, edges, R)
    m = cm.model(reg, area, edges, R)
    parent, roots = cm.reference_tree(reg, area, edges, R)
    assert np.array_equal(m["parent"], parent)
    assert np.array_equal(m["roots"], roots)


def test_the_closed_form_of_pos_is_the_post_order():
    for reg in NESTED.values():
        m, R = _run(reg)
        block = np.zeros(R, np.int64)
        at = 0
        for r in m["roots"]:
            block[r] = at
            at += m["subtree"][r]
        for r in sorted(range(R), key=lambda r: m["depth"][r]):
            at = block[r]
            for c in _children(m, r):
                block[c] = at
                at += m["subtree"][c]
        assert np.array_equal(block + m["subtree"] - 1, m["pos"].astype(np.int64))
        assert np.array_equal(m["order"][m["pos"]], np.arange(R))


def test_a_map_that_is_not_nested_differs_and_why():
    """Kept as documentation: 4 touches 2 (depth 1) and 3 (depth 2, inside the
    larger 1).  The reference's walk goes below 1 first, where 3 claims 4;
    breadth-first, 4 is at depth 2 under 2."""
    reg = cm.NOT_NESTED
    R = 5
    area, edges = cm.areas_of(reg, R), cm.edges_of(reg, 4)
    assert not cm.is_nested(reg, area, edges, R)
    m = cm.model(reg, area, edges, R)
    parent, roots = cm.reference_tree(reg, area, edges, R)
    assert m["parent"].tolist() == [cm.NONE, 0, 0, 1, 2]
    assert parent.tolist() == [cm.NONE, 0, 0, 1, 3]
    assert np.array_equal(m["roots"], roots)


def test_size_order_and_orphans():
    order, rank = cm.size_order([3, 7, 3, 1, 7])
    assert order.tolist() == [1, 4, 0, 2, 3] and rank.tolist() == [2, 0, 3, 4, 1]
    reg = cm.XCTEST_MAPS["4x4_bars"]
    m = cm.model(reg, cm.areas_of(reg, 5), cm.edges_of(reg)[:1], 5)   # the edge (0, 2) dropped, ids 3 and 4 absent
    assert m["depth"].tolist() == [0, 1, cm.NONE, cm.NONE, cm.NONE]
    assert m["reached"] == 2 and m["order"].tolist() == [1, 0]
    assert m["subtree"].tolist() == [2, 1, 0, 0, 0] and m["pos"].tolist() == [1, 0, cm.NONE, cm.NONE, cm.NONE]
    assert m["child_offsets"].tolist() == [0, 1, 1, 1, 1, 1]
