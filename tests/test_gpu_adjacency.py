"""GPU: the region adjacency graph of a region map (include/dq_hip.h, "region
adjacency graph").

The reference is adjacency_model of adjacency_model.py, which never uses the
code under test.  Equality is exact everywhere: array_equal on every array, and
the edge count E.  For regions = arange(w * h) the model gives E = 2wh - w - h
(4-connectivity) and 4wh - 3w - 3h + 2 (8) with every border 1; those closed
forms are asserted too.  The maps are adjacency_map of region_inputs.py.

The pixel passes work on chunks of 1024 pixels and a wave holds 64 consecutive
pixels; the shapes are the smallest at which each mechanism can fail."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import dq_fixtures as fx
from adjacency_model import adjacency_model
from region_dev import same, to_dev, to_host
from region_inputs import adjacency_base, frame

pytestmark = pytest.mark.gpu

GUARD_WORD = 0xA5A5A5A5
PER = {"edges": 2, "border": 1, "contact": 2, "step": 2}   # 4-byte words per edge


@functools.lru_cache(maxsize=None)
def _reference(name, w, h, connectivity):
    """The model of a map, once (with the steps of frame and, where the ids allow, the degree)."""
    reg = adjacency_base(name, w, h)
    nreg = int(reg.max()) + 1
    return adjacency_model(reg, connectivity, frame(w, h), nreg if nreg <= 1 << 20 else None)


def _unsigned(g):
    return {k: to_host(v, np.uint64 if k == "step" else np.uint32) for k, v in g.items()}


def _run(gpu, reg2d, connectivity, cap=0, pixels=None, num_regions=0, stream=None):
    """region_adjacency_device on fresh tensors -> (E, graph as unsigned numpy)."""
    import torch
    h, w = reg2d.shape
    t_reg = to_dev(reg2d.reshape(-1))
    t_px = to_dev(pixels) if pixels is not None else None
    if stream is not None:   # (the tensors above were filled on the current stream)
        stream.wait_stream(torch.cuda.current_stream())
    e, g = gpu.region_adjacency_device(t_reg, w, h, connectivity=connectivity, edge_capacity=cap, t_pixels=t_px,
                                       num_regions=num_regions, stream=stream)
    return e, _unsigned(g)


def _check(gpu, name, w, h, connectivity):
    """Everything at capacity E (1 where E is 0: no array may be written then)."""
    want = _reference(name, w, h, connectivity)
    nreg = len(want["degree"]) if "degree" in want else 0
    e, g = _run(gpu, adjacency_base(name, w, h), connectivity, cap=max(want["E"], 1), pixels=frame(w, h),
                num_regions=nreg)
    assert e == want["E"]
    assert sorted(g) == sorted(k for k in want if k != "E")
    same(g, want, [k for k in want if k != "E"])
    assert (g["edges"][:, 0] < g["edges"][:, 1]).all() and (g["contact"][:, 0] < g["contact"][:, 1]).all()
    return want


# ---------------------------------------------------------------------------
#            (w, h)
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (5, 3),
          (63, 3), (64, 3), (65, 3),     # a run across a wave boundary, a row start inside a wave
          (67, 31),                      # 2077 pixels: two chunks and a tail, every row start misaligned
          (1024, 2), (1025, 2),          # down neighbours exactly one chunk away, and one more
          (32, 33)]                      # a chunk boundary at a row start


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_every_pixel_its_own_id(gpu, shape, connectivity):
    """arange: all edges distinct, every border 1 (table growth and probing)."""
    w, h = shape
    want = _check(gpu, "arange", w, h, connectivity)
    closed = 2 * w * h - w - h if connectivity == 4 else 4 * w * h - 3 * w - 3 * h + 2
    assert want["E"] == closed and (want["border"] == 1).all()
    assert int(want["degree"].sum()) == 2 * closed


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_three_ids(gpu, shape, connectivity):
    """Three ids of noise: at most three edges, runs of every length."""
    _check(gpu, "noise3", shape[0], shape[1], connectivity)


MAPS = [("halves", 256, 40), ("quadrants", 256, 40),     # few edges, hundreds of contacts from many workgroups
        ("vstripes", 200, 7), ("k4", 66, 34), ("checker", 67, 31), ("constant", 67, 31),
        ("noise7", 130, 70), ("noise50000", 130, 70),
        ("reversed", 67, 31), ("permutation", 67, 31), ("huge_ids", 67, 31)]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", MAPS, ids=lambda c: c[0])
def test_maps(gpu, case, connectivity):
    name, w, h = case
    want = _check(gpu, name, w, h, connectivity)
    E = want["E"]
    if name == "halves":
        assert E == 1 and want["border"][0] == (h if connectivity == 4 else 3 * h - 2)
    if name == "quadrants":
        assert E == (4 if connectivity == 4 else 6)
    if name == "vstripes":
        assert E == 1 and want["contact"].tolist() == [[0, 1]]
    if name == "k4":
        assert E == (4 if connectivity == 4 else 6)
    if name == "checker":       # the diagonals join equal ids
        assert E == 1 and want["border"][0] == 2 * w * h - w - h
    if name == "constant":
        assert E == 0
    if name == "reversed":
        assert want["edges"][0].tolist() == [w * h - 2, w * h - 1]
    if name == "huge_ids":
        assert "degree" not in want and int(want["edges"].max()) == 0xFFFFFFFE


# ---------------------------------------------------------------------------
def _raw(gpu, reg2d, connectivity, cap, pixels=None, num_regions=0, with_arrays=True):
    """The C entry point on guard-filled arrays 8 entries longer than the
    capacity -> (E, {name: all words as uint32}, degree or None)."""
    import torch
    h, w = reg2d.shape
    t_reg = to_dev(reg2d.reshape(-1))
    t_px = to_dev(pixels) if pixels is not None else None
    guard = int(np.full(1, GUARD_WORD, np.uint32).view(np.int32)[0])
    bufs = {}
    if with_arrays:
        bufs = {k: torch.full(((cap + 8) * p,), guard, dtype=torch.int32, device="cuda:0") for k, p in PER.items()
                if k != "step" or pixels is not None}
    t_deg = torch.full((num_regions + 8,), guard, dtype=torch.int32, device="cuda:0") if num_regions else None
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    e = gpu.lib().dq_hip_region_adjacency_dev(0, ptr(t_reg), w, h, connectivity, cap, ptr(bufs.get("edges")),
                                              ptr(bufs.get("border")), ptr(bufs.get("contact")), ptr(t_px),
                                              ptr(bufs.get("step")), num_regions, ptr(t_deg), None)
    return e, {k: to_host(v, np.uint32) for k, v in bufs.items()}, None if t_deg is None else to_host(t_deg, np.uint32)


def _heads(bufs, m):
    out = {}
    for k, words in bufs.items():
        head = words[:m * PER[k]]
        out[k] = head.view(np.uint64) if k == "step" else head.reshape(m, 2) if PER[k] == 2 else head
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
def test_one_pixel_has_no_edge_and_nothing_is_written(gpu, connectivity):
    e, bufs, deg = _raw(gpu, np.full((1, 1), 3, np.uint32), connectivity, cap=4, pixels=np.zeros(1, np.uint32),
                        num_regions=5)
    assert e == 0
    for k, words in bufs.items():
        assert (words == GUARD_WORD).all(), k
    assert (deg[:5] == 0).all() and (deg[5:] == GUARD_WORD).all()


@pytest.mark.parametrize("which", ["zero", "one", "E-1", "E", "E+5"])
def test_edge_capacity(gpu, which):
    """The return value and the degree do not change with the capacity, the
    first min(E, cap) entries are the model's, and nothing behind them is
    written (guard words)."""
    w, h, connectivity = 67, 31, 8
    want = _reference("noise7", w, h, connectivity)
    E, nreg = want["E"], len(want["degree"])
    assert E == 21   # K7: every pair of the seven ids touches
    cap = {"zero": 0, "one": 1, "E-1": E - 1, "E": E, "E+5": E + 5}[which]
    m = min(E, cap)
    e, bufs, deg = _raw(gpu, adjacency_base("noise7", w, h), connectivity, cap, pixels=frame(w, h), num_regions=nreg)
    assert e == E
    assert np.array_equal(deg[:nreg], want["degree"]) and (deg[nreg:] == GUARD_WORD).all()
    for k, words in bufs.items():
        assert (words[m * PER[k]:] == GUARD_WORD).all(), k
    got = _heads(bufs, m)
    for k in ("edges", "border", "contact", "step"):
        assert np.array_equal(got[k], want[k][:m]), k


def test_count_only_call_then_the_full_call(gpu):
    w, h, connectivity = 130, 70, 8
    want = _reference("noise50000", w, h, connectivity)
    e0, bufs, _ = _raw(gpu, adjacency_base("noise50000", w, h), connectivity, cap=0, with_arrays=False)
    assert e0 == want["E"] and bufs == {}
    e1, g = _run(gpu, adjacency_base("noise50000", w, h), connectivity, cap=e0)
    assert e1 == e0 and sorted(g) == ["border", "contact", "edges"]
    same(g, want, ["edges", "border", "contact"])


def test_single_arrays(gpu):
    """Each edge array alone (the others NULL)."""
    import torch
    w, h, connectivity = 65, 3, 8
    want = _reference("noise3", w, h, connectivity)
    E = want["E"]
    t_reg, t_px = to_dev(adjacency_base("noise3", w, h).reshape(-1)), to_dev(frame(w, h))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for k, p in PER.items():
        t = torch.zeros(E * p, dtype=torch.int32, device="cuda:0")
        a = {name: (ptr(t) if name == k else None) for name in PER}
        e = gpu.lib().dq_hip_region_adjacency_dev(0, ptr(t_reg), w, h, connectivity, E, a["edges"], a["border"],
                                                  a["contact"], ptr(t_px) if k == "step" else None, a["step"], 0,
                                                  None, None)
        assert e == E
        assert np.array_equal(_heads({k: to_host(t, np.uint32)}, E)[k], want[k]), k


def test_top_bytes_of_the_frame_are_ignored(gpu):
    w, h, connectivity = 67, 31, 8
    want = _reference("noise7", w, h, connectivity)
    top = (fx.xorshift(w * h, seed=fx.SEED + 3) << np.uint32(24)).astype(np.uint32)
    assert len(np.unique(top >> 24)) > 100
    px = (frame(w, h) | top).astype(np.uint32)
    e, g = _run(gpu, adjacency_base("noise7", w, h), connectivity, cap=want["E"], pixels=px)
    assert e == want["E"] and np.array_equal(g["step"], want["step"])
    assert int(want["step"].sum()) > 0 and (want["step"] <= 765 * want["border"].astype(np.uint64)).all()


def test_same_input_twice_gives_identical_bytes(gpu):
    w, h = 130, 70
    E = _reference("noise50000", w, h, 8)["E"]
    a = _run(gpu, adjacency_base("noise50000", w, h), 8, cap=E, pixels=frame(w, h), num_regions=50000)
    b = _run(gpu, adjacency_base("noise50000", w, h), 8, cap=E, pixels=frame(w, h), num_regions=50000)
    assert a[0] == b[0] == E
    for k in a[1]:
        assert a[1][k].tobytes() == b[1][k].tobytes(), k


def test_two_streams_at_once(gpu):
    """Two calls with different maps on two streams from two host threads
    (scratch is owned by each call) both come out right."""
    import torch
    cases = [("noise7", 130, 70, 8), ("permutation", 67, 31, 4)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in cases]
    results = [None, None]
    wants = [_reference(*c) for c in cases]   # (the models, before the threads start)
    torch.cuda.synchronize()

    def work(i):
        name, w, h, connectivity = cases[i]
        results[i] = _run(gpu, adjacency_base(name, w, h), connectivity, cap=wants[i]["E"], pixels=frame(w, h),
                          num_regions=len(wants[i]["degree"]), stream=streams[i])

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for want, (e, g) in zip(wants, results):
        assert e == want["E"]
        same(g, want, ["edges", "border", "contact", "step", "degree"])


def test_host_form_equals_the_device_form(gpu):
    w, h = 67, 31
    for name, connectivity in (("noise7", 8), ("permutation", 4)):
        want = _reference(name, w, h, connectivity)
        reg = adjacency_base(name, w, h)
        g = gpu.region_adjacency(reg, connectivity=connectivity, pixels=frame(w, h))
        e, d = _run(gpu, reg, connectivity, cap=want["E"], pixels=frame(w, h), num_regions=int(reg.max()) + 1)
        assert e == want["E"] and sorted(g) == sorted(d) == ["border", "contact", "degree", "edges", "step"]
        same(g, d, sorted(g))
        same(g, want, sorted(g))
    g = gpu.region_adjacency(adjacency_base("constant", w, h), num_regions=9)    # no edge at all
    assert g["edges"].shape == (0, 2) and g["border"].shape == (0,) and "step" not in g
    assert g["degree"].tolist() == [0] * 9


def test_pipeline_labels_to_regions_to_graph_on_the_device(gpu):
    """A labelled pattern -> label_regions_device -> region_adjacency_device on
    the same device buffers.  The neighbour sets built from the edges equal
    the sets a literal 8-neighbour scan of the region map gives (the
    reference's parseSuperpixelEdges rule)."""
    import torch
    w, h = 45, 37
    ys, xs = np.mgrid[0:h, 0:w]
    lab = (((xs // 6) + (ys // 5)) % 3 + 3 * ((xs - w // 2) ** 2 + (ys - h // 2) ** 2 < 90)).astype(np.uint8)
    t_lab = torch.from_numpy(lab.reshape(-1).copy()).to("cuda:0")
    t_reg = torch.empty(w * h, dtype=torch.int32, device="cuda:0")
    t_px = to_dev(frame(w, h))
    R, _ = gpu.label_regions_device(t_lab, w, h, t_reg, connectivity=8)
    E, _ = gpu.region_adjacency_device(t_reg, w, h, connectivity=8)
    e, g = gpu.region_adjacency_device(t_reg, w, h, connectivity=8, edge_capacity=E, t_pixels=t_px, num_regions=R)
    assert e == E and E > 20
    g = _unsigned(g)
    reg = to_host(t_reg, np.uint32).reshape(h, w)
    sets = [set() for _ in range(R)]
    for y in range(h):
        for x in range(w):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and reg[yy, xx] != reg[y, x]:
                        sets[reg[y, x]].add(int(reg[yy, xx]))
    got = [set() for _ in range(R)]
    for a, b in g["edges"].tolist():
        assert b not in got[a]
        got[a].add(b)
        got[b].add(a)
    assert got == sets
    assert g["degree"].tolist() == [len(s) for s in sets]
    same(g, adjacency_model(reg, 8, frame(w, h), R), ["edges", "border", "contact", "step", "degree"])
