"""GPU: the containment tree of a region map (include/dq_hip.h, "containment
tree") and the size order alone.

The reference is the host model of tests/containment_model.py, written
against the definition and using none of the code under test
(test_containment_model.py pins it to the reference's XCTest literals).
Equality is exact everywhere: array_equal on every output array, == on nroots,
levels and reached.

Shapes are the smallest at which each mechanism can go wrong: chains of depth
17 and 33 (the level loop and its read-back end, subtree / enclosed / pos along
a path), 4 096 children of one parent (a row across the 1 024-value scan
chunks and the sort's tiles; equal areas show stability), noise maps where
every non-root has several candidates of equal area (the id tie-break) or
random areas (the area key), strips of up to 65 535 roots with areas past
2^16 (a three-digit key), orphans, and every output pointer NULL in turn."""
import ctypes
import functools

import numpy as np
import pytest

import containment_model as cm
from region_dev import to_dev

pytestmark = pytest.mark.gpu

NONE = cm.NONE
ARRAYS = cm.ARRAYS
GUARD = 0x5A5A5A5A


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a.view(np.uint32)


def run(gpu, reg, area, edges, nregions, outputs=None, stream=None):
    h, w = reg.shape
    t_edges = to_dev(np.asarray(edges, np.uint32).reshape(-1, 2)) if len(edges) else None
    nroots, levels, reached, out = gpu.region_containment_device(
        to_dev(reg.astype(np.uint32)), w, h, nregions, to_dev(np.asarray(area, np.uint32)), t_edges, outputs=outputs,
        stream=stream)
    got = {k: _host(v) for k, v in out.items()}
    got.update(nroots=nroots, levels=levels, reached=reached)
    return got


def same(got, want, names=ARRAYS):
    for k in ("nroots", "levels", "reached"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in names:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


@functools.lru_cache(maxsize=None)
def case(name):
    """(map, area, edges, R, the model's answer), computed once per case."""
    kind, *args = name.split(":")
    area = None
    if kind == "xctest":
        reg, conn = cm.XCTEST_MAPS[args[0]], 4
    elif kind == "rings":
        reg, conn = cm.rings(int(args[0])), 4
    elif kind == "islands":
        reg, conn = cm.islands(130, two_pixel_every=int(args[0])), 8
    elif kind == "noise":
        reg, conn = cm.noise(int(args[0])), int(args[1])
        if args[2] == "random":
            area = np.random.default_rng(int(args[0])).integers(1, 1 << 20, reg.size).astype(np.uint32)
    elif kind == "strip":
        w, h = int(args[0]), int(args[1])
        reg, conn = np.tile(np.arange(w, dtype=np.uint32), (h, 1)), 4
        area = np.random.default_rng(w + h).integers(1, 200000, w).astype(np.uint32)   # 1 .. above 2^16 (18 bits)
        area[:3] = (1, 70000, 70000)
    R = int(reg.max()) + 1
    area = cm.areas_of(reg, R) if area is None else area
    edges = cm.edges_of(reg, conn)
    return reg, area, edges, R, cm.model(reg, area, edges, R)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cm.XCTEST_MAPS))
def test_xctest_maps_through_both_forms(gpu, name):
    reg, area, edges, R, want = case("xctest:" + name)
    same(run(gpu, reg, area, edges, R), want)
    host = gpu.region_containment(reg, area, edges if len(edges) else None)
    same(dict(host, nroots=len(host["roots"])), want)
    literal = {"1x1": [0], "2x2_rows": [0, 1], "2x2_corner": [1, 0], "4x4_bars": [0]}[name]
    assert host["roots"].tolist() == literal
    if name == "4x4_bars":
        assert host["children"].tolist() == [1, 2] and host["child_offsets"].tolist() == [0, 2, 2, 2]


@pytest.mark.parametrize("side,depth", [(33, 17), (66, 33)])
def test_rings_are_a_chain(gpu, side, depth):
    reg, area, edges, R, want = case("rings:%d" % side)
    assert want["levels"] == depth and R == depth
    got = run(gpu, reg, area, edges, R)
    same(got, want)
    assert got["order"].tolist() == list(range(depth - 1, -1, -1))        # inside-out
    assert got["subtree"].tolist() == list(range(depth, 0, -1))
    assert int(got["enclosed"][0]) == side * side


@pytest.mark.parametrize("mixed", [0, 3])
def test_islands_are_one_long_row_of_children(gpu, mixed):
    reg, area, edges, R, want = case("islands:%d" % mixed)
    got = run(gpu, reg, area, edges, R)
    same(got, want)
    assert got["child_offsets"][1] == R - 1 and got["nroots"] == 1
    if mixed == 0:
        assert R == 4097 and got["children"].tolist() == list(range(1, R))   # equal areas: the id order survives
    else:
        assert R > 3000 and set(area[1:].tolist()) == {1, 2}
        assert (np.diff(area[got["children"]].astype(np.int64)) <= 0).all()


@pytest.mark.parametrize("side,conn,areas", [(64, 4, "own"), (64, 8, "own"), (96, 4, "own"), (96, 8, "own"),
                                             (64, 8, "random"), (96, 4, "random")])
def test_noise_ties_and_area_keys(gpu, side, conn, areas):
    reg, area, edges, R, want = case("noise:%d:%d:%s" % (side, conn, areas))
    assert want["levels"] == side // 2 and R == side * side
    same(run(gpu, reg, area, edges, R), want)


@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("w", [255, 256, 257, 1023, 1025, 65535])
def test_strips_every_region_a_root(gpu, w, h):
    reg, area, edges, R, want = case("strip:%d:%d" % (w, h))
    assert want["nroots"] == R == w and int(area.max()) > 65536
    got = run(gpu, reg, area, edges, R)
    same(got, want)
    assert np.array_equal(got["order"], got["roots"])


SIZE_R = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65537]


def _size_patterns(R):
    rng = np.random.default_rng(R)
    yield "equal", np.full(R, 7, np.uint32)
    yield "increasing", np.arange(1, R + 1, dtype=np.uint32)
    yield "decreasing", np.arange(R, 0, -1).astype(np.uint32)
    for bits in (8, 16, 24, 32):
        yield "random_2^%d" % bits, rng.integers(0, 1 << bits, R, dtype=np.uint64).astype(np.uint32)
    yield "two_values", np.where(rng.integers(0, 2, R) == 1, 70000, 3).astype(np.uint32)


@pytest.mark.parametrize("R", SIZE_R)
def test_regions_by_size_alone(gpu, R):
    for name, area in _size_patterns(R):
        want_order, want_rank = cm.size_order(area)
        order, rank = gpu.regions_by_size_device(to_dev(area))
        assert np.array_equal(_host(order), want_order), (name, R)
        assert np.array_equal(_host(rank), want_rank), (name, R)
    order, none = gpu.regions_by_size_device(to_dev(area), want_rank=False)
    assert none is None and np.array_equal(_host(order), want_order)
    none, rank = gpu.regions_by_size_device(to_dev(area), want_order=False)
    assert none is None and np.array_equal(_host(rank), want_rank)


# ---------------------------------------------------------------------------
def _label_map(w, h, nlabels, seed):
    """Blocky random labels with some pixel noise: regions nest a few levels deep."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, nlabels, ((h + 7) // 8, (w + 7) // 8))
    lab = np.kron(coarse, np.ones((8, 8), np.int64))[:h, :w]
    flip = rng.random((h, w)) < 0.06
    lab[flip] = rng.integers(0, nlabels, int(flip.sum()))
    return lab.astype(np.uint8)


@pytest.mark.parametrize("w,h", [(48, 40), (200, 130)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_label_maps_through_the_device_pipeline(gpu, w, h, seed):
    import torch
    nlabels = 2 + (seed * 7 + w) % 5          # 2 .. 6
    conn = 4 if seed % 2 else 8
    t_lab = to_dev(_label_map(w, h, nlabels, seed))
    t_reg = torch.empty(w * h, dtype=torch.int32, device="cuda:0")
    R, stats = gpu.label_regions_device(t_lab, w, h, t_reg, connectivity=conn, stats_capacity=w * h)
    E, _ = gpu.region_adjacency_device(t_reg, w, h, connectivity=conn)
    E2, graph = gpu.region_adjacency_device(t_reg, w, h, connectivity=conn, edge_capacity=E)
    assert E2 == E and E > 0
    reg, area, edges = _host(t_reg).reshape(h, w), _host(stats["area"]), _host(graph["edges"])
    want = cm.model(reg, area, edges, R)
    assert want["levels"] >= 2 and want["reached"] == R
    call = lambda e: gpu.region_containment_device(t_reg, w, h, R, stats["area"], e)  # noqa: E731
    nroots, levels, reached, out = call(graph["edges"])
    got = dict({k: _host(v) for k, v in out.items()}, nroots=nroots, levels=levels, reached=reached)
    same(got, want)
    # the same edges shuffled, a third of them twice, pairs swapped: identical outputs
    rng = np.random.default_rng(seed)
    mixed = np.concatenate([edges, edges[rng.random(E) < 1 / 3]])
    mixed = mixed[rng.permutation(len(mixed))]
    swap = rng.random(len(mixed)) < 0.5
    mixed[swap] = mixed[swap][:, ::-1]
    for e in (to_dev(mixed), graph["edges"]):   # (and the call repeated)
        nroots2, levels2, reached2, out2 = call(e)
        assert (nroots2, levels2, reached2) == (nroots, levels, reached)
        for k in ARRAYS:
            assert torch.equal(out[k], out2[k]), k


# ---------------------------------------------------------------------------
def _raw(gpu, reg, area, edges, R, stream=None):
    """The C entry with guard-filled outputs of R (+ 1) entries: what it leaves alone shows."""
    import torch
    h, w = reg.shape
    t = {k: torch.full((R + (k == "child_offsets"),), GUARD, dtype=torch.int64 if k == "enclosed" else torch.int32,
                       device="cuda:0") for k in ARRAYS}
    t_reg, t_area, t_edges = to_dev(reg.astype(np.uint32)), to_dev(area), to_dev(np.asarray(edges, np.uint32))
    levels, reached = ctypes.c_uint32(0), ctypes.c_uint32(0)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    nroots = gpu.lib().dq_hip_region_containment_dev(0, p(t_reg), w, h, R, p(t_area), len(edges), p(t_edges),
                                                     *[p(t[k]) for k in ARRAYS], ctypes.byref(levels),
                                                     ctypes.byref(reached), stream)
    got = {k: _host(v) for k, v in t.items()}
    got.update(nroots=int(nroots), levels=levels.value, reached=reached.value)
    return got


def test_orphans_and_nothing_written_behind_the_entries_in_use(gpu):
    reg = cm.islands_in_islands()
    top = int(reg.max())
    R = top + 4                                     # three ids the map does not use
    area = cm.areas_of(reg, R)
    area[top + 1:] = (5, 0, 9)                      # (an absent id may still carry an area)
    edges = cm.edges_of(reg, 4)
    cut = 3                                         # the 3 x 3 inside the first 5 x 5: its edges removed,
    edges = edges[(edges != cut).all(axis=1)]       # so it and the pixel inside it are orphans too
    want = cm.model(reg, area, edges, R)
    assert want["reached"] == R - 5 and want["depth"][cut] == NONE and want["depth"][cut + 1] == NONE
    got = _raw(gpu, reg, area, edges, R)
    nroots, reached = want["nroots"], want["reached"]
    for k, used in (("roots", nroots), ("children", reached - nroots), ("order", reached)):
        assert (got[k][used:] == GUARD).all(), k
        got[k] = got[k][:used]
    same(got, want)
    orphan = want["depth"] == NONE
    assert orphan.sum() == 5
    for k in ("depth", "parent", "pos"):
        assert (got[k][orphan] == NONE).all()
    assert (got["subtree"][orphan] == 0).all() and (got["enclosed"][orphan] == 0).all()
    assert not np.isin(np.flatnonzero(orphan), got["order"]).any()


def test_no_edges_on_a_map_of_roots(gpu):
    reg, area, _, R, _ = case("xctest:2x2_rows")
    want = cm.model(reg, area, np.zeros((0, 2), np.uint32), R)
    got = run(gpu, reg, area, [], R)
    same(got, want)
    assert got["nroots"] == 2 and got["levels"] == 1 and got["order"].tolist() == [0, 1]


@pytest.mark.parametrize("left_out", ARRAYS)
def test_each_output_left_out_in_turn(gpu, left_out):
    reg, area, edges, R, want = case("rings:33")
    names = [k for k in ARRAYS if k != left_out and not (left_out == "child_offsets" and k == "children")]
    got = run(gpu, reg, area, edges, R, outputs=names)
    assert left_out not in got
    same(got, want, names)


def test_a_call_on_another_stream(gpu):
    import torch
    reg, area, edges, R, want = case("noise:64:4:own")
    stream = torch.cuda.Stream()
    got = _raw(gpu, reg, area, edges, R, stream=ctypes.c_void_p(stream.cuda_stream))
    for k, used in (("roots", want["nroots"]), ("children", want["reached"] - want["nroots"]),
                    ("order", want["reached"])):
        got[k] = got[k][:used]
    same(got, want)
