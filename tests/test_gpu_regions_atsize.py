"""GPU: the region-map stages just past the sizes at which their code takes
another path (include/dq_hip.h: connected regions, adjacency graph, merge,
pixel lists, containment tree, size order).

The stage suites check every mechanism at the smallest shape that can show it,
and none of their maps has more than 153 600 pixels.  Three things happen only
above that, on every frame of product size:
  * the second block of the one-workgroup top scan (scan::scan_top_kernel, in
    every stage: over root, head, edge and bitmap counts as over rows) and the
    carry into it: more than 1024 chunks of 1024 values, so more than 2^20
    pixels, regions, rows or sort counts;
  * the second trip of the bounded grid-stride loops (contain_roots_kernel,
    contain_level_kernel, size_bits_kernel, merge_link_kernel): more than
    2048 * 256 = 524 288 regions or edges;
  * chunk, tile and slot indexes at those counts.
test_regions_atsize_inputs.py builds the inputs (two 1100 x 1000 noise maps,
A with three labels and B with 200, and area arrays of 4 * 2^20 + 1025
regions) and asserts that each is past the threshold it is here for.

The references are the stage suites' own models, taken by import and run once
per session (lru_cache): flood_fill_regions and stats_model (regions_model.py),
adjacency_model, merge_model, lists_model (pixels_model.py),
containment_model.model and size_order.  Equality is exact: array_equal on every output array, == on every
count.  The tensors a test hands to a call (region maps, offsets and lists)
are 8 words longer than needed and filled with a guard word that must still be
there afterwards; the stats, graph and tree tensors are allocated by the
package wrapper at exactly the capacity asked for.

Each test prints the seconds its device calls took (uploads and read-backs
included) -- the models' time is the session's, not the test's."""
import contextlib
import functools
import time

import numpy as np
import pytest

import containment_model as cm
import test_regions_atsize_inputs as inp
from merge_model import merge_model
from pixels_model import lists_model
from region_dev import body, guarded, to_dev
from region_inputs import permuted as permuted_ids, widen
from regions_model import stats_model

pytestmark = pytest.mark.gpu

W, H, N, CONN = inp.W, inp.H, inp.N, inp.CONN
GUARD = 8
FILL = 0xA5A5A5A5
U64 = ("sums", "step", "enclosed")       # the 8-byte arrays
ARRAYS = cm.ARRAYS
_guarded = functools.partial(guarded, guard=GUARD, fill=FILL)


def _host(t, key=None):
    return t.cpu().numpy().view(np.uint64 if key in U64 else np.uint32)


def _same(got, want, keys):
    """region_dev.same, and at these sizes how many words differ and where."""
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        g, w = got[k].reshape(-1), want[k].reshape(-1)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (k, "%d of %d words differ, the first at %d" % (bad.size, w.size, bad[0]), g[bad[:4]],
                               w[bad[:4]])
        assert np.array_equal(got[k], want[k]), k


@contextlib.contextmanager
def _device_part(what):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("device part of %s: %.3f s" % (what, time.perf_counter() - t0))


# ---------------------------------------------------------------------------
# 1. Connected regions: scan::scan_top_kernel's second block, 1075 chunks in flatten / number / assign.
@pytest.mark.parametrize("name,width,connectivity", [("A", 1, 4), ("B", 4, 4), ("A", 1, 8)])
def test_regions(gpu, name, width, connectivity):
    want_reg, want = inp.regions(name, connectivity)
    R = len(want["area"])
    lab = widen(inp.labels(name), width)
    with _device_part("regions %s u%d conn %d" % (name, 8 * width, connectivity)):
        t_reg = _guarded(N)
        r, st = gpu.label_regions_device(to_dev(lab.reshape(-1)), W, H, t_reg, connectivity=connectivity,
                                         stats_capacity=R, t_pixels=to_dev(inp.frame()))
        reg = body(t_reg, N, GUARD, FILL, "regions")
        got = {k: _host(v, k) for k, v in st.items()}
    assert r == R, "R = %d, the flood fill has %d" % (r, R)
    bad = np.flatnonzero(reg != want_reg.reshape(-1))
    assert bad.size == 0, "R = %d: %d pixels differ, the first is %d" % (r, bad.size, bad[0])
    assert sorted(got) == ["area", "bbox", "first", "label", "sums"]
    _same(got, want, ("area", "bbox", "first", "sums"))
    assert np.array_equal(got["label"], lab.reshape(-1)[want["first"]].astype(np.uint32)), "R = %d" % r
    assert int(got["area"].sum()) == N


# ---------------------------------------------------------------------------
# 2. Adjacency: both launches of scan::scan_top_kernel, the table above 2^21 slots on B.
@pytest.mark.parametrize("name", ["A", "B"])
def test_adjacency(gpu, name):
    want, R = inp.graph(name), inp.count(name)
    E = want["E"]
    with _device_part("adjacency %s" % name):
        t_reg, t_px = to_dev(inp.regions(name)[0].reshape(-1)), to_dev(inp.frame())
        e0, g0 = gpu.region_adjacency_device(t_reg, W, H, connectivity=CONN)
        e, g = gpu.region_adjacency_device(t_reg, W, H, connectivity=CONN, edge_capacity=E, t_pixels=t_px,
                                           num_regions=R)
        got = {k: _host(v, k) for k, v in g.items()}
    assert e0 == E and g0 == {}, "the count-only call: E = %d, the model has %d" % (e0, E)
    assert e == E
    assert sorted(got) == ["border", "contact", "degree", "edges", "step"]
    _same(got, want, ("edges", "border", "contact", "step", "degree"))
    assert int(got["degree"].sum()) == 2 * E


# ---------------------------------------------------------------------------
# 3. Merge: scan::scan_top_kernel's second block, counts[chunk] for chunks >= 1024 in the numbering; on B (more
# than 524 288 regions) merge_link_kernel strides.
@functools.lru_cache(maxsize=None)
def _merged(name, min_area):
    reg, st = inp.regions(name)
    want = merge_model(reg.reshape(-1), st["area"], st["first"], st["sums"], st["bbox"], inp.graph(name)["edges"],
                       min_area)
    again = stats_model(want["regions"], W, inp.frame())      # (the folded stats are those of the output map)
    for k in ("area", "first", "bbox", "sums"):
        assert np.array_equal(want[k], again[k]), k
    return want


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "apart"])
@pytest.mark.parametrize("name,min_area", [("A", 4), ("B", 2)])
def test_merge(gpu, name, min_area, in_place):
    want, R = _merged(name, min_area), inp.count(name)
    reg, st = inp.regions(name)
    edges = inp.graph(name)["edges"]
    assert 1 < want["R"] < R and want["rounds"] >= 1
    with _device_part("merge %s min_area %d %s" % (name, min_area, "in place" if in_place else "apart")):
        t_in = _guarded(N)
        t_in[:N] = to_dev(reg.reshape(-1))
        t_out = t_in if in_place else _guarded(N)
        t = {k: to_dev(st[k].reshape(-1)) for k in ("area", "first", "sums", "bbox")}
        r, rounds, out = gpu.merge_regions_device(t_in, R, t["area"], t["first"], t["sums"], to_dev(edges.reshape(-1)),
                                                  min_area, t_bbox=t["bbox"], num_edges=len(edges),
                                                  t_out_regions=None if in_place else t_out, stats_capacity=R, n=N)
        assert out["regions"] is t_out
        got = {k: _host(v, k) for k, v in out.items() if k != "regions"}
        got["regions"] = body(t_out, N, GUARD, FILL, "the output map")
        kept = None if in_place else body(t_in, N, GUARD, FILL, "the input map")
    assert (r, rounds) == (want["R"], want["rounds"]), "R' = %d in %d rounds, the model: %d in %d" % (
        r, rounds, want["R"], want["rounds"])
    assert kept is None or np.array_equal(kept, reg.reshape(-1))
    assert sorted(got) == ["area", "bbox", "first", "regions", "remap", "sums"]
    _same(got, want, ("regions", "remap", "area", "first", "sums", "bbox"))
    assert int(got["area"].sum()) == N


# ---------------------------------------------------------------------------
# 4. Pixel lists: scan::scan_top_kernel's second block over the heights (R > 2^20) and the table (T > 2^20).
@functools.lru_cache(maxsize=None)
def _region_map(name, permuted):
    reg = inp.regions(name)[0]
    if permuted:
        reg = permuted_ids(reg, 5)
        reg.setflags(write=False)
    return reg


@functools.lru_cache(maxsize=None)
def _lists(name, permuted):
    return lists_model(_region_map(name, permuted), inp.count(name), inp.frame())


def _pixel_lists(gpu, t_reg, R, t_px):
    """region_pixels_device on fresh guarded tensors -> the four arrays on the host."""
    t = {"offsets": _guarded(R + 1), "index": _guarded(N), "coords": _guarded(N), "colors": _guarded(N)}
    gpu.region_pixels_device(t_reg, W, H, R, t["offsets"], t_coords=t["coords"], t_index=t["index"], t_pixels=t_px,
                             t_colors=t["colors"])
    return {k: body(v, R + 1 if k == "offsets" else N, GUARD, FILL, k) for k, v in t.items()}


@pytest.mark.parametrize("permuted", [False, True], ids=["raster_ids", "permuted_ids"])
def test_pixels(gpu, permuted):
    R = inp.count("B")
    reg, want = _region_map("B", permuted), _lists("B", permuted)
    assert permuted == (not np.array_equal(reg, inp.regions("B")[0]))
    with _device_part("pixels B%s" % (" permuted" if permuted else "")):
        got = _pixel_lists(gpu, to_dev(reg.reshape(-1)), R, to_dev(inp.frame()))
    assert got["offsets"][R] == N
    _same(got, want, ("offsets", "index", "coords", "colors"))


# ---------------------------------------------------------------------------
# 5. Containment: on B the scans of childoff and S have R + 1 > 2^20 values, contain_roots_kernel strides over
# the regions and contain_level_kernel over the edges, on 496 levels; on A only the level kernel strides.
def _containment(gpu, t_reg, R, t_area, t_edges):
    nroots, levels, reached, out = gpu.region_containment_device(t_reg, W, H, R, t_area, t_edges)
    return out, dict(nroots=nroots, levels=levels, reached=reached)


def _same_tree(out, counts, want):
    for k in ("nroots", "levels", "reached"):
        assert counts[k] == want[k], (k, counts[k], want[k])
    assert sorted(out) == sorted(ARRAYS)
    _same({k: _host(v, k) for k, v in out.items()}, want, ARRAYS)


@pytest.mark.parametrize("name", ["A", "B"])
def test_containment(gpu, name):
    want, R = inp.tree(name), inp.count(name)
    assert want["levels"] >= 2 and want["reached"] == R
    with _device_part("containment %s" % name):
        out, counts = _containment(gpu, to_dev(inp.regions(name)[0].reshape(-1)), R,
                                   to_dev(inp.regions(name)[1]["area"]), to_dev(inp.graph(name)["edges"]))
    _same_tree(out, counts, want)


def test_containment_of_b_with_the_edges_shuffled_and_a_third_doubled(gpu):
    import torch
    R, edges = inp.count("B"), inp.graph("B")["edges"]
    rng = np.random.default_rng(7)
    mixed = np.concatenate([edges, edges[rng.random(len(edges)) < 1 / 3]])
    mixed = mixed[rng.permutation(len(mixed))]
    swap = rng.random(len(mixed)) < 0.5
    mixed[swap] = mixed[swap][:, ::-1]
    assert len(mixed) > len(edges) + len(edges) // 4
    with _device_part("containment B twice"):
        t_reg, t_area = to_dev(inp.regions("B")[0].reshape(-1)), to_dev(inp.regions("B")[1]["area"])
        out, counts = _containment(gpu, t_reg, R, t_area, to_dev(edges))
        out2, counts2 = _containment(gpu, t_reg, R, t_area, to_dev(mixed))
        equal = {k: torch.equal(out[k], out2[k]) for k in ARRAYS}
    assert counts2 == counts
    assert all(equal.values()), equal
    _same_tree(out2, counts2, inp.tree("B"))


# ---------------------------------------------------------------------------
# 6. The size order alone: 4098 sort tiles, 1025 chunks in the scan of the counts, size_bits_kernel strides.
@functools.lru_cache(maxsize=None)
def _areas(pattern):
    R = inp.SORT_R
    rng = np.random.default_rng(R)
    if pattern == "random_2^32":      # four passes
        area = rng.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    elif pattern == "two_values":
        area = np.where(rng.integers(0, 2, R) == 1, 70000, 3).astype(np.uint32)
    else:                             # stability over four million equal keys (one digit: every count that is
        #                               not zero lies in the scan's first block, the carry shows in the other two)
        assert pattern == "equal"
        area = np.full(R, 7, np.uint32)
    order, rank = cm.size_order(area)
    for a in (area, order, rank):
        a.setflags(write=False)
    return area, order, rank


@pytest.mark.parametrize("pattern", ["random_2^32", "two_values", "equal"])
def test_regions_by_size(gpu, pattern):
    area, want_order, want_rank = _areas(pattern)
    assert pattern != "random_2^32" or int(area.max()) >= 1 << 24
    with _device_part("size order %s" % pattern):
        order, rank = gpu.regions_by_size_device(to_dev(area))
        got = {"order": _host(order), "rank": _host(rank)}
    _same(got, {"order": want_order, "rank": want_rank}, ("order", "rank"))
    if pattern == "equal":
        assert np.array_equal(got["order"], np.arange(inp.SORT_R, dtype=np.uint32))


# ---------------------------------------------------------------------------
# 7. The chain on A, each stage on the device output of the one before.
def test_chain_on_the_device(gpu):
    lab = widen(inp.labels("A"), 1)
    want_reg, want_stats = inp.regions("A")
    R, E = inp.count("A"), inp.graph("A")["E"]
    with _device_part("chain A"):
        t_px = to_dev(inp.frame())
        t_reg = _guarded(N)
        r, st = gpu.label_regions_device(to_dev(lab.reshape(-1)), W, H, t_reg, connectivity=CONN, stats_capacity=N,
                                         t_pixels=t_px)
        e0, _ = gpu.region_adjacency_device(t_reg, W, H, connectivity=CONN)
        e, g = gpu.region_adjacency_device(t_reg, W, H, connectivity=CONN, edge_capacity=e0, t_pixels=t_px,
                                           num_regions=r)
        out, counts = _containment(gpu, t_reg, r, st["area"], g["edges"])
        lists = _pixel_lists(gpu, t_reg, r, t_px)
        reg = body(t_reg, N, GUARD, FILL, "regions")
    assert (r, e0, e) == (R, E, E)
    assert np.array_equal(reg, want_reg.reshape(-1))
    _same({k: _host(v, k) for k, v in st.items()}, want_stats, ("area", "bbox", "first", "sums"))
    _same({k: _host(v, k) for k, v in g.items()}, inp.graph("A"), ("edges", "border", "contact", "step", "degree"))
    _same_tree(out, counts, inp.tree("A"))
    _same(lists, _lists("A", False), ("offsets", "index", "coords", "colors"))
