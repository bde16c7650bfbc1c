"""The inputs of test_gpu_regions_atsize.py and the thresholds they are there to
cross (no GPU).

Two label maps of 1100 x 1000 pixels, 4-connected, from region_inputs.noise:
A (three labels) and B (200 labels), and the area arrays of the size order
alone.  The builders below run the stage suites' own models on them, once per
session (lru_cache); the GPU file imports them from here.  The tests assert
that every input is past the size at which the code it is meant for takes
another path -- the second block of a one-workgroup top scan, the second trip
of a bounded grid-stride loop -- so that a later edit to a map cannot quietly
put a test back below it.  The counts are asserted as inequalities only."""
import functools

import numpy as np

import containment_model as cm
import region_inputs
from adjacency_model import adjacency_model
from pixels_model import rows_total
from regions_model import flood_fill_regions

W, H = 1100, 1000
N = W * H
CONN = 4
LABELS = {"A": 3, "B": 200}
SORT_R = 4 * 2 ** 20 + 1025


def _frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def labels(name):
    lab = region_inputs.noise(W, H, LABELS[name], dtype=np.int64)
    lab.setflags(write=False)
    return lab


def frame():
    return region_inputs.frame(W, H)


@functools.lru_cache(maxsize=None)
def regions(name, connectivity=CONN):
    """(region map (H, W) uint32, stats) of a map by the flood fill, with the sums of the frame."""
    reg, st = flood_fill_regions(labels(name), connectivity, frame())
    _frozen([reg] + list(st.values()))
    return reg, st


def count(name):
    return len(regions(name)[1]["area"])


@functools.lru_cache(maxsize=None)
def graph(name):
    """adjacency_model of the map's regions, with steps and degree."""
    return adjacency_model(regions(name)[0], CONN, frame(), count(name))


@functools.lru_cache(maxsize=None)
def tree(name):
    """containment_model.model over the flood fill's areas and the adjacency model's edges."""
    reg, st = regions(name)
    want = cm.model(reg, st["area"], graph(name)["edges"], count(name))
    _frozen(want.values())
    return want


# ---------------------------------------------------------------------------
def test_the_maps_have_more_than_1024_chunks():
    # kRegionChunk = 1024 pixels a chunk (regions, adjacency; merge: 1024 bits of the first-pixel bitmap),
    # 1024 threads in scan::scan_top_kernel over the root, head, edge and bitmap counts: one block of each
    # top scan covers 1024 * 1024 pixels
    assert N > 1048576
    for name in LABELS:
        assert labels(name).shape == (H, W) and int(labels(name).max()) < 256   # (widen takes them)


def test_map_b_crosses_the_shared_scan_and_the_stride_loops():
    reg, _ = regions("B")
    R, E, T = count("B"), graph("B")["E"], rows_total(reg)
    # scan::kChunk = kRegionChunk = 1024 values a chunk, 1024 threads in scan::scan_top_kernel
    assert R > 1048576          # pixels: Heights; containment: childoff and S, R + 1 values
    assert T > 1048576          # pixels: table
    assert T <= N               # (or the pixel lists are refused)
    # kCountBlocks = 2048 workgroups of 256 threads: contain_roots_kernel (regions), contain_level_kernel (edges)
    assert E > 524288
    # kLinkBlocks = 2048 workgroups of 256 threads: merge_link_kernel (regions)
    assert R > 524288


def test_map_a_crosses_the_stride_loop_of_the_levels_alone():
    R, E = count("A"), graph("A")["E"]
    # kCountBlocks = 2048 workgroups of 256 threads: contain_level_kernel strides over the edges
    assert E > 524288
    # scan::kChunk = 1024 values a chunk, 1024 threads in scan::scan_top_kernel: A stays in one block there
    assert R < 1048576
    assert tree("A")["levels"] >= 2


def test_the_sort_counts_have_more_than_1024_chunks():
    # sort::kTile = 1024 pairs a tile, 256 counts a tile (sort::kDigits); their scan is scan::scan_top_kernel's
    tiles = -(-SORT_R // 1024)
    assert 256 * tiles > 1048576
    assert tiles > 1024         # (a digit's row of counts lies across several scan chunks)
    # kCountBlocks = 2048 workgroups of 256 threads: size_bits_kernel strides over the areas
    assert SORT_R > 524288
