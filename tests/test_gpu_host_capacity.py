"""GPU: what the host-pointer entry points copy back when the capacity is short.

The Python wrappers call count-first and then with the exact capacity, so the
copy-back sizes of dq_hip_label_regions, dq_hip_region_adjacency,
dq_hip_segment_labels, dq_hip_region_windows and dq_hip_window_tags at any other
capacity are reached only here: the library is called through ctypes on numpy
arrays.  The expectation is each entry's own result at an ample capacity (what
the stage suites verify against their models); the rules checked are the ones
include/dq_hip.h states:
  * entry arrays of regions / adjacency / segment hold min(count, cap) entries;
  * windows and tags write their offsets / rows but no list entry when the
    count exceeds the capacity;
  * a refused map (-2) leaves every host array as it was.
Every output array is filled with a sentinel first and carries guard words
behind its nominal end.  One 24 x 16 map of three noise labels, 8-connected:
62 regions, a few thousand window entries."""
import ctypes

import numpy as np
import pytest

from merge_model import NONE
from region_inputs import frame, noise, wmap

pytestmark = pytest.mark.gpu

W, H, CONN = 24, 16, 8
BLOCK, EXPAND = 4, 1
GUARD = 8
FILL = {np.dtype(np.uint32): 0xA5A5A5A5, np.dtype(np.uint64): 0xA5A5A5A5A5A5A5A5}
U64 = ("sums", "step")                  # the 8-byte arrays
AMPLE = 8192                            # a capacity well above every count of this map


def _out(entries, per=1, dtype=np.uint32):
    """A sentinel-filled output array of entries * per elements and the guard."""
    return np.full(entries * per + GUARD, FILL[np.dtype(dtype)], dtype)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _sentinel(a):
    return bool((a == FILL[a.dtype]).all())


def _outs(cap, per):
    return {k: _out(cap, p, np.uint64 if k in U64 else np.uint32) for k, p in per.items()}


def _prefix_only(got, want, per, cap):
    """Entries [0, cap) are the ample run's; entry cap, what follows and the guard are untouched."""
    for k, p in per.items():
        assert np.array_equal(got[k][:cap * p], want[k][:cap * p]), k
        assert _sentinel(got[k][cap * p:]), k


def _labels():
    lab = np.ascontiguousarray(noise(W, H, 3, seed=1), np.uint32)
    return lab, np.ascontiguousarray(frame(W, H), np.uint32)


# ---------------------------------------------------------------------------
REGION_PER = {"area": 1, "bbox": 4, "first": 1, "label": 1, "sums": 3}


def _regions(gpu, cap):
    lab, px = _labels()
    o = _outs(cap, REGION_PER)
    o["regions"] = _out(W * H)
    rc = gpu.lib().dq_hip_label_regions(_p(lab), 4, W, H, CONN, _p(o["regions"]), cap, _p(o["area"]), _p(o["bbox"]),
                                        _p(o["first"]), _p(o["label"]), _p(px), _p(o["sums"]))
    return rc, o


@pytest.fixture(scope="module")
def region_map(gpu):
    """(region ids, R, the stats at an ample capacity) of the map every case below uses."""
    R, o = _regions(gpu, AMPLE)
    assert 12 <= R < AMPLE
    reg = o["regions"][:W * H].copy()
    reg.setflags(write=False)
    return reg, int(R), o


def test_regions(gpu, region_map):
    _, R, ample = region_map
    assert _sentinel(ample["regions"][W * H:])
    for k, p in REGION_PER.items():      # ample: nothing behind entry R
        assert _sentinel(ample[k][R * p:]) and not _sentinel(ample[k][:R * p]), k
    rc, short = _regions(gpu, R - 1)
    assert rc == R
    assert np.array_equal(short["regions"], ample["regions"])
    _prefix_only(short, ample, REGION_PER, R - 1)


# ---------------------------------------------------------------------------
EDGE_PER = {"edges": 2, "border": 1, "contact": 2, "step": 1}


def _adjacency(gpu, reg, R, cap):
    _, px = _labels()
    o = _outs(cap, EDGE_PER)
    o["degree"] = _out(R)
    rc = gpu.lib().dq_hip_region_adjacency(_p(reg), W, H, CONN, cap, _p(o["edges"]), _p(o["border"]),
                                           _p(o["contact"]), _p(px), _p(o["step"]), R, _p(o["degree"]))
    return rc, o


def test_adjacency(gpu, region_map):
    reg, R, _ = region_map
    E, ample = _adjacency(gpu, reg, R, AMPLE)
    assert 12 <= E < AMPLE
    for k, p in EDGE_PER.items():
        assert _sentinel(ample[k][E * p:]) and not _sentinel(ample[k][:E * p]), k
    assert _sentinel(ample["degree"][R:]) and not _sentinel(ample["degree"][:R])
    rc, short = _adjacency(gpu, reg, R, E - 1)
    assert rc == E
    assert np.array_equal(short["degree"], ample["degree"])
    _prefix_only(short, ample, EDGE_PER, E - 1)


# ---------------------------------------------------------------------------
SEGMENT_PER = {"area": 1, "bbox": 4, "first": 1, "sums": 3}


def _segment(gpu, cap):
    lab, px = _labels()
    o = _outs(cap, SEGMENT_PER)
    o["regions"] = _out(W * H)
    rounds = ctypes.c_uint32(0)
    rc = gpu.lib().dq_hip_segment_labels(_p(lab), 4, W, H, CONN, _p(px), 3, NONE, 0, _p(o["regions"]), cap,
                                         _p(o["area"]), _p(o["bbox"]), _p(o["first"]), _p(o["sums"]),
                                         ctypes.byref(rounds))
    return rc, rounds.value, o


def test_segment(gpu, region_map):
    _, R, _ = region_map
    R2, rounds, ample = _segment(gpu, AMPLE)
    assert 2 <= R2 < R and rounds >= 1
    assert _sentinel(ample["regions"][W * H:]) and int(ample["regions"][:W * H].max()) == R2 - 1
    for k, p in SEGMENT_PER.items():
        assert _sentinel(ample[k][R2 * p:]) and not _sentinel(ample[k][:R2 * p]), k
    rc, rounds2, short = _segment(gpu, R2 - 1)
    assert rc == R2 and rounds2 == rounds
    assert np.array_equal(short["regions"], ample["regions"])
    _prefix_only(short, ample, SEGMENT_PER, R2 - 1)


# ---------------------------------------------------------------------------
LISTS = ("coords", "index", "colors")


def _windows(gpu, reg, w, h, R, cap, room=None, expand=EXPAND):
    px = np.ascontiguousarray(frame(w, h), np.uint32)
    o = {k: _out(cap if room is None else room) for k in LISTS}
    o["offsets"] = _out(R + 1)
    rc = gpu.lib().dq_hip_region_windows(_p(reg), w, h, R, BLOCK, expand, None, None, 0, _p(o["offsets"]), cap,
                                         _p(o["coords"]), _p(o["index"]), _p(px), _p(o["colors"]))
    return rc, o


def test_windows(gpu, region_map):
    reg, R, _ = region_map
    M, ample = _windows(gpu, reg, W, H, R, AMPLE)
    assert W * H <= M < AMPLE
    assert ample["offsets"][R] == M and _sentinel(ample["offsets"][R + 1:])
    for k in LISTS:
        assert _sentinel(ample[k][M:]) and not _sentinel(ample[k][:M]), k
    rc, short = _windows(gpu, reg, W, H, R, M - 1, room=M)
    assert rc == M
    assert np.array_equal(short["offsets"], ample["offsets"])
    for k in LISTS:                      # M > cap: no list entry at all
        assert _sentinel(short[k]), k


# ---------------------------------------------------------------------------
ENTRIES = ("ids", "counts", "first")
PER_REGION = ("inside", "best", "best_count")


def _tags(gpu, reg, w, h, R, cap, room=None, expand=EXPAND):
    o = {k: _out(cap if room is None else room) for k in ENTRIES}
    o.update({k: _out(R) for k in PER_REGION})
    o.update({k: _out(R + 1) for k in ("rows", "offsets")})
    rc = gpu.lib().dq_hip_window_tags(_p(reg), w, h, R, BLOCK, expand, None, None, 0, _p(o["rows"]), cap, _p(o["ids"]),
                                      _p(o["counts"]), _p(o["first"]), _p(o["inside"]), _p(o["best"]),
                                      _p(o["best_count"]), _p(o["offsets"]))
    return rc, o


def test_tags(gpu, region_map):
    reg, R, _ = region_map
    E, ample = _tags(gpu, reg, W, H, R, AMPLE)
    assert R <= E < AMPLE
    assert ample["rows"][R] == E
    for k in ("rows", "offsets"):
        assert _sentinel(ample[k][R + 1:]) and not _sentinel(ample[k][:R + 1]), k
    for k in PER_REGION:
        assert _sentinel(ample[k][R:]) and not _sentinel(ample[k][:R]), k
    for k in ENTRIES:
        assert _sentinel(ample[k][E:]) and not _sentinel(ample[k][:E]), k
    rc, short = _tags(gpu, reg, W, H, R, E - 1, room=E)
    assert rc == E
    for k in ("rows", "offsets") + PER_REGION:
        assert np.array_equal(short[k], ample[k]), k
    for k in ENTRIES:                    # E > cap: no entry at all
        assert _sentinel(short[k]), k


# ---------------------------------------------------------------------------
# A refused map leaves the offsets and the lists as they were.
def test_refused_pixels(gpu):
    w, h, R = 4, 64, 5                   # (test_gpu_pixels.py: the ids span 318 rows, the map has 256 pixels)
    reg = np.full((h, w), 4, np.uint32)
    reg[0] = reg[63] = np.arange(4)
    o = {k: _out(w * h) for k in LISTS}
    o["offsets"] = _out(R + 1)
    px = np.ascontiguousarray(frame(w, h), np.uint32)
    rc = gpu.lib().dq_hip_region_pixels(_p(reg), w, h, R, _p(o["offsets"]), _p(o["coords"]), _p(o["index"]), _p(px),
                                        _p(o["colors"]))
    assert rc == -2
    for k, v in o.items():
        assert _sentinel(v), k


@pytest.mark.parametrize("stage", [_windows, _tags], ids=["windows", "tags"])
def test_refused_windows(gpu, stage):
    reg, R = wmap("refused")             # (test_gpu_windows.py: 98 block rows, 50 pairs at d = 4, e = 0)
    h, w = reg.shape
    rc, o = stage(gpu, np.ascontiguousarray(reg.reshape(-1)), w, h, R, w * h, expand=0)
    assert rc == -2
    for k, v in o.items():
        assert _sentinel(v), k
