"""GPU: connected regions of a label map (include/dq_hip.h, "connected regions").

The reference is flood_fill_regions of regions_model.py, which never uses the
code under test.  Equality is exact everywhere: array_equal on the region map
and on every stats array, and the region count R.

A pattern (region_inputs.py) is a map of small integers; the u8 / u16 / u32
label maps are that map sent through an injective table per width (u16: values above 255; u32:
values above 65535 that differ ONLY in the top byte), so the three widths share
one flood fill per (pattern, connectivity) and differ only in the "label" stat.

T = pkg.REGION_TILE (DQ_HIP_REGION_TILE in the header) is the tile of the tile
pass; the shapes are the smallest at which each mechanism can fail."""
import ctypes
import functools
import os
import re
import threading

import numpy as np
import pytest

import dq_fixtures as fx
from region_dev import to_dev, to_host
from region_inputs import frame, regions_base, widen
from regions_model import flood_fill_regions

pytestmark = pytest.mark.gpu

T = 64
GUARD_WORD = 0xA5A5A5A5

PATTERNS = ["constant", "checker", "hstripes", "vstripes", "spiral", "comb", "rings", "diagonals",
            "noise2", "noise3", "noise200"]
PW, PH = 200, 150    # multi-tile: 4 x 3 tiles, partial tiles on both edges

#            (w, h)
SHAPES = [(1, 1), (7, 1), (1, 7),
          (T, T), (T + 1, T), (T, T + 1), (T + 1, T + 1),
          (3 * T - 1, 3 * T - 1),                      # (width % 4 == 3)
          (T + 2, 5), (T + 3, 5), (2 * T + 2, T + 6)]  # width % 4 == 2, 3, 2: u8 / u16 rows start misaligned


@functools.lru_cache(maxsize=None)
def _reference(name, w, h, connectivity):
    """The flood fill of a pattern, once (with the colour sums of frame)."""
    reg, st = flood_fill_regions(regions_base(name, w, h), connectivity, frame(w, h))
    for a in [reg] + list(st.values()):
        a.setflags(write=False)
    return reg, st


def _run(gpu, lab2d, connectivity, cap=0, pixels=None, stream=None):
    """label_regions_device on fresh tensors -> (R, regions2d, stats as unsigned numpy)."""
    import torch
    h, w = lab2d.shape
    t_lab = to_dev(lab2d.reshape(-1))
    t_reg = torch.full((h * w,), -1, dtype=torch.int32, device="cuda:0")
    t_px = to_dev(pixels) if pixels is not None else None
    if stream is not None:   # (the tensors above were filled on the current stream)
        stream.wait_stream(torch.cuda.current_stream())
    r, st = gpu.label_regions_device(t_lab, w, h, t_reg, connectivity=connectivity, stats_capacity=cap,
                                     t_pixels=t_px, stream=stream)
    out = {k: to_host(v, np.uint64 if k == "sums" else np.uint32) for k, v in st.items()}
    return r, to_host(t_reg, np.uint32).reshape(h, w), out


def _check(gpu, name, w, h, connectivity, width):
    want_reg, want = _reference(name, w, h, connectivity)
    lab = widen(regions_base(name, w, h), width)
    R = len(want["area"])
    r, reg, st = _run(gpu, lab, connectivity, cap=R, pixels=frame(w, h))
    assert r == R
    assert np.array_equal(reg, want_reg)
    assert sorted(st) == ["area", "bbox", "first", "label", "sums"]
    for k in ("area", "bbox", "first", "sums"):
        assert st[k].shape == want[k].shape and np.array_equal(st[k], want[k]), k
    assert np.array_equal(st["label"], lab.reshape(-1)[want["first"]].astype(np.uint32))
    assert int(st["area"].sum()) == w * h
    return R


def test_tile_constant_matches_the_header(gpu):
    text = open(os.path.join(fx.ROOT, "include", "dq_hip.h")).read()
    assert int(re.search(r"#define\s+DQ_HIP_REGION_TILE\s+(\d+)", text).group(1)) == gpu.REGION_TILE == T


@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes(gpu, shape, connectivity, width):
    """Three-label noise (dense runs, many unions, many seam pairs) at the
    shapes where a mechanism changes: one pixel, one row, one column, exactly
    one tile, one pixel more each way, partial last tiles, misaligned rows."""
    _check(gpu, "noise3", shape[0], shape[1], connectivity, width)


@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", PATTERNS)
def test_patterns(gpu, name, connectivity, width):
    R = _check(gpu, name, PW, PH, connectivity, width)
    if name == "constant":
        assert R == 1
    if name == "checker":
        assert R == (PW * PH if connectivity == 4 else 2)
    if name == "hstripes":
        assert R == PH
    if name == "vstripes":
        assert R == PW


def test_diagonals_differ_exactly_at_the_seams(gpu):
    """The lines of "diagonals" touch only at corners, also across the tile
    corners: one region per pixel of a line with 4-connectivity, one per line
    with 8 (the reference says so; here the two answers are told apart)."""
    base = regions_base("diagonals", PW, PH)
    r4 = _reference("diagonals", PW, PH, 4)[0]
    r8 = _reference("diagonals", PW, PH, 8)[0]
    assert base[T - 1, T - 1] == base[T, T] == 1 and base[T - 1, T] == base[T, T - 1] == 2
    assert r4[T - 1, T - 1] != r4[T, T] and r8[T - 1, T - 1] == r8[T, T]
    assert r4[T - 1, T] != r4[T, T - 1] and r8[T - 1, T] == r8[T, T - 1]


def test_cookie_crop_through_quant_labels(gpu):
    """Real data through the host forms: a 256 x 256 crop -> quant_labels at
    K = 16 -> regions with the colour sums of the crop."""
    px, w, h = fx.load_png_u32(os.path.join(fx.GOLDEN, "png", "cookie.png"))
    assert w >= 256 and h >= 256
    x0, y0 = (w - 256) // 2, (h - 256) // 2
    crop = np.ascontiguousarray(px.reshape(h, w)[y0:y0 + 256, x0:x0 + 256]).reshape(-1)
    labels, ct = gpu.quant_labels(crop, 16)
    assert labels.dtype == np.uint8 and len(ct) <= 16
    lab2d = labels.reshape(256, 256)
    for connectivity in (8, 4):
        want_reg, want = flood_fill_regions(lab2d, connectivity, crop)
        reg, st = gpu.label_regions(lab2d, connectivity=connectivity, pixels=crop)
        assert reg.dtype == np.uint32 and np.array_equal(reg, want_reg)
        assert sorted(st) == sorted(want)
        for k in want:
            assert st[k].dtype == want[k].dtype and np.array_equal(st[k], want[k]), k
        assert int(st["area"].sum()) == 256 * 256
        assert st["sums"].sum(axis=0).tolist() == [int(((crop >> s) & 0xFF).sum()) for s in (16, 8, 0)]


@pytest.mark.parametrize("which", ["zero", "half", "more"])
def test_stats_capacity(gpu, which):
    """Capacity 0, R // 2 and R + 5: the map and the return value do not
    change, the first min(R, cap) entries are the reference's, and nothing
    behind them is written (the arrays start as a guard pattern, 8 entries
    longer than the capacity)."""
    import torch
    w, h, connectivity = 2 * T + 2, T + 6, 8
    want_reg, want = _reference("noise3", w, h, connectivity)
    R = len(want["area"])
    cap = {"zero": 0, "half": R // 2, "more": R + 5}[which]
    m = min(R, cap)
    lab = widen(regions_base("noise3", w, h), 1)
    t_lab, t_px = to_dev(lab.reshape(-1)), to_dev(frame(w, h))
    t_reg = torch.full((w * h,), -1, dtype=torch.int32, device="cuda:0")
    guard = np.full(1, GUARD_WORD, np.uint32).view(np.int32)[0]
    per = {"area": 1, "bbox": 4, "first": 1, "label": 1, "sums": 6}   # 4-byte words per region
    bufs = {k: torch.full(((cap + 8) * p,), int(guard), dtype=torch.int32, device="cuda:0") for k, p in per.items()}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    r = gpu.lib().dq_hip_label_regions_dev(0, ptr(t_lab), 1, w, h, connectivity, ptr(t_reg), cap, ptr(bufs["area"]),
                                           ptr(bufs["bbox"]), ptr(bufs["first"]), ptr(bufs["label"]), ptr(t_px),
                                           ptr(bufs["sums"]), None)
    assert r == R
    assert np.array_equal(to_host(t_reg, np.uint32).reshape(h, w), want_reg)
    for k, p in per.items():
        got = to_host(bufs[k], np.uint32)
        assert (got[m * p:] == GUARD_WORD).all(), k
        head = got[:m * p]
        if k == "sums":
            head = head.view(np.uint64).reshape(m, 3)
        elif k == "bbox":
            head = head.reshape(m, 4)
        ref = lab.reshape(-1)[want["first"]].astype(np.uint32) if k == "label" else want[k]
        assert np.array_equal(head, ref[:m]), k


def test_two_streams_at_once(gpu):
    """Two calls with different inputs on two streams from two host threads
    (scratch is owned by each call) both come out right."""
    import torch
    cases = [("noise2", 8), ("spiral", 4)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in cases]
    results = [None, None]
    torch.cuda.synchronize()

    def work(i):
        name, connectivity = cases[i]
        lab = widen(regions_base(name, PW, PH), 2)
        results[i] = _run(gpu, lab, connectivity, cap=len(_reference(name, PW, PH, connectivity)[1]["area"]),
                          pixels=frame(PW, PH), stream=streams[i])

    for name, connectivity in cases:   # (the flood fills, before the threads start)
        _reference(name, PW, PH, connectivity)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for (name, connectivity), (r, reg, st) in zip(cases, results):
        want_reg, want = _reference(name, PW, PH, connectivity)
        assert r == len(want["area"]) and np.array_equal(reg, want_reg)
        for k in ("area", "bbox", "first", "sums"):
            assert np.array_equal(st[k], want[k]), k


def test_same_input_twice_gives_identical_bytes(gpu):
    lab = widen(regions_base("noise3", PW, PH), 1)
    R = len(_reference("noise3", PW, PH, 8)[1]["area"])
    a = _run(gpu, lab, 8, cap=R, pixels=frame(PW, PH))
    b = _run(gpu, lab, 8, cap=R, pixels=frame(PW, PH))
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
    for k in a[2]:
        assert a[2][k].tobytes() == b[2][k].tobytes(), k


@pytest.mark.parametrize("width", [1, 2, 4])
def test_pointers_offset_by_one_element(gpu, width):
    """Labels (and the region map) one element into their allocations: a u8
    map at an odd address, u16 at 2 mod 4, u32 and the regions at 4 mod 16."""
    import torch
    w, h, connectivity = T + 3, T + 2, 8
    want_reg, want = _reference("noise3", w, h, connectivity)
    lab = widen(regions_base("noise3", w, h), width).reshape(-1)
    room = torch.zeros(w * h + 1, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[width], device="cuda:0")
    room[1:] = to_dev(lab)
    t_lab = room[1:]
    t_reg = torch.full((w * h + 1,), -1, dtype=torch.int32, device="cuda:0")
    assert t_lab.is_contiguous() and t_lab.data_ptr() % (4 if width < 4 else 16) == width
    r, st = gpu.label_regions_device(t_lab, w, h, t_reg[1:], connectivity=connectivity, stats_capacity=4)
    got = to_host(t_reg, np.uint32)
    assert r == len(want["area"]) and got[0] == 0xFFFFFFFF
    assert np.array_equal(got[1:].reshape(h, w), want_reg)
    assert np.array_equal(to_host(st["area"], np.uint32), want["area"][:4])
