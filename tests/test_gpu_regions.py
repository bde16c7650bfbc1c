"""GPU: connected regions of a label map (include/dq_hip.h, "connected regions").

The reference is the plain raster-order flood fill below (numpy + a Python
stack, 4- and 8-connectivity): regions are numbered in the order the raster
scan meets their first pixel, which is the definition.  It also computes area,
bounding box, first pixel, label and colour sums, and never uses the code
under test.  Equality is exact everywhere: array_equal on the region map and on
every stats array, and the region count R.

A pattern is a map of small integers; the u8 / u16 / u32 label maps are that
map sent through an injective table per width (u16: values above 255; u32:
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

pytestmark = pytest.mark.gpu

T = 64
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32}
SIGNED = {1: np.uint8, 2: np.int16, 4: np.int32}      # (torch storage)
GUARD_WORD = 0xA5A5A5A5


# ---------------------------------------------------------------------------
# The reference.
def flood_fill_regions(lab2d, connectivity, pixels=None):
    """(regions2d uint32, stats) of a 2-D integer map by raster-order flood fill."""
    lab2d = np.asarray(lab2d)
    h, w = lab2d.shape
    n = h * w
    lab = lab2d.reshape(-1).tolist()
    reg = [-1] * n
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    else:
        assert connectivity == 4
    count = 0
    for s in range(n):
        if reg[s] >= 0:
            continue
        rid, L = count, lab[s]
        count += 1
        reg[s] = rid
        stack = [s]
        while stack:
            i = stack.pop()
            y, x = divmod(i, w)
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w:
                    j = yy * w + xx
                    if reg[j] < 0 and lab[j] == L:
                        reg[j] = rid
                        stack.append(j)
    reg = np.array(reg, np.int64)
    ys, xs = np.divmod(np.arange(n, dtype=np.int64), w)
    first = np.full(count, n, np.int64)
    np.minimum.at(first, reg, np.arange(n, dtype=np.int64))
    bbox = np.zeros((count, 4), np.int64)
    bbox[:, 0], bbox[:, 1] = w, h
    np.minimum.at(bbox[:, 0], reg, xs)
    np.minimum.at(bbox[:, 1], reg, ys)
    np.maximum.at(bbox[:, 2], reg, xs)
    np.maximum.at(bbox[:, 3], reg, ys)
    stats = {"area": np.bincount(reg, minlength=count).astype(np.uint32),
             "bbox": bbox.astype(np.uint32),
             "first": first.astype(np.uint32),
             "label": lab2d.reshape(-1)[first].astype(np.uint32)}
    if pixels is not None:
        px = np.asarray(pixels, np.uint32).reshape(-1)
        sums = np.zeros((count, 3), np.uint64)
        for c, shift in enumerate((16, 8, 0)):
            np.add.at(sums[:, c], reg, ((px >> shift) & 0xFF).astype(np.uint64))
        stats["sums"] = sums
    assert (np.diff(stats["first"].astype(np.int64)) > 0).all()   # numbered in raster order of the first pixel
    return reg.astype(np.uint32).reshape(h, w), stats


# ---------------------------------------------------------------------------
# Patterns: (h, w) maps of small non-negative integers.
def _noise(w, h, k, seed=0):
    return (fx.xorshift(w * h, seed=fx.SEED + seed) % np.uint32(k)).astype(np.int64).reshape(h, w)


def _spiral(w, h):
    a = np.zeros((h, w), np.int64)
    x = y = d = 0
    a[0, 0] = 1
    dirs = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    inside = lambda px, py: 0 <= px < w and 0 <= py < h  # noqa: E731
    while True:
        for _ in range(2):
            dx, dy = dirs[d]
            nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(nx, ny) and a[ny, nx] == 0 and (not inside(ax, ay) or a[ay, ax] == 0):
                x, y = nx, ny
                a[y, x] = 1
                break
            d = (d + 1) % 4
        else:
            return a


def _pattern(name, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    if name == "constant":
        return np.full((h, w), 5, np.int64)
    if name == "checker":
        return ((xs + ys) & 1).astype(np.int64)
    if name == "hstripes":
        return (ys & 1).astype(np.int64)
    if name == "vstripes":
        return (xs & 1).astype(np.int64)
    if name == "spiral":
        return _spiral(w, h)
    if name == "comb":      # teeth on the even columns, joined along the last row
        return (((xs & 1) == 0) | (ys == h - 1)).astype(np.int64)
    if name == "rings":
        return ((np.maximum(abs(xs - w // 2), abs(ys - h // 2)) // 3) & 1).astype(np.int64)
    if name == "diagonals":  # x == y passes (T-1, T-1) -> (T, T); x + y == 2T - 1 passes (T, T-1) -> (T-1, T)
        return np.where((xs - ys) % 8 == 0, 1, np.where((xs + ys) % 8 == 7, 2, 0)).astype(np.int64)
    if name.startswith("noise"):
        return _noise(w, h, int(name[5:]))
    raise KeyError(name)


PATTERNS = ["constant", "checker", "hstripes", "vstripes", "spiral", "comb", "rings", "diagonals",
            "noise2", "noise3", "noise200"]
PW, PH = 200, 150    # multi-tile: 4 x 3 tiles, partial tiles on both edges

#            (w, h)
SHAPES = [(1, 1), (7, 1), (1, 7),
          (T, T), (T + 1, T), (T, T + 1), (T + 1, T + 1),
          (3 * T - 1, 3 * T - 1),                      # (width % 4 == 3)
          (T + 2, 5), (T + 3, 5), (2 * T + 2, T + 6)]  # width % 4 == 2, 3, 2: u8 / u16 rows start misaligned


@functools.lru_cache(maxsize=None)
def _base(name, w, h):
    a = _pattern(name, w, h)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _frame(w, h):
    px = fx.xorshift(w * h, seed=fx.SEED + 77)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def _reference(name, w, h, connectivity):
    """The flood fill of a pattern, once (with the colour sums of _frame)."""
    reg, st = flood_fill_regions(_base(name, w, h), connectivity, _frame(w, h))
    for a in [reg] + list(st.values()):
        a.setflags(write=False)
    return reg, st


def _widen(base, width):
    """The pattern as a label map of `width` bytes through an injective table."""
    b = base.astype(np.uint32)
    assert b.max() < 256
    if width == 1:
        return b.astype(np.uint8)
    if width == 2:
        return (b * 257 + 300).astype(np.uint16)            # 300 .. 65535
    return ((b << 24) | np.uint32(0x00ABCDEF)).astype(np.uint32)   # differ only in the top byte


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {"u1": np.uint8, "u2": np.int16, "u4": np.int32, "u8": np.int64}[a.dtype.str[1:]]
    return torch.from_numpy(a.view(signed).copy()).to("cuda:0")


def _to_host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _run(gpu, lab2d, connectivity, cap=0, pixels=None, stream=None):
    """label_regions_device on fresh tensors -> (R, regions2d, stats as unsigned numpy)."""
    import torch
    h, w = lab2d.shape
    t_lab = _to_dev(lab2d.reshape(-1))
    t_reg = torch.full((h * w,), -1, dtype=torch.int32, device="cuda:0")
    t_px = _to_dev(pixels) if pixels is not None else None
    if stream is not None:   # (the tensors above were filled on the current stream)
        stream.wait_stream(torch.cuda.current_stream())
    r, st = gpu.label_regions_device(t_lab, w, h, t_reg, connectivity=connectivity, stats_capacity=cap,
                                     t_pixels=t_px, stream=stream)
    out = {k: _to_host(v, np.uint64 if k == "sums" else np.uint32) for k, v in st.items()}
    return r, _to_host(t_reg, np.uint32).reshape(h, w), out


def _check(gpu, name, w, h, connectivity, width):
    want_reg, want = _reference(name, w, h, connectivity)
    lab = _widen(_base(name, w, h), width)
    R = len(want["area"])
    r, reg, st = _run(gpu, lab, connectivity, cap=R, pixels=_frame(w, h))
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
    base = _base("diagonals", PW, PH)
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
    lab = _widen(_base("noise3", w, h), 1)
    t_lab, t_px = _to_dev(lab.reshape(-1)), _to_dev(_frame(w, h))
    t_reg = torch.full((w * h,), -1, dtype=torch.int32, device="cuda:0")
    guard = np.full(1, GUARD_WORD, np.uint32).view(np.int32)[0]
    per = {"area": 1, "bbox": 4, "first": 1, "label": 1, "sums": 6}   # 4-byte words per region
    bufs = {k: torch.full(((cap + 8) * p,), int(guard), dtype=torch.int32, device="cuda:0") for k, p in per.items()}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    r = gpu.lib().dq_hip_label_regions_dev(0, ptr(t_lab), 1, w, h, connectivity, ptr(t_reg), cap, ptr(bufs["area"]),
                                           ptr(bufs["bbox"]), ptr(bufs["first"]), ptr(bufs["label"]), ptr(t_px),
                                           ptr(bufs["sums"]), None)
    assert r == R
    assert np.array_equal(_to_host(t_reg, np.uint32).reshape(h, w), want_reg)
    for k, p in per.items():
        got = _to_host(bufs[k], np.uint32)
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
        lab = _widen(_base(name, PW, PH), 2)
        results[i] = _run(gpu, lab, connectivity, cap=len(_reference(name, PW, PH, connectivity)[1]["area"]),
                          pixels=_frame(PW, PH), stream=streams[i])

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
    lab = _widen(_base("noise3", PW, PH), 1)
    R = len(_reference("noise3", PW, PH, 8)[1]["area"])
    a = _run(gpu, lab, 8, cap=R, pixels=_frame(PW, PH))
    b = _run(gpu, lab, 8, cap=R, pixels=_frame(PW, PH))
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
    lab = _widen(_base("noise3", w, h), width).reshape(-1)
    room = torch.zeros(w * h + 1, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[width], device="cuda:0")
    room[1:] = _to_dev(lab)
    t_lab = room[1:]
    t_reg = torch.full((w * h + 1,), -1, dtype=torch.int32, device="cuda:0")
    assert t_lab.is_contiguous() and t_lab.data_ptr() % (4 if width < 4 else 16) == width
    r, st = gpu.label_regions_device(t_lab, w, h, t_reg[1:], connectivity=connectivity, stats_capacity=4)
    got = _to_host(t_reg, np.uint32)
    assert r == len(want["area"]) and got[0] == 0xFFFFFFFF
    assert np.array_equal(got[1:].reshape(h, w), want_reg)
    assert np.array_equal(_to_host(st["area"], np.uint32), want["area"][:4])
