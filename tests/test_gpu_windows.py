"""GPU: the capture windows of a region map (include/dq_hip.h, "capture
windows") and the region map -> windows -> per-window quant pipeline.

The reference is windows_model of windows_model.py, written from the definition
alone and using none of the code under test; the maps, masks and the CASES the
tests run are in region_inputs.py.  The pipeline is checked against the CPU
oracle's weighted quant_recurse on each window's colours in list order, and
against quant_weighted_regions_device on the same ranges.  Equality is exact everywhere: array_equal on every array, ==
on every scalar.  Every output buffer carries guard words behind its last entry.

Shapes are the smallest at which each mechanism can fail: maps smaller than a
block, one block row, clipped right and bottom blocks, windows that meet the
grid's border and each other, a line whose cross and square dilations differ,
one region per pixel (208 members per block, M far above n; 1600 at d = 8,
e = 3), masks that empty a block and a whole window, regions the area rule
skips, a map the call must refuse, and a 512 x 300 map whose pairs cross the
second top-level chunk of the scan."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import dq_fixtures as fx
from region_dev import body, guarded, same, to_dev, to_host
from region_inputs import CASES, frame, mask_of, wmap
from windows_model import dilate_square, window_grids, windows_model

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = 0xA5A5A5A5
ARRAYS = ("index", "coords", "colors")
_guarded = functools.partial(guarded, guard=GUARD, fill=FILL)


# ---------------------------------------------------------------------------
def _run(gpu, reg, R, px, d, e, mask=None, area=None, min_area=0, want=ARRAYS, stream=None, total=None):
    """region_windows_device on fresh guarded tensors: the count-only call (unless `total` is given),
    then the call with room -> dict of the arrays asked for, the offsets and M."""
    import torch
    h, w = reg.shape
    t_reg, t_px = to_dev(reg.reshape(-1)), to_dev(px)
    t_mask = to_dev(mask.reshape(-1), np.uint8) if mask is not None else None
    t_area = to_dev(area) if area is not None else None
    if stream is not None:   # (the tensors above were filled on the current stream)
        stream.wait_stream(torch.cuda.current_stream())
    kw = dict(block=d, expand=e, t_mask=t_mask, t_area=t_area, min_area=min_area, stream=stream)
    if total is None:
        t_off = _guarded(R + 1)
        total = gpu.region_windows_device(t_reg, w, h, R, t_off, **kw)
        a = to_host(t_off)
        assert (a[R + 1:] == FILL).all() and a[R] == total
    t = {"offsets": _guarded(R + 1)}
    t.update({k: _guarded(total) for k in want})
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    got = gpu.region_windows_device(t_reg, w, h, R, t["offsets"], capacity=total if want else 0,
                                    t_coords=t.get("coords"), t_index=t.get("index"),
                                    t_pixels=t_px if "colors" in want else None, t_colors=t.get("colors"), **kw)
    assert got == total
    out = {"M": total}
    for k, v in t.items():
        out[k] = body(v, R + 1 if k == "offsets" else total, GUARD, FILL, k)
    return out


def _same(got, want, keys=("offsets",) + ARRAYS):
    assert got["M"] == int(want["offsets"][-1])
    same(got, want, keys)


def _check(gpu, name, d, e, mask=None, area=None, min_area=0):
    reg, R = wmap(name)
    assert (name, d, e) in CASES
    px = frame(reg.shape[1], reg.shape[0])
    want = windows_model(reg, R, px, d, e, mask, area, min_area)
    got = _run(gpu, reg, R, px, d, e, mask, area, min_area)
    _same(got, want)
    return got, want


# ---------------------------------------------------------------------------
# 1. d = 1, e = 0: the pixel lists.
@pytest.mark.parametrize("name", ["rows65", "comb"])
def test_block_one_expand_zero_is_the_pixel_lists(gpu, name):
    import torch
    got, _ = _check(gpu, name, 1, 0)
    reg, R = wmap(name)
    h, w = reg.shape
    t = {k: _guarded(w * h) for k in ARRAYS}
    t_off = _guarded(R + 1)
    gpu.region_pixels_device(to_dev(reg.reshape(-1)), w, h, R, t_off, t_coords=t["coords"], t_index=t["index"],
                             t_pixels=to_dev(frame(w, h)), t_colors=t["colors"])
    torch.cuda.synchronize()
    assert got["M"] == w * h and np.array_equal(got["offsets"], to_host(t_off)[:R + 1])
    for k in ARRAYS:
        assert np.array_equal(got[k], to_host(t[k])[:w * h]), k


# 2. Clipped right and bottom blocks, maps smaller than a block, one block row, one region.
@pytest.mark.parametrize("name", ["noise97x41", "rows3x5", "rows1x7", "rows64", "one"])
def test_clipping(gpu, name):
    got, _ = _check(gpu, name, 4, 2)
    reg, R = wmap(name)
    if name in ("rows3x5", "rows1x7", "one"):   # (every window is the whole grid)
        assert got["M"] == R * reg.size


# 3. The element is the cross, not the square.
@pytest.mark.parametrize("e", [1, 2])
def test_the_element_is_the_cross(gpu, e):
    reg, R = wmap("diagonal")
    cross = {r: g for r, _, _, g in window_grids(reg, R, 4, e)}
    square = {r: g for r, _, _, g in window_grids(reg, R, 4, e, dilate=dilate_square)}
    assert not np.array_equal(cross[1], square[1])        # (a wrong element cannot pass)
    # the block diagonal to an own block: in the window at e = 2, not at e = 1
    assert cross[1][0, 0] and cross[1][1, 1] and cross[1][0, 1] and bool(cross[1][0, 2]) == (e == 2)
    assert bool(cross[1][2, 0]) == (e == 2) and square[1][0, 2]
    _check(gpu, "diagonal", 4, e)


# 4. Windows at the grid's borders and windows that overlap.
def test_grid_borders_and_overlap(gpu):
    got, want = _check(gpu, "islands", 4, 2)
    lengths = np.diff(want["offsets"].astype(np.int64))
    assert lengths[1] == 6 * 16 and lengths[5] == 13 * 16          # a corner's window; the middle one's
    a, b = (set(got["index"][got["offsets"][r]:got["offsets"][r + 1]]) for r in (6, 7))
    assert a & b and a - b and b - a


# 5. One region per pixel: many lists per pixel.
@pytest.mark.parametrize("d,e", [(4, 2), (8, 3), (2, 0)])
def test_many_lists_per_pixel(gpu, d, e):
    got, _ = _check(gpu, "each16x12", d, e)
    assert got["M"] > 16 * 12 * (1 if e == 0 else 50)


# 6. Block sizes and expansions, ids in raster order and not.
@pytest.mark.parametrize("d,e", [(2, 1), (4, 0), (4, 2), (8, 3)])
@pytest.mark.parametrize("name", ["noise96x80", "noise96x80-permuted"])
def test_parameters(gpu, name, d, e):
    _check(gpu, name, d, e)


# 7. The mask.
@pytest.mark.parametrize("name,kind", [("noise64x48", "random"), ("noise64x48", "block"), ("islands", "island-window")])
def test_mask(gpu, name, kind):
    reg, R = wmap(name)
    mask = mask_of(kind, *reg.shape)
    got, want = _check(gpu, name, 4, 2, mask=mask)
    assert not set(got["index"]) & set(np.nonzero(mask.reshape(-1))[0])
    lengths = np.diff(got["offsets"].astype(np.int64))
    if kind == "island-window":       # its list is empty, its neighbours' lists are not
        assert lengths[1] == 0 and (lengths[[0, 2, 3, 4, 5, 6, 7]] > 0).all()
    else:
        assert got["M"] < int(windows_model(reg, R, frame(64, 48), 4, 2)["offsets"][-1])


# 8. The area rule.
def test_area_rule(gpu):
    reg, R = wmap("noise64x48")
    area = np.bincount(reg.reshape(-1), minlength=R).astype(np.uint32)
    skipped = area <= 8
    assert skipped.any() and not skipped.all()
    got, _ = _check(gpu, "noise64x48", 4, 2, area=area, min_area=8)
    lengths = np.diff(got["offsets"].astype(np.int64))
    assert (lengths[skipped] == 0).all() and (lengths[~skipped] > 0).all()
    # their pixels still appear in other windows
    assert set(np.nonzero(skipped[reg.reshape(-1)])[0]) <= set(got["index"])


# 8b. Ids >= R found no block and have no list; their pixels are pixels of the frame like any other.
def test_ids_at_or_above_the_region_count_are_skipped(gpu):
    reg, R = wmap("noise97x41")
    px = frame(97, 41)
    want = windows_model(reg, R - 40, px, 4, 2)
    got = _run(gpu, reg, R - 40, px, 4, 2)
    _same(got, want)
    assert got["M"] < int(windows_model(reg, R, None, 4, 2, lists=False)["offsets"][-1])
    assert set(np.nonzero(reg.reshape(-1) >= R - 40)[0]) <= set(got["index"])


# 9. A capacity one short: M comes back, the offsets are written, no list entry is.
def test_capacity_one_short(gpu):
    reg, R = wmap("noise97x41")
    h, w = reg.shape
    want = windows_model(reg, R, None, 4, 2, lists=False)
    M = int(want["offsets"][-1])
    t = {k: _guarded(M) for k in ARRAYS}
    t_off = _guarded(R + 1)
    got = gpu.region_windows_device(to_dev(reg.reshape(-1)), w, h, R, t_off, capacity=M - 1, t_coords=t["coords"],
                                    t_index=t["index"], t_pixels=to_dev(frame(w, h)), t_colors=t["colors"])
    assert got == M
    a = to_host(t_off)
    assert np.array_equal(a[:R + 1], want["offsets"]) and (a[R + 1:] == FILL).all()
    for k in ARRAYS:
        assert (to_host(t[k]) == FILL).all(), k


# 10. The count alone, each list array alone, all three.
@pytest.mark.parametrize("want", [(), ("index",), ("coords",), ("colors",), ARRAYS], ids=lambda w: "+".join(w) or "count")
def test_output_combinations(gpu, want):
    reg, R = wmap("noise97x41")
    px = frame(97, 41)
    _same(_run(gpu, reg, R, px, 4, 2, want=want), windows_model(reg, R, px, 4, 2), keys=("offsets",) + tuple(want))


# 11. More than 2^20 pairs: the second top-level chunk of the scan.
def test_scan_chunks(gpu):
    reg, R = wmap("noise512x300")
    want = windows_model(reg, R, None, 4, 2, lists=False, bbox=True)
    assert want["P"] > 1 << 20 and want["T"] <= want["P"]
    t_off = _guarded(R + 1)
    M = gpu.region_windows_device(to_dev(reg.reshape(-1)), 512, 300, R, t_off)
    a = to_host(t_off)
    assert M == int(want["offsets"][-1]) and np.array_equal(a[:R + 1], want["offsets"]) and (a[R + 1:] == FILL).all()


# 12. A map whose windows span more block rows than they have blocks is refused before anything is written.
def test_a_map_with_too_many_block_rows_is_refused_and_nothing_is_written(gpu):
    reg, R = wmap("refused")
    h, w = reg.shape
    model = windows_model(reg, R, None, 4, 0, lists=False)
    assert (model["P"], model["T"]) == (50, 98)
    t_reg, t_px = to_dev(reg.reshape(-1)), to_dev(frame(w, h))
    t = {k: _guarded(w * h) for k in ARRAYS}
    t["offsets"] = _guarded(R + 1)
    p = lambda v: ctypes.c_void_p(v.data_ptr())   # noqa: E731
    rc = gpu.lib().dq_hip_region_windows_dev(0, p(t_reg), w, h, R, 4, 0, None, None, 0, p(t["offsets"]), w * h,
                                             p(t["coords"]), p(t["index"]), p(t_px), p(t["colors"]), None)
    assert rc == -2
    for k, v in t.items():
        assert (to_host(v) == FILL).all(), k
    with pytest.raises(gpu.RegionRowsError):
        gpu.region_windows_device(t_reg, w, h, R, t["offsets"], block=4, expand=0)
    with pytest.raises(gpu.RegionRowsError):
        gpu.region_windows(reg, block=4, expand=0)
    cts, k_outs = np.full((R, 4), FILL, np.uint32), np.full(R, FILL, np.uint32)
    with pytest.raises(gpu.RegionRowsError):
        gpu.quant_region_windows_device(t_reg, w, h, R, t_px, 4, t["offsets"], block=4, expand=0, capacity=w * h,
                                        t_out=t["index"], cts=cts, k_outs=k_outs)
    assert (to_host(t["index"]) == FILL).all() and (to_host(t["offsets"]) == FILL).all()
    assert (cts == FILL).all() and (k_outs == FILL).all()


# 13. Two streams at once from two threads: the results are each call's own.
def test_two_streams_from_two_threads(gpu):
    import torch
    cases = [("noise96x80", 4, 2), ("noise97x41-permuted", 4, 2)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in cases]
    got, errors = [None] * 2, []

    def work(i):
        try:
            torch.cuda.set_device(0)
            name, d, e = cases[i]
            reg, R = wmap(name)
            for _ in range(3):
                got[i] = _run(gpu, reg, R, frame(reg.shape[1], reg.shape[0]), d, e, stream=streams[i])
        except BaseException as err:   # noqa: B036 (reported by the test's thread)
            errors.append(err)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i, (name, d, e) in enumerate(cases):
        reg, R = wmap(name)
        _same(got[i], windows_model(reg, R, frame(reg.shape[1], reg.shape[0]), d, e))


# 14. The host forms.
@pytest.mark.parametrize("name,kind", [("noise97x41", None), ("islands", "island-window")])
def test_host_form(gpu, name, kind):
    reg, R = wmap(name)
    h, w = reg.shape
    px, mask = frame(w, h), mask_of(kind, h, w)
    area = np.bincount(reg.reshape(-1), minlength=R).astype(np.uint32)
    want = windows_model(reg, R, px, 4, 2, mask, area, 2)
    offsets, index, coords, colours = gpu.region_windows(reg, mask=mask, area=area, min_area=2, pixels=px)
    _same({"M": len(index), "offsets": offsets, "index": index, "coords": coords, "colors": colours}, want)
    offsets, index, coords, colours = gpu.region_windows(reg.astype(np.uint16), num_regions=R + 3, mask=mask)
    want = windows_model(reg, R, px, 4, 2, mask)
    assert colours is None and np.array_equal(index, want["index"]) and np.array_equal(coords, want["coords"])
    assert np.array_equal(offsets[:R + 1], want["offsets"]) and (offsets[R:] == len(index)).all()


# ---------------------------------------------------------------------------
# 15. The pipeline.
def _oracle(px, k):
    px = np.ascontiguousarray(px, np.uint32)
    out, ct, kk = np.zeros(len(px), np.uint32), np.zeros(k, np.uint32), ctypes.c_uint32(k)
    fx.oracle().dqo_quant_recurse_weighted(ctypes.c_uint32(len(px)), fx.vp(px), fx.vp(out), ctypes.byref(kk), fx.vp(ct))
    return out, ct[:kk.value]


def _check_pipeline(gpu, reg, R, px, k, mask, against_regions_call, host_form):
    """quant_region_windows_device against the oracle (and the regions call) window by window."""
    h, w = reg.shape
    want = windows_model(reg, R, px, 4, 2, mask)
    off, M = want["offsets"].astype(np.int64), int(want["offsets"][-1])
    t_reg, t_px = to_dev(reg.reshape(-1)), to_dev(px)
    t_mask = to_dev(mask.reshape(-1), np.uint8) if mask is not None else None
    t_off, t_out, t_colors = _guarded(R + 1), _guarded(M), _guarded(M)
    cts, k_outs = np.full((R, k), FILL, np.uint32), np.full(R, FILL, np.uint32)
    got_cts, got_k, empty = gpu.quant_region_windows_device(t_reg, w, h, R, t_px, k, t_off, t_mask=t_mask, capacity=M,
                                                            t_out=t_out, t_colors=t_colors, cts=cts, k_outs=k_outs)
    assert got_cts is cts and got_k is k_outs and empty >= 0
    a, c, o = to_host(t_out), to_host(t_colors), to_host(t_off)
    assert (a[M:] == FILL).all() and (c[M:] == FILL).all() and (o[R + 1:] == FILL).all()
    assert np.array_equal(o[:R + 1], want["offsets"]) and np.array_equal(c[:M], want["colors"])
    mapped = a[:M]
    for r in range(R):
        mine = want["colors"][off[r]:off[r + 1]]
        if len(mine) == 0:
            assert k_outs[r] == 0 and (cts[r] == FILL).all(), r
            continue
        ref_out, ref_ct = _oracle(mine, k)
        assert k_outs[r] == len(ref_ct) and np.array_equal(cts[r, :k_outs[r]], ref_ct), r
        assert np.array_equal(mapped[off[r]:off[r + 1]], ref_out), r
    if against_regions_call:
        present = [r for r in range(R) if off[r + 1] > off[r]]
        t_ins = [to_dev(want["colors"][off[r]:off[r + 1]]) for r in present]
        t_outs = [_guarded(int(off[r + 1] - off[r])) for r in present]
        ref_cts, _ = gpu.quant_weighted_regions_device(t_ins, t_outs, k)
        for r, ct, t in zip(present, ref_cts, t_outs):
            assert np.array_equal(cts[r, :k_outs[r]], ct), r
            assert np.array_equal(to_host(t)[:-GUARD], mapped[off[r]:off[r + 1]]), r
    # without the mapped colours and without a capacity: the call's own colours, the same tables
    cts2, k2, empty2 = gpu.quant_region_windows_device(t_reg, w, h, R, t_px, k, _guarded(R + 1), t_mask=t_mask)
    assert empty2 == empty and np.array_equal(k2, k_outs)
    for r in range(R):
        assert np.array_equal(cts2[r, :k2[r]], cts[r, :k2[r]]), r
    # the mapped colours asked for without room
    if M > 1:
        t_short = _guarded(M)
        with pytest.raises(gpu.WindowsCapacityError):
            gpu.quant_region_windows_device(t_reg, w, h, R, t_px, k, t_off, t_mask=t_mask, capacity=M - 1, t_out=t_short)
        assert (to_host(t_short) == FILL).all()
    if host_form:
        offsets, out, cts3, k3, empty3 = gpu.quant_region_windows(reg, px, k, num_regions=R, mask=mask)
        assert np.array_equal(offsets, want["offsets"]) and np.array_equal(out, mapped) and empty3 == empty
        assert np.array_equal(k3, k_outs)
        for r in range(R):
            assert np.array_equal(cts3[r, :k3[r]], cts[r, :k3[r]]), r
    return k_outs


def test_pipeline_on_islands_with_an_empty_window(gpu):
    reg, R = wmap("islands")
    px = fx.xorshift(64 * 48, seed=fx.SEED + 41)
    k_outs = _check_pipeline(gpu, reg, R, px, 4, mask_of("island-window", 48, 64), True, True)
    assert k_outs[1] == 0 and (np.delete(k_outs, 1) >= 1).all()


def test_pipeline_on_noise_with_a_mask(gpu):
    reg, R = wmap("noise64x48")
    k_outs = _check_pipeline(gpu, reg, R, frame(64, 48), 4, mask_of("random", 48, 64), True, False)
    assert (k_outs >= 1).all() and (k_outs <= 4).all()


def test_pipeline_with_a_window_above_the_one_launch_limit(gpu):
    reg, R = wmap("big")
    px = frame(512, 300) & np.uint32(0x00F0F0F0)          # (4096 colours at most)
    want = windows_model(reg, R, px, 4, 2, lists=False)
    assert int(np.diff(want["offsets"].astype(np.int64))[0]) == 512 * 300 > 131071
    _check_pipeline(gpu, reg, R, px, 4, None, False, False)
