"""GPU: the pixel lists of a region map (include/dq_hip.h, "pixel lists"), their
inverse and the region map -> per-region quant -> painted frame pipeline.

The reference is lists_model of pixels_model.py, written against the definition
and using none of the code under test; the maps are pixels_map of
region_inputs.py.  The pipeline is checked
against the CPU oracle's weighted quant_recurse on each region's pixels in
raster order, and against quant_weighted_regions_device on the same lists.
Equality is exact everywhere: array_equal on every array, == on every scalar.
Every output buffer carries guard words behind its last entry.

Shapes are the smallest at which each mechanism can fail: rows shorter than a
wave, chunk boundaries and tails (63, 64, 65, 129 wide), one id many times in
one chunk and in every chunk of a row (stripes), regions that leave and
re-enter rows (comb, rings), one region, one region per pixel, one row, ids
without pixels, a map the call must refuse, and 512 x 300 maps for the
1024-word chunks of the scans (R and T above a hundred thousand) and for a
region too large for the one-launch quant path."""
import ctypes
import functools
import os
import threading

import numpy as np
import pytest

import dq_fixtures as fx
from pixels_model import lists_model, rows_total
from region_dev import body, guarded, same, to_dev, to_host
from region_inputs import frame, pixels_map, with_gaps

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = 0xA5A5A5A5
ARRAYS = ("index", "coords", "colors")
_guarded = functools.partial(guarded, guard=GUARD, fill=FILL)


def _run(gpu, reg, R, pixels, want=ARRAYS, stream=None):
    """region_pixels_device on fresh guarded tensors -> dict of the arrays asked for (and the offsets)."""
    import torch
    h, w = reg.shape
    n = w * h
    t_reg, t_px = to_dev(reg.reshape(-1)), to_dev(pixels)
    t = {"offsets": _guarded(R + 1)}
    t.update({k: _guarded(n) for k in want})
    if stream is not None:   # (the tensors above were filled on the current stream)
        stream.wait_stream(torch.cuda.current_stream())
    gpu.region_pixels_device(t_reg, w, h, R, t["offsets"], t_coords=t.get("coords"), t_index=t.get("index"),
                             t_pixels=t_px if "colors" in want else None, t_colors=t.get("colors"), stream=stream)
    out = {}
    for k, v in t.items():
        out[k] = body(v, R + 1 if k == "offsets" else n, GUARD, FILL, k)
    return out


def _same(got, want, keys=("offsets",) + ARRAYS):
    assert sorted(got) == sorted(keys)
    same(got, want, keys)


def _check(gpu, name):
    reg, R = pixels_map(name)
    px = frame(reg.shape[1], reg.shape[0])
    _same(_run(gpu, reg, R, px), lists_model(reg, R, px))


# ---------------------------------------------------------------------------
# 1. Region maps of noise labels, and the same with permuted ids.
@pytest.mark.parametrize("name", ["noise64x48", "noise96x80", "noise97x41", "noise64x48-permuted",
                                  "noise96x80-permuted", "noise97x41-permuted"])
def test_noise_region_maps(gpu, name):
    _check(gpu, name)


# 2. Row widths around the wave.
@pytest.mark.parametrize("name", ["rows1x7", "rows3x5", "rows63", "rows64", "rows65", "rows129"])
def test_row_widths_around_the_wave(gpu, name):
    _check(gpu, name)


# 3. Runs and cursors.
@pytest.mark.parametrize("name", ["stripes", "comb", "rings"])
def test_one_id_many_times_in_a_row(gpu, name):
    _check(gpu, name)


# 4. Extremes of R.
@pytest.mark.parametrize("name", ["one", "each", "line", "column"])
def test_extremes_of_the_region_count(gpu, name):
    reg, R = pixels_map(name)
    assert name != "each" or R == reg.size
    _check(gpu, name)


# 5. Ids without a pixel.
@pytest.mark.parametrize("gaps", [(3, 0, 0), (0, 2, 0), (0, 0, 5), (2, 1, 1030)], ids=str)
def test_ids_without_pixels_have_empty_ranges(gpu, gaps):
    base, _ = pixels_map("noise64x48")
    reg, R = with_gaps(base, *gaps)
    px = frame(64, 48)
    want = lists_model(reg, R, px)
    got = _run(gpu, reg, R, px)
    _same(got, want)
    present = np.zeros(R, bool)
    present[reg.reshape(-1)] = True
    assert (~present).sum() >= sum(gaps[::2]) and got["offsets"][R] == reg.size
    assert (np.diff(got["offsets"].astype(np.int64))[~present] == 0).all()


# 6. A map whose ids span more rows than it has pixels is refused before anything is written.
def test_a_map_with_too_many_rows_is_refused_and_nothing_is_written(gpu):
    w, h, R = 4, 64, 5
    reg = np.full((h, w), 4, np.uint32)
    reg[0] = reg[63] = np.arange(4)
    assert rows_total(reg) == 4 * 64 + 62 == 318 > w * h
    t_reg, t_px = to_dev(reg.reshape(-1)), to_dev(frame(w, h))
    t = {k: _guarded(w * h) for k in ARRAYS}
    t["offsets"] = _guarded(R + 1)
    rc = gpu.lib().dq_hip_region_pixels_dev(0, ctypes.c_void_p(t_reg.data_ptr()), w, h, R,
                                            ctypes.c_void_p(t["offsets"].data_ptr()),
                                            ctypes.c_void_p(t["coords"].data_ptr()),
                                            ctypes.c_void_p(t["index"].data_ptr()), ctypes.c_void_p(t_px.data_ptr()),
                                            ctypes.c_void_p(t["colors"].data_ptr()), None)
    assert rc == -2
    for k, v in t.items():
        assert (to_host(v) == FILL).all(), k
    with pytest.raises(gpu.RegionRowsError):
        gpu.region_pixels_device(t_reg, w, h, R, t["offsets"])
    with pytest.raises(gpu.RegionRowsError):
        gpu.region_pixels(reg)
    cts, k_outs = np.full((R, 4), FILL, np.uint32), np.full(R, FILL, np.uint32)
    with pytest.raises(gpu.RegionRowsError):
        gpu.quant_region_map_device(t_reg, w, h, R, t_px, 4, t_out=t["index"], cts=cts, k_outs=k_outs)
    assert (to_host(t["index"]) == FILL).all() and (cts == FILL).all() and (k_outs == FILL).all()


# 7. The 1024-word chunks of both scans.
def test_scan_chunk_boundaries(gpu):
    reg, R = pixels_map("noise512x300")
    assert R > 100000 and rows_total(reg) > 100000
    _check(gpu, "noise512x300")


# 8. Each output pointer alone, the offsets only, all together.
@pytest.mark.parametrize("want", [(), ("index",), ("coords",), ("colors",), ARRAYS], ids=lambda w: "+".join(w) or "offsets")
def test_output_pointers(gpu, want):
    reg, R = pixels_map("noise97x41")
    px = frame(97, 41)
    _same(_run(gpu, reg, R, px, want=want), lists_model(reg, R, px), keys=("offsets",) + tuple(want))


def test_host_form(gpu):
    reg, R = pixels_map("noise97x41")
    px = frame(97, 41)
    want = lists_model(reg, R, px)
    offsets, index, coords, colours = gpu.region_pixels(reg, pixels=px)
    _same({"offsets": offsets, "index": index, "coords": coords, "colors": colours}, want)
    offsets, index, coords, colours = gpu.region_pixels(reg.astype(np.uint16), num_regions=R + 3)
    assert colours is None and np.array_equal(index, want["index"]) and np.array_equal(coords, want["coords"])
    assert np.array_equal(offsets[:R + 1], want["offsets"]) and (offsets[R:] == reg.size).all()


# 9. Two streams at once from two threads: the results are each call's own.
def test_two_streams_from_two_threads(gpu):
    import torch
    names = ["noise96x80", "noise97x41-permuted"]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in names]
    got, errors = [None] * 2, []

    def work(i):
        try:
            torch.cuda.set_device(0)
            reg, R = pixels_map(names[i])
            for _ in range(3):
                got[i] = _run(gpu, reg, R, frame(reg.shape[1], reg.shape[0]), stream=streams[i])
        except BaseException as e:   # noqa: B036 (reported by the test's thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i, name in enumerate(names):
        reg, R = pixels_map(name)
        _same(got[i], lists_model(reg, R, frame(reg.shape[1], reg.shape[0])))


# 10. The inverse.
def test_scatter_of_a_gather_is_the_identity(gpu):
    import torch
    reg, R = pixels_map("noise97x41")
    px = frame(97, 41)
    n = reg.size
    got = _run(gpu, reg, R, px)
    t_frame = _guarded(n)
    gpu.scatter_coords_device(to_dev(got["colors"]), to_dev(got["coords"]), n, 97, t_frame)
    torch.cuda.synchronize()
    a = to_host(t_frame)
    assert np.array_equal(a[:n], px) and (a[n:] == FILL).all()


def test_scatter_matches_fancy_assignment(gpu):
    import torch
    w, h = 97, 41
    m = 1000                                    # distinct pixels, in no order
    p = np.argsort(fx.xorshift(w * h, seed=fx.SEED + 21), kind="stable")[:m]
    values = fx.xorshift(m, seed=fx.SEED + 22)
    coords = ((p % w) | (p // w) << 16).astype(np.uint32)
    want = np.full(w * h, FILL, np.uint32)
    want[p] = values
    t_frame = _guarded(w * h)
    gpu.scatter_coords_device(to_dev(values), to_dev(coords), m, w, t_frame)
    gpu.scatter_coords_device(to_dev(values), to_dev(coords), 0, w, t_frame)   # (n = 0: nothing)
    torch.cuda.synchronize()
    a = to_host(t_frame)
    assert np.array_equal(a[:w * h], want) and (a[w * h:] == FILL).all()


# ---------------------------------------------------------------------------
# 11. The pipeline.
def _oracle(px, k):
    px = np.ascontiguousarray(px, np.uint32)
    out, ct, kk = np.zeros(len(px), np.uint32), np.zeros(k, np.uint32), ctypes.c_uint32(k)
    fx.oracle().dqo_quant_recurse_weighted(ctypes.c_uint32(len(px)), fx.vp(px), fx.vp(out), ctypes.byref(kk), fx.vp(ct))
    return out, ct[:kk.value]


def _check_pipeline(gpu, reg, R, px, k, against_regions_call):
    """quant_region_map_device against the oracle (and the regions call) region by region."""
    h, w = reg.shape
    n = w * h
    lists = lists_model(reg, R, px)
    off, order = lists["offsets"].astype(np.int64), lists["index"].astype(np.int64)
    t_out = _guarded(n)
    cts, k_outs = np.full((R, k), FILL, np.uint32), np.full(R, FILL, np.uint32)
    got_cts, got_k, empty = gpu.quant_region_map_device(to_dev(reg.reshape(-1)), w, h, R, to_dev(px), k, t_out=t_out,
                                                        cts=cts, k_outs=k_outs)
    assert got_cts is cts and got_k is k_outs and empty >= 0
    a = to_host(t_out)
    assert (a[n:] == FILL).all()
    painted, want_painted = a[:n], np.zeros(n, np.uint32)
    for r in range(R):
        mine = order[off[r]:off[r + 1]]
        if len(mine) == 0:
            assert k_outs[r] == 0 and (cts[r] == FILL).all(), r
            continue
        ref_out, ref_ct = _oracle(px[mine], k)
        assert k_outs[r] == len(ref_ct) and np.array_equal(cts[r, :k_outs[r]], ref_ct), r
        want_painted[mine] = ref_out
    assert np.array_equal(painted, want_painted)
    if against_regions_call:
        present = [r for r in range(R) if off[r + 1] > off[r]]
        t_ins = [to_dev(lists["colors"][off[r]:off[r + 1]]) for r in present]
        t_outs = [_guarded(int(off[r + 1] - off[r])) for r in present]
        ref_cts, _ = gpu.quant_weighted_regions_device(t_ins, t_outs, k)
        for r, ct, t in zip(present, ref_cts, t_outs):
            assert np.array_equal(cts[r, :k_outs[r]], ct), r
            assert np.array_equal(to_host(t)[:-GUARD], painted[order[off[r]:off[r + 1]]]), r
    # the host form and a call without a frame to paint give the same tables
    out2d, cts2, k2, empty2 = gpu.quant_region_map(reg, px, k, num_regions=R)
    assert np.array_equal(out2d.reshape(-1), painted) and empty2 == empty
    cts3, k3, _ = gpu.quant_region_map_device(to_dev(reg.reshape(-1)), w, h, R, to_dev(px), k)
    for r in range(R):
        assert k2[r] == k_outs[r] == k3[r]
        assert np.array_equal(cts2[r, :k2[r]], cts[r, :k2[r]]) and np.array_equal(cts3[r, :k2[r]], cts[r, :k2[r]])
    return k_outs


def test_pipeline_on_a_crop_of_batman(gpu):
    img, w, h = fx.load_png_u32(os.path.join(fx.GOLDEN, "png", "batman.png"))
    x0, y0, cw, ch = 1024, 928, 96, 64           # the 96 x 64 crop with the most distinct colours (edges, gradients)
    px = np.ascontiguousarray(img.reshape(h, w)[y0:y0 + ch, x0:x0 + cw]).reshape(-1)
    assert len(np.unique(px)) > 1000
    labels, ct = gpu.quant_labels(px, 8)
    reg, stats, _ = gpu.segment_labels(labels.reshape(ch, cw), px, 10)
    R = len(stats["area"])
    assert R > 1 and int(reg.max()) == R - 1
    k_outs = _check_pipeline(gpu, reg, R, px, 4, against_regions_call=True)
    assert (k_outs >= 1).all() and (k_outs <= 4).all()


def test_pipeline_with_a_region_above_the_one_launch_limit(gpu):
    reg, R = pixels_map("big")
    px = frame(512, 300).copy()
    px[reg.reshape(-1) == 0] &= np.uint32(0x00F0F0F0)     # (the background: 4096 colours at most)
    _check_pipeline(gpu, reg, R, px, 4, against_regions_call=False)


def test_pipeline_with_ids_without_pixels(gpu):
    base, _ = pixels_map("noise64x48")
    reg, R = with_gaps(base, 2, 1, 7)
    k_outs = _check_pipeline(gpu, reg, R, frame(64, 48), 4, against_regions_call=False)
    present = np.zeros(R, bool)
    present[reg.reshape(-1)] = True
    assert (k_outs[~present] == 0).all() and (k_outs[present] >= 1).all() and (~present).sum() > 9
