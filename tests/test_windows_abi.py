"""CPU: the argument contract of the capture-window entry points (include/dq_hip.h,
"capture windows").  Every check comes before the first HIP call, so a box
without a GPU gets -1: the calls below pass fake non-NULL pointers and never
reach the device.  The Python wrappers refuse bad tensors, lengths and scalars
with ValueError before they call into the library (here the library handle is
replaced by one that fails the test when touched).  The numpy model the GPU
tests compare against is checked here against the pixel lists' model, and every
map the GPU tests run is checked to be one the call takes (T' <= P)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dq_fixtures as fx
from pixels_model import lists_model
from region_inputs import CASES, WINDOWS_FAKE as FAKE, WINDOWS_SHAPES as SHAPES, frame, wmap
from windows_model import dilate_square, window_grids, windows_model

GOOD = dict(regions=FAKE["regions"], width=16, height=8, nregions=5, block=4, expand=2, mask=FAKE["mask"] + 1,
            area=FAKE["area"], min_area=3, offsets=FAKE["offsets"], cap=1000, coords=FAKE["coords"],
            index=FAKE["index"], pixels=FAKE["pixels"], colors=FAKE["colors"])
GOOD_QUANT = dict(GOOD, k=4, out=FAKE["out"], cts=FAKE["cts"], k_outs=FAKE["k_outs"], max_iters=10)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _window_args(a):
    return (_p(a["regions"]), a["width"], a["height"], a["nregions"], a["block"], a["expand"], _p(a["mask"]),
            _p(a["area"]), a["min_area"], _p(a["offsets"]), a["cap"], _p(a["coords"]), _p(a["index"]),
            _p(a["pixels"]), _p(a["colors"]))


def _windows(lib, host, **kw):
    args = _window_args(dict(GOOD, **kw))
    return lib.dq_hip_region_windows(*args) if host else lib.dq_hip_region_windows_dev(0, *args, None)


def _quant(lib, host, **kw):
    a = dict(GOOD_QUANT, **kw)
    args = _window_args(a) + (a["k"], _p(a["out"]), _p(a["cts"]), _p(a["k_outs"]), a["max_iters"])
    return lib.dq_hip_quant_region_windows(*args) if host else lib.dq_hip_quant_region_windows_dev(0, *args, None)


BAD = dict(SHAPES, **{
    "colors_without_pixels": dict(pixels=None),
    "colors_without_pixels_alone": dict(pixels=None, coords=None, index=None),
    "cap_without_a_list": dict(coords=None, index=None, colors=None),
    "cap_1_without_a_list": dict(cap=1, coords=None, index=None, colors=None, pixels=None),
})

BAD_QUANT = dict(SHAPES, **{
    "null_pixels": dict(pixels=None, colors=None),
    "null_cts": dict(cts=None),
    "null_k_outs": dict(k_outs=None),
    "k_0": dict(k=0),
    "k_2^31": dict(k=1 << 31),
    "max_iters_0": dict(max_iters=0),
    "max_iters_negative": dict(max_iters=-3),
    "out_2mod4": dict(out=FAKE["out"] + 2),
    "cap_without_a_list_or_out": dict(coords=None, index=None, colors=None, out=None),
})


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_window_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    fn = lib.dq_hip_region_windows if host else lib.dq_hip_region_windows_dev
    assert fn.restype is ctypes.c_int64
    assert _windows(lib, host, **BAD[case]) == -1


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD_QUANT))
def test_bad_pipeline_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    fn = lib.dq_hip_quant_region_windows if host else lib.dq_hip_quant_region_windows_dev
    assert fn.restype is ctypes.c_int64
    assert _quant(lib, host, **BAD_QUANT[case]) == -1


def test_the_header_declares_the_entries_and_the_abi_version_stays(pkg):
    text = open(os.path.join(fx.ROOT, "include", "dq_hip.h")).read()
    for name in ("dq_hip_region_windows_dev", "dq_hip_region_windows", "dq_hip_quant_region_windows_dev",
                 "dq_hip_quant_region_windows"):
        assert re.search(r"\bint64_t\s+%s\s*\(" % name, text), name
        assert hasattr(pkg.lib(), name), name
    assert text.index("pixel lists") < text.index("capture windows of a region map")
    assert "combinedCoords" in text            # (the subset the reference quantises is named as out of scope)
    assert pkg.lib().dq_hip_abi_version() == 1   # (adding entry points is compatible)
    assert re.search(r"#define\s+DQ_HIP_ABI_VERSION\s+1\b", text)
    assert (pkg.WINDOWS_MAX_BLOCK, pkg.WINDOWS_MAX_EXPAND, pkg.WINDOWS_BLOCK, pkg.WINDOWS_EXPAND) == (8, 3, 4, 2)
    assert pkg.WINDOWS_MAX_ENTRIES == (1 << 32) - 2
    for err in (pkg.RegionRowsError, pkg.WindowsOverflowError, pkg.WindowsCapacityError):
        assert issubclass(err, pkg.DivQuantError)


# ---------------------------------------------------------------------------
# The model.
@pytest.mark.parametrize("name", ["rows65", "comb"])
def test_the_model_at_block_one_expand_zero_is_the_pixel_lists_model(name):
    reg, R = wmap(name)
    px = frame(reg.shape[1], reg.shape[0])
    got, want = windows_model(reg, R, px, 1, 0), lists_model(reg, R, px)
    for k in ("offsets", "index", "coords", "colors"):
        assert np.array_equal(got[k], want[k]), k


def test_every_map_of_the_gpu_tests_is_one_the_call_takes():
    for name, d, e in CASES:
        reg, R = wmap(name)
        model = windows_model(reg, R, None, d, e, lists=False, bbox=True)
        assert 0 < model["T"] <= model["P"], (name, d, e)
    reg, R = wmap("refused")
    model = windows_model(reg, R, None, 4, 0, lists=False)
    assert (model["P"], model["T"]) == (50, 98)


def test_the_model_cut_to_bounding_boxes_is_the_model():
    reg, R = wmap("noise64x48")
    px = frame(64, 48)
    whole, cut = windows_model(reg, R, px, 4, 2), windows_model(reg, R, px, 4, 2, bbox=True)
    for k in ("offsets", "index", "P", "T"):
        assert np.array_equal(whole[k], cut[k]), k


def test_the_cross_and_the_square_differ_on_the_diagonal():
    reg, R = wmap("diagonal")
    cross = {r: g for r, _, _, g in window_grids(reg, R, 4, 1)}
    square = {r: g for r, _, _, g in window_grids(reg, R, 4, 1, dilate=dilate_square)}
    assert not np.array_equal(cross[1], square[1]) and not cross[1][0, 2] and square[1][0, 2]


# ---------------------------------------------------------------------------
@pytest.fixture
def no_library(pkg, monkeypatch):
    """The wrappers' own checks: reaching the library fails the test."""
    def touched():
        raise AssertionError("the wrapper called into the library")
    monkeypatch.setattr(pkg, "lib", touched)
    monkeypatch.setattr(pkg, "_require_gpu", touched)
    return pkg


W, H, R, K, CAP = 8, 4, 5, 4, 100
N = W * H


def _words(count):
    import torch
    return torch.zeros(count, dtype=torch.int32)


def _bytes(count):
    import torch
    return torch.zeros(count, dtype=torch.uint8)


def _good_windows():
    return dict(t_regions=_words(N), width=W, height=H, num_regions=R, t_offsets=_words(R + 1), t_mask=_bytes(N),
                t_area=_words(R), min_area=2, capacity=CAP, t_coords=_words(CAP), t_index=_words(CAP),
                t_pixels=_words(N), t_colors=_words(CAP))


def _good_quant():
    return dict(_good_windows(), num_clusters=K, t_out=_words(CAP))


def _refused(fn, good, **kw):
    with pytest.raises(ValueError):
        fn(**dict(good(), **kw))


def _strided(count, dtype=None):
    import torch
    t = torch.zeros(2 * count, dtype=dtype or torch.int32)[::2]
    assert not t.is_contiguous() and t.numel() == count
    return t


def test_wrapper_names(pkg):
    for name in ("region_windows_device", "region_windows", "quant_region_windows_device", "quant_region_windows"):
        assert callable(getattr(pkg, name)), name


WORD_TENSORS = (("t_regions", N), ("t_offsets", R + 1), ("t_area", R), ("t_coords", CAP), ("t_index", CAP),
                ("t_pixels", N), ("t_colors", CAP))


def _calls(pkg):
    return ((pkg.region_windows_device, _good_windows, WORD_TENSORS),
            (pkg.quant_region_windows_device, _good_quant, WORD_TENSORS + (("t_out", CAP),)))


def test_device_wrappers_refuse_non_contiguous_tensors(no_library):
    import torch
    for fn, good, tensors in _calls(no_library):
        for name, count in tensors:
            _refused(fn, good, **{name: _strided(count)})
            _refused(fn, good, **{name: np.zeros(2 * count, np.uint32)[::2]})   # (numpy arrays get the same checks)
        _refused(fn, good, t_mask=_strided(N, torch.uint8))


def test_device_wrappers_refuse_wrong_element_sizes(no_library):
    import torch
    for fn, good, tensors in _calls(no_library):
        for name, count in tensors:
            for bad in (_bytes(count), torch.zeros(count, dtype=torch.int16), torch.zeros(count, dtype=torch.int64),
                        np.zeros(count, np.uint64)):
                _refused(fn, good, **{name: bad})
            _refused(fn, good, **{name: 0x10000})     # a raw pointer has no length
        for bad in (_words(N), torch.zeros(N, dtype=torch.int16), np.zeros(N, np.uint32)):
            _refused(fn, good, t_mask=bad)


def test_device_wrappers_refuse_short_arrays(no_library):
    for fn, good, tensors in _calls(no_library):
        for name, count in tensors:
            _refused(fn, good, **{name: _words(count - 1)})
        _refused(fn, good, t_mask=_bytes(N - 1))
        _refused(fn, good, height=H + 1)              # every map-sized tensor is one row short
        _refused(fn, good, capacity=CAP + 1)          # every list array is one entry short
        _refused(fn, good, num_regions=R + 1)         # fewer offsets and areas than ids
        _refused(fn, good, t_regions=None)
        _refused(fn, good, t_offsets=None)
    _refused(no_library.region_windows_device, _good_windows, t_pixels=None)        # colours without the frame
    _refused(no_library.region_windows_device, _good_windows, t_coords=None, t_index=None, t_colors=None)
    _refused(no_library.quant_region_windows_device, _good_quant, t_pixels=None)
    _refused(no_library.quant_region_windows_device, _good_quant, t_coords=None, t_index=None, t_colors=None,
             t_out=None)
    _refused(no_library.quant_region_windows_device, _good_quant, cts=np.zeros((R, K - 1), np.uint32))
    _refused(no_library.quant_region_windows_device, _good_quant, cts=np.zeros((R, K), np.int64))
    _refused(no_library.quant_region_windows_device, _good_quant, cts=np.zeros((R, 2 * K), np.uint32)[:, ::2])
    _refused(no_library.quant_region_windows_device, _good_quant, k_outs=np.zeros(R - 1, np.uint32))
    _refused(no_library.quant_region_windows_device, _good_quant, k_outs=np.zeros(R, np.uint16))


def test_device_wrappers_refuse_out_of_range_scalars(no_library):
    for fn, good, _ in _calls(no_library):
        for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(width=65536, height=1),
                   dict(width=1, height=65536), dict(width=65535, height=65535), dict(num_regions=0),
                   dict(num_regions=-1), dict(num_regions=1 << 31), dict(block=0), dict(block=9), dict(block=-1),
                   dict(expand=-1), dict(expand=4), dict(min_area=-1), dict(min_area=1 << 32), dict(capacity=-1),
                   dict(capacity=1 << 32)):
            _refused(fn, good, **kw)
    for kw in (dict(num_clusters=0), dict(num_clusters=-1), dict(num_clusters=1 << 31), dict(max_iters=0),
               dict(max_iters=-1), dict(max_iters=1 << 31)):
        _refused(no_library.quant_region_windows_device, _good_quant, **kw)


def test_host_wrappers_refuse_bad_arrays_and_scalars(no_library):
    reg, px = np.zeros((H, W), np.uint32), np.zeros(N, np.uint32)
    for bad in (np.zeros(N, np.uint32), np.zeros((2, H, W), np.uint32), np.zeros((0, W), np.uint32),
                np.zeros((H, W), np.uint64), np.zeros((H, W), np.float32), np.full((H, W), -1, np.int32)):
        with pytest.raises(ValueError):
            no_library.region_windows(bad)
        with pytest.raises(ValueError):
            no_library.quant_region_windows(bad, px, K)
    for kw in (dict(pixels=px[:-1]), dict(mask=np.zeros(N - 1, np.uint8)), dict(mask=np.zeros(N, np.uint32)),
               dict(area=np.zeros(0, np.uint32)), dict(num_regions=0), dict(num_regions=1 << 31), dict(block=0),
               dict(block=9), dict(expand=4), dict(expand=-1), dict(min_area=-1)):
        with pytest.raises(ValueError):
            no_library.region_windows(reg, **kw)
    with pytest.raises(ValueError):   # an id the count does not cover
        no_library.region_windows(np.full((H, W), 3, np.uint32), num_regions=3)
    with pytest.raises(ValueError):
        no_library.quant_region_windows(reg, px[:-1], K)
    with pytest.raises(ValueError):
        no_library.quant_region_windows(reg, None, K)
    for k, kw in ((0, {}), (-1, {}), (1 << 31, {}), (K, dict(max_iters=0)), (K, dict(num_regions=0)),
                  (K, dict(block=9)), (K, dict(expand=4)), (K, dict(mask=np.zeros(N + 1, np.uint8))),
                  (K, dict(cts=np.zeros(K - 1, np.uint32))), (K, dict(k_outs=np.zeros(0, np.uint32)))):
        with pytest.raises(ValueError):
            no_library.quant_region_windows(reg, px, k, **kw)
