"""CPU: the argument contract of the pixel-list entry points (include/dq_hip.h,
"pixel lists").  Every check comes before the first HIP call, so a box without
a GPU gets -1: the calls below pass fake non-NULL pointers and never reach the
device.  The Python wrappers refuse bad tensors, lengths and scalars with
ValueError before they call into the library (here the library handle is
replaced by one that fails the test when touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dq_fixtures as fx

FAKE = {name: 0x10000 * (i + 1) for i, name in enumerate(
    ["regions", "offsets", "coords", "index", "pixels", "colors", "values", "frame", "out", "cts", "k_outs"])}

GOOD = dict(regions=FAKE["regions"], width=16, height=8, nregions=5, offsets=FAKE["offsets"], coords=FAKE["coords"],
            index=FAKE["index"], pixels=FAKE["pixels"], colors=FAKE["colors"])
GOOD_SCATTER = dict(values=FAKE["values"], coords=FAKE["coords"], n=128, width=16, frame=FAKE["frame"])
GOOD_MAP = dict(regions=FAKE["regions"], width=16, height=8, nregions=5, pixels=FAKE["pixels"], k=4, out=FAKE["out"],
                cts=FAKE["cts"], k_outs=FAKE["k_outs"], max_iters=10)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _lists(lib, host, **kw):
    a = dict(GOOD, **kw)
    args = (_p(a["regions"]), a["width"], a["height"], a["nregions"], _p(a["offsets"]), _p(a["coords"]),
            _p(a["index"]), _p(a["pixels"]), _p(a["colors"]))
    return lib.dq_hip_region_pixels(*args) if host else lib.dq_hip_region_pixels_dev(0, *args, None)


def _scatter(lib, **kw):
    a = dict(GOOD_SCATTER, **kw)
    return lib.dq_hip_scatter_coords_dev(0, _p(a["values"]), _p(a["coords"]), a["n"], a["width"], _p(a["frame"]), None)


def _map(lib, host, **kw):
    a = dict(GOOD_MAP, **kw)
    args = (_p(a["regions"]), a["width"], a["height"], a["nregions"], _p(a["pixels"]), a["k"], _p(a["out"]),
            _p(a["cts"]), _p(a["k_outs"]), a["max_iters"])
    return lib.dq_hip_quant_region_map(*args) if host else lib.dq_hip_quant_region_map_dev(0, *args, None)


SHAPES = {
    "null_regions": dict(regions=None),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536, height=1),
    "height_65536": dict(width=1, height=65536),
    "pixels_2^31": dict(width=65535, height=32769),      # 2^31 + 32767
    "pixels_65535x65535": dict(width=65535, height=65535),
    "nregions_0": dict(nregions=0),
    "nregions_2^31": dict(nregions=1 << 31),
    "nregions_max_u32": dict(nregions=0xFFFFFFFF),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "regions_odd": dict(regions=FAKE["regions"] + 1),
    "pixels_2mod4": dict(pixels=FAKE["pixels"] + 2),
}

BAD = dict(SHAPES, **{
    "null_offsets": dict(offsets=None),
    "offsets_2mod4": dict(offsets=FAKE["offsets"] + 2),
    "coords_odd": dict(coords=FAKE["coords"] + 1),
    "index_2mod4": dict(index=FAKE["index"] + 2),
    "colors_2mod4": dict(colors=FAKE["colors"] + 2),
    "colors_without_pixels": dict(pixels=None),
    "colors_without_pixels_alone": dict(pixels=None, coords=None, index=None),
})

BAD_SCATTER = {
    "null_values": dict(values=None),
    "null_coords": dict(coords=None),
    "null_frame": dict(frame=None),
    "width_0": dict(width=0),
    "values_2mod4": dict(values=FAKE["values"] + 2),
    "coords_odd": dict(coords=FAKE["coords"] + 1),
    "frame_2mod4": dict(frame=FAKE["frame"] + 2),
    "null_values_n0": dict(values=None, n=0),
}

BAD_MAP = dict(SHAPES, **{
    "null_pixels": dict(pixels=None),
    "null_cts": dict(cts=None),
    "null_k_outs": dict(k_outs=None),
    "k_0": dict(k=0),
    "max_iters_0": dict(max_iters=0),
    "max_iters_negative": dict(max_iters=-3),
    "out_2mod4": dict(out=FAKE["out"] + 2),
})


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_list_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    fn = lib.dq_hip_region_pixels if host else lib.dq_hip_region_pixels_dev
    assert fn.restype is ctypes.c_int64
    assert _lists(lib, host, **BAD[case]) == -1


@pytest.mark.parametrize("case", sorted(BAD_SCATTER))
def test_bad_scatter_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert _scatter(lib, **BAD_SCATTER[case]) == -1


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD_MAP))
def test_bad_pipeline_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    fn = lib.dq_hip_quant_region_map if host else lib.dq_hip_quant_region_map_dev
    assert fn.restype is ctypes.c_int64
    assert _map(lib, host, **BAD_MAP[case]) == -1


def test_the_header_declares_the_entries_and_the_abi_version_stays(pkg):
    text = open(os.path.join(fx.ROOT, "include", "dq_hip.h")).read()
    for name, res in (("dq_hip_region_pixels_dev", "int64_t"), ("dq_hip_region_pixels", "int64_t"),
                      ("dq_hip_scatter_coords_dev", "int"), ("dq_hip_quant_region_map_dev", "int64_t"),
                      ("dq_hip_quant_region_map", "int64_t")):
        assert re.search(r"\b%s\s+%s\s*\(" % (res, name), text), name
        assert hasattr(pkg.lib(), name), name
    assert pkg.lib().dq_hip_abi_version() == 1   # (adding entry points is compatible)
    assert re.search(r"#define\s+DQ_HIP_ABI_VERSION\s+1\b", text)
    assert pkg.PIXELS_MAX_PIXELS == (1 << 31) - 1 and pkg.PIXELS_MAX_REGIONS == (1 << 31) - 1
    assert issubclass(pkg.RegionRowsError, pkg.DivQuantError)


# ---------------------------------------------------------------------------
@pytest.fixture
def no_library(pkg, monkeypatch):
    """The wrappers' own checks: reaching the library fails the test."""
    def touched():
        raise AssertionError("the wrapper called into the library")
    monkeypatch.setattr(pkg, "lib", touched)
    monkeypatch.setattr(pkg, "_require_gpu", touched)
    return pkg


W, H, R, K = 8, 4, 5, 4
N = W * H


def _words(count):
    import torch
    return torch.zeros(count, dtype=torch.int32)


def _good_lists():
    return dict(t_regions=_words(N), width=W, height=H, num_regions=R, t_offsets=_words(R + 1), t_coords=_words(N),
                t_index=_words(N), t_pixels=_words(N), t_colors=_words(N))


def _good_scatter():
    return dict(t_values=_words(N), t_coords=_words(N), n=N, width=W, t_frame=_words(N))


def _good_map():
    return dict(t_regions=_words(N), width=W, height=H, num_regions=R, t_pixels=_words(N), num_clusters=K,
                t_out=_words(N))


def _refused(fn, good, **kw):
    with pytest.raises(ValueError):
        fn(**dict(good(), **kw))


def _strided(count, dtype=None):
    import torch
    t = torch.zeros(2 * count, dtype=dtype or torch.int32)[::2]
    assert not t.is_contiguous() and t.numel() == count
    return t


def _wrong_sizes(count):
    import torch
    return (torch.zeros(count, dtype=torch.uint8), torch.zeros(count, dtype=torch.int16),
            torch.zeros(count, dtype=torch.int64), np.zeros(count, np.uint64))


def test_wrapper_names(pkg):
    for name in ("region_pixels_device", "region_pixels", "scatter_coords_device", "quant_region_map_device",
                 "quant_region_map"):
        assert callable(getattr(pkg, name)), name


LIST_TENSORS = (("t_regions", N), ("t_offsets", R + 1), ("t_coords", N), ("t_index", N), ("t_pixels", N),
                ("t_colors", N))
SCATTER_TENSORS = (("t_values", N), ("t_coords", N), ("t_frame", N))
MAP_TENSORS = (("t_regions", N), ("t_pixels", N), ("t_out", N))


def test_device_wrappers_refuse_non_contiguous_tensors(no_library):
    for fn, good, tensors in ((no_library.region_pixels_device, _good_lists, LIST_TENSORS),
                              (no_library.scatter_coords_device, _good_scatter, SCATTER_TENSORS),
                              (no_library.quant_region_map_device, _good_map, MAP_TENSORS)):
        for name, count in tensors:
            _refused(fn, good, **{name: _strided(count)})
            _refused(fn, good, **{name: np.zeros(2 * count, np.uint32)[::2]})   # (numpy arrays get the same checks)


def test_device_wrappers_refuse_wrong_element_sizes(no_library):
    for fn, good, tensors in ((no_library.region_pixels_device, _good_lists, LIST_TENSORS),
                              (no_library.scatter_coords_device, _good_scatter, SCATTER_TENSORS),
                              (no_library.quant_region_map_device, _good_map, MAP_TENSORS)):
        for name, count in tensors:
            for bad in _wrong_sizes(count):
                _refused(fn, good, **{name: bad})
            _refused(fn, good, **{name: 0x10000})     # a raw pointer has no length


def test_device_wrappers_refuse_short_arrays(no_library):
    for fn, good, tensors in ((no_library.region_pixels_device, _good_lists, LIST_TENSORS),
                              (no_library.quant_region_map_device, _good_map, MAP_TENSORS)):
        for name, count in tensors:
            _refused(fn, good, **{name: _words(count - 1)})
        _refused(fn, good, height=H + 1)              # every map-sized tensor is one row short
        _refused(fn, good, t_regions=None)
    _refused(no_library.region_pixels_device, _good_lists, num_regions=R + 1)    # fewer offsets than ids + 1
    _refused(no_library.region_pixels_device, _good_lists, t_pixels=None)        # colours without the frame
    _refused(no_library.region_pixels_device, _good_lists, t_offsets=None)
    _refused(no_library.quant_region_map_device, _good_map, t_pixels=None)
    for name in ("t_values", "t_coords"):
        _refused(no_library.scatter_coords_device, _good_scatter, **{name: _words(N - 1)})
    _refused(no_library.scatter_coords_device, _good_scatter, t_frame=_words(0))
    _refused(no_library.quant_region_map_device, _good_map, cts=np.zeros((R, K - 1), np.uint32))
    _refused(no_library.quant_region_map_device, _good_map, cts=np.zeros((R, K), np.int64))
    _refused(no_library.quant_region_map_device, _good_map, cts=np.zeros((R, 2 * K), np.uint32)[:, ::2])
    _refused(no_library.quant_region_map_device, _good_map, k_outs=np.zeros(R - 1, np.uint32))
    _refused(no_library.quant_region_map_device, _good_map, k_outs=np.zeros(R, np.uint16))


def test_device_wrappers_refuse_out_of_range_scalars(no_library):
    for fn, good in ((no_library.region_pixels_device, _good_lists), (no_library.quant_region_map_device, _good_map)):
        for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(width=65536, height=1),
                   dict(width=1, height=65536), dict(width=65535, height=65535), dict(num_regions=0),
                   dict(num_regions=-1), dict(num_regions=1 << 31)):
            _refused(fn, good, **kw)
    for kw in (dict(num_clusters=0), dict(num_clusters=-1), dict(num_clusters=1 << 31), dict(max_iters=0),
               dict(max_iters=-1), dict(max_iters=1 << 31)):
        _refused(no_library.quant_region_map_device, _good_map, **kw)
    for kw in (dict(n=-1), dict(n=1 << 32), dict(width=0), dict(width=65536), dict(n=N + 1)):
        _refused(no_library.scatter_coords_device, _good_scatter, **kw)


def test_host_wrappers_refuse_bad_arrays_and_scalars(no_library):
    reg, px = np.zeros((H, W), np.uint32), np.zeros(N, np.uint32)
    for bad in (np.zeros(N, np.uint32), np.zeros((2, H, W), np.uint32), np.zeros((0, W), np.uint32),
                np.zeros((H, W), np.uint64), np.zeros((H, W), np.float32), np.full((H, W), -1, np.int32)):
        with pytest.raises(ValueError):
            no_library.region_pixels(bad)
        with pytest.raises(ValueError):
            no_library.quant_region_map(bad, px, K)
    with pytest.raises(ValueError):   # one pixel short
        no_library.region_pixels(reg, pixels=px[:-1])
    with pytest.raises(ValueError):
        no_library.quant_region_map(reg, px[:-1], K)
    with pytest.raises(ValueError):
        no_library.quant_region_map(reg, None, K)
    with pytest.raises(ValueError):   # an id the count does not cover
        no_library.region_pixels(np.full((H, W), 3, np.uint32), num_regions=3)
    for kw in (dict(num_regions=0), dict(num_regions=1 << 31)):
        with pytest.raises(ValueError):
            no_library.region_pixels(reg, **kw)
    for k, kw in ((0, {}), (-1, {}), (1 << 31, {}), (K, dict(max_iters=0)), (K, dict(num_regions=0)),
                  (K, dict(cts=np.zeros(K - 1, np.uint32))), (K, dict(k_outs=np.zeros(0, np.uint32)))):
        with pytest.raises(ValueError):
            no_library.quant_region_map(reg, px, k, **kw)
