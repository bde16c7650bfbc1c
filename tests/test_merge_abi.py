"""CPU: the argument contract of the region-merge entry points
(include/dq_hip.h, "region merge").  Every check comes before the first HIP
call, so a box without a GPU gets -1: the calls below pass fake non-NULL
pointers and never reach the device.  The Python wrappers refuse bad tensors,
lengths and scalars with ValueError before they call into the library (here the
library handle is replaced by one that fails the test when touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dq_fixtures as fx

FAKE = {name: 0x10000 * (i + 1) for i, name in enumerate(
    ["regions", "area", "first", "sums", "bbox", "edges", "out_regions", "remap", "out_area", "out_bbox", "out_first",
     "out_sums", "labels", "pixels"])}

GOOD = dict(regions=FAKE["regions"], n=128, nregions=8, area=FAKE["area"], first=FAKE["first"], sums=FAKE["sums"],
            bbox=None, nedges=4, edges=FAKE["edges"], min_area=10, max_dist=0xFFFFFFFF, max_rounds=0,
            out_regions=FAKE["out_regions"], remap=None, cap=4, out_area=FAKE["out_area"], out_bbox=None,
            out_first=None, out_sums=None)

GOOD_HOST = dict(labels=FAKE["labels"], label_bytes=1, width=16, height=8, connectivity=8, pixels=FAKE["pixels"],
                 min_area=10, max_dist=0xFFFFFFFF, max_rounds=0, regions=FAKE["regions"], cap=4, area=FAKE["area"],
                 bbox=None, first=None, sums=None)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _dev(lib, **kw):
    a = dict(GOOD, **kw)
    rounds = ctypes.c_uint32(0)
    return lib.dq_hip_merge_regions_dev(0, _p(a["regions"]), a["n"], a["nregions"], _p(a["area"]), _p(a["first"]),
                                        _p(a["sums"]), _p(a["bbox"]), a["nedges"], _p(a["edges"]), a["min_area"],
                                        a["max_dist"], a["max_rounds"], _p(a["out_regions"]), _p(a["remap"]), a["cap"],
                                        _p(a["out_area"]), _p(a["out_bbox"]), _p(a["out_first"]), _p(a["out_sums"]),
                                        ctypes.byref(rounds), None)


def _host(lib, **kw):
    a = dict(GOOD_HOST, **kw)
    return lib.dq_hip_segment_labels(_p(a["labels"]), a["label_bytes"], a["width"], a["height"], a["connectivity"],
                                     _p(a["pixels"]), a["min_area"], a["max_dist"], a["max_rounds"], _p(a["regions"]),
                                     a["cap"], _p(a["area"]), _p(a["bbox"]), _p(a["first"]), _p(a["sums"]), None)


BAD = {
    "null_regions": dict(regions=None),
    "null_area": dict(area=None),
    "null_first": dict(first=None),
    "null_sums": dict(sums=None),
    "null_out_regions": dict(out_regions=None),
    "n_0": dict(n=0),
    "n_2^31": dict(n=1 << 31),
    "n_max_u32": dict(n=0xFFFFFFFF),
    "nregions_0": dict(nregions=0),
    "nregions_over_n": dict(nregions=129),
    "edges_null_with_nedges": dict(edges=None),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "area_odd": dict(area=FAKE["area"] + 1),
    "first_2mod4": dict(first=FAKE["first"] + 2),
    "sums_4mod8": dict(sums=FAKE["sums"] + 4),
    "bbox_2mod4": dict(bbox=FAKE["bbox"] + 2),
    "edges_2mod4": dict(edges=FAKE["edges"] + 2),
    "out_regions_odd": dict(out_regions=FAKE["out_regions"] + 1),
    "remap_2mod4": dict(remap=FAKE["remap"] + 2),
    "out_area_2mod4": dict(out_area=FAKE["out_area"] + 2),
    "out_bbox_2mod4": dict(bbox=FAKE["bbox"], out_bbox=FAKE["out_bbox"] + 2),
    "out_first_odd": dict(out_first=FAKE["out_first"] + 1),
    "out_sums_4mod8": dict(out_sums=FAKE["out_sums"] + 4),
    "out_bbox_without_bbox": dict(out_bbox=FAKE["out_bbox"]),
    "out_bbox_without_bbox_cap0": dict(cap=0, out_area=None, out_bbox=FAKE["out_bbox"]),
    "cap_without_arrays": dict(out_area=None),
    "cap_without_arrays_remap_only": dict(out_area=None, remap=FAKE["remap"]),
}

BAD_HOST = {
    "null_pixels": dict(pixels=None),
    "null_labels": dict(labels=None),
    "null_regions": dict(regions=None),
    "label_bytes_3": dict(label_bytes=3),
    "label_bytes_8": dict(label_bytes=8),
    "labels_odd_u16": dict(label_bytes=2, labels=FAKE["labels"] + 1),
    "connectivity_6": dict(connectivity=6),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536, height=1),
    "pixels_2^30+32768": dict(width=32769, height=32768),     # the adjacency stage's limit
    "pixels_2mod4": dict(pixels=FAKE["pixels"] + 2),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "sums_4mod8": dict(sums=FAKE["sums"] + 4),
    "cap_without_arrays": dict(area=None),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert lib.dq_hip_merge_regions_dev.restype is ctypes.c_int64
    assert _dev(lib, **BAD[case]) == -1


@pytest.mark.parametrize("case", sorted(BAD_HOST))
def test_bad_host_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert lib.dq_hip_segment_labels.restype is ctypes.c_int64
    assert _host(lib, **BAD_HOST[case]) == -1


def test_the_header_declares_both_entries_and_the_abi_version_stays(pkg):
    text = open(os.path.join(fx.ROOT, "include", "dq_hip.h")).read()
    for name in ("dq_hip_merge_regions_dev", "dq_hip_segment_labels"):
        assert re.search(r"int64_t\s+%s\s*\(" % name, text), name
        assert hasattr(pkg.lib(), name), name
    assert pkg.lib().dq_hip_abi_version() == 1   # (adding entry points is compatible)
    assert pkg.MERGE_MAX_PIXELS == (1 << 31) - 1 and pkg.NO_DISTANCE_LIMIT == 0xFFFFFFFF


# ---------------------------------------------------------------------------
@pytest.fixture
def no_library(pkg, monkeypatch):
    """The wrappers' own checks: reaching the library fails the test."""
    def touched():
        raise AssertionError("the wrapper called into the library")
    monkeypatch.setattr(pkg, "lib", touched)
    monkeypatch.setattr(pkg, "_require_gpu", touched)
    return pkg


N, R, E = 32, 4, 3


def _good():
    import torch
    return dict(t_regions=torch.zeros(N, dtype=torch.int32), num_regions=R, t_area=torch.ones(R, dtype=torch.int32),
                t_first=torch.zeros(R, dtype=torch.int32), t_sums=torch.zeros((R, 3), dtype=torch.int64),
                t_edges=torch.zeros((E, 2), dtype=torch.int32), min_area=10)


def _refused(pkg, **kw):
    with pytest.raises(ValueError):
        pkg.merge_regions_device(**dict(_good(), **kw))


def test_wrapper_names(pkg):
    assert callable(pkg.merge_regions_device) and callable(pkg.segment_labels)


def test_device_wrapper_refuses_non_contiguous_tensors(no_library):
    import torch
    strided = lambda count, dtype=torch.int32: torch.zeros(2 * count, dtype=dtype)[::2]  # noqa: E731
    assert not strided(N).is_contiguous() and strided(N).numel() == N
    _refused(no_library, t_regions=strided(N))
    _refused(no_library, t_area=strided(R))
    _refused(no_library, t_first=strided(R))
    _refused(no_library, t_sums=strided(3 * R, torch.int64))
    _refused(no_library, t_bbox=strided(4 * R))
    _refused(no_library, t_edges=strided(2 * E))
    _refused(no_library, t_out_regions=strided(N))
    _refused(no_library, t_regions=np.zeros(2 * N, np.uint32)[::2])   # (numpy arrays get the same checks)


def test_device_wrapper_refuses_wrong_element_sizes(no_library):
    import torch
    for name, count in (("t_regions", N), ("t_area", R), ("t_first", R), ("t_bbox", 4 * R), ("t_edges", 2 * E),
                        ("t_out_regions", N)):
        for bad in (torch.zeros(count, dtype=torch.uint8), torch.zeros(count, dtype=torch.int16),
                    torch.zeros(count, dtype=torch.int64), np.zeros(count, np.uint64)):
            _refused(no_library, **{name: bad})
    for bad in (torch.zeros(3 * R, dtype=torch.int32), torch.zeros(6 * R, dtype=torch.int32),
                np.zeros(3 * R, np.uint32)):
        _refused(no_library, t_sums=bad)    # the sums are 8-byte


def test_device_wrapper_refuses_length_mismatches(no_library):
    import torch
    _refused(no_library, n=N + 1)                                     # fewer ids than n
    _refused(no_library, t_out_regions=torch.zeros(N - 1, dtype=torch.int32))
    _refused(no_library, num_regions=R + 1)                           # shorter stats than nregions
    _refused(no_library, t_area=torch.ones(R - 1, dtype=torch.int32))
    _refused(no_library, t_first=torch.zeros(R - 1, dtype=torch.int32))
    _refused(no_library, t_sums=torch.zeros(3 * R - 1, dtype=torch.int64))
    _refused(no_library, t_bbox=torch.zeros(4 * R - 1, dtype=torch.int32))
    _refused(no_library, num_edges=E + 1)                             # fewer pairs than nedges
    _refused(no_library, t_edges=None, num_edges=1)
    _refused(no_library, num_regions=0)
    _refused(no_library, num_regions=N + 1)
    _refused(no_library, n=0)
    _refused(no_library, t_regions=0x10000)                           # a raw pointer has no length


def test_device_wrapper_refuses_negative_and_over_wide_scalars(no_library):
    for name in ("min_area", "max_dist", "max_rounds", "stats_capacity", "num_edges"):
        _refused(no_library, **{name: -1})
        _refused(no_library, **{name: 1 << 32})
    _refused(no_library, n=1 << 31)


def test_host_wrapper_refuses_bad_arrays_and_scalars(no_library):
    W, H = 8, 4
    lab, px = np.zeros((H, W), np.uint8), np.zeros(W * H, np.uint32)
    for bad in (np.zeros(W * H, np.uint8), np.zeros((2, H, W), np.uint8), np.zeros((0, W), np.uint8),
                np.zeros((H, W), np.uint64), np.zeros((H, W), np.float32)):
        with pytest.raises(ValueError):
            no_library.segment_labels(bad, px, 10)
    with pytest.raises(ValueError):
        no_library.segment_labels(lab, None, 10)
    with pytest.raises(ValueError):   # one pixel short
        no_library.segment_labels(lab, px[:-1], 10)
    with pytest.raises(ValueError):
        no_library.segment_labels(lab, px, 10, connectivity=5)
    for kw in (dict(min_area=-1), dict(min_area=1 << 32), dict(min_area=10, max_dist=-1),
               dict(min_area=10, max_dist=1 << 32), dict(min_area=10, max_rounds=-1),
               dict(min_area=10, max_rounds=1 << 32), dict(min_area=10, stats_capacity=0),
               dict(min_area=10, stats_capacity=-1), dict(min_area=10, stats_capacity=1 << 32)):
        with pytest.raises(ValueError):
            no_library.segment_labels(lab, px, **kw)
    with pytest.raises(ValueError):   # more pixels than the adjacency stage takes
        no_library._adjacency_shape(32769, 32768, 8)
