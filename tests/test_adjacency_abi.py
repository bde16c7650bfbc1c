"""CPU: the argument contract of the region-adjacency entry points
(include/dq_hip.h, "region adjacency graph").  Every check comes before the
first HIP call, so a box without a GPU gets -1: the calls below pass fake
non-NULL device pointers and never reach the device.  The Python wrappers
refuse bad tensors and shapes with ValueError before they call into the library
(here the library handle is replaced by one that fails the test when touched).

The largest accepted map, 32768 x 32768 = 2^30 pixels, is checked only on the
wrappers' side (the shape helper stops before any device work); the library has
no entry that stops after the argument check, so its side of that boundary is
covered by the refusals just above it (32769 x 32768, 32768 x 32769)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dq_fixtures as fx

FAKE_REG = 0x10000
FAKE_EDGES = 0x20000
FAKE_BORDER = 0x30000
FAKE_CONTACT = 0x40000
FAKE_PX = 0x50000
FAKE_STEP = 0x60000
FAKE_DEG = 0x70000

GOOD = dict(regions=FAKE_REG, width=16, height=8, connectivity=8, cap=4, edges=FAKE_EDGES, border=None,
            contact=None, pixels=None, step=None, nregions=0, degree=None)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _dev(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.dq_hip_region_adjacency_dev(0, _p(a["regions"]), a["width"], a["height"], a["connectivity"], a["cap"],
                                           _p(a["edges"]), _p(a["border"]), _p(a["contact"]), _p(a["pixels"]),
                                           _p(a["step"]), a["nregions"], _p(a["degree"]), None)


def _host(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.dq_hip_region_adjacency(_p(a["regions"]), a["width"], a["height"], a["connectivity"], a["cap"],
                                       _p(a["edges"]), _p(a["border"]), _p(a["contact"]), _p(a["pixels"]),
                                       _p(a["step"]), a["nregions"], _p(a["degree"]))


BAD = {
    "null_regions": dict(regions=None),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536, height=1),
    "height_65536": dict(width=1, height=65536),
    "pixels_2^30+32768_wide": dict(width=32769, height=32768),     # one column too many
    "pixels_2^30+32768_tall": dict(width=32768, height=32769),     # one row too many
    "pixels_2^30+49151": dict(width=65535, height=16385),
    "pixels_over": dict(width=65535, height=65535),
    "connectivity_0": dict(connectivity=0),
    "connectivity_6": dict(connectivity=6),
    "connectivity_neg": dict(connectivity=-8),
    "regions_2mod4": dict(regions=FAKE_REG + 2),
    "regions_odd": dict(regions=FAKE_REG + 1),
    "edges_2mod4": dict(edges=FAKE_EDGES + 2),
    "border_odd": dict(border=FAKE_BORDER + 1),
    "contact_2mod4": dict(contact=FAKE_CONTACT + 2),
    "pixels_2mod4": dict(pixels=FAKE_PX + 2),
    "degree_2mod4": dict(degree=FAKE_DEG + 2, nregions=8),
    "step_4mod8": dict(pixels=FAKE_PX, step=FAKE_STEP + 4),
    "step_without_pixels": dict(step=FAKE_STEP),
    "step_without_pixels_cap0": dict(cap=0, edges=None, step=FAKE_STEP),
    "cap_without_arrays": dict(edges=None),
    "cap_without_arrays_pixels_only": dict(edges=None, pixels=FAKE_PX),
    "cap_without_arrays_degree_only": dict(edges=None, degree=FAKE_DEG, nregions=8),
    "degree_without_nregions": dict(degree=FAKE_DEG, nregions=0),
    "degree_without_nregions_cap0": dict(cap=0, edges=None, degree=FAKE_DEG),
}


def test_the_over_cases_are_over():
    for case in ("pixels_2^30+32768_wide", "pixels_2^30+32768_tall", "pixels_2^30+49151", "pixels_over"):
        a = dict(GOOD, **BAD[case])
        assert a["width"] <= 65535 and a["height"] <= 65535 and a["width"] * a["height"] > 1 << 30, case


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert lib.dq_hip_region_adjacency_dev.restype is ctypes.c_int64
    assert lib.dq_hip_region_adjacency.restype is ctypes.c_int64
    assert _dev(lib, **BAD[case]) == -1
    assert _host(lib, **BAD[case]) == -1


def test_constants_match_the_header(pkg):
    text = open(os.path.join(fx.ROOT, "include", "dq_hip.h")).read()
    assert int(re.search(r"#define\s+DQ_HIP_ADJACENCY_MAX_PIXELS\s+(0x[0-9A-Fa-f]+)u", text).group(1), 16) \
        == pkg.ADJACENCY_MAX_PIXELS == 1 << 30
    assert pkg.REGION_MAX_SIDE == 65535
    assert pkg.lib().dq_hip_abi_version() == 1   # (adding entry points is compatible)


# ---------------------------------------------------------------------------
@pytest.fixture
def no_library(pkg, monkeypatch):
    """The wrappers' own checks: reaching the library fails the test."""
    def touched():
        raise AssertionError("the wrapper called into the library")
    monkeypatch.setattr(pkg, "lib", touched)
    monkeypatch.setattr(pkg, "_require_gpu", touched)
    return pkg


W, H = 8, 4


def _tensors():
    import torch
    return torch, torch.zeros(W * H, dtype=torch.int32)


def test_wrapper_names(pkg):
    assert callable(pkg.region_adjacency_device) and callable(pkg.region_adjacency)


def test_shape_helper_accepts_2_to_the_30_pixels_and_refuses_more(no_library):
    assert no_library._adjacency_shape(32768, 32768, 8) == (32768, 32768)
    assert no_library._adjacency_shape(65535, 16384, 4) == (65535, 16384)
    for w, h in ((32769, 32768), (32768, 32769), (65535, 16385), (65535, 65535)):
        with pytest.raises(ValueError):
            no_library._adjacency_shape(w, h, 8)


def test_device_wrapper_refuses_non_contiguous_tensors(no_library):
    torch, reg = _tensors()
    strided = torch.zeros(2 * W * H, dtype=torch.int32)[::2]
    assert not strided.is_contiguous() and strided.numel() == W * H
    with pytest.raises(ValueError):
        no_library.region_adjacency_device(strided, W, H)
    with pytest.raises(ValueError):
        no_library.region_adjacency_device(reg, W, H, t_pixels=strided)
    with pytest.raises(ValueError):   # (numpy arrays get the same checks)
        no_library.region_adjacency_device(np.zeros(2 * W * H, np.uint32)[::2], W, H)


def test_device_wrapper_refuses_wrong_element_sizes(no_library):
    torch, reg = _tensors()
    for bad in (torch.zeros(W * H, dtype=torch.uint8), torch.zeros(W * H, dtype=torch.int16),
                torch.zeros(W * H, dtype=torch.int64), torch.zeros(W * H, dtype=torch.float64),
                np.zeros(W * H, np.uint64)):
        with pytest.raises(ValueError):   # the region map is 4-byte
            no_library.region_adjacency_device(bad, W, H)
        with pytest.raises(ValueError):   # and so is the packed frame
            no_library.region_adjacency_device(reg, W, H, t_pixels=bad)


def test_device_wrapper_refuses_length_mismatches(no_library):
    torch, reg = _tensors()
    with pytest.raises(ValueError):   # fewer ids than width * height
        no_library.region_adjacency_device(reg[:-1], W, H)
    with pytest.raises(ValueError):
        no_library.region_adjacency_device(reg, W, H, t_pixels=torch.zeros(W * H - 1, dtype=torch.int32))
    with pytest.raises(ValueError):   # (width * height decides, not the tensor)
        no_library.region_adjacency_device(reg, W, H + 1)


def test_device_wrapper_refuses_bad_shapes_connectivity_and_capacities(no_library):
    torch, reg = _tensors()
    for w, h in ((0, H), (W, 0), (65536, 1), (1, 65536), (32769, 32768)):
        with pytest.raises(ValueError):
            no_library.region_adjacency_device(reg, w, h)
    for connectivity in (0, 6, 16, None):
        with pytest.raises(ValueError):
            no_library.region_adjacency_device(reg, W, H, connectivity=connectivity)
    with pytest.raises(ValueError):
        no_library.region_adjacency_device(reg, W, H, edge_capacity=-1)
    with pytest.raises(ValueError):
        no_library.region_adjacency_device(reg, W, H, edge_capacity=1 << 32)
    with pytest.raises(ValueError):
        no_library.region_adjacency_device(reg, W, H, num_regions=-1)


def test_host_wrapper_refuses_bad_arrays(no_library):
    good = np.zeros((H, W), np.uint32)
    for bad in (np.zeros(W * H, np.uint32), np.zeros((2, H, W), np.uint32), np.zeros((0, W), np.uint32),
                np.zeros((H, W), np.uint64), np.zeros((H, W), np.float32), np.full((H, W), -1, np.int32)):
        with pytest.raises(ValueError):
            no_library.region_adjacency(bad)
    with pytest.raises(ValueError):
        no_library.region_adjacency(good, connectivity=5)
    with pytest.raises(ValueError):   # one pixel short
        no_library.region_adjacency(good, pixels=np.zeros(W * H - 1, np.uint32))
    with pytest.raises(ValueError):   # ids up to 3 need at least 4 degree entries
        no_library.region_adjacency(np.arange(4, dtype=np.uint32).reshape(2, 2), num_regions=3)
    with pytest.raises(ValueError):   # max + 1 does not fit the uint32 count
        no_library.region_adjacency(np.full((H, W), 0xFFFFFFFF, np.uint32))
