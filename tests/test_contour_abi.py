"""CPU: the argument contract of the contour entry points (include/dq_hip.h,
"region contours").  Every check comes before the first HIP call, so a box
without a GPU gets -1: the calls below pass fake non-NULL pointers and never
reach the device.  The Python wrappers refuse bad tensors, sizes and names with
ValueError before they call into the library (here the library handle is
replaced by one that fails the test when touched)."""
import ctypes

import numpy as np
import pytest

ARRAYS = ("offsets", "points", "codes", "len", "visits")
FAKE = {name: 0x100000 * (i + 1) for i, name in enumerate(("regions",) + ARRAYS)}

GOOD = dict(regions=FAKE["regions"], width=16, height=8, nregions=5, orientation=1, point_cap=100,
            offsets=FAKE["offsets"], points=FAKE["points"], codes=FAKE["codes"] + 1, len=FAKE["len"],
            visits=FAKE["visits"] + 3)

BAD = {
    "null_regions": dict(regions=None),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536),
    "height_65536": dict(height=65536),
    "2^31_pixels": dict(width=65535, height=32769),   # 2^31 + 32767 pixels
    "nregions_0": dict(nregions=0),
    "nregions_max_u32": dict(nregions=0xFFFFFFFF),
    "orientation_2": dict(orientation=2),
    "orientation_minus_1": dict(orientation=-1),
    "offsets_2mod4": dict(offsets=FAKE["offsets"] + 2),
    "points_odd": dict(points=FAKE["points"] + 1),
    "len_2mod4": dict(len=FAKE["len"] + 2),
    "every_output_null": dict(offsets=None, points=None, codes=None, len=None, visits=None, point_cap=0),
    "cap_without_a_list": dict(points=None, codes=None),
    "cap_2^40_without_a_list": dict(points=None, codes=None, point_cap=1 << 40),
}


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _contours(lib, host, **kw):
    a = dict(GOOD, **kw)
    args = (_p(a["regions"]), a["width"], a["height"], a["nregions"], a["orientation"], a["point_cap"]) + \
        tuple(_p(a[k]) for k in ARRAYS)
    return lib.dq_hip_region_contours(*args) if host else lib.dq_hip_region_contours_dev(0, *args, None)


def test_exports_and_restypes(lib):
    assert lib.dq_hip_abi_version() == 1
    assert lib.dq_hip_region_contours_dev.restype is ctypes.c_int64
    assert lib.dq_hip_region_contours.restype is ctypes.c_int64
    assert len(lib.dq_hip_region_contours_dev.argtypes) == 13 and len(lib.dq_hip_region_contours.argtypes) == 11
    assert lib.dq_hip_region_contours_dev.argtypes[6] is ctypes.c_uint64   # point_cap


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    assert _contours(lib, host, **BAD[case]) == -1


class _Untouched:
    def __getattr__(self, name):
        pytest.fail("the library was reached: %s" % name)


@pytest.fixture
def no_lib(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "lib", lambda: _Untouched())
    monkeypatch.setattr(pkg, "_require_gpu", lambda: pytest.fail("the device was asked for"))
    return pkg


def test_the_device_wrapper_refuses_before_the_library(no_lib):
    fn = no_lib.region_contours_device
    reg = np.zeros(16 * 8, np.uint32)
    with pytest.raises(ValueError):
        fn(reg, 0, 8, 5)
    with pytest.raises(ValueError):
        fn(reg, 16, 65536, 5)
    with pytest.raises(ValueError):
        fn(reg, 16, 9, 5)                      # too short for 16 x 9
    with pytest.raises(ValueError):
        fn(reg.astype(np.uint16), 16, 8, 5)    # 2-byte elements
    with pytest.raises(ValueError):
        fn(reg.reshape(8, 16)[:, ::2], 8, 8, 5)   # not contiguous
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 0)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 0xFFFFFFFF)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, orientation=2)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, outputs=("points", "area"))
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, outputs=())
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, point_capacity=-1)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, point_capacity=1 << 64)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, outputs=("len", "visits"), point_capacity=10)


def test_the_host_wrapper_refuses_before_the_library(no_lib):
    fn = no_lib.region_contours
    with pytest.raises(ValueError):
        fn(np.zeros(10, np.uint32))
    with pytest.raises(ValueError):
        fn(np.zeros((0, 4), np.uint32))
    with pytest.raises(ValueError):
        fn(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        fn(np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError):
        fn(np.full((4, 4), -1, np.int32))
    with pytest.raises(ValueError):
        fn(np.zeros((4, 4), np.uint32), num_regions=0)
    with pytest.raises(ValueError):
        fn(np.zeros((4, 4), np.uint32), orientation=3)
