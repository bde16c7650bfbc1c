"""CPU: the argument contract of the distance and cores entry points
(include/dq_hip.h, "region distance").  Every check comes before the first HIP
call, so a box without a GPU gets -1: the calls below pass fake non-NULL
pointers and never reach the device.  The Python wrappers refuse bad tensors,
sizes and names with ValueError before they call into the library (here the
library handle is replaced by one that fails the test when touched)."""
import ctypes

import numpy as np
import pytest

FAKE = {name: 0x100000 * (i + 1) for i, name in enumerate(
    ["regions", "dist", "dmax", "bbox", "thresh", "count", "centre", "core", "cored", "core_area"])}

GOOD = dict(regions=FAKE["regions"], width=16, height=8, nregions=5, rule=0, connectivity=8, dist=FAKE["dist"],
            dmax=FAKE["dmax"], bbox=FAKE["bbox"], thresh=FAKE["thresh"], count=FAKE["count"], centre=FAKE["centre"],
            core=FAKE["core"] + 1, cored=FAKE["cored"], core_area=FAKE["core_area"])

SHARED = {
    "null_regions": dict(regions=None),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536),
    "height_65536": dict(height=65536),
    "2^31_pixels": dict(width=65535, height=32769),   # 2^31 + 32767 pixels
    "nregions_0": dict(nregions=0),
    "rule_2": dict(rule=2),
    "rule_minus_1": dict(rule=-1),
    "dist_odd": dict(dist=FAKE["dist"] + 1),
    "centre_2mod4": dict(centre=FAKE["centre"] + 2),
}
BAD_DISTANCE = dict(SHARED, **{
    "dmax_odd": dict(dmax=FAKE["dmax"] + 1),
    "bbox_2mod4": dict(bbox=FAKE["bbox"] + 2),
    "thresh_2mod4": dict(thresh=FAKE["thresh"] + 2),
    "count_odd": dict(count=FAKE["count"] + 3),
    "every_output_null": dict(dist=None, dmax=None, bbox=None, thresh=None, count=None, centre=None),
})
BAD_CORES = dict(SHARED, **{
    "connectivity_6": dict(connectivity=6),
    "connectivity_0": dict(connectivity=0),
    "cored_2mod4": dict(cored=FAKE["cored"] + 2),
    "core_area_odd": dict(core_area=FAKE["core_area"] + 1),
    "every_output_null": dict(core=None, cored=None, centre=None, core_area=None, dist=None),
})


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _distance(lib, host, **kw):
    a = dict(GOOD, **kw)
    args = (_p(a["regions"]), a["width"], a["height"], a["nregions"], a["rule"], _p(a["dist"]), _p(a["dmax"]),
            _p(a["bbox"]), _p(a["thresh"]), _p(a["count"]), _p(a["centre"]))
    return lib.dq_hip_region_distance(*args) if host else lib.dq_hip_region_distance_dev(0, *args, None)


def _cores(lib, host, **kw):
    a = dict(GOOD, **kw)
    args = (_p(a["regions"]), a["width"], a["height"], a["nregions"], a["rule"], a["connectivity"], _p(a["core"]),
            _p(a["cored"]), _p(a["centre"]), _p(a["core_area"]), _p(a["dist"]))
    return lib.dq_hip_region_cores(*args) if host else lib.dq_hip_region_cores_dev(0, *args, None)


def test_exports_and_restypes(lib):
    assert lib.dq_hip_abi_version() == 1
    assert lib.dq_hip_region_distance_dev.restype is ctypes.c_int
    assert lib.dq_hip_region_distance.restype is ctypes.c_int
    assert lib.dq_hip_region_cores_dev.restype is ctypes.c_int64
    assert lib.dq_hip_region_cores.restype is ctypes.c_int64
    assert len(lib.dq_hip_region_distance_dev.argtypes) == 13 and len(lib.dq_hip_region_distance.argtypes) == 11
    assert len(lib.dq_hip_region_cores_dev.argtypes) == 13 and len(lib.dq_hip_region_cores.argtypes) == 11


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD_DISTANCE))
def test_bad_distance_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    assert _distance(lib, host, **BAD_DISTANCE[case]) == -1


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD_CORES))
def test_bad_cores_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    assert _cores(lib, host, **BAD_CORES[case]) == -1


class _Untouched:
    def __getattr__(self, name):
        pytest.fail("the library was reached: %s" % name)


@pytest.fixture
def no_lib(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "lib", lambda: _Untouched())
    monkeypatch.setattr(pkg, "_require_gpu", lambda: pytest.fail("the device was asked for"))
    return pkg


def test_the_device_wrappers_refuse_before_the_library(no_lib):
    pkg = no_lib
    reg = np.zeros(16 * 8, np.uint32)
    for fn in (pkg.region_distance_device, pkg.region_cores_device):
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
            fn(reg, 16, 8, 5, rule=2)
        with pytest.raises(ValueError):
            fn(reg, 16, 8, 5, outputs=("dmax", "area"))
        with pytest.raises(ValueError):
            fn(reg, 16, 8, 5, outputs=())
    with pytest.raises(ValueError):
        pkg.region_cores_device(reg, 16, 8, 5, connectivity=6)
    with pytest.raises(ValueError):
        pkg.region_cores_device(reg, 16, 8, 5, outputs=("core",), t_cored=reg)
    with pytest.raises(ValueError):
        pkg.region_cores_device(reg, 16, 8, 5, t_cored=reg[:100])


def test_the_host_wrappers_refuse_before_the_library(no_lib):
    pkg = no_lib
    for fn in (pkg.region_distance, pkg.region_cores):
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
            fn(np.zeros((4, 4), np.uint32), rule=3)
    with pytest.raises(ValueError):
        pkg.region_cores(np.zeros((4, 4), np.uint32), connectivity=5)
