"""CPU: the argument contract of the skeleton entry points (include/dq_hip.h,
"region skeleton").  Every check comes before the first HIP call, so a box
without a GPU gets -1: the calls below pass fake non-NULL pointers and never
reach the device.  The Python wrappers refuse bad tensors, sizes and names with
ValueError before they call into the library (here the library handle is
replaced by one that fails the test when touched)."""
import ctypes

import numpy as np
import pytest

ARRAYS = ("skel", "skeled", "when", "skel_area", "thick")
FAKE = {name: 0x100000 * (i + 1) for i, name in enumerate(("regions",) + ARRAYS)}

GOOD = dict(regions=FAKE["regions"], width=16, height=8, nregions=5, max_iters=0, skel=FAKE["skel"] + 1,
            skeled=FAKE["skeled"], when=FAKE["when"] + 2, skel_area=FAKE["skel_area"], thick=FAKE["thick"])

BAD = {
    "null_regions": dict(regions=None),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536),
    "height_65536": dict(height=65536),
    "2^31_pixels": dict(width=65535, height=32769),   # 2^31 + 32767 pixels
    "nregions_0": dict(nregions=0),
    "max_iters_65536": dict(max_iters=65536),
    "max_iters_2^32-1": dict(max_iters=0xFFFFFFFF),
    "skeled_2mod4": dict(skeled=FAKE["skeled"] + 2),
    "when_odd": dict(when=FAKE["when"] + 1),
    "skel_area_odd": dict(skel_area=FAKE["skel_area"] + 1),
    "thick_2mod4": dict(thick=FAKE["thick"] + 2),
    "every_output_null": dict(skel=None, skeled=None, when=None, skel_area=None, thick=None),
}


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _skeleton(lib, host, words=True, **kw):
    a = dict(GOOD, **kw)
    its, conv = ctypes.c_uint32(77), ctypes.c_uint32(77)
    tail = (ctypes.byref(its), ctypes.byref(conv)) if words else (None, None)
    args = (_p(a["regions"]), a["width"], a["height"], a["nregions"], a["max_iters"]) + \
        tuple(_p(a[k]) for k in ARRAYS) + tail
    r = lib.dq_hip_region_skeleton(*args) if host else lib.dq_hip_region_skeleton_dev(0, *args, None)
    assert its.value == 77 and conv.value == 77   # (a refused call writes nothing)
    return r


def test_exports_and_restypes(lib):
    assert lib.dq_hip_abi_version() == 1
    assert lib.dq_hip_region_skeleton_dev.restype is ctypes.c_int64
    assert lib.dq_hip_region_skeleton.restype is ctypes.c_int64
    assert len(lib.dq_hip_region_skeleton_dev.argtypes) == 14 and len(lib.dq_hip_region_skeleton.argtypes) == 12


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("words", [True, False], ids=["words", "null_words"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_minus_one_before_any_hip_call(lib, case, words, host):
    assert _skeleton(lib, host, words, **BAD[case]) == -1


class _Untouched:
    def __getattr__(self, name):
        pytest.fail("the library was reached: %s" % name)


@pytest.fixture
def no_lib(pkg, monkeypatch):
    monkeypatch.setattr(pkg, "lib", lambda: _Untouched())
    monkeypatch.setattr(pkg, "_require_gpu", lambda: pytest.fail("the device was asked for"))
    return pkg


def test_the_device_wrapper_refuses_before_the_library(no_lib):
    fn = no_lib.region_skeleton_device
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
        fn(reg, 16, 8, 5, max_iters=65536)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, max_iters=-1)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, outputs=("skel", "area"))
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, outputs=())
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, outputs=("skel",), t_skeled=reg)
    with pytest.raises(ValueError):
        fn(reg, 16, 8, 5, t_skeled=reg[:100])


def test_the_host_wrapper_refuses_before_the_library(no_lib):
    fn = no_lib.region_skeleton
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
        fn(np.zeros((4, 4), np.uint32), max_iters=65536)
