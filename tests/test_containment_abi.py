"""CPU: the argument contract of the containment entry points
(include/dq_hip.h, "containment tree").  Every check comes before the first
HIP call, so a box without a GPU gets -1: the calls below pass fake non-NULL
pointers and never reach the device.  The Python wrappers refuse bad tensors,
lengths and names with ValueError before they call into the library (here the
library handle is replaced by one that fails the test when touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dq_fixtures as fx

OUTS = ["depth", "parent", "roots", "child_offsets", "children", "subtree", "enclosed", "order", "pos"]
FAKE = {name: 0x10000 * (i + 1) for i, name in enumerate(["regions", "area", "edges", "rank"] + OUTS)}

GOOD = dict(regions=FAKE["regions"], width=16, height=8, nregions=8, area=FAKE["area"], nedges=4, edges=FAKE["edges"],
            **{name: FAKE[name] for name in OUTS})

GOOD_SIZE = dict(nregions=8, area=FAKE["area"], order=FAKE["order"], rank=FAKE["rank"])


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _dev(lib, **kw):
    a = dict(GOOD, **kw)
    levels, reached = ctypes.c_uint32(0), ctypes.c_uint32(0)
    return lib.dq_hip_region_containment_dev(0, _p(a["regions"]), a["width"], a["height"], a["nregions"],
                                             _p(a["area"]), a["nedges"], _p(a["edges"]), *[_p(a[o]) for o in OUTS],
                                             ctypes.byref(levels), ctypes.byref(reached), None)


def _host(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.dq_hip_region_containment(_p(a["regions"]), a["width"], a["height"], a["nregions"], _p(a["area"]),
                                         a["nedges"], _p(a["edges"]), *[_p(a[o]) for o in OUTS], None, None)


def _size(lib, **kw):
    a = dict(GOOD_SIZE, **kw)
    return lib.dq_hip_regions_by_size_dev(0, a["nregions"], _p(a["area"]), _p(a["order"]), _p(a["rank"]), None)


BAD = {
    "null_regions": dict(regions=None),
    "null_area": dict(area=None),
    "edges_null_with_nedges": dict(edges=None),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536),
    "height_65536": dict(height=65536),
    "nregions_0": dict(nregions=0),
    "nregions_over_pixels": dict(nregions=129),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "area_odd": dict(area=FAKE["area"] + 1),
    "edges_2mod4": dict(edges=FAKE["edges"] + 2),
    "enclosed_4mod8": dict(enclosed=FAKE["enclosed"] + 4),
    "children_without_child_offsets": dict(child_offsets=None),
}
BAD.update({"%s_2mod4" % o: {o: FAKE[o] + 2} for o in OUTS})

BAD_SIZE = {
    "null_area": dict(area=None),
    "nregions_0": dict(nregions=0),
    "both_null": dict(order=None, rank=None),
    "area_2mod4": dict(area=FAKE["area"] + 2),
    "order_odd": dict(order=FAKE["order"] + 1),
    "rank_2mod4": dict(rank=FAKE["rank"] + 2),
}


def test_the_three_exports_exist_and_the_header_declares_them(pkg):
    text = open(os.path.join(fx.ROOT, "include", "dq_hip.h")).read()
    for name, ret in (("dq_hip_region_containment_dev", "int64_t"), ("dq_hip_region_containment", "int64_t"),
                      ("dq_hip_regions_by_size_dev", "int")):
        assert re.search(r"%s\s+%s\s*\(" % (ret, name), text), name
        assert hasattr(pkg.lib(), name), name
    assert pkg.lib().dq_hip_abi_version() == 1   # (adding entry points is compatible)
    assert pkg.CONTAINMENT_NONE == 0xFFFFFFFF and list(pkg.CONTAINMENT_OUTPUTS) == OUTS


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert lib.dq_hip_region_containment_dev.restype is ctypes.c_int64
    assert _dev(lib, **BAD[case]) == -1


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_host_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert lib.dq_hip_region_containment.restype is ctypes.c_int64
    assert _host(lib, **BAD[case]) == -1


@pytest.mark.parametrize("case", sorted(BAD_SIZE))
def test_bad_size_order_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert _size(lib, **BAD_SIZE[case]) == -1


# ---------------------------------------------------------------------------
@pytest.fixture
def no_library(pkg, monkeypatch):
    """The wrappers' own checks: reaching the library fails the test."""
    def touched():
        raise AssertionError("the wrapper called into the library")
    monkeypatch.setattr(pkg, "lib", touched)
    monkeypatch.setattr(pkg, "_require_gpu", touched)
    return pkg


W, H, R, E = 8, 4, 4, 3


def _good():
    import torch
    return dict(t_regions=torch.zeros(W * H, dtype=torch.int32), width=W, height=H, num_regions=R,
                t_area=torch.ones(R, dtype=torch.int32), t_edges=torch.zeros((E, 2), dtype=torch.int32))


def _refused(pkg, **kw):
    with pytest.raises(ValueError):
        pkg.region_containment_device(**dict(_good(), **kw))


def test_wrapper_names(pkg):
    assert callable(pkg.region_containment_device) and callable(pkg.region_containment)
    assert callable(pkg.regions_by_size_device)


def test_device_wrapper_refuses_bad_tensors(no_library):
    import torch
    strided = lambda count: torch.zeros(2 * count, dtype=torch.int32)[::2]  # noqa: E731
    _refused(no_library, t_regions=strided(W * H))
    _refused(no_library, t_area=strided(R))
    _refused(no_library, t_edges=strided(2 * E))
    for name, count in (("t_regions", W * H), ("t_area", R), ("t_edges", 2 * E)):
        for bad in (torch.zeros(count, dtype=torch.uint8), torch.zeros(count, dtype=torch.int64),
                    np.zeros(count, np.uint16)):
            _refused(no_library, **{name: bad})
    _refused(no_library, t_regions=0x10000)                           # a raw pointer has no length


def test_device_wrapper_refuses_lengths_shapes_and_names(no_library):
    import torch
    _refused(no_library, t_regions=torch.zeros(W * H - 1, dtype=torch.int32))
    _refused(no_library, t_area=torch.ones(R - 1, dtype=torch.int32))
    _refused(no_library, num_edges=E + 1)
    _refused(no_library, t_edges=None, num_edges=1)
    _refused(no_library, num_edges=-1)
    _refused(no_library, num_edges=1 << 32)
    _refused(no_library, num_regions=0)
    _refused(no_library, num_regions=W * H + 1)
    _refused(no_library, width=0)
    _refused(no_library, height=0)
    _refused(no_library, width=65536)
    _refused(no_library, outputs=("depth", "nothing"))
    _refused(no_library, outputs=("children",))


def test_host_wrapper_refuses_bad_arrays(no_library):
    reg, area, edges = np.zeros((H, W), np.uint8), np.ones(1, np.uint32), None
    for bad in (np.zeros(W * H, np.uint8), np.zeros((0, W), np.uint8), np.zeros((H, W), np.uint64),
                np.zeros((H, W), np.float32), -np.ones((H, W), np.int32)):
        with pytest.raises(ValueError):
            no_library.region_containment(bad, area, edges)
    with pytest.raises(ValueError):
        no_library.region_containment(reg, None, edges)
    with pytest.raises(ValueError):
        no_library.region_containment(reg, np.ones(2, np.uint32), edges)    # one area too many
    with pytest.raises(ValueError):
        no_library.region_containment(reg, area, edges, num_regions=0)
    with pytest.raises(ValueError):
        no_library.region_containment(reg, area, np.zeros(3, np.uint32))     # not pairs
    with pytest.raises(ValueError):
        no_library.region_containment(reg, area, np.array([[0, 1]], np.uint32))   # an id that is none
    with pytest.raises(ValueError):
        no_library.region_containment(reg, area, np.array([[0, 0]], np.uint32))   # a loop


def test_size_order_wrapper_refuses_bad_tensors(no_library):
    import torch
    for bad in (torch.zeros(8, dtype=torch.int32)[::2], torch.zeros(4, dtype=torch.int64), np.zeros(4, np.uint8),
                0x10000, torch.zeros(0, dtype=torch.int32)):
        with pytest.raises(ValueError):
            no_library.regions_by_size_device(bad)
    good = torch.ones(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        no_library.regions_by_size_device(good, num_regions=5)
    with pytest.raises(ValueError):
        no_library.regions_by_size_device(good, num_regions=0)
    with pytest.raises(ValueError):
        no_library.regions_by_size_device(good, want_order=False, want_rank=False)
