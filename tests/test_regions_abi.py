"""CPU: the argument contract of the connected-region entry points
(include/dq_hip.h, "connected regions").  Every check comes before the first
HIP call, so a box without a GPU gets -1: the calls below pass fake non-NULL
device pointers and never reach the device.  The Python wrappers refuse bad
tensors and shapes with ValueError before they call into the library (here the
library handle is replaced by one that fails the test when touched)."""
import ctypes

import numpy as np
import pytest

FAKE_LAB = 0x10000
FAKE_REG = 0x20000
FAKE_STAT = 0x30000
FAKE_PX = 0x40000
FAKE_SUMS = 0x50000

GOOD = dict(labels=FAKE_LAB, label_bytes=1, width=16, height=8, connectivity=8, regions=FAKE_REG, cap=4,
            area=FAKE_STAT, bbox=None, first=None, label=None, pixels=None, sums=None)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _dev(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.dq_hip_label_regions_dev(0, _p(a["labels"]), a["label_bytes"], a["width"], a["height"],
                                        a["connectivity"], _p(a["regions"]), a["cap"], _p(a["area"]), _p(a["bbox"]),
                                        _p(a["first"]), _p(a["label"]), _p(a["pixels"]), _p(a["sums"]), None)


def _host(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.dq_hip_label_regions(_p(a["labels"]), a["label_bytes"], a["width"], a["height"], a["connectivity"],
                                    _p(a["regions"]), a["cap"], _p(a["area"]), _p(a["bbox"]), _p(a["first"]),
                                    _p(a["label"]), _p(a["pixels"]), _p(a["sums"]))


BAD = {
    "label_bytes_0": dict(label_bytes=0),
    "label_bytes_3": dict(label_bytes=3),
    "label_bytes_8": dict(label_bytes=8),
    "label_bytes_neg": dict(label_bytes=-1),
    "connectivity_0": dict(connectivity=0),
    "connectivity_6": dict(connectivity=6),
    "connectivity_neg": dict(connectivity=-8),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536, height=1),
    "height_65536": dict(width=1, height=65536),
    "pixels_2^31": dict(width=65536 // 2, height=65536),          # 2^31: one too many
    "pixels_over": dict(width=65535, height=65535),
    "null_labels": dict(labels=None),
    "null_regions": dict(regions=None),
    "u16_labels_odd": dict(label_bytes=2, labels=FAKE_LAB + 1),
    "u32_labels_2mod4": dict(label_bytes=4, labels=FAKE_LAB + 2),
    "regions_2mod4": dict(regions=FAKE_REG + 2),
    "regions_odd": dict(regions=FAKE_REG + 1),
    "sums_without_pixels": dict(sums=FAKE_SUMS),
    "sums_without_pixels_cap0": dict(cap=0, area=None, sums=FAKE_SUMS),
    "cap_without_stats": dict(area=None),
    "cap_without_stats_pixels_only": dict(area=None, pixels=FAKE_PX),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert lib.dq_hip_label_regions_dev.restype is ctypes.c_int64
    assert _dev(lib, **BAD[case]) == -1
    assert _host(lib, **BAD[case]) == -1


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
    return torch, torch.zeros(W * H, dtype=torch.uint8), torch.zeros(W * H, dtype=torch.int32)


def test_wrapper_names_and_tile(pkg):
    assert callable(pkg.label_regions_device) and callable(pkg.label_regions)
    assert pkg.REGION_TILE == 64


def test_device_wrapper_refuses_non_contiguous_tensors(no_library):
    torch, lab, reg = _tensors()
    strided8 = torch.zeros(2 * W * H, dtype=torch.uint8)[::2]
    strided32 = torch.zeros(2 * W * H, dtype=torch.int32)[::2]
    assert not strided8.is_contiguous() and strided8.numel() == W * H
    with pytest.raises(ValueError):
        no_library.label_regions_device(strided8, W, H, reg)
    with pytest.raises(ValueError):
        no_library.label_regions_device(lab, W, H, strided32)
    with pytest.raises(ValueError):
        no_library.label_regions_device(lab, W, H, reg, t_pixels=strided32)
    with pytest.raises(ValueError):   # (numpy arrays get the same checks)
        no_library.label_regions_device(np.zeros(2 * W * H, np.uint16)[::2], W, H, reg)


def test_device_wrapper_refuses_wrong_element_sizes(no_library):
    torch, lab, reg = _tensors()
    for bad in (torch.zeros(W * H, dtype=torch.int64), torch.zeros(W * H, dtype=torch.float64),
                np.zeros(W * H, np.uint64)):
        with pytest.raises(ValueError):
            no_library.label_regions_device(bad, W, H, reg)
    for bad in (torch.zeros(W * H, dtype=torch.uint8), torch.zeros(W * H, dtype=torch.int16),
                torch.zeros(W * H, dtype=torch.int64)):
        with pytest.raises(ValueError):   # the region map is 4-byte
            no_library.label_regions_device(lab, W, H, bad)
        with pytest.raises(ValueError):   # and so is the packed frame
            no_library.label_regions_device(lab, W, H, reg, t_pixels=bad)


def test_device_wrapper_refuses_length_mismatches(no_library):
    torch, lab, reg = _tensors()
    with pytest.raises(ValueError):   # fewer labels than width * height
        no_library.label_regions_device(lab[:-1], W, H, reg)
    with pytest.raises(ValueError):
        no_library.label_regions_device(lab, W, H, reg[:-1])
    with pytest.raises(ValueError):
        no_library.label_regions_device(lab, W, H, reg, t_pixels=torch.zeros(W * H - 1, dtype=torch.int32))
    with pytest.raises(ValueError):   # (width * height decides, not the tensor)
        no_library.label_regions_device(lab, W, H + 1, reg)


def test_device_wrapper_refuses_bad_shapes_and_connectivity(no_library):
    torch, lab, reg = _tensors()
    for w, h in ((0, H), (W, 0), (65536, 1), (1, 65536)):
        with pytest.raises(ValueError):
            no_library.label_regions_device(lab, w, h, reg)
    for connectivity in (0, 6, 16, None):
        with pytest.raises(ValueError):
            no_library.label_regions_device(lab, W, H, reg, connectivity=connectivity)


def test_host_wrapper_refuses_bad_arrays(no_library):
    good = np.zeros((H, W), np.uint8)
    for bad in (np.zeros(W * H, np.uint8), np.zeros((2, H, W), np.uint8), np.zeros((0, W), np.uint8),
                np.zeros((H, W), np.uint64), np.zeros((H, W), np.float32)):
        with pytest.raises(ValueError):
            no_library.label_regions(bad)
    with pytest.raises(ValueError):
        no_library.label_regions(good, connectivity=5)
    with pytest.raises(ValueError):   # one pixel short
        no_library.label_regions(good, pixels=np.zeros(W * H - 1, np.uint32))
