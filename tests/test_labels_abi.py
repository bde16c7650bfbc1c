"""CPU: the argument contract of the label entry points (include/dq_hip.h,
"cluster labels").  Every check comes before the first HIP call, so a box
without a GPU gets the negative code: the calls below pass fake non-NULL
device pointers and never reach the device.  The Python wrappers refuse a bad
label tensor with ValueError before they call into the library (here the
library handle is replaced by one that fails the test when touched)."""
import ctypes

import numpy as np
import pytest

FAKE_IN = ctypes.c_void_p(0x10000)
FAKE_LAB = ctypes.c_void_p(0x20000)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _ct(k):
    return np.zeros(max(k, 1), np.uint32)


def _map_labels(lib, d_in, n, d_lab, width, ct, k):
    return lib.dq_hip_map_labels_dev(0, d_in, n, d_lab, width, None if ct is None else ct.ctypes.data, k, None)


@pytest.mark.parametrize("width", [0, 3, 8, -1])
def test_map_labels_refuses_other_widths(lib, width):
    assert _map_labels(lib, FAKE_IN, 16, FAKE_LAB, width, _ct(4), 4) == -1


@pytest.mark.parametrize("width,k", [(1, 257), (2, 65537), (1, 16384)])
def test_map_labels_refuses_a_width_that_cannot_hold_k(lib, width, k):
    assert _map_labels(lib, FAKE_IN, 16, FAKE_LAB, width, _ct(k), k) == -1
    # (n = 0 does not excuse it: the width is checked first)
    assert _map_labels(lib, FAKE_IN, 0, FAKE_LAB, width, _ct(k), k) == -1


@pytest.mark.parametrize("k", [0, -1])
def test_map_labels_refuses_k_below_one(lib, k):
    for width in (1, 2, 4):
        assert _map_labels(lib, FAKE_IN, 16, FAKE_LAB, width, _ct(4), k) == -1


def test_map_labels_refuses_null_pointers(lib):
    ct = _ct(4)
    assert _map_labels(lib, None, 16, FAKE_LAB, 1, ct, 4) == -1
    assert _map_labels(lib, FAKE_IN, 16, None, 1, ct, 4) == -1
    assert _map_labels(lib, FAKE_IN, 16, FAKE_LAB, 1, None, 4) == -1


def test_map_labels_refuses_unaligned_wide_labels(lib):
    """u16 / u32 labels need their natural alignment (u8: any address)."""
    ct = _ct(4)
    assert _map_labels(lib, FAKE_IN, 16, ctypes.c_void_p(0x20001), 2, ct, 4) == -1
    assert _map_labels(lib, FAKE_IN, 16, ctypes.c_void_p(0x20002), 4, ct, 4) == -1
    assert _map_labels(lib, FAKE_IN, 0, ctypes.c_void_p(0x20001), 1, ct, 4) == 0


@pytest.mark.parametrize("width,k", [(1, 1), (1, 256), (2, 257), (2, 16384), (4, 16384)])
def test_map_labels_of_no_pixels_is_done(lib, width, k):
    """n = 0 with good arguments: 0, nothing to do (the widest legal K per width)."""
    assert _map_labels(lib, FAKE_IN, 0, FAKE_LAB, width, _ct(k), k) == 0


def _quant_labels_batch(lib, width, k, nframes=2, d_in=True, d_lab=True, uniq=1, max_iters=10):
    ins = (ctypes.c_void_p * 2)(FAKE_IN.value if d_in else None, FAKE_IN.value + 4096)
    labs = (ctypes.c_void_p * 2)(FAKE_LAB.value, FAKE_LAB.value + 4096 if d_lab else None)
    ns = np.array([64, 32], np.uint32)
    ct = np.zeros(2 * max(k, 1), np.uint32)
    kout = np.zeros(2, np.uint32)
    return lib.dq_hip_quant_labels_batch_dev(0, nframes, ctypes.cast(ins, ctypes.c_void_p), ns.ctypes.data,
                                             ctypes.cast(labs, ctypes.c_void_p), width, k, ct.ctypes.data,
                                             kout.ctypes.data, uniq, max_iters, None)


@pytest.mark.parametrize("uniq", [1, 0])
@pytest.mark.parametrize("width,k", [(0, 4), (3, 4), (8, 4), (1, 257), (2, 65537)])
def test_quant_labels_batch_refuses_width_and_k_mismatches(lib, width, k, uniq):
    """The requested K decides, before any work."""
    assert _quant_labels_batch(lib, width, k, uniq=uniq) == -1


def test_quant_labels_batch_refuses_bad_arguments(lib):
    assert _quant_labels_batch(lib, 1, 0) == -1
    assert _quant_labels_batch(lib, 1, 4, nframes=0) == -1
    assert _quant_labels_batch(lib, 1, 4, d_in=False) == -1
    assert _quant_labels_batch(lib, 1, 4, d_lab=False) == -1
    assert _quant_labels_batch(lib, 1, 4, max_iters=0) == -1


def test_quant_labels_host_refuses_bad_arguments(lib):
    px = np.zeros(16, np.uint32)
    lab = np.zeros(16, np.uint32)
    ct = np.zeros(300, np.uint32)

    def call(in_, n, labels, width, k):
        kk = ctypes.c_uint32(k)
        return lib.dq_hip_quant_labels(None if in_ is None else in_.ctypes.data, n,
                                       None if labels is None else labels.ctypes.data, width, ctypes.byref(kk),
                                       ct.ctypes.data, 1)

    assert call(px, 16, lab, 3, 4) == -1
    assert call(px, 16, lab, 1, 257) == -1
    assert call(px, 16, lab, 1, 0) == -1
    assert call(px, 0, lab, 1, 4) == -1
    assert call(None, 16, lab, 1, 4) == -1
    assert call(px, 16, None, 1, 4) == -1


# ---------------------------------------------------------------------------
@pytest.fixture
def no_library(pkg, monkeypatch):
    """The wrappers' own checks: reaching the library fails the test."""
    def touched():
        raise AssertionError("the wrapper called into the library")
    monkeypatch.setattr(pkg, "lib", touched)
    return pkg


def _tensors():
    import torch
    t_in = torch.zeros(16, dtype=torch.int32)
    return torch, t_in


def test_wrappers_refuse_a_non_contiguous_label_tensor(no_library):
    torch, t_in = _tensors()
    strided = torch.zeros(32, dtype=torch.uint8)[::2]
    assert not strided.is_contiguous() and strided.numel() == 16
    with pytest.raises(ValueError):
        no_library.map_labels_device(t_in, strided, np.arange(4, dtype=np.uint32))
    with pytest.raises(ValueError):
        no_library.quant_labels_batch_device([t_in], [strided], 4)
    with pytest.raises(ValueError):   # (numpy arrays get the same checks)
        no_library.map_labels_device(t_in, np.zeros(32, np.uint16)[::2], np.arange(4, dtype=np.uint32))


def test_wrappers_refuse_a_wrong_element_size(no_library):
    torch, t_in = _tensors()
    for bad in (torch.zeros(16, dtype=torch.int64), torch.zeros(16, dtype=torch.float64),
                np.zeros(16, np.uint64)):
        with pytest.raises(ValueError):
            no_library.map_labels_device(t_in, bad, np.arange(4, dtype=np.uint32))
        with pytest.raises(ValueError):
            no_library.quant_labels_batch_device([t_in], [bad], 4)
    with pytest.raises(ValueError):   # one width per batch
        no_library.quant_labels_batch_device([t_in, t_in], [torch.zeros(16, dtype=torch.uint8),
                                                            torch.zeros(16, dtype=torch.int16)], 4)
    with pytest.raises(ValueError):
        no_library.quant_labels(np.zeros(16, np.uint32), 4, dtype=np.float32)
    with pytest.raises(ValueError):
        no_library.quant_labels(np.zeros(16, np.uint32), 4, dtype=np.uint64)


def test_wrappers_refuse_length_mismatches(no_library):
    torch, t_in = _tensors()
    lab = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError):   # two frames, one label tensor
        no_library.quant_labels_batch_device([t_in, t_in], [lab], 4)
    with pytest.raises(ValueError):   # fewer labels than pixels
        no_library.quant_labels_batch_device([t_in], [torch.zeros(15, dtype=torch.uint8)], 4)
    with pytest.raises(ValueError):
        no_library.map_labels_device(t_in, torch.zeros(15, dtype=torch.int16), np.arange(4, dtype=np.uint32))
    with pytest.raises(ValueError):   # (n given: it decides)
        no_library.map_labels_device(t_in, lab, np.arange(4, dtype=np.uint32), n=17)
