"""CPU: the argument contract of the window-tag entry points (include/dq_hip.h,
"window tags").  Every check comes before the first HIP call, so a box without
a GPU gets -1: the calls below pass fake non-NULL pointers and never reach the
device.  The Python wrappers refuse bad tensors, lengths and scalars with
ValueError before they call into the library (here the library handle is
replaced by one that fails the test when touched).  The numpy model the GPU
tests compare against is checked here against the windows model it is built
from, on every map the GPU tests run, and on the two tie maps."""
import ctypes
import os
import re

import numpy as np
import pytest

import dq_fixtures as fx
from region_inputs import CASES, WINDOWS_SHAPES as SHAPES, tie_map, wmap
from windows_model import windows_model
from wtags_model import NONE, tags_model, votes_model

FAKE = {name: 0x10000 * (i + 1) for i, name in enumerate(
    ["regions", "offsets", "rows", "ids", "counts", "first", "inside", "best", "best_count", "mask", "area", "index",
     "mapped", "cts", "k_outs", "votes", "vbest"])}

GOOD = dict(regions=FAKE["regions"], width=16, height=8, nregions=5, block=4, expand=2, mask=FAKE["mask"] + 1,
            area=FAKE["area"], min_area=3, rows=FAKE["rows"], cap=1000, ids=FAKE["ids"], counts=FAKE["counts"],
            first=FAKE["first"], inside=FAKE["inside"], best=FAKE["best"], best_count=FAKE["best_count"],
            offsets=FAKE["offsets"])
GOOD_VOTES = dict(regions=FAKE["regions"], n=128, nregions=5, offsets=FAKE["offsets"], index=FAKE["index"], total=300,
                  mapped=FAKE["mapped"], cts=FAKE["cts"], k_outs=FAKE["k_outs"], k=4, votes=FAKE["votes"],
                  best=FAKE["vbest"])


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.lib()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _tags(lib, host, **kw):
    a = dict(GOOD, **kw)
    args = (_p(a["regions"]), a["width"], a["height"], a["nregions"], a["block"], a["expand"], _p(a["mask"]),
            _p(a["area"]), a["min_area"], _p(a["rows"]), a["cap"], _p(a["ids"]), _p(a["counts"]), _p(a["first"]),
            _p(a["inside"]), _p(a["best"]), _p(a["best_count"]), _p(a["offsets"]))
    return lib.dq_hip_window_tags(*args) if host else lib.dq_hip_window_tags_dev(0, *args, None)


def _votes(lib, **kw):
    a = dict(GOOD_VOTES, **kw)
    return lib.dq_hip_window_votes_dev(0, _p(a["regions"]), a["n"], a["nregions"], _p(a["offsets"]), _p(a["index"]),
                                       a["total"], _p(a["mapped"]), _p(a["cts"]), _p(a["k_outs"]), a["k"],
                                       _p(a["votes"]), _p(a["best"]), None)


def _tag_shape(kw):
    """A case of the windows tests in this call's terms: its d_offsets is d_rows here (required), its
    list arrays coords / index / colors are the entry arrays ids / counts / first; there is no frame."""
    names = {"offsets": "rows", "coords": "ids", "index": "counts", "colors": "first", "pixels": "best"}
    return {names.get(k, k): (FAKE[names[k]] + (v - v // 0x10000 * 0x10000) if k in names and v is not None else v)
            for k, v in kw.items()}


BAD = {name: _tag_shape(kw) for name, kw in SHAPES.items()}
BAD.update({
    "null_rows": dict(rows=None),
    "cap_without_an_entry_array": dict(ids=None, counts=None, first=None),
    "cap_1_without_an_entry_array": dict(cap=1, ids=None, counts=None, first=None, inside=None, best=None,
                                         best_count=None, offsets=None),
    "inside_2mod4": dict(inside=FAKE["inside"] + 2),
    "best_count_odd": dict(best_count=FAKE["best_count"] + 1),
    "own_offsets_2mod4": dict(offsets=FAKE["offsets"] + 2),
})

BAD_VOTES = {
    "null_regions": dict(regions=None),
    "null_offsets": dict(offsets=None),
    "null_index": dict(index=None),
    "null_mapped": dict(mapped=None),
    "null_cts": dict(cts=None),
    "null_k_outs": dict(k_outs=None),
    "null_votes": dict(votes=None),
    "null_best": dict(best=None),
    "regions_2mod4": dict(regions=FAKE["regions"] + 2),
    "offsets_odd": dict(offsets=FAKE["offsets"] + 1),
    "index_2mod4": dict(index=FAKE["index"] + 2),
    "mapped_2mod4": dict(mapped=FAKE["mapped"] + 2),
    "cts_2mod4": dict(cts=FAKE["cts"] + 2),
    "k_outs_odd": dict(k_outs=FAKE["k_outs"] + 3),
    "votes_2mod4": dict(votes=FAKE["votes"] + 2),
    "best_2mod4": dict(best=FAKE["vbest"] + 2),
    "k_0": dict(k=0),
    "k_257": dict(k=257),
    "k_max_u32": dict(k=0xFFFFFFFF),
    "nregions_0": dict(nregions=0),
    "nregions_2^31": dict(nregions=1 << 31),
    "n_0": dict(n=0),
    "n_2^31": dict(n=1 << 31),
    "total_max_u32": dict(total=0xFFFFFFFF),
}


def test_every_windows_shape_has_its_twin_here():
    assert set(SHAPES) <= set(BAD) and len(BAD) == len(SHAPES) + 6
    for name, kw in BAD.items():
        assert set(kw) <= set(GOOD), name
    assert BAD["offsets_2mod4"] == dict(rows=FAKE["rows"] + 2) and BAD["null_offsets"] == dict(rows=None)
    assert BAD["coords_odd"] == dict(ids=FAKE["ids"] + 1) and BAD["colors_2mod4"] == dict(first=FAKE["first"] + 2)


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_tag_arguments_return_minus_one_before_any_hip_call(lib, case, host):
    fn = lib.dq_hip_window_tags if host else lib.dq_hip_window_tags_dev
    assert fn.restype is ctypes.c_int64
    assert _tags(lib, host, **BAD[case]) == -1


@pytest.mark.parametrize("case", sorted(BAD_VOTES))
def test_bad_vote_arguments_return_minus_one_before_any_hip_call(lib, case):
    assert lib.dq_hip_window_votes_dev.restype is ctypes.c_int64
    assert _votes(lib, **BAD_VOTES[case]) == -1


def test_the_header_declares_the_entries_and_the_abi_version_stays(pkg):
    text = open(os.path.join(fx.ROOT, "include", "dq_hip.h")).read()
    for name in ("dq_hip_window_tags_dev", "dq_hip_window_tags", "dq_hip_window_votes_dev"):
        assert re.search(r"\bint64_t\s+%s\s*\(" % name, text), name
        assert hasattr(pkg.lib(), name), name
    assert not hasattr(pkg.lib(), "dq_hip_window_votes")          # (no host-pointer twin, and the header says so)
    assert "no host-pointer twin" in text
    assert text.index("capture windows of a region map") < text.index("---- window tags")
    assert pkg.lib().dq_hip_abi_version() == 1   # (adding entry points is compatible)
    assert re.search(r"#define\s+DQ_HIP_ABI_VERSION\s+1\b", text)
    assert (pkg.WINDOW_NO_ID, pkg.WINDOW_VOTES_MAX_CLUSTERS) == (0xFFFFFFFF, 256)


# ---------------------------------------------------------------------------
# The model.
@pytest.mark.parametrize("name,d,e", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_the_model_agrees_with_the_windows_model(name, d, e):
    reg, R = wmap(name)
    model = tags_model(reg, R, d, e)
    lengths = np.diff(windows_model(reg, R, None, d, e, lists=False)["offsets"].astype(np.int64))
    rows = model["rows"].astype(np.int64)
    area = np.bincount(reg.reshape(-1), minlength=R)
    for r in range(R):
        lo, hi = rows[r], rows[r + 1]
        assert model["counts"][lo:hi].sum() == lengths[r], r                 # row sums = list lengths
        if lengths[r]:
            assert model["inside"][r] == area[r], r                          # own(r) is part of window(r)
            assert (np.diff(model["first"][lo:hi].astype(np.int64)) > 0).all() and model["first"][lo] == 0, r
            assert len(set(model["ids"][lo:hi])) == hi - lo
            others = [(c, -int(s)) for s, c in zip(model["ids"][lo:hi], model["counts"][lo:hi]) if s != r]
            want = max(others) if others else (0, -NONE)
            assert (model["best_count"][r], model["best"][r]) == (want[0], -want[1]), r
        else:
            assert hi == lo and (model["inside"][r], model["best"][r], model["best_count"][r]) == (0, NONE, 0)


@pytest.mark.parametrize("order", [(1, 0, 2), (2, 0, 1)])
def test_the_tie_maps(order):
    reg, R = tie_map(order)
    assert reg.shape == (4, 12) and R == 3
    wm = windows_model(reg, R, None, 4, 1, lists=False)
    assert (wm["P"], wm["T"]) == (7, 3)                                      # (the call takes the map)
    model = tags_model(reg, R, 4, 1)
    lo, hi = model["rows"][0], model["rows"][1]
    assert list(model["ids"][lo:hi]) == list(order) and list(model["counts"][lo:hi]) == [16, 16, 16]
    assert model["best"][0] == 1 and model["best_count"][0] == 16


def test_the_votes_model_on_a_case_done_by_hand():
    flat = np.array([0, 0, 1, 1], np.uint32)
    offsets, index = np.array([0, 4, 6], np.uint32), np.array([0, 1, 2, 3, 2, 0], np.uint32)
    cts = np.array([[0xAA000005, 5, 7], [9, 9, 0]], np.uint32)               # a top byte, duplicates
    mapped = np.array([5, 7, 0xFF000007, 6, 9, 0], np.uint32)
    votes, best, misses = votes_model(flat, 2, offsets, index, mapped, cts, np.array([3, 2], np.uint32), 3)
    assert votes.tolist() == [[[1, 0, 1], [0, 0, 1]], [[1, 0, 0], [0, 0, 0]]]
    assert best.tolist() == [[0, 2], [0, NONE]] and misses == 2              # (6 is in no table; 0 is above k_outs)


# ---------------------------------------------------------------------------
@pytest.fixture
def no_library(pkg, monkeypatch):
    """The wrappers' own checks: reaching the library fails the test."""
    def touched():
        raise AssertionError("the wrapper called into the library")
    monkeypatch.setattr(pkg, "lib", touched)
    monkeypatch.setattr(pkg, "_require_gpu", touched)
    return pkg


W, H, R, K, CAP, M = 8, 4, 5, 4, 100, 60
N = W * H


def _words(count):
    import torch
    return torch.zeros(count, dtype=torch.int32)


def _bytes(count):
    import torch
    return torch.zeros(count, dtype=torch.uint8)


def _good_tags():
    return dict(t_regions=_words(N), width=W, height=H, num_regions=R, t_rows=_words(R + 1), t_mask=_bytes(N),
                t_area=_words(R), min_area=2, capacity=CAP, t_ids=_words(CAP), t_counts=_words(CAP),
                t_first=_words(CAP), t_inside=_words(R), t_best=_words(R), t_best_count=_words(R),
                t_offsets=_words(R + 1))


def _good_votes():
    return dict(t_regions=_words(N), num_pixels=N, num_regions=R, t_offsets=_words(R + 1), t_index=_words(M), total=M,
                t_mapped=_words(M), cts=np.zeros((R, K), np.uint32), k_outs=np.zeros(R, np.uint32), num_clusters=K,
                t_votes=_words(R * 2 * K), t_best=_words(R * 2))


TAG_TENSORS = (("t_regions", N), ("t_rows", R + 1), ("t_area", R), ("t_ids", CAP), ("t_counts", CAP), ("t_first", CAP),
               ("t_inside", R), ("t_best", R), ("t_best_count", R), ("t_offsets", R + 1))
VOTE_TENSORS = (("t_regions", N), ("t_offsets", R + 1), ("t_index", M), ("t_mapped", M), ("t_votes", R * 2 * K),
                ("t_best", R * 2))


def _calls(pkg):
    return ((pkg.window_tags_device, _good_tags, TAG_TENSORS), (pkg.window_votes_device, _good_votes, VOTE_TENSORS))


def _refused(fn, good, **kw):
    with pytest.raises(ValueError):
        fn(**dict(good(), **kw))


def _strided(count, dtype=None):
    import torch
    t = torch.zeros(2 * count, dtype=dtype or torch.int32)[::2]
    assert not t.is_contiguous() and t.numel() == count
    return t


def test_wrapper_names(pkg):
    for name in ("window_tags_device", "window_tags", "window_votes_device"):
        assert callable(getattr(pkg, name)), name


def test_device_wrappers_refuse_non_contiguous_tensors(no_library):
    import torch
    for fn, good, tensors in _calls(no_library):
        for name, count in tensors:
            _refused(fn, good, **{name: _strided(count)})
            _refused(fn, good, **{name: np.zeros(2 * count, np.uint32)[::2]})   # (numpy arrays get the same checks)
    _refused(no_library.window_tags_device, _good_tags, t_mask=_strided(N, torch.uint8))
    _refused(no_library.window_votes_device, _good_votes, cts=np.zeros((R, 2 * K), np.uint32)[:, ::2])


def test_device_wrappers_refuse_wrong_element_sizes(no_library):
    import torch
    for fn, good, tensors in _calls(no_library):
        for name, count in tensors:
            for bad in (_bytes(count), torch.zeros(count, dtype=torch.int16), torch.zeros(count, dtype=torch.int64),
                        np.zeros(count, np.uint64)):
                _refused(fn, good, **{name: bad})
            _refused(fn, good, **{name: 0x10000})     # a raw pointer has no length
    for bad in (_words(N), torch.zeros(N, dtype=torch.int16), np.zeros(N, np.uint32)):
        _refused(no_library.window_tags_device, _good_tags, t_mask=bad)
    _refused(no_library.window_votes_device, _good_votes, cts=np.zeros((R, K), np.int64))
    _refused(no_library.window_votes_device, _good_votes, k_outs=np.zeros(R, np.uint16))


def test_device_wrappers_refuse_short_arrays(no_library):
    for fn, good, tensors in _calls(no_library):
        for name, count in tensors:
            _refused(fn, good, **{name: _words(count - 1)})
        _refused(fn, good, num_regions=R + 1)         # fewer rows, offsets and per-region words than ids
        _refused(fn, good, t_regions=None)
    tags, votes = no_library.window_tags_device, no_library.window_votes_device
    _refused(tags, _good_tags, t_mask=_bytes(N - 1))
    _refused(tags, _good_tags, height=H + 1)          # the map-sized tensors are one row short
    _refused(tags, _good_tags, capacity=CAP + 1)      # every entry array is one entry short
    _refused(tags, _good_tags, t_rows=None)
    _refused(tags, _good_tags, t_ids=None, t_counts=None, t_first=None)      # a capacity without an entry array
    _refused(votes, _good_votes, num_pixels=N + 1)
    _refused(votes, _good_votes, total=M + 1)
    _refused(votes, _good_votes, num_clusters=K + 1)  # cts and t_votes are too small
    for name in ("t_offsets", "t_index", "t_mapped", "t_votes", "t_best", "cts", "k_outs"):
        _refused(votes, _good_votes, **{name: None})
    _refused(votes, _good_votes, cts=np.zeros((R, K - 1), np.uint32))
    _refused(votes, _good_votes, k_outs=np.zeros(R - 1, np.uint32))


def test_device_wrappers_refuse_out_of_range_scalars(no_library):
    for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(width=65536, height=1),
               dict(width=1, height=65536), dict(width=65535, height=65535), dict(num_regions=0),
               dict(num_regions=-1), dict(num_regions=1 << 31), dict(block=0), dict(block=9), dict(block=-1),
               dict(expand=-1), dict(expand=4), dict(min_area=-1), dict(min_area=1 << 32), dict(capacity=-1),
               dict(capacity=1 << 32)):
        _refused(no_library.window_tags_device, _good_tags, **kw)
    for kw in (dict(num_clusters=0), dict(num_clusters=257), dict(num_clusters=-1), dict(num_regions=0),
               dict(num_regions=1 << 31), dict(num_pixels=0), dict(num_pixels=1 << 31), dict(total=-1),
               dict(total=(1 << 32) - 1)):
        _refused(no_library.window_votes_device, _good_votes, **kw)


def test_host_wrapper_refuses_bad_arrays_and_scalars(no_library):
    reg = np.zeros((H, W), np.uint32)
    for bad in (np.zeros(N, np.uint32), np.zeros((2, H, W), np.uint32), np.zeros((0, W), np.uint32),
                np.zeros((H, W), np.uint64), np.zeros((H, W), np.float32), np.full((H, W), -1, np.int32)):
        with pytest.raises(ValueError):
            no_library.window_tags(bad)
    for kw in (dict(mask=np.zeros(N - 1, np.uint8)), dict(mask=np.zeros(N, np.uint32)),
               dict(area=np.zeros(0, np.uint32)), dict(num_regions=0), dict(num_regions=1 << 31), dict(block=0),
               dict(block=9), dict(expand=4), dict(expand=-1), dict(min_area=-1)):
        with pytest.raises(ValueError):
            no_library.window_tags(reg, **kw)
    with pytest.raises(ValueError):   # an id the count does not cover
        no_library.window_tags(np.full((H, W), 3, np.uint32), num_regions=3)
