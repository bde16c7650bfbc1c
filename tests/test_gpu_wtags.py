"""GPU: the tag histogram of every capture window and the inside / outside
votes of a window's quant (include/dq_hip.h, "window tags").

The references are tags_model and votes_model of wtags_model.py, numpy written
from the definition alone and using none of the code under test.  Equality is
exact everywhere: array_equal on every array, == on every scalar.  Every
output buffer is pre-filled with a sentinel and carries guard words behind its
last entry.

Shapes are the smallest at which each mechanism can fail: the windows tests'
maps (clipped blocks, overlapping windows, one region per pixel with up to 192
ids per row, ids permuted against the raster order), masks that remove an id
from a row and empty a row, regions the area rule skips, two tie maps, and one
map per scan that crosses the scan's first top-level chunk."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import dq_fixtures as fx
from region_dev import body, guarded, same, to_dev, to_host
from region_inputs import CASES, frame, mask_of, noise, tie_map, wmap
from regions_model import regions_model
from windows_model import windows_model
from wtags_model import NONE, tags_model, votes_model

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = 0xA5A5A5A5
ENTRY = ("ids", "counts", "first")
REGION = ("inside", "best", "best_count")
_guarded = functools.partial(guarded, guard=GUARD, fill=FILL)


def _take(t, size, what):
    return body(t, size, GUARD, FILL, what)


@functools.lru_cache(maxsize=None)
def _area(name):
    reg, R = wmap(name)
    return np.bincount(reg.reshape(-1), minlength=R).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _model(name, d, e, kind=None, min_area=None):
    """One model per case, shared by the tests and left unchanged."""
    reg, R = wmap(name)
    return tags_model(reg, R, d, e, mask_of(kind, *reg.shape), _area(name) if min_area is not None else None,
                      min_area or 0)


# ---------------------------------------------------------------------------
def _run(gpu, reg, R, d, e, mask=None, area=None, min_area=0, stream=None, cap=None):
    """window_tags_device on fresh guarded tensors: the count-only call, then the call with `cap`
    (default: E) -> dict of every array and E; the entry arrays are None when they were left alone."""
    import torch
    h, w = reg.shape
    t_reg = to_dev(reg.reshape(-1))
    t_mask = to_dev(mask.reshape(-1), np.uint8) if mask is not None else None
    t_area = to_dev(area) if area is not None else None
    t_rows = _guarded(R + 1)
    if stream is not None:   # (the tensors above were filled on the current stream, the sentinel included: a
        stream.wait_stream(torch.cuda.current_stream())   # fill that ran after the call would undo its output)
    kw = dict(block=d, expand=e, t_mask=t_mask, t_area=t_area, min_area=min_area, stream=stream)
    E = gpu.window_tags_device(t_reg, w, h, R, t_rows, **kw)
    assert _take(t_rows, R + 1, "rows")[R] == E
    cap = E if cap is None else cap
    t = {k: _guarded(R + 1) for k in ("rows", "offsets")}
    t.update({k: _guarded(max(cap, E)) for k in ENTRY})
    t.update({k: _guarded(R) for k in REGION})
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    got = gpu.window_tags_device(t_reg, w, h, R, t["rows"], capacity=cap, t_ids=t["ids"], t_counts=t["counts"],
                                 t_first=t["first"], t_inside=t["inside"], t_best=t["best"],
                                 t_best_count=t["best_count"], t_offsets=t["offsets"], **kw)
    assert got == E
    out = {"E": E}
    for k in ("rows", "offsets"):
        out[k] = _take(t[k], R + 1, k)
    for k in REGION:
        out[k] = _take(t[k], R, k)
    for k in ENTRY:
        if E <= cap:
            out[k] = _take(t[k], max(cap, E), k)[:E]
            assert (to_host(t[k])[E:] == FILL).all(), k
        else:
            assert (to_host(t[k]) == FILL).all(), k
            out[k] = None
    return out


def _same(got, want, keys=("rows", "offsets") + ENTRY + REGION):
    assert got["E"] == want["E"]
    same(got, want, keys)


def _check(gpu, name, d, e, kind=None, min_area=None):
    reg, R = wmap(name)
    assert (name, d, e) in CASES
    want = _model(name, d, e, kind, min_area)
    got = _run(gpu, reg, R, d, e, mask_of(kind, *reg.shape), _area(name) if min_area is not None else None,
               min_area or 0)
    _same(got, want)
    return got, want


# ---------------------------------------------------------------------------
# 1. Every map of the windows tests.
@pytest.mark.parametrize("name,d,e", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_every_case_of_the_windows_tests(gpu, name, d, e):
    got, want = _check(gpu, name, d, e)
    reg, R = wmap(name)
    lengths = np.diff(want["offsets"].astype(np.int64))
    assert got["E"] > 0 and np.array_equal(np.add.reduceat(got["counts"], got["rows"][:-1][lengths > 0]),
                                           lengths[lengths > 0])
    if (name, d, e) == ("each16x12", 8, 3):        # every block is in every window: rows of all 192 ids
        assert (np.diff(got["rows"]) == 192).all()
    if name.endswith("-permuted"):                 # first-appearance order is not id order
        assert any((np.diff(got["ids"][lo:hi].astype(np.int64)) < 0).any()
                   for lo, hi in zip(got["rows"][:-1], got["rows"][1:]))


# 2. Masks: ids that vanish from a row, an empty row.
@pytest.mark.parametrize("name,kind", [("noise64x48", "random"), ("noise64x48", "block"), ("noise97x41", "random"),
                                       ("noise97x41", "block"), ("islands", "island-window")])
def test_masks(gpu, name, kind):
    got, want = _check(gpu, name, 4, 2, kind=kind)
    plain = _model(name, 4, 2)
    assert got["E"] < plain["E"]                   # (some id's pixels in some window are all masked)
    if kind == "island-window":                    # island 1: an empty row, and it is in no other row
        assert got["rows"][1] == got["rows"][2] and 1 not in got["ids"]
        assert (got["inside"][1], got["best"][1], got["best_count"][1]) == (0, NONE, 0)


# 3. The area rule: absent regions have no row but appear as s.
@pytest.mark.parametrize("name,min_area", [("islands", 9), ("noise97x41", 8), ("noise64x48", 8)])
def test_area_rule(gpu, name, min_area):
    got, _ = _check(gpu, name, 4, 2, min_area=min_area)
    absent = _area(name) <= min_area
    assert absent.any() and not absent.all()
    widths = np.diff(got["rows"].astype(np.int64))
    assert (widths[absent] == 0).all() and (widths[~absent] > 0).all()
    assert set(np.nonzero(absent)[0]) <= set(got["ids"])
    assert (got["inside"][absent] == 0).all() and (got["best"][absent] == NONE).all()


# 4. Ids >= R are counted in no entry.
def test_ids_at_or_above_the_region_count(gpu):
    reg, R = wmap("noise97x41")
    want = tags_model(reg, R - 40, 4, 2)
    _same(_run(gpu, reg, R - 40, 4, 2), want)
    assert want["ids"].max() < R - 40 and want["E"] < _model("noise97x41", 4, 2)["E"]


# 5. Ties: the best other is the lowest id, whatever the order of the row.
@pytest.mark.parametrize("order", [(1, 0, 2), (2, 0, 1)])
def test_ties_go_to_the_lowest_id(gpu, order):
    reg, R = tie_map(order)
    got = _run(gpu, reg, R, 4, 1)
    _same(got, tags_model(reg, R, 4, 1))
    assert list(got["ids"][:3]) == list(order) and list(got["counts"][:3]) == [16, 16, 16]
    assert list(got["first"][:3]) == [0, 16, 32]
    assert (got["best"][0], got["best_count"][0], got["inside"][0]) == (1, 16, 16)


# 6. A map the windows call refuses: -2 and nothing written.
def test_a_refused_map_writes_nothing(gpu):
    reg, R = wmap("refused")
    h, w = reg.shape
    t_reg = to_dev(reg.reshape(-1))
    t = {k: _guarded(R + 1) for k in ("rows", "offsets")}
    t.update({k: _guarded(64) for k in ENTRY})
    t.update({k: _guarded(R) for k in REGION})
    p = lambda v: ctypes.c_void_p(v.data_ptr())   # noqa: E731
    rc = gpu.lib().dq_hip_window_tags_dev(0, p(t_reg), w, h, R, 4, 0, None, None, 0, p(t["rows"]), 64, p(t["ids"]),
                                          p(t["counts"]), p(t["first"]), p(t["inside"]), p(t["best"]),
                                          p(t["best_count"]), p(t["offsets"]), None)
    assert rc == -2
    for k, v in t.items():
        assert (to_host(v) == FILL).all(), k
    with pytest.raises(gpu.RegionRowsError):
        gpu.window_tags_device(t_reg, w, h, R, t["rows"], block=4, expand=0)
    with pytest.raises(gpu.RegionRowsError):
        gpu.window_tags(reg, block=4, expand=0)
    assert (to_host(t["rows"]) == FILL).all()


# 7. cap: E alone; one short leaves the entries alone and writes the rest; E writes them.
def test_capacity(gpu):
    reg, R = wmap("noise97x41")
    want = _model("noise97x41", 4, 2)
    short = _run(gpu, reg, R, 4, 2, cap=want["E"] - 1)     # (asserts the entry arrays are all sentinel)
    assert all(short[k] is None for k in ENTRY)
    _same(short, want, keys=("rows", "offsets") + REGION)
    _same(_run(gpu, reg, R, 4, 2, cap=want["E"]), want)
    _same(_run(gpu, reg, R, 4, 2, cap=want["E"] + 5), want)
    t_rows, t_ids = _guarded(R + 1), _guarded(want["E"])
    assert gpu.window_tags_device(to_dev(reg.reshape(-1)), 97, 41, R, t_rows, capacity=want["E"], t_ids=t_ids) \
        == want["E"]                                       # one entry array alone, no per-region array
    assert np.array_equal(_take(t_ids, want["E"], "ids"), want["ids"])


# 8. Against the other stages of the library.
def test_block_one_expand_zero_rows_are_the_areas(gpu):
    for name in ("rows65", "comb"):
        reg, R = wmap(name)
        got = _run(gpu, reg, R, 1, 0)
        assert got["E"] == R and np.array_equal(got["rows"], np.arange(R + 1))
        assert np.array_equal(got["ids"], np.arange(R)) and np.array_equal(got["counts"], _area(name))
        assert not got["first"].any() and np.array_equal(got["inside"], _area(name))
        assert (got["best"] == NONE).all() and not got["best_count"].any()


def test_block_one_expand_one_rows_are_the_adjacency_graph(gpu):
    lab = noise(97, 41, 3, seed=1)
    reg, _ = regions_model(lab, 4, frame(97, 41))
    reg = np.ascontiguousarray(reg.reshape(41, 97), np.uint32)
    R = int(reg.max()) + 1
    got = _run(gpu, reg, R, 1, 1)
    owner = np.repeat(np.arange(R), np.diff(got["rows"].astype(np.int64)))
    mine = {(int(r), int(s)) for r, s in zip(owner, got["ids"]) if r != s}
    t_reg = to_dev(reg.reshape(-1))
    E, graph = gpu.region_adjacency_device(t_reg, 97, 41, connectivity=4, edge_capacity=len(mine))
    assert 0 < E <= len(mine)
    edges = graph["edges"].cpu().numpy().view(np.uint32)
    assert mine == {(int(a), int(b)) for a, b in edges} | {(int(b), int(a)) for a, b in edges}
    # and the offsets are the windows call's
    t_off = _guarded(R + 1)
    gpu.region_windows_device(t_reg, 97, 41, R, t_off, block=1, expand=1)
    assert np.array_equal(got["offsets"], _take(t_off, R + 1, "offsets"))


# 9. The scans' first top-level chunks (2^20 elements each).
def test_scan_chunks(gpu):
    """The call has two scans of its own, both from dq_scan.h with top-level chunks of 2^20
    elements: the contribution count over the blocks, and the ranks over the words of the bitmap
    (one per 32 list positions).  8192 x 4100 bands at d = 1, e = 0: 33 587 200 blocks (33 chunks)
    and as many list positions, 1 049 602 bitmap words (2 chunks).  (The votes' scan over the
    regions is crossed in test_votes_scan_chunk.)"""
    import torch
    w, h, band = 8192, 4100, 3
    R = -(-h // band)
    t_reg = (torch.arange(h, dtype=torch.int32, device="cuda:0") // band).repeat_interleave(w)
    assert w * h // 32 + 2 > 1 << 20
    t = {k: _guarded(R + 1) for k in ("rows", "offsets")}
    t.update({k: _guarded(R) for k in ENTRY + REGION})
    E = gpu.window_tags_device(t_reg, w, h, R, t["rows"], block=1, expand=0, capacity=R, t_ids=t["ids"],
                               t_counts=t["counts"], t_first=t["first"], t_inside=t["inside"], t_best=t["best"],
                               t_best_count=t["best_count"], t_offsets=t["offsets"])
    area = np.minimum(band, h - band * np.arange(R)) * w
    assert E == R and np.array_equal(_take(t["rows"], R + 1, "rows"), np.arange(R + 1))
    assert np.array_equal(_take(t["offsets"], R + 1, "offsets"), np.concatenate([[0], np.cumsum(area)]))
    assert np.array_equal(_take(t["ids"], R, "ids"), np.arange(R))
    assert np.array_equal(_take(t["counts"], R, "counts"), area) and not _take(t["first"], R, "first").any()
    assert np.array_equal(_take(t["inside"], R, "inside"), area) and (_take(t["best"], R, "best") == NONE).all()


# 10. Two streams at once from two threads: the results are each call's own.
def test_two_streams_from_two_threads(gpu):
    import torch
    cases = [("noise96x80", 4, 2), ("noise97x41-permuted", 4, 2)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in cases]
    got, errors = [None] * 2, []

    def work(i):
        try:
            torch.cuda.set_device(0)
            name, d, e = cases[i]
            reg, R = wmap(name)
            for _ in range(3):
                got[i] = _run(gpu, reg, R, d, e, stream=streams[i])
        except BaseException as err:   # noqa: B036 (reported by the test's thread)
            errors.append(err)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i, (name, d, e) in enumerate(cases):
        _same(got[i], _model(name, d, e))


# 11. The host form.
def test_host_form(gpu):
    reg, R = wmap("islands")
    mask = mask_of("island-window", *reg.shape)
    got = gpu.window_tags(reg, mask=mask, area=_area("islands"), min_area=0)
    want = tags_model(reg, R, 4, 2, mask, _area("islands"), 0)
    _same(dict(got, E=len(got["ids"])), want)
    got = gpu.window_tags(reg.astype(np.uint16), num_regions=R + 3)
    want = _model("islands", 4, 2)
    assert np.array_equal(got["ids"], want["ids"]) and np.array_equal(got["rows"][:R + 1], want["rows"])
    assert (got["rows"][R:] == want["E"]).all() and (got["best"][R:] == NONE).all()


# ---------------------------------------------------------------------------
# Votes.
def _votes(gpu, flat, R, offsets, index, mapped, cts, k_outs, k):
    """window_votes_device on guarded tensors, against the model; returns (votes, best, misses)."""
    total = int(offsets[-1])
    t_votes, t_best = _guarded(R * 2 * k), _guarded(R * 2)
    misses = gpu.window_votes_device(to_dev(flat), len(flat), R, to_dev(offsets), to_dev(index), total,
                                     to_dev(mapped), np.ascontiguousarray(cts, np.uint32),
                                     np.ascontiguousarray(k_outs, np.uint32), k, t_votes, t_best)
    votes, best = _take(t_votes, R * 2 * k, "votes").reshape(R, 2, k), _take(t_best, R * 2, "best").reshape(R, 2)
    want_votes, want_best, want_misses = votes_model(flat, R, offsets, index, mapped, cts, k_outs, k)
    assert misses == want_misses
    assert np.array_equal(votes, want_votes) and np.array_equal(best, want_best)
    return votes, best, misses


def _synthetic(R, lengths, n, k, seed):
    """Lists of the given lengths over a map of n pixels with random ids: random colortables with
    k_outs[r] <= k, duplicate entries, a garbage top byte on cts and mapped; every mapped colour is an
    entry below k_outs[r] of its region's table."""
    rnd = lambda count, s: fx.xorshift(max(count, 1), seed=fx.SEED + seed + s)[:count]   # noqa: E731
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    total = int(offsets[-1])
    flat = (rnd(n, 1) % np.uint32(R)).astype(np.uint32)
    index = (rnd(total, 2) % np.uint32(n)).astype(np.uint32)
    owner = np.repeat(np.arange(R), lengths)
    by_id = np.argsort(flat, kind="stable")                                  # every second entry: a pixel of the
    start, have = np.searchsorted(flat[by_id], np.arange(R)), np.bincount(flat, minlength=R)   # region itself
    own = np.flatnonzero((np.arange(total) % 2 == 0) & (have[owner] > 0))
    index[own] = by_id[start[owner[own]] + index[own] % have[owner[own]]]
    k_outs = (1 + rnd(R, 3) % np.uint32(k)).astype(np.uint32)
    k_outs[::3] = k
    cts = (rnd(R * k, 4) & np.uint32(0x030303)).reshape(R, k)                # (64 colours: duplicates when k > 64)
    if k > 1:
        cts[:, 1] = cts[:, 0]                                                # a duplicate in every row: entry 0 wins
    pick = rnd(total, 5) % k_outs[owner]
    mapped = cts[owner, pick] | (rnd(total, 6) & np.uint32(0xFF000000))
    cts = cts | (rnd(R * k, 7).reshape(R, k) & np.uint32(0xFF000000))
    return flat, offsets, index, mapped.astype(np.uint32), cts.astype(np.uint32), k_outs


@pytest.mark.parametrize("k", [1, 4, 16, 256])
def test_votes_against_the_model(gpu, k):
    R = 37
    lengths = (fx.xorshift(R, seed=fx.SEED + 5) % np.uint32(300)).astype(np.int64)
    lengths[3] = 0                                                           # an empty window
    lengths[5] = 5000                                                        # three jobs
    flat, offsets, index, mapped, cts, k_outs = _synthetic(R, lengths, 4096, k, 100 * k)
    votes, best, misses = _votes(gpu, flat, R, offsets, index, mapped, cts, k_outs, k)
    assert misses == 0 and votes.sum() == offsets[-1]
    assert (best[3] == NONE).all() and not votes[3].any()
    if k > 1:
        assert not votes[:, :, 1].any()                                      # (the duplicate never wins)


def test_votes_ties_empty_sides_and_a_corrupted_word(gpu):
    # the map "one": a single region, every entry inside -> no outside vote
    reg, R = wmap("one")
    n = reg.size
    index = np.arange(n, dtype=np.uint32)
    cts, k_outs = np.array([[0x111111, 0x222222, 0x333333, 0x444444]], np.uint32), np.array([4], np.uint32)
    mapped = cts[0, [2, 1] * (n // 2) + [3]]                                 # 17 x entry 2, 17 x entry 1, 1 x entry 3
    assert n == 35
    votes, best, misses = _votes(gpu, reg.reshape(-1), 1, np.array([0, n], np.uint32), index, mapped, cts, k_outs, 4)
    assert misses == 0 and list(votes[0, 0]) == [0, 17, 17, 1] and tuple(best[0]) == (1, NONE)   # the tie: lowest i
    bad = mapped.copy()
    bad[4] ^= 0x000100                                                       # one corrupted word: a miss, no bin
    votes, best, misses = _votes(gpu, reg.reshape(-1), 1, np.array([0, n], np.uint32), index, bad, cts, k_outs, 4)
    assert misses == 1 and votes.sum() == n - 1
    # an entry above k_outs is no entry
    votes, best, misses = _votes(gpu, reg.reshape(-1), 1, np.array([0, n], np.uint32), index, mapped, cts,
                                 np.array([3], np.uint32), 4)
    assert misses == 1 and list(votes[0, 0]) == [0, 17, 17, 0]


def test_votes_one_long_list_beside_a_thousand_short_ones(gpu):
    """One list of 512 x 300 = 153 600 entries (75 jobs in 19 workgroups) beside 1000 lists of under 64."""
    R = 1001
    lengths = (fx.xorshift(R, seed=fx.SEED + 9) % np.uint32(64)).astype(np.int64)
    lengths[500] = 512 * 300
    flat, offsets, index, mapped, cts, k_outs = _synthetic(R, lengths, 512 * 300, 4, 7)
    votes, _, misses = _votes(gpu, flat, R, offsets, index, mapped, cts, k_outs, 4)
    assert misses == 0 and votes[500].sum() == 512 * 300


def test_votes_scan_chunk(gpu):
    """The scan over the regions (the first job of every list) crosses its first top-level chunk of
    2^20 elements: 2^20 + 5 regions with lists of 0 .. 2 entries."""
    R = (1 << 20) + 5
    lengths = (fx.xorshift(R, seed=fx.SEED + 11) % np.uint32(3)).astype(np.int64)
    flat, offsets, index, mapped, cts, k_outs = _synthetic(R, lengths, 4096, 2, 13)
    _, best, misses = _votes(gpu, flat, R, offsets, index, mapped, cts, k_outs, 2)
    assert misses == 0 and (best[lengths == 0] == NONE).all()


# ---------------------------------------------------------------------------
# End to end: region map -> windows -> per-window quant -> votes.
def test_pipeline_on_islands(gpu):
    reg, R = wmap("islands")
    h, w = reg.shape
    k = 4
    noise = fx.xorshift(w * h, seed=fx.SEED + 41) & np.uint32(0x0F0F0F)
    px = np.where(reg.reshape(-1) == 0, 0x202020 + noise, 0xC0C0C0 + noise).astype(np.uint32)   # islands bright
    wm = windows_model(reg, R, px, 4, 2)
    M = int(wm["offsets"][-1])
    t_reg, t_off, t_index, t_out = to_dev(reg.reshape(-1)), _guarded(R + 1), _guarded(M), _guarded(M)
    cts, k_outs, _ = gpu.quant_region_windows_device(t_reg, w, h, R, to_dev(px), k, t_off, capacity=M, t_out=t_out,
                                                     t_index=t_index)
    assert np.array_equal(_take(t_index, M, "index"), wm["index"])
    t_votes, t_best = _guarded(R * 2 * k), _guarded(R * 2)
    misses = gpu.window_votes_device(t_reg, w * h, R, t_off, t_index, M, t_out, cts, k_outs, k, t_votes, t_best)
    assert misses == 0
    # the model on the CPU oracle's outputs for the same ranges
    off = wm["offsets"].astype(np.int64)
    mapped, ref_cts, ref_k = np.zeros(M, np.uint32), np.zeros((R, k), np.uint32), np.zeros(R, np.uint32)
    for r in range(R):
        mine = np.ascontiguousarray(wm["colors"][off[r]:off[r + 1]])
        out, ct, kk = np.zeros(len(mine), np.uint32), np.zeros(k, np.uint32), ctypes.c_uint32(k)
        fx.oracle().dqo_quant_recurse_weighted(ctypes.c_uint32(len(mine)), fx.vp(mine), fx.vp(out), ctypes.byref(kk),
                                               fx.vp(ct))
        mapped[off[r]:off[r + 1]], ref_cts[r, :kk.value], ref_k[r] = out, ct[:kk.value], kk.value
    want_votes, want_best, want_misses = votes_model(reg.reshape(-1), R, wm["offsets"], wm["index"], mapped, ref_cts,
                                                     ref_k, k)
    assert want_misses == 0
    assert np.array_equal(_take(t_votes, R * 2 * k, "votes").reshape(R, 2, k), want_votes)
    best = _take(t_best, R * 2, "best").reshape(R, 2)
    assert np.array_equal(best, want_best)
    for r in range(1, R):                          # every island: inside and outside are different entries
        assert best[r, 0] != NONE and best[r, 1] != NONE and best[r, 0] != best[r, 1], r
        assert cts[r, best[r, 0]] != cts[r, best[r, 1]], r
