"""GPU: merging regions over their adjacency graph (include/dq_hip.h, "region
merge") and the host pipeline labels -> segments.

The reference is merge_model of merge_model.py on the regions of regions_model
(regions_model.py) and the edges of edges_model (adjacency_model.py), written
against the definition and using none of the code under test; the named inputs
are merge_inputs of region_inputs.py.  Equality is exact everywhere:
array_equal on the map, remap and every stats array, == on R' and the rounds.
test_merge_model.py pins the model's own R' and rounds on the 64 x 48 noise
map, so a weakened model cannot pass.

There is no fixture of batman labels under tests/golden (only the PNG), so the
host pipeline is checked on the noise maps alone.

With a distance limit the rounds are not bounded by 32 (a component may get
its first offer only after a neighbour's mean has moved): a star of 120 leaves
that come into range one per round must take 120 rounds.

Shapes are a few thousand pixels (the star: 31 thousand, a row per region):
the smallest at which each mechanism (rounds,
chains, one hot root, mutual pairs, capacities, the 1024-bit chunks of the
numbering, the 16-byte pixel pass and its tail) can fail."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import dq_fixtures as fx
from adjacency_model import edges_model
from merge_model import NONE, merge_model
from region_dev import same, to_dev, to_host
from region_inputs import merge_inputs, merge_labels_and_frame
from regions_model import regions_model

pytestmark = pytest.mark.gpu

GUARD_WORD = 0xA5A5A5A5
ALL = 1 << 31                  # min_area above every area: everything is restless
PER = {"area": 1, "bbox": 4, "first": 1, "sums": 6}   # 4-byte words per region


@functools.lru_cache(maxsize=None)
def _reference(name, min_area, max_dist=NONE, max_rounds=0):
    i = merge_inputs(name)
    return merge_model(i["regions"], i["area"], i["first"], i["sums"], i["bbox"], i["edges"], min_area, max_dist,
                       max_rounds)


def _run(gpu, inp, min_area, max_dist=NONE, max_rounds=0, edges=None, regions=None, stream=None):
    """merge_regions_device on fresh tensors, every output at capacity R
    -> (R', rounds, outputs as unsigned numpy)."""
    import torch
    edges = inp["edges"] if edges is None else edges
    t = {k: to_dev(inp[k].reshape(-1)) for k in ("area", "first", "sums", "bbox")}
    t_reg = to_dev(inp["regions"] if regions is None else regions)
    t_edges = to_dev(edges.reshape(-1)) if len(edges) else None
    if stream is not None:   # (the tensors above were filled on the current stream)
        stream.wait_stream(torch.cuda.current_stream())
    r, rounds, out = gpu.merge_regions_device(t_reg, inp["R"], t["area"], t["first"], t["sums"], t_edges, min_area,
                                              max_dist=max_dist, max_rounds=max_rounds, t_bbox=t["bbox"],
                                              num_edges=len(edges), stats_capacity=inp["R"], stream=stream)
    assert out["regions"] is t_reg
    return r, rounds, {k: to_host(v, np.uint64 if k == "sums" else np.uint32) for k, v in out.items()}


KEYS = ("regions", "remap", "area", "first", "sums", "bbox")


def _same(r, rounds, got, want):
    assert (r, rounds) == (want["R"], want["rounds"])
    assert sorted(got) == sorted(KEYS)
    same(got, want, KEYS)


# ---------------------------------------------------------------------------
# 1. Noise over a parameter grid.
GRID = [(2, NONE), (10, NONE), (ALL, NONE), (10, 20000), (ALL, 30000), (ALL, 0)]
@pytest.mark.parametrize("params", GRID, ids=lambda p: "area%d-dist%d" % p)
@pytest.mark.parametrize("name", ["noise64x48", "noise96x80", "noise97x41"])
def test_noise_grid(gpu, name, params):
    want = _reference(name, *params)
    r, rounds, got = _run(gpu, merge_inputs(name), *params)
    _same(r, rounds, got, want)
    assert int(got["area"].sum()) == len(got["regions"])


# 2. Chain and ties.
@pytest.mark.parametrize("max_rounds", [0, 1])
def test_chain_of_2047_links_in_one_round(gpu, max_rounds):
    inp = merge_inputs("chain")
    assert inp["R"] == 2048 and len(inp["edges"]) == 2047
    want = _reference("chain", ALL, NONE, max_rounds)
    assert (want["R"], want["rounds"]) == (1, 1)
    r, rounds, got = _run(gpu, inp, ALL, max_rounds=max_rounds)
    _same(r, rounds, got, want)
    assert got["area"].tolist() == [2048] and got["bbox"].tolist() == [[0, 0, 2047, 0]]


# 3. One hot root.
def test_a_thousand_islands_fold_into_one_root(gpu):
    inp = merge_inputs("islands")
    assert inp["R"] == 1025 and int((inp["area"] == 1).sum()) == 1024
    want = _reference("islands", 2)
    assert (want["R"], want["rounds"]) == (1, 1)
    r, rounds, got = _run(gpu, inp, 2)
    _same(r, rounds, got, want)
    px = inp["pixels"].astype(np.uint64)
    assert got["sums"].tolist() == [[int(((px >> s) & 0xFF).sum()) for s in (16, 8, 0)]]
    assert got["bbox"].tolist() == [[0, 0, 63, 63]] and got["first"].tolist() == [0]


# 4. Mutual pairs.
def test_mutual_pairs_keep_the_lower_id(gpu):
    inp = merge_inputs("stripes")
    assert inp["R"] == 16 and (inp["area"] == 48).all()
    want = _reference("stripes", 49)     # above a stripe's area, below a pair's
    assert (want["R"], want["rounds"]) == (8, 1)
    assert want["remap"].tolist() == [i // 2 for i in range(16)]
    assert want["first"].tolist() == [8 * i for i in range(8)]
    r, rounds, got = _run(gpu, inp, 49)
    _same(r, rounds, got, want)


# 5. Round limit.
@pytest.mark.parametrize("max_rounds", [1, 2])
def test_round_limit(gpu, max_rounds):
    assert _reference("noise64x48", ALL, 30000)["rounds"] >= 4
    want = _reference("noise64x48", ALL, 30000, max_rounds)
    assert want["rounds"] == max_rounds
    r, rounds, got = _run(gpu, merge_inputs("noise64x48"), ALL, 30000, max_rounds)
    _same(r, rounds, got, want)


# 5b. With a distance limit the rounds are not bounded by 32: a star whose
# leaves come into range of the centre one per round, as its mean moves.
STAR_LEAVES, STAR_DIST = 120, 5000


@functools.lru_cache(maxsize=None)
def _star():
    """Region r is row r of a 256-wide map (area 256, so its 8.8 mean of the R
    channel is its R sum); region 0 is the centre, every leaf touches only it.
    Leaf k + 1's mean is the centre component's mean after k merges + STAR_DIST:
    out of range before round k + 1, in range in it."""
    L = STAR_LEAVES
    sums = np.zeros((L + 1, 3), np.uint64)
    total = 0
    for k in range(1, L + 1):
        sums[k, 0] = (256 * total) // (256 * k) + STAR_DIST
        total += int(sums[k, 0])
    assert int(sums[:, 0].max()) <= 255 * 256 and (np.diff(sums[1:, 0].astype(np.int64)) > 0).all()
    rows = np.arange(L + 1, dtype=np.uint32)
    inp = dict(w=256, h=L + 1, R=L + 1, regions=np.repeat(rows, 256), area=np.full(L + 1, 256, np.uint32),
               first=(256 * rows).astype(np.uint32), sums=sums,
               bbox=np.stack([0 * rows, rows, 255 + 0 * rows, rows], axis=1).astype(np.uint32),
               edges=np.stack([0 * rows[1:], rows[1:]], axis=1).astype(np.uint32))
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp


def test_star_takes_a_round_per_leaf(gpu):
    inp = _star()
    want = merge_model(inp["regions"], inp["area"], inp["first"], inp["sums"], inp["bbox"], inp["edges"], ALL,
                       STAR_DIST)
    assert (want["R"], want["rounds"]) == (1, STAR_LEAVES) and STAR_LEAVES > 64
    r, rounds, got = _run(gpu, inp, ALL, STAR_DIST)
    _same(r, rounds, got, want)
    assert got["area"].tolist() == [256 * (STAR_LEAVES + 1)]


# 6. Edge list robustness.
@pytest.mark.parametrize("how", ["swapped", "shuffled", "three_times"])
def test_edge_list_order_and_duplicates_do_not_matter(gpu, how):
    inp = merge_inputs("noise96x80")
    e = inp["edges"]
    if how == "swapped":
        e = e[:, ::-1].copy()
        assert (e[:, 1] < e[:, 0]).all()
    elif how == "shuffled":
        e = e[np.argsort(fx.xorshift(len(e), seed=fx.SEED + 11), kind="stable")]
        e[::3] = e[::3, ::-1]
    else:
        e = np.concatenate([e, e[::-1], e[:, ::-1]])
    r, rounds, got = _run(gpu, inp, 10, 20000, edges=np.ascontiguousarray(e))
    _same(r, rounds, got, _reference("noise96x80", 10, 20000))


# 7. In place, another output map, capacities, single pointers, no remap.
def _raw(gpu, inp, min_area, cap, which=KEYS[2:], remap=True, in_place=True, offset=0):
    """The C entry point on guard-filled arrays 8 entries longer than the
    capacity -> (R', rounds, map, {name: all words as uint32}, remap words)."""
    import torch
    guard = int(np.full(1, GUARD_WORD, np.uint32).view(np.int32)[0])
    t = {k: to_dev(inp[k].reshape(-1)) for k in ("area", "first", "sums", "bbox", "edges")}
    n = len(inp["regions"])
    t_reg = torch.full((n + 8,), guard, dtype=torch.int32, device="cuda:0")
    t_reg[offset:offset + n] = to_dev(inp["regions"])       # offset 1: the map is not 16-byte aligned
    t_out = t_reg if in_place else torch.full((n + 8,), guard, dtype=torch.int32, device="cuda:0")
    bufs = {k: torch.full(((cap + 8) * PER[k],), guard, dtype=torch.int32, device="cuda:0") for k in which}
    t_remap = torch.full((inp["R"] + 8,), guard, dtype=torch.int32, device="cuda:0") if remap else None
    ptr = lambda x, off=0: None if x is None else ctypes.c_void_p(x.data_ptr() + 4 * off)  # noqa: E731
    rounds = ctypes.c_uint32(99)
    r = gpu.lib().dq_hip_merge_regions_dev(0, ptr(t_reg, offset), n, inp["R"], ptr(t["area"]), ptr(t["first"]),
                                           ptr(t["sums"]), ptr(t["bbox"]), len(inp["edges"]), ptr(t["edges"]),
                                           min_area, NONE, 0, ptr(t_out, offset), ptr(t_remap), cap,
                                           ptr(bufs.get("area")), ptr(bufs.get("bbox")), ptr(bufs.get("first")),
                                           ptr(bufs.get("sums")), ctypes.byref(rounds), None)
    if not in_place:
        assert np.array_equal(to_host(t_reg)[offset:offset + n], inp["regions"])   # the input map is left alone
    words = to_host(t_out)
    assert (words[:offset] == GUARD_WORD).all() and (words[offset + n:] == GUARD_WORD).all()
    return (r, rounds.value, words[offset:offset + n], {k: to_host(v) for k, v in bufs.items()},
            None if t_remap is None else to_host(t_remap))


def _heads(bufs, m):
    out = {}
    for k, words in bufs.items():
        head = words[:m * PER[k]]
        out[k] = head.view(np.uint64).reshape(m, 3) if k == "sums" else head.reshape(m, 4) if k == "bbox" else head
    return out


@pytest.mark.parametrize("which", ["zero", "one", "R-1", "R", "R+3"])
def test_stats_capacity(gpu, which):
    inp, want = merge_inputs("noise64x48"), _reference("noise64x48", 10)
    R2 = want["R"]
    cap = {"zero": 0, "one": 1, "R-1": R2 - 1, "R": R2, "R+3": R2 + 3}[which]
    m = min(R2, cap)
    r, rounds, reg, bufs, remap = _raw(gpu, inp, 10, cap, which=KEYS[2:] if cap else ())
    assert (r, rounds) == (R2, want["rounds"])
    assert np.array_equal(reg, want["regions"])
    assert np.array_equal(remap[:inp["R"]], want["remap"]) and (remap[inp["R"]:] == GUARD_WORD).all()
    for k, words in bufs.items():
        assert (words[m * PER[k]:] == GUARD_WORD).all(), k
    for k, head in _heads(bufs, m).items():
        assert np.array_equal(head, want[k][:m]), k


@pytest.mark.parametrize("which", ["area", "bbox", "first", "sums"])
def test_each_stats_pointer_alone(gpu, which):
    inp, want = merge_inputs("noise97x41"), _reference("noise97x41", 10)
    r, rounds, reg, bufs, _ = _raw(gpu, inp, 10, want["R"], which=(which,))
    assert (r, rounds) == (want["R"], want["rounds"]) and np.array_equal(reg, want["regions"])
    assert np.array_equal(_heads(bufs, want["R"])[which], want[which])
    assert (bufs[which][want["R"] * PER[which]:] == GUARD_WORD).all()


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
def test_output_map_in_place_or_apart_aligned_or_not_without_remap(gpu, in_place, offset):
    inp, want = merge_inputs("noise97x41"), _reference("noise97x41", 10)     # 3977 pixels: a tail of one
    r, rounds, reg, bufs, remap = _raw(gpu, inp, 10, want["R"], remap=False, in_place=in_place, offset=offset)
    assert remap is None and (r, rounds) == (want["R"], want["rounds"])
    assert np.array_equal(reg, want["regions"])
    for k, head in _heads(bufs, want["R"]).items():
        assert np.array_equal(head, want[k]), k


# 8. Degenerate inputs.
def test_one_region_no_edge(gpu):
    inp = merge_inputs("one")
    assert inp["R"] == 1 and len(inp["edges"]) == 0
    r, rounds, got = _run(gpu, inp, ALL)
    _same(r, rounds, got, _reference("one", ALL))
    assert (r, rounds) == (1, 0)


def test_min_area_zero_is_the_identity_on_a_raster_numbered_map(gpu):
    inp = merge_inputs("noise64x48")
    r, rounds, got = _run(gpu, inp, 0)
    assert (r, rounds) == (inp["R"], 0)
    assert np.array_equal(got["regions"], inp["regions"]) and np.array_equal(got["remap"], np.arange(inp["R"]))
    for k in ("area", "first", "sums", "bbox"):
        assert np.array_equal(got[k], inp[k]), k


def test_permuted_ids_come_out_numbered_by_first(gpu):
    base = merge_inputs("noise64x48")
    perm = np.argsort(fx.xorshift(base["R"], seed=fx.SEED + 5), kind="stable").astype(np.uint32)   # old -> new id
    inv = np.argsort(perm)
    inp = dict(base, regions=perm[base["regions"]], edges=perm[base["edges"]],
               **{k: base[k][inv] for k in ("area", "first", "sums", "bbox")})
    r, rounds, got = _run(gpu, inp, 0)
    assert (r, rounds) == (base["R"], 0)
    assert np.array_equal(got["regions"], base["regions"]) and np.array_equal(got["remap"], inv)
    assert np.array_equal(got["first"], base["first"])
    want = merge_model(inp["regions"], inp["area"], inp["first"], inp["sums"], inp["bbox"], inp["edges"], 10)
    _same(*_run(gpu, inp, 10), want)     # (ties go to the lowest INPUT id: not the raster-numbered answer)


# 9. Two streams at once.
def test_two_streams_at_once(gpu):
    """Two calls with different maps on two streams from two host threads
    (scratch is owned by each call) both come out right."""
    import torch
    cases = [("noise96x80", ALL, 30000), ("noise97x41", 10, NONE)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in cases]
    results = [None, None]
    wants = [_reference(*c) for c in cases]   # (the models, before the threads start)
    inps = [merge_inputs(c[0]) for c in cases]
    torch.cuda.synchronize()

    def work(i):
        results[i] = _run(gpu, inps[i], cases[i][1], cases[i][2], stream=streams[i])

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for want, (r, rounds, got) in zip(wants, results):
        _same(r, rounds, got, want)


# 10. Host pipeline.
@pytest.mark.parametrize("dtype", [np.uint8, np.uint32])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["noise64x48", "noise97x41"])
def test_segment_labels_equals_the_model_pipeline(gpu, name, connectivity, dtype):
    lab, px, _ = merge_labels_and_frame(name)
    h, w = lab.shape
    reg, st = regions_model(lab, connectivity, px)
    want = merge_model(reg, st["area"], st["first"], st["sums"], st["bbox"], edges_model(reg, w, h, connectivity),
                       10, 20000)
    assert 1 < want["R"] < len(st["area"]) and want["rounds"] >= 2
    if dtype is np.uint32:      # labels that differ only in the top byte
        lab = (lab.astype(np.uint32) << np.uint32(24)).astype(np.uint32)
    regions2d, stats, rounds = gpu.segment_labels(lab.astype(dtype), px, 10, max_dist=20000,
                                                  connectivity=connectivity)
    assert regions2d.shape == (h, w) and regions2d.dtype == np.uint32 and rounds == want["rounds"]
    assert np.array_equal(regions2d.reshape(-1), want["regions"])
    assert sorted(stats) == ["area", "bbox", "first", "sums"]
    for k, v in stats.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), k
    if dtype is np.uint8:       # room for fewer segments than there are: the wrapper calls once more
        again = gpu.segment_labels(lab.astype(dtype), px, 10, max_dist=20000, connectivity=connectivity,
                                   stats_capacity=16)
        assert want["R"] > 16 and again[2] == rounds and np.array_equal(again[0], regions2d)
        for k, v in again[1].items():
            assert np.array_equal(v, want[k]), k
