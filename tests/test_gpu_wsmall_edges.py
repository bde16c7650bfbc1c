"""The one-launch weighted kernel (dq_wsmall.hip) at the edges of its own
mechanisms -- the cases of tests/wsmall_edges.py, each proven to be what it
claims on the CPU (tests/test_wsmall_edges.py): the fullest and the boundary
hash buckets of its counting sort, a crowded LDS hash slot whose probe chain
wraps, its four limits and the fall-backs one step above them, root lengths
around the 368-summand fold chunks, their 16- and 8-wide tails and the
1024-record partition steps, and maps with R+G+B ties, or with a centre
dropped by the dedup, at 16 / 17 colours and 16384 / 16385 pixels.

Equality is exact everywhere: colortable, returned K, painted pixels, split
trace, centroid doubles (as uint64 bits; the means of empty clusters are not
recorded by the reference and not compared) and cluster sizes, against both
the reference's record (tests/golden/weighted3.*) and the oracle composed as
the kernel is (dqo_color_table + dqo_cluster_weighted(max_iters) + first-
occurrence dedup + dqo_map).  Which path ran is asserted.  Every output
tensor carries guard words behind its end.

Which case notices which slip of the kernel:
  the rank comparison in the bucket loop (`>` to `<`)    test_case[bucket_fullest], [bucket_0], [bucket_20022],
                                                           [bucket_pair_*], [bucket_order_asc], [bucket_order_desc]
  kWsSeqChunk's 8-wide tail (its last summand dropped)    test_case[fold_*] (44 cases: trace and centroid bits)
  the bail-out above kWsMaxU (`>` to `>=`)                test_case[u6144_n6144], [u6144_n131071] (last_rounds);
                                                           the other direction: [u6145] (last_rounds > 1)
  n <= kWsMapInline where the kernel maps (`<=` to `<`)   test_case[tie_*_n16384], [fold_2049_pow2] (16384 pixels)
  the map's `j > s` rank rule (`>` to `>=`)               test_case[tie_m16_*], [tie_m2_*], [fold_7..9*]
"""
import functools

import numpy as np
import pytest

import dq_fixtures as fx
import wsmall_edges as we

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = 0xA5A5A5A5
SPECS = we.case_specs()
NAMES = [s["name"] for s in SPECS]
BY_NAME = {s["name"]: s for s in SPECS}
INDEX = {n: i for i, n in enumerate(NAMES)}
RECORDS = fx.load_json("weighted3.json")
FALL_BACK = ("u6145", "k65", "n131072")
ITER_CASES = [n for n in NAMES if n.startswith("fold_") or n == "bucket_fullest"
              or (n.split("_n")[0] in we.TIE_DENSE)]


@functools.lru_cache(maxsize=None)
def _px(name):
    px = we.build(BY_NAME[name])
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def _oracle(name, max_iters=10):
    return we.oracle_run(_px(name), BY_NAME[name]["k"], max_iters)


@functools.lru_cache(maxsize=None)
def _arrs():
    z = fx.load_npz("weighted3.npz")
    return {k: z[k] for k in z.files}


def _to_dev(px):
    import torch
    return torch.from_numpy(np.array(px, np.uint32).view(np.int32)).to("cuda:0")   # (a writable copy)


def _guarded(count):
    import torch
    return torch.full((count + GUARD,), FILL - (1 << 32), dtype=torch.int32, device="cuda:0")


def _unguard(t, n):
    a = t.cpu().numpy().view(np.uint32)
    assert (a[n:] == FILL).all(), "guard words behind the output"
    return a[:n]


def _run(gpu, name, max_iters=10):
    """One quant_device(.., all_pixels_unique=0) call of the case on fresh tensors."""
    import torch
    px, k = _px(name), BY_NAME[name]["k"]
    t, o = _to_dev(px), _guarded(len(px))
    ct, _ = gpu.quant_device(t, o, k, max_iters=max_iters, n=len(px), all_pixels_unique=0)
    torch.cuda.synchronize()
    means, sizes = gpu.last_centroids(k)
    return {"ct": ct, "out": _unguard(o, len(px)), "trace": gpu.last_trace(k), "means": means, "sizes": sizes,
            "rounds": gpu.last_rounds(), "prof": gpu.last_wsmall_profile()}


def _equals_oracle(got, name, max_iters=10):
    ref = _oracle(name, max_iters)
    assert np.array_equal(got["ct"], ref["ct"]) and len(got["ct"]) == len(ref["ct"]), (name, got["ct"], ref["ct"])
    assert np.array_equal(got["out"], ref["out"]), name
    if "trace" in got:
        assert np.array_equal(got["trace"], ref["trace"]), name
        assert np.array_equal(got["sizes"], ref["sizes"]), name
        f = ref["sizes"] > 0
        assert np.array_equal(got["means"][f].view(np.uint64), ref["means"][f].view(np.uint64)), name


def _equals_record(got, name):
    i = INDEX[name]
    c = RECORDS[i]
    assert c["spec"] == BY_NAME[name] and c["n_px"] == len(got["out"])
    assert [int(v) for v in got["ct"]] == c["ct"] and len(got["ct"]) == c["k_out"], name
    assert "%016x" % fx.fnv(got["out"]) == c["out_fnv"], name
    if "trace" in got:
        assert np.array_equal(got["trace"], _arrs()["trace_%d" % i]), name
        assert we.filled_means_equal(got["means"], got["sizes"], _arrs()["means_%d" % i]), name


def _path_is(got, name, kernel):
    if kernel:
        assert got["rounds"] == 1 and got["prof"], (name, got["rounds"])
    else:
        assert got["prof"] == {}, name
        if name in FALL_BACK:
            assert got["rounds"] > 1, (name, got["rounds"])


@pytest.mark.parametrize("name", NAMES)
def test_case(gpu, name):
    """Every case through quant_device: the record, the oracle, and the path."""
    got = _run(gpu, name)
    _path_is(got, name, name not in FALL_BACK)
    _equals_record(got, name)
    _equals_oracle(got, name)
    if BY_NAME[name]["kind"] in ("tie", "dedup"):
        # up to 16 colours: the kernel's map (inline, or its second launch above 16384 pixels); 17: the host's
        assert len(got["ct"]) == BY_NAME[name]["m"]


def test_limits_both_paths(gpu):
    """The limit cases once more with the kernel off: the multi-kernel rounds
    give the same outputs (6145 colours, K = 65 and 131072 pixels took them
    anyway: asserted by test_case)."""
    try:
        for name in we.LIMIT_CASES:
            gpu.set_wsmall(True)
            a = _run(gpu, name)
            _path_is(a, name, name not in FALL_BACK)
            gpu.set_wsmall(False)
            b = _run(gpu, name)
            _path_is(b, name, False)
            for got in (a, b):
                _equals_record(got, name)
                _equals_oracle(got, name)
            assert np.array_equal(a["ct"], b["ct"]) and np.array_equal(a["out"], b["out"]), name
            assert np.array_equal(a["trace"], b["trace"]) and np.array_equal(a["sizes"], b["sizes"]), name
    finally:
        gpu.set_wsmall(True)


@pytest.mark.parametrize("max_iters", [1, 2, 3, 10])
def test_max_iters_and_fixed_point(gpu, max_iters):
    """max_iters 1, 2, 3, 10 with the exact fixed point on and off, on the
    fold-length, fullest-bucket and tie cases: identical outputs, both the
    oracle's at that max_iters; with the switch off the kernel's 2-means loop
    runs exactly (K - 1) * max_iters passes, with it on no more."""
    try:
        for name in ITER_CASES:
            k = BY_NAME[name]["k"]
            gpu.set_fixed_point(True)
            on = _run(gpu, name, max_iters)
            gpu.set_fixed_point(False)
            off = _run(gpu, name, max_iters)
            for got in (on, off):
                _path_is(got, name, True)
                _equals_oracle(got, name, max_iters)
                if max_iters == 10:
                    _equals_record(got, name)
            assert off["prof"]["passes"]["kmeans"] == (k - 1) * max_iters, (name, off["prof"]["passes"])
            assert on["prof"]["passes"]["kmeans"] <= (k - 1) * max_iters, (name, on["prof"]["passes"])
            assert on["prof"]["passes"]["split"] == off["prof"]["passes"]["split"] == k - 1
            assert on["prof"]["passes"]["init"] == off["prof"]["passes"]["init"] == 1
    finally:
        gpu.set_fixed_point(True)


def _batch(gpu, names, max_iters=10):
    """quant_weighted_regions_device over the cases `names` in one call -> [(ct, out)]."""
    import torch
    ts = [_to_dev(_px(n)) for n in names]
    outs = [_guarded(len(_px(n))) for n in names]
    w = gpu.WeightedRegions(ts, outs, [BY_NAME[n]["k"] for n in names])
    assert list(w.ns) == [len(_px(n)) for n in names]   # (the guard words lie behind each region's n)
    w.run(max_iters)
    torch.cuda.synchronize()
    return [{"ct": w.colortable(i), "out": _unguard(outs[i], len(_px(n)))} for i, n in enumerate(names)]


def test_batch_equals_single_calls(gpu):
    """All cases as regions of ONE quant_weighted_regions_device call, between
    two calls of fewer than 10 regions: mixed K, regions above 16384 pixels
    with at most 16 colours (a batch has no second launch: the host maps
    them), with and without a centre dropped by the dedup, and the
    6145-colour, K = 65 and 131072-pixel regions, which are taken one by one.
    Every region equals its single call and its record.  (More than 64
    regions: the staging tables start at 64 entries, so this call grows them
    when no earlier call of the process has -- they never shrink, so in the
    whole suite an earlier region batch may already have.)"""
    assert len(NAMES) > 64 and len(set(BY_NAME[n]["k"] for n in NAMES)) >= 6
    big16 = [n for n in NAMES if len(_px(n)) > we.MAP_INLINE and len(_oracle(n)["ct"]) <= we.MAP_MAX
             and n not in FALL_BACK]
    assert "tie_m16_n16385" in big16 and "dedup_m16_n16385" in big16 and "n131071" in big16
    small_a = NAMES[:7]
    small_b = ["k2", "dedup_m17_n16385", "u6145", "fold_369", "dedup_m16_n16384", "dedup_m16_n16385"]
    for names in (small_a, NAMES, small_b):
        assert len(names) < 10 or len(names) > 64
        got = _batch(gpu, names)
        for g, name in zip(got, names):
            _equals_record(g, name)
            _equals_oracle(g, name)
            single = _run(gpu, name)
            assert np.array_equal(g["ct"], single["ct"]) and np.array_equal(g["out"], single["out"]), name


ORDER_A = ["dedup_m16_n16384", "dedup_m16_n16385", "dedup_m17_n16385", "u6145", "tie_m16_n16384", "k64", "k2"]
ORDER_B = ["k64", "k2", "tie_lattice_n16384", "tie_lattice_n16385", "tie_m17_n16384", "n131072", "tie_m1_n16384"]


def test_two_orders(gpu):
    """The single calls in two fixed orders in one process.  By their specs
    (pixel count, deduped colours, the limits) both orders hold the
    adjacencies inline map -> second-launch map -> host map -> fall-back ->
    inline map, and K = 64 followed by K = 2; which map ran is not reported
    by the engine and not observed here, only kernel or rounds (_path_is).
    Every result equals its record (and the oracle) in both orders: nothing
    of a call survives into the next."""
    rest = [n for n in NAMES if n not in ORDER_A]
    order1 = ORDER_A + rest
    rest = [n for n in reversed(NAMES) if n not in ORDER_B]
    order2 = rest[:40] + ORDER_B + rest[40:]
    assert sorted(order1) == sorted(order2) == sorted(NAMES) and order1 != order2
    for order in (order1, order2):
        maps = []
        for name in order:
            got = _run(gpu, name)
            _path_is(got, name, name not in FALL_BACK)
            _equals_record(got, name)
            _equals_oracle(got, name)
            n, m = len(_px(name)), len(got["ct"])
            maps.append("fall-back" if name in FALL_BACK else "host" if m > we.MAP_MAX else
                        "inline" if n <= we.MAP_INLINE else "second")
        chain = ",".join(maps)
        assert "inline,second,host,fall-back,inline" in chain
        ks = [BY_NAME[n]["k"] for n in order]
        assert any(a == 64 and b == 2 for a, b in zip(ks, ks[1:]))
