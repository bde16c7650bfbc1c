"""CPU: the edge cases of the one-launch weighted kernel (tests/wsmall_edges.py)
are what they claim to be, and the oracle reproduces the reference's records
of them (tests/golden/weighted3.*, made by make_golden.py --only weighted3)
bit for bit: colortable, output hash, split trace and centroid doubles.

The properties are asserted with numpy and the oracle alone.  The two hash
formulas are restated here once more, independently of the builders:
  bucket(c) = (33023 R + 30013 G + 27011 B) % 20023   (test_gpu_color_table._buckets)
  slot(c)   = ((c * 0x9E3779B1) mod 2^32) >> 19        (dq_wsmall.hip's LDS hash set)
"""
import numpy as np
import pytest

import dq_fixtures as fx
import wsmall_edges as we

SPECS = we.case_specs()
NAMES = [s["name"] for s in SPECS]
RECORDS = fx.load_json("weighted3.json")
FALL_BACK = {"u6145", "k65", "n131072"}   # the multi-kernel rounds take these


def _bucket(c):
    c = int(c) & 0xFFFFFF
    return (33023 * (c >> 16) + 30013 * ((c >> 8) & 255) + 27011 * (c & 255)) % 20023


def _slot(c):
    return (((int(c) & 0xFFFFFF) * 0x9E3779B1) % (1 << 32)) >> 19


def _is_pow2(v):
    v = np.asarray(v, np.int64)
    return bool(np.all((v > 0) & ((v & (v - 1)) == 0)))


def _runs(px):
    """(start, length) of the maximal runs of equal pixels."""
    starts = np.concatenate([[0], np.nonzero(px[1:] != px[:-1])[0] + 1])
    return starts, np.diff(np.concatenate([starts, [len(px)]]))


def _tied_pixels(px, pal):
    """How many pixels are at the minimum squared distance from two or more different palette colours."""
    pal = np.unique(np.asarray(pal, np.uint32))
    u, cnt = np.unique(px & np.uint32(0xFFFFFF), return_counts=True)
    p = np.stack([(u >> 16) & 0xFF, (u >> 8) & 0xFF, u & 0xFF], 1).astype(np.int64)
    q = np.stack([(pal >> 16) & 0xFF, (pal >> 8) & 0xFF, pal & 0xFF], 1).astype(np.int64)
    d = ((p[:, None, :] - q[None, :, :]) ** 2).sum(2)
    return int(cnt[(d == d.min(1, keepdims=True)).sum(1) >= 2].sum())


def _table_in_reference_order(px):
    """The oracle's colour table is in bucket order and, inside a bucket, first occurrence descending."""
    col, w = we.oracle_table(px)
    cols, first, cnt = we.first_occurrences(px)
    assert sorted(col.tolist()) == cols.tolist()
    f = dict(zip(cols.tolist(), first.tolist()))
    keys = [(_bucket(c), -f[c]) for c in col.tolist()]
    assert keys == sorted(keys)
    n = dict(zip(cols.tolist(), cnt.tolist()))
    assert np.array_equal(w.view(np.uint64), np.array([(1.0 / len(px)) * n[c] for c in col.tolist()]).view(np.uint64))


def test_specs_are_the_issue_list():
    """Nothing dropped: every family of the list is there by name, names are unique,
    and the records were made from exactly these specs."""
    assert len(set(NAMES)) == len(NAMES)
    want = ["bucket_fullest", "bucket_0", "bucket_20022", "bucket_order_asc", "bucket_order_desc", "bucket_order_mixed",
            "last_pixel_first", "u6144_n6144", "u6144_n131071", "u6145", "k64", "k65", "n131071", "n131072",
            "one_colour_n131071", "k_above_1_colours", "k_above_2_colours", "k_above_3_colours", "k1", "k2",
            "topbyte_table", "tie_m16_topbyte_n16385"]
    want += ["bucket_pair_%d_%d" % p for p in ((19, 20), (1279, 1280), (10000, 10001))]
    want += ["slot_runs_%d" % r for r in (1, 16, 64, 8192)]
    counts = [1, 7, 8, 9, 15, 16, 17, 367, 368, 369, 375, 376, 377, 735, 736, 737, 1023, 1024, 1025, 2047, 2048, 2049]
    want += ["fold_%d%s" % (u, t) for u in counts for t in ("", "_pow2")]
    want += ["tie_%s_n%d" % (v, n) for v in ("m1", "m2", "m16", "m17", "lattice") for n in (16384, 16385)]
    want += ["dedup_%s_n%d" % (v, n) for v in ("m16", "m17") for n in (16384, 16385)] + ["dedup_inexact_m16_n16385"]
    assert sorted(want) == sorted(NAMES)
    assert [c["spec"] for c in RECORDS] == SPECS
    assert set(we.LIMIT_CASES) <= set(NAMES)


@pytest.mark.parametrize("spec", SPECS, ids=NAMES)
def test_case_is_what_it_claims(spec):
    name, kind, k = spec["name"], spec["kind"], spec["k"]
    px = we.build(spec)
    assert px.dtype == np.uint32 and px.ndim == 1 and len(px) >= 1
    assert np.array_equal(px, we.build(spec)), "deterministic"
    n = len(px)
    assert n <= 131071 or name == "n131072"
    cols, first, cnt = we.first_occurrences(px)
    if spec.get("topbyte"):   # bits 24-31 set everywhere; the oracle ignores them
        assert int((px >> np.uint32(24)).min()) >= 1
        a, b = we.oracle_run(px, k), we.oracle_run(px & np.uint32(0xFFFFFF), k)
        assert np.array_equal(a["ct"], b["ct"]) and np.array_equal(a["out"], b["out"])
        assert np.array_equal(a["means"].view(np.uint64), b["means"].view(np.uint64))
    else:
        assert int(px.max()) < (1 << 24)
    assert we.takes_kernel(spec, px) == (name not in FALL_BACK)
    assert (n <= 131071 and k <= 64 and len(cols) <= 6144) == (name not in FALL_BACK)
    bs = np.array([_bucket(c) for c in cols])

    if kind == "bucket_fullest":
        allb = we.buckets_of(np.arange(1 << 24, dtype=np.int64))
        sizes = np.bincount(allb, minlength=20023)
        assert sizes.max() == 844 == len(cols) and (bs == int(np.argmax(sizes))).all()
        assert len(np.unique(px[:844])) == 844 and n == 844 + 60000   # each once, then 60 000 repeats
        assert not np.array_equal(px[:844], np.sort(px[:844]))        # shuffled
        _table_in_reference_order(px)
    elif kind == "bucket_only":
        assert spec["buckets"][0] in (0, 20022) and (bs == spec["buckets"][0]).all() and len(cols) >= 100
        _table_in_reference_order(px)
    elif kind == "bucket_pair":
        lo, hi = spec["buckets"]
        assert hi == lo + 1 and set(bs.tolist()) == {lo, hi}
        assert (bs == lo).sum() >= 100 and (bs == hi).sum() >= 100
        # the scan's boundaries: 20 buckets per thread, 64 threads per wave, two counts per word
        assert {(19, 20): lo // 20 != hi // 20, (1279, 1280): lo // 1280 != hi // 1280,
                (10000, 10001): lo % 2 == 0 and lo // 2 == hi // 2}[(lo, hi)]
        _table_in_reference_order(px)
    elif kind == "bucket_order":
        h = np.bincount(bs).argmax()
        inb = bs == h
        assert inb.sum() >= 3
        d = np.diff(first[inb])   # first occurrences, by ascending colour value
        assert {"asc": (d > 0).all(), "desc": (d < 0).all(), "mixed": (d > 0).any() and (d < 0).any()}[spec["order"]]
        _table_in_reference_order(px)
    elif kind == "last_pixel_first":
        assert n == 131071 and first[np.searchsorted(cols, px[-1])] == n - 1 == (1 << 17) - 2
        _table_in_reference_order(px)
    elif kind == "slot_runs":
        assert all(_slot(c) == 8190 for c in cols) and len(cols) == spec["ncol"] > 2   # 8190, 8191, then 0, 1, ..
        starts, lens = _runs(px)
        run = spec["run"]
        assert (lens[1:-1] == run).all() and lens[0] + (lens[-1] if run > 1 else 0) in (run, 2 * run)
        if run == 1:
            assert len(cols) == 1500 == n
        else:   # run heads off the 16-lane rows / waves; 8192-pixel runs straddle the 8 x 1024 blocks
            assert (starts[1:] % 16 != 0).all() and lens.max() == run
        if run >= 64:
            assert (starts[1:] % 64 != 0).all()
        if run == 8192:
            assert (starts[1:-1] // 8192 != (starts[1:-1] + lens[1:-1] - 1) // 8192).all()   # (whole runs)
        _table_in_reference_order(px)
    elif kind == "distinct":
        assert len(np.unique(px)) == spec["u"] and n == spec["n"]
        assert (spec["u"], n) in ((6144, 6144), (6144, 131071), (6145, 6145))
    elif kind == "kcase":
        assert k in (64, 65) and n == 131071 and len(cols) <= 6144
    elif kind == "npix":
        assert n == spec["n"] and n in (131071, 131072) and 500 <= len(cols) <= 512
    elif kind == "one_colour":
        assert len(cols) == 1 and n == 131071
    elif kind == "few":
        assert len(cols) == spec["ncol"] < k
    elif kind == "ksmall":
        assert k in (1, 2) and len(cols) > 2
    elif kind == "fold":
        assert len(cols) == spec["u"] == len(we.oracle_table(px)[0])   # the root node's length
        if spec["pow2"]:
            assert _is_pow2(cnt) and _is_pow2([n])
            assert spec["u"] == 1 or len(np.unique(cnt)) > 1
        else:
            assert (cnt == 1).all() and n == spec["u"]
        assert k == 4
    elif kind == "tie":
        assert n == spec["n"] and n in (16384, 16385)
        low = px & np.uint32(0xFFFFFF) & ~np.uint32(0xC0C0C0)
        assert (low & ~np.uint32(0x010101 if spec["two"] else 0) == 0).all()   # the lattice (+ {0, 1}^3)
        ct = we.oracle_run(px, k)["ct"]
        assert len(ct) == spec["m"]
        if name.split("_n")[0] in ("tie_m1", "tie_m2", "tie_m16", "tie_m17", "tie_m16_topbyte"):
            assert spec["m"] in (1, 2, 16, 17) and 16 <= k <= 64
        if spec["m"] >= 2:
            s = ((ct >> 16) & 0xFF) + ((ct >> 8) & 0xFF) + (ct & 0xFF)
            assert len(np.unique(s)) < len(s)   # centres tie on R+G+B
        if name.split("_n")[0] in we.TIE_DENSE:
            assert _tied_pixels(px, ct) >= n // 100
    elif kind == "dedup":   # the first-occurrence dedup drops a centre, down to exactly 16 / 17 colours
        assert n == spec["n"] and n in (16384, 16385) and 16 <= k <= 64 and spec["m"] in (16, 17)
        ch = np.stack([(px >> 16) & 0xFF, (px >> 8) & 0xFF, px & 0xFF])
        assert ((ch & 0x3F) <= 2).all()   # the lattice plus {0, 1, 2}^3
        r = we.oracle_run(px, k)
        assert len(r["ct"]) == spec["m"] < r["k_raw"] <= k
        assert len(np.unique(r["ct"])) == len(r["ct"])
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("i", range(len(SPECS)), ids=NAMES)
def test_oracle_reproduces_the_reference_record(i):
    c = RECORDS[i]
    arrs = fx.load_npz("weighted3.npz")
    spec = c["spec"]
    px = we.build(spec)
    assert len(px) == c["n_px"]
    r = we.oracle_run(px, spec["k"])
    assert [int(v) for v in r["ct"]] == c["ct"] and len(r["ct"]) == c["k_out"]
    assert "%016x" % fx.fnv(r["out"]) == c["out_fnv"]
    assert np.array_equal(r["trace"], arrs["trace_%d" % i])
    assert we.filled_means_equal(r["means"], r["sizes"], arrs["means_%d" % i])
    if spec["k"] > 1:
        assert int(r["trace"][:, 2].sum()) == c["sum_split_sizes"]
