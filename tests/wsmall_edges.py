"""Case builders for the one-launch weighted kernel (dq_wsmall.hip) at the edges
of its own mechanisms: the reference's 20023 hash buckets (counting sort, 16-bit
counts two per word, the rank loop inside a bucket), the kernel's 8192-slot LDS
hash set, its four limits (131071 pixels, 6144 colours, K = 64, 16 mapped
colours), the first-occurrence dedup of its centres, the chunk lengths of its sequential folds (368 summands, 16- and
8-wide tails), the 1024-record steps of its partition, and its map (R+G+B ties,
the inline / second-launch boundary at 16384 pixels, the host map above 16
colours).

Shared by tests/test_wsmall_edges.py (CPU: every case's property, and the
oracle against the reference's records), tests/test_gpu_wsmall_edges.py and
tests/golden/make_golden.py (the `weighted3` records).  Inputs are rebuilt
from the spec; only specs and results are committed.

The two hash formulas are restated here from the sources they mirror:
  bucket(c) = (33023 R + 30013 G + 27011 B) % 20023      (calc_color_table's HASH)
  slot(c)   = ((c * 0x9E3779B1) mod 2^32) >> 19           (the kernel's LDS hash set)
"""
import ctypes
import functools

import numpy as np

import dq_fixtures as fx

N_BUCKETS = 20023
N_SLOTS = 8192
MAX_N = 131071        # the kernel's limits (dq_weighted.h)
MAX_U = 6144
MAX_K = 64
MAP_MAX = 16
MAP_INLINE = 16384
SLOT = 8190           # the probe chain of a crowded slot 8190 wraps past 8191 to 0

FOLD_COUNTS = [1, 7, 8, 9, 15, 16, 17, 367, 368, 369, 375, 376, 377, 735, 736, 737,
               1023, 1024, 1025, 2047, 2048, 2049]
BUCKET_PAIRS = [(19, 20), (1279, 1280), (10000, 10001)]   # scan thread | wave | one shared count word
RUNS = [(1, 0, 1500), (16, 7, 1500), (64, 37, 1500), (8192, 1000, 15)]   # (run length, roll, colours)
# lattice triples (mask 0xC0C0C0) whose channel permutations share R+G+B
TRIPLES = [(0, 64, 128), (64, 64, 192), (0, 128, 192), (64, 128, 192), (0, 0, 192), (128, 128, 192)]


def buckets_of(c):
    c = np.asarray(c).astype(np.int64) & 0xFFFFFF
    return (((c >> 16) & 255) * 33023 + ((c >> 8) & 255) * 30013 + (c & 255) * 27011) % N_BUCKETS


def slots_of(c):
    c = np.asarray(c).astype(np.uint64) & np.uint64(0xFFFFFF)
    return (((c * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _all_buckets():
    return buckets_of(np.arange(1 << 24, dtype=np.int64)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def fullest_bucket():
    return int(np.argmax(np.bincount(_all_buckets(), minlength=N_BUCKETS)))


def colours_of_buckets(bs):
    return np.nonzero(np.isin(_all_buckets(), np.asarray(bs, np.int32)))[0].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _slot_colours():
    return np.nonzero(slots_of(np.arange(1 << 24, dtype=np.int64)) == SLOT)[0].astype(np.uint32)


def first_occurrences(px):
    """(colours ascending, index of each one's first pixel, its pixel count) of the masked pixels."""
    return np.unique(np.asarray(px, np.uint32) & np.uint32(0xFFFFFF), return_index=True, return_counts=True)


def _distinct(rng, u):
    c = np.unique(rng.integers(0, 1 << 24, u + u // 8 + 64, dtype=np.uint32))
    assert len(c) >= u
    return rng.permutation(c)[:u].astype(np.uint32)


def _once_then_repeats(rng, cols, n):
    """Every colour once in shuffled order, then random repeats up to n pixels."""
    return np.concatenate([rng.permutation(cols), cols[rng.integers(0, len(cols), n - len(cols))]]).astype(np.uint32)


def _top_bytes(rng, px):
    return (px | (rng.integers(1, 256, len(px), dtype=np.uint32) << np.uint32(24))).astype(np.uint32)


def pow2_counts(rng, u):
    """u pixel counts, each a power of two, adding up to a power of two >= 4u."""
    total = 1
    while total < 4 * u:
        total *= 2
    if u == 1:
        return np.array([total], np.int64)
    cnt = np.ones(u, np.int64)
    left = total - u
    while left > 0:   # (every count and `left` are multiples of the smallest count: one always fits)
        fit = np.nonzero(cnt <= left)[0]
        i = int(fit[rng.integers(0, len(fit))])
        left -= int(cnt[i])
        cnt[i] *= 2
    return cnt


# Two sets of nine colours of a {0, 1, 2}^3 cube with their pixel counts.  Alone, the weighted clustering leaves
# clusters of which two round to one colour: the first at K = 4 (means (65, 64, 64) and (65.5, 64.5, 64) above a
# base of 64, the halves landing just below .5: it needs weights that are not powers of two), the second at
# K = 6 (means (64.5, 65.5, 64.5) and (65, 66, 65): exact halves round up).
DEDUP_GADGETS = [
    ([0x010000, 0x010100, 0x020201, 0x010002, 0x000102, 0x020000, 0x020200, 0x010201, 0x000202],
     [8, 2, 16, 2, 16, 2, 8, 2, 4], 4),
    ([0x000002, 0x000102, 0x000200, 0x020202, 0x020001, 0x010101, 0x010001, 0x010201, 0x000001],
     [1, 32, 2, 16, 4, 2, 1, 2, 32], 6),
]


def tie_colours(spec):
    """Channel permutations of the first `triples` lattice triples; with `two`
    each plus the offsets {0, 1}^3 (two values per channel around every base)."""
    bases = []
    for t in TRIPLES[:spec["triples"]]:
        for p in sorted(set([(t[0], t[1], t[2]), (t[0], t[2], t[1]), (t[1], t[0], t[2]),
                             (t[1], t[2], t[0]), (t[2], t[0], t[1]), (t[2], t[1], t[0])])):
            bases.append(p)
    cols = []
    for (r, g, b) in bases:
        for o in range(8 if spec["two"] else 1):
            cols.append(((r + (o >> 2)) << 16) | ((g + ((o >> 1) & 1)) << 8) | (b + (o & 1)))
    return np.array(cols, np.uint32)[:spec.get("ncol")]


def build(spec):
    """The pixels of a case (uint32, top byte clear unless spec['topbyte'])."""
    kind = spec["kind"]
    rng = np.random.default_rng(spec["seed"])
    if kind == "bucket_fullest":
        cols = colours_of_buckets([fullest_bucket()])
        px = _once_then_repeats(rng, cols, len(cols) + 60000)
    elif kind in ("bucket_only", "bucket_pair"):
        cols = colours_of_buckets(spec["buckets"])
        px = _once_then_repeats(rng, cols, len(cols) + 3000)
    elif kind == "bucket_order":
        cols = np.sort(colours_of_buckets([fullest_bucket()]))[100:105]
        order = {"asc": [0, 1, 2, 3, 4], "desc": [4, 3, 2, 1, 0], "mixed": [2, 0, 4, 1, 3]}[spec["order"]]
        others = np.setdiff1d(_distinct(rng, 24), cols)[:20]
        pool = np.concatenate([cols, others])
        px = np.concatenate([cols[order], pool[rng.integers(0, len(pool), 400)]])
    elif kind == "last_pixel_first":
        px = rng.integers(0, 1 << 24, MAX_N, dtype=np.uint32) & np.uint32(0xE0E0E0)
        px[-1] = 0x010203
    elif kind == "slot_runs":
        cols = rng.permutation(_slot_colours())[:spec["ncol"]]
        px = np.roll(np.repeat(cols, spec["run"]), spec["roll"])
    elif kind == "distinct":
        px = _once_then_repeats(rng, _distinct(rng, spec["u"]), spec["n"])
    elif kind == "kcase":
        px = _once_then_repeats(rng, _distinct(rng, 6000), MAX_N)
    elif kind == "npix":
        px = rng.integers(0, 1 << 24, spec["n"], dtype=np.uint32) & np.uint32(0xE0E0E0)
    elif kind == "one_colour":
        px = np.full(MAX_N, 0x6B8E23, np.uint32)
    elif kind == "few":
        px = _once_then_repeats(rng, np.array([0x204060, 0xC08040, 0x40C0A0], np.uint32)[:spec["ncol"]], 97)
    elif kind == "ksmall":
        px = _once_then_repeats(rng, _distinct(rng, 300), 5000)
    elif kind == "fold":
        cols = _distinct(rng, spec["u"])
        px = rng.permutation(np.repeat(cols, pow2_counts(rng, spec["u"]))) if spec["pow2"] else cols
    elif kind == "tie":
        cols = tie_colours(spec)
        # skewed counts: colour i about 2^-(i % skew) as frequent as the first
        p = 0.5 ** (rng.permutation(len(cols)) % spec["skew"])
        draw = cols[rng.choice(len(cols), MAP_INLINE + 1, p=p / p.sum())]
        px = np.concatenate([cols, draw])[:spec["n"]]   # (the 16385-pixel case is the 16384-pixel one plus a pixel)
    elif kind == "dedup":
        # a DEDUP_GADGETS entry at one lattice colour (mask 0xC0C0C0), `fillers` other lattice colours around it, every
        # count a power of two but the last filler's, which takes what is left of n
        lat = rng.permutation(64)[:spec["fillers"] + 1]
        lat = (((lat >> 4) & 3) << 22) | (((lat >> 2) & 3) << 14) | ((lat & 3) << 6)
        cols = np.concatenate([lat[0] + np.array(DEDUP_GADGETS[spec["gadget"]][0], np.int64), lat[1:]]).astype(np.uint32)
        cnt = np.concatenate([np.array(DEDUP_GADGETS[spec["gadget"]][1], np.int64) << int(rng.integers(0, 4)),
                              1 << rng.integers(3, 10, spec["fillers"])])
        cnt[-1] = spec["n"] - cnt[:-1].sum()
        assert cnt[-1] > 0
        px = rng.permutation(np.repeat(cols, cnt))
    else:
        raise ValueError(kind)
    px = np.ascontiguousarray(px, np.uint32)
    if spec.get("topbyte"):
        px = _top_bytes(rng, px)
    return px


def _s(name, kind, k, seed, **kw):
    return dict(name=name, kind=kind, k=k, seed=seed, **kw)


def _tie(name, n, v, **kw):
    (k, seed, triples, two, skew, m, ncol) = v
    if ncol:
        kw["ncol"] = ncol
    return _s("%s_n%d" % (name, n), "tie", k, seed, n=n, triples=triples, two=two, skew=skew, m=m, **kw)


# name -> (K, seed, triples, two-valued offsets, skew, deduped colours m, colours kept).  m = 1 and 2 are one
# and two colours (15 and 14 empty clusters: a drop to those values is not reachable at K >= 16); here 16 and 17
# are K = m centres that tie on R+G+B.  The cases in which the first-occurrence dedup brings a larger raw count
# down to 16 and 17 are DEDUP_VARIANTS.
TIE_VARIANTS = {
    "tie_m1": (16, 1, 1, False, 1, 1, 1),
    "tie_m2": (16, 2, 1, False, 1, 2, 2),
    "tie_m16": (16, 1, 3, True, 4, 16, 0),
    "tie_m17": (17, 1, 3, True, 4, 17, 0),
    "tie_lattice": (6, 3, 6, False, 2, 6, 0),
}
TIE_DENSE = ("tie_m16", "tie_m17", "tie_lattice")   # cases whose pixels sit at equal distance from two centres


# name -> (gadget, fillers, seed, K, deduped colours m): the raw count is m + 1
DEDUP_VARIANTS = {
    "dedup_m16": (1, 11, 0, 17, 16),
    "dedup_m17": (1, 12, 0, 18, 17),
}


def _dedup(name, n, v):
    (gadget, fillers, seed, k, m) = v
    return _s("%s_n%d" % (name, n), "dedup", k, seed, n=n, gadget=gadget, fillers=fillers, m=m)


def case_specs():
    s = [_s("bucket_fullest", "bucket_fullest", 8, 101)]
    s += [_s("bucket_%d" % b, "bucket_only", 4, 110 + i, buckets=[b]) for i, b in enumerate((0, N_BUCKETS - 1))]
    s += [_s("bucket_pair_%d_%d" % p, "bucket_pair", 4, 120 + i, buckets=list(p)) for i, p in enumerate(BUCKET_PAIRS)]
    s += [_s("bucket_order_" + o, "bucket_order", 4, 130 + i, order=o) for i, o in enumerate(("asc", "desc", "mixed"))]
    s += [_s("last_pixel_first", "last_pixel_first", 4, 140)]
    s += [_s("slot_runs_%d" % r, "slot_runs", 4, 150 + i, run=r, roll=ro, ncol=nc) for i, (r, ro, nc) in enumerate(RUNS)]
    s += [_s("u6144_n6144", "distinct", 4, 160, u=MAX_U, n=MAX_U),
          _s("u6144_n131071", "distinct", 4, 161, u=MAX_U, n=MAX_N),
          _s("u6145", "distinct", 4, 162, u=MAX_U + 1, n=MAX_U + 1),
          _s("k64", "kcase", 64, 163), _s("k65", "kcase", 65, 163),
          _s("n131071", "npix", 4, 164, n=MAX_N), _s("n131072", "npix", 4, 164, n=MAX_N + 1),
          _s("one_colour_n131071", "one_colour", 4, 165)]
    s += [_s("k_above_%d_colours" % c, "few", 4, 170 + c, ncol=c) for c in (1, 2, 3)]
    s += [_s("k1", "ksmall", 1, 175), _s("k2", "ksmall", 2, 175)]
    for p2 in (False, True):
        s += [_s("fold_%d%s" % (u, "_pow2" if p2 else ""), "fold", 4, 1000 + u + (5000 if p2 else 0), u=u, pow2=p2)
              for u in FOLD_COUNTS]
    for n in (MAP_INLINE, MAP_INLINE + 1):
        s += [_tie(name, n, v) for name, v in TIE_VARIANTS.items()]
    for n in (MAP_INLINE, MAP_INLINE + 1):
        s += [_dedup(name, n, v) for name, v in DEDUP_VARIANTS.items()]
    s.append(_dedup("dedup_inexact_m16", MAP_INLINE + 1, (0, 13, 1, 17, 16)))   # (the gadget of inexact weights)
    s.append(_s("topbyte_table", "bucket_pair", 4, 180, buckets=[19, 20], topbyte=True))
    s.append(_tie("tie_m16_topbyte", MAP_INLINE + 1, TIE_VARIANTS["tie_m16"], topbyte=True))
    return s


def spec_by_name():
    return {s["name"]: s for s in case_specs()}


def takes_kernel(spec, px):
    """The limits: whether the one-launch kernel holds the case (else the multi-kernel rounds)."""
    return len(px) <= MAX_N and spec["k"] <= MAX_K and len(first_occurrences(px)[0]) <= MAX_U


LIMIT_CASES = ["u6144_n6144", "u6144_n131071", "u6145", "k64", "k65", "n131071", "n131072", "one_colour_n131071",
               "k_above_1_colours", "k_above_2_colours", "k_above_3_colours", "k1", "k2"]


# ---------------------------------------------------------------------------
# The oracle, composed as the kernel is: colour table, weighted clustering at
# max_iters, first-occurrence dedup, map.
def oracle_table(px):
    px = np.ascontiguousarray(px, np.uint32)
    col = np.zeros(len(px), np.uint32)
    w = np.zeros(len(px), np.float64)
    u = fx.oracle().dqo_color_table(ctypes.c_uint32(len(px)), fx.vp(px), fx.vp(col), fx.vp(w))
    return col[:u].copy(), w[:u].copy()


def oracle_run(px, k, max_iters=10):
    orc = fx.oracle()
    px = np.ascontiguousarray(px, np.uint32)
    col, w = oracle_table(px)
    raw = np.zeros(k, np.uint32)
    kk = ctypes.c_uint32(k)
    means = np.zeros((k, 3), np.float64)
    sizes = np.zeros(k, np.int64)
    trace = np.zeros((max(k - 1, 1), 4), np.int64)
    orc.dqo_cluster_weighted(ctypes.c_uint32(len(col)), fx.vp(col), fx.vp(w), ctypes.byref(kk), fx.vp(raw),
                             ctypes.c_int(max_iters), fx.vp(means), fx.vp(sizes), fx.vp(trace))
    raw = raw[:kk.value]
    ct = []
    for c in raw:   # first-occurrence dedup (quant_util.cpp:93-118)
        if int(c) not in ct:
            ct.append(int(c))
    ct = np.array(ct, np.uint32)
    out = np.zeros(len(px), np.uint32)
    orc.dqo_map(fx.vp(px), ctypes.c_uint32(len(px)), fx.vp(out), fx.vp(ct), ctypes.c_int(len(ct)))
    return {"nu": len(col), "k_raw": len(raw), "ct": ct, "out": out, "trace": trace[:k - 1].copy(),
            "means": means, "sizes": sizes}


def filled_means_equal(means, sizes, ref_means):
    """As test_gpu_parity._check_centroids: the reference records mean[ic] of
    non-empty clusters only (NaN elsewhere); those are compared bit for bit."""
    filled = ~np.isnan(ref_means[:, 0])
    return bool(np.array_equal(filled, np.asarray(sizes) > 0) and
                np.array_equal(np.ascontiguousarray(means[filled]).view(np.uint64),
                               np.ascontiguousarray(ref_means[filled]).view(np.uint64)))
