"""Shared fixture helpers for tests/, tests/golden/make_golden.py and bench.py.

Test infrastructure: the input generators, the hash and the golden-file I/O.
The xorshift generator and the FNV hash run in C (oracle/_build/libdqoracle.so,
``dqo_xorshift_fill`` / ``dqo_fnv1a64``) because the big configs have 10^7-10^8
pixels.  Nothing here reads /root/reference at run time (the GPU box has none).
"""
import ctypes
import json
import os

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, "golden")
ORACLE_SO = os.path.join(ROOT, "oracle", "_build", "libdqoracle.so")
SEED = 0x9E3779B97F4A7C15

_orc = None


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def oracle():
    """Load (building if needed) the CPU restatement -- the checker."""
    global _orc
    if _orc is None:
        if not os.path.exists(ORACLE_SO):
            import subprocess
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "port"])
        lib = ctypes.CDLL(ORACLE_SO)
        lib.dqo_fnv1a64.restype = ctypes.c_uint64
        lib.dqo_cluster.restype = ctypes.c_int
        lib.dqo_quant_recurse.restype = ctypes.c_int
        _orc = lib
    return _orc


def xorshift(n, seed=SEED):
    out = np.empty(n, np.uint32)
    oracle().dqo_xorshift_fill(vp(out), ctypes.c_uint64(n), ctypes.c_uint64(seed))
    return out


def fnv(a):
    a = np.ascontiguousarray(a, np.uint32)
    return int(oracle().dqo_fnv1a64(vp(a), ctypes.c_uint64(a.size)))


def labels_of(out, ct):
    """Index of each output colour in the colortable (colours are unique after dedup)."""
    lut = {int(c): i for i, c in enumerate(ct)}
    return np.array([lut[int(v)] for v in out], np.int32)


def dump_json(name, obj):
    with open(os.path.join(GOLDEN, name), "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def load_npz(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


# --------------------------------------------------------------------------
# Test/DivQuantTest.m inputs, restated (the 7 known-answer tests).
def kat_inputs():
    gray10 = np.array([(i * 25) * 0x010101 for i in range(10)], np.uint32)  # :33-46 step=(255-0)/10
    umbrella = np.array([0xEBC58B, 0xDAD4E7, 0xD7779D, 0x7E393D, 0xABA4BA, 0xCF4B53,
                         0xC49AC7, 0xAC7292, 0xECEFE7, 0xDC789D, 0xA8ABC4, 0x906E9E,
                         0xB54748, 0xA24F44, 0x857E77, 0x7F654B], np.uint32)  # :219-235
    return {
        "testQuantN1": (gray10, 1),                                   # :31-64
        "testQuantN2": (gray10, 2),                                   # :66-101
        "testQuantN3": (gray10, 3),                                   # :103-142
        "testQuantN3N2": (np.array([0x8DC63F, 0xF26522], np.uint32), 3),  # :147-178
        "testQuantGray2": (np.array([0x0A0A0A, 0xF5F5F5], np.uint32), 2),  # :182-213
        "testQuant_4x4_N4": (umbrella, 4),                            # :218-258
        "testQuant_4x4_N16": (umbrella, 16),                          # :263-319
    }


# Colortables the XCTest asserts literally (Test/DivQuantTest.m line cited).
KAT_EXPECTED = {
    "testQuantN1": [0x000000],                                        # :60-61
    "testQuantN2": [0x323232, 0xAFAFAF],                              # :95-98
    "testQuantN3": [0x191919, 0xAFAFAF, 0x585858],                    # :135-139
    "testQuantN3N2": [0xF26522, 0x8DC63F],                            # :172-175
    "testQuantGray2": [0x0A0A0A, 0xF5F5F5],                           # :207-210
    "testQuant_4x4_N4": [0xA14D48, 0xC292B3, 0xE6D8C8, 0x96758D],      # :251-255
    "testQuant_4x4_N16": [0x7E393D, 0xD7779D, 0xEBC58B, 0x857E77, 0xDAD4E7, 0xABA4BA,
                          0xA24F44, 0xAC7292, 0xCF4B53, 0x7F654B, 0x906E9E, 0xC49AC7,
                          0xECEFE7, 0xB54748, 0xA8ABC4, 0xDC789D],    # :296-316
}


# --------------------------------------------------------------------------
# Small synthetic cases: (n, k, kind, seed).  Inputs are regenerated from the
# spec so only the spec and the expected outputs are committed.
def small_case_specs():
    specs = []
    sizes_k = [(1, 1), (1, 4), (2, 2), (3, 16), (10, 3), (50, 7), (257, 16), (1000, 16),
               (1000, 64), (4099, 256), (4099, 300), (777, 1024), (20000, 256),
               (70001, 32), (65536, 16)]
    kinds = ["uniform", "ties", "gray", "clustered", "coarse", "topbyte"]
    for i, (n, k) in enumerate(sizes_k):
        for j, kind in enumerate(kinds):
            if n > 20000 and kind not in ("uniform", "clustered", "coarse"):
                continue
            specs.append({"n": n, "k": k, "kind": kind, "seed": 1000 + 17 * i + j})
    return specs


def make_case(spec):
    n, kind, seed = spec["n"], spec["kind"], spec["seed"]
    r = xorshift(n, seed=SEED ^ (seed * 0x100000001B3))
    if kind == "uniform":
        return r
    if kind == "topbyte":            # bits 24-31 must be ignored everywhere
        return r | ((xorshift(n, seed=seed) & 0xFF) << 24).astype(np.uint32)
    if kind == "ties":               # 4 colours, many exact duplicates
        pal = np.array([0x3F3F3F, 0x7E7E7E, 0x123456, 0x563412], np.uint32)
        return pal[r % 4]
    if kind == "gray":
        return ((r & 0xFF) * 0x010101).astype(np.uint32)
    if kind == "clustered":          # 5 centres +- 8 noise per channel
        cen = np.array([[20, 30, 40], [200, 10, 90], [128, 128, 128], [250, 240, 230], [60, 200, 60]])
        c = cen[r % 5]
        noise = np.stack([(r >> 8) & 15, (r >> 12) & 15, (r >> 16) & 15], 1).astype(np.int64) - 8
        v = np.clip(c + noise, 0, 255).astype(np.uint32)
        return (v[:, 0] << 16) | (v[:, 1] << 8) | v[:, 2]
    if kind == "coarse":             # 3 bits per channel: heavy ties on every axis
        return (r & 0xE0E0E0).astype(np.uint32)
    raise ValueError(kind)


# --------------------------------------------------------------------------
# Palettes for the map_colors_mps-only fixtures.
def map_palette_specs():
    specs = []
    for k in (1, 2, 3, 5, 16, 64, 255, 256, 1024):
        specs.append({"k": k, "kind": "random", "seed": 77 + k})
    for k in (2, 7, 33, 256, 1000):
        specs.append({"k": k, "kind": "sametsum", "seed": 91 + k})
    for k in (4, 40, 300):
        specs.append({"k": k, "kind": "dups", "seed": 5 + k})
    specs.append({"k": 125, "kind": "subdivided", "seed": 0})
    specs.append({"k": 64, "kind": "gray", "seed": 3})
    return specs


def subdivided_colors():
    """getSubdividedColors (superpixels/OpenCVUtil.cpp:853-897): 5^3 colours, alpha 0xFF."""
    vals = [0, 63, 127, 191, 255]
    return np.array([(0xFF << 24) | (r << 16) | (g << 8) | b
                     for r in vals for g in vals for b in vals], np.uint32)


def make_palette(spec):
    k, kind = spec["k"], spec["kind"]
    r = xorshift(max(k, 1) * 4, seed=SEED + 1 + spec["seed"])
    if kind == "random":
        return r[:k].copy()
    if kind == "sametsum":           # many entries share R+G+B -> std::sort tie order matters
        s = (r[:k] % 5) * 60 + 90
        a = np.minimum(r[k:2 * k] % 256, s)
        b = np.minimum((r[2 * k:3 * k] % 256), s - a)
        c = s - a - b
        ok = c <= 255
        c = np.where(ok, c, 255)
        return ((a << 16) | (b << 8) | c).astype(np.uint32)
    if kind == "dups":
        base = r[:max(1, k // 4)]
        return base[r[k:2 * k] % len(base)].astype(np.uint32)
    if kind == "subdivided":
        return subdivided_colors()
    if kind == "gray":
        return (((r[:k] & 0xFF)) * 0x010101).astype(np.uint32)
    if kind == "lattice":            # every multiple of `step` per channel: midpoints tie 2-, 4-, 8-way
        v = np.arange(0, 256, spec["step"], dtype=np.uint32)
        assert len(v) ** 3 == k
        return ((v[:, None, None] << 16) | (v[None, :, None] << 8) | v[None, None, :]).reshape(-1)
    if kind == "cube":               # side^3 entries of step 2 from 100: a few cells hold them all
        v = (100 + 2 * np.arange(spec["side"])).astype(np.uint32)
        assert len(v) ** 3 == k and v[-1] < 256
        return ((v[:, None, None] << 16) | (v[None, :, None] << 8) | v[None, None, :]).reshape(-1)
    if kind == "cluster":            # k distinct colours of ONE 8x8x8 cell: that cell has exactly k candidates
        assert k <= 512
        q = xorshift(3 + 512, seed=SEED + 1 + spec["seed"])
        o = np.argsort(q[3:], kind="stable")[:k].astype(np.uint32)
        c = (q[:3] % 32) * 8
        return (((c[0] + (o >> 6)) << 16) | ((c[1] + ((o >> 3) & 7)) << 8) | (c[2] + (o & 7))).astype(np.uint32)
    raise ValueError(kind)


# --------------------------------------------------------------------------
# Tie-dense map fixtures (map2.json): palettes whose midpoints are exact
# distance ties, palettes at the map's candidate-count thresholds (3 compact
# inline, 7 inline, 32 per-cell cap) and palettes above 1024 entries (the
# second map kernel, u16 region lists), mapped on probe pixels built from the
# palette itself.
def map2_palette_specs():
    specs = [{"k": 512, "kind": "lattice", "step": 32, "seed": 0},
             {"k": 4096, "kind": "lattice", "step": 16, "seed": 0},
             {"k": 1000, "kind": "cube", "side": 10, "seed": 0},
             {"k": 4096, "kind": "cube", "side": 16, "seed": 0}]
    for k in (3, 4, 7, 8, 9, 32, 33, 40):
        specs.append({"k": k, "kind": "cluster", "seed": 300 + k})
    for k in (1025, 4096, 16384):
        specs.append({"k": k, "kind": "random", "seed": 77 + k})
    specs.append({"k": 16384, "kind": "sametsum", "seed": 91 + 16384})
    specs.append({"k": 2048, "kind": "dups", "seed": 5 + 2048})
    specs.append({"k": 125, "kind": "subdivided", "seed": 0})
    specs.append({"k": 2, "kind": "gray", "seed": 3})
    return specs


def map2_cube_specs():
    """Palettes mapped over all 2^24 colours (np.arange(1 << 24))."""
    return [{"k": 125, "kind": "subdivided", "seed": 0}, {"k": 16, "kind": "random", "seed": 77 + 16}]


def map2_seed(spec):
    return 40000 + 131 * spec["k"] + 7 * spec["seed"] + len(spec["kind"])


def _channels(p):
    return (p >> 16) & 0xFF, (p >> 8) & 0xFF, p & 0xFF


def _midpoints(a, b):
    """Per-channel floor midpoint of colour pairs."""
    ca, cb = _channels(a.astype(np.uint32)), _channels(b.astype(np.uint32))
    m = [(x + y) >> 1 for x, y in zip(ca, cb)]
    return ((m[0] << 16) | (m[1] << 8) | m[2]).astype(np.uint32)


MAP_PROBE_PAIRS = 12000   # random-pair midpoints: the first of part (ii)


def map_probe_parts(pal, seed):
    """The parts of map_probe_pixels, top byte clear: (i) every palette entry,
    (ii) midpoints of MAP_PROBE_PAIRS random entry pairs, then of the pairs
    adjacent in R+G+B order (at most 8000), (iii) the 8 corners of 1000 cells,
    (iv) uniform pixels."""
    pal = np.ascontiguousarray(pal, np.uint32) & np.uint32(0xFFFFFF)
    k = len(pal)
    r = xorshift(2 * MAP_PROBE_PAIRS + 3000, seed=SEED ^ (seed * 0x100000001B3))
    a, b = pal[r[:MAP_PROBE_PAIRS] % k], pal[r[MAP_PROBE_PAIRS:2 * MAP_PROBE_PAIRS] % k]
    ch = _channels(pal)
    by_sum = pal[np.argsort((ch[0] + ch[1] + ch[2]).astype(np.int64), kind="stable")]
    adj = _midpoints(by_sum[:-1], by_sum[1:])[:8000]
    c = (r[2 * MAP_PROBE_PAIRS:] % 32).reshape(1000, 3) * 8
    corners = []
    for m in range(8):
        x = [c[:, i] + (7 if (m >> i) & 1 else 0) for i in range(3)]
        corners.append((x[0] << 16) | (x[1] << 8) | x[2])
    corners = np.stack(corners, 1).reshape(-1).astype(np.uint32)
    return {"entries": pal.copy(), "mid": np.concatenate([_midpoints(a, b), adj]), "corners": corners,
            "uniform": xorshift(20000, seed=seed + 1)}


def map_probe_pixels(pal, seed):
    """Probe pixels of a palette: map_probe_parts concatenated, more uniform
    pixels up to a length = 5 (mod 8) (ragged for the 8-pixel groups), and
    (v) a garbage top byte in every pixel (the map ignores bits 24-31)."""
    parts = map_probe_parts(pal, seed)
    px = np.concatenate([parts["entries"], parts["mid"], parts["corners"], parts["uniform"]])
    pad = (5 - len(px)) % 8
    px = np.concatenate([px, xorshift(pad + 1, seed=seed + 2)[:pad]])
    assert len(px) % 8 == 5
    return (px | ((xorshift(len(px), seed=seed + 3) & 0xFF) << 24)).astype(np.uint32)


# --------------------------------------------------------------------------
def load_png_u32(path):
    """Decode like OpenCV imread(IMREAD_COLOR) + Vec3BToUID (OpenCVUtil.h:19-27):
    alpha dropped, pixel = R<<16 | G<<8 | B."""
    from PIL import Image
    im = Image.open(path).convert("RGB")
    a = np.asarray(im, dtype=np.uint32)
    px = (a[:, :, 0] << 16) | (a[:, :, 1] << 8) | a[:, :, 2]
    return np.ascontiguousarray(px.reshape(-1), np.uint32), im.width, im.height


# --------------------------------------------------------------------------
# Weighted-path (allPixelsUnique=0) cases: duplicate-heavy inputs where the
# reference's weighted FP64 folds and the uniform-weight integer sums often
# decide differently (near-tie TSEs, cuts, 2-means planes), and image regions
# like the app's per-region calls (ClusteringSegmentation.cpp:1779-1803, K=4).
def weighted_case_specs():
    specs = []
    kinds = ["fewcolours", "greyramp", "tight", "coarse"]
    ks = [1, 2, 3, 4, 5, 8, 16, 64]
    for i in range(320):
        n = 1 + (int(xorshift(1, seed=0xA5A5 + i)[0]) % 3000)
        specs.append({"n": n, "k": ks[i % len(ks)], "kind": kinds[i % 4], "seed": 5000 + i})
    for i, (name, k) in enumerate([(nm, k) for nm in ("batman", "cookie") for k in (2, 4, 8, 16)]):
        for j in range(4):
            specs.append({"n": 0, "k": k, "kind": "crop_" + name, "seed": 7000 + 10 * i + j})
    return specs


def make_weighted_case(spec):
    n, kind, seed = spec["n"], spec["kind"], spec["seed"]
    if kind.startswith("crop_"):   # a rectangle of a sample image, 1K..40K pixels
        px, w, h = load_png_u32(os.path.join(GOLDEN, "png", kind[5:] + ".png"))
        r = xorshift(4, seed=seed)
        cw, ch = 16 + int(r[0]) % 200, 16 + int(r[1]) % 200
        x0, y0 = int(r[2]) % (w - cw), int(r[3]) % (h - ch)
        return np.ascontiguousarray(px.reshape(h, w)[y0:y0 + ch, x0:x0 + cw].reshape(-1))
    r = xorshift(4 * n + 64, seed=seed)
    if kind == "fewcolours":   # a small palette, skewed counts (geometric-like)
        ncol = 2 + int(r[0]) % 38
        pal = r[1:1 + ncol]
        sel = np.minimum(np.log2(1 + (r[64:64 + n] & 0xFFFF)).astype(np.int64), ncol - 1)
        return pal[sel].astype(np.uint32)
    if kind == "greyramp":
        return (((r[64:64 + n] % 32) * 8) * 0x010101).astype(np.uint32)
    if kind == "tight":        # one cluster, +-3 per channel
        base = np.array([60 + int(r[0]) % 140, 60 + int(r[1]) % 140, 60 + int(r[2]) % 140], np.int64)
        d = np.stack([r[64:64 + n] % 7, (r[64:64 + n] >> 8) % 7, (r[64:64 + n] >> 16) % 7], 1).astype(np.int64) - 3
        c = np.clip(base + d, 0, 255).astype(np.uint32)
        return (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    if kind == "coarse":
        return (r[64:64 + n] & 0xC0C0C0).astype(np.uint32)
    raise ValueError(kind)


# --------------------------------------------------------------------------
# quant_varpart_fast's cut_bits / decimation paths (DivQuantCluster.cpp:1130-
# 1146): num_bits < 8 and/or dec_factor > 1, either flag value.
# Frame shapes keep the reference's numRows-stride index (calc_color_table
# :124) inside the buffer: rows == 1, or rows <= cols.
def varpart_case_specs():
    specs = []
    shapes = [(1, 4096), (64, 64), (48, 80), (1, 3001), (33, 57), (128, 128)]
    kinds = ["uniform", "crop_batman", "crop_cookie", "fewcolours", "tight", "greyramp"]
    ks = [1, 2, 4, 16, 64, 256]
    i = 0
    for nb in range(1, 9):
        for dec in (1, 2, 3, 5):
            for uniq in (0, 1):
                if nb == 8 and dec == 1:
                    continue   # the plain paths (cases / weighted fixtures)
                rows, cols = shapes[i % len(shapes)]
                specs.append({"rows": rows, "cols": cols, "num_bits": nb, "dec": dec, "uniq": uniq,
                              "k": ks[(i * 7) % len(ks)], "kind": kinds[i % len(kinds)], "seed": 9000 + i,
                              "max_iters": 10 if i % 5 else 3})
                i += 1
    return specs


def make_varpart_case(spec):
    n = spec["rows"] * spec["cols"]
    kind = spec["kind"]
    if kind == "uniform":
        return xorshift(n, seed=spec["seed"])
    if kind.startswith("crop_"):
        px, w, h = load_png_u32(os.path.join(GOLDEN, "png", kind[5:] + ".png"))
        r = xorshift(2, seed=spec["seed"])
        x0, y0 = int(r[0]) % (w - 128), int(r[1]) % (h - 128)
        crop = px.reshape(h, w)[y0:y0 + 128, x0:x0 + 128].reshape(-1)
        return np.ascontiguousarray(crop[:n])
    return make_weighted_case({"n": n, "kind": kind, "seed": spec["seed"]})
