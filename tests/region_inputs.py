"""The named frames and maps of the region-map suites and of tools/*_ab.py: every
builder that more than one file uses.  Each is a pure function of its
arguments; the cached ones return read-only arrays.  test_region_inputs.py pins
every input the suites build to its sha256."""
import functools

import numpy as np

import dq_fixtures as fx
from adjacency_model import edges_model
from pixels_model import rows_total
from regions_model import regions_model


@functools.lru_cache(maxsize=None)
def frame(w, h):
    px = fx.xorshift(w * h, seed=fx.SEED + 77)   # 0x00RRGGBB
    px.setflags(write=False)
    return px


def noise(w, h, k, seed=0, dtype=np.uint32):
    return (fx.xorshift(w * h, seed=fx.SEED + seed) % np.uint32(k)).astype(dtype).reshape(h, w)


# ---------------------------------------------------------------------------
# Connected regions.  Patterns: (h, w) maps of small non-negative integers.
def spiral(w, h):
    a = np.zeros((h, w), np.int64)
    x = y = d = 0
    a[0, 0] = 1
    dirs = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    inside = lambda px, py: 0 <= px < w and 0 <= py < h  # noqa: E731
    while True:
        for _ in range(2):
            dx, dy = dirs[d]
            nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(nx, ny) and a[ny, nx] == 0 and (not inside(ax, ay) or a[ay, ax] == 0):
                x, y = nx, ny
                a[y, x] = 1
                break
            d = (d + 1) % 4
        else:
            return a


def regions_pattern(name, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    if name == "constant":
        return np.full((h, w), 5, np.int64)
    if name == "checker":
        return ((xs + ys) & 1).astype(np.int64)
    if name == "hstripes":
        return (ys & 1).astype(np.int64)
    if name == "vstripes":
        return (xs & 1).astype(np.int64)
    if name == "spiral":
        return spiral(w, h)
    if name == "comb":      # teeth on the even columns, joined along the last row
        return (((xs & 1) == 0) | (ys == h - 1)).astype(np.int64)
    if name == "rings":
        return ((np.maximum(abs(xs - w // 2), abs(ys - h // 2)) // 3) & 1).astype(np.int64)
    if name == "diagonals":  # x == y passes (T-1, T-1) -> (T, T); x + y == 2T - 1 passes (T, T-1) -> (T-1, T)
        return np.where((xs - ys) % 8 == 0, 1, np.where((xs + ys) % 8 == 7, 2, 0)).astype(np.int64)
    if name.startswith("noise"):
        return noise(w, h, int(name[5:]), dtype=np.int64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def regions_base(name, w, h):
    a = regions_pattern(name, w, h)
    a.setflags(write=False)
    return a


def widen(base, width):
    """The pattern as a label map of `width` bytes through an injective table."""
    b = base.astype(np.uint32)
    assert b.max() < 256
    if width == 1:
        return b.astype(np.uint8)
    if width == 2:
        return (b * 257 + 300).astype(np.uint16)            # 300 .. 65535
    return ((b << 24) | np.uint32(0x00ABCDEF)).astype(np.uint32)   # differ only in the top byte


# ---------------------------------------------------------------------------
# Adjacency.  Maps: (h, w) arrays of uint32 ids.
def adjacency_map(name, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    n = w * h
    if name == "arange":
        return np.arange(n, dtype=np.uint32).reshape(h, w)
    if name == "reversed":      # a > b at p < q everywhere
        return np.arange(n, dtype=np.uint32)[::-1].reshape(h, w).copy()
    if name == "permutation":
        return np.argsort(fx.xorshift(n, seed=fx.SEED + 5), kind="stable").astype(np.uint32).reshape(h, w)
    if name == "halves":
        return (xs >= w // 2).astype(np.uint32)
    if name == "quadrants":
        return ((xs >= w // 2) + 2 * (ys >= h // 2)).astype(np.uint32)
    if name == "vstripes":      # one edge, a run of right-contacts across every wave
        return (xs & 1).astype(np.uint32)
    if name == "k4":            # [[0, 1], [2, 3]] tiled: K4 at every corner, crossing diagonals
        return ((xs & 1) + 2 * (ys & 1)).astype(np.uint32)
    if name == "checker":       # 8-connectivity diagonals join equal ids: no contact
        return ((xs + ys) & 1).astype(np.uint32)
    if name == "constant":
        return np.full((h, w), 7, np.uint32)
    if name == "huge_ids":      # ids up to 0xFFFFFFFE (no degree array is possible)
        return (noise(w, h, 5, seed=9) + np.uint32(0xFFFFFFFA)).astype(np.uint32)
    if name.startswith("noise"):
        return noise(w, h, int(name[5:]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def adjacency_base(name, w, h):
    a = adjacency_map(name, w, h)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------
# Merge.  A label map, its frame, the model's regions and edges.
def merge_labels_and_frame(name):
    """(labels2d, frame, connectivity) of a named case."""
    if name == "noise64x48":
        return noise(64, 48, 4, seed=1), frame(64, 48), 8
    if name == "noise96x80":
        return noise(96, 80, 4, seed=1), frame(96, 80), 4
    if name == "noise97x41":
        return noise(97, 41, 3, seed=1), frame(97, 41), 8
    if name == "chain":         # every pixel its own region, one colour: every distance 0
        return np.arange(2048, dtype=np.uint32).reshape(1, 2048), np.full(2048, 0x00406080, np.uint32), 8
    if name == "islands":       # background 0, a one-pixel island at every even (x, y) of 64 x 64
        ys, xs = np.mgrid[0:64, 0:64]
        island = (xs % 2 == 0) & (ys % 2 == 0)
        lab = np.where(island, 1 + (ys // 2) * 32 + xs // 2, 0).astype(np.uint32)
        px = np.where(island.reshape(-1), frame(64, 64), np.uint32(0x00102030)).astype(np.uint32)
        return lab, px, 8
    if name == "stripes":       # 16 vertical stripes 4 wide; 2i and 2i + 1 are 1 level apart, pairs 30 apart
        ys, xs = np.mgrid[0:12, 0:64]
        lab = (xs // 4).astype(np.uint32)
        level = 30 * (lab // 2) + (lab % 2)      # <= 211
        return lab, (level * np.uint32(0x010101)).astype(np.uint32).reshape(-1), 4
    if name == "one":
        return np.zeros((5, 7), np.uint32), frame(7, 5), 8
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def merge_inputs(name):
    lab, px, connectivity = merge_labels_and_frame(name)
    h, w = lab.shape
    reg, st = regions_model(lab, connectivity, px)
    inp = dict(st, w=w, h=h, connectivity=connectivity, labels=lab, pixels=px, regions=reg,
               edges=edges_model(reg, w, h, connectivity), R=len(st["area"]))
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp


# ---------------------------------------------------------------------------
# Pixel lists.
def permuted(reg2d, seed):
    R = int(reg2d.max()) + 1
    perm = np.argsort(fx.xorshift(R, seed=fx.SEED + seed), kind="stable").astype(np.uint32)
    return perm[reg2d]


@functools.lru_cache(maxsize=None)
def pixels_map(name):
    """(region ids (H, W) uint32, R) of a named case."""
    if name.endswith("-permuted"):
        reg, R = pixels_map(name[:-len("-permuted")])
        return permuted(reg, 5), R
    if name.startswith("noise"):
        w, h, k, conn = {"noise64x48": (64, 48, 4, 8), "noise96x80": (96, 80, 4, 4), "noise97x41": (97, 41, 3, 8),
                         "noise512x300": (512, 300, 16, 4)}[name]
        lab = (fx.xorshift(w * h, seed=fx.SEED + 1) % np.uint32(k)).astype(np.uint32).reshape(h, w)
        assert name == "noise512x300" or np.array_equal(lab, noise(w, h, k, seed=1))
        reg, _ = regions_model(lab, conn, frame(w, h))
        reg = reg.reshape(h, w)
    elif name.startswith("rows"):         # three rows (or as given) of a width around the wave
        w, h = {"rows1x7": (1, 7), "rows3x5": (3, 5), "rows63": (63, 3), "rows64": (64, 3), "rows65": (65, 3),
                "rows129": (129, 3)}[name]
        lab = (fx.xorshift(w * h, seed=fx.SEED + 9) % np.uint32(3)).astype(np.uint32).reshape(h, w)
        reg = regions_model(lab, 4, frame(w, h))[0].reshape(h, w)
    elif name == "stripes":               # not connected: id x % 3 in every row, T = 15 <= n
        reg = np.tile(np.arange(200, dtype=np.uint32) % 3, (5, 1))
        assert rows_total(reg) == 15
    elif name == "comb":                  # two combs whose teeth interlock: A B A B in every middle row
        ys, xs = np.mgrid[0:21, 0:150]
        reg = np.where((ys == 0) | ((xs % 2 == 0) & (ys < 20)), 0, 1).astype(np.uint32)
    elif name == "rings":                 # ring i leaves a row on the left and re-enters it on the right
        ys, xs = np.mgrid[0:30, 0:70]
        reg = np.minimum(np.minimum(xs, 69 - xs), np.minimum(ys, 29 - ys)).astype(np.uint32)
    elif name == "one":
        reg = np.zeros((5, 7), np.uint32)
    elif name == "each":                  # R = n
        reg = np.arange(64 * 48, dtype=np.uint32).reshape(48, 64)
    elif name == "line":                  # 2048 wide, 1 tall: one wave walks 32 chunks
        reg = (np.arange(2048, dtype=np.uint32) // 5).reshape(1, 2048)
    elif name == "column":                # 1 wide, 2048 tall: a wave per pixel
        reg = (np.arange(2048, dtype=np.uint32) // 7).reshape(2048, 1)
    elif name == "big":                   # a background of more than 131071 pixels and 300 islands of 3 x 3
        reg = np.zeros((300, 512), np.uint32)
        for i in range(300):
            x, y = 4 + 20 * (i % 25), 4 + 24 * (i // 25)
            reg[y:y + 3, x:x + 3] = 1 + i
        reg = relabel_by_first(reg)
        assert int((reg == 0).sum()) > 131071 and int(reg.max()) == 300
    else:
        raise KeyError(name)
    reg = np.ascontiguousarray(reg, np.uint32)
    reg.setflags(write=False)
    assert rows_total(reg) <= reg.size, name
    return reg, int(reg.max()) + 1


def relabel_by_first(reg):
    _, first, inv = np.unique(reg.reshape(-1), return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv].reshape(reg.shape).astype(np.uint32)


def with_gaps(reg, front, middle, end):
    """The same map with `front` unused ids before the first id, `middle`
    after every id below the median and `end` behind the last one."""
    R = int(reg.max()) + 1
    ids = np.arange(R, dtype=np.int64)
    new = front + ids + middle * np.minimum(ids, R // 2)
    return new.astype(np.uint32)[reg], int(new[-1]) + 1 + end


# ---------------------------------------------------------------------------
# Capture windows and window tags.
def islands(h, w, places):
    reg = np.zeros((h, w), np.uint32)
    for i, (x, y) in enumerate(places):
        reg[y:y + 3, x:x + 3] = 1 + i
    return reg


@functools.lru_cache(maxsize=None)
def wmap(name):
    """(region ids (H, W) uint32, R) of a named case; the names of pixels_map pass through."""
    if name == "diagonal":            # a one-pixel-wide line of id 1 on a background of id 0
        reg = np.eye(40, dtype=np.uint32)
    elif name == "islands":           # 3 x 3 islands in the four corners and the middle, and a pair whose
        reg = islands(48, 64, [(0, 0), (61, 0), (0, 45), (61, 45), (29, 21), (10, 30), (22, 30)])   # windows overlap
    elif name == "each16x12":         # one region per pixel
        reg = np.arange(16 * 12, dtype=np.uint32).reshape(12, 16)
    elif name == "refused":           # id 0 in the first and the last block, id 1 between: T' = 98 > P = 50
        reg = np.ones((200, 4), np.uint32)
        reg[0:4] = reg[196:200] = 0
    else:
        return pixels_map(name)
    reg = np.ascontiguousarray(reg, np.uint32)
    reg.setflags(write=False)
    return reg, int(reg.max()) + 1


def mask_of(kind, h, w):
    if kind is None:
        return None
    mask = np.zeros((h, w), np.uint8)
    if kind == "random":              # about 30 %
        mask = (fx.xorshift(h * w, seed=fx.SEED + 31) % np.uint32(10) < 3).astype(np.uint8).reshape(h, w)
        assert 0.25 < mask.mean() < 0.35
    elif kind == "block":             # one whole block: m(b) = 0
        mask[8:12, 20:24] = 1
    elif kind == "island-window":     # the whole window of the island at the top left corner of "islands"
        mask[0:12, 0:12] = 7
    else:
        raise KeyError(kind)
    mask.setflags(write=False)
    return mask


# every (map, d, e) the windows and tags tests run, for the CPU check that T' <= P
CASES = ([("rows65", 1, 0), ("comb", 1, 0), ("noise97x41", 4, 2), ("rows3x5", 4, 2), ("rows1x7", 4, 2),
          ("rows64", 4, 2), ("one", 4, 2), ("diagonal", 4, 1), ("diagonal", 4, 2), ("islands", 4, 2),
          ("each16x12", 4, 2), ("each16x12", 8, 3), ("each16x12", 2, 0), ("noise64x48", 4, 2), ("big", 4, 2),
          ("noise97x41-permuted", 4, 2)] +
         [(name, d, e) for name in ("noise96x80", "noise96x80-permuted") for d, e in ((2, 1), (4, 0), (4, 2), (8, 3))])


@functools.lru_cache(maxsize=None)
def tie_map(order):
    """4 rows x 12 columns, three 4 x 4 blocks with the ids `order`: at d = 4, e = 1 row 0 of [1, 0, 2]
    (and of [2, 0, 1]) holds all three ids with 16 pixels each."""
    reg = np.repeat(np.array(order, np.uint32), 4)[None, :].repeat(4, axis=0)
    reg = np.ascontiguousarray(reg)
    reg.setflags(write=False)
    return reg, 3


# The fake non-NULL pointers and the bad shapes of the capture-window argument checks; test_wtags_abi.py restates
# every shape in its own call's terms.
WINDOWS_FAKE = {name: 0x10000 * (i + 1) for i, name in enumerate(
    ["regions", "offsets", "coords", "index", "pixels", "colors", "mask", "area", "out", "cts", "k_outs"])}

WINDOWS_SHAPES = {
    "null_regions": dict(regions=None),
    "null_offsets": dict(offsets=None),
    "width_0": dict(width=0),
    "height_0": dict(height=0),
    "width_65536": dict(width=65536, height=1),
    "height_65536": dict(width=1, height=65536),
    "pixels_2^31": dict(width=65535, height=32769),      # 2^31 + 32767
    "pixels_65535x65535": dict(width=65535, height=65535),
    "nregions_0": dict(nregions=0),
    "nregions_2^31": dict(nregions=1 << 31),
    "nregions_max_u32": dict(nregions=0xFFFFFFFF),
    "block_0": dict(block=0),
    "block_9": dict(block=9),
    "block_max_u32": dict(block=0xFFFFFFFF),
    "expand_4": dict(expand=4),
    "expand_max_u32": dict(expand=0xFFFFFFFF),
    "regions_2mod4": dict(regions=WINDOWS_FAKE["regions"] + 2),
    "regions_odd": dict(regions=WINDOWS_FAKE["regions"] + 1),
    "offsets_2mod4": dict(offsets=WINDOWS_FAKE["offsets"] + 2),
    "area_2mod4": dict(area=WINDOWS_FAKE["area"] + 2),
    "coords_odd": dict(coords=WINDOWS_FAKE["coords"] + 1),
    "index_2mod4": dict(index=WINDOWS_FAKE["index"] + 2),
    "colors_2mod4": dict(colors=WINDOWS_FAKE["colors"] + 2),
    "pixels_2mod4": dict(pixels=WINDOWS_FAKE["pixels"] + 2),
}
