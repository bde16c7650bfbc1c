"""Host models of the containment tree (include/dq_hip.h, "containment tree"),
checkers only.

model(regions2d, area, edges, nregions)  the definition, in numpy and plain
    loops: roots, breadth-first depth, parent by (area, lowest id), size order,
    children rows, subtree / enclosed, the post-order.
reference_tree(...)  a sequential restatement of the reference's rule
    (recurseSuperpixelContainment): depth-first, a visited region claims every
    neighbour nobody has claimed, later siblings are blocked while the walk is
    below an earlier one, siblings are taken in size order.  It is well defined
    only on NESTED maps; there its parents and roots equal the model's.
Plus the map builders the tests share and a host edge list of a map.
"""
import numpy as np

NONE = 0xFFFFFFFF
# the tree's output arrays, in the order of the C entry point's pointers
ARRAYS = ("depth", "parent", "roots", "child_offsets", "children", "subtree", "enclosed", "order", "pos")


def edges_of(regions2d, connectivity=4):
    """The sorted distinct (a < b) id pairs of touching pixels."""
    r = np.asarray(regions2d).astype(np.int64)
    pairs = [(r[:, :-1], r[:, 1:]), (r[:-1, :], r[1:, :])]
    if connectivity == 8:
        pairs += [(r[:-1, :-1], r[1:, 1:]), (r[:-1, 1:], r[1:, :-1])]
    out = set()
    for a, b in pairs:
        a, b = a.reshape(-1), b.reshape(-1)
        m = a != b
        lo, hi = np.minimum(a[m], b[m]), np.maximum(a[m], b[m])
        out.update(zip(lo.tolist(), hi.tolist()))
    return np.array(sorted(out), np.uint32).reshape(-1, 2)


def areas_of(regions2d, nregions):
    return np.bincount(np.asarray(regions2d).reshape(-1), minlength=nregions).astype(np.uint32)


def size_order(area):
    """Ids by area decreasing, ties by id increasing; and the rank of every id."""
    area = np.asarray(area, np.uint32)
    order = np.lexsort((np.arange(area.size), -area.astype(np.int64))).astype(np.uint32)
    rank = np.empty(area.size, np.uint32)
    rank[order] = np.arange(area.size, dtype=np.uint32)
    return order, rank


def _neighbours(edges, R):
    nb = [set() for _ in range(R)]
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2):
        if a != b and a < R and b < R:
            nb[a].add(int(b))
            nb[b].add(int(a))
    return nb


def border_ids(regions2d, R):
    r = np.asarray(regions2d)
    ids = np.concatenate([r[0, :], r[-1, :], r[:, 0], r[:, -1]])
    return sorted(set(int(i) for i in ids if i < R))


def model(regions2d, area, edges, nregions):
    R = int(nregions)
    area = np.asarray(area, np.uint32)
    nb = _neighbours(edges, R)
    depth = np.full(R, NONE, np.uint32)
    front = border_ids(regions2d, R)
    depth[front] = 0
    level = 0
    while front:
        level += 1
        nxt = sorted({q for r in front for q in nb[r] if depth[q] == NONE})
        depth[nxt] = level
        front = nxt
    levels = level
    parent = np.full(R, NONE, np.uint32)
    for r in range(R):
        if depth[r] != NONE and depth[r] > 0:
            cand = [q for q in nb[r] if depth[q] == depth[r] - 1]
            parent[r] = min(cand, key=lambda q: (-int(area[q]), q))
    order_by_size, rank = size_order(area)
    reached_ids = [int(r) for r in order_by_size if depth[r] != NONE]
    roots = [r for r in reached_ids if depth[r] == 0]
    rows = [[] for _ in range(R)]
    for r in reached_ids:
        if depth[r] > 0:
            rows[int(parent[r])].append(r)
    child_offsets = np.zeros(R + 1, np.uint32)
    child_offsets[1:] = np.cumsum([len(x) for x in rows])
    children = np.array([c for x in rows for c in x], np.uint32)
    subtree = np.zeros(R, np.uint32)
    enclosed = np.zeros(R, np.uint64)
    for r in sorted(reached_ids, key=lambda r: -int(depth[r])):   # deepest first
        subtree[r] += 1
        enclosed[r] += np.uint64(area[r])
        if depth[r] > 0:
            subtree[parent[r]] += subtree[r]
            enclosed[parent[r]] += enclosed[r]
    order = []
    stack = [(r, False) for r in reversed(roots)]   # (an explicit stack: chains are deep)
    while stack:
        r, done = stack.pop()
        if done:
            order.append(r)
            continue
        stack.append((r, True))
        stack.extend((c, False) for c in reversed(rows[r]))
    order = np.array(order, np.uint32)
    pos = np.full(R, NONE, np.uint32)
    pos[order] = np.arange(order.size, dtype=np.uint32)
    return dict(depth=depth, parent=parent, roots=np.array(roots, np.uint32), child_offsets=child_offsets,
                children=children, subtree=subtree, enclosed=enclosed, order=order, pos=pos, rank=rank,
                nroots=len(roots), levels=levels, reached=len(reached_ids))


def reference_tree(regions2d, area, edges, nregions):
    """(parent, roots): the reference's depth-first claim, siblings in size order."""
    R = int(nregions)
    nb = _neighbours(edges, R)
    _, rank = size_order(area)
    roots = sorted(border_ids(regions2d, R), key=lambda r: rank[r])
    parent = np.full(R, NONE, np.uint32)
    claimed = np.zeros(R, bool)
    claimed[roots] = True
    stack = list(reversed(roots))
    while stack:
        r = stack.pop()
        mine = sorted((q for q in nb[r] if not claimed[q]), key=lambda q: rank[q])
        for q in mine:   # all claimed before the walk goes below the first of them
            claimed[q] = True
            parent[q] = r
        stack.extend(reversed(mine))
    return parent, np.array(roots, np.uint32)


def is_nested(regions2d, area, edges, nregions):
    m = model(regions2d, area, edges, nregions)
    nb = _neighbours(edges, int(nregions))
    for r in range(int(nregions)):
        d = m["depth"][r]
        if d == NONE or d == 0:
            continue
        if sum(1 for q in nb[r] if m["depth"][q] < d) != 1:
            return False
        if any(m["depth"][q] == d and m["parent"][q] != m["parent"][r] for q in nb[r]):
            return False
    return True


# ---- maps --------------------------------------------------------------------
XCTEST_MAPS = {   # Test/ContainmentTest.mm, ids = tag - 1
    "1x1": np.array([[0]], np.uint32),
    "2x2_rows": np.array([[0, 0], [1, 1]], np.uint32),
    "2x2_corner": np.array([[0, 1], [1, 1]], np.uint32),
    "4x4_bars": np.array([[0, 0, 0, 0], [0, 1, 2, 0], [0, 1, 2, 0], [0, 0, 0, 0]], np.uint32),
}


def rings(side):
    """Concentric one-pixel square rings: ring k has id k, a chain of depth (side + 1) // 2."""
    y, x = np.mgrid[0:side, 0:side]
    return np.minimum(np.minimum(x, y), np.minimum(side - 1 - x, side - 1 - y)).astype(np.uint32)


def islands(side, two_pixel_every=0):
    """A background (id 0) with one-pixel islands on the odd stride-2 grid points,
    numbered in raster order.  With two_pixel_every = k, every k-th grid point
    in a column x = 1 mod 4 grows one pixel to the right and the grid point after
    it stays empty: islands of one and two pixels that do not touch."""
    ys, xs = np.mgrid[1:side - 1:2, 1:side - 1:2]
    land = np.zeros((side, side), bool)
    land[ys, xs] = True
    if two_pixel_every:
        k = np.arange(ys.size).reshape(ys.shape)
        pick = (k % two_pixel_every == 0) & (xs % 4 == 1) & (xs + 2 < side - 1)
        land[ys[pick], xs[pick] + 1] = True
        land[ys[pick], xs[pick] + 2] = False
    first = land.copy()
    first[:, 1:] &= ~land[:, :-1]          # the left pixel of every island
    ids = np.cumsum(first.reshape(-1)).reshape(land.shape).astype(np.uint32)   # raster order, from 1
    reg = np.where(land, ids, 0).astype(np.uint32)
    return reg


def islands_in_islands():
    """Two roots (left and right half), each with 5 x 5 islands that hold a 3 x 3 and that a 1 x 1."""
    reg = np.zeros((16, 32), np.uint32)
    reg[:, 16:] = 1
    nxt = 2
    for (y, x) in ((2, 2), (9, 8), (3, 20), (9, 25)):
        reg[y:y + 5, x:x + 5] = nxt
        reg[y + 1:y + 4, x + 1:x + 4] = nxt + 1
        reg[y + 2, x + 2] = nxt + 2
        nxt += 3
    return reg


def noise(side):
    """Every pixel its own region, ids in raster order."""
    return np.arange(side * side, dtype=np.uint32).reshape(side, side)


NOT_NESTED = np.array([   # 4 touches 2 (one level up) and 3 (its own level, inside 1): the reference's walk is
    [0, 0, 0, 0, 0, 0, 0],   # below the larger 1 first and 3 claims 4; breadth-first, 4 belongs to 2
    [0, 1, 1, 1, 2, 2, 0],
    [0, 1, 1, 3, 4, 2, 0],
    [0, 1, 1, 1, 2, 2, 0],
    [0, 0, 0, 0, 0, 0, 0]], np.uint32)
