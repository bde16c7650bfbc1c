"""Host models of the connected regions of a label map (include/dq_hip.h,
"connected regions"), written against the definition and using none of the
code under test.

flood_fill_regions is the plain raster-order flood fill (numpy + a Python
stack, 4- and 8-connectivity): regions are numbered in the order the raster
scan meets their first pixel, which is the definition.  It also computes area,
bounding box, first pixel, label and colour sums.

regions_model is the second, independent statement the merge, pixel-list and
window suites build their maps with: union-find over equal-label neighbours,
numbered by first pixel; stats_model folds area, first, bbox and sums of a flat
id map by np.bincount / np.minimum.at / np.maximum.at / np.add.at."""
import numpy as np


def flood_fill_regions(lab2d, connectivity, pixels=None):
    """(regions2d uint32, stats) of a 2-D integer map by raster-order flood fill."""
    lab2d = np.asarray(lab2d)
    h, w = lab2d.shape
    n = h * w
    lab = lab2d.reshape(-1).tolist()
    reg = [-1] * n
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    else:
        assert connectivity == 4
    count = 0
    for s in range(n):
        if reg[s] >= 0:
            continue
        rid, L = count, lab[s]
        count += 1
        reg[s] = rid
        stack = [s]
        while stack:
            i = stack.pop()
            y, x = divmod(i, w)
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w:
                    j = yy * w + xx
                    if reg[j] < 0 and lab[j] == L:
                        reg[j] = rid
                        stack.append(j)
    reg = np.array(reg, np.int64)
    ys, xs = np.divmod(np.arange(n, dtype=np.int64), w)
    first = np.full(count, n, np.int64)
    np.minimum.at(first, reg, np.arange(n, dtype=np.int64))
    bbox = np.zeros((count, 4), np.int64)
    bbox[:, 0], bbox[:, 1] = w, h
    np.minimum.at(bbox[:, 0], reg, xs)
    np.minimum.at(bbox[:, 1], reg, ys)
    np.maximum.at(bbox[:, 2], reg, xs)
    np.maximum.at(bbox[:, 3], reg, ys)
    stats = {"area": np.bincount(reg, minlength=count).astype(np.uint32),
             "bbox": bbox.astype(np.uint32),
             "first": first.astype(np.uint32),
             "label": lab2d.reshape(-1)[first].astype(np.uint32)}
    if pixels is not None:
        px = np.asarray(pixels, np.uint32).reshape(-1)
        sums = np.zeros((count, 3), np.uint64)
        for c, shift in enumerate((16, 8, 0)):
            np.add.at(sums[:, c], reg, ((px >> shift) & 0xFF).astype(np.uint64))
        stats["sums"] = sums
    assert (np.diff(stats["first"].astype(np.int64)) > 0).all()   # numbered in raster order of the first pixel
    return reg.astype(np.uint32).reshape(h, w), stats


def _neighbour_pairs(w, h, connectivity):
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    pairs = [(idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])]
    if connectivity == 8:
        pairs += [(idx[:-1, 1:], idx[1:, :-1]), (idx[:-1, :-1], idx[1:, 1:])]
    else:
        assert connectivity == 4
    return (np.concatenate([a.reshape(-1) for a, _ in pairs]), np.concatenate([b.reshape(-1) for _, b in pairs]))


def regions_model(lab2d, connectivity, pixels):
    """(flat region ids numbered by first pixel, stats) of a 2-D label map."""
    lab2d = np.asarray(lab2d)
    h, w = lab2d.shape
    n = h * w
    lab = lab2d.reshape(-1)
    p, q = _neighbour_pairs(w, h, connectivity)
    same = lab[p] == lab[q]
    up = list(range(n))

    def find(i):
        while up[i] != i:
            up[i] = up[up[i]]
            i = up[i]
        return i
    for a, b in zip(p[same].tolist(), q[same].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            up[max(ra, rb)] = min(ra, rb)      # the root is the lowest pixel: the region's first
    root = np.array([find(i) for i in range(n)], np.int64)
    firsts, reg = np.unique(root, return_inverse=True)
    return reg.reshape(-1).astype(np.uint32), stats_model(reg.reshape(-1), w, pixels, firsts)


def stats_model(reg, w, pixels, firsts=None):
    """area, first, bbox, sums of a flat id map whose ids are 0 .. R-1."""
    reg = np.asarray(reg).astype(np.int64)
    n, R = len(reg), int(reg.max()) + 1
    ys, xs = np.divmod(np.arange(n, dtype=np.int64), w)
    first = np.full(R, n, np.int64)
    np.minimum.at(first, reg, np.arange(n, dtype=np.int64))
    assert firsts is None or np.array_equal(first, firsts)
    bbox = np.zeros((R, 4), np.int64)
    bbox[:, 0], bbox[:, 1] = w, n
    np.minimum.at(bbox[:, 0], reg, xs)
    np.minimum.at(bbox[:, 1], reg, ys)
    np.maximum.at(bbox[:, 2], reg, xs)
    np.maximum.at(bbox[:, 3], reg, ys)
    px = np.asarray(pixels, np.uint32).reshape(-1)
    sums = np.zeros((R, 3), np.uint64)
    for c, shift in enumerate((16, 8, 0)):
        np.add.at(sums[:, c], reg, ((px >> shift) & 0xFF).astype(np.uint64))
    return {"area": np.bincount(reg, minlength=R).astype(np.uint32), "first": first.astype(np.uint32),
            "bbox": bbox.astype(np.uint32), "sums": sums}
