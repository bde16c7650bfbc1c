"""A numpy model of the "region distance" block of include/dq_hip.h, written from
the definition and using none of the library's code.

    brute_distance     rule 1 by the definition, O(n^2): tiny maps only
    scan_distance      rule 1 as eight prefix scans (heads and tails along lines)
    scipy_distance     rule 1 per region with scipy's taxicab chamfer transform
    scale_byte, radius_of, thresh_of       rule 3
    region_values      rules 1-5: dist, dmax, bbox, thresh, count, centre
    region_cores       rule 6: core, cored, core_area, kept
"""
import math

import numpy as np

NONE = 0xFFFFFFFF


def brute_distance(reg, nreg):
    reg = np.asarray(reg)
    h, w = reg.shape
    ys, xs = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w), np.uint16)
    for y in range(h):
        for x in range(w):
            r = reg[y, x]
            if r >= nreg:
                continue
            best = min(x + 1, w - x, y + 1, h - y)   # the positions just outside the frame
            other = reg != r
            if other.any():
                best = min(best, int((np.abs(ys - y) + np.abs(xs - x))[other].min()))
            out[y, x] = best
    return out


def _line_gap(reg, axis):
    """Per pixel: min(i - lastHead + 1, firstTail - i + 1) along `axis`, and the two terms."""
    reg = np.moveaxis(np.asarray(reg), axis, 0)
    n = reg.shape[0]
    idx = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * (reg.ndim - 1))
    change = np.ones(reg.shape, bool)
    change[1:] = reg[1:] != reg[:-1]
    head = np.maximum.accumulate(np.where(change, idx, -1), axis=0)
    change = np.ones(reg.shape, bool)
    change[:-1] = reg[:-1] != reg[1:]
    tail = np.minimum.accumulate(np.where(change, idx, 1 << 40)[::-1], axis=0)[::-1]
    a, b = idx - head + 1, tail - idx + 1
    return np.moveaxis(a, 0, axis), np.moveaxis(b, 0, axis)


def scan_distance(reg, nreg):
    reg = np.asarray(reg)
    h, w = reg.shape
    up, down = _line_gap(reg, 0)
    g = np.minimum(up, down)
    left, right = _line_gap(reg, 1)
    x = np.arange(w, dtype=np.int64)[None, :]
    fwd = x + np.minimum.accumulate(g - x, axis=1)
    bwd = -x + np.minimum.accumulate((g + x)[:, ::-1], axis=1)[:, ::-1]
    d = np.minimum(np.minimum(left, right), np.minimum(fwd, bwd))
    d[reg >= nreg] = 0
    return d.astype(np.uint16)


def scipy_distance(reg, nreg):
    """Per region the taxicab transform of its zero-padded mask (needs scipy)."""
    from scipy.ndimage import distance_transform_cdt
    reg = np.asarray(reg)
    out = np.zeros(reg.shape, np.uint16)
    for r in np.unique(reg):
        if r >= nreg:
            continue
        mask = np.pad(reg == r, 1)
        d = distance_transform_cdt(mask, metric="taxicab")[1:-1, 1:-1]
        out[reg == r] = d[reg == r]
    return out


def c_round(x):
    return math.floor(x + 0.5)   # C round() of a non-negative value


def radius_of(bw, bh):
    return math.isqrt(((bw + 2) ** 2 + (bh + 2) ** 2) >> 2) + 1


def radius_reference(bw, bh):
    """The reference's int(round(hypot((bw+2)/2, (bh+2)/2) + 0.5) + 0.01) over the padded mask."""
    return int(c_round(math.hypot((bw + 2) * 0.5, (bh + 2) * 0.5) + 0.5) + 0.01)


def scale_byte(d, radius):
    if d == 1:
        return 1
    return max(1, int(math.sqrt(float(d)) / float(radius) * 255 + 0.5) & 0xFF)


def thresh_of(dmax, bw, bh, rule):
    if rule == 0 or dmax <= 1:
        return dmax
    radius = radius_of(bw, bh)
    target = scale_byte(dmax, radius)
    lo, hi = 1, dmax
    while lo < hi:
        mid = (lo + hi) // 2
        if scale_byte(mid, radius) >= target:
            hi = mid
        else:
            lo = mid + 1
    return lo


def thresh_by_walk(dmax, bw, bh):
    radius = radius_of(bw, bh)
    return next(d for d in range(1, dmax + 1) if scale_byte(d, radius) == scale_byte(dmax, radius))


def region_values(reg, nreg, rule=0, dist=None):
    reg = np.asarray(reg).astype(np.int64)
    h, w = reg.shape
    d = scan_distance(reg, nreg).astype(np.int64) if dist is None else np.asarray(dist).astype(np.int64)
    ys, xs = np.mgrid[0:h, 0:w]
    on = reg < nreg
    ids, dd, yy, xx = reg[on], d[on], ys[on], xs[on]
    dmax = np.zeros(nreg, np.int64)
    np.maximum.at(dmax, ids, dd)
    big = NONE
    bbox = np.tile(np.array([big, big, 0, 0], np.int64), (nreg, 1))
    np.minimum.at(bbox[:, 0], ids, xx)
    np.minimum.at(bbox[:, 1], ids, yy)
    np.maximum.at(bbox[:, 2], ids, xx)
    np.maximum.at(bbox[:, 3], ids, yy)
    thresh = np.zeros(nreg, np.int64)
    for r in np.flatnonzero(dmax):
        thresh[r] = thresh_of(int(dmax[r]), int(bbox[r, 2] - bbox[r, 0] + 1), int(bbox[r, 3] - bbox[r, 1] + 1), rule)
    in_s = dd >= thresh[ids]
    ids, yy, xx = ids[in_s], yy[in_s], xx[in_s]   # (raster order)
    count = np.bincount(ids, minlength=nreg)
    order = np.argsort(ids, kind="stable")
    ids, yy, xx = ids[order], yy[order], xx[order]
    start = np.concatenate(([0], np.cumsum(count)))
    centre = np.full(nreg, NONE, np.int64)
    for r in np.flatnonzero(count):
        sy, sx = yy[start[r]:start[r + 1]], xx[start[r]:start[r + 1]]
        if count[r] <= 2:
            row = sy.max()
            cx, cy = int(sx[sy == row].min()), int(row)
        else:
            cx, cy = int(sx.sum()) // int(count[r]), int(sy.sum()) // int(count[r])
            if not ((sx == cx) & (sy == cy)).any():
                k = int(np.argmin((sx - cx) ** 2 + (sy - cy) ** 2))   # (the first of the lowest: raster order)
                cx, cy = int(sx[k]), int(sy[k])
        centre[r] = cx | cy << 16
    return dict(dist=d.astype(np.uint16), dmax=dmax.astype(np.uint32), bbox=bbox.astype(np.uint32),
                thresh=thresh.astype(np.uint32), count=count.astype(np.uint32), centre=centre.astype(np.uint32))


def region_cores(reg, nreg, centre, connectivity=8):
    reg = np.asarray(reg)
    h, w = reg.shape
    core = np.zeros((h, w), np.uint8)
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)]
    if connectivity == 8:
        steps += [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    for r in range(nreg):
        if centre[r] == NONE:
            continue
        x, y = int(centre[r]) & 0xFFFF, int(centre[r]) >> 16
        assert reg[y, x] == r
        core[y, x] = 1
        stack = [(y, x)]
        while stack:
            y, x = stack.pop()
            for dy, dx in steps:
                v, u = y + dy, x + dx
                if 0 <= v < h and 0 <= u < w and not core[v, u] and reg[v, u] == r:
                    core[v, u] = 1
                    stack.append((v, u))
    cored = np.where(core == 1, reg, NONE).astype(np.uint32)
    area = np.bincount(reg[core == 1].astype(np.int64), minlength=nreg).astype(np.uint32)
    return dict(core=core, cored=cored, core_area=area, kept=int(core.sum()))
