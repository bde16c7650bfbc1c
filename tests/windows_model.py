"""Host model of the capture windows of a region map (include/dq_hip.h,
"capture windows"), written from the definition alone and using none of the
code under test: per region a boolean grid of the blocks it has a pixel in,
`expand` shift-and-or dilations by the plus-shaped cross, then the blocks of
the window in raster order and in each block its pixels in raster order,
without the pixels outside the frame and the masked ones.  (The reference
application needs OpenCV, which is not available to the tests: the model is the
oracle, as in the adjacency, merge and pixel-list stages.)"""
import numpy as np


def dilate_cross(grid):
    """One dilation by the 3 x 3 cross; nothing comes in from outside the grid."""
    out = grid.copy()
    out[1:, :] |= grid[:-1, :]
    out[:-1, :] |= grid[1:, :]
    out[:, 1:] |= grid[:, :-1]
    out[:, :-1] |= grid[:, 1:]
    return out


def dilate_square(grid):
    """One dilation by the full 3 x 3 square (what the element is NOT)."""
    rows = grid.copy()
    rows[1:, :] |= grid[:-1, :]
    rows[:-1, :] |= grid[1:, :]
    out = rows.copy()
    out[:, 1:] |= rows[:, :-1]
    out[:, :-1] |= rows[:, 1:]
    return out


def own_blocks(reg2d, R, d):
    """Per id < R the (block row, block column) arrays of the blocks it has a pixel in."""
    h, w = reg2d.shape
    bw = -(-w // d)
    ys, xs = np.mgrid[0:h, 0:w]
    ids = reg2d.reshape(-1).astype(np.int64)
    blocks = ((ys // d) * bw + xs // d).reshape(-1)
    keep = ids < R
    pairs = np.unique(ids[keep] * (1 << 32) + blocks[keep])
    owner, block = pairs >> 32, pairs & 0xFFFFFFFF
    starts = np.searchsorted(owner, np.arange(R + 1))
    return [(block[starts[r]:starts[r + 1]] // bw, block[starts[r]:starts[r + 1]] % bw) for r in range(R)]


def window_grids(reg2d, R, d, e, area=None, min_area=0, dilate=dilate_cross, bbox=False):
    """Yields (r, j_lo, i_lo, boolean grid of window(r) from block (j_lo, i_lo)) for every region with a
    window.  bbox: the grid is cut to the own blocks' bounding box grown by e (all else is False anyway)."""
    h, w = reg2d.shape
    bh, bw = -(-h // d), -(-w // d)
    for r, (bj, bi) in enumerate(own_blocks(reg2d, R, d)):
        if len(bj) == 0 or (area is not None and area[r] <= min_area):
            continue
        j0, j1, i0, i1 = 0, bh, 0, bw
        if bbox:
            j0, j1 = max(int(bj.min()) - e, 0), min(int(bj.max()) + e + 1, bh)
            i0, i1 = max(int(bi.min()) - e, 0), min(int(bi.max()) + e + 1, bw)
        grid = np.zeros((j1 - j0, i1 - i0), bool)
        grid[bj - j0, bi - i0] = True
        for _ in range(e):
            grid = dilate(grid)
        yield r, j0, i0, grid


def block_pixels(h, w, d, mask=None):
    """Per block (raster order of blocks) its surviving pixel indexes in raster order."""
    bh, bw = -(-h // d), -(-w // d)
    alive = np.ones(h * w, bool) if mask is None else np.asarray(mask).reshape(-1) == 0
    out = []
    for j in range(bh):
        for i in range(bw):
            ys, xs = np.mgrid[j * d:min(j * d + d, h), i * d:min(i * d + d, w)]
            p = (ys * w + xs).reshape(-1)
            out.append(p[alive[p]])
    return out


def windows_model(reg2d, R, pixels, d, e, mask=None, area=None, min_area=0, lists=True, bbox=False):
    """The outputs of the definition, and P and T' of the refusal rule."""
    reg2d = np.asarray(reg2d)
    h, w = reg2d.shape
    bw = -(-w // d)
    per_block = block_pixels(h, w, d, mask)
    m = np.array([len(p) for p in per_block], np.int64)
    lengths, chunks, P, T = np.zeros(R, np.int64), [], 0, 0
    for r, j0, i0, grid in window_grids(reg2d, R, d, e, area, min_area, bbox=bbox):
        js, is_ = np.nonzero(grid)                       # (raster order of blocks)
        blocks = (js + j0) * bw + is_ + i0
        P += len(blocks)
        T += int(js.max() - js.min() + 1)
        lengths[r] = m[blocks].sum()
        if lists:
            chunks.extend(per_block[b] for b in blocks)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    assert offsets[-1] <= (1 << 32) - 1
    out = {"offsets": offsets.astype(np.uint32), "P": P, "T": T}
    if lists:
        order = np.concatenate(chunks).astype(np.int64) if chunks else np.zeros(0, np.int64)
        out.update(index=order.astype(np.uint32), coords=((order % w) | (order // w) << 16).astype(np.uint32),
                   colors=np.asarray(pixels, np.uint32).reshape(-1)[order])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
