"""Host model of the pixel lists of a region map (include/dq_hip.h, "pixel
lists"), written against the definition and using none of the code under test:
a stable argsort of the ids, bincount and cumsum for the offsets, the lists by
fancy indexing.  rows_total is T of the refusal rule."""
import numpy as np


def lists_model(reg2d, R, pixels):
    reg2d = np.asarray(reg2d)
    h, w = reg2d.shape
    regions = reg2d.reshape(-1).astype(np.int64)
    order = np.argsort(regions, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(regions, minlength=R))])
    out = {"offsets": offsets.astype(np.uint32), "index": order.astype(np.uint32),
           "coords": ((order % w) | (order // w) << 16).astype(np.uint32),
           "colors": np.asarray(pixels, np.uint32).reshape(-1)[order]}
    for v in out.values():
        v.setflags(write=False)
    return out


def rows_total(reg2d):
    """T of the definition: over the ids present, last row - first row + 1."""
    reg2d = np.asarray(reg2d)
    ys = np.repeat(np.arange(reg2d.shape[0]), reg2d.shape[1])
    ids = reg2d.reshape(-1).astype(np.int64)
    lo, hi = np.full(ids.max() + 1, 1 << 40), np.full(ids.max() + 1, -1)
    np.minimum.at(lo, ids, ys)
    np.maximum.at(hi, ids, ys)
    return int((hi - lo + 1)[hi >= 0].sum())
