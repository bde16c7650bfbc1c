"""Host models of the region adjacency graph of a region map (include/dq_hip.h,
"region adjacency graph"), written against the definition and using none of
the code under test.

adjacency_model: per direction the pairs (p, q) with different ids, all
contacts sorted by (p, q), np.unique over the keys (a << 32 | b), edges ordered
by the index of their first contact, step by np.add.at, degree by np.bincount.
For regions = arange(w * h) it gives E = 2wh - w - h (4-connectivity) and
4wh - 3w - 3h + 2 (8) with every border 1.

edges_model is the short form the merge suite feeds its model with: np.unique
over the neighbour pairs with different ids, sorted."""
import numpy as np

from regions_model import _neighbour_pairs


def adjacency_model(reg2d, connectivity, pixels=None, num_regions=None):
    """dict(E, edges, border, contact[, step][, degree]) of a 2-D id map."""
    reg2d = np.asarray(reg2d)
    h, w = reg2d.shape
    r = reg2d.reshape(-1).astype(np.uint64)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    pairs = [(idx[:, :-1], idx[:, 1:])]                         # right
    if connectivity == 8:
        pairs.append((idx[:-1, 1:], idx[1:, :-1]))              # down-left
    else:
        assert connectivity == 4
    pairs.append((idx[:-1, :], idx[1:, :]))                     # down
    if connectivity == 8:
        pairs.append((idx[:-1, :-1], idx[1:, 1:]))              # down-right
    p = np.concatenate([a.reshape(-1) for a, _ in pairs])
    q = np.concatenate([b.reshape(-1) for _, b in pairs])
    assert (p < q).all()
    keep = r[p] != r[q]
    p, q = p[keep], q[keep]
    order = np.lexsort((q, p))
    p, q = p[order], q[order]
    a, b = np.minimum(r[p], r[q]), np.maximum(r[p], r[q])
    key = (a << np.uint64(32)) | b
    uniq, first, inverse, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), np.int64)
    rank[by_first] = np.arange(len(uniq))
    uniq, first, counts = uniq[by_first], first[by_first], counts[by_first]
    out = {"E": len(uniq),
           "edges": np.stack([uniq >> np.uint64(32), uniq & np.uint64(0xFFFFFFFF)], axis=1).astype(np.uint32),
           "border": counts.astype(np.uint32),
           "contact": np.stack([p[first], q[first]], axis=1).astype(np.uint32)}
    if pixels is not None:
        px = np.asarray(pixels, np.uint32).reshape(-1)
        d = np.zeros(len(p), np.uint64)
        for shift in (16, 8, 0):
            cp, cq = ((px[p] >> shift) & 0xFF).astype(np.int64), ((px[q] >> shift) & 0xFF).astype(np.int64)
            d += np.abs(cp - cq).astype(np.uint64)
        step = np.zeros(len(uniq), np.uint64)
        np.add.at(step, rank[inverse.reshape(-1)], d)
        out["step"] = step
    if num_regions is not None:
        out["degree"] = np.bincount(out["edges"].reshape(-1).astype(np.int64), minlength=num_regions).astype(np.uint32)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def edges_model(reg, w, h, connectivity):
    """The (E, 2) pairs a < b of ids that touch, sorted."""
    reg = np.asarray(reg).astype(np.int64)
    p, q = _neighbour_pairs(w, h, connectivity)
    a, b = np.minimum(reg[p], reg[q]), np.maximum(reg[p], reg[q])
    keep = a != b
    return np.unique(np.stack([a[keep], b[keep]], axis=1), axis=0).astype(np.uint32).reshape(-1, 2)
