"""Host model of merging regions over their adjacency graph (include/dq_hip.h,
"region merge"), written against the definition and using none of the code
under test.

The merge goes round by round: 8.8 fixed-point means by integer division, keys
(d << 32 | other) reduced by np.minimum.at, the link rule, roots by pointer
jumping, stats folded by np.add.at / np.minimum.at / np.maximum.at, final ids
by the rank of the roots' first pixels.  Its inputs come from regions_model
(regions_model.py) and edges_model (adjacency_model.py).
test_merge_model.py pins its R' and rounds on the 64 x 48 noise map to the
figures it gave when the definition was fixed, so a weakened model cannot pass.

With a distance limit the rounds are not bounded by 32 (a component may get
its first offer only after a neighbour's mean has moved)."""
import numpy as np

NONE = 0xFFFFFFFF              # max_dist: no limit
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def merge_model(reg, area, first, sums, bbox, edges, min_area, max_dist=NONE, max_rounds=0):
    """dict(R, rounds, regions, remap, area, first, sums, bbox) by the definition."""
    reg = np.asarray(reg).astype(np.int64)
    R = len(area)
    area = np.asarray(area).astype(np.int64).copy()
    first = np.asarray(first).astype(np.int64).copy()
    sums = np.asarray(sums).astype(np.int64).copy()
    bbox = np.asarray(bbox).astype(np.int64).copy()
    ea = np.asarray(edges).reshape(-1, 2)[:, 0].astype(np.int64)
    eb = np.asarray(edges).reshape(-1, 2)[:, 1].astype(np.int64)
    comp = np.arange(R, dtype=np.int64)
    ids = np.arange(R, dtype=np.int64)
    live = np.ones(R, bool)
    rounds = 0
    while not (max_rounds and rounds >= max_rounds):
        restless = live & (area < min_area)                                   # 1
        mean = (256 * sums) // np.maximum(area, 1)[:, None]                   # 2
        A, B = comp[ea], comp[eb]
        d = np.abs(mean[A] - mean[B]).sum(axis=1)                             # 3
        ok = (A != B) & (d <= max_dist)                                       # 4
        A, B, d = A[ok], B[ok], d[ok].astype(np.uint64)
        best = np.full(R, NO_KEY, np.uint64)
        for X, Y in ((A, B), (B, A)):
            offered = restless[X]
            np.minimum.at(best, X[offered], (d[offered] << np.uint64(32)) | Y[offered].astype(np.uint64))
        has = best != NO_KEY                                                   # 5
        target = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
        target[~has] = ids[~has]
        stays = has & has[target] & (target[target] == ids) & (ids < target)
        links = has & ~stays
        if not links.any():                                                    # 6
            break
        parent = np.where(links, target, ids)                                  # 7
        root, jumps = parent, 0
        while not np.array_equal(root[root], root):
            root, jumps = root[root], jumps + 1
            assert jumps <= 32, "a cycle in parent"
        moved = np.nonzero(live & (root != ids))[0]
        np.add.at(area, root[moved], area[moved])
        np.add.at(sums, root[moved], sums[moved])
        np.minimum.at(first, root[moved], first[moved])
        np.minimum.at(bbox[:, 0], root[moved], bbox[moved, 0])
        np.minimum.at(bbox[:, 1], root[moved], bbox[moved, 1])
        np.maximum.at(bbox[:, 2], root[moved], bbox[moved, 2])
        np.maximum.at(bbox[:, 3], root[moved], bbox[moved, 3])
        live[moved] = False
        comp = root[comp]
        rounds += 1
    roots = np.nonzero(live)[0]
    assert np.array_equal(np.unique(comp), roots)
    order = roots[np.argsort(first[roots], kind="stable")]
    newid = np.full(R, -1, np.int64)
    newid[order] = np.arange(len(order))
    remap = newid[comp]
    out = {"R": len(order), "rounds": rounds, "regions": remap[reg].astype(np.uint32), "remap": remap.astype(np.uint32),
           "area": area[order].astype(np.uint32), "first": first[order].astype(np.uint32),
           "sums": sums[order].astype(np.uint64), "bbox": bbox[order].astype(np.uint32)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
