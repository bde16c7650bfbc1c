"""The skeletons of all regions of a region map (include/dq_hip.h, "region
skeleton") in numpy, written from the rules and using none of the code under
test: Guo-Hall two-subiteration thinning where a pixel's neighbour is on only if
it lies in the frame, has the pixel's own id and is still alive.
test_skeleton_model.py pins it to scalar loops over one region's padded mask at
a time and to hand-checked literals."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_ITERS = 65535
# n0 .. n7 as (dy, dx): NW, N, NE, E, SE, S, SW, W
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1))


def _shifted(padded, dy, dx):
    h, w = padded.shape[0] - 2, padded.shape[1] - 2
    return padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def _subiteration(alive, same, second):
    padded = np.pad(alive, 1)
    n = [_shifted(padded, dy, dx) & same[k] for k, (dy, dx) in enumerate(NEIGHBOURS)]
    i = lambda b: b.astype(np.int8)  # noqa: E731
    c = i(~n[1] & (n[2] | n[3])) + i(~n[3] & (n[4] | n[5])) + i(~n[5] & (n[6] | n[7])) + i(~n[7] & (n[0] | n[1]))
    n1 = i(n[0] | n[1]) + i(n[2] | n[3]) + i(n[4] | n[5]) + i(n[6] | n[7])
    n2 = i(n[1] | n[2]) + i(n[3] | n[4]) + i(n[5] | n[6]) + i(n[7] | n[0])
    m = np.minimum(n1, n2)
    side = (n[5] | n[6] | ~n[0]) & n[7] if second else (n[1] | n[2] | ~n[4]) & n[3]
    return alive & ~((c == 1) & ((m == 2) | (m == 3)) & ~side)


def region_skeleton(reg, nreg, max_iters=0):
    """skel, skeled, when, skel_area, thick, kept, iterations, converged of the map `reg` with R = nreg."""
    reg = np.asarray(reg)
    assert reg.ndim == 2 and 0 <= max_iters <= MAX_ITERS
    ids = reg.astype(np.int64)
    region = ids < nreg
    padded = np.pad(ids, 1, constant_values=-1)
    same = [region & (_shifted(padded, dy, dx) == ids) for dy, dx in NEIGHBOURS]
    alive = region.copy()
    when = np.zeros(reg.shape, np.uint16)
    iterations = converged = 0
    for it in range(1, (max_iters or MAX_ITERS) + 1):
        after = _subiteration(_subiteration(alive, same, False), same, True)
        gone = alive & ~after
        alive = after
        if not gone.any():
            converged = 1
            break
        when[gone] = it
        iterations = it
    skel_area = np.bincount(ids[alive], minlength=nreg)[:nreg].astype(np.uint32)
    thick = np.zeros(nreg, np.uint32)
    np.maximum.at(thick, ids[region], when[region])
    return {"skel": alive.astype(np.uint8), "skeled": np.where(alive, ids, NONE).astype(np.uint32), "when": when,
            "skel_area": skel_area, "thick": thick, "kept": int(alive.sum()), "iterations": iterations,
            "converged": converged}
