"""The model of the region-contour stage (include/dq_hip.h, "region contours"):
rules 1-6 written out with numpy for what is per pixel and a scalar loop for the
trace, using none of the code under test.  test_contour_model.py pins it to an
independent scalar statement of OpenCV's loop on one region's zero-padded mask
at a time and to hand-checked literals."""
import numpy as np

NO_CODE = 8
# rule 1, y down: E, NE, N, NW, W, SW, S, SE
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)
START_ORDER = (0, 7, 6, 5)   # rule 2: E, SE, S, SW


def neighbour_bits(reg, nreg):
    """(H, W) uint8: bit d is set iff the neighbour in direction d lies in the frame and has the
    pixel's own id, and that id is a region's (< nreg)."""
    reg = np.asarray(reg).astype(np.int64)
    h, w = reg.shape
    pad = np.full((h + 2, w + 2), -1, np.int64)
    pad[1:-1, 1:-1] = np.where(reg < nreg, reg, -1)
    own = pad[1:-1, 1:-1]
    bits = np.zeros((h, w), np.uint8)
    for d in range(8):
        there = pad[1 + DY[d]:1 + DY[d] + h, 1 + DX[d]:1 + DX[d] + w]
        bits |= (((there == own) & (own >= 0)).astype(np.uint8) << d).astype(np.uint8)
    return bits


def _next_on_table():
    """NEXT[m][d]: the first of d + 1, d + 2, .. (mod 8) whose bit is set in m (rule 3); -1 for m == 0."""
    table = []
    for m in range(256):
        row = []
        for d in range(8):
            s = -1
            for k in range(1, 9):
                if m >> ((d + k) & 7) & 1:
                    s = (d + k) & 7
                    break
            row.append(s)
        table.append(row)
    return table


NEXT = _next_on_table()


def trace(bits, w, p0):
    """Rules 2-4 from the flat index p0 over the flat list `bits`: (flat indexes, codes) as followed."""
    m = bits[p0]
    if m == 0:
        return [p0], [NO_CODE]
    d0 = next(d for d in START_ORDER if m >> d & 1)
    off = [DY[d] * w + DX[d] for d in range(8)]
    pts, codes = [], []
    p, d = p0, d0
    while True:
        s = NEXT[bits[p]][d]
        pts.append(p)
        codes.append(s)
        p, d = p + off[s], (s + 4) & 7
        if p == p0 and d == d0:
            return pts, codes


def region_contours(reg, nreg, orientation=0):
    """The dictionary of outputs the entry gives: "offsets" (R + 1,), "len" (R,), "points" (M,)
    uint32, "codes" (M,) uint8, "visits" (H, W) uint8, and the int "total"."""
    reg = np.ascontiguousarray(reg, np.uint32)
    h, w = reg.shape
    flat = reg.reshape(-1)
    bits = neighbour_bits(reg, nreg).reshape(-1).tolist()
    ids, first = np.unique(flat, return_index=True)
    length = np.zeros(nreg, np.uint32)
    points, codes = {}, {}
    for r, p0 in zip(ids.tolist(), first.tolist()):
        if r >= nreg:
            continue
        pts, cds = trace(bits, w, p0)
        pts, cds = np.array(pts, np.int64), np.array(cds, np.uint8)
        if orientation == 1 and len(pts) > 1:   # rule 5: the list reversed, the codes walked back
            pts, cds = pts[::-1], (np.roll(cds[::-1], -1) + 4) & 7
        length[r] = len(pts)
        points[r], codes[r] = pts, cds.astype(np.uint8)
    offsets = np.zeros(nreg + 1, np.uint64)
    offsets[1:] = np.cumsum(length.astype(np.uint64))
    total = int(offsets[-1])
    assert total < 0xFFFFFFFF
    order = sorted(points)
    at = np.concatenate([points[r] for r in order]) if order else np.zeros(0, np.int64)
    out_codes = np.concatenate([codes[r] for r in order]) if order else np.zeros(0, np.uint8)
    visits = np.bincount(at, minlength=h * w)
    assert visits.max(initial=0) <= 255
    return {"offsets": offsets.astype(np.uint32), "len": length,
            "points": ((at % w) | ((at // w) << 16)).astype(np.uint32), "codes": out_codes.astype(np.uint8),
            "visits": visits.astype(np.uint8).reshape(h, w), "total": total}
