"""Host models of the tag histogram of every capture window and of the inside /
outside votes of a window's quant (include/dq_hip.h, "window tags"), written
from the definition alone and using none of the code under test.

tags_model takes the window lists of windows_model (windows_model.py): per row
reg.flat[index[lo:hi]], np.unique with the first indexes and the counts,
ordered by first index; the best other is the largest count among the other
ids, ties to the lowest id.  votes_model walks the list entries with the
definition's lowest-matching-entry rule."""
import numpy as np

from windows_model import windows_model

NONE = 0xFFFFFFFF


def tags_model(reg2d, R, d, e, mask=None, area=None, min_area=0):
    """The outputs of the definition, from the window lists of windows_model."""
    reg2d = np.asarray(reg2d)
    flat = reg2d.reshape(-1)
    wm = windows_model(reg2d, R, np.zeros(reg2d.size, np.uint32), d, e, mask, area, min_area)
    off, index = wm["offsets"].astype(np.int64), wm["index"].astype(np.int64)
    rows = np.zeros(R + 1, np.int64)
    ids, counts, first = [], [], []
    inside, best, best_count = np.zeros(R, np.uint32), np.full(R, NONE, np.uint32), np.zeros(R, np.uint32)
    for r in range(R):
        tags = flat[index[off[r]:off[r + 1]]]
        tags = np.where(tags < R, tags, NONE)
        s, f, c = np.unique(tags, return_index=True, return_counts=True)
        keep = s != NONE                       # (ids >= R are counted in no entry)
        s, f, c = s[keep], f[keep], c[keep]
        order = np.argsort(f, kind="stable")
        s, f, c = s[order], f[order], c[order]
        rows[r + 1] = rows[r] + len(s)
        ids.append(s), counts.append(c), first.append(f)
        inside[r] = c[s == r].sum()
        other = s != r
        if other.any():
            top = c[other].max()
            best[r], best_count[r] = s[other][c[other] == top].min(), top
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0)).astype(np.uint32)   # noqa: E731
    out = dict(rows=rows.astype(np.uint32), ids=cat(ids), counts=cat(counts), first=cat(first), inside=inside,
               best=best, best_count=best_count, offsets=wm["offsets"], E=int(rows[-1]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def votes_model(flat, R, offsets, index, mapped, cts, k_outs, k):
    """(votes (R, 2, k), best (R, 2), misses) of the definition."""
    off = np.asarray(offsets, np.int64)
    owner = np.repeat(np.arange(R, dtype=np.int64), np.diff(off))
    idx = np.asarray(index, np.int64)[:len(owner)]
    side = (np.asarray(flat, np.int64)[idx] != owner).astype(np.int64)
    colour = np.asarray(mapped, np.uint32)[:len(owner)] & np.uint32(0xFFFFFF)
    cts = np.asarray(cts, np.uint32).reshape(R, k)
    hit = np.full(len(owner), k, np.int64)
    for i in range(k - 1, -1, -1):             # (downwards: the lowest matching entry stays)
        match = ((cts[owner, i] & np.uint32(0xFFFFFF)) == colour) & (i < np.asarray(k_outs, np.int64)[owner])
        hit[match] = i
    found = hit < k
    votes = np.bincount((owner[found] * 2 + side[found]) * k + hit[found], minlength=R * 2 * k).astype(np.uint32)
    votes = votes.reshape(R, 2, k)
    best = np.where(votes.max(axis=2) > 0, votes.argmax(axis=2), NONE).astype(np.uint32)   # (argmax: the lowest)
    return votes, best, int((~found).sum())
