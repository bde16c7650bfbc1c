#!/usr/bin/env python3
"""The containment tree on the device against the two ways around it.

    python tools/containment_ab.py --input smooth|batman|segments|noise [--steps 20] [--torch-steps N]
                                   [--out FILE.json] [--no-host] [--no-torch]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/containment_ab.py --input smooth --out profiles/containment/containment_ab_smooth.json && \\
    timeout -k 10 300 python tools/containment_ab.py --input batman --out profiles/containment/containment_ab_batman.json && \\
    timeout -k 10 300 python tools/containment_ab.py --input segments --out profiles/containment/containment_ab_segments.json && \\
    timeout -k 10 900 python tools/containment_ab.py --input noise --no-host --torch-steps 3 --out profiles/containment/containment_ab_noise.json

Inputs, each quantised to u8 labels on the device, labelled into connected
regions (label_regions_device) and given their edge list
(region_adjacency_device), 8-connectivity throughout:
    smooth    a 3840 x 2160 smooth synthetic frame at K = 256
    batman    tests/golden/png/batman.png at K = 16: its connected regions
    segments  the same after merge_regions_device with min_area 10
    noise     the 3840 x 2160 xorshift frame at K = 256 (millions of regions,
              a tree about a thousand levels deep: the known worst case)
Timings, HIP events on the call's stream around the synchronous call (its
per-level read-backs included), after --warmup calls:
    first_ms            the first timed call alone (a single run)
    containment_ms      the median of --steps calls, every output asked for
    by_size_ms          regions_by_size_device alone
    torch_ms            the same definition written with torch on the device
                        (torch.sort by composite key, scatter_reduce / index_add
                        per level, one .item() per level), median of --steps
    host_ms             download of map, areas and edges + the same definition in
                        vectorised numpy on one core + upload of the nine arrays,
                        once (host_model_ms: the numpy part alone)
    torch_agrees, host_agrees: every array equal to the device's
levels, launches_derived and readbacks_derived: the levels are the call's own
answer; the launches follow from them and the sort's passes by the formulas of
csrc/dq_contain.hip and are NOT observed.  The kernels' share of the call comes
from a kernel trace of this tool in a run of its own (rocprofv3 --kernel-trace
--stats -- python tools/containment_ab.py --input X --steps 5 --no-host
--no-torch): the contain_*, sort_* and scan_* rows.  Prints one JSON object
(and writes it to --out).
"""
import argparse
import os
import statistics
import time

import numpy as np

import ab_common as ab

NONE = 0xFFFFFFFF
ARRAYS = ("depth", "parent", "roots", "child_offsets", "children", "subtree", "enclosed", "order", "pos")


def numpy_tree(reg2d, area, edges, R):
    """The definition of include/dq_hip.h ("containment tree") in vectorised numpy."""
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    a, b = np.concatenate([a, b]), np.concatenate([b, a])           # both directions: a reaches b
    depth = np.full(R, -1, np.int64)
    border = np.unique(np.concatenate([reg2d[0], reg2d[-1], reg2d[:, 0], reg2d[:, -1]]))
    depth[border[border < R]] = 0
    levels = 1
    while True:
        hit = (depth[a] == levels - 1) & (depth[b] < 0)
        if not hit.any():
            break
        depth[b[hit]] = levels
        levels += 1
    area64 = area.astype(np.int64)
    up = (depth[a] >= 0) & (depth[a] + 1 == depth[b])
    key = np.zeros(R, np.int64)
    np.maximum.at(key, b[up], (area64[a[up]] << 32) | (0xFFFFFFFF - a[up]))
    reached = depth >= 0
    parent = np.where(depth > 0, 0xFFFFFFFF - (key & 0xFFFFFFFF), -1)
    by_size = np.lexsort((np.arange(R), -area64))
    pkey = np.where(reached, parent + 1, R + 1)
    seq = by_size[np.argsort(pkey[by_size], kind="stable")]
    nroots, nreached = int((depth == 0).sum()), int(reached.sum())
    counts = np.bincount(parent[depth > 0], minlength=R)
    child_offsets = np.concatenate([[0], np.cumsum(counts)])
    subtree, enclosed = reached.astype(np.int64), np.where(reached, area64, 0)
    for level in range(levels - 1, 0, -1):
        at = np.flatnonzero(depth == level)
        np.add.at(subtree, parent[at], subtree[at])
        np.add.at(enclosed, parent[at], enclosed[at])
    S = np.concatenate([[0], np.cumsum(subtree[seq])])[:R]
    pos = np.full(R, -1, np.int64)
    j = np.arange(nreached)
    r = seq[:nreached]
    for level in range(levels):
        m = depth[r] == level
        rr, block = r[m], S[j[m]]
        if level:
            p = parent[rr]
            block = pos[p] - (subtree[p] - 1) + block - S[nroots + child_offsets[p]]
        pos[rr] = block + subtree[rr] - 1
    order = np.empty(nreached, np.int64)
    order[pos[r]] = r
    u = lambda x: (x & 0xFFFFFFFF).astype(np.uint32)  # noqa: E731  (-1 -> 2^32 - 1)
    return dict(depth=u(depth), parent=u(parent), roots=u(seq[:nroots]), child_offsets=u(child_offsets),
                children=u(seq[nroots:nreached]), subtree=u(subtree), enclosed=enclosed.astype(np.uint64),
                order=u(order), pos=u(pos), levels=levels, nroots=nroots, reached=nreached)


def torch_tree(torch, t_reg2d, t_area, t_edges, R):
    """The same with torch on the device; int64 throughout."""
    dev = t_area.device
    e = t_edges.to(torch.int64)
    a, b = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
    depth = torch.full((R,), -1, dtype=torch.int64, device=dev)
    border = torch.cat([t_reg2d[0], t_reg2d[-1], t_reg2d[:, 0], t_reg2d[:, -1]]).to(torch.int64)
    depth[border[border < R]] = 0
    levels = 1
    while True:
        hit = (depth[a] == levels - 1) & (depth[b] < 0)
        if not bool(hit.any().item()):
            break
        depth[b[hit]] = levels
        levels += 1
    area64 = t_area.to(torch.int64)
    up = (depth[a] >= 0) & (depth[a] + 1 == depth[b])
    key = torch.zeros(R, dtype=torch.int64, device=dev)
    key.scatter_reduce_(0, b[up], (area64[a[up]] << 32) | (0xFFFFFFFF - a[up]), reduce="amax")
    reached = depth >= 0
    parent = torch.where(depth > 0, 0xFFFFFFFF - (key & 0xFFFFFFFF), torch.full_like(key, -1))
    ids = torch.arange(R, device=dev)
    by_size = torch.sort(((0xFFFFFFFF - area64) << 32) | ids).indices          # the composite key: stable by itself
    pkey = torch.where(reached, parent + 1, torch.full_like(parent, R + 1))
    seq = by_size[torch.sort(pkey[by_size], stable=True).indices]
    nroots, nreached = int((depth == 0).sum().item()), int(reached.sum().item())
    counts = torch.bincount(parent[depth > 0], minlength=R)
    child_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
    subtree, enclosed = reached.to(torch.int64), torch.where(reached, area64, torch.zeros_like(area64))
    for level in range(levels - 1, 0, -1):
        at = torch.nonzero(depth == level).reshape(-1)
        subtree.index_add_(0, parent[at], subtree[at])
        enclosed.index_add_(0, parent[at], enclosed[at])
    S = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(subtree[seq], 0)])[:R]
    pos = torch.full((R,), -1, dtype=torch.int64, device=dev)
    j = torch.arange(nreached, device=dev)
    r = seq[:nreached]
    for level in range(levels):
        m = depth[r] == level
        rr, block = r[m], S[j[m]]
        if level:
            p = parent[rr]
            block = pos[p] - (subtree[p] - 1) + block - S[nroots + child_offsets[p]]
        pos[rr] = block + subtree[rr] - 1
    order = torch.empty(nreached, dtype=torch.int64, device=dev)
    order[pos[r]] = r
    return dict(depth=depth, parent=parent, roots=seq[:nroots], child_offsets=child_offsets,
                children=seq[nroots:nreached], subtree=subtree, enclosed=enclosed, order=order, pos=pos,
                levels=levels, nroots=nroots, reached=nreached)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "batman", "segments", "noise"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--torch-steps", type=int, default=None, help="steps of the torch formulation (default: --steps)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from __graft_entry__ import load_package
    pkg = load_package()

    px, w, h, k = ab.load_input(pkg, a.input)
    n, conn = w * h, a.connectivity
    stream = torch.cuda.Stream(device="cuda:0")

    def timed(fn, steps):
        return ab.timed(stream, fn, steps)

    t_px = torch.from_numpy(px.view(np.int32)).to("cuda:0")
    _, t_lab, t_reg, R = ab.region_map(pkg, t_px, w, h, k, conn)
    R, st, E, g = ab.region_graph(pkg, t_px, t_lab, t_reg, w, h, R, conn)
    t_area = st["area"]
    if a.input == "segments":
        R, out = ab.segments_in_place(pkg, t_reg, R, st, E, g)
        t_area = out["area"]
        E, _ = pkg.region_adjacency_device(t_reg, w, h, connectivity=conn)
        E, g = pkg.region_adjacency_device(t_reg, w, h, connectivity=conn, edge_capacity=E)
    t_edges = g["edges"] if E else None
    torch.cuda.synchronize()

    def call():
        return pkg.region_containment_device(t_reg, w, h, R, t_area, t_edges, num_edges=E, stream=stream)

    for _ in range(a.warmup):
        call()
    ms = timed(call, a.steps)
    nroots, levels, reached, out = call()
    row = {"input": a.input, "width": w, "height": h, "regions": R, "edges": E, "connectivity": conn,
           "steps": a.steps, "nroots": nroots, "levels": levels, "reached": reached,
           "first_ms": ms[0], "containment_ms": statistics.median(ms), "containment_min_ms": min(ms),
           "containment_max_ms": max(ms), "lib": os.path.basename(pkg.LIB_PATH)}
    area_bits = int(t_area.max().item()).bit_length()
    passes = max(1, (area_bits + 7) // 8) + max(1, ((R + 1).bit_length() + 7) // 8)
    # derived, not observed: init, border, roots; a level launch per level (the last finds nobody, unless all are
    # reached); parent, settle; 5 per sort pass; rows; two scans of 3; a fold per level below the roots; a place
    # per level
    level_launches = levels - 1 + (1 if reached < R else 0) if E else 0
    row["launches_derived"] = (3 + level_launches + (2 if E else 1) + 5 * passes + (1 if reached > nroots else 0) + 6
                               + (levels - 1) + levels)
    row["readbacks_derived"] = 1 + level_launches
    row["sort_passes_derived"] = passes
    row["by_size_ms"] = statistics.median(timed(lambda: pkg.regions_by_size_device(t_area, R, stream=stream), a.steps))

    u = lambda t, d=np.uint32: t.cpu().numpy().view(d)  # noqa: E731
    dev = {key: u(out[key], np.uint64 if key == "enclosed" else np.uint32) for key in ARRAYS}
    t_reg2d = t_reg.reshape(h, w)

    if not a.no_torch:
        def with_torch():
            with torch.cuda.stream(stream):
                return torch_tree(torch, t_reg2d, t_area, t_edges, R)
        torch.cuda.synchronize()
        for _ in range(2):
            with_torch()
        row["torch_steps"] = a.steps if a.torch_steps is None else a.torch_steps
        row["torch_ms"] = statistics.median(timed(with_torch, row["torch_steps"]))
        t = with_torch()
        stream.synchronize()
        row["torch_agrees"] = bool(
            (t["nroots"], t["levels"], t["reached"]) == (nroots, levels, reached)
            and all(np.array_equal((t[key].cpu().numpy() & (0xFFFFFFFF if key != "enclosed" else -1)).astype(
                np.uint64), dev[key].astype(np.uint64)) for key in ARRAYS))

    if not a.no_host:
        t0 = time.perf_counter()
        reg, area, edges = u(t_reg).reshape(h, w), u(t_area), u(t_edges).reshape(-1, 2)
        t1 = time.perf_counter()
        m = numpy_tree(reg, area, edges, R)
        t2 = time.perf_counter()
        up = [torch.from_numpy(m[key].view(np.int64 if key == "enclosed" else np.int32)).to("cuda:0") for key in ARRAYS]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        row["host_ms"], row["host_model_ms"] = (t3 - t0) * 1e3, (t2 - t1) * 1e3
        row["host_how"] = "download + vectorised numpy on one core + upload"
        row["host_agrees"] = bool((m["nroots"], m["levels"], m["reached"]) == (nroots, levels, reached)
                                  and all(np.array_equal(m[key], dev[key]) for key in ARRAYS))
        del up

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
