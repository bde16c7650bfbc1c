#!/usr/bin/env python3
"""The region adjacency graph on the device against what surrounds it.

    python tools/adjacency_ab.py --input smooth|noise|batman [--steps 50] [--out FILE.json] [--no-host]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/adjacency_ab.py --input smooth --out profiles/adjacency/smooth.json && \\
    timeout -k 10 600 python tools/adjacency_ab.py --input noise --out profiles/adjacency/noise.json && \\
    timeout -k 10 300 python tools/adjacency_ab.py --input batman --out profiles/adjacency/batman.json

Inputs, each quantised to u8 labels on the device (quant_labels_batch_device)
and then labelled into connected regions (label_regions_device, 8-connectivity):
    smooth   a 3840 x 2160 smooth synthetic frame at K = 256 (a few hundred regions)
    noise    the 3840 x 2160 xorshift frame at K = 256 (millions of regions,
             every contact its own edge: the worst case for the table)
    batman   tests/golden/png/batman.png at K = 16
Medians of --steps calls after warm-up, HIP events on the call's stream (the
call is synchronous: an event before it and one after it bracket exactly its
device work, the read-back of the head count between its two halves included):
    adjacency_ms        dq_hip_region_adjacency_dev, every edge array for all E
                        edges, step sums and the degree of all R regions
    adjacency_count_ms  the count-only call (capacity 0, no array)
    copy_pass_ms        a plain device pass that moves what one pass over the map
                        must move at least: n label bytes read, 4 n written
    host_ms             the numpy model of tests/adjacency_model.py on one
                        core, once, and whether it agrees on E
heads / table_slots / scratch_bytes: the heads are recomputed here on the host
by the rule of csrc/dq_adjacency.hip (per direction, runs of equal id pairs
along 64 consecutive pixels); the rest follows the formula in include/dq_hip.h.
The per-pass split comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/adjacency_ab.py --input X --steps 10 --no-host):
the adjacency_*_kernel rows.  DQ_HIP_LIB selects another build of the library
(the insert pass without LDS slots).  Prints one JSON object (and writes it to --out).
"""
import argparse
import os
import statistics
import time

import numpy as np

import ab_common as ab

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def count_heads(reg2d, connectivity):
    """Heads of a region map: per direction, a pixel with a contact whose key
    differs from the key of the pixel before it, or whose index is a multiple
    of 64 (the first lane of a wave)."""
    h, w = reg2d.shape
    r = reg2d.astype(np.uint64)
    heads = 0
    shifts = [(0, 1)] + ([(1, -1)] if connectivity == 8 else []) + [(1, 0)] + ([(1, 1)] if connectivity == 8 else [])
    wave_start = (np.arange(h * w) % 64) == 0
    for dy, dx in shifts:
        key = np.full((h, w), NO_KEY, np.uint64)
        ys = slice(0, h - dy)
        xs = slice(max(0, -dx), w - max(0, dx))
        xq = slice(max(0, -dx) + dx, w - max(0, dx) + dx)
        a, b = r[ys, xs], r[dy:, xq] if dy else r[:, xq]
        k = (np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)
        key[ys, xs] = np.where(a != b, k, NO_KEY)
        key = key.reshape(-1)
        start = wave_start.copy()
        start[1:] |= key[1:] != key[:-1]
        heads += int(np.count_nonzero(start & (key != NO_KEY)))
    return heads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "noise", "batman"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from __graft_entry__ import load_package
    pkg = load_package()

    px, w, h, k = ab.load_input(pkg, a.input)
    n = w * h
    stream = torch.cuda.Stream(device="cuda:0")

    def timed(fn):
        return statistics.median(ab.timed(stream, fn, a.steps, a.warmup))

    t_px = torch.from_numpy(px.view(np.int32)).to("cuda:0")
    cts, t_lab, t_reg, R = ab.region_map(pkg, t_px, w, h, k, a.connectivity)
    torch.cuda.synchronize()

    adj = lambda **kw: pkg.region_adjacency_device(t_reg, w, h, connectivity=a.connectivity,  # noqa: E731
                                                   stream=stream, **kw)
    E, _ = adj()
    row = {"input": a.input, "width": w, "height": h, "k": int(len(cts[0])), "regions": R, "edges": E,
           "steps": a.steps, "connectivity": a.connectivity, "lib": os.path.basename(pkg.LIB_PATH)}
    row["adjacency_count_ms"] = timed(lambda: adj())
    row["adjacency_ms"] = timed(lambda: adj(edge_capacity=E, t_pixels=t_px, num_regions=R))
    E2, g = adj(edge_capacity=E, t_pixels=t_px, num_regions=R)
    row["degree_sums_to_2E"] = bool(E2 == E and int(g["degree"].to(torch.int64).sum()) == 2 * E)
    row["border_sum"] = int(g["border"].to(torch.int64).sum())

    def copy_pass():
        with torch.cuda.stream(stream):
            t_reg2.copy_(t_lab)
    t_reg2 = torch.empty(n, dtype=torch.int32, device="cuda:0")
    row["copy_pass_ms"] = timed(copy_pass)
    row["copy_pass_bytes"] = 5 * n
    row["passes"] = 4   # pixel passes: count, insert, flag, emit

    reg2d = t_reg.cpu().numpy().view(np.uint32).reshape(h, w)
    heads = count_heads(reg2d, a.connectivity)
    slots = max(1024, 1 << max(0, (2 * heads - 1).bit_length()))
    row["heads"], row["table_slots"] = heads, slots
    row["scratch_bytes"] = slots * 24 + 4 * ((n + 1023) // 1024) + 4
    row["scratch_bytes_count_only"] = slots * 16 + 4 * ((n + 1023) // 1024) + 4
    if not a.no_host:
        from adjacency_model import adjacency_model
        t0 = time.perf_counter()
        m = adjacency_model(reg2d, a.connectivity, px, R)
        row["host_ms"] = (time.perf_counter() - t0) * 1e3
        row["host_how"] = "numpy model (tests/adjacency_model.py), one core"
        row["host_edges"] = int(m["E"])
        row["host_agrees"] = bool(
            m["E"] == E and np.array_equal(m["edges"], g["edges"].cpu().numpy().view(np.uint32))
            and np.array_equal(m["border"], g["border"].cpu().numpy().view(np.uint32))
            and np.array_equal(m["contact"], g["contact"].cpu().numpy().view(np.uint32))
            and np.array_equal(m["step"], g["step"].cpu().numpy().view(np.uint64))
            and np.array_equal(m["degree"], g["degree"].cpu().numpy().view(np.uint32)))

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
