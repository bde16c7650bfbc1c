#!/usr/bin/env python3
"""The region merge on the device against what surrounds it.

    python tools/merge_ab.py --input smooth|noise|batman [--steps 50] [--out FILE.json] [--no-host]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/merge_ab.py --input smooth --out profiles/merge/merge_ab_smooth.json && \\
    timeout -k 10 900 python tools/merge_ab.py --input noise --out profiles/merge/merge_ab_noise.json && \\
    timeout -k 10 300 python tools/merge_ab.py --input batman --out profiles/merge/merge_ab_batman.json

Inputs, each quantised to u8 labels on the device (quant_labels_batch_device),
labelled into connected regions with their stats (label_regions_device) and
given their edge list (region_adjacency_device), 8-connectivity throughout:
    smooth   a 3840 x 2160 smooth synthetic frame at K = 256 (a few hundred regions)
    noise    the 3840 x 2160 xorshift frame at K = 256 (millions of regions)
    batman   tests/golden/png/batman.png at K = 16 (most regions are specks)
The merge runs with --min-area 10 (the reference's MaxSmallNumPixelsVal) and no
distance limit, into a second map (the input map is kept for the next call).
Medians of --steps calls after warm-up, HIP events on the call's stream (the
call is synchronous: an event before it and one after it bracket exactly its
device work, the per-round read-backs of the link count included):
    merge_ms            dq_hip_merge_regions_dev: remap, bbox and every stats
                        array for all R' segments
    merge_renumber_ms   the same call with min_area 0 (no round: init, the
                        numbering and the pixel pass alone)
    regions_count_ms, adjacency_count_ms
                        the count-only calls of the two stages before it: what
                        dq_hip_segment_labels pays for learning R and E first
    copy_pass_ms        a plain device pass that moves what one pass over the map
                        must move at least: n label bytes read, 4 n written
    host_ms             the numpy model of tests/merge_model.py on one core,
                        once, and whether every array it gives equals the device's
launches_derived / readbacks_derived / scratch_bytes_derived are NOT observed:
they follow from the rounds, R and n by the formulas of csrc/dq_merge.h and
the host loop (the launch count agrees with the kernel trace's launches per
call plus the bitmap fill).
The per-kernel split comes from a kernel trace of this tool in a run of its own
(rocprofv3 --kernel-trace -- python tools/merge_ab.py --input X --steps 10 --no-host):
the merge_*_kernel rows.  DQ_HIP_LIB selects another build of the library (the
fold pass without LDS slots).  Prints one JSON object (and writes it to --out).
"""
import argparse
import os
import statistics
import time

import numpy as np

import ab_common as ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "noise", "batman"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--min-area", type=int, default=10)
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
    R, st, E, g = ab.region_graph(pkg, t_px, t_lab, t_reg, w, h, R, a.connectivity)
    t_edges = g["edges"] if E else None
    t_out = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def merge(min_area):
        return pkg.merge_regions_device(t_reg, R, st["area"], st["first"], st["sums"], t_edges, min_area,
                                        t_bbox=st["bbox"], num_edges=E, t_out_regions=t_out, stats_capacity=R,
                                        stream=stream)

    R2, rounds, out = merge(a.min_area)
    row = {"input": a.input, "width": w, "height": h, "k": int(len(cts[0])), "regions": R, "edges": E,
           "min_area": a.min_area, "segments": R2, "rounds": rounds, "steps": a.steps,
           "connectivity": a.connectivity, "lib": os.path.basename(pkg.LIB_PATH)}
    row["merge_ms"] = timed(lambda: merge(a.min_area))
    row["merge_renumber_ms"] = timed(lambda: merge(0))
    row["regions_count_ms"] = timed(lambda: pkg.label_regions_device(t_lab, w, h, t_out, connectivity=a.connectivity,
                                                                    stream=stream))
    row["adjacency_count_ms"] = timed(lambda: pkg.region_adjacency_device(t_reg, w, h, connectivity=a.connectivity,
                                                                         stream=stream))
    R2, rounds, out = merge(a.min_area)
    areas = out["area"].to(torch.int64)
    row["areas_sum_to_n"] = bool(int(areas.sum()) == n)
    row["smallest_segment"] = int(areas.min())
    # derived, not observed (see the docstring): init + 3 per round started + a fold per counted round + 8 to finish
    row["launches_derived"] = 1 + 3 * (rounds + 1) + rounds + 8 if E and a.min_area else 9
    row["readbacks_derived"] = (rounds + 1 if E and a.min_area else 0) + 1
    row["scratch_bytes_derived"] = R * 76 + 4 * (33 * ((n + 1023) // 1024) + 2)   # with bbox and remap

    def copy_pass():
        with torch.cuda.stream(stream):
            t_copy.copy_(t_lab)
    t_copy = torch.empty(n, dtype=torch.int32, device="cuda:0")
    row["copy_pass_ms"] = timed(copy_pass)
    row["copy_pass_bytes"] = 5 * n

    if not a.no_host:
        from merge_model import merge_model
        u = lambda t, d=np.uint32: t.cpu().numpy().view(d)  # noqa: E731
        host = {key: u(st[key], np.uint64 if key == "sums" else np.uint32) for key in ("area", "first", "sums", "bbox")}
        edges = u(t_edges).reshape(-1, 2) if E else np.zeros((0, 2), np.uint32)
        reg = u(t_reg)
        t0 = time.perf_counter()
        m = merge_model(reg, host["area"], host["first"], host["sums"], host["bbox"], edges, a.min_area)
        row["host_ms"] = (time.perf_counter() - t0) * 1e3
        row["host_how"] = "numpy model (tests/merge_model.py), one core"
        row["host_segments"], row["host_rounds"] = int(m["R"]), int(m["rounds"])
        row["host_agrees"] = bool(
            m["R"] == R2 and m["rounds"] == rounds and np.array_equal(m["regions"], u(out["regions"]))
            and np.array_equal(m["remap"], u(out["remap"])) and np.array_equal(m["area"], u(out["area"]))
            and np.array_equal(m["first"], u(out["first"])) and np.array_equal(m["bbox"], u(out["bbox"]))
            and np.array_equal(m["sums"], u(out["sums"], np.uint64)))

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
