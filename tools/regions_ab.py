#!/usr/bin/env python3
"""Connected regions of a label map on the device against what surrounds them.

    python tools/regions_ab.py [--steps 50] [--out FILE.json] [--no-host]

Inputs, each quantised to u8 labels on the device first (quant_labels_batch_device):
    smooth   a 3840 x 2160 smooth synthetic frame at K = 256 (a few thousand regions)
    noise    the 3840 x 2160 xorshift frame at K = 256 (millions of regions: the
             worst case for the atomics and for the scan)
    batman   tests/golden/png/batman.png at K = 16
Per input, medians of --steps calls after warm-up, HIP events on the call's
stream (the call is synchronous: an event before it and one after it bracket
exactly its device work):
    regions_ms        dq_hip_label_regions_dev, map only (capacity 0), 8-connectivity
    regions_stats_ms  the same with every stat for all R regions, colour sums included
    copy_pass_ms      a plain device pass that moves what one pass of the six must
                      move at least: label_bytes * n read, 4 n written (a widening copy)
    map_ms            the label map kernel that produced the input (the library's
                      stat kind 7 of the quantise call)
    host_ms           the same regions on the host, once: scipy.ndimage.label per
                      label value where scipy can be imported, else the flood
                      fill of tests/regions_model.py (only up to --host-max pixels)
The per-pass split comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/regions_ab.py --steps 10 --no-host):
the six region_*_kernel rows.  Prints one JSON object (and writes it to --out).
"""
import argparse
import statistics
import time

import numpy as np

import ab_common as ab


def host_regions(lab2d, connectivity, host_max):
    """(ms, R, how) of the regions on the host."""
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    t0 = time.perf_counter()
    if ndimage is not None:
        structure = np.ones((3, 3), int) if connectivity == 8 else None
        count = 0
        for v in np.unique(lab2d):
            count += ndimage.label(lab2d == v, structure=structure)[1]
        return (time.perf_counter() - t0) * 1e3, int(count), "scipy.ndimage.label per label value"
    if lab2d.size > host_max:
        return None, None, "skipped: flood fill of %d pixels" % lab2d.size
    from regions_model import flood_fill_regions
    _, st = flood_fill_regions(lab2d, connectivity)
    return (time.perf_counter() - t0) * 1e3, int(len(st["area"])), "python flood fill (tests/regions_model.py)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-max", type=int, default=2_000_000)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.set_timing(True)

    inputs = [(name,) + ab.load_input(pkg, name) for name in ("smooth", "noise", "batman")]
    stream = torch.cuda.Stream(device="cuda:0")

    def timed(fn):
        return statistics.median(ab.timed(stream, fn, a.steps, a.warmup))

    res = {"steps": a.steps, "connectivity": a.connectivity, "label_bytes": 1, "inputs": {}}
    for name, px, w, h, k in inputs:
        n = w * h
        t_px = torch.from_numpy(px.view(np.int32)).to("cuda:0")
        t_lab = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        pkg.reset_stats()
        cts, _ = pkg.quant_labels_batch_device([t_px], [t_lab], k)
        launches, map_ms = pkg.get_stats()["map"][:2]
        t_reg = torch.empty(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        R, _ = pkg.label_regions_device(t_lab, w, h, t_reg, connectivity=a.connectivity, stream=stream)
        row = {"width": w, "height": h, "k": int(len(cts[0])), "regions": R,
               "map_ms": map_ms / max(launches, 1), "map_launches": launches}
        row["regions_ms"] = timed(lambda: pkg.label_regions_device(t_lab, w, h, t_reg, connectivity=a.connectivity,
                                                                   stream=stream))
        row["regions_stats_ms"] = timed(lambda: pkg.label_regions_device(
            t_lab, w, h, t_reg, connectivity=a.connectivity, stats_capacity=R, t_pixels=t_px, stream=stream))
        R2, st = pkg.label_regions_device(t_lab, w, h, t_reg, connectivity=a.connectivity, stats_capacity=R,
                                          t_pixels=t_px, stream=stream)
        row["area_sums_to_n"] = bool(R2 == R and int(st["area"].to(torch.int64).sum()) == n)

        def copy_pass():
            with torch.cuda.stream(stream):
                t_reg.copy_(t_lab)
        row["copy_pass_ms"] = timed(copy_pass)
        row["copy_pass_bytes"] = 5 * n
        row["passes"] = 6
        if not a.no_host:
            ms, hr, how = host_regions(t_lab.cpu().numpy().reshape(h, w), a.connectivity, a.host_max)
            row["host_ms"], row["host_regions"], row["host_how"] = ms, hr, how
            row["host_agrees_on_R"] = None if hr is None else bool(hr == R)
        res["inputs"][name] = row
        del t_px, t_lab, t_reg

    ab.emit(res, a.out)


if __name__ == "__main__":
    main()
