#!/usr/bin/env python3
"""The distance transform, centres and cores on the device against the way around them.

    python tools/distance_ab.py --input smooth|batman|segments|noise [--steps 20] [--rule 0|1]
                                [--out FILE.json] [--no-host] [--host-regions N]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/distance_ab.py --input smooth --out profiles/distance/distance_ab_smooth.json && \\
    timeout -k 10 300 python tools/distance_ab.py --input batman --out profiles/distance/distance_ab_batman.json && \\
    timeout -k 10 300 python tools/distance_ab.py --input segments --out profiles/distance/distance_ab_segments.json && \\
    timeout -k 10 300 python tools/distance_ab.py --input noise --no-host --out profiles/distance/distance_ab_noise.json

Inputs, each quantised to u8 labels on the device and labelled into connected
regions (label_regions_device), 8-connectivity throughout:
    smooth    a 3840 x 2160 smooth synthetic frame at K = 256
    batman    tests/golden/png/batman.png at K = 16: its connected regions
    segments  the same after merge_regions_device with min_area 10
    noise     the 3840 x 2160 xorshift frame at K = 256 (millions of specks)
Timings, HIP events on the call's stream around the synchronous call, after
--warmup calls, single runs:
    first_ms        the first timed call alone
    distance_ms     the median of --steps calls of region_distance_device, every output asked for
    cores_ms        the same of region_cores_device (it holds a distance call)
    copy_ms         a device-to-device copy that moves the bytes of the distance
                    call's model (bytes_per_pixel_model x pixels, half read, half
                    written): what the call would cost were it bound by bytes alone
    host_ms         download of the map + scipy's distance_transform_cdt (taxicab)
                    per region on its zero-padded bounding box, one core + upload of
                    the distances, once; over the --host-regions largest regions
                    only when there are more (host_regions says how many: the
                    figure is then a lower bound of the whole)
    host_agrees     the host's distances equal the device's on those regions
launches: 11 for the distance call, 8 more for the cores call (6 of them the
component labelling, its seam pass only with more than one 64 x 64 tile), as
csrc/dq_distance.hip and csrc/dq_regions.hip enqueue them; not observed.
bytes_per_pixel_model: heads 4 + 0.25, columns 0.25 + 2, rows 2 x (4 + 2) + 2 +
2 + 2, stats 6, sums 6, nearest 4: what the passes read and write per pixel,
gathers of per-region words left out.  Prints one JSON object (and writes it
to --out).
"""
import argparse
import os
import statistics
import time

import numpy as np

import ab_common as ab

BYTES_PER_PIXEL = 4.25 + 2.25 + 18 + 6 + 6 + 4


def host_distance(reg, ids, bbox):
    """scipy's taxicab transform per region on its zero-padded bounding box."""
    from scipy.ndimage import distance_transform_cdt
    out = np.zeros(reg.shape, np.uint16)
    for r in ids:
        x0, y0, x1, y1 = (int(v) for v in bbox[r])
        box = reg[y0:y1 + 1, x0:x1 + 1] == r
        # the frame's border counts as another id, like the padding; inside the frame other ids surround the box
        d = distance_transform_cdt(np.pad(box, 1), metric="taxicab")[1:-1, 1:-1]
        out[y0:y1 + 1, x0:x1 + 1][box] = d[box]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "batman", "segments", "noise"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rule", type=int, default=0)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--host-regions", type=int, default=2000)
    ap.add_argument("--no-host", action="store_true")
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
    if a.input == "segments":
        R, _ = ab.segments_in_place(pkg, t_reg, *ab.region_graph(pkg, t_px, t_lab, t_reg, w, h, R, conn))
    torch.cuda.synchronize()

    def distance():
        return pkg.region_distance_device(t_reg, w, h, R, rule=a.rule, stream=stream)

    def cores():
        return pkg.region_cores_device(t_reg, w, h, R, rule=a.rule, connectivity=conn, stream=stream)

    for _ in range(a.warmup):
        distance()
        cores()
    ms = timed(distance, a.steps)
    cores_ms = timed(cores, a.steps)
    out = distance()
    kept, _ = cores()
    half = int(BYTES_PER_PIXEL * n / 2)
    t_a = torch.empty(half, dtype=torch.uint8, device="cuda:0")
    t_b = torch.empty(half, dtype=torch.uint8, device="cuda:0")

    def copy():
        with torch.cuda.stream(stream):
            t_b.copy_(t_a)
    for _ in range(a.warmup):
        copy()
    copy_ms = timed(copy, a.steps)
    dmax = out["dmax"].cpu().numpy().view(np.uint32)
    row = {"input": a.input, "width": w, "height": h, "regions": R, "connectivity": conn, "rule": a.rule,
           "steps": a.steps, "first_ms": ms[0], "distance_ms": statistics.median(ms), "distance_min_ms": min(ms),
           "distance_max_ms": max(ms), "cores_ms": statistics.median(cores_ms), "cores_min_ms": min(cores_ms),
           "cores_max_ms": max(cores_ms), "copy_ms": statistics.median(copy_ms), "copy_bytes": 2 * half,
           "bytes_per_pixel_model": BYTES_PER_PIXEL, "distance_launches": 11, "cores_launches": 19,
           "highest_dmax": int(dmax.max()), "kept": kept, "lib": os.path.basename(pkg.LIB_PATH)}

    if not a.no_host:
        bbox = out["bbox"].cpu().numpy().view(np.uint32)
        area = np.bincount(t_reg.cpu().numpy().view(np.uint32), minlength=R)
        ids = np.argsort(-area, kind="stable")[:a.host_regions]
        ids = ids[area[ids] > 0]
        t0 = time.perf_counter()
        reg = t_reg.cpu().numpy().view(np.uint32).reshape(h, w)
        t1 = time.perf_counter()
        d = host_distance(reg, ids, bbox)
        t2 = time.perf_counter()
        up = torch.from_numpy(d.view(np.int16)).to("cuda:0")
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        dev = out["dist"].cpu().numpy().view(np.uint16)
        on = np.isin(reg, ids)
        row["host_ms"], row["host_model_ms"], row["host_regions"] = (t3 - t0) * 1e3, (t2 - t1) * 1e3, int(ids.size)
        row["host_pixels"] = int(on.sum())
        row["host_how"] = "download + scipy distance_transform_cdt(taxicab) per region on one core + upload"
        row["host_agrees"] = bool(np.array_equal(d[on], dev[on]))
        del up

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
