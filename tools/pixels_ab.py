#!/usr/bin/env python3
"""The pixel lists of a region map on the device against what they replace.

    python tools/pixels_ab.py --input smooth|noise|batman [--steps 50] [--out FILE.json] [--no-host]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/pixels_ab.py --input smooth --out profiles/pixels/pixels_ab_smooth.json && \\
    timeout -k 10 600 python tools/pixels_ab.py --input noise --out profiles/pixels/pixels_ab_noise.json && \\
    timeout -k 10 300 python tools/pixels_ab.py --input batman --out profiles/pixels/pixels_ab_batman.json

Inputs as in tools/merge_ab.py, each quantised to u8 labels on the device and
labelled into connected regions (label_regions_device, 8-connectivity):
    smooth   a 3840 x 2160 smooth synthetic frame at K = 256 (a few hundred regions)
    noise    the 3840 x 2160 xorshift frame at K = 256 (millions of regions)
    batman   tests/golden/png/batman.png at K = 16 (most regions are specks)
Medians of --steps calls after warm-up, HIP events on the call's stream (the
call is synchronous: an event before it and one after it bracket exactly its
device work, the read-back of T included):
    lists_ms          dq_hip_region_pixels_dev with offsets, indexes, Coords and colours
    offsets_ms        the same call with the offsets alone (no row walk)
    copy_pass_ms      a plain device pass that moves what the lists must move at
                      least: n words read, 3 n written
    torch_sort_ms     torch.sort(regions, stable=True) alone, same device and map
    torch_lists_ms    that sort, then the offsets (bincount, cumsum) and the three
                      lists (index, Coords, colours gathered) -- the device
                      alternative; torch_agrees: every array equals the library's
    host_ms           the detour the call replaces: the map downloaded, numpy's
                      stable argsort and the lists on one core, the lists uploaded
                      (once; host_agrees likewise)
regions, rows_total (T, computed here with torch, not read from the call) and
scratch_bytes_derived (the formulas of csrc/dq_pixels.h) describe the map.
For batman the segment map (the merge with --min-area 10) also goes through
quant_region_map_device with K = 4 and a painted frame: region_map_ms, and its
stages timed apart: the lists it needs (offsets, Coords, colours), the one
weighted-regions call over the lists (its pointer arrays built beforehand),
the scatter.  The per-kernel split comes from a kernel trace of this tool in a
run of its own (rocprofv3 --kernel-trace --stats -- python tools/pixels_ab.py
--input X --steps 10 --no-host --no-alternatives): the pixels_*_kernel rows.
Prints one JSON object (and writes it to --out).
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
    ap.add_argument("--clusters", type=int, default=4)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-alternatives", action="store_true", help="the library's calls alone (for a kernel trace)")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from __graft_entry__ import load_package
    pkg = load_package()

    px, w, h, k = ab.load_input(pkg, a.input)
    n = w * h
    dev = "cuda:0"
    stream = torch.cuda.Stream(device=dev)

    def timed(fn):
        return statistics.median(ab.timed(stream, fn, a.steps, a.warmup))

    words = lambda count: torch.empty(count, dtype=torch.int32, device=dev)  # noqa: E731
    u = lambda t, d=np.uint32: t.cpu().numpy().view(d)  # noqa: E731
    t_px = torch.from_numpy(px.view(np.int32)).to(dev)
    cts, t_lab, t_reg, R = ab.region_map(pkg, t_px, w, h, k, a.connectivity)
    t_off, t_idx, t_crd, t_col = words(R + 1), words(n), words(n), words(n)
    torch.cuda.synchronize()

    def lists(everything=True):
        pkg.region_pixels_device(t_reg, w, h, R, t_off, t_coords=t_crd if everything else None,
                                 t_index=t_idx if everything else None, t_pixels=t_px if everything else None,
                                 t_colors=t_col if everything else None, stream=stream)

    reg64 = t_reg.to(torch.int64)
    ys = torch.arange(n, device=dev, dtype=torch.int64) // w
    y0 = torch.full((R,), h, dtype=torch.int64, device=dev).scatter_reduce_(0, reg64, ys, "amin")
    y1 = torch.full((R,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, reg64, ys, "amax")
    T = int((y1 - y0 + 1)[y1 >= 0].sum())
    del reg64, ys, y0, y1
    chunks = lambda c: (c + 1023) // 1024  # noqa: E731
    row = {"input": a.input, "width": w, "height": h, "k": int(len(cts[0])), "regions": R, "rows_total": T,
           "steps": a.steps, "connectivity": a.connectivity, "lib": os.path.basename(pkg.LIB_PATH),
           "scratch_bytes_derived": 4 * (2 * R + chunks(R) + 1) + 4 * (T + chunks(T) + 1),
           "lists_bytes": 4 * (R + 1) + 12 * n}
    row["lists_ms"] = timed(lists)
    row["offsets_ms"] = timed(lambda: lists(False))
    lists()
    mine = {"offsets": u(t_off), "index": u(t_idx), "coords": u(t_crd), "colors": u(t_col)}

    if not a.no_alternatives:
        t3 = torch.empty((3, n), dtype=torch.int32, device=dev)

        def copy_pass():
            with torch.cuda.stream(stream):
                t3.copy_(t_px.unsqueeze(0).expand(3, n))
        row["copy_pass_ms"] = timed(copy_pass)
        row["copy_pass_bytes"] = 16 * n
        del t3

        def torch_sort():
            with torch.cuda.stream(stream):
                return torch.sort(t_reg, stable=True)

        def torch_lists():
            with torch.cuda.stream(stream):
                _, order = torch.sort(t_reg, stable=True)
                counts = torch.bincount(t_reg, minlength=R)
                offsets = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
                index = order.to(torch.int32)
                coords = ((order % w) | ((order // w) << 16)).to(torch.int32)
                return offsets, index, coords, t_px[order]
        stream.wait_stream(torch.cuda.current_stream())
        row["torch_sort_ms"] = timed(torch_sort)
        row["torch_lists_ms"] = timed(torch_lists)
        got = torch_lists()
        stream.synchronize()
        row["torch_agrees"] = bool(all(np.array_equal(u(t), mine[key])
                                       for t, key in zip(got, ("offsets", "index", "coords", "colors"))))
        del got

    if not a.no_host:
        t0 = time.perf_counter()
        reg = u(t_reg)
        order = np.argsort(reg, kind="stable")
        host = {"offsets": np.concatenate([[0], np.cumsum(np.bincount(reg, minlength=R))]).astype(np.uint32),
                "index": order.astype(np.uint32), "coords": ((order % w) | (order // w) << 16).astype(np.uint32),
                "colors": px[order]}
        up = [torch.from_numpy(v.view(np.int32)).to(dev) for v in host.values()]
        torch.cuda.synchronize()
        row["host_ms"] = (time.perf_counter() - t0) * 1e3
        row["host_how"] = "download, numpy stable argsort and the lists on one core, upload"
        row["host_agrees"] = bool(all(np.array_equal(host[key], mine[key]) for key in host))
        del up

    if a.input == "batman":
        R, st, E, g = ab.region_graph(pkg, t_px, t_lab, t_reg, w, h, R, a.connectivity)
        t_seg = words(n)
        S, _, _ = pkg.merge_regions_device(t_reg, R, st["area"], st["first"], st["sums"], g["edges"] if E else None,
                                           a.min_area, t_bbox=st["bbox"], num_edges=E, t_out_regions=t_seg,
                                           with_remap=False)
        kk = a.clusters
        t_out, s_off, s_map = words(n), words(S + 1), words(n)
        cts4, kouts = np.zeros((S, kk), np.uint32), np.zeros(S, np.uint32)
        torch.cuda.synchronize()

        def region_map():
            return pkg.quant_region_map_device(t_seg, w, h, S, t_px, kk, t_out=t_out, cts=cts4, k_outs=kouts,
                                               stream=stream)

        def seg_lists():
            pkg.region_pixels_device(t_seg, w, h, S, s_off, t_coords=t_crd, t_pixels=t_px, t_colors=t_col,
                                     stream=stream)
        row.update({"segments": S, "clusters": kk})
        row["region_map_ms"] = timed(region_map)
        row["region_map_lists_ms"] = timed(seg_lists)
        seg_lists()
        off = u(s_off).astype(np.int64)
        row["largest_segment"] = int(np.diff(off).max())
        wr = pkg.WeightedRegions([t_col[off[r]:off[r + 1]] for r in range(S)],
                                 [s_map[off[r]:off[r + 1]] for r in range(S)], kk)
        row["region_map_quant_ms"] = timed(lambda: wr.run(stream=stream))
        row["region_map_scatter_ms"] = timed(lambda: pkg.scatter_coords_device(s_map, t_crd, n, w, t_out,
                                                                               stream=stream))
        row["region_map_offsets_readback_bytes"] = 4 * (S + 1)
        _, _, empty = region_map()
        row["region_map_empty_clusters"] = int(empty)
        painted = np.zeros(n, np.uint32)     # the stages' colours at the stages' Coords, on the host
        crd = u(t_crd)
        painted[(crd >> 16).astype(np.int64) * w + (crd & 0xFFFF)] = u(s_map)
        row["region_map_agrees_with_stages"] = bool(
            all(np.array_equal(cts4[r, :kouts[r]], wr.colortable(r)) for r in range(S))
            and np.array_equal(painted, u(t_out)))

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
