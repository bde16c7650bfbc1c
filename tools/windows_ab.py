#!/usr/bin/env python3
"""The capture windows of a region map on the device against what they replace.

    python tools/windows_ab.py --input smooth|noise|batman [--steps 20] [--out FILE.json] [--no-host]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/windows_ab.py --input smooth --out profiles/windows/windows_ab_smooth.json && \\
    timeout -k 10 600 python tools/windows_ab.py --input noise --out profiles/windows/windows_ab_noise.json && \\
    timeout -k 10 300 python tools/windows_ab.py --input batman --out profiles/windows/windows_ab_batman.json

Inputs and region maps as in tools/pixels_ab.py (u8 labels, label_regions_device,
8-connectivity); block 4, expand 2, no mask, no area rule: the reference's
windows.  Medians of --steps calls after warm-up, HIP events on the call's
stream (the call is synchronous: an event before it and one after it bracket
exactly its device work, the read-backs of P, T and M included):
    count_ms          dq_hip_region_windows_dev without list arrays: the offsets and M
    lists_ms          the same call with indexes, Coords and colours, capacity M
                      (lists_skipped instead when 12 M bytes exceed --max-list-bytes)
    torch_count_ms    the device alternative up to the offsets: torch.unique of
                      (id, block), the 13 shifted copies, torch.unique again (the
                      windows, id-major in raster order), block sizes, cumsum
    torch_lists_ms    that, then the three lists by repeat_interleave and
                      arithmetic; torch_agrees: every array equals the library's
                      (torch_lists_skipped when M exceeds --max-alt-entries)
    host_ms           the detour the call replaces: the map downloaded, the same
                      formulation with numpy on one core, the lists uploaded
                      (once; host_agrees likewise; the offsets alone when M
                      exceeds --max-alt-entries)
regions, pairs (P), rows_total (T) -- computed here with torch, not read from
the call -- entries (M) and scratch_bytes_derived (the formulas of
csrc/dq_windows.h) describe the map.  For batman the segment map (the merge
with --min-area 10) goes through the same calls with the reference's area rule
(min_area = 8, superpixelDim^2 / 2): the segments_* fields.
Prints one JSON object (and writes it to --out).
"""
import argparse
import os
import statistics
import time

import numpy as np

import ab_common as ab

D, E = 4, 2
BALL = [(dy, dx) for dy in range(-E, E + 1) for dx in range(-(E - abs(dy)), E - abs(dy) + 1)]


def formulation(xp, reg, w, h, R, px, lists):
    """The windows by sorting: xp is numpy or torch, reg the ids as int64.  Returns (offsets, index,
    coords, colours, P, T); the lists are None without `lists`."""
    tor = xp.__name__ == "torch"
    kw = dict(device=reg.device) if tor else {}
    cat = xp.cat if tor else xp.concatenate
    repeat = xp.repeat_interleave if tor else xp.repeat
    bw, bh = -(-w // D), -(-h // D)
    nb = bw * bh
    p = xp.arange(w * h, dtype=xp.int64, **kw)
    own = xp.unique(reg * nb + (p // w // D) * bw + (p % w) // D)
    ids, bj, bi = own // nb, own % nb // bw, own % bw
    shifted = []
    for dy, dx in BALL:
        nj, ni = bj + dy, bi + dx
        ok = (nj >= 0) & (nj < bh) & (ni >= 0) & (ni < bw)
        shifted.append((ids * nb + nj * bw + ni)[ok])
    win = xp.unique(cat(shifted))                      # sorted: id-major, blocks in raster order
    wid, wj, wi = win // nb, win % nb // bw, win % bw
    cols, rows = xp.clip(w - wi * D, None, D), xp.clip(h - wj * D, None, D)
    lens = cols * rows
    if tor:
        per_id = xp.zeros(R, dtype=xp.int64, **kw).scatter_add_(0, wid, lens)
    else:
        per_id = np.bincount(wid, weights=lens, minlength=R).astype(np.int64)   # (exact: below 2^53)
    offsets = cat([xp.zeros(1, dtype=xp.int64, **kw), xp.cumsum(per_id, 0)])
    j0, j1 = xp.full((R,), bh, dtype=xp.int64, **kw), xp.full((R,), -1, dtype=xp.int64, **kw)
    if tor:
        j0.scatter_reduce_(0, ids, bj, "amin")
        j1.scatter_reduce_(0, ids, bj, "amax")
    else:
        np.minimum.at(j0, ids, bj)
        np.maximum.at(j1, ids, bj)
    span = xp.clip(j1 + E, None, bh - 1) - xp.clip(j0 - E, 0, None) + 1
    T = int(span[j1 >= 0].sum())
    out = [offsets, None, None, None, int(len(win)), T]
    if lists:
        start = xp.cumsum(lens, 0) - lens
        pair = repeat(xp.arange(len(win), dtype=xp.int64, **kw), lens)
        rank = xp.arange(int(offsets[-1]), dtype=xp.int64, **kw) - start[pair]
        x, y = wi[pair] * D + rank % cols[pair], wj[pair] * D + rank // cols[pair]
        index = y * w + x
        out[1:4] = index, x | (y << 16), px[index]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "noise", "batman"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--min-area", type=int, default=10)
    ap.add_argument("--max-list-bytes", type=int, default=64 << 30)
    ap.add_argument("--max-alt-entries", type=int, default=1 << 28)
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

    words = lambda count: torch.empty(max(count, 1), dtype=torch.int32, device=dev)  # noqa: E731
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    chunks = lambda c: (c + 1023) // 1024  # noqa: E731
    t_px = torch.from_numpy(px.view(np.int32)).to(dev)
    cts, t_lab, t_reg, R = ab.region_map(pkg, t_px, w, h, k, a.connectivity)
    torch.cuda.synchronize()
    row = {"input": a.input, "width": w, "height": h, "k": int(len(cts[0])), "steps": a.steps, "block": D, "expand": E,
           "connectivity": a.connectivity, "lib": os.path.basename(pkg.LIB_PATH)}

    def measure(t_map, R, prefix, t_area=None, min_area=0):
        """The library's calls and the alternatives on one map; fields get `prefix`."""
        t_off = words(R + 1)
        kw = dict(block=D, expand=E, t_area=t_area, min_area=min_area, stream=stream)
        M = pkg.region_windows_device(t_map, w, h, R, t_off, **kw)
        nb = -(-w // D) * -(-h // D)
        out = {"regions": R, "entries": M, "lists_bytes": 4 * (R + 1) + 12 * M}
        out["count_ms"] = timed(lambda: pkg.region_windows_device(t_map, w, h, R, t_off, **kw))
        mine = {"offsets": u(t_off)[:R + 1].copy()}
        if 12 * M <= a.max_list_bytes:
            t_idx, t_crd, t_col = words(M), words(M), words(M)

            def lists():
                pkg.region_windows_device(t_map, w, h, R, t_off, capacity=M, t_coords=t_crd, t_index=t_idx,
                                          t_pixels=t_px, t_colors=t_col, **kw)
            out["lists_ms"] = timed(lists)
            if M <= a.max_alt_entries:
                mine.update(index=u(t_idx)[:M], coords=u(t_crd)[:M], colors=u(t_col)[:M])
            del t_idx, t_crd, t_col
        else:
            out["lists_skipped"] = "12 M bytes exceed --max-list-bytes"
        keys = ("offsets", "index", "coords", "colors")
        with_lists = M <= a.max_alt_entries and t_area is None
        if not a.no_alternatives and t_area is None:
            reg64 = t_map[:n].to(torch.int64)

            def alt(lists):
                with torch.cuda.stream(stream):
                    return formulation(torch, reg64, w, h, R, t_px, lists)
            stream.wait_stream(torch.cuda.current_stream())
            got = alt(False)
            stream.synchronize()
            out.update(pairs=got[4], rows_total=got[5])
            out["scratch_bytes_derived"] = (4 * ((D * D + 2) * nb + 1 + chunks(nb + 1) + 1 + 2 * R + chunks(R) + 1)
                                            + 4 * (2 * got[4] + got[5] + chunks(got[5]) + 1))
            out["torch_count_ms"] = timed(lambda: alt(False))
            if with_lists:
                out["torch_lists_ms"] = timed(lambda: alt(True))
                got = alt(True)
                stream.synchronize()
            else:
                out["torch_lists_skipped"] = "M exceeds --max-alt-entries"
            out["torch_agrees"] = bool(all(np.array_equal(t.cpu().numpy().astype(np.uint32), mine[key])
                                           for t, key in zip(got[:4], keys) if t is not None and key in mine))
            del got, reg64
        if not a.no_host and t_area is None:
            t0 = time.perf_counter()
            host = formulation(np, u(t_map)[:n].astype(np.int64), w, h, R, px, with_lists)
            up = [torch.from_numpy(v.astype(np.uint32).view(np.int32)).to(dev) for v in host[:4] if v is not None]
            torch.cuda.synchronize()
            out["host_ms"] = (time.perf_counter() - t0) * 1e3
            out["host_how"] = ("download, the windows by numpy's unique on one core, %s, upload"
                               % ("the lists" if with_lists else "the offsets alone"))
            out["host_agrees"] = bool(all(np.array_equal(v.astype(np.uint32), mine[key])
                                          for v, key in zip(host[:4], keys) if v is not None and key in mine))
            del up, host
        row.update({prefix + key: v for key, v in out.items()})

    measure(t_reg, R, "")

    if a.input == "batman":
        R, st, Ed, g = ab.region_graph(pkg, t_px, t_lab, t_reg, w, h, R, a.connectivity)
        t_seg = words(n)
        S, _, seg = pkg.merge_regions_device(t_reg, R, st["area"], st["first"], st["sums"],
                                                g["edges"] if Ed else None, a.min_area, t_bbox=st["bbox"],
                                                num_edges=Ed, t_out_regions=t_seg, with_remap=False,
                                                stats_capacity=R)
        torch.cuda.synchronize()
        row["segments_min_area_rule"] = D * D // 2
        measure(t_seg, S, "segments_", t_area=seg["area"], min_area=D * D // 2)

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
