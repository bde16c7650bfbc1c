#!/usr/bin/env python3
"""The window tags and votes of a region map on the device against what they replace.

    python tools/wtags_ab.py --input smooth|noise|batman [--steps 20] [--out FILE.json] [--no-host] [--no-votes]
                             [--no-alternatives]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/wtags_ab.py --input smooth --out profiles/wtags/wtags_ab_smooth.json && \\
    timeout -k 10 300 python tools/wtags_ab.py --input batman --out profiles/wtags/wtags_ab_batman.json && \\
    timeout -k 10 600 python tools/wtags_ab.py --input noise --out profiles/wtags/wtags_ab_noise.json

Inputs and region maps as in tools/windows_ab.py (u8 labels, label_regions_device,
8-connectivity); block 4, expand 2, no mask.  `batman` also runs its segment map
(the merge with --min-area 10) with the reference's area rule (min_area = 8):
the segments_* fields.  `noise` runs the 4K noise frame with the area rule
only (it leaves almost no window, as in the reference) and the region map of
the frame's top left 512 x 512 crop without it: the crop_* fields.
Every comparison is asserted equal before anything is timed.  Medians of
--steps calls after --warmup, HIP events on the call's stream (the call is
synchronous: the events bracket exactly its device work, read-backs included):
    count_ms          dq_hip_window_tags_dev with d_rows alone: E and the CSR offsets
    full_ms           the same call with all seven arrays and the offsets, capacity E
    windows_ms        dq_hip_region_windows_dev without list arrays on the same map: the
                      part of the call that is the shared windows stage (without the walk)
    torch_ms          the same tables on the same device from the windows lists: the
                      windows call with indexes at capacity M, torch.unique of
                      (row, id) with the counts, the first positions by scatter-min,
                      a sort by first position (skipped when M exceeds --max-alt-entries)
    host_ms           the detour the call replaces: indexes and offsets downloaded,
                      numpy's unique on one core, the tables uploaded (once)
    votes_ms          dq_hip_window_votes_dev at K = 4 on the mapped colours of
                      quant_region_windows_device (K = 4); votes_misses must be 0
entries (E) is what the call returned; contributions (Q) and pairs (P) are
computed here with torch, not read from the call; scratch_bytes_derived follows
from them by the formulas of csrc/dq_windows.h and csrc/dq_wtags.h.
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
NONE = 0xFFFFFFFF
KEYS = ("rows", "ids", "counts", "first", "inside", "best", "best_count")


def tables(xp, owner_tag, pos, offsets, R):
    """The seven arrays from the (row, id) key and the global list position of every list entry
    with an id < R; xp is numpy or torch."""
    tor = xp.__name__ == "torch"
    kw = dict(device=owner_tag.device) if tor else {}
    if tor:
        keys, inv, counts = xp.unique(owner_tag, return_inverse=True, return_counts=True)
        first = xp.full((len(keys),), 1 << 62, dtype=xp.int64, **kw).scatter_reduce_(0, inv, pos, "amin")
        order = xp.argsort(first)
    else:
        keys, at, counts = np.unique(owner_tag, return_index=True, return_counts=True)
        first = pos[at]                                     # (pos ascends: the first occurrence is the lowest)
        order = np.argsort(first, kind="stable")
    keys, counts, first = keys[order], counts[order], first[order]
    row, ids = keys // R, keys % R
    per_row = xp.bincount(row, minlength=R)
    rows = xp.cumsum(per_row, 0)
    rows = (xp.cat if tor else np.concatenate)([xp.zeros(1, dtype=xp.int64, **kw), rows])
    inside = xp.zeros(R, dtype=xp.int64, **kw)
    own = ids == row
    inside[row[own]] = counts[own]
    # the best other: the largest count, ties to the lowest id
    score = counts[~own] * (1 << 32) + (NONE - ids[~own])
    best = xp.zeros(R, dtype=xp.int64, **kw)
    if tor:
        best.scatter_reduce_(0, row[~own], score, "amax")
    else:
        np.maximum.at(best, row[~own], score)
    best_id = xp.where(best > 0, NONE - best % (1 << 32), xp.full_like(best, NONE))
    return dict(rows=rows, ids=ids, counts=counts, first=first - offsets[row], inside=inside, best=best_id,
                best_count=best >> 32)


def contributions(torch, reg64, w, h, R, area, min_area):
    """(P, Q) of a map, from the definition: the pairs (window block, member id) and, over them, the
    distinct ids of the block (no mask: every pixel survives)."""
    bw, bh = -(-w // D), -(-h // D)
    nb = bw * bh
    p = torch.arange(w * h, dtype=torch.int64, device=reg64.device)
    block = (p // w // D) * bw + (p % w) // D
    own = torch.unique(reg64 * nb + block)
    live = torch.bincount(own % nb, minlength=nb)
    if area is not None:
        own = own[area.to(torch.int64)[own // nb] > min_area]
    ids, bj, bi = own // nb, own % nb // bw, own % bw
    shifted = []
    for dy, dx in BALL:
        nj, ni = bj + dy, bi + dx
        ok = (nj >= 0) & (nj < bh) & (ni >= 0) & (ni < bw)
        shifted.append((ids * nb + nj * bw + ni)[ok])
    win = torch.unique(torch.cat(shifted))
    return int(len(win)), int(live[win % nb].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "noise", "batman"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--min-area", type=int, default=10)
    ap.add_argument("--max-alt-entries", type=int, default=1 << 27)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-votes", action="store_true")
    ap.add_argument("--no-alternatives", action="store_true", help="the library's calls alone (for a kernel trace)")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from __graft_entry__ import load_package
    pkg = load_package()

    px, w, h, k = ab.load_input(pkg, a.input)
    dev = "cuda:0"
    stream = torch.cuda.Stream(device=dev)

    def timed(fn):
        return statistics.median(ab.timed(stream, fn, a.steps, a.warmup))

    words = lambda count: torch.empty(max(count, 1), dtype=torch.int32, device=dev)  # noqa: E731
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    chunks = lambda c: (c + 1023) // 1024  # noqa: E731
    row = {"input": a.input, "steps": a.steps, "block": D, "expand": E, "connectivity": a.connectivity,
           "lib": os.path.basename(pkg.LIB_PATH)}

    def region_map(px, w, h, k, stats=False):
        t_px = torch.from_numpy(np.ascontiguousarray(px).view(np.int32)).to(dev)
        _, t_lab, t_reg, R = ab.region_map(pkg, t_px, w, h, k, a.connectivity)
        st = None
        if stats:
            R, st = pkg.label_regions_device(t_lab, w, h, t_reg, connectivity=a.connectivity, stats_capacity=R,
                                             t_pixels=t_px)
        torch.cuda.synchronize()
        return t_px, t_lab, t_reg, R, st

    def measure(t_map, t_px, w, h, R, prefix, t_area=None, min_area=0):
        """The library's calls and the alternatives on one map; fields get `prefix`."""
        n = w * h
        kw = dict(block=D, expand=E, t_area=t_area, min_area=min_area, stream=stream)
        t_rows, t_off = words(R + 1), words(R + 1)
        entries = pkg.window_tags_device(t_map, w, h, R, t_rows, **kw)
        M = pkg.region_windows_device(t_map, w, h, R, t_off, **kw)
        t = {key: words(entries) for key in ("ids", "counts", "first")}
        t.update({key: words(R) for key in ("inside", "best", "best_count")})

        def full():
            return pkg.window_tags_device(t_map, w, h, R, t_rows, capacity=entries, t_ids=t["ids"],
                                          t_counts=t["counts"], t_first=t["first"], t_inside=t["inside"],
                                          t_best=t["best"], t_best_count=t["best_count"], t_offsets=t_off, **kw)
        assert full() == entries
        sizes = dict(rows=R + 1, ids=entries, counts=entries, first=entries, inside=R, best=R, best_count=R)
        mine = {key: u(t_rows if key == "rows" else t[key])[:sizes[key]].copy() for key in KEYS}
        offsets = u(t_off)[:R + 1].astype(np.int64)
        assert int(offsets[-1]) == M
        nb = -(-w // D) * -(-h // D)
        out = {"width": w, "height": h, "regions": R, "list_entries": M, "entries": entries,
               "lists_bytes_avoided": 4 * (R + 1) + 4 * M}
        reg64 = t_map[:n].to(torch.int64)
        P, Q = contributions(torch, reg64, w, h, R, t_area, min_area)
        slots = min(max(2 * Q, 1024), (1 << 32) - 1)
        bits = M // 32 + 2
        out.update(pairs=P, contributions=Q, table_slots=slots)
        out["scratch_bytes_derived_own"] = 4 * (P + nb + chunks(nb) + 1 + 4 * slots + 3 * R + 2 * bits
                                                + chunks(bits) + 1)
        # the alternatives, from the windows lists; each asserted equal before anything is timed
        lists_ok = M <= a.max_alt_entries and not a.no_alternatives
        if lists_ok:
            t_idx = words(M)

            def lists():
                pkg.region_windows_device(t_map, w, h, R, t_off, capacity=M, t_index=t_idx, **kw)

            def alt():
                lists()
                with torch.cuda.stream(stream):
                    off = t_off[:R + 1].to(torch.int64)
                    owner = torch.repeat_interleave(torch.arange(R, dtype=torch.int64, device=dev), off[1:] - off[:-1])
                    tag = reg64[t_idx[:M].to(torch.int64)]
                    pos = torch.arange(M, dtype=torch.int64, device=dev)
                    keep = tag < R
                    return tables(torch, (owner * R + tag)[keep], pos[keep], off, R)
            got = alt()
            stream.synchronize()
            for key in KEYS:
                assert np.array_equal(got[key].cpu().numpy().astype(np.uint32), mine[key]), (prefix, "torch", key)
            out["torch_agrees"] = True
            del got
            if not a.no_host:
                t0 = time.perf_counter()
                lists()
                index, off = u(t_idx)[:M].astype(np.int64), u(t_off)[:R + 1].astype(np.int64)
                flat = u(t_map)[:n].astype(np.int64)
                owner = np.repeat(np.arange(R, dtype=np.int64), np.diff(off))
                tag = flat[index]
                keep = tag < R
                host = tables(np, (owner * R + tag)[keep], np.arange(M, dtype=np.int64)[keep], off, R)
                up = [torch.from_numpy(host[key].astype(np.uint32).view(np.int32)).to(dev) for key in KEYS]
                torch.cuda.synchronize()
                out["host_ms"] = (time.perf_counter() - t0) * 1e3
                for key in KEYS:
                    assert np.array_equal(host[key].astype(np.uint32), mine[key]), (prefix, "host", key)
                out["host_agrees"] = True
                del up, host, index, flat, owner, tag
        else:
            out["alternatives_skipped"] = "M exceeds --max-alt-entries"
        votes = None
        if not a.no_votes and 0 < M <= a.max_alt_entries:
            kv = 4
            t_idx, t_out = words(M), words(M)
            cts, k_outs, _ = pkg.quant_region_windows_device(t_map, w, h, R, t_px, kv, t_off, capacity=M, t_out=t_out,
                                                             t_index=t_idx, **kw)
            t_votes, t_vbest = words(R * 2 * kv), words(R * 2)
            votes = lambda: pkg.window_votes_device(t_map, n, R, t_off, t_idx, M, t_out, cts, k_outs, kv, t_votes,  # noqa: E731
                                                    t_vbest, stream=stream)
            out["votes_misses"] = votes()
            assert out["votes_misses"] == 0
            got = u(t_votes)[:R * 2 * kv].reshape(R, 2, kv)
            assert int(got.sum()) == M and np.array_equal(got[:, 0].sum(axis=1), mine["inside"])
            out["votes_k"] = kv
        out["count_ms"] = timed(lambda: pkg.window_tags_device(t_map, w, h, R, t_rows, **kw))
        out["full_ms"] = timed(full)
        out["windows_ms"] = timed(lambda: pkg.region_windows_device(t_map, w, h, R, t_off, **kw))
        if lists_ok:
            out["torch_ms"] = timed(alt)
        if votes is not None:
            out["votes_ms"] = timed(votes)
        row.update({prefix + key: v for key, v in out.items()})

    if a.input == "noise":
        t_px, t_lab, t_reg, R, st = region_map(px, w, h, k, stats=True)
        row["frame_min_area_rule"] = D * D // 2
        measure(t_reg, t_px, w, h, R, "frame_", t_area=st["area"], min_area=D * D // 2)
        del t_px, t_lab, t_reg, st
        crop = np.ascontiguousarray(px.reshape(h, w)[:512, :512]).reshape(-1)
        t_px, t_lab, t_reg, R, _ = region_map(crop, 512, 512, k)
        measure(t_reg, t_px, 512, 512, R, "crop_")
    else:
        t_px, t_lab, t_reg, R, _ = region_map(px, w, h, k)
        measure(t_reg, t_px, w, h, R, "")

    if a.input == "batman":
        R, st, Ed, g = ab.region_graph(pkg, t_px, t_lab, t_reg, w, h, R, a.connectivity)
        t_seg = words(w * h)
        S, _, seg = pkg.merge_regions_device(t_reg, R, st["area"], st["first"], st["sums"],
                                             g["edges"] if Ed else None, a.min_area, t_bbox=st["bbox"],
                                             num_edges=Ed, t_out_regions=t_seg, with_remap=False,
                                             stats_capacity=R)
        torch.cuda.synchronize()
        row["segments_min_area_rule"] = D * D // 2
        measure(t_seg, t_px, w, h, S, "segments_", t_area=seg["area"], min_area=D * D // 2)

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
