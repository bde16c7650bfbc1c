#!/usr/bin/env python3
"""The contours of all regions on the device against the ways around the call.

    python tools/contour_ab.py --input smooth|batman|segments|noise|full [--steps 20] [--out FILE.json]
                               [--torch-steps 3] [--no-torch] [--no-host]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/contour_ab.py --input smooth --out profiles/contour/contour_ab_smooth.json && \\
    timeout -k 10 300 python tools/contour_ab.py --input batman --out profiles/contour/contour_ab_batman.json && \\
    timeout -k 10 300 python tools/contour_ab.py --input segments --out profiles/contour/contour_ab_segments.json && \\
    timeout -k 10 400 python tools/contour_ab.py --input noise --out profiles/contour/contour_ab_noise.json && \\
    timeout -k 10 300 python tools/contour_ab.py --input full --out profiles/contour/contour_ab_full.json

Inputs, 8-connectivity throughout:
    smooth    a 3840 x 2160 smooth synthetic frame at K = 256, its connected regions
    batman    tests/golden/png/batman.png at K = 16: its connected regions
    segments  the same after merge_regions_device with min_area 10
    noise     the 3840 x 2160 xorshift frame at K = 256 (millions of specks)
    full      one region over the whole 3840 x 2160 frame: one contour along the frame's edge
Timings, HIP events on the call's stream around the synchronous call, after
--warmup calls, single runs, orientation 1 (what the reference hands on):
    first_ms      the first timed call alone
    contour_ms    the median of --steps calls of dq_hip_region_contours_dev with room for all M points,
                  every output asked for (contour_min_ms, contour_max_ms: the least and the most)
    count_ms      the same of the counting call (no list; offsets, len and visits written)
    torch_ms      the same list ranking as torch ops on the same device: the neighbour planes, the
                  border states numbered by nonzero(), successors by gathers, pointer jumping with one
                  read-back per round, the lists by scatter; the median of --torch-steps runs;
                  torch_agrees: its offsets, points and codes equal the call's
    host_ms       download of the map + the scalar trace of tests/contour_model.py + upload of
                  offsets, points and codes, once; host_agrees: the model's arrays equal the call's
launches and read_backs: what csrc/dq_abi_regions.cpp enqueues for the longest contour the call
reported (13 + one per round, rounds in groups of 4, 4, then 8; one read-back per group + 2); not observed.
Prints one JSON object (and writes it to --out).
"""
import argparse
import os
import statistics
import time

import numpy as np

import ab_common as ab


def schedule(longest):
    """(rounds, groups) of a call whose longest contour has `longest` points."""
    if longest < 2:
        return 0, 0          # (no state at all only when every contour is a pixel; else one group)
    need = max(0, (longest - 2).bit_length()) + 1   # ceil(log2(longest - 1)) and the round that sees the end
    rounds = groups = 0
    while rounds < need:
        rounds += 4 if rounds < 8 else 8
        groups += 1
    return min(rounds, 33), groups


def torch_contours(torch, reg2d, nreg, orientation, next_table):
    """Rules 1-6 as torch ops on the map's device: (offsets, points, codes, rounds)."""
    import torch.nn.functional as F
    dev = reg2d.device
    ids = reg2d.to(torch.int64) & 0xFFFFFFFF
    h, w = ids.shape
    n = h * w
    region = ids < nreg
    dx = torch.tensor([1, 1, 0, -1, -1, -1, 0, 1], device=dev)
    dy = torch.tensor([0, -1, -1, -1, 0, 1, 1, 1], device=dev)
    padded = F.pad(ids, (1, 1, 1, 1), value=-1)
    on = torch.stack([region & (padded[1 + int(dy[d]):1 + int(dy[d]) + h, 1 + int(dx[d]):1 + int(dx[d]) + w] == ids)
                      for d in range(8)], -1)                                  # (h, w, 8)
    bits = (on.to(torch.int64) << torch.arange(8, device=dev)).sum(-1).reshape(-1)
    border = region.reshape(-1) & ((bits & 0x55) != 0x55)
    where = (on.reshape(n, 8) & border[:, None]).reshape(-1).nonzero().squeeze(1)   # state -> 8 p + d
    S = where.numel()
    number = torch.full((8 * n,), -1, dtype=torch.int64, device=dev)
    number[where] = torch.arange(S, device=dev)
    p, d = where >> 3, where & 7
    s = next_table[bits[p], d]
    nxt = number[8 * (p + dy[s] * w + dx[s]) + ((s + 4) & 7)]                 # -1: off the border pixels
    # starts: the first pixel of every id, the first of E, SE, S, SW that is on
    flat = ids.reshape(-1)
    pix = torch.arange(n, device=dev)
    first = torch.full((nreg,), n, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, flat[region.reshape(-1)], pix[region.reshape(-1)], "amin")
    present = first < n
    m0 = torch.where(present, bits[first.clamp(max=n - 1)], 0)
    d0 = torch.where(m0 & 1 != 0, 0, torch.where(m0 & 0x80 != 0, 7, torch.where(m0 & 0x40 != 0, 6, 5)))
    traced = present & (m0 != 0)
    start = torch.where(traced, number[(8 * first.clamp(max=n - 1) + d0)], -1)
    length = torch.where(present, 1, 0)
    rounds = 0
    if S:
        sinks = start[traced]
        after = nxt[sinks]
        dist = torch.ones(S, dtype=torch.int64, device=dev)
        nxt[sinks], dist[sinks] = sinks, 0
        while bool((nxt[after] != sinks).any()):
            live = (nxt >= 0).nonzero().squeeze(1)
            hop = nxt[live]
            dist[live] = dist[live] + dist[hop]
            nxt[live] = nxt[hop]
            rounds += 1
        length[traced] = dist[after] + 1
    offsets = F.pad(length.cumsum(0), (1, 0))
    total = int(offsets[-1])
    points = torch.zeros(total, dtype=torch.int64, device=dev)
    codes = torch.full((total,), 8, dtype=torch.int64, device=dev)
    alone = present & (m0 == 0)
    points[offsets[:-1][alone]] = (first[alone] % w) | (first[alone] // w) << 16
    if S:
        rid = flat[p]
        mine = (nxt == start[rid]) & (start[rid] >= 0)
        rid, pp, ss, dd = rid[mine], p[mine], s[mine], dist[mine]
        ln = length[rid]
        j = torch.where(dd == 0, 0, ln - dd)
        coord = (pp % w) | (pp // w) << 16
        if orientation:
            points[offsets[rid] + ln - 1 - j] = coord
            codes[offsets[rid] + torch.where(j + 1 == ln, ln - 1, ln - 2 - j)] = (ss + 4) & 7
        else:
            points[offsets[rid] + j] = coord
            codes[offsets[rid] + j] = ss
    return offsets, points, codes, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "batman", "segments", "noise", "full"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    import contour_model as cm
    from __graft_entry__ import load_package
    pkg = load_package()
    conn, orientation = 8, 1
    stream = torch.cuda.Stream(device="cuda:0")

    def timed(fn, steps):
        return ab.timed(stream, fn, steps)

    if a.input == "full":
        w, h, R = ab.W4K, ab.H4K, 1
        t_reg = torch.zeros(w * h, dtype=torch.int32, device="cuda:0")
    else:
        px, w, h, k = ab.load_input(pkg, a.input)
        t_px = torch.from_numpy(px.view(np.int32)).to("cuda:0")
        _, t_lab, t_reg, R = ab.region_map(pkg, t_px, w, h, k, conn)
        if a.input == "segments":
            R, _ = ab.segments_in_place(pkg, t_reg, *ab.region_graph(pkg, t_px, t_lab, t_reg, w, h, R, conn))
    torch.cuda.synchronize()

    total, _ = pkg.region_contours_device(t_reg, w, h, R, orientation=orientation, outputs=("len",), stream=stream)

    def contours():
        return pkg.region_contours_device(t_reg, w, h, R, orientation=orientation, point_capacity=total, stream=stream)

    def count():
        return pkg.region_contours_device(t_reg, w, h, R, orientation=orientation, outputs=("offsets", "len", "visits"),
                                          stream=stream)

    for _ in range(a.warmup):
        contours()
    ms = timed(contours, a.steps)
    cms = timed(count, a.steps)
    got_total, out = contours()
    assert got_total == total
    longest = int(out["len"].cpu().numpy().view(np.uint32).max())
    rounds, groups = schedule(longest)
    visits = out["visits"]
    row = {"input": a.input, "width": w, "height": h, "regions": R, "steps": a.steps, "orientation": orientation,
           "first_ms": ms[0], "contour_ms": statistics.median(ms), "contour_min_ms": min(ms), "contour_max_ms": max(ms),
           "count_ms": statistics.median(cms), "points": total, "longest": longest,
           "contour_pixels": int((visits > 0).sum()), "most_visits": int(visits.max()), "rounds": rounds,
           "launches": 13 + rounds, "read_backs": groups + 2, "lib": os.path.basename(pkg.LIB_PATH)}
    offsets = out["offsets"].cpu().numpy().view(np.uint32)
    points = out["points"].cpu().numpy().view(np.uint32)
    codes = out["codes"].cpu().numpy()

    if not a.no_torch:
        got = [None]
        table = torch.tensor(cm.NEXT, device="cuda:0")

        def by_torch():
            with torch.cuda.stream(stream):
                got[0] = torch_contours(torch, t_reg.view(h, w), R, orientation, table)
        by_torch()
        tms = timed(by_torch, a.torch_steps)
        t_off, t_points, t_codes, t_rounds = got[0]
        row["torch_ms"], row["torch_min_ms"], row["torch_max_ms"] = statistics.median(tms), min(tms), max(tms)
        row["torch_steps"], row["torch_rounds"] = a.torch_steps, t_rounds
        row["torch_agrees"] = bool(np.array_equal(t_off.cpu().numpy(), offsets) and
                                   np.array_equal(t_points.cpu().numpy(), points) and
                                   np.array_equal(t_codes.cpu().numpy(), codes))

    if not a.no_host:
        t0 = time.perf_counter()
        reg = t_reg.cpu().numpy().view(np.uint32).reshape(h, w)
        t1 = time.perf_counter()
        model = cm.region_contours(reg, R, orientation)
        t2 = time.perf_counter()
        up = (torch.from_numpy(model["offsets"].view(np.int32)).to("cuda:0"),
              torch.from_numpy(model["points"].view(np.int32)).to("cuda:0"), torch.from_numpy(model["codes"]).to("cuda:0"))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        row["host_ms"], row["host_model_ms"] = (t3 - t0) * 1e3, (t2 - t1) * 1e3
        row["host_how"] = "download + the scalar trace (tests/contour_model.py), one core + upload of offsets, points and codes"
        row["host_agrees"] = bool(np.array_equal(model["offsets"], offsets) and np.array_equal(model["points"], points) and
                                  np.array_equal(model["codes"], codes) and
                                  np.array_equal(model["visits"], visits.cpu().numpy()))
        del up

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
