#!/usr/bin/env python3
"""The skeletons of all regions on the device against the ways around the call.

    python tools/skeleton_ab.py --input smooth|batman|segments|noise|full [--steps 20] [--out FILE.json]
                                [--torch-steps 3] [--no-torch] [--no-host] [--host-iters N]

One input per process, so that each GPU step runs under a time limit of its
own and a step that fails ends the chain:

    timeout -k 10 300 python tools/skeleton_ab.py --input smooth --out profiles/skeleton/skeleton_ab_smooth.json && \\
    timeout -k 10 300 python tools/skeleton_ab.py --input batman --out profiles/skeleton/skeleton_ab_batman.json && \\
    timeout -k 10 300 python tools/skeleton_ab.py --input segments --out profiles/skeleton/skeleton_ab_segments.json && \\
    timeout -k 10 300 python tools/skeleton_ab.py --input noise --out profiles/skeleton/skeleton_ab_noise.json && \\
    timeout -k 10 400 python tools/skeleton_ab.py --input full --host-iters 8 --out profiles/skeleton/skeleton_ab_full.json

Inputs, 8-connectivity throughout:
    smooth    a 3840 x 2160 smooth synthetic frame at K = 256, its connected regions
    batman    tests/golden/png/batman.png at K = 16: its connected regions
    segments  the same after merge_regions_device with min_area 10
    noise     the 3840 x 2160 xorshift frame at K = 256 (millions of specks)
    full      one region over the whole 3840 x 2160 frame: the most iterations a frame of the size can take
Timings, HIP events on the call's stream around the synchronous call, after
--warmup calls, single runs:
    first_ms      the first timed call alone
    skeleton_ms   the median of --steps calls of region_skeleton_device, every output asked for
                  (skeleton_min_ms, skeleton_max_ms: the least and the most)
    torch_ms      the same subiterations as torch ops on the same device over the whole frame, the
                  sameness planes made once per call, `when` kept, one read-back per iteration (the
                  reference's stop rule); the median of --torch-steps runs; torch_agrees: its skel and
                  when equal the call's
    host_ms       download of the map + the numpy model of tests/skeleton_model.py + upload of skel
                  and when, once.  With --host-iters N the model stops after N iterations
                  (host_iters says so: the figure is then that part of the whole only);
                  host_agrees: the model's arrays equal the call's (cut at N)
launches and read_backs: what csrc/dq_abi_regions.cpp enqueues for the iterations the call reported
(2 + one per 16 iterations in groups of 2, 4, then 8, + 1; one read-back per group + 1); not observed.
Prints one JSON object (and writes it to --out).
"""
import argparse
import os
import statistics
import time

import numpy as np

import ab_common as ab

ITERS_PER_LAUNCH = 16


def schedule(iterations, limit=65535):
    """(thinning launches, groups) of a call whose last deleting iteration is `iterations`."""
    need = min(iterations + 1, limit)            # the iteration that deletes nothing is run too
    launches = groups = 0
    while launches * ITERS_PER_LAUNCH < need:
        launches += 2 if launches < 2 else 4 if launches < 6 else 8
        groups += 1
    return min(launches, -(-limit // ITERS_PER_LAUNCH)), groups


def torch_skeleton(torch, reg2d, nreg):
    """Rules 1-4 as torch ops on the map's device: (skel bool, when int16, iterations)."""
    import torch.nn.functional as F
    ids = reg2d.to(torch.int64) & 0xFFFFFFFF
    region = ids < nreg
    h, w = ids.shape
    offs = ((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1))
    padded = F.pad(ids, (1, 1, 1, 1), value=-1)
    same = [region & (padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] == ids) for dy, dx in offs]

    def sub(alive, second):
        p = F.pad(alive, (1, 1, 1, 1))
        n = [p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] & same[k] for k, (dy, dx) in enumerate(offs)]
        i = lambda b: b.to(torch.int8)  # noqa: E731
        c = i(~n[1] & (n[2] | n[3])) + i(~n[3] & (n[4] | n[5])) + i(~n[5] & (n[6] | n[7])) + i(~n[7] & (n[0] | n[1]))
        n1 = i(n[0] | n[1]) + i(n[2] | n[3]) + i(n[4] | n[5]) + i(n[6] | n[7])
        n2 = i(n[1] | n[2]) + i(n[3] | n[4]) + i(n[5] | n[6]) + i(n[7] | n[0])
        m = torch.minimum(n1, n2)
        side = (n[5] | n[6] | ~n[0]) & n[7] if second else (n[1] | n[2] | ~n[4]) & n[3]
        return alive & ~((c == 1) & ((m == 2) | (m == 3)) & ~side)

    alive = region.clone()
    when = torch.zeros((h, w), dtype=torch.int16, device=ids.device)
    it = 0
    while it < 65535:
        after = sub(sub(alive, False), True)
        gone = alive & ~after
        alive = after
        if not bool(gone.any()):
            break
        it += 1
        when[gone] = it if it < 32768 else it - 65536
    return alive, when, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True, choices=["smooth", "batman", "segments", "noise", "full"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-iters", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    import skeleton_model as sm
    from __graft_entry__ import load_package
    pkg = load_package()
    conn = 8
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

    def skeleton():
        return pkg.region_skeleton_device(t_reg, w, h, R, stream=stream)

    for _ in range(a.warmup):
        skeleton()
    ms = timed(skeleton, a.steps)
    kept, out = skeleton()
    launches, groups = schedule(out["iterations"])
    row = {"input": a.input, "width": w, "height": h, "regions": R, "steps": a.steps, "first_ms": ms[0],
           "skeleton_ms": statistics.median(ms), "skeleton_min_ms": min(ms), "skeleton_max_ms": max(ms),
           "iterations": out["iterations"], "converged": out["converged"], "kept": kept,
           "highest_thick": int(out["thick"].max()), "thin_launches": launches, "launches": launches + 3,
           "read_backs": groups + 1, "iters_per_launch": ITERS_PER_LAUNCH, "lib": os.path.basename(pkg.LIB_PATH)}
    skel = out["skel"].cpu().numpy()
    when = out["when"].cpu().numpy().view(np.uint16)

    if not a.no_torch:
        got = [None]

        def by_torch():
            with torch.cuda.stream(stream):
                got[0] = torch_skeleton(torch, t_reg.view(h, w), R)
        by_torch()
        tms = timed(by_torch, a.torch_steps)
        t_skel, t_when, t_its = got[0]
        row["torch_ms"], row["torch_min_ms"], row["torch_max_ms"] = statistics.median(tms), min(tms), max(tms)
        row["torch_steps"], row["torch_iterations"] = a.torch_steps, t_its
        row["torch_agrees"] = bool(np.array_equal(t_skel.cpu().numpy().astype(np.uint8), skel) and
                                   np.array_equal(t_when.cpu().numpy().view(np.uint16), when))

    if not a.no_host:
        t0 = time.perf_counter()
        reg = t_reg.cpu().numpy().view(np.uint32).reshape(h, w)
        t1 = time.perf_counter()
        model = sm.region_skeleton(reg, R, a.host_iters)
        t2 = time.perf_counter()
        up = (torch.from_numpy(model["skel"]).to("cuda:0"), torch.from_numpy(model["when"].view(np.int16)).to("cuda:0"))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        row["host_ms"], row["host_model_ms"], row["host_iters"] = (t3 - t0) * 1e3, (t2 - t1) * 1e3, a.host_iters
        row["host_how"] = "download + the numpy model (tests/skeleton_model.py), one core + upload of skel and when"
        if a.host_iters:
            cut = np.where(when <= a.host_iters, when, 0)
            row["host_agrees"] = bool(np.array_equal(model["when"], cut) and
                                      np.array_equal(model["skel"] == 1, (reg < R) & (cut == 0)))
        else:
            row["host_agrees"] = bool(np.array_equal(model["skel"], skel) and np.array_equal(model["when"], when))
        del up

    ab.emit(row, a.out)


if __name__ == "__main__":
    main()
