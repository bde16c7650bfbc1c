#!/usr/bin/env python3
"""Label maps against the colour map, and this build's colour map against
another build's, on one device in one process.

    python tools/labels_ab.py [--base-lib OTHER/libdivquant_hip.so] [--out FILE.json]

The workload: --frames (8) synth frames of --width x --height (3840 x 2160)
as one device buffer, mapped onto the K = --k (256) colortable of frame 0 in
ONE map call per step.  The variants (colour, u8, u16, u32 labels and, with
--base-lib, the other build's colour map) alternate step by step; the time of
a step is the map kernel's own (the library's timing, stat kind 7 "map": HIP
events around the launch), so host work and the cell build are not in it.
Per round: the median of --steps (50) steps per variant; --rounds (5) rounds,
each with its own seeded order of the variants (what a variant runs behind
-- whose output sits in the caches -- moves its time more than repetition
does).  `spread` is (max - min) / min of a variant's round medians.  Prints
one JSON object (and writes it to --out).

The label outputs are checked once against the colour map: ct[labels] must
equal its output, for every width.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAP_KIND = 7


def bind(lib):
    vp, c = ctypes.c_void_p, ctypes
    lib.dq_hip_map_dev.argtypes = [c.c_int, vp, c.c_uint32, vp, vp, c.c_int, vp]
    lib.dq_hip_map_dev.restype = c.c_int
    lib.dq_hip_set_timing.argtypes = [c.c_int, c.c_int]
    lib.dq_hip_set_timing.restype = None
    lib.dq_hip_reset_stats.argtypes = [c.c_int]
    lib.dq_hip_reset_stats.restype = None
    lib.dq_hip_get_stat.argtypes = [c.c_int, c.c_int, c.POINTER(c.c_uint64), c.POINTER(c.c_double),
                                    c.POINTER(c.c_double)]
    lib.dq_hip_get_stat.restype = c.c_int
    return lib


def map_ms(lib, call):
    """The map kernels' time of one call (ms), from the library's own timing."""
    lib.dq_hip_reset_stats(0)
    if call() < 0:
        raise SystemExit("map call refused")
    n, ms, by = ctypes.c_uint64(0), ctypes.c_double(0), ctypes.c_double(0)
    lib.dq_hip_get_stat(0, MAP_KIND, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(by))
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", help="another build's libdivquant_hip.so: its colour map joins the rotation")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    lib = pkg.lib()
    libs = {"this": lib}
    if a.base_lib:
        libs["base"] = bind(ctypes.CDLL(os.path.abspath(a.base_lib)))
    for l in libs.values():
        l.dq_hip_set_timing(0, 1)

    per = a.width * a.height
    n = a.frames * per
    px = np.concatenate([pkg.synth_frame(per, f) for f in range(a.frames)])
    t_in = torch.from_numpy(px.view(np.int32)).to("cuda:0")
    t_tmp = torch.empty(per, dtype=torch.int32, device="cuda:0")
    ct, _ = pkg.quant_device(t_in[:per], t_tmp, a.k)
    ctp = ctypes.c_void_p(ct.ctypes.data)
    t_out = torch.empty(n, dtype=torch.int32, device="cuda:0")
    t_lab = {1: torch.empty(n, dtype=torch.uint8, device="cuda:0"),
             2: torch.empty(n, dtype=torch.int16, device="cuda:0"),
             4: torch.empty(n, dtype=torch.int32, device="cuda:0")}
    p_in, p_out = ctypes.c_void_p(t_in.data_ptr()), ctypes.c_void_p(t_out.data_ptr())

    def colour(l):
        return lambda: l.dq_hip_map_dev(0, p_in, n, p_out, ctp, len(ct), None)

    def labels(w):
        p = ctypes.c_void_p(t_lab[w].data_ptr())
        return lambda: lib.dq_hip_map_labels_dev(0, p_in, n, p, w, ctp, len(ct), None)

    variants = [("colour", lib, colour(lib)), ("u8", lib, labels(1)), ("u16", lib, labels(2)),
                ("u32", lib, labels(4))]
    if a.base_lib:
        variants.insert(1, ("base_colour", libs["base"], colour(libs["base"])))

    # the outputs, once
    checks = {}
    if a.base_lib:
        colour(libs["base"])()
        torch.cuda.synchronize()
        base_out = t_out.clone()
    colour(lib)()
    torch.cuda.synchronize()
    if a.base_lib:
        checks["colour_equals_base"] = bool(torch.equal(t_out, base_out))
        del base_out
    t_ct = torch.from_numpy(ct.view(np.int32)).to("cuda:0")
    for w in (1, 2, 4):
        labels(w)()
        torch.cuda.synchronize()
        idx = t_lab[w].to(torch.int64)
        if w < 4:
            idx &= (1 << (8 * w)) - 1
        checks["u%d_labels_reproduce_colour" % (8 * w)] = bool(torch.equal(t_ct[idx], t_out))
        del idx

    for _, l, call in variants:   # warm-up
        for _ in range(3):
            map_ms(l, call)
    rounds = {name: [] for name, _, _ in variants}
    orders = []
    for r in range(a.rounds):
        times = {name: [] for name, _, _ in variants}
        order = list(variants)
        random.Random(r).shuffle(order)   # (every round its own seeded order)
        orders.append([name for name, _, _ in order])
        for _ in range(a.steps):
            for name, l, call in order:
                times[name].append(map_ms(l, call))
        for name in times:
            rounds[name].append(statistics.median(times[name]))
    res = {"workload": {"frames": a.frames, "width": a.width, "height": a.height, "k_requested": a.k,
                        "k": int(len(ct)), "pixels": n, "steps": a.steps, "rounds": a.rounds},
           "checks": checks, "median_ms_per_round": rounds, "order_per_round": orders,
           "median_ms": {k: statistics.median(v) for k, v in rounds.items()},
           "spread": {k: (max(v) - min(v)) / min(v) for k, v in rounds.items()}}
    col = res["median_ms"]["colour"]
    res["vs_colour"] = {k: v / col for k, v in res["median_ms"].items()}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(checks.values()):
        raise SystemExit("output check failed: %s" % checks)


if __name__ == "__main__":
    main()
