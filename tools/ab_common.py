"""What the region-map A/B tools (regions_ab.py .. skeleton_ab.py) share: the
import paths, the three inputs, the chain frame -> u8 labels -> region map
(-> stats and edge list -> segments), the HIP-event timing loop and the JSON
tail.  A tool imports this module first: importing it puts the repository, tests/
and tools/ on sys.path."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

W4K, H4K = 3840, 2160


def smooth_frame(w, h):
    """Slow gradients in all three channels with a few broad waves."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 127.5 + 127.5 * np.sin(xs / w * 3.0 + ys / h * 1.5)
    g = 255.0 * ys / (h - 1)
    b = 127.5 + 127.5 * np.cos((xs / w) ** 2 * 4.0 - ys / h * 2.0)
    u = lambda a: np.clip(a, 0, 255).astype(np.uint32)  # noqa: E731
    return ((u(r) << 16) | (u(g) << 8) | u(b)).reshape(-1)


def load_input(pkg, name):
    """(px, w, h, k) of "smooth", "noise" or the batman frame (any other name: "batman", "segments")."""
    if name == "smooth":
        return smooth_frame(W4K, H4K), W4K, H4K, 256
    if name == "noise":
        return pkg.synth_frame(W4K * H4K), W4K, H4K, 256
    import dq_fixtures as fx
    px, w, h = fx.load_png_u32(os.path.join(ROOT, "tests", "golden", "png", "batman.png"))
    return px, w, h, 16


def region_map(pkg, t_px, w, h, k, connectivity):
    """The frame quantised to u8 labels and labelled into connected regions (the count-only call)
    -> (cts, t_lab, t_reg, R)."""
    import torch
    n = w * h
    t_lab = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    cts, _ = pkg.quant_labels_batch_device([t_px], [t_lab], k)
    t_reg = torch.empty(n, dtype=torch.int32, device="cuda:0")
    R, _ = pkg.label_regions_device(t_lab, w, h, t_reg, connectivity=connectivity)
    return cts, t_lab, t_reg, R


def region_graph(pkg, t_px, t_lab, t_reg, w, h, R, connectivity):
    """The stats of all R regions (colour sums included) and the edge list of their map -> (R, st, E, g)."""
    R, st = pkg.label_regions_device(t_lab, w, h, t_reg, connectivity=connectivity, stats_capacity=R, t_pixels=t_px)
    E, _ = pkg.region_adjacency_device(t_reg, w, h, connectivity=connectivity)
    E, g = pkg.region_adjacency_device(t_reg, w, h, connectivity=connectivity, edge_capacity=E)
    return R, st, E, g


def segments_in_place(pkg, t_reg, R, st, E, g, min_area=10):
    """The "segments" input: the region map merged in place -> (R', the segments' stats)."""
    R, _, out = pkg.merge_regions_device(t_reg, R, st["area"], st["first"], st["sums"], g["edges"], min_area,
                                         num_edges=E, stats_capacity=R)
    return R, out


def timed(stream, fn, steps, warmup=0):
    """The ms of `steps` calls of fn after `warmup` calls, each between two HIP events on the stream."""
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def emit(row, out):
    """One JSON object with sorted keys to stdout, and to the file `out` if given."""
    line = json.dumps(row, sort_keys=True)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
