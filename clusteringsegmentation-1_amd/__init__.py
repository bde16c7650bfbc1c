"""clusteringsegmentation-1_amd -- MI355X-native DivQuant hot path.

Python mirror of the reference's DivQuant interface (DivQuant/quant_util.h,
DivQuant/DivQuantHeader.h) over the C ABI of ``libdivquant_hip.so``
(include/dq_hip.h).  The compute runs in hand-written gfx950 kernels; there is
no CPU fallback: without the built library or without a HIP device every
compute call raises.

The directory name is not a Python identifier, so load it with
``load_package()`` (tests/, bench.py and __graft_entry__.py do).

Reference-named entry points (same argument meaning, host numpy arrays):
    quant_recurse(pixels, num_clusters, all_pixels_unique=1) -> (out, colortable)
    map_colors_mps(pixels, colortable)                       -> out
    quant_varpart_fast(pixels, num_clusters, max_iters=10)   -> colortable
Device-resident entry points (torch tensors / raw device pointers on HBM):
    quant_device, quant_batch_device, cluster_device, map_device
Cluster labels (each pixel's index into the colortable, u8 / u16 / u32):
    map_labels_device, quant_labels_batch_device, quant_labels
Connected regions of a label map (equal labels joined by 4- / 8-neighbours,
numbered in raster order) with area, bounding box, first pixel, colour sums:
    label_regions_device, label_regions
Adjacency graph of a region map (the pairs of ids that touch, numbered in
raster order of their first contact) with border, first contact, colour step:
    region_adjacency_device, region_adjacency
Region merge over that graph (small regions join their most alike neighbour in
rounds, exact integers) and the whole labels -> segments pipeline on the device:
    merge_regions_device, segment_labels
Pixel lists of a region map (stable counting sort by id: offsets, indexes,
Coords, colours), their inverse and region map -> per-region quant -> frame:
    region_pixels_device, region_pixels, scatter_coords_device,
    quant_region_map_device, quant_region_map
Capture windows of a region map (per region the pixels of the d x d blocks within
L1 distance e of its own blocks: one pixel in many lists) and a quant per window:
    region_windows_device, region_windows,
    quant_region_windows_device, quant_region_windows
L1 distance of every pixel to the nearest pixel of another id, every region's
centre (the reference's findRegionCenter rule) and core (the component of the
region that holds the centre):
    region_distance_device, region_distance, region_cores_device, region_cores
Skeletons of all regions of a region map (Guo-Hall thinning, the reference's
skelReduce on every region's mask at once) with the iteration that deleted
each pixel, the skeleton's area and the region's thickness:
    region_skeleton_device, region_skeleton
Contours of all regions of a region map (border following, the reference's
findContourOutline on every region's mask at once): per region the ordered
border pixels with their chain codes, and per pixel how often it is visited:
    region_contours_device, region_contours
Row-tile sharding (one frame over shards / GPUs, RCCL allreduce per pass):
    quant_rows_device, comm_init_torch (comm_unique_id, comm_init, comm_destroy);
    loopback_rows_device (tests: N ranks in one process, loopback collective)
Full-frame block histograms (genHistogramsForBlocks):
    get_subdivided_colors, gen_histograms_for_blocks, block_hist_device
BGR24 (OpenCV CV_8UC3) ingestion / output on the GPU (Vec3BToUID / PixelToVec3b):
    pack_bgr24_device, unpack_bgr24_device, gather_bgr24_device
"""
import ctypes
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# DQ_HIP_LIB: another build of the same library (kernel variants in experiments)
LIB_PATH = os.environ.get("DQ_HIP_LIB") or os.path.join(PKG_DIR, "libdivquant_hip.so")

STAT_KINDS = ["pass_init", "pass_split", "pass_kmeans", "pass_klast",
              "epilogue", "partition", "map_cells", "map", "plan", "kloop"]

_lib = None


class DivQuantError(RuntimeError):
    pass


def lib():
    """The ctypes handle of libdivquant_hip.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP/HSA runtime per process: when PyTorch is present, import it first
    # so the library binds (by soname) to the libamdhip64 torch already mapped
    # instead of mapping /opt/rocm's copy beside it -- two runtimes in one
    # process cannot both open the GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise DivQuantError("libdivquant_hip.so is not built (run __graft_entry__.build() "
                            "or make -C clusteringsegmentation-1_amd)")
    L = ctypes.CDLL(LIB_PATH)
    u32p, vp = ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p
    c = ctypes
    sigs = {
        "dq_hip_abi_version": ([], c.c_int),
        "dq_hip_device_count": ([], c.c_int),
        "dq_hip_quant": ([vp, c.c_uint32, vp, u32p, vp, c.c_int, c.c_int], c.c_int),
        "dq_hip_map": ([vp, c.c_uint32, vp, vp, c.c_int], c.c_int),
        "dq_hip_quant_dev": ([c.c_int, vp, c.c_uint32, vp, u32p, vp, c.c_int, vp], c.c_int),
        "dq_hip_quant_batch_dev": ([c.c_int, c.c_int, vp, vp, vp, c.c_uint32, vp, vp, c.c_int, vp],
                                   c.c_int),
        "dq_hip_quant_rows_dev": ([c.c_int, c.c_int, vp, vp, vp, vp, c.c_int, vp, c.c_uint32, vp, vp,
                                   c.c_int, vp], c.c_int),
        "dq_hip_comm_unique_id": ([vp], c.c_int),
        "dq_hip_comm_init": ([c.c_int, c.c_int, c.c_int, vp], c.c_int),
        "dq_hip_comm_destroy": ([c.c_int], c.c_int),
        "dq_hip_comm_size": ([c.c_int], c.c_int),
        "dq_hip_cluster_dev": ([c.c_int, vp, c.c_uint32, u32p, vp, c.c_int, vp], c.c_int),
        "dq_hip_map_dev": ([c.c_int, vp, c.c_uint32, vp, vp, c.c_int, vp], c.c_int),
        "dq_hip_map_labels_dev": ([c.c_int, vp, c.c_uint32, vp, c.c_int, vp, c.c_int, vp], c.c_int),
        "dq_hip_quant_labels_batch_dev": ([c.c_int, c.c_int, vp, vp, vp, c.c_int, c.c_uint32, vp, vp, c.c_int,
                                           c.c_int, vp], c.c_int),
        "dq_hip_quant_labels": ([vp, c.c_uint32, vp, c.c_int, u32p, vp, c.c_int], c.c_int),
        "dq_hip_label_regions_dev": ([c.c_int, vp, c.c_int, c.c_uint32, c.c_uint32, c.c_int, vp, c.c_uint32, vp, vp,
                                      vp, vp, vp, vp, vp], c.c_int64),
        "dq_hip_label_regions": ([vp, c.c_int, c.c_uint32, c.c_uint32, c.c_int, vp, c.c_uint32, vp, vp, vp, vp, vp,
                                  vp], c.c_int64),
        "dq_hip_region_adjacency_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, vp, vp, vp, vp, vp,
                                         c.c_uint32, vp, vp], c.c_int64),
        "dq_hip_region_adjacency": ([vp, c.c_uint32, c.c_uint32, c.c_int, c.c_uint32, vp, vp, vp, vp, vp, c.c_uint32,
                                     vp], c.c_int64),
        "dq_hip_merge_regions_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, vp, vp, vp, vp, c.c_uint32, vp, c.c_uint32,
                                      c.c_uint32, c.c_uint32, vp, vp, c.c_uint32, vp, vp, vp, vp, u32p, vp],
                                     c.c_int64),
        "dq_hip_segment_labels": ([vp, c.c_int, c.c_uint32, c.c_uint32, c.c_int, vp, c.c_uint32, c.c_uint32,
                                   c.c_uint32, vp, c.c_uint32, vp, vp, vp, vp, u32p], c.c_int64),
        "dq_hip_region_pixels_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp, vp],
                                     c.c_int64),
        "dq_hip_region_pixels": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp], c.c_int64),
        "dq_hip_scatter_coords_dev": ([c.c_int, vp, vp, c.c_uint32, c.c_uint32, vp, vp], c.c_int),
        "dq_hip_quant_region_map_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, c.c_uint32, vp, vp, vp,
                                         c.c_int, vp], c.c_int64),
        "dq_hip_quant_region_map": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, c.c_uint32, vp, vp, vp, c.c_int],
                                    c.c_int64),
        "dq_hip_region_windows_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp,
                                       c.c_uint32, vp, c.c_uint32, vp, vp, vp, vp, vp], c.c_int64),
        "dq_hip_region_windows": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, c.c_uint32,
                                   vp, c.c_uint32, vp, vp, vp, vp], c.c_int64),
        "dq_hip_quant_region_windows_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32,
                                             vp, vp, c.c_uint32, vp, c.c_uint32, vp, vp, vp, vp, c.c_uint32, vp, vp,
                                             vp, c.c_int, vp], c.c_int64),
        "dq_hip_quant_region_windows": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp,
                                         c.c_uint32, vp, c.c_uint32, vp, vp, vp, vp, c.c_uint32, vp, vp, vp, c.c_int],
                                        c.c_int64),
        "dq_hip_window_tags_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp,
                                    c.c_uint32, vp, c.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp], c.c_int64),
        "dq_hip_window_tags": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, c.c_uint32, vp,
                                c.c_uint32, vp, vp, vp, vp, vp, vp, vp], c.c_int64),
        "dq_hip_window_votes_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, vp, vp, c.c_uint32, vp, vp, vp, c.c_uint32,
                                     vp, vp, vp], c.c_int64),
        "dq_hip_region_containment_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, c.c_uint32, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp, vp, u32p, u32p, vp], c.c_int64),
        "dq_hip_region_containment": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, c.c_uint32, vp, vp, vp, vp, vp, vp,
                                       vp, vp, vp, vp, u32p, u32p], c.c_int64),
        "dq_hip_regions_by_size_dev": ([c.c_int, c.c_uint32, vp, vp, vp, vp], c.c_int),
        "dq_hip_region_distance_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, vp, vp, vp, vp, vp,
                                        vp, vp], c.c_int),
        "dq_hip_region_distance": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, vp, vp, vp, vp, vp, vp], c.c_int),
        "dq_hip_region_cores_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.c_int, vp, vp, vp,
                                     vp, vp, vp], c.c_int64),
        "dq_hip_region_cores": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.c_int, vp, vp, vp, vp, vp],
                                c.c_int64),
        "dq_hip_region_skeleton_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp,
                                        u32p, u32p, vp], c.c_int64),
        "dq_hip_region_skeleton": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp, u32p, u32p],
                                   c.c_int64),
        "dq_hip_region_contours_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.c_uint64, vp, vp, vp,
                                        vp, vp, vp], c.c_int64),
        "dq_hip_region_contours": ([vp, c.c_uint32, c.c_uint32, c.c_uint32, c.c_int, c.c_uint64, vp, vp, vp, vp, vp],
                                   c.c_int64),
        "dq_hip_quant_weighted_dev": ([c.c_int, vp, c.c_uint32, vp, u32p, vp, c.c_int, vp], c.c_int),
        "dq_hip_quant_weighted_regions_dev": ([c.c_int, c.c_int, vp, vp, vp, vp, vp, c.c_uint32, vp, c.c_int, vp],
                                              c.c_int),
        "dq_hip_last_centroids": ([c.c_int, vp, vp, c.c_int], c.c_int),
        "dq_hip_last_trace": ([c.c_int, vp, c.c_int], c.c_int),
        "dq_hip_last_rounds": ([c.c_int], c.c_int),
        "dq_hip_last_points_swept": ([c.c_int], c.c_uint64),
        "dq_hip_last_points_full": ([c.c_int], c.c_uint64),
        "dq_hip_last_seq_tiles": ([c.c_int], c.c_uint64),
        "dq_hip_last_cursor_fixes": ([c.c_int], c.c_uint64),
        "dq_hip_set_fixed_point": ([c.c_int, c.c_int], None),
        "dq_hip_set_planned_rounds": ([c.c_int, c.c_int], None),
        "dq_hip_last_planned_rounds": ([c.c_int], c.c_int),
        "dq_hip_set_loop_max": ([c.c_int, c.c_uint32], None),
        "dq_hip_last_loop_rounds": ([c.c_int], c.c_int),
        "dq_hip_set_persist": ([c.c_int, c.c_int], None),
        "dq_hip_set_wsmall": ([c.c_int, c.c_int], None),
        "dq_hip_set_lds_map": ([c.c_int, c.c_int], None),
        "dq_hip_last_wsmall_profile": ([c.c_int, c.c_void_p, c.c_int], c.c_int),
        "dq_hip_last_persist_rounds": ([c.c_int], c.c_int),
        "dq_hip_set_timing": ([c.c_int, c.c_int], None),
        "dq_hip_reset_stats": ([c.c_int], None),
        "dq_hip_get_stat": ([c.c_int, c.c_int, c.POINTER(c.c_uint64), c.POINTER(c.c_double),
                             c.POINTER(c.c_double)], c.c_int),
        "dq_hip_stat_name": ([c.c_int], c.c_char_p),
        "dq_hip_set_lanes": ([c.c_int], None),
        "dq_hip_get_lanes": ([], c.c_int),
        "dq_hip_block_hist": ([vp, c.c_uint32, c.c_uint32, vp, c.c_int, c.c_uint32, c.c_uint32,
                               c.c_uint32, vp, vp, vp, vp, vp], c.c_int),
        "dq_hip_block_hist_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, vp, c.c_int, c.c_uint32,
                                   c.c_uint32, c.c_uint32, vp, vp, vp, vp, vp, vp], c.c_int),
        "dq_subdivided_colors": ([vp], None),
        "dq_synth_xorshift": ([vp, c.c_uint64, c.c_uint64], None),
        "dq_fnv1a64": ([vp, c.c_uint64], c.c_uint64),
        "dq_hip_pack_bgr24_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp], c.c_int),
        "dq_hip_unpack_bgr24_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp],
                                    c.c_int),
        "dq_hip_gather_bgr24_dev": ([c.c_int, vp, c.c_uint32, vp, c.c_uint32, vp, vp], c.c_int),
        "dq_hip_varpart_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, u32p, vp, c.c_int, c.c_int,
                                c.c_int, c.c_int, vp], c.c_int),
        "dq_hip_cut_bits_dev": ([c.c_int, vp, c.c_uint32, vp, c.c_int, c.c_int, c.c_int, vp], c.c_int),
        "dq_hip_quant_bgr24_batch_dev": ([c.c_int, c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp,
                                          c.c_uint32, vp, vp, c.c_int, c.c_int, vp], c.c_int),
        "dq_hip_quant_bgr24_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, u32p, vp, c.c_int,
                                    c.c_int, vp], c.c_int),
        "dq_hip_map_bgr24_dev": ([c.c_int, vp, c.c_uint32, c.c_uint32, c.c_uint32, vp, vp, c.c_int, vp],
                                 c.c_int),
        "quant_recurse": ([c.c_uint32, vp, vp, u32p, vp, c.c_int], None),
        "dq_hip_build_id": ([], c.c_uint64),
        "dq_hip_set_debug": ([c.c_int, c.c_int], None),
        "dq_hip_loopback_rows_dev": ([c.c_int, c.c_int, c.c_int, vp, c.c_uint32, c.c_uint32, vp, c.c_uint32,
                                      vp, vp, c.c_int, vp, c.c_int, vp], c.c_int),
    }
    ab = "DQ_HIP_LIB" in os.environ   # (A/B runs against an older build: its newer entry points absent)
    for name, (args, res) in sigs.items():
        if ab and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _require_gpu():
    if lib().dq_hip_device_count() < 1:
        raise DivQuantError("no HIP device visible: the DivQuant hot path runs only on the GPU")


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------
# Reference-named host entry points.
def quant_recurse(pixels, num_clusters, all_pixels_unique=1):
    """quant_recurse (DivQuant/quant_util.cpp:20-158): returns (out, colortable)."""
    _require_gpu()
    px = _u32(pixels).reshape(-1)
    if px.size == 0 or num_clusters <= 0:
        raise DivQuantError("numPixels and numClusters must be > 0")
    out = np.zeros(px.size, np.uint32)
    ct = np.zeros(num_clusters, np.uint32)
    k = ctypes.c_uint32(num_clusters)
    lib().quant_recurse(px.size, _ptr(px), _ptr(out), ctypes.byref(k), _ptr(ct), int(all_pixels_unique))
    return out, ct[:k.value].copy()


def quant_host(pixels, num_clusters, all_pixels_unique=1, ngpus=1):
    """dq_hip_quant (quant_recurse without the timer lines) on host pixels;
    ngpus > 1 shards the frame over this process's devices (RCCL in-process)."""
    _require_gpu()
    px = _u32(pixels).reshape(-1)
    out = np.zeros(px.size, np.uint32)
    ct = np.zeros(num_clusters, np.uint32)
    k = ctypes.c_uint32(num_clusters)
    if lib().dq_hip_quant(_ptr(px), px.size, _ptr(out), ctypes.byref(k), _ptr(ct), int(all_pixels_unique),
                          int(ngpus)) < 0:
        raise DivQuantError("dq_hip_quant: bad arguments")
    return out, ct[:k.value].copy()


def map_colors_mps(pixels, colortable):
    """map_colors_mps (DivQuant/DivQuantMapColors.cpp:243-539)."""
    _require_gpu()
    px = _u32(pixels).reshape(-1)
    ct = _u32(colortable).reshape(-1)
    if ct.size == 0:
        raise DivQuantError("colormapSize must be > 0")
    out = np.zeros(px.size, np.uint32)
    if lib().dq_hip_map(_ptr(px), px.size, _ptr(out), _ptr(ct), ct.size) < 0:
        raise DivQuantError("dq_hip_map failed")
    return out


def quant_varpart_fast(pixels, num_clusters, max_iters=10, device=0, all_pixels_unique=1, num_bits=8,
                       dec_factor=1, num_rows=1, num_cols=None):
    """quant_varpart_fast (DivQuantCluster.cpp:1099-1179): the non-empty
    cluster colours in cluster-index order (not deduplicated); uniform-weight
    path, or the weighted one for all_pixels_unique=0; num_bits < 8 /
    dec_factor > 1 take cut_bits and the decimated colour table over a
    num_rows x num_cols frame (:1139-1146)."""
    import torch
    _require_gpu()
    px = torch.from_numpy(_u32(pixels).reshape(-1).view(np.int32)).to(f"cuda:{device}")
    if num_bits != 8 or dec_factor != 1 or num_rows != 1 or (num_cols not in (None, px.numel())):
        ct = np.zeros(num_clusters, np.uint32)
        k = ctypes.c_uint32(num_clusters)
        rc = lib().dq_hip_varpart_dev(device, _dptr(px), px.numel(), num_rows,
                                      px.numel() if num_cols is None else num_cols, ctypes.byref(k), _ptr(ct),
                                      num_bits, dec_factor, max_iters, all_pixels_unique, None)
        if rc < 0:
            raise DivQuantError("dq_hip_varpart_dev: bad arguments (%d)" % rc)
        return ct[:k.value].copy()
    if all_pixels_unique:
        ct, _ = cluster_device(px, num_clusters, max_iters=max_iters, device=device)
        return ct
    ct = np.zeros(num_clusters, np.uint32)
    k = ctypes.c_uint32(num_clusters)
    if lib().dq_hip_quant_weighted_dev(device, _dptr(px), px.numel(), None, ctypes.byref(k), _ptr(ct),
                                       max_iters, None) < 0:
        raise DivQuantError("dq_hip_quant_weighted_dev: bad arguments")
    return ct[:k.value].copy()


# ---------------------------------------------------------------------------
# Device-resident entry points.  `t_in` / `t_out` are torch tensors (int32 or
# uint32 storage, contiguous, on cuda:device) or raw integer device pointers.
def _dptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _nelem(t, n):
    return n if n is not None else t.numel()


def _stream_ptr(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


def quant_device(t_in, t_out, num_clusters, max_iters=10, device=0, n=None, stream=None,
                 all_pixels_unique=1):
    """Cluster + dedup + map of device-resident pixels; returns (colortable, empty).
    all_pixels_unique=0: the weighted path (calc_color_table + ordered folds)."""
    n = _nelem(t_in, n)
    ct = np.zeros(num_clusters, np.uint32)
    k = ctypes.c_uint32(num_clusters)
    fn = lib().dq_hip_quant_dev if all_pixels_unique else lib().dq_hip_quant_weighted_dev
    r = fn(device, _dptr(t_in), n, _dptr(t_out), ctypes.byref(k), _ptr(ct), max_iters, _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_quant_dev: bad arguments")
    return ct[:k.value].copy(), r


class WeightedRegions:
    """A set of device-resident regions for dq_hip_quant_weighted_regions_dev
    with its argument arrays built once (for repeated calls on the same
    buffers: the per-call marshalling of thousands of pointers is Python's
    cost, not the library's)."""

    def __init__(self, t_ins, t_outs, num_clusters):
        nr = len(t_ins)
        self.nr = nr
        self.ks = np.array(num_clusters if hasattr(num_clusters, "__len__") else [num_clusters] * nr, np.uint32)
        self.stride = int(self.ks.max()) if nr else 1
        self.ins = (ctypes.c_void_p * max(nr, 1))(*[_dptr(t).value for t in t_ins])
        self.outs = (ctypes.c_void_p * max(nr, 1))(*[_dptr(t).value for t in t_outs]) if t_outs is not None else None
        self.ns = np.array([t.numel() for t in t_ins], np.uint32)
        self.ct = np.zeros((max(nr, 1), self.stride), np.uint32)
        self.kout = np.zeros(max(nr, 1), np.uint32)
        self._refs = (t_ins, t_outs)   # (keep the buffers alive)

    def run(self, max_iters=10, device=0, stream=None):
        """One call over every region; returns the total of empty clusters
        (colortables: self.colortable(i))."""
        r = lib().dq_hip_quant_weighted_regions_dev(
            device, self.nr, ctypes.cast(self.ins, ctypes.c_void_p), _ptr(self.ns),
            ctypes.cast(self.outs, ctypes.c_void_p) if self.outs is not None else None,
            _ptr(self.ks), _ptr(self.ct), self.stride, _ptr(self.kout), max_iters, _stream_ptr(stream))
        if r < 0:
            raise DivQuantError("dq_hip_quant_weighted_regions_dev: bad arguments")
        return r

    def colortable(self, i):
        return self.ct[i, :self.kout[i]].copy()


def quant_weighted_regions_device(t_ins, t_outs, num_clusters, max_iters=10, device=0, stream=None):
    """The app's per-superpixel-region calls quant_recurse(N_region, .., K,
    allPixelsUnique=0) (ClusteringSegmentation.cpp:1779-1803) for many
    device-resident regions in one call (one launch for every region of at
    most 131071 pixels / 6144 colours / K <= 64).  num_clusters: one K or a
    list.  t_outs may be None (cluster + dedup only).  Returns ([colortable
    per region], total_empty)."""
    w = WeightedRegions(t_ins, t_outs, num_clusters)
    r = w.run(max_iters, device, stream)
    return [w.colortable(i) for i in range(w.nr)], r


def quant_batch_device(t_ins, t_outs, num_clusters, max_iters=10, device=0, stream=None):
    """quant_recurse over a batch of device-resident frames in one call (every
    pass of every split round is one launch over all frames).
    Returns ([colortable per frame], total_empty)."""
    nf = len(t_ins)
    ins = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_ins])
    outs = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_outs])
    ns = np.array([t.numel() for t in t_ins], np.uint32)
    ct = np.zeros((nf, num_clusters), np.uint32)
    kout = np.zeros(nf, np.uint32)
    r = lib().dq_hip_quant_batch_dev(device, nf, ctypes.cast(ins, ctypes.c_void_p),
                                     _ptr(ns), ctypes.cast(outs, ctypes.c_void_p), num_clusters,
                                     _ptr(ct), _ptr(kout), max_iters, _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_quant_batch_dev: bad arguments")
    return [ct[i, :kout[i]].copy() for i in range(nf)], r


def quant_bgr24_batch_device(t_bgrs, width, height, t_outs, num_clusters, stride=None, max_iters=10,
                             device=0, stream=None, all_pixels_unique=1):
    """quant_recurse of device BGR24 frames (OpenCV CV_8UC3 rows), read
    directly by the root's passes, partition and map; outputs
    packed colours.  Returns ([colortable per frame], total_empty)."""
    nf = len(t_bgrs)
    stride = 3 * width if stride is None else stride
    ins = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_bgrs])
    outs = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_outs])
    ct = np.zeros((nf, num_clusters), np.uint32)
    kout = np.zeros(nf, np.uint32)
    r = lib().dq_hip_quant_bgr24_batch_dev(device, nf, ctypes.cast(ins, ctypes.c_void_p), width, height, stride,
                                           ctypes.cast(outs, ctypes.c_void_p), num_clusters, _ptr(ct), _ptr(kout),
                                           all_pixels_unique, max_iters, _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_quant_bgr24_batch_dev: bad arguments")
    return [ct[i, :kout[i]].copy() for i in range(nf)], r


def quant_bgr24_device(t_bgr, width, height, t_out, num_clusters, stride=None, max_iters=10, device=0,
                       stream=None, all_pixels_unique=1):
    """quant_recurse of one device BGR24 frame; returns (colortable, empty)."""
    cts, r = quant_bgr24_batch_device([t_bgr], width, height, [t_out], num_clusters, stride, max_iters, device,
                                      stream, all_pixels_unique)
    return cts[0], r


def map_bgr24_device(t_bgr, width, height, t_out, colortable, stride=None, device=0, stream=None):
    """map_colors_mps of a device BGR24 frame into packed colours."""
    stride = 3 * width if stride is None else stride
    ct = _u32(colortable)
    if lib().dq_hip_map_bgr24_dev(device, _dptr(t_bgr), width, height, stride, _dptr(t_out), _ptr(ct), len(ct),
                                  _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_map_bgr24_dev: bad arguments")


def quant_rows_device(t_ins, t_outs, num_clusters, widths=None, n_globals=None, nshard=1,
                      max_iters=10, device=0, stream=None):
    """Row-tile sharded quant_recurse: t_ins[i] holds THIS
    process's rows of frame i.  nshard > 1 splits them into row ranges
    processed as separate shards on this GPU; n_globals[i] > numel means the
    other rows live in other processes, joined by the RCCL communicator of
    comm_init (every pass's integer node totals are allreduced).  Returns
    ([colortable per frame], total_empty) -- identical on every process."""
    nf = len(t_ins)
    ins = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_ins])
    outs = None
    if t_outs is not None:
        outs = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_outs])
    ns = np.array([t.numel() for t in t_ins], np.uint32)
    ws = np.array(widths if widths is not None else [0] * nf, np.uint32)
    ng = np.array(n_globals if n_globals is not None else [0] * nf, np.uint64)
    ct = np.zeros((nf, num_clusters), np.uint32)
    kout = np.zeros(nf, np.uint32)
    r = lib().dq_hip_quant_rows_dev(device, nf, ctypes.cast(ins, ctypes.c_void_p), _ptr(ns),
                                    _ptr(ws), _ptr(ng), nshard,
                                    ctypes.cast(outs, ctypes.c_void_p) if outs is not None else None,
                                    num_clusters, _ptr(ct), _ptr(kout), max_iters,
                                    _stream_ptr(stream))
    if r == -2:
        raise DivQuantError("dq_hip_quant_rows_dev: n_global > n needs comm_init first")
    if r < 0:
        raise DivQuantError("dq_hip_quant_rows_dev: bad arguments")
    return [ct[i, :kout[i]].copy() for i in range(nf)], r


def loopback_rows_device(t_ins, t_outs, width, height, num_clusters, nranks, max_iters=10, device=0,
                         log_cap=8192):
    """Test-only: row-tile sharding of `nranks` processes, run as nranks
    engines of this process on `device` (own stream and host thread each)
    joined by the in-process loopback collective instead of RCCL -- the
    TOT_ALLREDUCE path with every rank's local counts != the global totals.
    t_ins / t_outs: whole width x height frames; rank r maps its rows
    [r*H/N, (r+1)*H/N) into t_outs.  Returns (cts, logs, empty): cts[r][i] =
    rank r's colortable of frame i, logs[r] = the element counts of the
    collectives rank r enqueued, in order."""
    nf = len(t_ins)
    ins = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_ins])
    outs = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_outs])
    ct = np.zeros((nranks, nf, num_clusters), np.uint32)
    kout = np.zeros((nranks, nf), np.uint32)
    log = np.zeros((nranks, log_cap), np.uint64)
    nlog = np.zeros(nranks, np.int32)
    r = lib().dq_hip_loopback_rows_dev(device, nranks, nf, ctypes.cast(ins, ctypes.c_void_p), width, height,
                                       ctypes.cast(outs, ctypes.c_void_p), num_clusters, _ptr(ct), _ptr(kout),
                                       max_iters, _ptr(log), log_cap, _ptr(nlog))
    if r < 0:
        raise DivQuantError("dq_hip_loopback_rows_dev: bad arguments")
    if nlog.max() > log_cap:
        raise DivQuantError("collective log longer than log_cap")
    cts = [[ct[q, i, :kout[q, i]].copy() for i in range(nf)] for q in range(nranks)]
    logs = [log[q, :nlog[q]].tolist() for q in range(nranks)]
    return cts, logs, r


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it; broadcast it to the other ranks)."""
    buf = ctypes.create_string_buffer(128)
    if lib().dq_hip_comm_unique_id(buf) != 0:
        raise DivQuantError("dq_hip_comm_unique_id failed")
    return buf.raw


def comm_init(nranks, rank, uid, device=0):
    """Join the engine on `device` to an RCCL communicator (one process per GPU)."""
    buf = ctypes.create_string_buffer(bytes(uid), 128)
    if lib().dq_hip_comm_init(device, nranks, rank, buf) != 0:
        raise DivQuantError("dq_hip_comm_init: bad arguments")


def comm_destroy(device=0):
    lib().dq_hip_comm_destroy(device)


def comm_size(device=0):
    """Ranks of the engine's RCCL communicator on `device` (1: none)."""
    return lib().dq_hip_comm_size(device)


def comm_init_torch(device=0, group=None):
    """comm_init over an initialised torch.distributed process group: rank 0's
    id is broadcast with the group (any backend), then every rank joins."""
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    obj = [comm_unique_id() if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0, group=group)
    comm_init(world, rank, obj[0], device=device)


def cluster_device(t_in, num_clusters, max_iters=10, device=0, n=None, stream=None):
    """DivQuantCluster on device-resident pixels; returns (colortable, empty)."""
    n = _nelem(t_in, n)
    ct = np.zeros(num_clusters, np.uint32)
    k = ctypes.c_uint32(num_clusters)
    r = lib().dq_hip_cluster_dev(device, _dptr(t_in), n, ctypes.byref(k), _ptr(ct), max_iters,
                                 _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_cluster_dev: bad arguments")
    return ct[:k.value].copy(), r


def map_device(t_in, t_out, colortable, device=0, n=None, stream=None):
    n = _nelem(t_in, n)
    ct = _u32(colortable).reshape(-1)
    if lib().dq_hip_map_dev(device, _dptr(t_in), n, _dptr(t_out), _ptr(ct), ct.size,
                            _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_map_dev: bad arguments")


# ---------------------------------------------------------------------------
# Cluster labels: each pixel's index into the colortable instead of its mapped
# colour (include/dq_hip.h: the lowest i with ct[i] == the mapped colour).  The
# label width is the label tensor's element size: 1, 2 or 4 bytes (uint8,
# uint16 / int16, uint32 / int32 storage).
def _label_width(t, n, what="t_labels"):
    """Element size of a label tensor (torch tensor or numpy array) after the
    checks every label entry point makes before it calls the library."""
    if isinstance(t, np.ndarray):
        size, contiguous, count = t.itemsize, t.flags.c_contiguous, t.size
    elif hasattr(t, "element_size"):
        size, contiguous, count = t.element_size(), t.is_contiguous(), t.numel()
    else:
        raise ValueError("%s: a tensor or an array (its element size is the label width)" % what)
    if size not in (1, 2, 4):
        raise ValueError("%s: labels are 1, 2 or 4 bytes wide, not %d" % (what, size))
    if not contiguous:
        raise ValueError("%s is not contiguous" % what)
    if count < n:
        raise ValueError("%s holds %d labels, the input has %d pixels" % (what, count, n))
    return size


def map_labels_device(t_in, t_labels, colortable, device=0, n=None, stream=None):
    """The cluster label of each of n device-resident pixels: the lowest index
    i with colortable[i] == the colour map_device writes for the pixel.
    t_labels: a contiguous device tensor of at least n elements of 1, 2 or 4
    bytes (the width must hold len(colortable) - 1).  ValueError for a bad
    label tensor (nothing runs), DivQuantError when the library refuses."""
    n = _nelem(t_in, n)
    width = _label_width(t_labels, n)
    ct = _u32(colortable).reshape(-1)
    if lib().dq_hip_map_labels_dev(device, _dptr(t_in), n, _dptr(t_labels), width, _ptr(ct), ct.size,
                                   _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_map_labels_dev: bad arguments")


def quant_labels_batch_device(t_ins, t_labels, num_clusters, all_pixels_unique=1, max_iters=10, device=0,
                              stream=None):
    """quant_batch_device with labels in place of colours: frame i's labels
    (t_labels[i], one width for the whole batch) index its deduplicated
    colortable.  all_pixels_unique=0: every frame through the weighted path.
    Returns ([colortable per frame], total_empty)."""
    nf = len(t_ins)
    if len(t_labels) != nf:
        raise ValueError("%d label tensors for %d frames" % (len(t_labels), nf))
    widths = {_label_width(t, ti.numel(), "t_labels[%d]" % i) for i, (t, ti) in enumerate(zip(t_labels, t_ins))}
    if len(widths) > 1:
        raise ValueError("the label tensors of a batch must have one element size")
    if nf == 0:
        raise ValueError("empty batch")
    ins = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_ins])
    labs = (ctypes.c_void_p * nf)(*[_dptr(t).value for t in t_labels])
    ns = np.array([t.numel() for t in t_ins], np.uint32)
    ct = np.zeros((nf, num_clusters), np.uint32)
    kout = np.zeros(nf, np.uint32)
    r = lib().dq_hip_quant_labels_batch_dev(device, nf, ctypes.cast(ins, ctypes.c_void_p), _ptr(ns),
                                            ctypes.cast(labs, ctypes.c_void_p), widths.pop(), num_clusters,
                                            _ptr(ct), _ptr(kout), int(all_pixels_unique), max_iters,
                                            _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_quant_labels_batch_dev: bad arguments")
    return [ct[i, :kout[i]].copy() for i in range(nf)], r


def quant_labels(pixels, num_clusters, all_pixels_unique=1, dtype=None):
    """quant_recurse of host pixels returning (labels, colortable): labels[i]
    is pixel i's index into the (deduplicated) colortable.  dtype: uint8,
    uint16 or uint32 (None: the narrowest that holds num_clusters - 1)."""
    if dtype is None:
        dtype = np.uint8 if num_clusters <= 256 else np.uint16 if num_clusters <= 65536 else np.uint32
    dtype = np.dtype(dtype)
    if dtype.itemsize not in (1, 2, 4) or dtype.kind not in "ui":
        raise ValueError("labels are 1-, 2- or 4-byte integers, not %s" % dtype)
    _require_gpu()
    px = _u32(pixels).reshape(-1)
    labels = np.zeros(px.size, dtype)
    ct = np.zeros(max(int(num_clusters), 1), np.uint32)
    k = ctypes.c_uint32(max(int(num_clusters), 0))
    if lib().dq_hip_quant_labels(_ptr(px), px.size, _ptr(labels), dtype.itemsize, ctypes.byref(k), _ptr(ct),
                                 int(all_pixels_unique)) < 0:
        raise DivQuantError("dq_hip_quant_labels: bad arguments")
    return labels, ct[:k.value].copy()


# ---------------------------------------------------------------------------
# Connected regions of a label map (include/dq_hip.h, "connected regions"):
# pixels joined by a path of 4- / 8-neighbours with equal labels, numbered in
# raster order of their first pixel.  Exact integers, independent of scheduling.
REGION_TILE = 64          # DQ_HIP_REGION_TILE: the tile pass works on 64 x 64 tiles
REGION_MAX_SIDE = 65535   # width, height (the Coord layout)
REGION_MAX_PIXELS = (1 << 31) - 1


def _region_shape(width, height, connectivity):
    width, height = int(width), int(height)
    if not (1 <= width <= REGION_MAX_SIDE and 1 <= height <= REGION_MAX_SIDE) or width * height > REGION_MAX_PIXELS:
        raise ValueError("a %d x %d map: sides are 1..65535, at most 2^31 - 1 pixels" % (width, height))
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8, not %r" % (connectivity,))
    return width, height


def _words(t, n, what):
    """A contiguous tensor / array of at least n 4-byte elements."""
    if _label_width(t, n, what) != 4:
        raise ValueError("%s: 4-byte elements (int32 / uint32 storage)" % what)


def label_regions_device(t_labels, width, height, t_regions, connectivity=8, stats_capacity=0, t_pixels=None,
                         device=0, stream=None):
    """Connected regions of a device-resident width x height label map.
    t_labels: contiguous, 1, 2 or 4 bytes per label; t_regions: contiguous,
    4-byte elements, gets each pixel's region id.  Returns (R, stats): R the
    region count, stats a dict of device tensors holding the first
    min(R, stats_capacity) regions -- "area", "bbox" (x0, y0, x1, y1,
    inclusive), "first" (y * width + x of the first pixel), "label" (int32
    storage of the uint32 values) and, with t_pixels (the packed 0x00RRGGBB
    frame), "sums" (int64: R, G, B sums) -- empty at capacity 0.  Synchronous.
    ValueError for bad tensors or shapes (nothing runs)."""
    width, height = _region_shape(width, height, connectivity)
    n = width * height
    lb = _label_width(t_labels, n)
    _words(t_regions, n, "t_regions")
    if t_pixels is not None:
        _words(t_pixels, n, "t_pixels")
    cap = int(stats_capacity)
    if not 0 <= cap <= 0xFFFFFFFF:
        raise ValueError("stats_capacity %d" % cap)
    st = {}
    if cap:
        import torch
        dev = f"cuda:{device}"
        st = {"area": torch.empty(cap, dtype=torch.int32, device=dev),
              "bbox": torch.empty((cap, 4), dtype=torch.int32, device=dev),
              "first": torch.empty(cap, dtype=torch.int32, device=dev),
              "label": torch.empty(cap, dtype=torch.int32, device=dev)}
        if t_pixels is not None:
            st["sums"] = torch.empty((cap, 3), dtype=torch.int64, device=dev)
    opt = lambda name: _dptr(st[name]) if name in st else None  # noqa: E731
    r = lib().dq_hip_label_regions_dev(device, _dptr(t_labels), lb, width, height, connectivity, _dptr(t_regions),
                                       cap, opt("area"), opt("bbox"), opt("first"), opt("label"),
                                       _dptr(t_pixels) if t_pixels is not None else None, opt("sums"),
                                       _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_label_regions_dev: bad arguments")
    return int(r), {k: v[:min(int(r), cap)] for k, v in st.items()}


def label_regions(labels2d, connectivity=8, pixels=None):
    """Connected regions of a host (H, W) label map of 1-, 2- or 4-byte
    integers.  Returns (regions2d, stats): regions2d (H, W) uint32 and stats a
    dict of numpy arrays sized to the region count R -- "area" (R,), "bbox"
    (R, 4: x0, y0, x1, y1 inclusive), "first" (R,), "label" (R,), all uint32,
    and with pixels (H * W packed 0x00RRGGBB words) "sums" (R, 3) uint64.
    Two calls: one for the map and R, one with room for R regions."""
    lab = np.asarray(labels2d)
    if lab.ndim != 2 or lab.size == 0:
        raise ValueError("labels2d must be a non-empty (H, W) array")
    if lab.dtype.kind not in "ui" or lab.dtype.itemsize not in (1, 2, 4):
        raise ValueError("labels are 1-, 2- or 4-byte integers, not %s" % lab.dtype)
    lab = np.ascontiguousarray(lab)
    h, w = lab.shape
    _region_shape(w, h, connectivity)
    px = None
    if pixels is not None:
        px = _u32(pixels).reshape(-1)
        if px.size != lab.size:
            raise ValueError("%d pixels for %d labels" % (px.size, lab.size))
    _require_gpu()
    regions = np.zeros((h, w), np.uint32)
    call = lib().dq_hip_label_regions
    r = call(_ptr(lab), lab.dtype.itemsize, w, h, connectivity, _ptr(regions), 0, None, None, None, None, None, None)
    if r < 0:
        raise DivQuantError("dq_hip_label_regions: bad arguments")
    st = {"area": np.zeros(r, np.uint32), "bbox": np.zeros((r, 4), np.uint32), "first": np.zeros(r, np.uint32),
          "label": np.zeros(r, np.uint32)}
    if px is not None:
        st["sums"] = np.zeros((r, 3), np.uint64)
    r2 = call(_ptr(lab), lab.dtype.itemsize, w, h, connectivity, _ptr(regions), r, _ptr(st["area"]), _ptr(st["bbox"]),
              _ptr(st["first"]), _ptr(st["label"]), _ptr(px) if px is not None else None,
              _ptr(st["sums"]) if px is not None else None)
    if r2 != r:
        raise DivQuantError("dq_hip_label_regions: %d regions, then %d" % (r, r2))
    return regions, st


# ---------------------------------------------------------------------------
# Region adjacency graph of a region map (include/dq_hip.h, "region adjacency
# graph"): the pairs of ids that touch, numbered in raster order of their first
# contact, with border length, first contact, colour step sum and the degree of
# every id.  Exact integers, independent of scheduling.
ADJACENCY_MAX_PIXELS = 1 << 30   # DQ_HIP_ADJACENCY_MAX_PIXELS: a contact is the word 4 * p + dir


def _adjacency_shape(width, height, connectivity):
    width, height = int(width), int(height)
    if (not (1 <= width <= REGION_MAX_SIDE and 1 <= height <= REGION_MAX_SIDE)
            or width * height > ADJACENCY_MAX_PIXELS):
        raise ValueError("a %d x %d map: sides are 1..65535, at most 2^30 pixels" % (width, height))
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8, not %r" % (connectivity,))
    return width, height


def region_adjacency_device(t_regions, width, height, connectivity=8, edge_capacity=0, t_pixels=None,
                            num_regions=0, device=0, stream=None):
    """The adjacency graph of a device-resident width x height map of region
    ids (contiguous, 4-byte elements; any id map).  Returns (E, graph): E the
    edge count, graph a dict of device tensors holding the first
    min(E, edge_capacity) edges -- "edges" (., 2: a < b), "border" (contacts of
    the edge), "contact" (., 2: p < q of its first contact; int32 storage of
    the uint32 values) and, with t_pixels (the packed 0x00RRGGBB frame), "step"
    (int64: sum of |dR| + |dG| + |dB| over the contacts) -- none of them at
    capacity 0, and with num_regions > 0 "degree" (num_regions,): the edges at
    every id, over all E edges (ids in the map must be < num_regions).
    Synchronous.  ValueError for bad tensors or shapes (nothing runs)."""
    width, height = _adjacency_shape(width, height, connectivity)
    n = width * height
    _words(t_regions, n, "t_regions")
    if t_pixels is not None:
        _words(t_pixels, n, "t_pixels")
    cap, nreg = int(edge_capacity), int(num_regions)
    if not 0 <= cap <= 0xFFFFFFFF:
        raise ValueError("edge_capacity %d" % cap)
    if not 0 <= nreg <= 0xFFFFFFFF:
        raise ValueError("num_regions %d" % nreg)
    g = {}
    if cap or nreg:
        import torch
        dev = f"cuda:{device}"
        if cap:
            g = {"edges": torch.empty((cap, 2), dtype=torch.int32, device=dev),
                 "border": torch.empty(cap, dtype=torch.int32, device=dev),
                 "contact": torch.empty((cap, 2), dtype=torch.int32, device=dev)}
            if t_pixels is not None:
                g["step"] = torch.empty(cap, dtype=torch.int64, device=dev)
        if nreg:
            g["degree"] = torch.empty(nreg, dtype=torch.int32, device=dev)
    opt = lambda name: _dptr(g[name]) if name in g else None  # noqa: E731
    e = lib().dq_hip_region_adjacency_dev(device, _dptr(t_regions), width, height, connectivity, cap, opt("edges"),
                                          opt("border"), opt("contact"),
                                          _dptr(t_pixels) if t_pixels is not None else None, opt("step"), nreg,
                                          opt("degree"), _stream_ptr(stream))
    if e < 0:
        raise DivQuantError("dq_hip_region_adjacency_dev: bad arguments")
    return int(e), {k: (v if k == "degree" else v[:min(int(e), cap)]) for k, v in g.items()}


def region_adjacency(regions2d, connectivity=8, pixels=None, num_regions=None):
    """The adjacency graph of a host (H, W) map of region ids (integers of at
    most 4 bytes).  Returns a dict of numpy arrays sized to the edge count E --
    "edges" (E, 2: a < b), "border" (E,), "contact" (E, 2: p < q), all uint32,
    with pixels (H * W packed 0x00RRGGBB words) "step" (E,) uint64 -- and
    "degree" (num_regions,) uint32; num_regions=None takes regions2d.max() + 1.
    Two calls: one for E, one with room for E edges."""
    reg = np.asarray(regions2d)
    if reg.ndim != 2 or reg.size == 0:
        raise ValueError("regions2d must be a non-empty (H, W) array")
    if reg.dtype.kind not in "ui" or reg.dtype.itemsize > 4:
        raise ValueError("region ids are integers of at most 4 bytes, not %s" % reg.dtype)
    if reg.dtype.kind == "i" and reg.min() < 0:
        raise ValueError("region ids are not negative")
    reg = _u32(reg)
    h, w = reg.shape
    _adjacency_shape(w, h, connectivity)
    px = None
    if pixels is not None:
        px = _u32(pixels).reshape(-1)
        if px.size != reg.size:
            raise ValueError("%d pixels for %d region ids" % (px.size, reg.size))
    nreg = int(reg.max()) + 1 if num_regions is None else int(num_regions)
    if not int(reg.max()) < nreg <= 0xFFFFFFFF:
        raise ValueError("num_regions %d for ids up to %d" % (nreg, int(reg.max())))
    _require_gpu()
    degree = np.zeros(nreg, np.uint32)
    call = lib().dq_hip_region_adjacency
    e = call(_ptr(reg), w, h, connectivity, 0, None, None, None, None, None, 0, None)
    if e < 0:
        raise DivQuantError("dq_hip_region_adjacency: bad arguments")
    g = {"edges": np.zeros((e, 2), np.uint32), "border": np.zeros(e, np.uint32),
         "contact": np.zeros((e, 2), np.uint32)}
    if px is not None:
        g["step"] = np.zeros(e, np.uint64)
    some = e > 0   # (capacity 0 takes no edge pointers)
    e2 = call(_ptr(reg), w, h, connectivity, e, _ptr(g["edges"]) if some else None,
              _ptr(g["border"]) if some else None, _ptr(g["contact"]) if some else None,
              _ptr(px) if px is not None else None, _ptr(g["step"]) if px is not None and some else None,
              nreg, _ptr(degree))
    if e2 != e:
        raise DivQuantError("dq_hip_region_adjacency: %d edges, then %d" % (e, e2))
    g["degree"] = degree
    return g


# ---------------------------------------------------------------------------
# Region merge over the adjacency graph (include/dq_hip.h, "region merge"):
# components under min_area join their most alike neighbour (8.8 fixed-point
# mean colour, ties to the lowest id) in Boruvka-style rounds; the result is
# numbered by first pixel.  Exact integers, independent of scheduling.
MERGE_MAX_PIXELS = (1 << 31) - 1
NO_DISTANCE_LIMIT = 0xFFFFFFFF


def _elems(t, count, size, what):
    """A contiguous tensor / array of at least `count` elements of `size` bytes."""
    if isinstance(t, np.ndarray):
        have, contiguous, length = t.itemsize, t.flags.c_contiguous, t.size
    elif hasattr(t, "element_size"):
        have, contiguous, length = t.element_size(), t.is_contiguous(), t.numel()
    else:
        raise ValueError("%s: a tensor or an array" % what)
    if have != size:
        raise ValueError("%s: %d-byte elements, not %d" % (what, size, have))
    if not contiguous:
        raise ValueError("%s is not contiguous" % what)
    if length < count:
        raise ValueError("%s holds %d elements, %d are needed" % (what, length, count))


def _scalar32(v, what):
    v = int(v)
    if not 0 <= v <= 0xFFFFFFFF:
        raise ValueError("%s %d is not a uint32" % (what, v))
    return v


def merge_regions_device(t_regions, num_regions, t_area, t_first, t_sums, t_edges, min_area,
                         max_dist=NO_DISTANCE_LIMIT, max_rounds=0, t_bbox=None, num_edges=None, t_out_regions=None,
                         stats_capacity=0, with_remap=True, n=None, device=0, stream=None):
    """Merges the regions of a device-resident id map over their adjacency
    graph.  t_regions: n ids < num_regions (contiguous, 4-byte elements; n
    defaults to its length); t_area, t_first (num_regions words), t_sums
    (num_regions x 3, 8-byte elements) and optionally t_bbox (num_regions x 4
    words) as label_regions_device gives them; t_edges: num_edges x 2 ids
    (num_edges defaults to its length / 2; None with no edge).
    t_out_regions=None relabels t_regions in place.  Returns (R', rounds, out):
    out["regions"] the relabelled map, out["remap"] (num_regions,) the new id
    of every old region (unless with_remap=False) and the first
    min(R', stats_capacity) new regions' "area", "first", "sums" (int64) and,
    with t_bbox, "bbox" -- none of them at capacity 0.  Synchronous.
    ValueError for bad tensors, lengths or scalars (nothing runs)."""
    _elems(t_regions, 0, 4, "t_regions")     # (tensors only: the lengths are checked against them)
    if n is None:
        n = t_regions.size if isinstance(t_regions, np.ndarray) else t_regions.numel()
    n, nreg = int(n), int(num_regions)
    if not 1 <= n <= MERGE_MAX_PIXELS:
        raise ValueError("%d pixels: 1 .. 2^31 - 1" % n)
    if not 1 <= nreg <= n:
        raise ValueError("num_regions %d for %d pixels" % (nreg, n))
    _elems(t_regions, n, 4, "t_regions")
    _elems(t_area, nreg, 4, "t_area")
    _elems(t_first, nreg, 4, "t_first")
    _elems(t_sums, 3 * nreg, 8, "t_sums")
    if t_bbox is not None:
        _elems(t_bbox, 4 * nreg, 4, "t_bbox")
    if num_edges is None:
        if t_edges is not None:
            _elems(t_edges, 0, 4, "t_edges")
        num_edges = 0 if t_edges is None else (t_edges.size if isinstance(t_edges, np.ndarray) else t_edges.numel()) // 2
    nedges = _scalar32(num_edges, "num_edges")
    if nedges:
        if t_edges is None:
            raise ValueError("%d edges without t_edges" % nedges)
        _elems(t_edges, 2 * nedges, 4, "t_edges")
    if t_out_regions is None:
        t_out_regions = t_regions
    else:
        _elems(t_out_regions, n, 4, "t_out_regions")
    min_area, max_dist = _scalar32(min_area, "min_area"), _scalar32(max_dist, "max_dist")
    max_rounds, cap = _scalar32(max_rounds, "max_rounds"), _scalar32(stats_capacity, "stats_capacity")
    out = {"regions": t_out_regions}
    st = {}
    if cap or with_remap:
        import torch
        dev = f"cuda:{device}"
        if with_remap:
            out["remap"] = torch.empty(nreg, dtype=torch.int32, device=dev)
        if cap:
            st = {"area": torch.empty(cap, dtype=torch.int32, device=dev),
                  "first": torch.empty(cap, dtype=torch.int32, device=dev),
                  "sums": torch.empty((cap, 3), dtype=torch.int64, device=dev)}
            if t_bbox is not None:
                st["bbox"] = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    opt = lambda d, name: _dptr(d[name]) if name in d else None  # noqa: E731
    rounds = ctypes.c_uint32(0)
    r = lib().dq_hip_merge_regions_dev(device, _dptr(t_regions), n, nreg, _dptr(t_area), _dptr(t_first), _dptr(t_sums),
                                       _dptr(t_bbox) if t_bbox is not None else None, nedges,
                                       _dptr(t_edges) if nedges else None, min_area, max_dist, max_rounds,
                                       _dptr(t_out_regions), opt(out, "remap"), cap, opt(st, "area"), opt(st, "bbox"),
                                       opt(st, "first"), opt(st, "sums"), ctypes.byref(rounds), _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_merge_regions_dev: bad arguments")
    out.update({k: v[:min(int(r), cap)] for k, v in st.items()})
    return int(r), int(rounds.value), out


def segment_labels(labels2d, pixels, min_area, max_dist=NO_DISTANCE_LIMIT, connectivity=8, max_rounds=0,
                   stats_capacity=1 << 16):
    """Segments of a host (H, W) label map of 1-, 2- or 4-byte integers and
    its frame (H * W packed 0x00RRGGBB words): connected regions, their
    adjacency graph and the merge, all on the device between one upload and one
    download.  Returns (regions2d, stats, rounds): regions2d (H, W) uint32 with
    R' segments numbered by first pixel, stats a dict of numpy arrays sized to
    R' -- "area" (R',), "bbox" (R', 4: x0, y0, x1, y1 inclusive), "first"
    (R',), all uint32, "sums" (R', 3) uint64 -- and the rounds counted.
    stats_capacity: the segments the first call has room for (48 B each on the
    host); a frame that ends with more is run once more with room for all."""
    lab = np.asarray(labels2d)
    if lab.ndim != 2 or lab.size == 0:
        raise ValueError("labels2d must be a non-empty (H, W) array")
    if lab.dtype.kind not in "ui" or lab.dtype.itemsize not in (1, 2, 4):
        raise ValueError("labels are 1-, 2- or 4-byte integers, not %s" % lab.dtype)
    lab = np.ascontiguousarray(lab)
    h, w = lab.shape
    _adjacency_shape(w, h, connectivity)
    if pixels is None:
        raise ValueError("the frame is needed: the merge compares mean colours")
    px = _u32(pixels).reshape(-1)
    if px.size != lab.size:
        raise ValueError("%d pixels for %d labels" % (px.size, lab.size))
    min_area, max_dist = _scalar32(min_area, "min_area"), _scalar32(max_dist, "max_dist")
    max_rounds, cap = _scalar32(max_rounds, "max_rounds"), _scalar32(stats_capacity, "stats_capacity")
    if cap < 1:
        raise ValueError("stats_capacity is at least 1")
    _require_gpu()
    regions = np.zeros((h, w), np.uint32)
    rounds = ctypes.c_uint32(0)
    cap = min(cap, lab.size)
    while True:     # (R' is not known before the call: at most one more call, with room for R')
        st = {"area": np.zeros(cap, np.uint32), "bbox": np.zeros((cap, 4), np.uint32),
              "first": np.zeros(cap, np.uint32), "sums": np.zeros((cap, 3), np.uint64)}
        r = lib().dq_hip_segment_labels(_ptr(lab), lab.dtype.itemsize, w, h, connectivity, _ptr(px), min_area,
                                        max_dist, max_rounds, _ptr(regions), cap, _ptr(st["area"]), _ptr(st["bbox"]),
                                        _ptr(st["first"]), _ptr(st["sums"]), ctypes.byref(rounds))
        if r < 0:
            raise DivQuantError("dq_hip_segment_labels: bad arguments")
        if r <= cap:
            return regions, {k: v[:r].copy() for k, v in st.items()}, int(rounds.value)
        cap = int(r)


# ---------------------------------------------------------------------------
# Pixel lists of a region map (include/dq_hip.h, "pixel lists"): the stable
# counting sort of the pixels by region id, as offsets (CSR) plus the pixel
# indexes, Coord words and frame words in that order; its inverse; and the
# region map -> per-region quant -> painted frame pipeline on top of them.
# Exact integers, independent of scheduling.
PIXELS_MAX_PIXELS = (1 << 31) - 1
PIXELS_MAX_REGIONS = (1 << 31) - 1


class RegionRowsError(DivQuantError):
    """The library's -2: the ids of the map span more rows in total than the
    map has pixels (never so for connected regions)."""


def _pixels_shape(width, height, num_regions):
    width, height, nreg = int(width), int(height), int(num_regions)
    if not (1 <= width <= REGION_MAX_SIDE and 1 <= height <= REGION_MAX_SIDE) or width * height > PIXELS_MAX_PIXELS:
        raise ValueError("a %d x %d map: sides are 1..65535, at most 2^31 - 1 pixels" % (width, height))
    if not 1 <= nreg <= PIXELS_MAX_REGIONS:
        raise ValueError("num_regions %d: 1 .. 2^31 - 1" % nreg)
    return width, height, nreg


def _pixels_result(r, name):
    if r == -2:
        raise RegionRowsError("%s: the ids span more rows in total than the map has pixels" % name)
    if r < 0:
        raise DivQuantError("%s: bad arguments" % name)
    return int(r)


def region_pixels_device(t_regions, width, height, num_regions, t_offsets, t_coords=None, t_index=None,
                         t_pixels=None, t_colors=None, device=0, stream=None):
    """The pixel lists of a device-resident width x height map of region ids
    (< num_regions each; contiguous, 4-byte elements).  t_offsets gets
    num_regions + 1 words: t_offsets[r] = the pixels with an id < r.  Each of
    t_coords (x | y << 16), t_index (y * width + x) and t_colors (t_pixels
    there; needs t_pixels), width * height words, is filled when given: region
    r's pixels in raster order at [t_offsets[r], t_offsets[r + 1]).
    Synchronous.  ValueError for bad tensors or shapes (nothing runs),
    RegionRowsError when the library refuses the map (nothing is written)."""
    width, height, nreg = _pixels_shape(width, height, num_regions)
    n = width * height
    _elems(t_regions, n, 4, "t_regions")
    _elems(t_offsets, nreg + 1, 4, "t_offsets")
    for t, what in ((t_coords, "t_coords"), (t_index, "t_index"), (t_pixels, "t_pixels"), (t_colors, "t_colors")):
        if t is not None:
            _elems(t, n, 4, what)
    if t_colors is not None and t_pixels is None:
        raise ValueError("t_colors without t_pixels")
    opt = lambda t: _dptr(t) if t is not None else None  # noqa: E731
    r = lib().dq_hip_region_pixels_dev(device, _dptr(t_regions), width, height, nreg, _dptr(t_offsets), opt(t_coords),
                                       opt(t_index), opt(t_pixels), opt(t_colors), _stream_ptr(stream))
    _pixels_result(r, "dq_hip_region_pixels_dev")


def _region_map(regions2d, num_regions):
    """A host (H, W) map of ids as contiguous uint32, and its id count."""
    reg = np.asarray(regions2d)
    if reg.ndim != 2 or reg.size == 0:
        raise ValueError("regions2d must be a non-empty (H, W) array")
    if reg.dtype.kind not in "ui" or reg.dtype.itemsize > 4:
        raise ValueError("region ids are integers of at most 4 bytes, not %s" % reg.dtype)
    if reg.dtype.kind == "i" and reg.min() < 0:
        raise ValueError("region ids are not negative")
    reg = _u32(reg)
    top = int(reg.max())
    nreg = top + 1 if num_regions is None else int(num_regions)
    if not top < nreg:
        raise ValueError("num_regions %d for ids up to %d" % (nreg, top))
    _pixels_shape(reg.shape[1], reg.shape[0], nreg)
    return reg, nreg


def region_pixels(regions2d, num_regions=None, pixels=None):
    """The pixel lists of a host (H, W) map of region ids (integers of at most
    4 bytes; num_regions=None takes regions2d.max() + 1).  Returns (offsets,
    index, coords, colours), uint32: offsets (num_regions + 1,), and per pixel
    in list order its index y * W + x, its Coord word x | y << 16 and, with
    pixels (H * W words), its frame word (None without)."""
    reg, nreg = _region_map(regions2d, num_regions)
    h, w = reg.shape
    px = None
    if pixels is not None:
        px = _u32(pixels).reshape(-1)
        if px.size != reg.size:
            raise ValueError("%d pixels for %d region ids" % (px.size, reg.size))
    _require_gpu()
    offsets = np.zeros(nreg + 1, np.uint32)
    index, coords = np.zeros(reg.size, np.uint32), np.zeros(reg.size, np.uint32)
    colours = np.zeros(reg.size, np.uint32) if px is not None else None
    r = lib().dq_hip_region_pixels(_ptr(reg), w, h, nreg, _ptr(offsets), _ptr(coords), _ptr(index),
                                   _ptr(px) if px is not None else None,
                                   _ptr(colours) if px is not None else None)
    _pixels_result(r, "dq_hip_region_pixels")
    return offsets, index, coords, colours


def scatter_coords_device(t_values, t_coords, n, width, t_frame, device=0, stream=None):
    """t_frame[(c >> 16) * width + (c & 0xFFFF)] = t_values[i] for the n Coord
    words c = t_coords[i] (the inverse of a gather by Coords), asynchronous.
    Coords are not range-checked.  ValueError for bad tensors or scalars."""
    n, width = _scalar32(n, "n"), int(width)
    if not 1 <= width <= REGION_MAX_SIDE:
        raise ValueError("width %d: 1 .. 65535" % width)
    _elems(t_values, n, 4, "t_values")
    _elems(t_coords, n, 4, "t_coords")
    _elems(t_frame, min(n, 1), 4, "t_frame")
    if lib().dq_hip_scatter_coords_dev(device, _dptr(t_values), _dptr(t_coords), n, width, _dptr(t_frame),
                                       _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_scatter_coords_dev: bad arguments")


def _region_map_tables(nreg, k, cts, k_outs):
    """The host colortable rows and sizes of a region-map call (given: filled in place)."""
    if cts is None:
        cts = np.zeros((nreg, k), np.uint32)
    elif not (isinstance(cts, np.ndarray) and cts.dtype == np.uint32 and cts.flags.c_contiguous and cts.size >= nreg * k):
        raise ValueError("cts: a contiguous uint32 array of num_regions * num_clusters entries")
    if k_outs is None:
        k_outs = np.zeros(nreg, np.uint32)
    elif not (isinstance(k_outs, np.ndarray) and k_outs.dtype == np.uint32 and k_outs.flags.c_contiguous
              and k_outs.size >= nreg):
        raise ValueError("k_outs: a contiguous uint32 array of num_regions entries")
    return cts, k_outs


def _region_map_scalars(num_clusters, max_iters):
    k, max_iters = int(num_clusters), int(max_iters)
    if not 1 <= k <= 0x7FFFFFFF:
        raise ValueError("num_clusters %d" % k)
    if not 1 <= max_iters <= 0x7FFFFFFF:
        raise ValueError("max_iters %d" % max_iters)
    return k, max_iters


def quant_region_map_device(t_regions, width, height, num_regions, t_pixels, num_clusters, t_out=None, max_iters=10,
                            cts=None, k_outs=None, device=0, stream=None):
    """quant_recurse(N_region, .., K, allPixelsUnique=0) of every region of a
    device-resident region map (ClusteringSegmentation.cpp:1779-1846): the
    pixel lists, one call of the weighted-regions path over them and, with
    t_out (width * height words), every pixel painted with its mapped colour.
    Returns (cts, k_outs, empty): region r's colortable is
    cts[r, :k_outs[r]]; an id without a pixel has k_outs[r] == 0 and its row of
    cts (zeros, or the array passed in) untouched.  Synchronous.  ValueError
    for bad tensors, shapes or scalars (nothing runs), RegionRowsError when
    the library refuses the map."""
    width, height, nreg = _pixels_shape(width, height, num_regions)
    n = width * height
    k, max_iters = _region_map_scalars(num_clusters, max_iters)
    _elems(t_regions, n, 4, "t_regions")
    _elems(t_pixels, n, 4, "t_pixels")
    if t_out is not None:
        _elems(t_out, n, 4, "t_out")
    cts, k_outs = _region_map_tables(nreg, k, cts, k_outs)
    r = lib().dq_hip_quant_region_map_dev(device, _dptr(t_regions), width, height, nreg, _dptr(t_pixels), k,
                                          _dptr(t_out) if t_out is not None else None, _ptr(cts), _ptr(k_outs),
                                          max_iters, _stream_ptr(stream))
    return cts, k_outs, _pixels_result(r, "dq_hip_quant_region_map_dev")


def quant_region_map(regions2d, pixels, num_clusters, num_regions=None, max_iters=10, paint=True, cts=None,
                     k_outs=None):
    """quant_region_map_device on a host (H, W) map of region ids and its frame
    (H * W packed 0x00RRGGBB words), between one upload and one download.
    Returns (out2d, cts, k_outs, empty): out2d (H, W) uint32, the painted
    frame (None with paint=False)."""
    reg, nreg = _region_map(regions2d, num_regions)
    h, w = reg.shape
    if pixels is None:
        raise ValueError("the frame is needed")
    px = _u32(pixels).reshape(-1)
    if px.size != reg.size:
        raise ValueError("%d pixels for %d region ids" % (px.size, reg.size))
    k, max_iters = _region_map_scalars(num_clusters, max_iters)
    cts, k_outs = _region_map_tables(nreg, k, cts, k_outs)
    _require_gpu()
    out = np.zeros((h, w), np.uint32) if paint else None
    r = lib().dq_hip_quant_region_map(_ptr(reg), w, h, nreg, _ptr(px), k, _ptr(out) if paint else None, _ptr(cts),
                                      _ptr(k_outs), max_iters)
    return out, cts, k_outs, _pixels_result(r, "dq_hip_quant_region_map")


# ---------------------------------------------------------------------------
# Capture windows of a region map (include/dq_hip.h, "capture windows"): per
# region the pixels of the block x block blocks at L1 distance <= expand from a
# block the region has a pixel in, block by block in raster order, without the
# masked pixels -- the lists captureRegionMask works on.  One pixel is in many
# lists: the total length M is not bounded by the map and is counted first.
WINDOWS_MAX_BLOCK = 8
WINDOWS_MAX_EXPAND = 3
WINDOWS_MAX_ENTRIES = (1 << 32) - 2     # M (and the pairs of a block and a member id)
WINDOWS_BLOCK, WINDOWS_EXPAND = 4, 2    # the reference's


class WindowsOverflowError(DivQuantError):
    """The library's -3: the lists hold 2^32 - 1 entries or more."""


class WindowsCapacityError(DivQuantError):
    """The library's -4: the mapped colours were asked for and the lists are
    longer than the capacity given (the offsets are written: their last word
    is the length needed)."""


def _windows_scalars(block, expand, min_area, capacity):
    block, expand = int(block), int(expand)
    if not 1 <= block <= WINDOWS_MAX_BLOCK:
        raise ValueError("block %d: 1 .. 8" % block)
    if not 0 <= expand <= WINDOWS_MAX_EXPAND:
        raise ValueError("expand %d: 0 .. 3" % expand)
    return block, expand, _scalar32(min_area, "min_area"), _scalar32(capacity, "capacity")


def _windows_result(r, name):
    if r == -2:
        raise RegionRowsError("%s: the windows span more block rows in total than they have blocks" % name)
    if r == -3:
        raise WindowsOverflowError("%s: the lists hold 2^32 - 1 entries or more" % name)
    if r == -4:
        raise WindowsCapacityError("%s: the lists are longer than the capacity given" % name)
    if r < 0:
        raise DivQuantError("%s: bad arguments" % name)
    return int(r)


def _windows_tensors(n, nreg, cap, t_regions, t_offsets, t_mask, t_area, t_pixels, lists):
    """The tensor checks of the windows calls; lists: (tensor, name) of `cap` words each."""
    _elems(t_regions, n, 4, "t_regions")
    _elems(t_offsets, nreg + 1, 4, "t_offsets")
    if t_mask is not None:
        _elems(t_mask, n, 1, "t_mask")
    if t_area is not None:
        _elems(t_area, nreg, 4, "t_area")
    if t_pixels is not None:
        _elems(t_pixels, n, 4, "t_pixels")
    for t, what in lists:
        if t is not None:
            _elems(t, cap, 4, what)
    if cap > 0 and all(t is None for t, _ in lists):
        raise ValueError("a capacity without a list array")


def _opt(t):
    return _dptr(t) if t is not None else None


def region_windows_device(t_regions, width, height, num_regions, t_offsets, block=WINDOWS_BLOCK, expand=WINDOWS_EXPAND,
                          t_mask=None, t_area=None, min_area=0, capacity=0, t_coords=None, t_index=None,
                          t_pixels=None, t_colors=None, device=0, stream=None):
    """The capture windows of a device-resident width x height map of region
    ids (< num_regions each; contiguous, 4-byte elements).  t_mask: width *
    height bytes, nonzero = consumed, left out of every list; t_area
    (num_regions words) with min_area: a region with t_area[r] <= min_area has
    no window.  t_offsets gets num_regions + 1 words: t_offsets[r] = the length
    of the lists of the ids < r, the last one M.  Each of t_coords (x | y <<
    16), t_index (y * width + x) and t_colors (t_pixels there; needs
    t_pixels), `capacity` words, is filled when given and M <= capacity, and
    not touched when M > capacity.  Returns M: call without list arrays
    (capacity 0) for it, then with room.  Synchronous.  ValueError for bad
    tensors, shapes or scalars (nothing runs), RegionRowsError when the
    library refuses the map, WindowsOverflowError for M >= 2^32 - 1 (nothing
    is written)."""
    width, height, nreg = _pixels_shape(width, height, num_regions)
    block, expand, min_area, cap = _windows_scalars(block, expand, min_area, capacity)
    _windows_tensors(width * height, nreg, cap, t_regions, t_offsets, t_mask, t_area, t_pixels,
                     ((t_coords, "t_coords"), (t_index, "t_index"), (t_colors, "t_colors")))
    if t_colors is not None and t_pixels is None:
        raise ValueError("t_colors without t_pixels")
    r = lib().dq_hip_region_windows_dev(device, _dptr(t_regions), width, height, nreg, block, expand, _opt(t_mask),
                                        _opt(t_area), min_area, _dptr(t_offsets), cap, _opt(t_coords), _opt(t_index),
                                        _opt(t_pixels), _opt(t_colors), _stream_ptr(stream))
    return _windows_result(r, "dq_hip_region_windows_dev")


def _windows_host(regions2d, num_regions, block, expand, mask, area, min_area, pixels):
    """The host inputs of a windows call, checked: (reg, nreg, block, expand, mask, area, min_area, px)."""
    reg, nreg = _region_map(regions2d, num_regions)
    block, expand, min_area, _ = _windows_scalars(block, expand, min_area, 0)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.size != reg.size or mask.dtype.itemsize != 1:
            raise ValueError("mask: one byte per pixel")
        mask = np.ascontiguousarray(mask).view(np.uint8).reshape(-1)
    if area is not None:
        area = _u32(area).reshape(-1)
        if area.size < nreg:
            raise ValueError("%d areas for %d regions" % (area.size, nreg))
    px = None
    if pixels is not None:
        px = _u32(pixels).reshape(-1)
        if px.size != reg.size:
            raise ValueError("%d pixels for %d region ids" % (px.size, reg.size))
    return reg, nreg, block, expand, mask, area, min_area, px


def _optp(a):
    return _ptr(a) if a is not None else None


def region_windows(regions2d, num_regions=None, block=WINDOWS_BLOCK, expand=WINDOWS_EXPAND, mask=None, area=None,
                   min_area=0, pixels=None):
    """The capture windows of a host (H, W) map of region ids (integers of at
    most 4 bytes; num_regions=None takes regions2d.max() + 1); mask (H * W
    bytes), area with min_area and pixels (H * W words) as in
    region_windows_device.  Two calls: the count, then the lists with room.
    Returns (offsets, index, coords, colours), uint32: offsets (num_regions +
    1,), and per list entry the pixel's index y * W + x, its Coord word
    x | y << 16 and, with pixels, its frame word (None without)."""
    reg, nreg, block, expand, mask, area, min_area, px = _windows_host(regions2d, num_regions, block, expand, mask,
                                                                       area, min_area, pixels)
    h, w = reg.shape
    _require_gpu()
    offsets = np.zeros(nreg + 1, np.uint32)

    def call(cap, coords, index, colours):
        r = lib().dq_hip_region_windows(_ptr(reg), w, h, nreg, block, expand, _optp(mask), _optp(area), min_area,
                                        _ptr(offsets), cap, _optp(coords), _optp(index),
                                        _optp(px) if colours is not None else None, _optp(colours))
        return _windows_result(r, "dq_hip_region_windows")
    total = call(0, None, None, None)
    index, coords = np.zeros(total, np.uint32), np.zeros(total, np.uint32)
    colours = np.zeros(total, np.uint32) if px is not None else None
    if total:
        call(total, coords, index, colours)
    return offsets, index, coords, colours


def quant_region_windows_device(t_regions, width, height, num_regions, t_pixels, num_clusters, t_offsets,
                                block=WINDOWS_BLOCK, expand=WINDOWS_EXPAND, t_mask=None, t_area=None, min_area=0,
                                capacity=0, t_out=None, t_coords=None, t_index=None, t_colors=None, max_iters=10,
                                cts=None, k_outs=None, device=0, stream=None):
    """quant_recurse(N_window, .., K, allPixelsUnique=0) of every capture
    window of a device-resident region map: region_windows_device with the same
    arguments, then one call of the weighted-regions path in which region r's
    input is its window's colours in list order.  t_out (`capacity` words)
    gets the mapped colours in list order (windows overlap: there is no frame
    to paint).  Returns (cts, k_outs, empty): region r's colortable is
    cts[r, :k_outs[r]]; an empty window has k_outs[r] == 0 and its row of cts
    (zeros, or the array passed in) untouched.  The reference quantises a
    heuristic subset of the window (combinedCoords): that subset is not built
    here.  Synchronous.  ValueError for bad tensors, shapes or scalars (nothing
    runs); RegionRowsError, WindowsOverflowError as region_windows_device;
    WindowsCapacityError when t_out is given and the lists are longer than
    capacity (t_offsets is written, nothing is quantised)."""
    width, height, nreg = _pixels_shape(width, height, num_regions)
    block, expand, min_area, cap = _windows_scalars(block, expand, min_area, capacity)
    k, max_iters = _region_map_scalars(num_clusters, max_iters)
    if t_pixels is None:
        raise ValueError("the frame is needed")
    _windows_tensors(width * height, nreg, cap, t_regions, t_offsets, t_mask, t_area, t_pixels,
                     ((t_coords, "t_coords"), (t_index, "t_index"), (t_colors, "t_colors"), (t_out, "t_out")))
    cts, k_outs = _region_map_tables(nreg, k, cts, k_outs)
    r = lib().dq_hip_quant_region_windows_dev(device, _dptr(t_regions), width, height, nreg, block, expand,
                                              _opt(t_mask), _opt(t_area), min_area, _dptr(t_offsets), cap,
                                              _opt(t_coords), _opt(t_index), _dptr(t_pixels), _opt(t_colors), k,
                                              _opt(t_out), _ptr(cts), _ptr(k_outs), max_iters, _stream_ptr(stream))
    return cts, k_outs, _windows_result(r, "dq_hip_quant_region_windows_dev")


def quant_region_windows(regions2d, pixels, num_clusters, num_regions=None, block=WINDOWS_BLOCK,
                         expand=WINDOWS_EXPAND, mask=None, area=None, min_area=0, max_iters=10, mapped=True, cts=None,
                         k_outs=None):
    """quant_region_windows_device on a host (H, W) map of region ids and its
    frame (H * W packed 0x00RRGGBB words).  Returns (offsets, out, cts, k_outs,
    empty): out holds the mapped colours in list order (None with
    mapped=False, which also saves the counting call)."""
    if pixels is None:
        raise ValueError("the frame is needed")
    reg, nreg, block, expand, mask, area, min_area, px = _windows_host(regions2d, num_regions, block, expand, mask,
                                                                       area, min_area, pixels)
    h, w = reg.shape
    k, max_iters = _region_map_scalars(num_clusters, max_iters)
    cts, k_outs = _region_map_tables(nreg, k, cts, k_outs)
    _require_gpu()
    offsets = np.zeros(nreg + 1, np.uint32)
    total, out = 0, None
    if mapped:
        r = lib().dq_hip_region_windows(_ptr(reg), w, h, nreg, block, expand, _optp(mask), _optp(area), min_area,
                                        _ptr(offsets), 0, None, None, None, None)
        total = _windows_result(r, "dq_hip_region_windows")
        out = np.zeros(total, np.uint32)
    r = lib().dq_hip_quant_region_windows(_ptr(reg), w, h, nreg, block, expand, _optp(mask), _optp(area), min_area,
                                          _ptr(offsets), total, None, None, _ptr(px), None, k,
                                          _ptr(out) if total else None, _ptr(cts), _ptr(k_outs), max_iters)
    return offsets, out, cts, k_outs, _windows_result(r, "dq_hip_quant_region_windows")


# ---------------------------------------------------------------------------
# Window tags (include/dq_hip.h, "window tags"): per capture window which
# regions' pixels lie in it and how many each, in the order the ids first
# appear in the window's list; and per window and side (the region's own
# pixels, everything else) how many entries were mapped to each colortable
# entry.  Exact integers, independent of scheduling.
WINDOW_NO_ID = 0xFFFFFFFF               # best other / best vote: there is none
WINDOW_VOTES_MAX_CLUSTERS = 256


def _window_tags_result(r, name):
    if r == -3:   # (the call cannot say which of its three counts it was)
        raise WindowsOverflowError("%s: the lists hold 2^32 - 1 entries or more, or the windows as many pairs "
                                   "(block, member id), or the call as many contributions (pair, id alive in the "
                                   "block)" % name)
    return _windows_result(r, name)


def window_tags_device(t_regions, width, height, num_regions, t_rows, block=WINDOWS_BLOCK, expand=WINDOWS_EXPAND,
                       t_mask=None, t_area=None, min_area=0, capacity=0, t_ids=None, t_counts=None, t_first=None,
                       t_inside=None, t_best=None, t_best_count=None, t_offsets=None, device=0, stream=None):
    """The tag histogram of every capture window of a device-resident region
    map; t_regions .. min_area as in region_windows_device.  With c(r, s) = the
    entries of the list of r whose pixel has id s and f(r, s) = the first of
    them: t_rows gets num_regions + 1 CSR offsets, the last one E; entry
    t_rows[r] + i of t_ids, t_counts and t_first (`capacity` words each) is the
    i-th id s of row r, c(r, s) and f(r, s), in ascending f: filled when given
    and E <= capacity, not touched when E > capacity.  t_inside, t_best and
    t_best_count (num_regions words each) get c(r, r), the other id with the
    largest count (ties to the lowest id; WINDOW_NO_ID without one) and that
    count; t_offsets (num_regions + 1) the windows call's offsets.  Returns E:
    call without entry arrays (capacity 0) for it, then with room.
    Synchronous.  ValueError for bad tensors, shapes or scalars (nothing runs),
    RegionRowsError when the library refuses the map, WindowsOverflowError for
    2^32 - 1 list entries or contributions or more (nothing is written)."""
    width, height, nreg = _pixels_shape(width, height, num_regions)
    block, expand, min_area, cap = _windows_scalars(block, expand, min_area, capacity)
    _windows_tensors(width * height, nreg, cap, t_regions, t_rows, t_mask, t_area, None,
                     ((t_ids, "t_ids"), (t_counts, "t_counts"), (t_first, "t_first")))
    for t, what in ((t_inside, "t_inside"), (t_best, "t_best"), (t_best_count, "t_best_count")):
        if t is not None:
            _elems(t, nreg, 4, what)
    if t_offsets is not None:
        _elems(t_offsets, nreg + 1, 4, "t_offsets")
    r = lib().dq_hip_window_tags_dev(device, _dptr(t_regions), width, height, nreg, block, expand, _opt(t_mask),
                                     _opt(t_area), min_area, _dptr(t_rows), cap, _opt(t_ids), _opt(t_counts),
                                     _opt(t_first), _opt(t_inside), _opt(t_best), _opt(t_best_count), _opt(t_offsets),
                                     _stream_ptr(stream))
    return _window_tags_result(r, "dq_hip_window_tags_dev")


def window_tags(regions2d, num_regions=None, block=WINDOWS_BLOCK, expand=WINDOWS_EXPAND, mask=None, area=None,
                min_area=0):
    """window_tags_device on a host (H, W) map of region ids (as
    region_windows).  Two calls: the count, then the entries with room.
    Returns a dict of uint32 arrays: rows and offsets (num_regions + 1,), ids,
    counts and first (E,), inside, best and best_count (num_regions,)."""
    reg, nreg, block, expand, mask, area, min_area, _ = _windows_host(regions2d, num_regions, block, expand, mask,
                                                                      area, min_area, None)
    h, w = reg.shape
    _require_gpu()
    out = {k: np.zeros(nreg + 1, np.uint32) for k in ("rows", "offsets")}
    out.update({k: np.zeros(nreg, np.uint32) for k in ("inside", "best", "best_count")})

    def call(cap):
        r = lib().dq_hip_window_tags(_ptr(reg), w, h, nreg, block, expand, _optp(mask), _optp(area), min_area,
                                     _ptr(out["rows"]), cap, _optp(out.get("ids")), _optp(out.get("counts")),
                                     _optp(out.get("first")), _ptr(out["inside"]), _ptr(out["best"]),
                                     _ptr(out["best_count"]), _ptr(out["offsets"]))
        return _window_tags_result(r, "dq_hip_window_tags")
    entries = call(0)
    out.update({k: np.zeros(entries, np.uint32) for k in ("ids", "counts", "first")})
    if entries:
        call(entries)
    return out


def window_votes_device(t_regions, num_pixels, num_regions, t_offsets, t_index, total, t_mapped, cts, k_outs,
                        num_clusters, t_votes, t_best, device=0, stream=None):
    """The inside / outside votes of every window's quant: t_offsets, t_index
    and total as region_windows_device gave them, t_mapped (total words) the
    t_out of quant_region_windows_device, cts (num_regions, num_clusters) and
    k_outs (num_regions) the host arrays it returned.  For entry j of the list
    of r, mapped to the lowest entry i < k_outs[r] of r's colortable with its
    colour (low 24 bits): t_votes[(2 r + side) * num_clusters + i] += 1, side 0
    for a pixel of r itself and 1 for any other.  t_votes: num_regions * 2 *
    num_clusters words, all written; t_best: num_regions * 2 words, per side the
    lowest i with the largest non-zero count or WINDOW_NO_ID.  Returns the
    entries whose colour is not in their colortable (0 on the pipeline's own
    outputs).  Synchronous.  ValueError for bad tensors or scalars."""
    n, nreg, total, k = int(num_pixels), int(num_regions), int(total), int(num_clusters)
    if not 1 <= n <= PIXELS_MAX_PIXELS:
        raise ValueError("num_pixels %d: 1 .. 2^31 - 1" % n)
    if not 1 <= nreg <= PIXELS_MAX_REGIONS:
        raise ValueError("num_regions %d: 1 .. 2^31 - 1" % nreg)
    if not 0 <= total <= WINDOWS_MAX_ENTRIES:
        raise ValueError("total %d: 0 .. 2^32 - 2" % total)
    if not 1 <= k <= WINDOW_VOTES_MAX_CLUSTERS:
        raise ValueError("num_clusters %d: 1 .. 256" % k)
    _elems(t_regions, n, 4, "t_regions")
    _elems(t_offsets, nreg + 1, 4, "t_offsets")
    for t, what in ((t_index, "t_index"), (t_mapped, "t_mapped")):
        if t is not None or total > 0:
            _elems(t, total, 4, what)
    _elems(t_votes, nreg * 2 * k, 4, "t_votes")
    _elems(t_best, nreg * 2, 4, "t_best")
    if cts is None or k_outs is None:
        raise ValueError("cts and k_outs are needed")
    cts, k_outs = _region_map_tables(nreg, k, cts, k_outs)
    r = lib().dq_hip_window_votes_dev(device, _dptr(t_regions), n, nreg, _dptr(t_offsets), _opt(t_index), total,
                                      _opt(t_mapped), _ptr(cts), _ptr(k_outs), k, _dptr(t_votes), _dptr(t_best),
                                      _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_window_votes_dev: bad arguments")
    return int(r)


# ---------------------------------------------------------------------------
# Containment tree of a region map (include/dq_hip.h, "containment tree"):
# roots touch the image border, depth is the breadth-first distance from them
# over the edge list, the parent is the largest neighbour one level up (ties to
# the lowest id), siblings stand in size order and `order` is the post-order:
# the inside-out order to visit regions in.  Exact integers, independent of
# scheduling.
CONTAINMENT_NONE = 0xFFFFFFFF          # no parent (a root); depth, parent and pos of an orphan
CONTAINMENT_OUTPUTS = ("depth", "parent", "roots", "child_offsets", "children", "subtree", "enclosed", "order", "pos")


def _containment_shape(width, height, num_regions):
    width, height, nreg = int(width), int(height), int(num_regions)
    if not (1 <= width <= REGION_MAX_SIDE and 1 <= height <= REGION_MAX_SIDE):
        raise ValueError("a %d x %d map: sides are 1..65535" % (width, height))
    if not 1 <= nreg <= width * height:
        raise ValueError("num_regions %d for %d pixels" % (nreg, width * height))
    return width, height, nreg


def _containment_outputs(outputs):
    want = tuple(CONTAINMENT_OUTPUTS if outputs is None else outputs)
    for name in want:
        if name not in CONTAINMENT_OUTPUTS:
            raise ValueError("no output %r: %s" % (name, ", ".join(CONTAINMENT_OUTPUTS)))
    if "children" in want and "child_offsets" not in want:
        raise ValueError("children come with child_offsets")
    return want


def _edge_count(t_edges, num_edges):
    if num_edges is None:
        if t_edges is not None:
            _elems(t_edges, 0, 4, "t_edges")
        num_edges = 0 if t_edges is None else (t_edges.size if isinstance(t_edges, np.ndarray) else t_edges.numel()) // 2
    nedges = _scalar32(num_edges, "num_edges")
    if nedges:
        if t_edges is None:
            raise ValueError("%d edges without t_edges" % nedges)
        _elems(t_edges, 2 * nedges, 4, "t_edges")
    return nedges


def region_containment_device(t_regions, width, height, num_regions, t_area, t_edges, num_edges=None, outputs=None,
                              device=0, stream=None):
    """The containment tree of a device-resident width x height map of region
    ids < num_regions (contiguous, 4-byte elements).  t_area: num_regions
    words; t_edges: num_edges x 2 ids as region_adjacency_device gives them
    (num_edges defaults to its length / 2; None with no edge).  outputs: the
    names wanted of CONTAINMENT_OUTPUTS (None: all).  Returns (nroots, levels,
    reached, out): out a dict of device tensors -- "depth", "parent",
    "subtree", "pos" (num_regions,; int32 storage of the uint32 values),
    "enclosed" (num_regions,; int64), "roots" (nroots,), "child_offsets"
    (num_regions + 1,), "children" (reached - nroots,) and "order" (reached,).
    Synchronous.  ValueError for bad tensors, lengths or names (nothing runs)."""
    width, height, nreg = _containment_shape(width, height, num_regions)
    n = width * height
    _elems(t_regions, n, 4, "t_regions")
    _elems(t_area, nreg, 4, "t_area")
    nedges = _edge_count(t_edges, num_edges)
    want = _containment_outputs(outputs)
    import torch
    dev = f"cuda:{device}"
    out = {name: torch.empty(nreg + (name == "child_offsets"), dtype=torch.int64 if name == "enclosed" else torch.int32,
                             device=dev) for name in want}
    opt = lambda name: _dptr(out[name]) if name in out else None  # noqa: E731
    levels, reached = ctypes.c_uint32(0), ctypes.c_uint32(0)
    r = lib().dq_hip_region_containment_dev(device, _dptr(t_regions), width, height, nreg, _dptr(t_area), nedges,
                                            _dptr(t_edges) if nedges else None, opt("depth"), opt("parent"),
                                            opt("roots"), opt("child_offsets"), opt("children"), opt("subtree"),
                                            opt("enclosed"), opt("order"), opt("pos"), ctypes.byref(levels),
                                            ctypes.byref(reached), _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_region_containment_dev: bad arguments")
    used = {"roots": int(r), "children": reached.value - int(r), "order": reached.value}
    return int(r), int(levels.value), int(reached.value), {k: v[:used.get(k, v.numel())] for k, v in out.items()}


def region_containment(regions2d, area, edges, num_regions=None):
    """The containment tree of a host (H, W) map of region ids (integers of at
    most 4 bytes), its areas (num_regions; None takes regions2d.max() + 1) and
    its edge list ((E, 2) ids, or None).  Returns a dict of numpy arrays:
    "depth", "parent", "subtree", "pos" (R,) uint32, "enclosed" (R,) uint64,
    "roots" (nroots,), "child_offsets" (R + 1,), "children" (reached - nroots,),
    "order" (reached,), and the ints "levels" and "reached"."""
    reg = np.asarray(regions2d)
    if reg.ndim != 2 or reg.size == 0:
        raise ValueError("regions2d must be a non-empty (H, W) array")
    if reg.dtype.kind not in "ui" or reg.dtype.itemsize > 4:
        raise ValueError("region ids are integers of at most 4 bytes, not %s" % reg.dtype)
    if reg.dtype.kind == "i" and reg.min() < 0:
        raise ValueError("region ids are not negative")
    reg = _u32(reg)
    top = int(reg.max())
    nreg = top + 1 if num_regions is None else int(num_regions)
    if not top < nreg:
        raise ValueError("num_regions %d for ids up to %d" % (nreg, top))
    h, w = reg.shape
    _containment_shape(w, h, nreg)
    if area is None:
        raise ValueError("the areas are needed: they order parents and siblings")
    ar = _u32(area).reshape(-1)
    if ar.size != nreg:
        raise ValueError("%d areas for %d regions" % (ar.size, nreg))
    ed = np.zeros((0, 2), np.uint32) if edges is None else _u32(edges)
    if ed.size % 2 or (ed.size and ed.ndim != 2):
        raise ValueError("edges are (E, 2) ids")
    nedges = _scalar32(ed.size // 2, "the edge count")
    if nedges and (int(ed.max()) >= nreg or bool((ed[:, 0] == ed[:, 1]).any())):
        raise ValueError("an edge joins two different ids below num_regions")
    _require_gpu()
    out = {name: np.zeros(nreg + (name == "child_offsets"), np.uint64 if name == "enclosed" else np.uint32)
           for name in CONTAINMENT_OUTPUTS}
    levels, reached = ctypes.c_uint32(0), ctypes.c_uint32(0)
    r = lib().dq_hip_region_containment(_ptr(reg), w, h, nreg, _ptr(ar), nedges, _ptr(ed) if nedges else None,
                                        *[_ptr(out[name]) for name in CONTAINMENT_OUTPUTS], ctypes.byref(levels),
                                        ctypes.byref(reached))
    if r < 0:
        raise DivQuantError("dq_hip_region_containment: bad arguments")
    used = {"roots": int(r), "children": reached.value - int(r), "order": reached.value}
    out = {k: v[:used.get(k, v.size)].copy() for k, v in out.items()}
    out["levels"], out["reached"] = int(levels.value), int(reached.value)
    return out


def regions_by_size_device(t_area, num_regions=None, want_order=True, want_rank=True, device=0, stream=None):
    """The size order of num_regions areas on the device (t_area: contiguous,
    4-byte elements; num_regions defaults to its length): area decreasing, ties
    by id increasing.  Returns (order, rank), device tensors of num_regions
    words (int32 storage of the uint32 values): order[i] the id at position i,
    rank[id] its position; None for the one not wanted.  Synchronous.
    ValueError for bad tensors or lengths (nothing runs)."""
    _elems(t_area, 0, 4, "t_area")
    if num_regions is None:
        num_regions = t_area.size if isinstance(t_area, np.ndarray) else t_area.numel()
    nreg = _scalar32(num_regions, "num_regions")
    if nreg < 1:
        raise ValueError("num_regions is at least 1")
    _elems(t_area, nreg, 4, "t_area")
    if not (want_order or want_rank):
        raise ValueError("neither the order nor the rank is wanted")
    import torch
    dev = f"cuda:{device}"
    order = torch.empty(nreg, dtype=torch.int32, device=dev) if want_order else None
    rank = torch.empty(nreg, dtype=torch.int32, device=dev) if want_rank else None
    r = lib().dq_hip_regions_by_size_dev(device, nreg, _dptr(t_area), _dptr(order) if want_order else None,
                                         _dptr(rank) if want_rank else None, _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_regions_by_size_dev: bad arguments")
    return order, rank


# ---------------------------------------------------------------------------
# Distance transform, centres and cores of a region map (include/dq_hip.h,
# "region distance"): D(p) the L1 distance to the nearest pixel of another id or
# position outside the frame, per region dmax, bbox, the threshold (rule 0: dmax;
# rule 1: the reference's 8-bit scale), the centre set's size and the centre;
# the core of a region is its component that holds the centre.  Exact integers,
# independent of scheduling.  An id >= num_regions is background.
DISTANCE_NONE = 0xFFFFFFFF             # the centre of an id with no pixel; d_cored off the cores
DISTANCE_OUTPUTS = ("dist", "dmax", "bbox", "thresh", "count", "centre")
CORES_OUTPUTS = ("core", "cored", "centre", "core_area", "dist")


def _distance_shape(width, height, num_regions, rule, connectivity=8):
    width, height = _region_shape(width, height, connectivity)
    nreg = int(num_regions)
    if not 1 <= nreg <= 0xFFFFFFFF:
        raise ValueError("num_regions %d: at least 1, a uint32" % nreg)
    if rule not in (0, 1):
        raise ValueError("rule is 0 (exact) or 1 (the 8-bit scale), not %r" % (rule,))
    return width, height, nreg


def _distance_outputs(outputs, names):
    want = tuple(names if outputs is None else outputs)
    for name in want:
        if name not in names:
            raise ValueError("no output %r: %s" % (name, ", ".join(names)))
    if not want:
        raise ValueError("no output is wanted")
    return want


def _distance_map(regions2d, num_regions):
    """A host (H, W) map of ids as contiguous uint32, and its region count (ids at or above it: background)."""
    reg = np.asarray(regions2d)
    if reg.ndim != 2 or reg.size == 0:
        raise ValueError("regions2d must be a non-empty (H, W) array")
    if reg.dtype.kind not in "ui" or reg.dtype.itemsize > 4:
        raise ValueError("region ids are integers of at most 4 bytes, not %s" % reg.dtype)
    if reg.dtype.kind == "i" and reg.min() < 0:
        raise ValueError("region ids are not negative")
    reg = _u32(reg)
    return reg, int(reg.max()) + 1 if num_regions is None else int(num_regions)


def _distance_shapes(w, h, nreg):
    """name -> (shape, numpy dtype, torch dtype name) of every output of the two calls."""
    return {"dist": ((h, w), np.uint16, "int16"), "dmax": ((nreg,), np.uint32, "int32"),
            "bbox": ((nreg, 4), np.uint32, "int32"), "thresh": ((nreg,), np.uint32, "int32"),
            "count": ((nreg,), np.uint32, "int32"), "centre": ((nreg,), np.uint32, "int32"),
            "core": ((h, w), np.uint8, "uint8"), "cored": ((h, w), np.uint32, "int32"),
            "core_area": ((nreg,), np.uint32, "int32")}


def _distance_tensors(want, w, h, nreg, device):
    import torch
    shapes = _distance_shapes(w, h, nreg)
    return {name: torch.empty(shapes[name][0], dtype=getattr(torch, shapes[name][2]), device=f"cuda:{device}")
            for name in want}


def region_distance_device(t_regions, width, height, num_regions, rule=0, outputs=None, device=0, stream=None):
    """The L1 distance transform and the centres of a device-resident width x
    height map of region ids (contiguous, 4-byte elements; an id >= num_regions
    is background).  outputs: the names wanted of DISTANCE_OUTPUTS (None: all).
    Returns a dict of device tensors: "dist" (height, width) int16 storage of
    the uint16 values, "dmax", "thresh", "count", "centre" (num_regions,) and
    "bbox" (num_regions, 4), int32 storage of the uint32 values.  Synchronous.
    ValueError for bad tensors, sizes or names (nothing runs)."""
    width, height, nreg = _distance_shape(width, height, num_regions, rule)
    _elems(t_regions, width * height, 4, "t_regions")
    want = _distance_outputs(outputs, DISTANCE_OUTPUTS)
    out = _distance_tensors(want, width, height, nreg, device)
    opt = lambda name: _dptr(out[name]) if name in out else None  # noqa: E731
    r = lib().dq_hip_region_distance_dev(device, _dptr(t_regions), width, height, nreg, rule,
                                         *[opt(name) for name in DISTANCE_OUTPUTS], _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_region_distance_dev: bad arguments")
    return out


def region_distance(regions2d, num_regions=None, rule=0):
    """The same of a host (H, W) map of ids (integers of at most 4 bytes;
    num_regions None takes regions2d.max() + 1).  Returns a dict of numpy
    arrays: "dist" (H, W) uint16, "dmax", "thresh", "count", "centre" (R,)
    uint32 and "bbox" (R, 4) uint32."""
    reg, nreg = _distance_map(regions2d, num_regions)
    h, w = reg.shape
    _distance_shape(w, h, nreg, rule)
    _require_gpu()
    shapes = _distance_shapes(w, h, nreg)
    out = {name: np.zeros(shapes[name][0], shapes[name][1]) for name in DISTANCE_OUTPUTS}
    r = lib().dq_hip_region_distance(_ptr(reg), w, h, nreg, rule, *[_ptr(out[name]) for name in DISTANCE_OUTPUTS])
    if r < 0:
        raise DivQuantError("dq_hip_region_distance: bad arguments")
    return out


def region_cores_device(t_regions, width, height, num_regions, rule=0, connectivity=8, outputs=None, t_cored=None,
                        device=0, stream=None):
    """The cores of a device-resident map: per region the component (equal ids
    under `connectivity`) that holds its centre.  outputs: the names wanted of
    CORES_OUTPUTS (None: all).  t_cored: where "cored" goes instead of a new
    tensor; it may be t_regions itself (in place).  Returns (kept, out): the
    pixels kept and a dict of device tensors -- "core" (height, width) uint8,
    "cored" (height, width) the id or 0xFFFFFFFF, "centre", "core_area"
    (num_regions,), "dist" (height, width) int16 storage.  Synchronous.
    ValueError for bad tensors, sizes or names (nothing runs)."""
    width, height, nreg = _distance_shape(width, height, num_regions, rule, connectivity)
    _elems(t_regions, width * height, 4, "t_regions")
    want = _distance_outputs(outputs, CORES_OUTPUTS)
    if t_cored is not None:
        _elems(t_cored, width * height, 4, "t_cored")
        if "cored" not in want:
            raise ValueError("t_cored without the output \"cored\"")
    out = _distance_tensors([name for name in want if not (name == "cored" and t_cored is not None)], width, height,
                            nreg, device)
    if t_cored is not None:
        out["cored"] = t_cored
    opt = lambda name: _dptr(out[name]) if name in out else None  # noqa: E731
    r = lib().dq_hip_region_cores_dev(device, _dptr(t_regions), width, height, nreg, rule, connectivity,
                                      *[opt(name) for name in CORES_OUTPUTS], _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_region_cores_dev: bad arguments")
    return int(r), out


def region_cores(regions2d, num_regions=None, rule=0, connectivity=8):
    """The same of a host (H, W) map of ids.  Returns a dict of numpy arrays
    ("core" uint8, "cored" uint32, "dist" uint16: (H, W); "centre", "core_area":
    (R,) uint32) and the int "kept"."""
    reg, nreg = _distance_map(regions2d, num_regions)
    h, w = reg.shape
    _distance_shape(w, h, nreg, rule, connectivity)
    _require_gpu()
    shapes = _distance_shapes(w, h, nreg)
    out = {name: np.zeros(shapes[name][0], shapes[name][1]) for name in CORES_OUTPUTS}
    r = lib().dq_hip_region_cores(_ptr(reg), w, h, nreg, rule, connectivity, *[_ptr(out[name]) for name in CORES_OUTPUTS])
    if r < 0:
        raise DivQuantError("dq_hip_region_cores: bad arguments")
    out["kept"] = int(r)
    return out


# ---------------------------------------------------------------------------
# Skeletons of all regions of a region map (include/dq_hip.h, "region
# skeleton"): Guo-Hall two-subiteration thinning, a pixel's neighbour counting
# only when it has the pixel's own id, so every region thins as its own mask
# would alone (the reference's skelReduce).  Exact bits, independent of
# scheduling.  An id >= num_regions is background.
SKELETON_OUTPUTS = ("skel", "skeled", "when", "skel_area", "thick")
SKELETON_MAX_ITERS = 65535


def _skeleton_shape(width, height, num_regions, max_iters):
    width, height, nreg = _distance_shape(width, height, num_regions, 0)
    max_iters = int(max_iters)
    if not 0 <= max_iters <= SKELETON_MAX_ITERS:
        raise ValueError("max_iters %d: 0 (until stable) .. %d" % (max_iters, SKELETON_MAX_ITERS))
    return width, height, nreg, max_iters


def _skeleton_shapes(w, h, nreg):
    """name -> (shape, numpy dtype, torch dtype name) of every output of the call."""
    return {"skel": ((h, w), np.uint8, "uint8"), "skeled": ((h, w), np.uint32, "int32"),
            "when": ((h, w), np.uint16, "int16"), "skel_area": ((nreg,), np.uint32, "int32"),
            "thick": ((nreg,), np.uint32, "int32")}


def region_skeleton_device(t_regions, width, height, num_regions, max_iters=0, outputs=None, t_skeled=None, device=0,
                           stream=None):
    """The skeletons of all regions of a device-resident width x height map of
    region ids (contiguous, 4-byte elements; an id >= num_regions is
    background).  max_iters: 0 runs until nothing is deleted.  outputs: the names
    wanted of SKELETON_OUTPUTS (None: all).  t_skeled: where "skeled" goes instead
    of a new tensor; it may be t_regions itself (in place).  Returns (kept, out):
    the pixels kept and a dict of device tensors -- "skel" (height, width) uint8,
    "skeled" (height, width) the id or 0xFFFFFFFF, "when" (height, width) int16
    storage of the uint16 iteration that deleted the pixel, "skel_area", "thick"
    (num_regions,) -- and the ints "iterations" (the last iteration that deleted a
    pixel) and "converged".  Synchronous.  ValueError for bad tensors, sizes or
    names (nothing runs)."""
    width, height, nreg, max_iters = _skeleton_shape(width, height, num_regions, max_iters)
    _elems(t_regions, width * height, 4, "t_regions")
    want = _distance_outputs(outputs, SKELETON_OUTPUTS)
    if t_skeled is not None:
        _elems(t_skeled, width * height, 4, "t_skeled")
        if "skeled" not in want:
            raise ValueError("t_skeled without the output \"skeled\"")
    import torch
    shapes = _skeleton_shapes(width, height, nreg)
    out = {name: torch.empty(shapes[name][0], dtype=getattr(torch, shapes[name][2]), device=f"cuda:{device}")
           for name in want if not (name == "skeled" and t_skeled is not None)}
    if t_skeled is not None:
        out["skeled"] = t_skeled
    opt = lambda name: _dptr(out[name]) if name in out else None  # noqa: E731
    iterations, converged = ctypes.c_uint32(0), ctypes.c_uint32(0)
    r = lib().dq_hip_region_skeleton_dev(device, _dptr(t_regions), width, height, nreg, max_iters,
                                         *[opt(name) for name in SKELETON_OUTPUTS], ctypes.byref(iterations),
                                         ctypes.byref(converged), _stream_ptr(stream))
    if r < 0:
        raise DivQuantError("dq_hip_region_skeleton_dev: bad arguments")
    out["iterations"], out["converged"] = int(iterations.value), int(converged.value)
    return int(r), out


def region_skeleton(regions2d, num_regions=None, max_iters=0):
    """The same of a host (H, W) map of ids (integers of at most 4 bytes;
    num_regions None takes regions2d.max() + 1).  Returns a dict of numpy arrays
    ("skel" uint8, "skeled" uint32, "when" uint16: (H, W); "skel_area", "thick":
    (R,) uint32) and the ints "kept", "iterations" and "converged"."""
    reg, nreg = _distance_map(regions2d, num_regions)
    h, w = reg.shape
    _, _, nreg, max_iters = _skeleton_shape(w, h, nreg, max_iters)
    _require_gpu()
    shapes = _skeleton_shapes(w, h, nreg)
    out = {name: np.zeros(shapes[name][0], shapes[name][1]) for name in SKELETON_OUTPUTS}
    iterations, converged = ctypes.c_uint32(0), ctypes.c_uint32(0)
    r = lib().dq_hip_region_skeleton(_ptr(reg), w, h, nreg, max_iters, *[_ptr(out[name]) for name in SKELETON_OUTPUTS],
                                     ctypes.byref(iterations), ctypes.byref(converged))
    if r < 0:
        raise DivQuantError("dq_hip_region_skeleton: bad arguments")
    out["kept"], out["iterations"], out["converged"] = int(r), int(iterations.value), int(converged.value)
    return out


# ---------------------------------------------------------------------------
# Contours of all regions of a region map (include/dq_hip.h, "region
# contours"): OpenCV's border following of the outer border of the component
# that holds a region's first pixel, a neighbour counting only when it has the
# pixel's own id (the reference's findContourOutline on every region's mask).
# Exact integers, independent of scheduling.  An id >= num_regions is background.
CONTOUR_OUTPUTS = ("offsets", "points", "codes", "len", "visits")
CONTOUR_LISTS = ("points", "codes")
CONTOUR_MAX_REGIONS = 0xFFFFFFFF - 1024
CONTOUR_NO_CODE = 8                    # the code of the one point of a contour of length 1


class ContourOverflowError(DivQuantError):
    """The contours of the map have 2^32 - 1 points or more (-2), or its border pixels more than
    2^32 - 2 neighbours of their own id (-3)."""


def _contour_shape(width, height, num_regions, orientation, point_capacity=None):
    width, height, nreg = _distance_shape(width, height, num_regions, 0)
    if nreg > CONTOUR_MAX_REGIONS:
        raise ValueError("num_regions %d: at most 2^32 - 1025" % nreg)
    if orientation not in (0, 1):
        raise ValueError("orientation is 0 (as followed) or 1 (reversed), not %r" % (orientation,))
    if point_capacity is not None:
        point_capacity = int(point_capacity)
        if not 0 <= point_capacity <= 0xFFFFFFFFFFFFFFFF:
            raise ValueError("point_capacity %d is not a uint64" % point_capacity)
    return width, height, nreg, point_capacity


def _contour_shapes(w, h, nreg, cap):
    """name -> (shape, numpy dtype, torch dtype name) of every output of the call."""
    return {"offsets": ((nreg + 1,), np.uint32, "int32"), "points": ((cap,), np.uint32, "int32"),
            "codes": ((cap,), np.uint8, "uint8"), "len": ((nreg,), np.uint32, "int32"),
            "visits": ((h, w), np.uint8, "uint8")}


def _contour_result(r, name):
    if r in (-2, -3):
        raise ContourOverflowError("%s: the contours do not fit 32-bit offsets (%d)" % (name, r))
    if r < 0:
        raise DivQuantError("%s: bad arguments" % name)
    return int(r)


def region_contours_device(t_regions, width, height, num_regions, orientation=0, outputs=None, point_capacity=None,
                           device=0, stream=None):
    """The contours of all regions of a device-resident width x height map of
    region ids (contiguous, 4-byte elements; an id >= num_regions is
    background).  orientation: 0 the points as border following emits them
    (counter-clockwise on the screen, from the region's first pixel), 1 the
    reference's reversed list.  outputs: the names wanted of CONTOUR_OUTPUTS
    (None: all).  point_capacity: the entries of room in "points" and "codes";
    None counts first and sizes them to M (two calls when a list is wanted).
    Returns (M, out): the points of all contours and a dict of device tensors --
    "offsets" (num_regions + 1,) and "len" (num_regions,) int32 storage of the
    uint32 values, "points" Coord words x | y << 16 and "codes" uint8 (written
    only when M <= their length), "visits" (height, width) uint8.  Synchronous.
    ValueError for bad tensors, sizes or names (nothing runs)."""
    width, height, nreg, cap = _contour_shape(width, height, num_regions, orientation, point_capacity)
    _elems(t_regions, width * height, 4, "t_regions")
    want = _distance_outputs(outputs, CONTOUR_OUTPUTS)
    lists = [name for name in CONTOUR_LISTS if name in want]
    if cap is not None and cap > 0 and not lists:
        raise ValueError("point_capacity without the output \"points\" or \"codes\"")
    import torch
    fn, reg = lib().dq_hip_region_contours_dev, _dptr(t_regions)
    if lists and cap is None:   # count, then fill
        t_len = torch.empty(nreg, dtype=torch.int32, device=f"cuda:{device}")
        cap = _contour_result(fn(device, reg, width, height, nreg, orientation, 0, None, None, None, _dptr(t_len), None,
                                 _stream_ptr(stream)), "dq_hip_region_contours_dev")
    shapes = _contour_shapes(width, height, nreg, cap or 0)
    out = {name: torch.empty(shapes[name][0], dtype=getattr(torch, shapes[name][2]), device=f"cuda:{device}")
           for name in want}
    opt = lambda name: _dptr(out[name]) if name in out and out[name].numel() else None  # noqa: E731
    r = fn(device, reg, width, height, nreg, orientation, cap if lists else 0, *[opt(name) for name in CONTOUR_OUTPUTS],
           _stream_ptr(stream))
    return _contour_result(r, "dq_hip_region_contours_dev"), out


def region_contours(regions2d, num_regions=None, orientation=0):
    """The same of a host (H, W) map of ids (integers of at most 4 bytes;
    num_regions None takes regions2d.max() + 1).  Returns a dict of numpy arrays
    ("offsets" (R + 1,), "len" (R,), "points" (M,) uint32; "codes" (M,) uint8;
    "visits" (H, W) uint8) and the int "total" (M)."""
    reg, nreg = _distance_map(regions2d, num_regions)
    h, w = reg.shape
    _contour_shape(w, h, nreg, orientation)
    _require_gpu()
    fn = lib().dq_hip_region_contours
    count = np.zeros(nreg, np.uint32)
    total = _contour_result(fn(_ptr(reg), w, h, nreg, orientation, 0, None, None, None, _ptr(count), None),
                            "dq_hip_region_contours")
    shapes = _contour_shapes(w, h, nreg, total)
    out = {name: np.zeros(shapes[name][0], shapes[name][1]) for name in CONTOUR_OUTPUTS}
    opt = lambda name: _ptr(out[name]) if out[name].size else None  # noqa: E731
    r = fn(_ptr(reg), w, h, nreg, orientation, total, *[opt(name) for name in CONTOUR_OUTPUTS])
    out["total"] = _contour_result(r, "dq_hip_region_contours")
    return out


# ---------------------------------------------------------------------------
# BGR24 frames.  `t_bgr`: uint8 device tensor (or pointer)
# holding a CV_8UC3 frame, `stride` bytes per row (default 3 * width).
def pack_bgr24_device(t_bgr, width, height, t_out, stride=None, device=0, stream=None):
    """t_out[y*width+x] = Vec3BToUID(img(y, x)) (OpenCVUtil.h:19-27), asynchronous."""
    stride = 3 * width if stride is None else stride
    if lib().dq_hip_pack_bgr24_dev(device, _dptr(t_bgr), width, height, stride, _dptr(t_out),
                                   _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_pack_bgr24_dev: bad arguments")


def unpack_bgr24_device(t_in, width, height, t_bgr, stride=None, device=0, stream=None):
    """img(y, x) = PixelToVec3b(t_in[y*width+x]) (OpenCVUtil.h:53-59), asynchronous."""
    stride = 3 * width if stride is None else stride
    if lib().dq_hip_unpack_bgr24_dev(device, _dptr(t_in), width, height, stride, _dptr(t_bgr),
                                     _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_unpack_bgr24_dev: bad arguments")


def gather_bgr24_device(t_bgr, stride, t_coords, n, t_out, device=0, stream=None):
    """t_out[i] = Vec3BToUID(img(c.y, c.x)) for Coord words c = x | y << 16
    (Coord.h:30-33; ClusteringSegmentation.cpp:1795-1800), asynchronous."""
    if lib().dq_hip_gather_bgr24_dev(device, _dptr(t_bgr), stride, _dptr(t_coords), n,
                                     _dptr(t_out), _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_gather_bgr24_dev: bad arguments")


# ---------------------------------------------------------------------------
# Synthetic benchmark frames and the fixtures' output checksum (host code).
SYNTH_SEED = 0x9E3779B97F4A7C15


def synth_frame(n, frame=0, seed=SYNTH_SEED):
    """Frame `frame` of the benchmark batch: n xorshift64 draws
    & 0xFFFFFF from seed + frame."""
    out = np.empty(n, np.uint32)
    lib().dq_synth_xorshift(_ptr(out), n, (seed + frame) & 0xFFFFFFFFFFFFFFFF)
    return out


def fnv1a64(a):
    """Word-wise FNV-1a-64 of a uint32 array (the golden fixtures' out_fnv)."""
    a = _u32(a).reshape(-1)
    return int(lib().dq_fnv1a64(_ptr(a), a.size))


# ---------------------------------------------------------------------------
# Full-frame fixed-palette map + per-block mode.
def get_subdivided_colors():
    """getSubdividedColors (superpixels/OpenCVUtil.cpp:853-897): the 125
    colours 0xFFRRGGBB of the {0,63,127,191,255}^3 cube (no GPU needed)."""
    out = np.zeros(125, np.uint32)
    lib().dq_subdivided_colors(_ptr(out))
    return out


def block_grid(width, height, superpixel_dim=4):
    """(blockWidth, blockHeight) as clusteringCombine computes them
    (ClusteringSegmentationMain.cpp:138-149): ceil(W/dim), ceil(H/dim)."""
    return -(-width // superpixel_dim), -(-height // superpixel_dim)


def gen_histograms_for_blocks(frame, superpixel_dim=4, palette=None, tables=False):
    """genHistogramsForBlocks (ClusteringSegmentation.cpp:365-576) on a frame of
    0x00RRGGBB words shaped (H, W) (the Vec3BToUID packing of the BGR Mat).

    Returns (block_bgr, region_quant_pixel, quant[, (ndistinct, keys, counts)]):
    block_bgr (bh, bw, 3) uint8 is the returned blockMat (B, G, R bytes);
    region_quant_pixel (bh, bw) uint32 is each block's HistogramForBlock::
    regionQuantPixel; quant (H, W) the map_colors_mps output.  With tables=True
    also each block's pixelToCountTable in iteration order: ndistinct (bh, bw)
    and keys/counts (bh, bw, dim*dim), zero past ndistinct."""
    _require_gpu()
    fr = _u32(frame)
    if fr.ndim != 2 or fr.size == 0:
        raise DivQuantError("frame must be a non-empty (H, W) array")
    h, w = fr.shape
    bw, bh = block_grid(w, h, superpixel_dim)
    pal = get_subdivided_colors() if palette is None else _u32(palette).reshape(-1)
    quant = np.zeros((h, w), np.uint32)
    mode = np.zeros((bh, bw), np.uint32)
    cap = superpixel_dim * superpixel_dim
    nd = np.zeros((bh, bw), np.uint32) if tables else None
    keys = np.zeros((bh, bw, cap), np.uint32) if tables else None
    counts = np.zeros((bh, bw, cap), np.uint32) if tables else None
    none = ctypes.c_void_p(0)
    rc = lib().dq_hip_block_hist(_ptr(fr), w, h, _ptr(pal), pal.size, superpixel_dim, bw, bh,
                                 _ptr(quant), _ptr(mode), _ptr(nd) if tables else none,
                                 _ptr(keys) if tables else none, _ptr(counts) if tables else none)
    if rc < 0:
        raise DivQuantError("dq_hip_block_hist: bad arguments")
    bgr = np.stack([mode & 0xFF, (mode >> 8) & 0xFF, (mode >> 16) & 0xFF], axis=-1).astype(np.uint8)
    if tables:
        return bgr, mode, quant, (nd, keys, counts)
    return bgr, mode, quant


def block_hist_device(t_in, width, height, t_quant, t_mode, palette=None, superpixel_dim=4,
                      t_ndistinct=None, t_keys=None, t_counts=None, device=0, stream=None):
    """dq_hip_block_hist_dev on torch tensors / device pointers (asynchronous)."""
    pal = get_subdivided_colors() if palette is None else _u32(palette).reshape(-1)
    bw, bh = block_grid(width, height, superpixel_dim)
    opt = lambda t: _dptr(t) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    if lib().dq_hip_block_hist_dev(device, _dptr(t_in), width, height, _ptr(pal), pal.size,
                                   superpixel_dim, bw, bh, _dptr(t_quant), _dptr(t_mode),
                                   opt(t_ndistinct), opt(t_keys), opt(t_counts),
                                   _stream_ptr(stream)) < 0:
        raise DivQuantError("dq_hip_block_hist_dev: bad arguments")


def last_centroids(k, device=0):
    """(means[k,3] float64, sizes[k] int64) of the last clustering on `device`."""
    means = np.zeros((k, 3), np.float64)
    sizes = np.zeros(k, np.int64)
    if lib().dq_hip_last_centroids(device, _ptr(means), _ptr(sizes), k) < 0:
        raise DivQuantError("k does not match the last clustering")
    return means, sizes


def last_trace(k, device=0):
    tr = np.zeros((max(k - 1, 0), 4), np.int64)
    if lib().dq_hip_last_trace(device, _ptr(tr) if tr.size else None, k) < 0:
        raise DivQuantError("k does not match the last clustering")
    return tr


def last_rounds(device=0):
    return lib().dq_hip_last_rounds(device)


def last_points_swept(device=0):
    return int(lib().dq_hip_last_points_swept(device))


def last_points_full(device=0):
    """Points the last run would have swept with all max_iters iterations."""
    return int(lib().dq_hip_last_points_full(device))


def last_seq_tiles(device=0):
    """Weighted path: tiles of the last run folded one summand at a time."""
    return int(lib().dq_hip_last_seq_tiles(device))


def last_cursor_fixes(device=0):
    """Records of the last run partitioned after a frame's last planned round
    (PS_STATS: no cursors counted there) whose cursors were counted then."""
    return int(lib().dq_hip_last_cursor_fixes(device))


def set_fixed_point(on, device=0):
    """Fixed-point finalisation of 2-means splits (identical outputs)."""
    lib().dq_hip_set_fixed_point(device, 1 if on else 0)


def set_planned_rounds(on, device=0):
    """Device-planned (speculative) rounds (identical outputs)."""
    lib().dq_hip_set_planned_rounds(device, 1 if on else 0)


def last_planned_rounds(device=0):
    return lib().dq_hip_last_planned_rounds(device)


def set_loop_max(max_points, device=0):
    """kloop_kernel eligibility: records of at most max_points points (0: off)."""
    lib().dq_hip_set_loop_max(device, int(max_points))


def last_loop_rounds(device=0):
    return lib().dq_hip_last_loop_rounds(device)


def set_persist(on, device=0):
    """kpersist_kernel rounds on / off (every lane of the device)."""
    lib().dq_hip_set_persist(device, 1 if on else 0)


def set_wsmall(on, device=0):
    """The one-launch weighted path for small inputs on / off (every lane)."""
    lib().dq_hip_set_wsmall(device, 1 if on else 0)


def set_lds_map(on, device=0):
    """map_lds_kernel for palettes of at most 1024 entries on / off (every
    lane); off: map_kernel, as for larger palettes (identical outputs)."""
    lib().dq_hip_set_lds_map(device, 1 if on else 0)


def last_wsmall_profile(device=0):
    """The last weighted call's one-launch phase profile in microseconds
    (hash set, colour table, clustering, map, of which fold passes and
    partitions) and its passes by kind; {} if it did not take that path."""
    buf = np.zeros(8, np.uint64)
    if lib().dq_hip_last_wsmall_profile(device, buf.ctypes.data_as(ctypes.c_void_p), 8) < 8:
        return {}
    t = [float(v) / 100.0 for v in buf[:7]]   # 100 MHz ticks -> us
    k = int(buf[7])
    return {"hash_us": t[1] - t[0], "table_us": t[2] - t[1], "cluster_us": t[3] - t[2], "map_us": t[4] - t[3],
            "passes_us": t[5], "partitions_us": t[6],
            "passes": {"init": k & 0xFFFF, "split": (k >> 16) & 0xFFFF, "kmeans": (k >> 32) & 0xFFFF}}


def last_persist_rounds(device=0):
    return lib().dq_hip_last_persist_rounds(device)


def set_lanes(lanes):
    """Engine lanes a batch is split over (0: default, DQ_HIP_LANES, else 4 with
    GPU_MAX_HW_QUEUES >= 6, else 3)."""
    lib().dq_hip_set_lanes(int(lanes))


def get_lanes():
    return lib().dq_hip_get_lanes()


def build_id():
    """FNV-1a-64 of the sources the loaded library was built from (tools/source_id.py)."""
    return int(lib().dq_hip_build_id())


def set_debug(flags, device=0):
    """Test-only interleaving knobs (dq_hip.h dq_hip_set_debug; 0 in production):
    1 prewarm the 2-means hand-off lines, 2 uneven workgroup stalls, 4 host
    delays between a round's status and its results, 8 plan-kernel stall,
    16 check that the round arena is all zero when a run starts, 32 release the
    round arena at every run's start (its rounds allocate new chunks)."""
    lib().dq_hip_set_debug(device, int(flags))


def set_timing(on, device=0):
    lib().dq_hip_set_timing(device, 1 if on else 0)


def reset_stats(device=0):
    lib().dq_hip_reset_stats(device)


def get_stats(device=0):
    """{kind: (launches, total_ms, engine-model bytes, points)} from HIP events on the launch stream."""
    res = {}
    for i, name in enumerate(STAT_KINDS):
        l, ms, b, u = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        lib().dq_hip_get_stat(device, i, ctypes.byref(l), ctypes.byref(ms), ctypes.byref(b))
        lib().dq_hip_get_stat_units(device, i, ctypes.byref(u))
        res[name] = (int(l.value), float(ms.value), float(b.value), float(u.value))
    return res
