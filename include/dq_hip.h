/*
 * dq_hip.h -- the thin C ABI of libdivquant_hip.so (MI355X / gfx950).
 *
 * Plain pointers and sizes only (no torch, no HIP types in the signatures;
 * `stream` is a hipStream_t passed as void*; NULL = the library's stream,
 * which first waits for the work already queued on the default stream, so
 * inputs written there -- a framework's host-to-device copy -- are seen).
 * The reference-signature wrappers (include/DivQuantHeader.h,
 * include/quant_util.h) are implemented on top of these entry points; an FFI
 * (ctypes, cgo, JNI...) can bind them directly -- see INTEGRATION.md.
 *
 * Errors: HIP/runtime failures abort the process with a message on stderr,
 * like the reference's abort() paths (DivQuantCluster.cpp:1021-1026,
 * DivQuantMapColors.cpp:43-51).  Invalid arguments return a negative code.
 */
#ifndef DQ_HIP_H
#define DQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQ_HIP_ABI_VERSION 1

int dq_hip_abi_version(void);
/* Number of visible HIP devices (0 when none). */
int dq_hip_device_count(void);

/* ---- host-pointer entry points (SURVEY 8b build-side shim) ---------------
 * dq_hip_quant: quant_recurse semantics (quant_util.cpp:20-158) without the
 * stdout timer lines.  uniq: allPixelsUnique (1: uniform weights; 0: the
 * weighted path -- calc_color_table dedup + ordered FP64 folds, exactly the
 * reference's).  ngpus <= 1: current device; ngpus > 1 (uniform
 * weights): the pixels split into ngpus ranges over devices 0..ngpus-1 of
 * this process (clamped to the visible devices), every pass's node totals
 * allreduced over an in-process RCCL communicator set (ncclCommInitAll,
 * xGMI), each device mapping its own range.
 * Returns the number of empty clusters (>= 0) or < 0 on bad arguments. */
int dq_hip_quant(const uint32_t *in, uint32_t n, uint32_t *out, uint32_t *k,
                 uint32_t *ct, int uniq, int ngpus);
/* map_colors_mps semantics (DivQuantMapColors.cpp:243-539). */
int dq_hip_map(const uint32_t *in, uint32_t n, uint32_t *out,
               const uint32_t *ct, int k);

/* genHistogramsForBlocks (ClusteringSegmentation.cpp:365-576) without the
 * OpenCV Mats: map the W x H frame `in` (0x00RRGGBB, Vec3BToUID packing,
 * OpenCVUtil.h:19-27) onto `palette` (npal colours; the app passes
 * getSubdividedColors, see dq_subdivided_colors) with map_colors_mps, then per
 * block of dim x dim pixels (block_w x block_h blocks, row-major) the most
 * frequent mapped colour, ties broken by the reference's unordered_map
 * iteration order.  mode: block_w*block_h words = HistogramForBlock::
 * regionQuantPixel (and the BGR of blockMat).  Optional (NULL to skip):
 * quant (W*H mapped frame), ndistinct (per block table size), keys/counts
 * (block_w*block_h*dim*dim words: each block's pixelToCountTable in iteration
 * order).  dim 1..4 (the app uses 4, ClusteringSegmentationMain.cpp:138);
 * every block must hold a pixel.  Returns 0 or < 0. */
int dq_hip_block_hist(const uint32_t *in, uint32_t width, uint32_t height,
                      const uint32_t *palette, int npal, uint32_t dim,
                      uint32_t block_w, uint32_t block_h, uint32_t *quant,
                      uint32_t *mode, uint32_t *ndistinct, uint32_t *keys,
                      uint32_t *counts);
/* getSubdividedColors (superpixels/OpenCVUtil.cpp:853-897): 125 colours. */
void dq_subdivided_colors(uint32_t *out125);
/* Synthetic benchmark frames: xorshift64 s^=s<<13; s^=s>>7;
 * s^=s<<17, one draw per pixel, pixel = draw & 0xFFFFFF; frame f of a batch
 * uses seed 0x9E3779B97F4A7C15 + f.  Host memory, no GPU needed. */
void dq_synth_xorshift(uint32_t *out, uint64_t n, uint64_t seed);
/* Word-wise FNV-1a-64 of n uint32 words (the golden fixtures' output hash). */
uint64_t dq_fnv1a64(const uint32_t *w, uint64_t n);

/* ---- device-pointer entry points (inputs already resident in HBM) --------
 * d_in/d_out: device pointers on `device`; k/ct: host.  Synchronous with
 * respect to the host on return (ct and *k are final). */
int dq_hip_quant_dev(int device, const uint32_t *d_in, uint32_t n,
                     uint32_t *d_out, uint32_t *k, uint32_t *ct,
                     int max_iters, void *stream);
/* A batch of frames in one call: every pass of every split round is one
 * kernel launch over the points of all frames.  d_in/d_out/n: nframes
 * entries; ct: nframes*k host words (frame i at ct + i*k); k_out[i] = its
 * colour count.  Returns the total number of empty clusters or < 0. */
int dq_hip_quant_batch_dev(int device, int nframes, const uint32_t *const *d_in,
                           const uint32_t *n, uint32_t *const *d_out, uint32_t k,
                           uint32_t *ct, uint32_t *k_out, int max_iters,
                           void *stream);
/* dq_hip_block_hist on device pointers (in, quant, mode, ndistinct, keys,
 * counts; quant is required: the mapped frame); palette is host memory.
 * Asynchronous on `stream`; with stream NULL the legacy default stream is
 * ordered after the work (as for every asynchronous entry below). */
int dq_hip_block_hist_dev(int device, const uint32_t *d_in, uint32_t width,
                          uint32_t height, const uint32_t *palette, int npal,
                          uint32_t dim, uint32_t block_w, uint32_t block_h,
                          uint32_t *d_quant, uint32_t *d_mode,
                          uint32_t *d_ndistinct, uint32_t *d_keys,
                          uint32_t *d_counts, void *stream);
/* BGR24 ingestion / output, device pointers, asynchronous
 * on `stream` (NULL: the library's stream of `device`).  d_bgr: an OpenCV
 * CV_8UC3 frame, `stride` bytes per row (>= 3*width; 3*width when
 * continuous).  Fast path when width, stride and d_bgr are 4-B aligned and
 * the u32 frame is 16-B aligned; any other layout is handled per pixel.
 * Return 0 or -1 on bad arguments.
 *   pack:   d_out[y*width+x] = Vec3BToUID(img(y,x))   (superpixels/OpenCVUtil.h:19-27;
 *           the loop at ClusteringSegmentation.cpp:381-395)
 *   unpack: img(y,x) = PixelToVec3b(d_in[y*width+x])  (OpenCVUtil.h:53-59;
 *           ClusteringSegmentation.cpp:1812-1817); bits 24-31 are dropped
 *   gather: d_out[i] = Vec3BToUID(img(c.y, c.x)) for the i-th Coord, passed
 *           as its 32-bit layout (x | y << 16, superpixels/Coord.h:30-33);
 *           ClusteringSegmentation.cpp:1795-1800.  Coords are not range-checked. */
int dq_hip_pack_bgr24_dev(int device, const uint8_t *d_bgr, uint32_t width,
                          uint32_t height, uint32_t stride, uint32_t *d_out,
                          void *stream);
int dq_hip_unpack_bgr24_dev(int device, const uint32_t *d_in, uint32_t width,
                            uint32_t height, uint32_t stride, uint8_t *d_bgr,
                            void *stream);
int dq_hip_gather_bgr24_dev(int device, const uint8_t *d_bgr, uint32_t stride,
                            const uint32_t *d_coords, uint32_t n, uint32_t *d_out,
                            void *stream);
/* Row-tile sharding.  Frame i's rows are d_in[i] (n[i] points,
 * width[i] per row; width NULL or 0: shard boundaries on 4-point multiples).
 * Inside this process the rows are split into nshard (1..8) row ranges that
 * are processed as separate shards on `device` (the exact arithmetic of
 * multi-GPU sharding); across processes, n_global[i] (NULL or 0: n[i]) is the
 * whole frame's size and every pass's integer node totals are allreduced
 * over the communicator of dq_hip_comm_init (RCCL over xGMI).  Every
 * process gets the same colortables; d_out[i] receives this process's rows
 * mapped (d_out NULL: clustering only).  Returns empty clusters, -1 on bad
 * arguments, -2 if n_global > n without a communicator. */
int dq_hip_quant_rows_dev(int device, int nframes, const uint32_t *const *d_in,
                          const uint32_t *n, const uint32_t *width,
                          const uint64_t *n_global, int nshard,
                          uint32_t *const *d_out, uint32_t k, uint32_t *ct,
                          uint32_t *k_out, int max_iters, void *stream);
/* RCCL communicator of the engine on `device` (one process per GPU): rank 0
 * creates the 128-byte id, the launcher broadcasts it (e.g. with
 * torch.distributed), every rank calls dq_hip_comm_init.  Return 0 / < 0. */
int dq_hip_comm_unique_id(void *id128);
int dq_hip_comm_init(int device, int nranks, int rank, const void *id128);
int dq_hip_comm_destroy(int device);
/* Ranks of the engine's communicator on `device` (1: none). */
int dq_hip_comm_size(int device);
/* Clustering only (quant_varpart_fast, DivQuantCluster.cpp:1099-1179):
 * writes the non-empty cluster colours (cluster-index order, NOT deduped). */
int dq_hip_cluster_dev(int device, const uint32_t *d_in, uint32_t n,
                       uint32_t *k, uint32_t *ct, int max_iters, void *stream);
/* The weighted path (allPixelsUnique = 0) on device pixels: calc_color_table
 * on the GPU (DivQuantMapColors.cpp:82-203), DivQuantCluster<false,*,true>
 * with the reference's ordered FP64 folds, then (d_out != NULL) the colortable
 * dedup and map_colors_mps into d_out; d_out NULL: quant_varpart_fast's table
 * (cluster-index order, not deduped).  Synchronous on return. */
int dq_hip_quant_weighted_dev(int device, const uint32_t *d_in, uint32_t n,
                              uint32_t *d_out, uint32_t *k, uint32_t *ct,
                              int max_iters, void *stream);
/* Many weighted calls at once -- the app's per-superpixel-region
 * quant_recurse(N_region, .., K, allPixelsUnique=0)
 * (ClusteringSegmentation.cpp:1779-1803): region i reads d_ins[i][0..ns[i]),
 * writes its mapped colours to d_outs[i] (d_outs may be NULL: cluster + dedup
 * only), its deduped colortable to cts + i*ct_stride (ks[i] <= ct_stride
 * entries of room) and its size to k_outs[i].  Regions of at most 131071
 * pixels, 6144 colours and K <= 64 run in ONE launch, one workgroup each;
 * the others one by one.  Every result equals the region's own call.
 * Returns the total of empty clusters, or < 0 (bad arguments). */
int dq_hip_quant_weighted_regions_dev(int device, int nregions, const uint32_t *const *d_ins,
                                      const uint32_t *ns, uint32_t *const *d_outs, const uint32_t *ks,
                                      uint32_t *cts, uint32_t ct_stride, uint32_t *k_outs,
                                      int max_iters, void *stream);
/* quant_varpart_fast semantics (DivQuantCluster.cpp:1099-1179) on device
 * pixels for every (num_bits, dec_factor, allPixelsUnique): uniform weights
 * when uniq && num_bits == 8 && dec_factor == 1, else cut_bits to num_bits
 * (DivQuantUni.cpp:28-100; skipped when !uniq && num_bits == 8), the
 * decimated calc_color_table walk over a rows x cols frame with the
 * reference's numRows stride (DivQuantMapColors.cpp:120-125) and the weighted
 * clustering, centres shifted back by 8 - num_bits (:1050-1052).  ct gets
 * the table in cluster-index order (not deduped, not mapped).  Returns the
 * number of empty clusters, -1 on bad arguments, -2 when the walk would read
 * past n (the reference reads out of bounds there).  Synchronous on return. */
int dq_hip_varpart_dev(int device, const uint32_t *d_in, uint32_t n, uint32_t rows,
                       uint32_t cols, uint32_t *k, uint32_t *ct, int num_bits,
                       int dec_factor, int max_iters, int uniq, void *stream);
/* cut_bits (DivQuantUni.cpp:28-100) on device pixels: each channel shifted
 * right by 8 - its bit count (1..8); d_out may equal d_in.  Stream-ordered. */
int dq_hip_cut_bits_dev(int device, const uint32_t *d_in, uint32_t n, uint32_t *d_out,
                        int num_bits_red, int num_bits_green, int num_bits_blue,
                        void *stream);
int dq_hip_map_dev(int device, const uint32_t *d_in, uint32_t n,
                   uint32_t *d_out, const uint32_t *ct, int k, void *stream);

/* ---- cluster labels (what a segmentation consumer works with) ------------
 * The label of pixel p for a colortable ct[0..k): with c the colour
 * dq_hip_map_dev writes for p, the lowest i with (ct[i] & 0xFFFFFF) ==
 * (c & 0xFFFFFF) -- unique for the deduplicated colortables the quant entry
 * points return (the command line's "tag"), well defined for palettes with
 * duplicate entries.  Labels are uint8_t, uint16_t or uint32_t: label_bytes =
 * 1, 2 or 4.  Any other label_bytes, a width that cannot hold index k - 1
 * (for the quant entries: the requested k) or a label pointer that is not
 * naturally aligned is a bad argument: -1, nothing runs.  d_labels: n labels
 * on `device`; exactly those n * label_bytes bytes are written.  Input is
 * packed 0x00RRGGBB (top byte ignored).
 * dq_hip_map_labels_dev: the labels of dq_hip_map_dev's colours; stream and
 * synchronisation as dq_hip_map_dev.  Returns 0 or < 0. */
int dq_hip_map_labels_dev(int device, const uint32_t *d_in, uint32_t n, void *d_labels,
                          int label_bytes, const uint32_t *ct, int k, void *stream);
/* dq_hip_quant_batch_dev (uniq = 1) with labels in place of colours: the same
 * ct (frame i at ct + i*k), k_out and return value; frame i's labels index
 * its deduplicated colortable ct + i*k [0..k_out[i]).  uniq = 0: every frame
 * through the weighted path, as dq_hip_quant_weighted_dev would, one after
 * the other.  Synchronous on return. */
int dq_hip_quant_labels_batch_dev(int device, int nframes, const uint32_t *const *d_in,
                                  const uint32_t *n, void *const *d_labels, int label_bytes,
                                  uint32_t k, uint32_t *ct, uint32_t *k_out, int uniq,
                                  int max_iters, void *stream);
/* Host pointers, the current device: dq_hip_quant with n labels (label_bytes
 * each) in place of the mapped colours. */
int dq_hip_quant_labels(const uint32_t *in, uint32_t n, void *labels, int label_bytes,
                        uint32_t *k, uint32_t *ct, int uniq);

/* ---- connected regions of a label map (labels -> segments on the device) --
 * A cluster label is not yet a segment: two patches on opposite sides of a
 * frame share a label.  The reference works on connected regions (floodFill /
 * floodFillMask with 8-connectivity over tag images, region masks with pixel
 * counts and bounding rectangles); these entries give them without a host
 * flood fill.
 * Definition.  Input: a width x height row-major map of labels, label_bytes
 * (1, 2 or 4) each, and a connectivity (4 or 8).  Two pixels are in the same
 * region when a path of 4- / 8-neighbours with EQUAL label values joins them
 * (u32 labels: all 32 bits are compared -- mask mapped colours first).
 * Regions are numbered 0 .. R-1 in raster order of their first pixel, the
 * lowest y * width + x of the region.  The answer is therefore unique: exact
 * integers that do not depend on scheduling.
 * d_regions (required): width * height uint32 region ids, always complete.
 * Stats (each pointer may be NULL), stats_cap entries each; regions with id >=
 * stats_cap are left out of the stats (the map still numbers them, the return
 * value still counts them) and nothing behind entry min(R, stats_cap) is
 * written:
 *   d_area   pixels of the region
 *   d_bbox   4 words per region: x0, y0, x1, y1, inclusive
 *   d_first  y * width + x of the region's first pixel in raster order
 *   d_label  the region's label value
 *   d_sums   3 uint64 per region: the R, G and B sums of d_pixels (the packed
 *            0x00RRGGBB frame the labels came from) over the region; needs
 *            d_pixels
 * Both forms return R >= 1 and are synchronous on return.  -1, before any
 * device work, for: label_bytes not 1/2/4, connectivity not 4/8, width or
 * height 0 or above 65535 (the Coord layout, x | y << 16) or width * height
 * above 2^31 - 1, NULL labels or regions, labels / regions / stats arrays not
 * naturally aligned, d_sums without d_pixels, stats_cap > 0 with every stats
 * pointer NULL.
 * Scratch: 4 B per pixel + 4 B per 1024 pixels, allocated and freed in stream
 * order by the call (calls on two streams may overlap).  The tile pass works
 * on DQ_HIP_REGION_TILE x DQ_HIP_REGION_TILE pixel tiles. */
#define DQ_HIP_REGION_TILE 64
int64_t dq_hip_label_regions_dev(int device, const void *d_labels, int label_bytes,
                                 uint32_t width, uint32_t height, int connectivity,
                                 uint32_t *d_regions,
                                 uint32_t stats_cap, uint32_t *d_area, uint32_t *d_bbox,
                                 uint32_t *d_first, uint32_t *d_label,
                                 const uint32_t *d_pixels, uint64_t *d_sums,
                                 void *stream);
/* Host pointers, the current device. */
int64_t dq_hip_label_regions(const void *labels, int label_bytes, uint32_t width,
                             uint32_t height, int connectivity, uint32_t *regions,
                             uint32_t stats_cap, uint32_t *area, uint32_t *bbox,
                             uint32_t *first, uint32_t *label,
                             const uint32_t *pixels, uint64_t *sums);

/* ---- region adjacency graph of a region map (regions -> the regions that
 * touch, on the device) --------------------------------------------------
 * The first thing the reference builds from a tag image is the set of
 * neighbour tags of every superpixel (SuperpixelImage::parseSuperpixelEdges,
 * the SuperpixelEdgeTable: the 8 neighbours of every pixel); its merge code
 * walks those sets.  These entries give the same graph as an edge list with
 * per-edge stats, without a host scan of the map.
 * Definition.  Input: a width x height row-major map of uint32 region ids and
 * a connectivity (4 or 8).  The map is ANY id map (the region map of
 * dq_hip_label_regions_dev is the intended one): ids need not be connected,
 * numbered in raster order, or dense.
 * A contact is a pair of pixel indexes p < q (y * width + x) that are 4- / 8-
 * neighbours with regions[p] != regions[q].  For one p the possible q are, in
 * increasing order: right p + 1, down-left p + width - 1 (8 only), down
 * p + width, down-right p + width + 1 (8 only); nothing wraps around a row end.
 * An edge is an unordered pair of ids {a, b}, stored a < b, with at least one
 * contact.  Edges are numbered 0 .. E-1 in the order of their first contacts
 * (the lexicographically lowest (p, q) of each): the order in which a raster
 * scan over p, and over q for each p, first meets them.  The answer is
 * therefore unique: exact integers that do not depend on scheduling.
 * Edge arrays (each pointer may be NULL), edge_cap entries each; edges with
 * index >= edge_cap are left out (the return value still counts them) and
 * nothing behind entry min(E, edge_cap) is written:
 *   d_edges    2 words per edge: a, b (a < b)
 *   d_border   the edge's number of contacts
 *   d_contact  2 words per edge: p, q of its first contact
 *   d_step     uint64: the sum over the edge's contacts of |dR| + |dG| + |dB|
 *              between the two pixels of d_pixels (the packed 0x00RRGGBB
 *              frame, top byte ignored); needs d_pixels.  step / border is the
 *              mean colour step across the border.
 * edge_cap == 0 with every edge pointer NULL is the count-only call.
 * d_degree (may be NULL): nregions words, degree[r] = the number of edges
 * with r as an end (the size of the reference's neighbour set of tag r), 0
 * for ids that touch nothing; it counts all E edges whatever edge_cap is.
 * Every id in the map must then be < nregions (not checked, like Coords).
 * nregions is ignored without d_degree.
 * Both forms return E >= 0 and are synchronous on return.  -1, before any
 * device work, for: NULL regions, connectivity not 4/8, width or height 0 or
 * above 65535, width * height above DQ_HIP_ADJACENCY_MAX_PIXELS = 2^30, an
 * array not naturally aligned (4 B; 8 B for d_step), d_step without d_pixels,
 * edge_cap > 0 with every edge pointer NULL, d_degree with nregions == 0.
 * Why 2^30: with n <= 2^30 pixels a contact is the single word 4 * p + dir
 * (dir 0..3 in the order above), whose order is the order of (p, q); E < the
 * number of contacts < 4 n <= 2^32, so E fits uint32; and 0xFFFFFFFF is no
 * valid contact (the last pixel has no down-right neighbour), so it can mark
 * "none yet".
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): 4 B per 1024 pixels + 4 B, and a
 * hash table of S slots of 16 B (24 B with d_step), S = the power of two
 * >= 2 * Hd, at least 1024.  Hd ("heads") is counted first and read back by
 * the host: per direction, the runs of equal id pairs along 64 consecutive
 * pixels; E <= Hd <= the number of contacts.  A smooth frame has few; a map
 * where every contact is its own edge (noise) has Hd ~ 4 n, i.e. up to
 * 8 n slots. */
#define DQ_HIP_ADJACENCY_MAX_PIXELS 0x40000000u
int64_t dq_hip_region_adjacency_dev(int device, const uint32_t *d_regions,
                                    uint32_t width, uint32_t height, int connectivity,
                                    uint32_t edge_cap, uint32_t *d_edges /*2 per edge: a, b*/,
                                    uint32_t *d_border, uint32_t *d_contact /*2 per edge: p, q*/,
                                    const uint32_t *d_pixels, uint64_t *d_step,
                                    uint32_t nregions, uint32_t *d_degree, void *stream);
/* Host pointers, the current device. */
int64_t dq_hip_region_adjacency(const uint32_t *regions, uint32_t width, uint32_t height,
                                int connectivity, uint32_t edge_cap, uint32_t *edges,
                                uint32_t *border, uint32_t *contact,
                                const uint32_t *pixels, uint64_t *step,
                                uint32_t nregions, uint32_t *degree);

/* ---- region merge (regions + their graph -> segments, on the device) ------
 * Connected regions of a cluster-label map are mostly specks; the reference
 * absorbs them with sequential heuristics (mergeSmallSuperpixels: superpixels
 * under 10 pixels go to their most alike neighbour).  These entries merge over
 * the adjacency graph by a rule with ONE exact integer answer that does not
 * depend on scheduling (Boruvka-style rounds).
 * Inputs.  A flat map of n uint32 region ids, each < nregions = R.  Per region
 * d_area[r] > 0, d_first[r] (its lowest pixel index, distinct per region) and
 * d_sums[r][3] (uint64 R, G, B sums): the arrays dq_hip_label_regions_dev
 * writes; optionally d_bbox[r][4].  A list of nedges id pairs (a, b), a != b,
 * both < R: the order within a pair, the order of the pairs and duplicates do
 * not matter (the d_edges of dq_hip_region_adjacency_dev is the intended one).
 * State.  comp[r], the component of region r, at first r itself.  A component
 * carries area, sums, first and bbox of its regions together.
 * One round.
 *   1 A component A is restless when area[A] < min_area.
 *   2 mean(A, c) = floor(256 * sums[A][c] / area[A]), integer, < 2^16.
 *   3 d(A, B) = the sum over c of |mean(A, c) - mean(B, c)| (<= 195840).
 *   4 Every edge with A = comp[a] != B = comp[b] and d(A, B) <= max_dist
 *     offers A, if restless, the key (d << 32) | B, and B, if restless, the
 *     key (d << 32) | A.  best[A] is the lowest key offered to A: the lowest
 *     distance, ties to the lowest component id.
 *   5 A restless A with a best has the target T = the low word of best[A].
 *     If T is restless, best[T] targets A and A < T, A stays a root;
 *     otherwise parent[A] = T.
 *   6 A round that makes no link is not counted and ends the call.
 *   7 Otherwise the root of a component is the fixed point of parent; area,
 *     sums, the minimum first and the bbox union of every component are added
 *     into its root, comp[r] = root(comp[r]) for every r, and the round counts.
 *   (Along a cycle of parent choices the distances cannot increase, so they
 *   are equal; among equal distances everyone picks its lowest neighbour, so
 *   the node after the cycle's lowest id points back at it: a mutual pair, of
 *   which rule 5 keeps the lower as the root.  parent is a forest.)
 * End.  After a round without a link, or after max_rounds rounds (0: no
 * limit).  Every counted round removes at least one component, so there are
 * fewer than nregions rounds.  With max_dist = 0xFFFFFFFF the restless
 * components at least halve per round (32 rounds at most); with a distance
 * limit a component may get its first offer only after a neighbour's mean has
 * moved, and a star of such leaves takes one round per leaf.  The final
 * components are numbered 0 .. R'-1 in increasing order of their first, the
 * numbering rule of the connected regions above.
 * Outputs.  d_out_regions (required, may be d_regions): the n new ids.
 * d_remap (may be NULL): nregions words, the new id of old region r.  Stats of
 * the new regions (each pointer may be NULL), stats_cap entries each, regions
 * with new id >= stats_cap left out and nothing behind entry min(R', stats_cap)
 * written: d_out_area, d_out_bbox (4 words; needs d_bbox), d_out_first,
 * d_out_sums (3 uint64).  *rounds (host, may be NULL): the rounds counted.
 * nedges == 0 or min_area == 0 is a valid call that only renumbers by first.
 * Returns R' >= 1, synchronous on return.  -1, before any device work, for:
 * NULL d_regions, d_area, d_first, d_sums or d_out_regions; n == 0 or n above
 * 2^31 - 1; nregions == 0 or above n; nedges > 0 with NULL d_edges; a pointer
 * not naturally aligned (4 B; 8 B for the sums); d_out_bbox without d_bbox;
 * stats_cap > 0 with every output stats pointer NULL.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): 60 B per region (76 B with
 * d_bbox, 4 B more without d_remap), one bit per pixel and 4 B per 1024
 * pixels.  The host reads 4 bytes back per round (the links made). */
int64_t dq_hip_merge_regions_dev(int device, const uint32_t *d_regions, uint32_t n,
                                 uint32_t nregions, const uint32_t *d_area,
                                 const uint32_t *d_first, const uint64_t *d_sums,
                                 const uint32_t *d_bbox /*may be NULL*/,
                                 uint32_t nedges, const uint32_t *d_edges /*2 per edge*/,
                                 uint32_t min_area, uint32_t max_dist, uint32_t max_rounds,
                                 uint32_t *d_out_regions /*may equal d_regions*/,
                                 uint32_t *d_remap /*may be NULL*/,
                                 uint32_t stats_cap, uint32_t *d_out_area, uint32_t *d_out_bbox,
                                 uint32_t *d_out_first, uint64_t *d_out_sums,
                                 uint32_t *rounds /*host, may be NULL*/, void *stream);
/* Host labels -> segments, the current device: one upload (labels and the
 * packed 0x00RRGGBB frame), connected regions, their adjacency graph and the
 * merge above on the device, one download (the map and the stats of the R'
 * segments; bbox x0, y0, x1, y1 inclusive).  The region and edge counts are
 * known only after those stages ran, so each of the two runs twice: count-only,
 * then with exact capacity.  Returns R'; -1, before any device work, for what
 * dq_hip_label_regions or dq_hip_region_adjacency refuse (label_bytes,
 * connectivity, sides above 65535, more than DQ_HIP_ADJACENCY_MAX_PIXELS
 * pixels, NULL or misaligned labels / regions / stats arrays, stats_cap > 0
 * with every stats pointer NULL) and for NULL pixels. */
int64_t dq_hip_segment_labels(const void *labels, int label_bytes, uint32_t width,
                              uint32_t height, int connectivity, const uint32_t *pixels,
                              uint32_t min_area, uint32_t max_dist, uint32_t max_rounds,
                              uint32_t *regions, uint32_t stats_cap, uint32_t *area,
                              uint32_t *bbox, uint32_t *first, uint64_t *sums,
                              uint32_t *rounds /*may be NULL*/);

/* ---- pixel lists (region map -> the pixels of every region, on the device) --
 * The reference keeps a vector<Coord> per region, gathers inPixels[i] =
 * Vec3BToUID(inputImg(c.y, c.x)) from it before the region's quant_recurse
 * (ClusteringSegmentation.cpp:1795-1800) and paints outPixels[i] back at
 * Coord i (:1836-1846).  These entries build all the lists of a region map at
 * once, in CSR form, and run the per-region calls on them.
 * Definition.  A stable counting sort of the pixels by region id: ONE exact
 * integer answer that does not depend on scheduling.  With n = width * height
 * and every id < nregions = R (not checked, like Coords; the kernels skip a
 * larger id, whose pixel is then in no list, and write nothing out of bounds):
 *   d_offsets[r] = the number of pixels whose id is < r, d_offsets[R] = n
 *   (an id that owns no pixel is allowed: its range is empty);
 *   the j-th pixel of region r in raster order (increasing p = y * width + x)
 *   is entry d_offsets[r] + j of each output array given (n words each):
 *     d_index   p
 *     d_coords  x | y << 16   (the Coord word dq_hip_gather_bgr24_dev reads)
 *     d_colors  d_pixels[p], the whole word
 * d_offsets is required; each of the three arrays may be NULL (all three NULL:
 * the offsets only); d_colors needs d_pixels.
 * Accepted maps.  T = the sum, over the ids present, of (last row - first row
 * + 1).  Every map with T <= n is taken.  A 4- or 8-connected region has a
 * pixel in every row it spans, so the maps of dq_hip_label_regions_dev and
 * dq_hip_merge_regions_dev always qualify; other maps do when they fit.
 * Returns 0, synchronous on return.  -2 when T > n: decided once T is known
 * and before any output array is written (d_offsets included).  -1, before any
 * device work, for: NULL d_regions or d_offsets; width or height 0 or above
 * 65535; n above 2^31 - 1; nregions 0 or above 2^31 - 1; an array not 4-byte
 * aligned; d_colors without d_pixels.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): 8 B per region + 4 B per 1024
 * regions + 4 B; then, once T is read back (4 bytes), 4 B per table entry (T
 * <= n entries) + 4 B per 1024 entries + 4 B.
 * One wave walks one row of the map, 64 pixels at a time: a 65535 x 1 map is
 * one wave's work, correct and slow. */
int64_t dq_hip_region_pixels_dev(int device, const uint32_t *d_regions, uint32_t width,
                                 uint32_t height, uint32_t nregions,
                                 uint32_t *d_offsets /* nregions + 1 */,
                                 uint32_t *d_coords, uint32_t *d_index,
                                 const uint32_t *d_pixels, uint32_t *d_colors, void *stream);
/* Host pointers, the current device.  A refused map (-2) leaves them as they were. */
int64_t dq_hip_region_pixels(const uint32_t *regions, uint32_t width, uint32_t height,
                             uint32_t nregions, uint32_t *offsets, uint32_t *coords,
                             uint32_t *index, const uint32_t *pixels, uint32_t *colors);
/* The inverse of a gather by Coords: d_frame[(c >> 16) * width + (c & 0xFFFF)]
 * = d_values[i] for the n Coord words c = d_coords[i].  Asynchronous on
 * `stream`; Coords are not range-checked (as in dq_hip_gather_bgr24_dev).
 * Returns 0; -1 for a NULL or misaligned pointer or width 0. */
int dq_hip_scatter_coords_dev(int device, const uint32_t *d_values, const uint32_t *d_coords,
                              uint32_t n, uint32_t width, uint32_t *d_frame, void *stream);
/* Region map -> painted frame: the pixel lists above (offsets, Coords, colours),
 * the nregions + 1 offsets read back, ONE dq_hip_quant_weighted_regions_dev
 * style call in which region r's list is its range of the colours and its K is
 * k (the jobs go to that path 8192 at a time: it keeps a pinned argument and
 * result record per job of a call), and, with d_out, the mapped colours
 * scattered back to their pixels: every pixel of d_out is written.  Region r's
 * colortable is cts[r * k .. r * k + k_outs[r]), equal to its own
 * dq_hip_quant_weighted_dev call on its pixels in raster order.  An id without
 * a pixel is skipped: k_outs[r] = 0, its cts row untouched.  Returns the total
 * of empty clusters, synchronous on return; -2 as above; -1, before any device
 * work, for what dq_hip_region_pixels_dev refuses, NULL d_pixels, cts or
 * k_outs, a misaligned d_out, k == 0 (or above 2^31 - 1) or max_iters < 1.
 * Device memory of the call: 4 (nregions + 1) + 4 n bytes (12 n with d_out)
 * and the scratch above.  The quant runs on the device's engine (its lock is
 * held for that stage alone). */
int64_t dq_hip_quant_region_map_dev(int device, const uint32_t *d_regions, uint32_t width,
                                    uint32_t height, uint32_t nregions,
                                    const uint32_t *d_pixels, uint32_t k,
                                    uint32_t *d_out /* n words, may be NULL */,
                                    uint32_t *cts /* host, nregions * k */,
                                    uint32_t *k_outs /* host, nregions */, int max_iters,
                                    void *stream);
/* Host pointers, the current device (one upload, one download). */
int64_t dq_hip_quant_region_map(const uint32_t *regions, uint32_t width, uint32_t height,
                                uint32_t nregions, const uint32_t *pixels, uint32_t k,
                                uint32_t *out /* may be NULL */, uint32_t *cts,
                                uint32_t *k_outs, int max_iters);

/* ---- capture windows of a region map ----------------------------------------
 * The block-dilated pixel lists the reference's captureRegionMask works on
 * (ClusteringSegmentation.cpp:1038-1190 through morphRegionMask, :849-1029, and
 * expandBlockRegion, OpenCVUtil.cpp:668-731; DESIGN.md 5a''''''): one list per
 * region, and one pixel in many lists.
 * The grid: BW = ceil(width / block) by BH = ceil(height / block) blocks, pixel
 * (x, y) in block (x / block, y / block).  own(r) = the blocks that hold a
 * pixel of r (the mask plays no part).  window(r) = the blocks of the grid at
 * L1 distance <= expand from a block of own(r): `expand` dilations by OpenCV's
 * 3 x 3 MORPH_ELLIPSE element, which is the plus-shaped cross, with nothing
 * coming in from outside the grid.  The reference has block 4, expand 2.
 * With d_area (nregions words) a region with d_area[r] <= min_area is absent
 * (:1061-1069): its window is empty; its pixels stay pixels of the frame.
 * The list of r: the blocks of window(r) in raster order of blocks, in each
 * block its pixels in raster order, without the pixels outside the frame
 * (right and bottom blocks are clipped) and the pixels p with d_mask[p] != 0
 * (n bytes, may be NULL; consumed by an earlier capture, :1079-1105).
 * d_offsets[r] = the total length of the lists of the ids < r, d_offsets[nregions]
 * = M; entry d_offsets[r] + j of d_index, d_coords and d_colors is the j-th
 * pixel of the list of r: p, x | y << 16 and d_pixels[p], the words of
 * dq_hip_region_pixels_dev.  With block 1, expand 0, no mask and no area these
 * are exactly the pixel lists.  An id >= nregions (not allowed) founds no
 * block and has no list; its pixels are pixels of the frame like any other.
 * Returns M >= 0, synchronous on return; d_offsets is then written.  The three
 * list arrays, `cap` words each and each may be NULL, are written when M <= cap
 * and not touched when M > cap: call with cap 0 and no list array for M, then
 * with room.  -3 when M, or P below, reaches 2^32 - 1: the sums saturate there
 * (so an M of exactly 2^32 - 1 is given up too); decided before any output
 * array is written.  -2 for a map the call refuses, before any output array is
 * written: with P = the sum over the regions of |window(r)| and T = the sum
 * over the regions with a window of the block rows it spans, a map with T > P.
 * A 4- or 8-connected region has a window block in every block row its window
 * spans (its own blocks cover the rows of the region, the blocks straight
 * above and below them the `expand` rows on each side), so the maps of
 * dq_hip_label_regions_dev and dq_hip_merge_regions_dev always qualify; other
 * maps do when they fit.  -1, before any device work, for: NULL d_regions or
 * d_offsets; width or height 0 or above 65535; n above 2^31 - 1; nregions 0 or
 * above 2^31 - 1; block outside 1..8; expand above 3; a word array not 4-byte
 * aligned; d_colors without d_pixels; cap > 0 with all three list arrays NULL.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap), with NB = BW * BH blocks:
 * 4 (block^2 + 2) B per block + 8 B per region + 4 B per 1024 of each + 12 B;
 * then, once P and T are read back (8 bytes), 8 B per pair + 4 B per table
 * entry (T <= P) + 4 B per 1024 entries + 4 B.  M is read back as well.
 * One wave walks the pairs of one block row, 64 at a time. */
int64_t dq_hip_region_windows_dev(int device, const uint32_t *d_regions, uint32_t width,
                                  uint32_t height, uint32_t nregions, uint32_t block,
                                  uint32_t expand, const uint8_t *d_mask, const uint32_t *d_area,
                                  uint32_t min_area, uint32_t *d_offsets /* nregions + 1 */,
                                  uint32_t cap, uint32_t *d_coords, uint32_t *d_index,
                                  const uint32_t *d_pixels, uint32_t *d_colors, void *stream);
/* Host pointers, the current device.  A call that returns < 0 leaves them as
 * they were; M > cap leaves the list arrays as they were. */
int64_t dq_hip_region_windows(const uint32_t *regions, uint32_t width, uint32_t height,
                              uint32_t nregions, uint32_t block, uint32_t expand,
                              const uint8_t *mask, const uint32_t *area, uint32_t min_area,
                              uint32_t *offsets, uint32_t cap, uint32_t *coords, uint32_t *index,
                              const uint32_t *pixels, uint32_t *colors);
/* Region map -> one colortable per capture window: the windows call above with
 * the same arguments (d_pixels is needed), the nregions + 1 offsets read back,
 * and ONE dq_hip_quant_weighted_regions_dev style call in which region r's
 * input is its range of the colours in list order and its K is k (marshalled
 * as in dq_hip_quant_region_map_dev).  cts[r * k .. r * k + k_outs[r]) equals
 * the region's own dq_hip_quant_weighted_dev call on its window in list order;
 * an empty window gives k_outs[r] = 0 and leaves its cts row untouched.  d_out
 * (`cap` words, may be NULL) gets the mapped colours in list order: windows
 * overlap, so there is no scatter to a frame.  The colours are the caller's
 * d_colors when M <= cap, else the call's own (the windows are then built a
 * second time, with room).  Returns the total of empty clusters, synchronous on
 * return; -4 when M > cap with d_out given (d_offsets is written, nothing is
 * quantised); -2 and -3 as above; -1, before any device work, for what the
 * windows call refuses (d_out counts as a list array there), NULL d_pixels,
 * cts or k_outs, a misaligned d_out, k == 0 (or above 2^31 - 1) or max_iters
 * < 1.  The reference quantises a heuristic subset of the window
 * (combinedCoords, :1791-1803); that subset stays out of scope: this entry
 * gives the per-window table that the subset's logic starts from. */
int64_t dq_hip_quant_region_windows_dev(int device, const uint32_t *d_regions, uint32_t width,
                                        uint32_t height, uint32_t nregions, uint32_t block,
                                        uint32_t expand, const uint8_t *d_mask,
                                        const uint32_t *d_area, uint32_t min_area,
                                        uint32_t *d_offsets /* nregions + 1 */, uint32_t cap,
                                        uint32_t *d_coords, uint32_t *d_index,
                                        const uint32_t *d_pixels, uint32_t *d_colors, uint32_t k,
                                        uint32_t *d_out /* cap words, may be NULL */,
                                        uint32_t *cts /* host, nregions * k */,
                                        uint32_t *k_outs /* host, nregions */, int max_iters,
                                        void *stream);
/* Host pointers, the current device. */
int64_t dq_hip_quant_region_windows(const uint32_t *regions, uint32_t width, uint32_t height,
                                    uint32_t nregions, uint32_t block, uint32_t expand,
                                    const uint8_t *mask, const uint32_t *area, uint32_t min_area,
                                    uint32_t *offsets, uint32_t cap, uint32_t *coords,
                                    uint32_t *index, const uint32_t *pixels, uint32_t *colors,
                                    uint32_t k, uint32_t *out /* cap words, may be NULL */,
                                    uint32_t *cts, uint32_t *k_outs, int max_iters);

/* ---- window tags (which regions lie in a window, which colours on which side)
 * The two exact integer tables the reference reads off every capture window
 * before its heuristics branch: the tag histogram (tagHistogram,
 * sort_keys_by_count, mostCommonOtherTag; ClusteringSegmentation.cpp:1644-1663)
 * and the inside / outside histograms of the window's quant (:2009-2068);
 * DESIGN.md 5a'''''''.  All terms and the arguments d_regions .. min_area are
 * those of "capture windows" above.
 * For a region r with a window and an id s < nregions: c(r, s) = the number of
 * entries j of the list of r with d_regions[index[j]] == s, f(r, s) = the
 * smallest such j, relative to the start of r's list.  Row r holds the ids s
 * with c(r, s) > 0 in ascending f(r, s): the order in which the ids first
 * appear in the list of r, fixed by the definition alone.  So s = r is an entry
 * of its own row (the "inside" count); a region the area rule makes absent has
 * no row and still appears as s in other rows; an id whose pixels in the window
 * are all masked appears in no row.  Pixels with an id >= nregions (not
 * allowed) are counted in no entry.  The reference orders a row by count with
 * undefined ties (unordered_map order through an unstable sort) and uses only
 * the head of that order, so the call does not sort and gives the head exactly:
 * best other = the s != r with the largest c(r, s), ties to the lowest id.
 * Outputs, device word arrays, 4-byte aligned:
 *   d_rows[nregions + 1]  (required) CSR offsets, d_rows[nregions] = E, the
 *                         number of entries.  Returns E >= 0, synchronous.
 *   d_ids, d_counts, d_first  `cap` words each, each may be NULL: entry
 *                         d_rows[r] + i is the i-th entry of row r: s, c(r, s),
 *                         f(r, s).  Written when E <= cap, not touched when
 *                         E > cap; cap 0 with no entry array returns E alone.
 *   d_inside, d_best, d_best_count  nregions words each, each may be NULL:
 *                         c(r, r), the best other id (0xFFFFFFFF when the row
 *                         has no other id) and its count (0 then); a region
 *                         without a window gets 0, 0xFFFFFFFF, 0.  Written
 *                         whenever the call returns >= 0, whatever cap.
 *   d_offsets[nregions + 1]  (may be NULL here) the windows call's offsets.
 * -1, before any device work, for everything dq_hip_region_windows_dev refuses
 * (d_rows in the place of its d_offsets), a NULL d_rows, and cap > 0 with all
 * three entry arrays NULL.  -2 and -3 as the windows call (T > P; P or M
 * saturated); -3 also when the call's own contribution count Q reaches
 * 2^32 - 1, Q = the sum over the pairs (block b, member id r) of the windows
 * stage of the distinct ids with a surviving pixel in b.  All decided before
 * any output array is written.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): the windows call's (its lists
 * are never built); 4 B per block + 4 B per 1024 blocks + 4 B; 4 B per pair
 * (the member ids); then, with Q (read back with P and T), 16 B per slot of a hash
 * table of the entries, slots = 2 Q (>= 1024, below 2^32); 8 B per 32
 * list entries (one bit per list position and the rank of every word of them)
 * + 4 B per 32768 + 24 B; 12 B per region; 4 (nregions + 1) B when d_offsets
 * is NULL.  E is read back as well.  The table is sized from Q with no upper
 * bound: like every allocation of the library, one that fails aborts the
 * process with a message (a map of single-pixel regions without the area rule
 * can ask for tens of GB). */
int64_t dq_hip_window_tags_dev(int device, const uint32_t *d_regions, uint32_t width,
                               uint32_t height, uint32_t nregions, uint32_t block,
                               uint32_t expand, const uint8_t *d_mask, const uint32_t *d_area,
                               uint32_t min_area, uint32_t *d_rows /* nregions + 1 */,
                               uint32_t cap, uint32_t *d_ids, uint32_t *d_counts,
                               uint32_t *d_first, uint32_t *d_inside, uint32_t *d_best,
                               uint32_t *d_best_count, uint32_t *d_offsets /* may be NULL */,
                               void *stream);
/* Host pointers, the current device.  A call that returns < 0 leaves them as
 * they were; E > cap leaves the entry arrays as they were. */
int64_t dq_hip_window_tags(const uint32_t *regions, uint32_t width, uint32_t height,
                           uint32_t nregions, uint32_t block, uint32_t expand,
                           const uint8_t *mask, const uint32_t *area, uint32_t min_area,
                           uint32_t *rows, uint32_t cap, uint32_t *ids, uint32_t *counts,
                           uint32_t *first, uint32_t *inside, uint32_t *best,
                           uint32_t *best_count, uint32_t *offsets);
/* The inside / outside votes of every window's quant.  d_regions: n region
 * ids; d_offsets (nregions + 1), d_index and total (= M): the windows call's;
 * d_mapped: M words, the d_out of dq_hip_quant_region_windows_dev; cts
 * (nregions * k) and k_outs (nregions): HOST arrays as that call returns them,
 * uploaded by this call in stream order; 1 <= k <= 256 (the reference asserts
 * <= 256, :1962).  For j in the list of r: side = 0 if
 * d_regions[d_index[j]] == r, else 1; i = the lowest i < k_outs[r] with
 * ((cts[r * k + i] ^ d_mapped[j]) & 0xFFFFFF) == 0;
 * d_votes[(2 r + side) * k + i] += 1.  An entry with no such i (or with a
 * d_index[j] >= n) is a miss and is counted in no bin.  d_votes: nregions * 2
 * * k words, all written, zeros included.  d_best: nregions * 2 words, per
 * side the lowest i with the largest non-zero count (insideQuantPixel /
 * outsideQuantPixel are cts[r * k + that]), 0xFFFFFFFF when the side has no
 * vote.  Returns the number of misses (0 on the pipeline's own outputs),
 * synchronous on return.  -1, before any device work, for a NULL or misaligned
 * array (d_index and d_mapped may be NULL when total is 0), k outside 1..256,
 * nregions 0 or above 2^31 - 1, n 0 or above 2^31 - 1, total 2^32 - 1.
 * Scratch, in stream order, no engine state: the device copies of cts and
 * k_outs, 4 B per region + 4 B per 1024 regions + 24 B.  A list is cut into
 * jobs of 2048 entries, one wave each.  There is no host-pointer twin: the
 * call consumes device arrays that only the device pipeline produces. */
int64_t dq_hip_window_votes_dev(int device, const uint32_t *d_regions, uint32_t n,
                                uint32_t nregions, const uint32_t *d_offsets,
                                const uint32_t *d_index, uint32_t total, const uint32_t *d_mapped,
                                const uint32_t *cts /* host, nregions * k */,
                                const uint32_t *k_outs /* host, nregions */, uint32_t k,
                                uint32_t *d_votes /* nregions * 2 * k */,
                                uint32_t *d_best /* nregions * 2 */, void *stream);

/* ---- containment tree (region map + its graph -> which region lies in which,
 * and the inside-out order to visit them in) ------------------------------------
 * The reference's clusteringCombine does not visit regions in id order.  It
 * builds a containment tree of the tag image (recurseSuperpixelContainment,
 * ClusteringSegmentation.cpp:8545-8814: the roots are the tags that touch the
 * image border, a tag's children the tags nested one step further in) and walks
 * it inside-out, most deeply contained first (recurseSuperpixelIterate and a
 * stack), handing every visit a mask of the pixels consumed so far: the optional
 * d_mask of dq_hip_region_windows_dev.  The reference's tree is a depth-first
 * claim: a visited tag claims all its unprocessed neighbours and blocks later
 * siblings while it recurses, and its sibling order is an accident of an
 * unstable sort over an unordered_set.  These entries build the data-parallel
 * counterpart with ONE exact integer answer that does not depend on scheduling.
 * Inputs.  d_regions: a width x height map of uint32 ids, each < nregions = R
 * (any id map; dq_hip_label_regions_dev's is the intended one; an id >= R is
 * passed over).  d_area[R].  nedges id pairs d_edges, (a, b) with a != b and
 * both < R: the order within a pair, the order of the pairs and duplicates do
 * not matter (the d_edges of dq_hip_region_adjacency_dev is the intended list;
 * its connectivity is the caller's choice; a pair that is no such pair is
 * skipped).
 * Rules.
 *   1 Roots.  r is a root when some pixel of r lies in row 0, row height - 1,
 *     column 0 or column width - 1.  depth[r] = 0.
 *   2 Depth.  Otherwise depth[r] = 1 + the lowest depth among r's neighbours in
 *     the edge list: the breadth-first distance from the roots.  An id no root
 *     reaches is an ORPHAN (ids absent from the map, ids the edge list does not
 *     connect): depth = parent = pos = 0xFFFFFFFF, subtree = 0, enclosed = 0,
 *     left out of roots, children and order.
 *   3 Parent.  A root's parent is 0xFFFFFFFF.  For depth[r] > 0 the parent is,
 *     among the neighbours q with depth[q] = depth[r] - 1, the one with the
 *     highest area[q], ties to the lowest id (the reference walks larger regions
 *     first, and the first to arrive claims).
 *   4 Size order.  All R ids by area decreasing, ties by id increasing (the
 *     reference's sortSuperpixelsBySize with its ties made definite);
 *     rank[r] is r's position in it.
 *   5 roots[0 .. nroots) are the roots in size order;
 *     children[child_offsets[p] .. child_offsets[p + 1]) the regions whose
 *     parent is p, in size order; child_offsets has R + 1 words and
 *     child_offsets[R] = reached - nroots.
 *   6 subtree[r] = 1 + the sum of subtree over r's children; enclosed[r]
 *     (uint64) = area[r] + the sum of enclosed over its children.
 *   7 Inside-out order.  order[0 .. reached) is the post-order of the forest:
 *     the roots in root order, for each the subtrees of its children in sibling
 *     order, then the region itself.  It equals what the reference's reversed
 *     pre-order walk plus stack pop produces (ClusteringSegmentation.hpp:99-111,
 *     ClusteringSegmentationMain.cpp:223-250): a pre-order over reversed sibling
 *     lists, read backwards, is the post-order over forward lists.  In closed
 *     form block(root i) = the sum of subtree of the roots before it,
 *     block(child) = block(parent) + the sum of subtree of its earlier
 *     siblings, pos[r] = block(r) + subtree[r] - 1 and order[pos[r]] = r.
 * Agreement with the reference.  Call a map NESTED when every reached non-root
 * region touches exactly one region of lower depth and no region of its own
 * depth that has a different parent (rings, islands in islands, every case of
 * Test/ContainmentTest.mm).  On nested maps parent[] and the set of roots equal
 * the reference's containsTreeMap and rootTags whatever its sibling order
 * happens to be.  On other maps they can differ: there the reference's answer
 * hangs on the order in which its depth-first walk happens to claim, which
 * nothing exact can be pinned to.
 * Outputs, every pointer may be NULL, arrays sized by R so that no count is
 * needed first, nothing behind the entries in use written: d_depth, d_parent,
 * d_subtree, d_pos (R words), d_enclosed (R uint64), d_roots (nroots entries
 * written), d_child_offsets (R + 1), d_children (reached - nroots; needs
 * d_child_offsets), d_order (reached).  *levels (host, may be NULL) = 1 + the
 * highest depth reached; *reached (host, may be NULL) = the non-orphans.
 * Returns nroots >= 1, synchronous on return.  -1, before any device work, for:
 * NULL d_regions or d_area; nedges > 0 with NULL d_edges; width or height 0 or
 * above 65535; nregions == 0 or above width * height; a pointer not naturally
 * aligned (4 B; 8 B for d_enclosed); d_children without d_child_offsets.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): 68 B per region plus 1 KiB per
 * 1024 regions, nothing per edge; every output is computed there and the ones
 * asked for are copied out.  The host reads 8 bytes back per level (the regions
 * reached so far); a tree of D levels costs about 3 D + 40 launches. */
int64_t dq_hip_region_containment_dev(int device, const uint32_t *d_regions, uint32_t width,
                                      uint32_t height, uint32_t nregions, const uint32_t *d_area,
                                      uint32_t nedges, const uint32_t *d_edges /*2 per edge*/,
                                      uint32_t *d_depth, uint32_t *d_parent,
                                      uint32_t *d_roots, uint32_t *d_child_offsets /*R + 1*/,
                                      uint32_t *d_children, uint32_t *d_subtree,
                                      uint64_t *d_enclosed, uint32_t *d_order, uint32_t *d_pos,
                                      uint32_t *levels /*host, may be NULL*/,
                                      uint32_t *reached /*host, may be NULL*/, void *stream);
/* The same on host arrays, the current device: one upload (map, areas, edges),
 * the call above, one download of the arrays asked for (as many entries of
 * roots, children and order as are in use).  Same returns. */
int64_t dq_hip_region_containment(const uint32_t *regions, uint32_t width, uint32_t height,
                                  uint32_t nregions, const uint32_t *area, uint32_t nedges,
                                  const uint32_t *edges, uint32_t *depth, uint32_t *parent,
                                  uint32_t *roots, uint32_t *child_offsets, uint32_t *children,
                                  uint32_t *subtree, uint64_t *enclosed, uint32_t *order,
                                  uint32_t *pos, uint32_t *levels, uint32_t *reached);
/* Rule 4 alone: d_order[i] = the id at position i of the size order, d_rank[id]
 * = its position (either may be NULL, not both).  A stable LSD radix sort over
 * the area bits in use; the host reads 4 bytes back (the OR of the areas).
 * Returns 0, synchronous on return; -1, before any device work, for NULL
 * d_area, nregions == 0, both outputs NULL or a misaligned pointer.  Scratch in
 * stream order, no engine state: 20 B per region plus 1 KiB per 1024 regions. */
int dq_hip_regions_by_size_dev(int device, uint32_t nregions, const uint32_t *d_area,
                               uint32_t *d_order, uint32_t *d_rank, void *stream);

/* ---- region distance (region map -> the L1 distance of every pixel to the
 * nearest pixel of another id, every region's centre and its core) --------------
 * The last live step of the reference's captureRegion
 * (ClusteringSegmentation.cpp:2538-2679): once the votes have switched the mask
 * pixels on it takes the Manhattan distance transform of the mask
 * (findRegionCenter, superpixels/OpenCVUtil.cpp:204-618: Meijster's algorithm
 * with ManhattanMetric), picks one centre among the pixels of highest distance
 * and flood-fills 8-connected from it, switching off what the fill did not
 * reach.  These entries do the same for ALL regions of an id map in one call,
 * with ONE exact integer answer that does not depend on scheduling.
 * Inputs.  d_regions: a width x height map of uint32 ids.  An id < nregions = R
 * is a region; its pixels need not be connected.  An id >= R is background: it
 * has distance 0, no stats, and counts as "another id" for its neighbours.
 * Rules.
 *   1 Distance.  For a pixel p of region r, D(p) is the smallest |dx| + |dy| to
 *     any pixel whose id is not r, or to any position just outside the frame
 *     (column -1 or width, row -1 or height).  So D >= 1 on every region pixel
 *     and D <= 32768 under the argument limits: exactly what the reference
 *     computes for one mask inside its 1-pixel black border.
 *   2 Per region.  dmax[r] is the highest D of r; bbox[r] = (x0, y0, x1, y1),
 *     inclusive, the layout of dq_hip_label_regions_dev's d_bbox.  An id with no
 *     pixel has dmax = 0, count = 0, thresh = 0, centre = 0xFFFFFFFF,
 *     core_area = 0 and bbox = (0xFFFFFFFF, 0xFFFFFFFF, 0, 0).
 *   3 Threshold.  rule = 0 (exact): thresh[r] = dmax[r].  rule = 1 (the
 *     reference's 8-bit scale): thresh[r] is the lowest d in 1 .. dmax with
 *     byte(d) == byte(dmax), where byte(1) = 1 and otherwise
 *     byte(d) = max(1, (uint8)(sqrt((double)d) / (double)radius * 255 + 0.5)),
 *     evaluated in FP64 in exactly this order, and
 *     radius = isqrt(((bw + 2)^2 + (bh + 2)^2) >> 2) + 1 for a bbox of bw x bh
 *     pixels: the reference's int(round(hypot((bw+2)/2, (bh+2)/2) + 0.5) + 0.01).
 *     byte is monotone in d.  The reference's normalize(NORM_MINMAX) plus
 *     threshold(254) keeps exactly the pixels with byte(D) == byte(dmax).
 *   4 Centre set.  S[r] = { p of r : D(p) >= thresh[r] }; count[r] = |S|; the
 *     sums of x and of y over S are uint64.
 *   5 Centre, as the Coord word x | y << 16.  If count <= 2: the leftmost pixel
 *     of S in the last row that holds one (the reference's loop breaks out of
 *     its inner loop only, OpenCVUtil.cpp:545-553).  Otherwise
 *     c = (sum x / count, sum y / count) in integer division (frame coordinates
 *     give the same c as the reference's padded ROI coordinates); if c is in S
 *     the centre is c, else the pixel of S with the lowest dx^2 + dy^2 to c,
 *     ties to the lowest raster index.  This equals the reference's float hypot
 *     with strict < in raster order wherever that lowest distance is under 2048
 *     pixels: there distinct integers dx^2 + dy^2 give distinct floats.  Beyond
 *     2048 pixels the reference's ties hang on float rounding and can differ.
 *   6 Core.  Take the components of equal ids under `connectivity` 4 or 8 (the
 *     reference's flood uses 8).  core(p) = 1 iff p is a region pixel in the
 *     component of centre[id(p)]; d_cored[p] = the id there, else 0xFFFFFFFF;
 *     core_area[r] the number of such pixels.
 * Outputs: every pointer may be NULL (not all of them); arrays are sized by
 * width * height or by R, nothing behind them is written.  d_cored may be
 * d_regions itself (in place: a pixel's id is read before its word is written,
 * and components come from a copy); no other output may overlap the map.
 * dq_hip_region_distance_dev returns 0, dq_hip_region_cores_dev the pixels kept
 * (the sum of core_area); both are synchronous on return.  -1, before any device
 * work, for: NULL d_regions; width or height 0 or above 65535; width * height
 * above 2^31 - 1; nregions == 0; rule not 0 or 1; connectivity not 4 or 8; a
 * pointer not naturally aligned (2 B for d_dist, 4 B for the words); every
 * output NULL.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): 2.25 B per pixel and 32 B per
 * region, plus 2 B per pixel without d_dist and 4 to 16 B per region for each
 * per-region output left NULL (the distance call: 11 launches, no read-back).
 * The cores call adds 8 B per pixel (the components and their union-find) and
 * 4 B per region without d_core_area: 19 launches, 4 bytes read back. */
int dq_hip_region_distance_dev(int device, const uint32_t *d_regions, uint32_t width,
                               uint32_t height, uint32_t nregions, int rule,
                               uint16_t *d_dist /*W*H*/, uint32_t *d_dmax,
                               uint32_t *d_bbox /*4 per region*/, uint32_t *d_thresh,
                               uint32_t *d_count, uint32_t *d_centre, void *stream);
int64_t dq_hip_region_cores_dev(int device, const uint32_t *d_regions, uint32_t width,
                                uint32_t height, uint32_t nregions, int rule, int connectivity,
                                uint8_t *d_core /*W*H*/,
                                uint32_t *d_cored /*W*H: id or 0xFFFFFFFF*/,
                                uint32_t *d_centre, uint32_t *d_core_area, uint16_t *d_dist,
                                void *stream);
/* The same on host arrays, the current device: one upload of the map, the call
 * above, one download of the arrays asked for.  Same returns. */
int dq_hip_region_distance(const uint32_t *regions, uint32_t width, uint32_t height,
                           uint32_t nregions, int rule, uint16_t *dist, uint32_t *dmax,
                           uint32_t *bbox, uint32_t *thresh, uint32_t *count, uint32_t *centre);
int64_t dq_hip_region_cores(const uint32_t *regions, uint32_t width, uint32_t height,
                            uint32_t nregions, int rule, int connectivity, uint8_t *core,
                            uint32_t *cored, uint32_t *centre, uint32_t *core_area,
                            uint16_t *dist);

/* ---- region skeleton (region map -> the one-pixel-wide skeleton of every
 * region, by Guo-Hall two-subiteration thinning) -------------------------------
 * The live body of the reference's captureRegion, clockwiseScanForShapeBounds
 * (ClusteringSegmentation.cpp:1276-1306), renders each visited region into a
 * frame-sized mask and thins it (ClusteringSegmentation.cpp:6303-6321 ->
 * skelReduce, superpixels/OpenCVUtil.cpp:1619 -> NormalizeLetter, :1548-1617 ->
 * ThinSubiteration1 / ThinSubiteration2, :1458-1546).  This entry does the same
 * for ALL regions of an id map in one call.  Regions are disjoint and a pixel's
 * neighbour counts only when it has the pixel's own id, so every region gets
 * exactly the bits the reference gets from that region's mask alone: ONE exact
 * answer that does not depend on scheduling.
 * Inputs.  d_regions: a width x height map of uint32 ids.  An id < nregions = R
 * is a region; its pixels need not be connected.  An id >= R is background.
 * max_iters: 0 runs until nothing is deleted any more.
 * Rules.
 *   1 Neighbours.  For a pixel p of region r: n0 = NW, n1 = N, n2 = NE, n3 = E,
 *     n4 = SE, n5 = S, n6 = SW, n7 = W.  n_k = 1 iff that position lies in the
 *     frame, has id r and is still alive; else 0 (the reference's mask has a
 *     1-pixel border of zeros, and another region is not in the mask).
 *   2 Counts.  C  = (!n1 & (n2|n3)) + (!n3 & (n4|n5)) + (!n5 & (n6|n7)) +
 *     (!n7 & (n0|n1)); N1 = (n0|n1) + (n2|n3) + (n4|n5) + (n6|n7);
 *     N2 = (n1|n2) + (n3|n4) + (n5|n6) + (n7|n0); N = min(N1, N2).
 *   3 Subiteration 1 deletes every alive p with C == 1, N in {2, 3} and
 *     ((n1 | n2 | !n4) & n3) == 0; subiteration 2 the same with
 *     ((n5 | n6 | !n0) & n7) == 0.  A subiteration decides for all pixels from
 *     the state before it.  (The reference writes ~ on 0/1 ints; under its & with
 *     a 0/1 value that is the logical not.)
 *   4 Iterations.  An iteration is subiteration 1, then subiteration 2 on its
 *     result; iterations count from 1.  The run stops after the first iteration
 *     that deletes nothing (converged = 1; the reference's stop rule), after
 *     max_iters iterations when max_iters > 0, and after 65535 in any case; in the
 *     last two cases converged = 1 only if the last iteration that ran deleted
 *     nothing.  *iterations = the number of the last iteration that deleted a
 *     pixel, 0 if none did.
 *   5 Outputs.  skel[p] = 1 iff p is a region pixel still alive, else 0;
 *     skeled[p] = the id there, else 0xFFFFFFFF; when[p] = the iteration that
 *     deleted p, 0 for a pixel kept and for background; skel_area[r] = the alive
 *     pixels of r; thick[r] = the highest when over r, 0 if r lost nothing.  An id
 *     with no pixel has skel_area = 0 and thick = 0.
 * Outputs: every array pointer may be NULL (not all five); arrays are sized by
 * width * height or by R, nothing behind them is written.  iterations and
 * converged are host words and may be NULL.  d_skeled may be d_regions itself
 * (in place: the ids are read by one pass before the first thinning step, and
 * at the end each pixel's id is read before its word is written); no other
 * output may overlap the map.  Returns the pixels kept (the sum of skel_area),
 * synchronous on return.  -1, before any device work, for: NULL d_regions;
 * width or height 0 or above 65535; width * height above 2^31 - 1;
 * nregions == 0; max_iters > 65535; a pointer not naturally aligned (2 B for
 * d_when, 4 B for the words); every output array NULL.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): 0.75 B per pixel (six bit planes,
 * rows padded to 64 pixels), 8 B per tile of 384 x 64 pixels and 16 KB; nothing
 * per region; plus 2 B per pixel when d_thick is given without d_when.
 * Launches: 3 + one per 16 iterations (sent in groups of 2, 4, then 8 at a time;
 * those past the end cost a flag test per tile); read-backs: one per group (4 B a
 * launch) and the pixels kept. */
int64_t dq_hip_region_skeleton_dev(int device, const uint32_t *d_regions, uint32_t width,
                                   uint32_t height, uint32_t nregions, uint32_t max_iters,
                                   uint8_t *d_skel /*W*H*/,
                                   uint32_t *d_skeled /*W*H: id or 0xFFFFFFFF*/,
                                   uint16_t *d_when /*W*H*/, uint32_t *d_skel_area,
                                   uint32_t *d_thick, uint32_t *iterations, uint32_t *converged,
                                   void *stream);
/* The same on host arrays, the current device: one upload of the map, the call
 * above, one download of the arrays asked for.  Same returns. */
int64_t dq_hip_region_skeleton(const uint32_t *regions, uint32_t width, uint32_t height,
                               uint32_t nregions, uint32_t max_iters, uint8_t *skel,
                               uint32_t *skeled, uint16_t *when, uint32_t *skel_area,
                               uint32_t *thick, uint32_t *iterations, uint32_t *converged);

/* ---- region contours (region map -> the ordered border pixels of every region,
 * by border following) ---------------------------------------------------------
 * The first thing the reference's clockwiseScanForShapeBounds does with a
 * visited region (ClusteringSegmentation.cpp:5856 -> clockwiseScanOfHullCoords,
 * superpixels/OpenCVHull.cpp:280-360 -> findContourOutline, :69-274): it renders
 * the region into a frame-sized mask, takes findContours(RETR_LIST,
 * CHAIN_APPROX_NONE) of the mask inside a 1-pixel border of zeros, subtracts
 * (1, 1) from every point and reverses the list (:329-337).  This entry does
 * the same for ALL regions of an id map in one call.  The rules are OpenCV
 * 3.1's border-following loop for an outer border, written out: ONE exact
 * answer per region that does not depend on scheduling.
 * Inputs.  d_regions: a width x height map of uint32 ids.  An id < nregions = R
 * is a region; its pixels need not be connected.  An id >= R is background.
 * on_r(q) = q lies in the frame and id(q) == r; outside the frame counts as off
 * (the reference's border of zeros; coordinates are frame coordinates, i.e.
 * after its - (1, 1)).
 * Rules.
 *   1 Directions, y down: 0 = E (1,0), 1 = NE (1,-1), 2 = N (0,-1),
 *     3 = NW (-1,-1), 4 = W (-1,0), 5 = SW (-1,1), 6 = S (0,1), 7 = SE (1,1).
 *   2 Start.  p0[r] = the pixel of r with the lowest raster index (its W, NW, N
 *     and NE neighbours are off).  d0 = the first of E, SE, S, SW (0, 7, 6, 5)
 *     whose neighbour is on: OpenCV's clockwise search from s = 4.  If none is
 *     on, the contour is [p0], len = 1.
 *   3 Step.  A state is (p, d): a pixel p of r and a direction d whose neighbour
 *     p + delta[d] is on ("the pixel we came from").  step(p, d): s = the first
 *     of d + 1, d + 2, ... (mod 8) with on_r(p + delta[s]); the step emits point
 *     p with code s and goes to state (p + delta[s], (s + 4) & 7).
 *   4 Contour.  step from (p0, d0) until it is the start state again; the points
 *     emitted, in that order, are findContours' outer border of the 8-connected
 *     component that holds p0: counter-clockwise on the screen, starting at p0.
 *     A pixel can appear more than once (a one-pixel spur is walked out and
 *     back).  len[r] = the number of points, 0 for an id with no pixel.  Only the
 *     component of p0 is traced and only its outer border: holes and further
 *     components of an id are not (the reference asserts there are none,
 *     OpenCVHull.cpp:134-184).
 *   5 Orientation.  0: the list as in rule 4.  1: the reference's reversal,
 *     point'[i] = point[len - 1 - i], what clockwiseScanOfHullCoords hands on.
 *     In both, code[i] = the direction from point i to point (i + 1) mod len;
 *     code[i] = 8 when len == 1.
 *   6 Outputs.  offsets[0 .. R]: the exclusive prefix sum of len, offsets[R] = M;
 *     points[offsets[r] + i]: the Coord word x | y << 16; codes: u8 per point;
 *     len[r]; visits[p]: u8 per pixel, how often p appears in its own region's
 *     contour, 0 for background.
 * Returns M, synchronous on return.  d_points and d_codes are written only when
 * M <= point_cap; with point_cap = 0 and both NULL the call only counts (offsets,
 * len and visits are still written).  -2, with only d_len written, when M does
 * not fit below 2^32 - 1.  -3, with nothing written, when the border pixels of
 * the map have more than 2^32 - 2 on neighbours in all (the states the call
 * numbers; no map below 2^29 pixels has).  -1, before any device work, for: NULL
 * d_regions; width or height 0 or above 65535; width * height above 2^31 - 1;
 * nregions == 0 or above 2^32 - 1025; orientation not 0 or 1; a word pointer
 * (d_regions, d_offsets, d_points, d_len) not 4-B aligned; every output NULL;
 * point_cap > 0 with both list pointers NULL.  Every output pointer may be NULL;
 * nothing behind an array's stated size is written; no output may overlap the map.
 * Scratch, allocated and freed in stream order by the call (no engine state is
 * touched: calls on two streams may overlap): 5 B per pixel (a neighbour byte
 * and the number of the pixel's first state), 12 B per region, 4 B per 1024
 * pixels or regions and 136 B; 16 B per state (two buffers of (next, distance)
 * words; a state is an on neighbour of a border pixel, a region pixel with a
 * 4-neighbour off: 2 to 3 per border pixel on a smooth map); plus 4 B per
 * region for each of d_len and d_offsets that is NULL.
 * Launches: 13 + one per pointer-jumping round; ceil(log2(the longest len - 1))
 * rounds are needed and one more sees that none is, sent 4, 4, then 8 at a time
 * (33 at most).  Read-backs: the states, one per group of rounds (4 B a round),
 * and M. */
int64_t dq_hip_region_contours_dev(int device, const uint32_t *d_regions, uint32_t width,
                                   uint32_t height, uint32_t nregions, int orientation,
                                   uint64_t point_cap, uint32_t *d_offsets /*R + 1*/,
                                   uint32_t *d_points /*point_cap*/,
                                   uint8_t *d_codes /*point_cap*/, uint32_t *d_len /*R*/,
                                   uint8_t *d_visits /*W*H*/, void *stream);
/* The same on host arrays, the current device: one upload of the map, the call
 * above, one download of the arrays asked for.  Same returns. */
int64_t dq_hip_region_contours(const uint32_t *regions, uint32_t width, uint32_t height,
                               uint32_t nregions, int orientation, uint64_t point_cap,
                               uint32_t *offsets, uint32_t *points, uint8_t *codes,
                               uint32_t *len, uint8_t *visits);

/* ---- BGR24 frames (OpenCV CV_8UC3: B, G, R bytes, `stride` bytes per row)
 * quant_recurse of device BGR24 frames without the packed conversion
 * (SURVEY 8f.3): with uniq = 1 and continuous rows (stride == 3*width) the
 * root's passes, its partition and the map read the 3-B pixels directly
 * (a frame whose pointer is not 16-B aligned or whose pixel count is not a
 * multiple of 16 is first copied to aligned scratch); padded rows or uniq = 0
 * (the weighted path's colour table) pack the frame on the GPU first.  d_out
 * gets packed 0x00RRGGBB colours (the reference's output format).  The batch
 * form runs every frame of a call over the engine lanes like
 * dq_hip_quant_batch_dev (ct: nframes * k, k_out: nframes).  Returns the
 * number of empty clusters or < 0. */
int dq_hip_quant_bgr24_batch_dev(int device, int nframes, const uint8_t *const *d_bgr,
                                 uint32_t width, uint32_t height, uint32_t stride,
                                 uint32_t *const *d_out, uint32_t k, uint32_t *ct,
                                 uint32_t *k_out, int uniq, int max_iters, void *stream);
int dq_hip_quant_bgr24_dev(int device, const uint8_t *d_bgr, uint32_t width, uint32_t height,
                           uint32_t stride, uint32_t *d_out, uint32_t *k, uint32_t *ct,
                           int uniq, int max_iters, void *stream);
/* map_colors_mps of a device BGR24 frame (read directly when K <= 1024 and
 * the rows are continuous) into packed colours. */
int dq_hip_map_bgr24_dev(int device, const uint8_t *d_bgr, uint32_t width, uint32_t height,
                         uint32_t stride, uint32_t *d_out, const uint32_t *ct, int k,
                         void *stream);

/* ---- diagnostics of the last clustering on `device` ----------------------
 * means: k*3 doubles (the reference's mean[ic] per cluster index, the north
 * star's "float centroids"); sizes: k cluster sizes; trace: (k-1)*4 of
 * new_index, old_index, |C|, |new| per split.  Return 0 or < 0. */
int dq_hip_last_centroids(int device, double *means, int64_t *sizes, int k);
int dq_hip_last_trace(int device, int64_t *trace, int k);
int dq_hip_last_rounds(int device);
/* Points read by all statistics passes of the last clustering. */
uint64_t dq_hip_last_points_swept(int device);
/* Points the last run would have swept without fixed-point finalisation
 * (every split: split pass + max_iters 2-means passes, as the reference). */
uint64_t dq_hip_last_points_full(int device);
/* Weighted path: tiles of the last run whose folds ran one summand at a time
 * (the exact parallel fold's fallback). */
uint64_t dq_hip_last_seq_tiles(int device);
/* Records of the last run finalised at a frame's last planned round (whose
 * partition counts no partition cursors) that a later round partitioned:
 * their cursors counted then. */
uint64_t dq_hip_last_cursor_fixes(int device);
/* Fixed-point finalisation (default on; DQ_HIP_TUNE=full_iters=1 turns the
 * default off).  A split whose 2-means pass reproduces the previous pass's exact
 * integer sums is final: the remaining iterations of the reference's loop
 * (DivQuantCluster.cpp:613) would recompute the same means and decision.
 * Outputs are identical either way; only the swept points differ. */
void dq_hip_set_fixed_point(int device, int on);
/* Device-planned rounds (default on; DQ_HIP_TUNE=plan=0 turns the default off):
 * while a frame may still need splits, the next round's tables are built on
 * the GPU from the current round's results and the round is enqueued before
 * the host has seen them.  Outputs are identical either way;
 * speculation may expand nodes the greedy replay never uses.
 * dq_hip_last_planned_rounds: how many rounds of the last run were planned. */
void dq_hip_set_planned_rounds(int device, int on);
int dq_hip_last_planned_rounds(int device);
/* One-launch 2-means loops: a round whose records all hold at
 * most max_points points (default 49152; DQ_HIP_TUNE=kloop_max=N) and that has at
 * most one record per CU runs all its 2-means iterations in one
 * kloop_kernel launch, one workgroup per record.  0 turns it off.  Outputs
 * are identical either way.  dq_hip_last_loop_rounds: how many rounds of the
 * last run did so. */
void dq_hip_set_loop_max(int device, uint32_t max_points);
int dq_hip_last_loop_rounds(int device);
/* One-launch 2-means loops over a round's tiles (default on,
 * DQ_HIP_TUNE=persist=0 turns the default off): a round kloop does not take,
 * of one shard per record, planar records and at most 4 tiles per CU (or,
 * once its split status is known, at most 4 tiles per CU of records still
 * active), runs all its 2-means iterations in one kpersist_kernel launch, a
 * record's workgroups meeting per iteration.  Outputs are identical either way.
 * dq_hip_last_persist_rounds: how many rounds of the last run did so. */
void dq_hip_set_persist(int device, int on);
int dq_hip_last_persist_rounds(int device);
/* The weighted path (allPixelsUnique = 0) of a small input -- at most 131071
 * pixels, 6144 colours, 64 clusters, no cut_bits / decimation: a superpixel
 * region of the app, ClusteringSegmentation.cpp:1779-1803 -- in ONE launch of
 * one workgroup (DESIGN.md 5d'; default on, DQ_HIP_TUNE=wsmall=0 turns the
 * default off): colour table, the splits in the reference's order with its
 * sequential folds, dedup and, for at most 16 deduped colours, the map.
 * Outputs are identical either way. */
void dq_hip_set_wsmall(int device, int on);
/* The map kernel of palettes of at most 1024 entries: on (the default;
 * DQ_HIP_TUNE=lds_map=0 turns the default off) -- map_lds_kernel, the compact
 * cell table in LDS; off -- map_kernel, the cell records gathered through L2,
 * which every larger palette and every misaligned buffer takes anyway.
 * Every lane of the device.  Outputs are identical either way. */
void dq_hip_set_lds_map(int device, int on);
/* Phase profile of the last weighted call if it took the one-launch path
 * (0 values otherwise): wall_clock64 ticks (100 MHz) at its start, hash set,
 * sorted colour table, clustering, map; ticks in fold passes and partitions;
 * passes by kind (init | split << 16 | 2-means << 32).  Returns the count. */
int dq_hip_last_wsmall_profile(int device, uint64_t* out, int nout);

/* Engine lanes a batch of frames is split over (each: own stream, own host
 * thread; DQ_HIP_LANES; default 4 when GPU_MAX_HW_QUEUES >= 6 at the first
 * batch call, else 3 -- HIP reads GPU_MAX_HW_QUEUES once, when it
 * initialises, so set it before any HIP call of the process).  lanes = 0
 * restores the default. */
void dq_hip_set_lanes(int lanes);
int dq_hip_get_lanes(void);

/* ---- per-kernel timing (HIP events on the launch stream) -----------------
 * kinds: 0 init pass, 1 split pass, 2 2-means pass, 3 last 2-means pass,
 * 4 epilogue, 5 partition, 6 map cells, 7 map, 8 plan.  bytes = the engine
 * work model's bytes (4 B per point read from the caller's
 * packed frame, 3 B per point read or written in the planar working
 * buffers, 8 B per mapped pixel); units = points (pixels) processed. */
void dq_hip_set_timing(int device, int on);
void dq_hip_reset_stats(int device);
int dq_hip_get_stat(int device, int kind, uint64_t *launches, double *ms,
                    double *bytes);
int dq_hip_get_stat_units(int device, int kind, double *units);
const char *dq_hip_stat_name(int kind);

/* ---- build identity and test-only knobs ----------------------------------
 * dq_hip_build_id: FNV-1a-64 of the sources the library was built from
 * (tools/source_id.py; a test compares it with the tree beside the .so).
 * dq_hip_set_debug: interleaving knobs for the hand-off tests (flags of
 * dq_kernels.h kDebug*: 1 prewarm the 2-means hand-off lines, 2 uneven
 * workgroup stalls, 4 host delays between status and results, 8 plan-kernel
 * stall, 16 abort unless the round arena is all zero when a run starts, 32
 * release the round arena at every run's start: new chunks); every
 * lane of `device`; 0 (the default) in production.  Outputs are identical
 * under every flag. */
uint64_t dq_hip_build_id(void);
void dq_hip_set_debug(int device, int flags);
/* Test-only: the row-tile sharding of nranks (1..8) processes, run by
 * nranks engines of THIS process on `device`, each with its own stream and
 * host thread, joined by an in-process loopback collective instead of RCCL
 * (the TOT_ALLREDUCE path with every rank's local counts != the global
 * totals).  Rank r holds rows [r*height/nranks, (r+1)*height/nranks) of every
 * frame (width x height, d_in / d_out whole frames), maps them into the same
 * rows of d_out and writes its colortables to ct + (r*nframes + i)*k, its
 * counts to k_out[r*nframes + i].  coll_log (nranks x log_cap, may be NULL)
 * gets the element count of each collective rank r enqueued, log_len[r] how
 * many it enqueued.  Synchronous; returns rank 0's empty clusters or -1. */
int dq_hip_loopback_rows_dev(int device, int nranks, int nframes, const uint32_t *const *d_in,
                             uint32_t width, uint32_t height, uint32_t *const *d_out,
                             uint32_t k, uint32_t *ct, uint32_t *k_out, int max_iters,
                             uint64_t *coll_log, int log_cap, int *log_len);

#ifdef __cplusplus
}
#endif

#endif /* DQ_HIP_H */
