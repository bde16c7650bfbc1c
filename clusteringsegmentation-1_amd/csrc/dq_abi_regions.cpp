// dq_abi_regions.cpp -- the region-map pipeline of the C ABI (include/dq_hip.h):
// regions, adjacency, merge, containment, distance and cores, skeletons, contours, pixel lists,
// capture windows, window tags and votes, and the per-region / per-window quant over them.
//
// Every stage has the same shape.  Both of its entry points fill the stage's
// argument struct of the launch layer (dq_*.h; what the call owns left NULL),
// args_ok(args) checks it -- host and device pointers alike, before the first
// HIP call -- and run_on(stream, args) enqueues the stage with scratch owned by
// the call and waits.  A host-pointer entry runs the stage on device twins of
// its arrays (Staging, dq_abi_util.h) and copies back what the stage wrote.
// No stage but the quant calls touches engine state: calls on two streams may
// overlap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/dq_hip.h"
#include "dq_abi_util.h"
#include "dq_adjacency.h"
#include "dq_contain.h"
#include "dq_contour.h"
#include "dq_distance.h"
#include "dq_merge.h"
#include "dq_pixels.h"
#include "dq_regions.h"
#include "dq_skeleton.h"
#include "dq_windows.h"
#include "dq_wtags.h"

using dq::Engine;
using dq::engine_for;
using dq::engine_stream;
using dq::Staging;

namespace {

using u64 = unsigned long long;   // (uint64_t in the ABI, unsigned long long in the kernels' structs)

bool aligned(std::initializer_list<const void*> ps, uintptr_t bytes = 4) {
  for (const void* p : ps)
    if (((uintptr_t)p & (bytes - 1)) != 0) return false;
  return true;
}

hipStream_t host_stream() { return engine_for(dq::current_device()).stream(); }

// -------------------------------------------------------------------------
// Connected regions of a label map (dq_regions.hip).
bool args_ok(const dq::RegionArgs& a) {
  if (a.label_bytes != 1 && a.label_bytes != 2 && a.label_bytes != 4) return false;
  if (a.connectivity != 4 && a.connectivity != 8) return false;
  if (a.width == 0 || a.height == 0 || a.width > 65535u || a.height > 65535u ||
      (uint64_t)a.width * a.height > 0x7FFFFFFFull)
    return false;
  if (!a.labels || !a.regions) return false;
  if (!aligned({a.labels}, (uintptr_t)a.label_bytes)) return false;
  if (!aligned({a.regions, a.area, a.bbox, a.first, a.label, a.pixels}) || !aligned({a.sums}, 8)) return false;
  if (a.sums && !a.pixels) return false;
  if (a.stats_cap > 0 && !a.area && !a.bbox && !a.first && !a.label && !a.sums) return false;
  return true;
}

// Enqueues the passes on st with scratch owned by the call, waits, returns R.
int64_t run_on(hipStream_t st, dq::RegionArgs a) {
  Staging s(st);
  a.scratch = s.alloc<uint32_t>(dq::region_scratch_words(a.width, a.height));
  dq::launch_label_regions(a, st);
  uint32_t count = 0;
  s.fetch(&count, dq::region_count_word(a));
  s.finish();
  return (int64_t)count;
}

// -------------------------------------------------------------------------
// Region adjacency graph of a region map (dq_adjacency.hip).  nregions: the
// words of `degree`.
bool args_ok(const dq::AdjacencyArgs& a, uint32_t nregions) {
  if (a.connectivity != 4 && a.connectivity != 8) return false;
  // n <= 2^30: a contact is the one word 4 * p + dir, and E < 4 n fits uint32
  if (a.width == 0 || a.height == 0 || a.width > 65535u || a.height > 65535u ||
      (uint64_t)a.width * a.height > DQ_HIP_ADJACENCY_MAX_PIXELS)
    return false;
  if (!a.regions) return false;
  if (!aligned({a.regions, a.edges, a.border, a.contact, a.pixels, a.degree}) || !aligned({a.step}, 8)) return false;
  if (a.step && !a.pixels) return false;
  if (a.edge_cap > 0 && !a.edges && !a.border && !a.contact && !a.step) return false;
  if (a.degree && nregions == 0) return false;
  return true;
}

// Enqueues both halves on st with scratch owned by the call, waits, returns E.
// One small read-back sits between the halves: the table is sized from the
// heads the first half counted.
int64_t run_on(hipStream_t st, dq::AdjacencyArgs a, uint32_t nregions) {
  Staging s(st);
  a.counts = s.alloc<uint32_t>(dq::adjacency_count_words(a.width, a.height));
  if (a.degree) DQ_HIP(hipMemsetAsync(a.degree, 0, (size_t)nregions * 4, st));
  dq::launch_adjacency_count(a, st);
  const uint32_t heads = s.read_word(dq::adjacency_heads_word(a));
  uint32_t count = 0;
  if (heads != 0) {   // (no head: no contact, no edge)
    a.table = s.alloc_bytes(dq::adjacency_scratch_bytes(heads, a.step != nullptr));
    dq::launch_adjacency_build(a, heads, st);
    s.fetch(&count, dq::adjacency_edges_word(a));
  }
  s.finish();
  return (int64_t)count;
}

// -------------------------------------------------------------------------
// Region merge over the adjacency graph (dq_merge.hip).
bool args_ok(const dq::MergeArgs& a) {
  if (!a.regions || !a.area || !a.first || !a.sums || !a.out_regions) return false;
  if (a.n == 0 || a.n > 0x7FFFFFFFu) return false;
  if (a.nregions == 0 || a.nregions > a.n) return false;
  if (a.nedges > 0 && !a.edges) return false;
  if (!aligned({a.regions, a.area, a.first, a.bbox, a.edges, a.out_regions, a.remap, a.out_area, a.out_bbox,
                a.out_first}) ||
      !aligned({a.sums, a.out_sums}, 8))
    return false;
  if (a.out_bbox && !a.bbox) return false;
  if (a.stats_cap > 0 && !a.out_area && !a.out_bbox && !a.out_first && !a.out_sums) return false;
  return true;
}

// Enqueues the rounds on st with scratch owned by the call, waits, returns R'.
// The host reads the links of a round back (4 bytes) and stops at 0.
int64_t run_on(hipStream_t st, dq::MergeArgs a, uint32_t max_rounds, uint32_t* rounds) {
  Staging s(st);
  a.scratch = s.alloc_bytes(dq::merge_scratch_bytes(a.n, a.nregions, a.bbox != nullptr, a.remap != nullptr));
  dq::launch_merge_init(a, st);
  uint32_t done = 0;
  // Every counted round makes a link, i.e. removes at least one component: fewer than nregions rounds,
  // so the loop ends by itself.  (Without a distance limit the restless components at least halve per
  // round; with one, a component may get its first offer only after a neighbour's mean has moved, and
  // a star of such leaves takes a round per leaf.)
  while (a.nedges != 0 && a.min_area != 0 && (max_rounds == 0 || done < max_rounds)) {
    dq::launch_merge_choose(a, st);
    if (s.read_word(dq::merge_links_word(a)) == 0) break;
    dq::launch_merge_fold(a, st);
    ++done;
  }
  DQ_HIP(dq::launch_merge_finish(a, st));
  uint32_t count = 0;
  s.fetch(&count, dq::merge_count_word(a));
  s.finish();
  if (rounds) *rounds = done;
  return (int64_t)count;
}

// -------------------------------------------------------------------------
// Containment tree of a region map (dq_contain.hip).  The outputs (device or
// host arrays, each optional):
struct ContainOut {
  uint32_t *depth, *parent, *roots, *child_offsets, *children, *subtree;
  uint64_t* enclosed;
  uint32_t *order, *pos;
};

bool args_ok(const dq::ContainArgs& a, const ContainOut& to) {
  if (!a.regions || !a.area) return false;
  if (a.nedges > 0 && !a.edges) return false;
  if (a.width == 0 || a.height == 0 || a.width > 65535u || a.height > 65535u) return false;
  if (a.nregions == 0 || a.nregions > (uint64_t)a.width * a.height) return false;
  if (!aligned({a.regions, a.area, a.edges, to.depth, to.parent, to.roots, to.child_offsets, to.children, to.subtree,
                to.order, to.pos}) ||
      !aligned({to.enclosed}, 8))
    return false;
  if (to.children && !to.child_offsets) return false;
  return true;
}

// Enqueues the stages on st with scratch owned by the call, copies what is
// wanted to `to` (device or host arrays: `kind`), waits, returns nroots.  The
// host reads the regions reached back once per level (8 bytes) and stops at a
// level that reached nobody.
int64_t run_on(hipStream_t st, dq::ContainArgs a, const ContainOut& to, hipMemcpyKind kind, uint32_t* levels,
               uint32_t* reached) {
  Staging s(st);
  a.scratch = s.alloc_bytes(dq::contain_scratch_bytes(a.nregions));
  dq::launch_contain_roots(a, st);
  uint32_t words[2] = {0, 0};   // reached so far, the OR of the areas
  s.fetch(words, dq::contain_counters(a), 2);
  s.sync();
  const uint32_t nroots = words[0], area_bits = dq::sort_key_bits(words[1]);
  // Every level but the last reaches at least one region: at most nregions levels, the loop ends by itself.
  uint32_t nlevels = 1, have = nroots;
  while (a.nedges != 0 && have < a.nregions) {
    dq::launch_contain_level(a, nlevels, st);
    s.fetch(words, dq::contain_counters(a), 2);
    s.sync();
    if (words[0] == have) break;
    have = words[0];
    ++nlevels;
  }
  dq::launch_contain_tree(a, nlevels, nroots, have, area_bits, st);
  DQ_HIP(hipGetLastError());
  const dq::ContainResults r = dq::contain_results(a);
  const size_t R = a.nregions, nchildren = have - nroots;
  // nothing behind the entries in use is written
  if (to.depth) DQ_HIP(hipMemcpyAsync(to.depth, r.depth, R * 4, kind, st));
  if (to.parent) DQ_HIP(hipMemcpyAsync(to.parent, r.parent, R * 4, kind, st));
  if (to.roots && nroots) DQ_HIP(hipMemcpyAsync(to.roots, r.sequence, (size_t)nroots * 4, kind, st));
  if (to.child_offsets) DQ_HIP(hipMemcpyAsync(to.child_offsets, r.child_offsets, (R + 1) * 4, kind, st));
  if (to.children && nchildren) DQ_HIP(hipMemcpyAsync(to.children, r.sequence + nroots, nchildren * 4, kind, st));
  if (to.subtree) DQ_HIP(hipMemcpyAsync(to.subtree, r.subtree, R * 4, kind, st));
  if (to.enclosed) DQ_HIP(hipMemcpyAsync(to.enclosed, r.enclosed, R * 8, kind, st));
  if (to.order && have) DQ_HIP(hipMemcpyAsync(to.order, r.order, (size_t)have * 4, kind, st));
  if (to.pos) DQ_HIP(hipMemcpyAsync(to.pos, r.pos, R * 4, kind, st));
  s.finish();
  if (levels) *levels = nlevels;
  if (reached) *reached = have;
  return (int64_t)nroots;
}

// -------------------------------------------------------------------------
// Distance transform, centres and cores of a region map (dq_distance.hip).
// The outputs of the cores call beside the distance call's (each optional):
struct CoresOut {
  uint8_t* core;
  uint32_t *cored, *core_area;
};

bool args_ok(const dq::DistanceArgs& a) {
  if (!a.regions) return false;
  if (a.width == 0 || a.height == 0 || a.width > 65535u || a.height > 65535u ||
      (uint64_t)a.width * a.height > 0x7FFFFFFFull)
    return false;
  if (a.nregions == 0 || (a.rule != 0 && a.rule != 1)) return false;
  return aligned({a.regions, a.dmax, a.bbox, a.thresh, a.count, a.centre}) && aligned({a.dist}, 2);
}

bool args_ok(const dq::DistanceArgs& a, const CoresOut& to, int connectivity) {
  if (!args_ok(a) || (connectivity != 4 && connectivity != 8)) return false;
  if (!to.core && !to.cored && !to.core_area && !a.centre && !a.dist) return false;
  return aligned({to.cored, to.core_area});
}

bool no_output(const dq::DistanceArgs& a) { return !a.dist && !a.dmax && !a.bbox && !a.thresh && !a.count && !a.centre; }

// Enqueues the distance launches on st: what the caller left NULL is scratch of `s`.
void distance_on(Staging& s, dq::DistanceArgs& a) {
  const size_t n = (size_t)a.width * a.height, R = a.nregions;
  if (!a.dist) a.dist = s.alloc<uint16_t>(n);
  if (!a.dmax) a.dmax = s.alloc<uint32_t>(R);
  if (!a.bbox) a.bbox = s.alloc<uint32_t>(R * 4);
  if (!a.thresh) a.thresh = s.alloc<uint32_t>(R);
  if (!a.count) a.count = s.alloc<uint32_t>(R);
  if (!a.centre) a.centre = s.alloc<uint32_t>(R);
  a.scratch = s.alloc_bytes(dq::distance_scratch_bytes(a.width, a.height, a.nregions));
  dq::launch_region_distance(a, s.stream());
  DQ_HIP(hipGetLastError());
}

int run_on(hipStream_t st, dq::DistanceArgs a) {
  Staging s(st);
  distance_on(s, a);
  s.finish();
  return 0;
}

// The distance launches, the components of the map read as u32 labels, then
// the cores pass; waits, returns the pixels kept.
int64_t run_on(hipStream_t st, dq::DistanceArgs a, CoresOut to, int connectivity) {
  Staging s(st);
  distance_on(s, a);
  s.release(a.scratch);
  const size_t n = (size_t)a.width * a.height;
  dq::RegionArgs r{};
  r.labels = a.regions, r.label_bytes = 4, r.width = a.width, r.height = a.height, r.connectivity = connectivity;
  r.regions = s.alloc<uint32_t>(n);
  r.scratch = s.alloc<uint32_t>(dq::region_scratch_words(a.width, a.height));
  dq::launch_label_regions(r, st);
  dq::CoresArgs c{};
  c.regions = a.regions, c.width = a.width, c.height = a.height, c.nregions = a.nregions;
  c.component = r.regions, c.centre = a.centre, c.core = to.core, c.cored = to.cored;
  c.core_area = to.core_area ? to.core_area : s.alloc<uint32_t>(a.nregions);
  c.kept = s.alloc<uint32_t>(1);
  dq::launch_region_cores(c, st);
  uint32_t kept = 0;
  s.fetch(&kept, c.kept);
  s.finish();
  return (int64_t)kept;
}

// -------------------------------------------------------------------------
// Skeletons of a region map (dq_skeleton.hip).
bool args_ok(const dq::SkeletonArgs& a) {
  if (!a.regions) return false;
  if (a.width == 0 || a.height == 0 || a.width > 65535u || a.height > 65535u ||
      (uint64_t)a.width * a.height > 0x7FFFFFFFull)
    return false;
  if (a.nregions == 0 || a.max_iters > dq::kSkeletonMaxIters) return false;
  if (!a.skel && !a.skeled && !a.when && !a.skel_area && !a.thick) return false;
  return aligned({a.regions, a.skeled, a.skel_area, a.thick}) && aligned({a.when}, 2);
}

// How many thinning launches go out before the next read-back: 2, 4, then 8 at a time.
uint32_t skeleton_group(uint32_t launches) { return launches < 2 ? 2u : launches < 6 ? 4u : 8u; }

// Enqueues the planes pass, the thinning launches in groups and the outputs pass
// on st with scratch owned by the call, waits, returns the pixels kept.  The host
// reads one word per launch of a group back (the last iteration of the launch that
// deleted) and stops at a launch with an iteration that deleted nothing.
int64_t run_on(hipStream_t st, dq::SkeletonArgs a, uint32_t* iterations, uint32_t* converged) {
  Staging s(st);
  if (a.thick && !a.when) a.when = s.alloc<uint16_t>((size_t)a.width * a.height);
  a.scratch = s.alloc_bytes(dq::skeleton_scratch_bytes(a.width, a.height));
  dq::launch_skeleton_planes(a, st);
  const uint32_t limit = a.max_iters ? a.max_iters : dq::kSkeletonMaxIters;
  uint32_t ran = 0, launches = 0, last_deleting = 0;
  bool stable = false;
  uint32_t last[8];
  // An iteration that deletes nothing leaves a fixed point: the deleting iterations are 1 .. I.
  while (ran < limit && !stable) {
    const uint32_t from = launches, group = skeleton_group(launches);
    for (; launches < from + group && ran < limit; ++launches) {
      const uint32_t iters = std::min(dq::kSkeletonIters, limit - ran);
      dq::launch_skeleton_thin(a, launches, iters, st);
      ran += iters;
    }
    s.fetch(last, dq::skeleton_last_words(a) + from, launches - from);
    s.sync();
    for (uint32_t l = from; l < launches && !stable; ++l) {
      const uint32_t first = l * dq::kSkeletonIters, iters = std::min(dq::kSkeletonIters, limit - first);
      if (last[l - from]) last_deleting = first + last[l - from];
      stable = last[l - from] < iters;
    }
  }
  dq::launch_skeleton_outputs(a, launches, st);
  uint32_t kept = 0;
  s.fetch(&kept, dq::skeleton_kept_word(a));
  s.finish();
  if (iterations) *iterations = last_deleting;
  if (converged) *converged = stable ? 1u : 0u;
  return (int64_t)kept;
}

// -------------------------------------------------------------------------
// Contours of a region map (dq_contour.hip).
bool args_ok(const dq::ContourArgs& a) {
  if (!a.regions) return false;
  if (a.width == 0 || a.height == 0 || a.width > 65535u || a.height > 65535u ||
      (uint64_t)a.width * a.height > 0x7FFFFFFFull)
    return false;
  // (the scans walk the regions in chunks: the last chunk's indexes stay below 2^32)
  if (a.nregions == 0 || a.nregions > 0xFFFFFFFFu - dq::kRegionChunk) return false;
  if (a.orientation != 0 && a.orientation != 1) return false;
  if (!a.offsets && !a.points && !a.codes && !a.len && !a.visits) return false;
  if (a.point_cap > 0 && !a.points && !a.codes) return false;
  return aligned({a.regions, a.offsets, a.points, a.len});
}

// How many pointer-jumping rounds go out before the next read-back.
uint32_t contour_group(uint32_t rounds) { return rounds < 8 ? 4u : 8u; }

// Enqueues the mark pass, the links, the rounds in groups, the lengths and the
// emit pass on st with scratch owned by the call, waits, returns M.  Read-backs:
// S (sizes the links), one word per round of a group (a round that found every
// start's chain resolved ends the rounds) and M (-2; do the lists fit).
int64_t run_on(hipStream_t st, dq::ContourArgs a) {
  Staging s(st);
  const size_t R = a.nregions;
  if (!a.len) a.len = s.alloc<uint32_t>(R);
  a.scratch = s.alloc_bytes(dq::contour_scratch_bytes(a.width, a.height, a.nregions));
  dq::launch_contour_mark(a, st);
  const uint32_t states = s.read_word(dq::contour_states_word(a));
  if (states > dq::kContourMaxStates) {
    s.finish();
    return -3;
  }
  if (states) a.links = s.alloc_bytes(dq::contour_links_bytes(states));
  dq::launch_contour_links(a, states, st);
  uint32_t rounds = 0;
  bool resolved = states == 0;
  uint32_t todo[8];
  // A chain of L states is resolved after ceil(log2(L)) rounds: at most kContourMaxRounds, the loop ends by itself.
  while (!resolved && rounds < dq::kContourMaxRounds) {
    const uint32_t from = rounds, group = contour_group(rounds);
    for (; rounds < from + group && rounds < dq::kContourMaxRounds; ++rounds) dq::launch_contour_jump(a, states, rounds, st);
    s.fetch(todo, dq::contour_round_words(a) + from, rounds - from);
    s.sync();
    for (uint32_t l = from; l < rounds; ++l) resolved = resolved || todo[l - from] == 0;
  }
  dq::launch_contour_lengths(a, states, rounds, st);
  const uint32_t total = s.read_word(dq::contour_total_word(a));
  if (total == 0xFFFFFFFFu) {   // (the saturated sum: only len is written)
    s.finish();
    return -2;
  }
  if (!a.offsets) a.offsets = s.alloc<uint32_t>(R + 1);
  DQ_HIP(dq::launch_contour_emit(a, states, rounds, total <= a.point_cap && total != 0, st));
  DQ_HIP(hipGetLastError());
  s.finish();
  return (int64_t)total;
}

// -------------------------------------------------------------------------
// Pixel lists of a region map (dq_pixels.hip).
bool args_ok(const dq::PixelsArgs& a) {
  if (!a.regions || !a.offsets) return false;
  if (a.width == 0 || a.height == 0 || a.width > 65535u || a.height > 65535u ||
      (uint64_t)a.width * a.height > 0x7FFFFFFFull)
    return false;
  if (a.nregions == 0 || a.nregions > 0x7FFFFFFFu) return false;
  if (!aligned({a.regions, a.offsets, a.coords, a.index, a.pixels, a.colors})) return false;
  if (a.colors && !a.pixels) return false;
  return true;
}

// Enqueues both halves on st with scratch owned by the call and waits.  One
// small read-back sits between the halves: the table is sized from T, and a
// map with T > n is refused there, before any output array is written.
int64_t run_on(hipStream_t st, dq::PixelsArgs a) {
  Staging s(st);
  a.rows = s.alloc_bytes<uint32_t>(dq::pixels_rows_bytes(a.nregions));
  dq::launch_pixels_rows(a, st);
  const uint32_t total = s.read_word(dq::pixels_total_word(a));
  const bool fits = total <= a.width * a.height;
  if (fits) {
    a.table = s.alloc_bytes<uint32_t>(dq::pixels_table_bytes(total));
    dq::launch_pixels_lists(a, total, st);
    DQ_HIP(hipGetLastError());
  }
  s.finish();
  return fits ? 0 : -2;
}

// -------------------------------------------------------------------------
// One weighted quant per region or window: K and the host arrays of the
// results.  `out` is where the mapped colours go (optional; device memory).
struct QuantArgs {
  uint32_t k;
  uint32_t* out;
  uint32_t *cts, *k_outs;
  int max_iters;
};

bool quant_ok(const uint32_t* pixels, const QuantArgs& q) {
  if (!pixels || !q.cts || !q.k_outs || q.k == 0 || q.k > 0x7FFFFFFFu || q.max_iters < 1) return false;
  return aligned({q.out});
}

// Region map -> pixel lists -> one weighted quant per region -> painted frame.
// The regions path keeps one pinned argument and one pinned result record per
// job of a call (about 4.5 KB): the jobs go to it kRegionMapJobs at a time.
constexpr size_t kRegionMapJobs = 8192;

bool quant_map_ok(dq::PixelsArgs a, const QuantArgs& q) {
  if (!quant_ok(a.pixels, q)) return false;
  // (the offsets and lists are the call's own: any aligned non-NULL pointer stands in for them)
  a.offsets = const_cast<uint32_t*>(a.regions);
  return args_ok(a);
}

// One weighted-regions call over the ranges [off[r], off[r + 1]) of d_colors, region r's K = q.k: its
// colortable to q.cts + r * k, its count to q.k_outs[r] (0 for an empty range, the row untouched), its
// mapped colours to the same range of q.out when given.  Returns the total of empty clusters.
int64_t quant_ranges_on(int device, hipStream_t st, const std::vector<uint32_t>& off, const uint32_t* d_colors,
                        const QuantArgs& q) {
  const uint32_t nregions = (uint32_t)off.size() - 1;
  int64_t empty = 0;
  Engine& e = engine_for(device);
  std::vector<dq::FrameJob> jobs;
  std::vector<uint32_t> ids;
  jobs.reserve(std::min<size_t>(nregions, kRegionMapJobs));
  ids.reserve(jobs.capacity());
  auto flush = [&] {
    if (jobs.empty()) return;
    {
      std::lock_guard<std::mutex> g(e.mutex());
      e.run_weighted_regions(jobs.data(), (int)jobs.size(), q.max_iters, st);
    }
    for (size_t i = 0; i < jobs.size(); ++i) {
      q.k_outs[ids[i]] = (uint32_t)jobs[i].k_out;
      empty += jobs[i].num_empty;
    }
    jobs.clear();
    ids.clear();
  };
  for (uint32_t r = 0; r < nregions; ++r) {
    const uint32_t len = off[r + 1] - off[r];
    if (len == 0) {   // an empty list: no call, its colortable row stays as it is
      q.k_outs[r] = 0;
      continue;
    }
    dq::FrameJob j;
    j.d_in = d_colors + off[r];
    j.n = len;
    j.d_out = q.out ? q.out + off[r] : nullptr;
    j.k = (int)q.k;
    j.ct = q.cts + (size_t)r * q.k;
    jobs.push_back(j);
    ids.push_back(r);
    if (jobs.size() == kRegionMapJobs) flush();
  }
  flush();
  return empty;
}

// a: the map and the frame (the offsets and lists are the call's own); q.out: the painted frame.
int64_t quant_region_map_on(int device, hipStream_t st, dq::PixelsArgs a, const QuantArgs& q) {
  Staging s(st);
  const size_t n = (size_t)a.width * a.height, no = (size_t)a.nregions + 1;
  a.offsets = s.alloc<uint32_t>(no);
  a.colors = s.alloc<uint32_t>(n);
  QuantArgs lists = q;   // (the mapped colours in list order)
  if (q.out) {
    a.coords = s.alloc<uint32_t>(n);
    lists.out = s.alloc<uint32_t>(n);
    // (an id >= nregions leaves its pixel out of the lists: the scatter below then reads Coord 0, not garbage)
    DQ_HIP(hipMemsetAsync(a.coords, 0, n * 4, st));
  }
  int64_t rc = run_on(st, a);
  if (rc == 0) {
    std::vector<uint32_t> off(no);
    s.download(off.data(), a.offsets, no);
    s.sync();
    rc = quant_ranges_on(device, st, off, a.colors, lists);
    if (q.out) {
      dq::launch_scatter_coords(lists.out, a.coords, (uint32_t)n, a.width, q.out, st);
      DQ_HIP(hipGetLastError());
    }
  }
  s.finish();
  return rc;
}

// -------------------------------------------------------------------------
// Capture windows of a region map (dq_windows.hip).  cap: the entries of room
// in the list arrays.
dq::PixelsArgs lists_of(const dq::WindowsArgs& a) {
  dq::PixelsArgs p{};
  p.regions = a.regions, p.width = a.width, p.height = a.height, p.nregions = a.nregions;
  p.offsets = a.offsets, p.coords = a.coords, p.index = a.index, p.pixels = a.pixels, p.colors = a.colors;
  return p;
}

bool args_ok(const dq::WindowsArgs& a, uint32_t cap) {
  if (!args_ok(lists_of(a))) return false;
  if (a.block < 1 || a.block > 8 || a.expand > 3) return false;
  if (!aligned({a.area})) return false;
  if (cap > 0 && !a.coords && !a.index && !a.colors) return false;
  return true;
}

// What the first half of a windows or tags call finds: 0 or the refusal (-2, -3), P, T and M, and
// the word of the caller's own launch.
struct WindowsCounts {
  int64_t rc;
  uint32_t npairs, nrows, total, extra;
};

// The first half of the windows and the tags stage, up to "M is known or the call is refused": the
// blocks scratch and launch_windows_blocks; P and T read back (a map with T > P is refused, and -3
// is decided there); the pairs and launch_windows_count; M read back (-3).  `after_blocks`
// (optional) enqueues a launch of the caller's behind launch_windows_blocks and returns the device
// word of a saturating count of it, which comes back with P and T under the same synchronisation.
// The scratch stays with `s` (a.blocks, a.pairs).
WindowsCounts windows_counts(Staging& s, dq::WindowsArgs& a,
                             const std::function<const uint32_t*()>& after_blocks = nullptr) {
  hipStream_t st = s.stream();
  a.blocks = s.alloc_bytes<uint32_t>(dq::windows_blocks_bytes(a.width, a.height, a.block, a.nregions));
  dq::launch_windows_blocks(a, st);
  const uint32_t* extra = after_blocks ? after_blocks() : nullptr;
  uint32_t w[3] = {0, 0, 0};
  s.read_words({dq::windows_pairs_word(a), dq::windows_rows_word(a), extra}, w);
  WindowsCounts c{0, w[0], w[1], 0, w[2]};
  if (c.npairs == 0xFFFFFFFFu || c.extra == 0xFFFFFFFFu) {
    c.rc = -3;   // (the pairs are indexed by words)
  } else if (c.nrows > c.npairs) {
    c.rc = -2;
  } else {
    a.pairs = s.alloc_bytes<uint32_t>(dq::windows_pairs_bytes(c.npairs, c.nrows));
    if (c.npairs != 0 && c.nrows != 0) {
      dq::launch_windows_count(a, c.npairs, c.nrows, st);
      c.total = s.read_word(dq::windows_total_word(a, c.npairs, c.nrows));
    }
    if (c.total == 0xFFFFFFFFu) c.rc = -3;
  }
  return c;
}

// Enqueues the parts on st with scratch owned by the call and waits.  Two small
// read-backs sit between them: P and T size the pairs and the table (a map with
// T > P is refused there), and M decides -3 and whether the lists fit, before
// any output array is written.
int64_t run_on(hipStream_t st, dq::WindowsArgs a, uint32_t cap) {
  Staging s(st);
  const WindowsCounts c = windows_counts(s, a);
  if (c.rc == 0) {
    dq::launch_windows_offsets(a, c.npairs, c.nrows, c.total, st);
    if (c.total <= cap) dq::launch_windows_lists(a, c.npairs, c.nrows, c.total, st);
    DQ_HIP(hipGetLastError());
  }
  s.finish();
  return c.rc < 0 ? c.rc : (int64_t)c.total;
}

// The device copies of a host windows call's inputs (the frame only when it is read); no output yet.
dq::WindowsArgs windows_inputs(Staging& s, const dq::WindowsArgs& h, bool frame) {
  const size_t n = (size_t)h.width * h.height;
  dq::WindowsArgs d = h;
  d.regions = s.upload(h.regions, n), d.mask = s.upload(h.mask, n), d.area = s.upload(h.area, h.nregions);
  d.pixels = frame ? s.upload(h.pixels, n) : nullptr;
  d.offsets = d.coords = d.index = d.colors = nullptr;
  return d;
}

// -------------------------------------------------------------------------
// Region map -> capture windows -> one weighted quant per window.
bool quant_windows_ok(dq::WindowsArgs a, uint32_t cap, const QuantArgs& q) {
  if (!quant_ok(a.pixels, q)) return false;
  if (cap > 0 && !a.coords && !a.index && !a.colors && q.out) a.coords = q.out;   // (d_out alone is a list array of cap words)
  return args_ok(a, cap);
}

int64_t quant_region_windows_on(int device, hipStream_t st, const dq::WindowsArgs& a, uint32_t cap,
                                const QuantArgs& q) {
  const size_t no = (size_t)a.nregions + 1;
  const bool lists = a.coords || a.index || a.colors;
  int64_t rc = run_on(st, a, lists ? cap : 0u);
  if (rc < 0) return rc;
  const int64_t total = rc;
  if (q.out && total > (int64_t)cap) return -4;
  // the colours in list order: the caller's when they were written, else the call's own
  Staging s(st);
  const uint32_t* colors = a.colors;
  if (!(a.colors && total <= (int64_t)cap) && total > 0) {
    dq::WindowsArgs own = a;
    own.offsets = s.alloc<uint32_t>(no);
    own.coords = own.index = nullptr;
    own.colors = s.alloc<uint32_t>((size_t)total);
    rc = run_on(st, own, (uint32_t)total);
    colors = own.colors;
  }
  if (rc >= 0) {
    std::vector<uint32_t> off(no);
    s.download(off.data(), a.offsets, no);
    s.sync();
    rc = quant_ranges_on(device, st, off, colors, q);
  }
  s.finish();
  return rc;
}

// -------------------------------------------------------------------------
// Window tags (dq_wtags.hip): the windows stage up to the pair positions, then
// the tag histogram of every window from its pairs.  a: the windows call's
// inputs and (optional) offsets; t: the outputs; cap: the entries of room.
bool args_ok(const dq::WindowsArgs& a, const dq::WtagsArgs& t, uint32_t cap) {
  // (rows stands where the windows call has its offsets: required; the entry arrays are its list arrays)
  dq::WindowsArgs stand = a;
  stand.offsets = t.rows, stand.coords = t.ids, stand.index = t.counts;
  if (!args_ok(stand, 0)) return false;
  if (cap > 0 && !t.ids && !t.counts && !t.first) return false;
  return aligned({t.first, t.inside, t.best, t.best_count, a.offsets});
}

// Three read-backs with a synchronisation each: P, T and Q (Q sizes the table;
// a map with T > P is refused and -3 is decided there), M (-3; sizes the bitmap)
// and E (do the entries fit), all before any output array is written.
int64_t run_on(hipStream_t st, dq::WindowsArgs a, dq::WtagsArgs t, uint32_t cap) {
  Staging s(st);
  t.regions = a.regions, t.width = a.width, t.height = a.height, t.nregions = a.nregions, t.block = a.block;
  t.mask = a.mask;
  const WindowsCounts c = windows_counts(s, a, [&] {
    const dq::WindowsView v = dq::windows_view(a, 0);   // (what the first part leaves: the pairs come later)
    t.nblocks = v.nblocks, t.pairbase = v.pairbase;
    t.live = s.alloc_bytes<uint32_t>(dq::wtags_live_bytes(v.nblocks));
    dq::launch_wtags_count(t, st);   // (the members of every block are counted by then: Q needs no pair)
    return dq::wtags_contribs_word(t);
  });
  int64_t rc = c.rc;
  if (rc == 0) {
    const uint32_t ncontribs = c.npairs != 0 && c.nrows != 0 ? c.extra : 0u;   // (no pair, no contribution)
    const dq::WindowsView v = dq::windows_view(a, c.npairs);
    uint32_t* pair_ids = nullptr;
    if (ncontribs != 0) {
      // the member ids of the pairs: the walk below turns the windows stage's into positions
      pair_ids = s.alloc<uint32_t>(c.npairs);
      DQ_HIP(hipMemcpyAsync(pair_ids, v.pair_word, (size_t)c.npairs * 4, hipMemcpyDeviceToDevice, st));
    }
    t.pair_id = pair_ids, t.pair_pos = v.pair_word, t.npairs = c.npairs, t.total = c.total;
    if (!a.offsets) a.offsets = s.alloc<uint32_t>((size_t)a.nregions + 1);
    t.offsets = a.offsets;
    dq::launch_windows_offsets(a, c.npairs, c.nrows, c.total, st);
    if (ncontribs != 0) dq::launch_windows_walk(a, c.npairs, c.nrows, st);
    t.table = s.alloc_bytes<uint32_t>(dq::wtags_table_bytes(ncontribs, c.total, a.nregions));
    dq::launch_wtags_fill(t, ncontribs, st);
    const uint32_t nentries = s.read_word(dq::wtags_entries_word(t, ncontribs));
    rc = nentries;
    dq::launch_wtags_rows(t, ncontribs, st);
    if (nentries <= cap) dq::launch_wtags_entries(t, ncontribs, nentries, st);
    DQ_HIP(hipGetLastError());
  }
  s.finish();
  return rc;
}

}  // namespace

// =========================================================================
extern "C" {

int64_t dq_hip_label_regions_dev(int device, const void* d_labels, int label_bytes, uint32_t width,
                                 uint32_t height, int connectivity, uint32_t* d_regions, uint32_t stats_cap,
                                 uint32_t* d_area, uint32_t* d_bbox, uint32_t* d_first, uint32_t* d_label,
                                 const uint32_t* d_pixels, uint64_t* d_sums, void* stream) {
  dq::RegionArgs a{};
  a.labels = d_labels, a.label_bytes = label_bytes, a.width = width, a.height = height, a.connectivity = connectivity;
  a.regions = d_regions, a.stats_cap = stats_cap, a.area = d_area, a.bbox = d_bbox, a.first = d_first;
  a.label = d_label, a.pixels = d_pixels, a.sums = (u64*)d_sums;
  if (!args_ok(a)) return -1;
  return run_on(engine_stream(device, stream), a);
}

int64_t dq_hip_label_regions(const void* labels, int label_bytes, uint32_t width, uint32_t height,
                             int connectivity, uint32_t* regions, uint32_t stats_cap, uint32_t* area,
                             uint32_t* bbox, uint32_t* first, uint32_t* label, const uint32_t* pixels,
                             uint64_t* sums) {
  dq::RegionArgs h{};
  h.labels = labels, h.label_bytes = label_bytes, h.width = width, h.height = height, h.connectivity = connectivity;
  h.regions = regions, h.stats_cap = stats_cap, h.area = area, h.bbox = bbox, h.first = first;
  h.label = label, h.pixels = pixels, h.sums = (u64*)sums;
  if (!args_ok(h)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height, cap = stats_cap;
  dq::RegionArgs d = h;
  d.labels = s.upload((const uint8_t*)labels, n * (size_t)label_bytes);
  d.regions = s.alloc<uint32_t>(n);
  d.area = s.twin(area, cap), d.bbox = s.twin(bbox, cap * 4), d.first = s.twin(first, cap), d.label = s.twin(label, cap);
  d.sums = s.twin(h.sums, cap * 3);
  d.pixels = d.sums ? s.upload(pixels, n) : nullptr;
  const int64_t count = run_on(st, d);
  // nothing behind entry min(R, stats_cap) is written
  const size_t m = std::min((size_t)count, cap);
  s.download(regions, d.regions, n);
  s.download(area, d.area, m), s.download(bbox, d.bbox, m * 4), s.download(first, d.first, m);
  s.download(label, d.label, m), s.download(h.sums, d.sums, m * 3);
  s.sync();
  return count;
}

int64_t dq_hip_region_adjacency_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                    int connectivity, uint32_t edge_cap, uint32_t* d_edges, uint32_t* d_border,
                                    uint32_t* d_contact, const uint32_t* d_pixels, uint64_t* d_step,
                                    uint32_t nregions, uint32_t* d_degree, void* stream) {
  dq::AdjacencyArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.connectivity = connectivity, a.edge_cap = edge_cap;
  a.edges = d_edges, a.border = d_border, a.contact = d_contact, a.pixels = d_pixels, a.step = (u64*)d_step;
  a.degree = d_degree;
  if (!args_ok(a, nregions)) return -1;
  return run_on(engine_stream(device, stream), a, nregions);
}

int64_t dq_hip_region_adjacency(const uint32_t* regions, uint32_t width, uint32_t height, int connectivity,
                                uint32_t edge_cap, uint32_t* edges, uint32_t* border, uint32_t* contact,
                                const uint32_t* pixels, uint64_t* step, uint32_t nregions, uint32_t* degree) {
  dq::AdjacencyArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.connectivity = connectivity, h.edge_cap = edge_cap;
  h.edges = edges, h.border = border, h.contact = contact, h.pixels = pixels, h.step = (u64*)step;
  h.degree = degree;
  if (!args_ok(h, nregions)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height, cap = edge_cap;
  dq::AdjacencyArgs d = h;
  d.regions = s.upload(regions, n);
  d.edges = s.twin(edges, cap * 2), d.border = s.twin(border, cap), d.contact = s.twin(contact, cap * 2);
  d.step = s.twin(h.step, cap);
  d.pixels = d.step ? s.upload(pixels, n) : nullptr;
  d.degree = s.twin(degree, nregions);
  const int64_t count = run_on(st, d, nregions);
  // nothing behind entry min(E, edge_cap) is written
  const size_t m = std::min((size_t)count, cap);
  s.download(edges, d.edges, m * 2), s.download(border, d.border, m), s.download(contact, d.contact, m * 2);
  s.download(h.step, d.step, m), s.download(degree, d.degree, nregions);
  s.sync();
  return count;
}

int64_t dq_hip_merge_regions_dev(int device, const uint32_t* d_regions, uint32_t n, uint32_t nregions,
                                 const uint32_t* d_area, const uint32_t* d_first, const uint64_t* d_sums,
                                 const uint32_t* d_bbox, uint32_t nedges, const uint32_t* d_edges, uint32_t min_area,
                                 uint32_t max_dist, uint32_t max_rounds, uint32_t* d_out_regions, uint32_t* d_remap,
                                 uint32_t stats_cap, uint32_t* d_out_area, uint32_t* d_out_bbox,
                                 uint32_t* d_out_first, uint64_t* d_out_sums, uint32_t* rounds, void* stream) {
  dq::MergeArgs a{};
  a.regions = d_regions, a.n = n, a.nregions = nregions, a.area = d_area, a.first = d_first;
  a.sums = (const u64*)d_sums, a.bbox = d_bbox, a.nedges = nedges, a.edges = d_edges;
  a.min_area = min_area, a.max_dist = max_dist, a.out_regions = d_out_regions, a.remap = d_remap;
  a.stats_cap = stats_cap, a.out_area = d_out_area, a.out_bbox = d_out_bbox, a.out_first = d_out_first;
  a.out_sums = (u64*)d_out_sums;
  if (!args_ok(a)) return -1;
  return run_on(engine_stream(device, stream), a, max_rounds, rounds);
}

int64_t dq_hip_segment_labels(const void* labels, int label_bytes, uint32_t width, uint32_t height, int connectivity,
                              const uint32_t* pixels, uint32_t min_area, uint32_t max_dist, uint32_t max_rounds,
                              uint32_t* regions, uint32_t stats_cap, uint32_t* area, uint32_t* bbox, uint32_t* first,
                              uint64_t* sums, uint32_t* rounds) {
  // what the call is given, as the regions stage and the adjacency stage (no edge output) would be
  dq::RegionArgs h{};
  h.labels = labels, h.label_bytes = label_bytes, h.width = width, h.height = height, h.connectivity = connectivity;
  h.regions = regions, h.stats_cap = stats_cap, h.area = area, h.bbox = bbox, h.first = first;
  h.pixels = pixels, h.sums = (u64*)sums;
  dq::AdjacencyArgs g{};
  g.regions = regions, g.width = width, g.height = height, g.connectivity = connectivity, g.pixels = pixels;
  if (!pixels || !args_ok(h) || !args_ok(g, 0)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height;
  // R and E are known only after their stages ran: count-only, then with exact capacity
  dq::RegionArgs r{};
  r.labels = s.upload((const uint8_t*)labels, n * (size_t)label_bytes), r.label_bytes = label_bytes;
  r.width = width, r.height = height, r.connectivity = connectivity;
  const uint32_t* d_pixels = s.upload(pixels, n);
  r.regions = s.alloc<uint32_t>(n);
  const int64_t R = run_on(st, r);
  r.stats_cap = (uint32_t)R, r.area = s.alloc<uint32_t>((size_t)R), r.first = s.alloc<uint32_t>((size_t)R);
  r.sums = s.alloc<u64>((size_t)R * 3);
  if (stats_cap && bbox) r.bbox = s.alloc<uint32_t>((size_t)R * 4);
  r.pixels = d_pixels;
  run_on(st, r);
  g.regions = r.regions, g.pixels = nullptr;
  const int64_t E = run_on(st, g, 0);
  if (E > 0) {
    g.edge_cap = (uint32_t)E, g.edges = s.alloc<uint32_t>((size_t)E * 2);
    run_on(st, g, 0);
  }
  const size_t cap = std::min((size_t)stats_cap, (size_t)R);   // (R' <= R)
  dq::MergeArgs m{};
  m.regions = r.regions, m.n = (uint32_t)n, m.nregions = (uint32_t)R, m.area = r.area, m.first = r.first;
  m.sums = r.sums, m.bbox = r.bbox, m.nedges = (uint32_t)E, m.edges = g.edges;
  m.min_area = min_area, m.max_dist = max_dist, m.out_regions = r.regions, m.stats_cap = (uint32_t)cap;
  m.out_area = s.twin(area, cap), m.out_bbox = s.twin(bbox, cap * 4), m.out_first = s.twin(first, cap);
  m.out_sums = s.twin(h.sums, cap * 3);
  const int64_t count = run_on(st, m, max_rounds, rounds);
  // nothing behind entry min(R', stats_cap) is written
  const size_t k = std::min((size_t)count, cap);
  s.download(regions, m.out_regions, n);
  s.download(area, m.out_area, k), s.download(bbox, m.out_bbox, k * 4), s.download(first, m.out_first, k);
  s.download(h.sums, m.out_sums, k * 3);
  s.sync();
  return count;
}

int64_t dq_hip_region_containment_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                      uint32_t nregions, const uint32_t* d_area, uint32_t nedges,
                                      const uint32_t* d_edges, uint32_t* d_depth, uint32_t* d_parent,
                                      uint32_t* d_roots, uint32_t* d_child_offsets, uint32_t* d_children,
                                      uint32_t* d_subtree, uint64_t* d_enclosed, uint32_t* d_order, uint32_t* d_pos,
                                      uint32_t* levels, uint32_t* reached, void* stream) {
  dq::ContainArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.area = d_area;
  a.nedges = nedges, a.edges = d_edges;
  ContainOut to{};
  to.depth = d_depth, to.parent = d_parent, to.roots = d_roots, to.child_offsets = d_child_offsets;
  to.children = d_children, to.subtree = d_subtree, to.enclosed = d_enclosed, to.order = d_order, to.pos = d_pos;
  if (!args_ok(a, to)) return -1;
  return run_on(engine_stream(device, stream), a, to, hipMemcpyDeviceToDevice, levels, reached);
}

int64_t dq_hip_region_containment(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                  const uint32_t* area, uint32_t nedges, const uint32_t* edges, uint32_t* depth,
                                  uint32_t* parent, uint32_t* roots, uint32_t* child_offsets, uint32_t* children,
                                  uint32_t* subtree, uint64_t* enclosed, uint32_t* order, uint32_t* pos,
                                  uint32_t* levels, uint32_t* reached) {
  dq::ContainArgs a{};
  a.regions = regions, a.width = width, a.height = height, a.nregions = nregions, a.area = area;
  a.nedges = nedges, a.edges = edges;
  ContainOut to{};
  to.depth = depth, to.parent = parent, to.roots = roots, to.child_offsets = child_offsets;
  to.children = children, to.subtree = subtree, to.enclosed = enclosed, to.order = order, to.pos = pos;
  if (!args_ok(a, to)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  a.regions = s.upload(regions, (size_t)width * height);
  a.area = s.upload(area, nregions);
  a.edges = nedges ? s.upload(edges, (size_t)nedges * 2) : nullptr;
  return run_on(st, a, to, hipMemcpyDeviceToHost, levels, reached);
}

int dq_hip_region_distance_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                               uint32_t nregions, int rule, uint16_t* d_dist, uint32_t* d_dmax, uint32_t* d_bbox,
                               uint32_t* d_thresh, uint32_t* d_count, uint32_t* d_centre, void* stream) {
  dq::DistanceArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.rule = rule;
  a.dist = d_dist, a.dmax = d_dmax, a.bbox = d_bbox, a.thresh = d_thresh, a.count = d_count, a.centre = d_centre;
  if (!args_ok(a) || no_output(a)) return -1;
  return run_on(engine_stream(device, stream), a);
}

int dq_hip_region_distance(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions, int rule,
                           uint16_t* dist, uint32_t* dmax, uint32_t* bbox, uint32_t* thresh, uint32_t* count,
                           uint32_t* centre) {
  dq::DistanceArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.rule = rule;
  h.dist = dist, h.dmax = dmax, h.bbox = bbox, h.thresh = thresh, h.count = count, h.centre = centre;
  if (!args_ok(h) || no_output(h)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height, R = nregions;
  dq::DistanceArgs d = h;
  d.regions = s.upload(regions, n);
  d.dist = s.twin(dist, n), d.dmax = s.twin(dmax, R), d.bbox = s.twin(bbox, R * 4), d.thresh = s.twin(thresh, R);
  d.count = s.twin(count, R), d.centre = s.twin(centre, R);
  const int rc = run_on(st, d);
  s.download(dist, d.dist, n), s.download(dmax, d.dmax, R), s.download(bbox, d.bbox, R * 4);
  s.download(thresh, d.thresh, R), s.download(count, d.count, R), s.download(centre, d.centre, R);
  s.sync();
  return rc;
}

int64_t dq_hip_region_cores_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                uint32_t nregions, int rule, int connectivity, uint8_t* d_core, uint32_t* d_cored,
                                uint32_t* d_centre, uint32_t* d_core_area, uint16_t* d_dist, void* stream) {
  dq::DistanceArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.rule = rule;
  a.dist = d_dist, a.centre = d_centre;
  const CoresOut to{d_core, d_cored, d_core_area};
  if (!args_ok(a, to, connectivity)) return -1;
  return run_on(engine_stream(device, stream), a, to, connectivity);
}

int64_t dq_hip_region_cores(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions, int rule,
                            int connectivity, uint8_t* core, uint32_t* cored, uint32_t* centre, uint32_t* core_area,
                            uint16_t* dist) {
  dq::DistanceArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.rule = rule;
  h.dist = dist, h.centre = centre;
  if (!args_ok(h, CoresOut{core, cored, core_area}, connectivity)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height, R = nregions;
  dq::DistanceArgs d = h;
  d.regions = s.upload(regions, n);
  d.dist = s.twin(dist, n), d.centre = s.twin(centre, R);
  const CoresOut to{s.twin(core, n), s.twin(cored, n), s.twin(core_area, R)};
  const int64_t kept = run_on(st, d, to, connectivity);
  s.download(core, to.core, n), s.download(cored, to.cored, n), s.download(core_area, to.core_area, R);
  s.download(dist, d.dist, n), s.download(centre, d.centre, R);
  s.sync();
  return kept;
}

int64_t dq_hip_region_skeleton_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                   uint32_t nregions, uint32_t max_iters, uint8_t* d_skel, uint32_t* d_skeled,
                                   uint16_t* d_when, uint32_t* d_skel_area, uint32_t* d_thick, uint32_t* iterations,
                                   uint32_t* converged, void* stream) {
  dq::SkeletonArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.max_iters = max_iters;
  a.skel = d_skel, a.skeled = d_skeled, a.when = d_when, a.skel_area = d_skel_area, a.thick = d_thick;
  if (!args_ok(a)) return -1;
  return run_on(engine_stream(device, stream), a, iterations, converged);
}

int64_t dq_hip_region_skeleton(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                               uint32_t max_iters, uint8_t* skel, uint32_t* skeled, uint16_t* when,
                               uint32_t* skel_area, uint32_t* thick, uint32_t* iterations, uint32_t* converged) {
  dq::SkeletonArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.max_iters = max_iters;
  h.skel = skel, h.skeled = skeled, h.when = when, h.skel_area = skel_area, h.thick = thick;
  if (!args_ok(h)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height, R = nregions;
  dq::SkeletonArgs d = h;
  d.regions = s.upload(regions, n);
  d.skel = s.twin(skel, n), d.skeled = s.twin(skeled, n), d.when = s.twin(when, n);
  d.skel_area = s.twin(skel_area, R), d.thick = s.twin(thick, R);
  const int64_t kept = run_on(st, d, iterations, converged);
  s.download(skel, d.skel, n), s.download(skeled, d.skeled, n), s.download(when, d.when, n);
  s.download(skel_area, d.skel_area, R), s.download(thick, d.thick, R);
  s.sync();
  return kept;
}

int64_t dq_hip_region_contours_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                   uint32_t nregions, int orientation, uint64_t point_cap, uint32_t* d_offsets,
                                   uint32_t* d_points, uint8_t* d_codes, uint32_t* d_len, uint8_t* d_visits,
                                   void* stream) {
  dq::ContourArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.orientation = orientation;
  a.point_cap = point_cap, a.offsets = d_offsets, a.points = d_points, a.codes = d_codes, a.len = d_len;
  a.visits = d_visits;
  if (!args_ok(a)) return -1;
  return run_on(engine_stream(device, stream), a);
}

int64_t dq_hip_region_contours(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                               int orientation, uint64_t point_cap, uint32_t* offsets, uint32_t* points,
                               uint8_t* codes, uint32_t* len, uint8_t* visits) {
  dq::ContourArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.orientation = orientation;
  h.point_cap = point_cap, h.offsets = offsets, h.points = points, h.codes = codes, h.len = len, h.visits = visits;
  if (!args_ok(h)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height, R = nregions;
  const size_t cap = (size_t)std::min<uint64_t>(point_cap, 0xFFFFFFFFull);   // (M is a word)
  dq::ContourArgs d = h;
  d.regions = s.upload(regions, n);
  d.offsets = s.twin(offsets, R + 1), d.points = s.twin(points, cap), d.codes = s.twin(codes, cap);
  d.len = s.twin(len, R), d.visits = s.twin(visits, n);
  const int64_t total = run_on(st, d);
  // nothing but len at -2; the lists only when all M entries fit
  if (total >= 0 || total == -2) s.download(len, d.len, R);
  if (total >= 0) {
    const size_t m = (uint64_t)total <= point_cap ? (size_t)total : 0;
    s.download(offsets, d.offsets, R + 1), s.download(visits, d.visits, n);
    s.download(points, d.points, m), s.download(codes, d.codes, m);
  }
  s.sync();
  return total;
}

int dq_hip_regions_by_size_dev(int device, uint32_t nregions, const uint32_t* d_area, uint32_t* d_order,
                               uint32_t* d_rank, void* stream) {
  if (!d_area || nregions == 0 || (!d_order && !d_rank)) return -1;
  if (!aligned({d_area, d_order, d_rank})) return -1;
  hipStream_t st = engine_stream(device, stream);
  Staging s(st);
  void* scratch = s.alloc_bytes(dq::size_scratch_bytes(nregions));
  dq::launch_size_bits(nregions, d_area, scratch, st);
  // the OR of the areas: the sort runs over the key bits in use
  const uint32_t bits = s.read_word(dq::size_bits_word(scratch));
  dq::launch_size_order(nregions, d_area, dq::sort_key_bits(bits), d_order, d_rank, scratch, st);
  DQ_HIP(hipGetLastError());
  s.finish();
  return 0;
}

int64_t dq_hip_region_pixels_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                 uint32_t nregions, uint32_t* d_offsets, uint32_t* d_coords, uint32_t* d_index,
                                 const uint32_t* d_pixels, uint32_t* d_colors, void* stream) {
  dq::PixelsArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.offsets = d_offsets;
  a.coords = d_coords, a.index = d_index, a.pixels = d_pixels, a.colors = d_colors;
  if (!args_ok(a)) return -1;
  return run_on(engine_stream(device, stream), a);
}

int64_t dq_hip_region_pixels(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                             uint32_t* offsets, uint32_t* coords, uint32_t* index, const uint32_t* pixels,
                             uint32_t* colors) {
  dq::PixelsArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.offsets = offsets;
  h.coords = coords, h.index = index, h.pixels = pixels, h.colors = colors;
  if (!args_ok(h)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t n = (size_t)width * height, no = (size_t)nregions + 1;
  dq::PixelsArgs d = h;
  d.regions = s.upload(regions, n);
  d.offsets = s.alloc<uint32_t>(no);
  d.coords = s.twin(coords, n), d.index = s.twin(index, n), d.colors = s.twin(colors, n);
  d.pixels = d.colors ? s.upload(pixels, n) : nullptr;
  const int64_t rc = run_on(st, d);
  if (rc == 0) {   // (a refused map leaves the host arrays as they were)
    s.download(offsets, d.offsets, no);
    s.download(coords, d.coords, n), s.download(index, d.index, n), s.download(colors, d.colors, n);
    s.sync();
  }
  return rc;
}

int dq_hip_scatter_coords_dev(int device, const uint32_t* d_values, const uint32_t* d_coords, uint32_t n,
                              uint32_t width, uint32_t* d_frame, void* stream) {
  if (!d_values || !d_coords || !d_frame || width == 0) return -1;
  if (!aligned({d_values, d_coords, d_frame})) return -1;
  if (n == 0) return 0;
  hipStream_t st = engine_stream(device, stream);
  dq::launch_scatter_coords(d_values, d_coords, n, width, d_frame, st);
  dq::join_default_stream(stream, st);
  DQ_HIP(hipGetLastError());
  return 0;
}

int64_t dq_hip_quant_region_map_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                    uint32_t nregions, const uint32_t* d_pixels, uint32_t k, uint32_t* d_out,
                                    uint32_t* cts, uint32_t* k_outs, int max_iters, void* stream) {
  dq::PixelsArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.pixels = d_pixels;
  QuantArgs q{};
  q.k = k, q.out = d_out, q.cts = cts, q.k_outs = k_outs, q.max_iters = max_iters;
  if (!quant_map_ok(a, q)) return -1;
  return quant_region_map_on(device, engine_stream(device, stream), a, q);
}

int64_t dq_hip_quant_region_map(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                const uint32_t* pixels, uint32_t k, uint32_t* out, uint32_t* cts, uint32_t* k_outs,
                                int max_iters) {
  dq::PixelsArgs a{};
  a.regions = regions, a.width = width, a.height = height, a.nregions = nregions, a.pixels = pixels;
  QuantArgs q{};
  q.k = k, q.out = out, q.cts = cts, q.k_outs = k_outs, q.max_iters = max_iters;
  if (!quant_map_ok(a, q)) return -1;
  const int device = dq::current_device();
  hipStream_t st = engine_for(device).stream();
  Staging s(st);
  const size_t n = (size_t)width * height;
  a.regions = s.upload(regions, n);
  a.pixels = s.upload(pixels, n);
  q.out = s.twin(out, n);
  const int64_t rc = quant_region_map_on(device, st, a, q);
  if (rc >= 0 && out) {
    s.download(out, q.out, n);
    s.sync();
  }
  return rc;
}

int64_t dq_hip_region_windows_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                  uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                                  const uint32_t* d_area, uint32_t min_area, uint32_t* d_offsets, uint32_t cap,
                                  uint32_t* d_coords, uint32_t* d_index, const uint32_t* d_pixels, uint32_t* d_colors,
                                  void* stream) {
  dq::WindowsArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.block = block, a.expand = expand;
  a.mask = d_mask, a.area = d_area, a.min_area = min_area, a.offsets = d_offsets;
  a.coords = d_coords, a.index = d_index, a.pixels = d_pixels, a.colors = d_colors;
  if (!args_ok(a, cap)) return -1;
  return run_on(engine_stream(device, stream), a, cap);
}

int64_t dq_hip_region_windows(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                              uint32_t block, uint32_t expand, const uint8_t* mask, const uint32_t* area,
                              uint32_t min_area, uint32_t* offsets, uint32_t cap, uint32_t* coords, uint32_t* index,
                              const uint32_t* pixels, uint32_t* colors) {
  dq::WindowsArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.block = block, h.expand = expand;
  h.mask = mask, h.area = area, h.min_area = min_area, h.offsets = offsets;
  h.coords = coords, h.index = index, h.pixels = pixels, h.colors = colors;
  if (!args_ok(h, cap)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t no = (size_t)nregions + 1;
  dq::WindowsArgs d = windows_inputs(s, h, colors != nullptr);
  d.offsets = s.alloc<uint32_t>(no);
  d.coords = s.twin(coords, cap), d.index = s.twin(index, cap), d.colors = s.twin(colors, cap);
  const int64_t rc = run_on(st, d, cap);
  if (rc >= 0) {   // (a refused map leaves the host arrays as they were)
    s.download(offsets, d.offsets, no);
    if (rc <= (int64_t)cap) {   // (M > cap leaves the lists as they were)
      s.download(coords, d.coords, (size_t)rc), s.download(index, d.index, (size_t)rc);
      s.download(colors, d.colors, (size_t)rc);
    }
    s.sync();
  }
  return rc;
}

int64_t dq_hip_quant_region_windows_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                                        uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                                        const uint32_t* d_area, uint32_t min_area, uint32_t* d_offsets, uint32_t cap,
                                        uint32_t* d_coords, uint32_t* d_index, const uint32_t* d_pixels,
                                        uint32_t* d_colors, uint32_t k, uint32_t* d_out, uint32_t* cts,
                                        uint32_t* k_outs, int max_iters, void* stream) {
  dq::WindowsArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.block = block, a.expand = expand;
  a.mask = d_mask, a.area = d_area, a.min_area = min_area, a.offsets = d_offsets;
  a.coords = d_coords, a.index = d_index, a.pixels = d_pixels, a.colors = d_colors;
  QuantArgs q{};
  q.k = k, q.out = d_out, q.cts = cts, q.k_outs = k_outs, q.max_iters = max_iters;
  if (!quant_windows_ok(a, cap, q)) return -1;
  return quant_region_windows_on(device, engine_stream(device, stream), a, cap, q);
}

int64_t dq_hip_quant_region_windows(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions,
                                    uint32_t block, uint32_t expand, const uint8_t* mask, const uint32_t* area,
                                    uint32_t min_area, uint32_t* offsets, uint32_t cap, uint32_t* coords,
                                    uint32_t* index, const uint32_t* pixels, uint32_t* colors, uint32_t k,
                                    uint32_t* out, uint32_t* cts, uint32_t* k_outs, int max_iters) {
  dq::WindowsArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.block = block, h.expand = expand;
  h.mask = mask, h.area = area, h.min_area = min_area, h.offsets = offsets;
  h.coords = coords, h.index = index, h.pixels = pixels, h.colors = colors;
  QuantArgs q{};
  q.k = k, q.out = out, q.cts = cts, q.k_outs = k_outs, q.max_iters = max_iters;
  if (!quant_windows_ok(h, cap, q)) return -1;
  const int device = dq::current_device();
  hipStream_t st = engine_for(device).stream();
  Staging s(st);
  const size_t no = (size_t)nregions + 1;
  dq::WindowsArgs d = windows_inputs(s, h, true);
  d.offsets = s.alloc<uint32_t>(no);
  d.coords = s.twin(coords, cap), d.index = s.twin(index, cap), d.colors = s.twin(colors, cap);
  q.out = out ? s.alloc<uint32_t>(std::max<uint32_t>(cap, 1u)) : nullptr;
  const int64_t rc = quant_region_windows_on(device, st, d, cap, q);
  if (rc >= 0) {   // (a refused call leaves the host arrays as they were)
    uint32_t total = 0;
    s.download(offsets, d.offsets, no);
    s.download(&total, d.offsets + nregions, 1);
    s.sync();
    if (total > 0 && total <= cap) {
      s.download(coords, d.coords, total), s.download(index, d.index, total), s.download(colors, d.colors, total);
      s.download(out, q.out, total);
      s.sync();
    }
  }
  return rc;
}

int64_t dq_hip_window_tags_dev(int device, const uint32_t* d_regions, uint32_t width, uint32_t height,
                               uint32_t nregions, uint32_t block, uint32_t expand, const uint8_t* d_mask,
                               const uint32_t* d_area, uint32_t min_area, uint32_t* d_rows, uint32_t cap,
                               uint32_t* d_ids, uint32_t* d_counts, uint32_t* d_first, uint32_t* d_inside,
                               uint32_t* d_best, uint32_t* d_best_count, uint32_t* d_offsets, void* stream) {
  dq::WindowsArgs a{};
  a.regions = d_regions, a.width = width, a.height = height, a.nregions = nregions, a.block = block, a.expand = expand;
  a.mask = d_mask, a.area = d_area, a.min_area = min_area, a.offsets = d_offsets;
  dq::WtagsArgs t{};
  t.rows = d_rows, t.ids = d_ids, t.counts = d_counts, t.first = d_first;
  t.inside = d_inside, t.best = d_best, t.best_count = d_best_count;
  if (!args_ok(a, t, cap)) return -1;
  return run_on(engine_stream(device, stream), a, t, cap);
}

int64_t dq_hip_window_tags(const uint32_t* regions, uint32_t width, uint32_t height, uint32_t nregions, uint32_t block,
                           uint32_t expand, const uint8_t* mask, const uint32_t* area, uint32_t min_area,
                           uint32_t* rows, uint32_t cap, uint32_t* ids, uint32_t* counts, uint32_t* first,
                           uint32_t* inside, uint32_t* best, uint32_t* best_count, uint32_t* offsets) {
  dq::WindowsArgs h{};
  h.regions = regions, h.width = width, h.height = height, h.nregions = nregions, h.block = block, h.expand = expand;
  h.mask = mask, h.area = area, h.min_area = min_area, h.offsets = offsets;
  dq::WtagsArgs t{};
  t.rows = rows, t.ids = ids, t.counts = counts, t.first = first;
  t.inside = inside, t.best = best, t.best_count = best_count;
  if (!args_ok(h, t, cap)) return -1;
  hipStream_t st = host_stream();
  Staging s(st);
  const size_t no = (size_t)nregions + 1;
  dq::WindowsArgs d = windows_inputs(s, h, false);
  // the device twins of the host arrays given: rows | offsets, the three entry arrays, the three per region
  d.offsets = s.twin(offsets, no);
  dq::WtagsArgs dt{};
  dt.rows = s.twin(rows, no), dt.ids = s.twin(ids, cap), dt.counts = s.twin(counts, cap), dt.first = s.twin(first, cap);
  dt.inside = s.twin(inside, nregions), dt.best = s.twin(best, nregions), dt.best_count = s.twin(best_count, nregions);
  const int64_t rc = run_on(st, d, dt, cap);
  if (rc >= 0) {   // (a refused map leaves the host arrays as they were)
    s.download(rows, dt.rows, no), s.download(offsets, d.offsets, no);
    if (rc <= (int64_t)cap) {   // (E > cap leaves the entry arrays as they were)
      s.download(ids, dt.ids, (size_t)rc), s.download(counts, dt.counts, (size_t)rc);
      s.download(first, dt.first, (size_t)rc);
    }
    s.download(inside, dt.inside, nregions), s.download(best, dt.best, nregions);
    s.download(best_count, dt.best_count, nregions);
    s.sync();
  }
  return rc;
}

// Window votes (dq_wtags.hip).  There is no host-pointer twin: the call consumes
// device arrays that only the device pipeline produces.
int64_t dq_hip_window_votes_dev(int device, const uint32_t* d_regions, uint32_t n, uint32_t nregions,
                                const uint32_t* d_offsets, const uint32_t* d_index, uint32_t total,
                                const uint32_t* d_mapped, const uint32_t* cts, const uint32_t* k_outs, uint32_t k,
                                uint32_t* d_votes, uint32_t* d_best, void* stream) {
  if (!d_regions || !d_offsets || !cts || !k_outs || !d_votes || !d_best) return -1;
  if (total > 0 && (!d_index || !d_mapped)) return -1;
  if (n == 0 || n > 0x7FFFFFFFu || nregions == 0 || nregions > 0x7FFFFFFFu || k < 1 || k > dq::kVotesMaxK) return -1;
  if (total == 0xFFFFFFFFu) return -1;   // (the windows call gives such an M up)
  if (!aligned({d_regions, d_offsets, d_index, d_mapped, cts, k_outs, d_votes, d_best})) return -1;
  hipStream_t st = engine_stream(device, stream);
  Staging s(st);
  dq::WvotesArgs a{};
  a.regions = d_regions, a.n = n, a.nregions = nregions, a.offsets = d_offsets, a.index = d_index;
  a.mapped = d_mapped, a.total = total, a.k = k, a.votes = d_votes, a.best = d_best;
  a.cts = s.upload(cts, (size_t)nregions * k);
  a.k_outs = s.upload(k_outs, nregions);
  a.jobs = s.alloc_bytes<uint32_t>(dq::wvotes_jobs_bytes(nregions));
  dq::launch_wvotes(a, st);
  DQ_HIP(hipGetLastError());
  u64 misses = 0;
  s.download(&misses, dq::wvotes_misses_word(a), 1);
  s.finish();
  return (int64_t)misses;
}

}  // extern "C"
