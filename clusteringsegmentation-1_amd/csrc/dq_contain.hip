// dq_contain.hip -- the containment tree of a region map on gfx950 (MI355X).
//
// Input: a width x height map of region ids < R, per region its area, and a
// list of id pairs that touch.  include/dq_hip.h, "containment tree", has the
// full definition; in short:
//   a region with a pixel on the image border is a ROOT, depth 0; every other
//   region's depth is 1 + the lowest depth among its neighbours (the breadth-
//   first distance from the roots; an id no root reaches is an ORPHAN); its
//   parent is the neighbour one level up with the largest area, ties to the
//   lowest id.  Roots and the children of a parent stand in SIZE ORDER (area
//   decreasing, ties id increasing); subtree[] counts a region and everything
//   below it, enclosed[] sums their areas; order[] is the post-order of the
//   forest, the inside-out order the reference walks regions in.
// Every output is an integer that does not depend on scheduling.
//
// Kernels, over border pixels, edges or regions, never over the map (no kernel
// waits for another workgroup; what atomics write in one launch only later
// launches read, except where noted):
//   init     depth = none, parent key = 0, child counts = 0
//   border   the 2 (w + h) border pixels: depth[id] = 0 (every writer writes 0)
//   roots    per region: the roots counted, the areas ORed (the key bits of the
//            size sort); one add and one or per workgroup of a bounded grid
//   level L  per edge with one end at depth L - 1 and the other at none:
//            atomicMin(depth[other], L), counted where it was none before.  A
//            thread may see L at an end another thread has just reached: L is
//            neither L - 1 nor none, so the edge does nothing, which is what it
//            would have done one launch later.  Only depths of level L - 1 make
//            a region reach another, so the order of the edges does not matter.
//            The host reads the count of reached regions back (8 bytes) and
//            stops at a level that reached nobody.
//   parent   per edge whose ends are one level apart: a 64-bit atomicMax into
//            the deeper end of (area << 32 | ~id) of the other end
//   settle   per region: parent from the key, subtree = 1, enclosed = area
//            (orphans: 0)
//   sort     dq_sort.h, twice: ids by ~area (the size order), then the size
//            order by parent + 1 (roots 0, orphans R + 1): the SEQUENCE
//            [roots | children grouped by parent | orphans]
//   rows     per child in sequence order: the children of every parent counted,
//            then dq_scan.h over the counts: the CSR rows of the children
//   fold L   L = levels - 1 .. 1, per child of depth L in sequence order:
//            subtree and enclosed added into the parent by integer atomicAdd
//            (u32, u64).  In rows and fold a wave sums each run of equal parents
//            first and adds once per run
//   place L  the scan S of subtree[] over the sequence, then L = 0 .. levels - 1
//            per sequence entry j of depth L: block = S[j] for a root, else
//            block(parent) + S[j] - S[first child of the parent];
//            pos = block + subtree - 1, order[pos] = the region
// The three level loops are launches over all edges or all reached regions: D levels
// cost 3 D launches and D read-backs (DESIGN.md 5a'''''''' has the figures).
// No floating point anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dq_contain.h"
#include "dq_scan.h"
#include "dq_sort.h"
#include "dq_stage.h"

namespace dq {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kCountBlocks = 2048;   // grids that add into one word stride over their items

struct Scratch {
  unsigned long long* key;        // R: the parent choice, (area << 32 | ~id)
  unsigned long long* enclosed;   // R
  uint32_t* depth;                // R
  uint32_t* parent;               // R
  uint32_t* childoff;             // R + 1: child counts, then their exclusive scan
  uint32_t* bysize;               // R: the size order
  uint32_t* seq;                  // R: the sequence
  uint32_t* subtree;              // R
  uint32_t* S;                    // R: exclusive scan of subtree over the sequence
  uint32_t* pos;                  // R
  uint32_t* order;                // R
  uint32_t* sums;                 // chunks_of(R + 1) + 1: the scans' chunk sums
  uint32_t* counters;             // reached, OR of the areas
  sort::Buffers sort;
};

size_t scan_sums_words(uint32_t R) { return (size_t)scan::chunks_of(R + 1) + 1; }

Scratch carve(void* scratch, uint32_t nregions) {
  const size_t R = nregions;
  Scratch s;
  s.key = (unsigned long long*)scratch;
  s.enclosed = s.key + R;
  s.depth = (uint32_t*)(s.enclosed + R);
  s.parent = s.depth + R;
  s.childoff = s.parent + R;
  s.bysize = s.childoff + R + 1;
  s.seq = s.bysize + R;
  s.subtree = s.seq + R;
  s.S = s.subtree + R;
  s.pos = s.S + R;
  s.order = s.pos + R;
  s.sums = s.order + R;
  s.counters = s.sums + scan_sums_words(nregions);
  s.sort = sort::carve(s.counters + 2, nregions);
  return s;
}

uint32_t bounded_blocks(uint64_t items) { return std::max(1u, std::min(blocks_for(items), kCountBlocks)); }

// The workgroup's sum of v, in thread 0 (every thread calls it).
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s_word) {
  if (threadIdx.x == 0) *s_word = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  if ((threadIdx.x & 63u) == 0 && v) atomicAdd(s_word, v);
  __syncthreads();
  return *s_word;
}

// ---- roots -----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void contain_init_kernel(uint32_t R, Scratch s) {
  const uint64_t r = global_thread();
  if (r == 0) s.counters[0] = s.counters[1] = 0;
  if (r > R) return;
  s.childoff[r] = 0;   // (R + 1 words)
  if (r == R) return;
  s.depth[r] = kNone;
  s.key[r] = 0;
}

__global__ __launch_bounds__(kThreads) void contain_border_kernel(const uint32_t* __restrict__ regions, uint32_t w,
                                                                 uint32_t h, uint32_t R, uint32_t* depth) {
  uint64_t t = global_thread();
  uint32_t x, y;
  if (t < w) { x = (uint32_t)t; y = 0; }
  else if ((t -= w) < w) { x = (uint32_t)t; y = h - 1; }
  else if ((t -= w) < h) { x = 0; y = (uint32_t)t; }
  else if ((t -= h) < h) { x = w - 1; y = (uint32_t)t; }
  else return;
  const uint32_t id = regions[(size_t)y * w + x];
  if (id < R) depth[id] = 0;
}

__global__ __launch_bounds__(kThreads) void contain_roots_kernel(uint32_t R, const uint32_t* __restrict__ area,
                                                                Scratch s) {
  __shared__ uint32_t s_count, s_bits;
  if (threadIdx.x == 0) s_bits = 0;
  uint32_t roots = 0, bits = 0;
  for (uint64_t r = global_thread(); r < R; r += (uint64_t)gridDim.x * kThreads) {
    roots += s.depth[r] == 0 ? 1u : 0u;
    bits |= area[r];
  }
  const uint32_t total = block_sum(roots, &s_count);   // (its first barrier orders s_bits = 0 before the ors)
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) bits |= __shfl_xor(bits, d);
  if ((threadIdx.x & 63u) == 0 && bits) atomicOr(&s_bits, bits);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (total) atomicAdd(&s.counters[0], total);
    if (s_bits) atomicOr(&s.counters[1], s_bits);
  }
}

// ---- depth -----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void contain_level_kernel(uint32_t R, uint32_t E,
                                                                const uint32_t* __restrict__ edges, uint32_t level,
                                                                uint32_t* depth, uint32_t* counters) {
  __shared__ uint32_t s_count;
  uint32_t found = 0;
  for (uint64_t i = global_thread(); i < E; i += (uint64_t)gridDim.x * kThreads) {
    const uint32_t a = edges[2 * i], b = edges[2 * i + 1];
    if (a >= R || b >= R || a == b) continue;   // (not an edge: the pair is skipped)
    const uint32_t da = depth[a], db = depth[b];
    if (da == level - 1 && db == kNone) found += atomicMin(&depth[b], level) == kNone ? 1u : 0u;
    if (db == level - 1 && da == kNone) found += atomicMin(&depth[a], level) == kNone ? 1u : 0u;
  }
  const uint32_t total = block_sum(found, &s_count);
  if (threadIdx.x == 0 && total) atomicAdd(&counters[0], total);
}

// ---- parent ----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void contain_parent_kernel(uint32_t R, uint32_t E,
                                                                 const uint32_t* __restrict__ edges,
                                                                 const uint32_t* __restrict__ area,
                                                                 const uint32_t* __restrict__ depth,
                                                                 unsigned long long* key) {
  const uint64_t i = global_thread();
  if (i >= E) return;
  const uint32_t a = edges[2 * i], b = edges[2 * i + 1];
  if (a >= R || b >= R || a == b) return;
  const uint32_t da = depth[a], db = depth[b];
  if (da == kNone || db == kNone) return;   // (both or neither: an edge never leaves the reached set)
  if (da + 1 == db) atomicMax(&key[b], ((unsigned long long)area[a] << 32) | (uint32_t)~a);
  if (db + 1 == da) atomicMax(&key[a], ((unsigned long long)area[b] << 32) | (uint32_t)~b);
}

__global__ __launch_bounds__(kThreads) void contain_settle_kernel(uint32_t R, const uint32_t* __restrict__ area,
                                                                 Scratch s) {
  const uint64_t r = global_thread();
  if (r >= R) return;
  const uint32_t d = s.depth[r];
  uint32_t parent = kNone;
  if (d != kNone && d != 0) {
    parent = ~(uint32_t)s.key[r];
    if (parent >= R) parent = kNone;   // (no key: cannot be, a region of depth d has a neighbour of depth d - 1)
  }
  s.parent[r] = parent;
  s.subtree[r] = d != kNone ? 1u : 0u;
  s.enclosed[r] = d != kNone ? (unsigned long long)area[r] : 0ull;
  s.pos[r] = kNone;
}

// ---- the two sorts' sources ------------------------------------------------
struct BySize {   // ids in id order, key ~area over the bits in use: area decreasing, stable: id increasing
  const uint32_t* area;
  uint32_t mask;
  __device__ uint32_t key(uint32_t i) const { return ~area[i] & mask; }
  __device__ uint32_t value(uint32_t i) const { return i; }
};

struct ByParent {   // the size order, key parent + 1: roots 0, orphans R + 1
  const uint32_t* bysize;
  const uint32_t* depth;
  const uint32_t* parent;
  uint32_t R;
  __device__ uint32_t key(uint32_t i) const {
    const uint32_t r = bysize[i];
    if (r >= R) return R + 1;   // (cannot be: the size order is a permutation)
    return depth[r] == kNone ? R + 1 : parent[r] + 1;   // (a root's parent is 2^32 - 1)
  }
  __device__ uint32_t value(uint32_t i) const { return bysize[i]; }
};

uint32_t mask_of(uint32_t bits) { return bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1u; }

__global__ __launch_bounds__(kThreads) void size_rank_kernel(uint32_t R, const uint32_t* __restrict__ order,
                                                            uint32_t* __restrict__ rank) {
  const uint64_t i = global_thread();
  if (i >= R) return;
  const uint32_t r = order[i];
  if (r < R) rank[r] = (uint32_t)i;
}

__global__ void size_zero_kernel(uint32_t* word) {
  if (threadIdx.x == 0) *word = 0;
}

__global__ __launch_bounds__(kThreads) void size_bits_kernel(uint32_t R, const uint32_t* __restrict__ area,
                                                            uint32_t* word) {
  __shared__ uint32_t s_bits;
  if (threadIdx.x == 0) s_bits = 0;
  __syncthreads();
  uint32_t bits = 0;
  for (uint64_t r = global_thread(); r < R; r += (uint64_t)gridDim.x * kThreads) bits |= area[r];
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) bits |= __shfl_xor(bits, d);
  if ((threadIdx.x & 63u) == 0 && bits) atomicOr(&s_bits, bits);
  __syncthreads();
  if (threadIdx.x == 0 && s_bits) atomicOr(word, s_bits);
}

// ---- children rows, subtree, enclosed --------------------------------------
// Both run over the children part of the sequence, where the children of one
// parent stand side by side: a wave first sums every run of equal parents among
// its 64 entries (dq_stage.h's wave runs), and the last lane of a run makes the
// run's one atomic add.  One add per child instead took 212 us of a
// 0.92 ms call on batman.png, whose background has 20 000 children: adds to one
// address go one after the other.
__device__ __forceinline__ WaveRun run_of_parents(uint32_t key) { return wave_run(__shfl_up(key, 1) != key); }

// Entry j of the children part and its parent, or kNone (past the end, or not
// of this level): such lanes form runs of their own and add nothing.
__device__ __forceinline__ uint32_t child_at(uint64_t j, uint32_t R, uint32_t nroots, uint32_t reached,
                                             uint32_t level, const Scratch& s, uint32_t& r) {
  r = kNone;
  if (j >= reached - nroots) return kNone;
  r = s.seq[nroots + j];
  if (r >= R || (level != 0 && s.depth[r] != level)) return kNone;
  const uint32_t p = s.parent[r];
  return p < R ? p : kNone;
}

__global__ __launch_bounds__(kThreads) void contain_rows_kernel(uint32_t R, uint32_t nroots, uint32_t reached,
                                                               Scratch s) {
  uint32_t r;
  const uint32_t p = child_at(global_thread(), R, nroots, reached, 0u, s, r);   // (every lane stays for the shuffles)
  const WaveRun run = run_of_parents(p);
  const uint32_t count = run_sum(1u, run);
  if (run.tail && p != kNone) atomicAdd(&s.childoff[p], count);
}

// Level L adds the finished sums of depth L into depth L - 1: what one launch
// reads no thread of it writes.
__global__ __launch_bounds__(kThreads) void contain_fold_kernel(uint32_t R, uint32_t level, uint32_t nroots,
                                                               uint32_t reached, Scratch s) {
  uint32_t r;
  const uint32_t p = child_at(global_thread(), R, nroots, reached, level, s, r);
  const WaveRun run = run_of_parents(p);
  const uint32_t below = run_sum(p != kNone ? s.subtree[r] : 0u, run);
  const unsigned long long inside = run_sum(p != kNone ? s.enclosed[r] : 0ull, run);
  if (run.tail && p != kNone) {
    atomicAdd(&s.subtree[p], below);
    atomicAdd(&s.enclosed[p], inside);
  }
}

// ---- post-order ------------------------------------------------------------
struct SubtreeOfSequence {
  const uint32_t* seq;
  const uint32_t* subtree;
  uint32_t R;
  __device__ uint32_t operator()(uint32_t i) const {
    const uint32_t r = seq[i];
    return r < R ? subtree[r] : 0u;
  }
};

// Level L reads pos[] of depth L - 1 and writes pos[] of depth L.
__global__ __launch_bounds__(kThreads) void contain_place_kernel(uint32_t R, uint32_t level, uint32_t nroots,
                                                                uint32_t reached, Scratch s) {
  const uint64_t j = global_thread();
  if (j >= reached) return;
  const uint32_t r = s.seq[j];
  if (r >= R || s.depth[r] != level) return;
  uint32_t block = s.S[j];
  if (level != 0) {
    const uint32_t p = s.parent[r];
    if (p >= R) return;
    const uint64_t row = (uint64_t)nroots + s.childoff[p];
    if (row >= reached) return;   // (cannot be: r itself is in the parent's row)
    block = s.pos[p] - (s.subtree[p] - 1u) + (block - s.S[row]);
  }
  const uint32_t pos = block + s.subtree[r] - 1u;
  s.pos[r] = pos;
  if (pos < reached) s.order[pos] = r;   // (pos < reached by construction: the bound keeps a broken tree inside the array)
}

}  // namespace

size_t contain_scratch_bytes(uint32_t nregions) {
  const size_t R = nregions;
  return 16 * R + 4 * (9 * R + 1 + scan_sums_words(nregions) + 2 + sort::buffer_words(nregions));
}

const uint32_t* contain_counters(const ContainArgs& a) { return carve(a.scratch, a.nregions).counters; }

ContainResults contain_results(const ContainArgs& a) {
  const Scratch s = carve(a.scratch, a.nregions);
  return ContainResults{s.depth, s.parent, s.seq, s.childoff, s.subtree, s.enclosed, s.order, s.pos};
}

void launch_contain_roots(const ContainArgs& a, hipStream_t st) {
  const Scratch s = carve(a.scratch, a.nregions);
  const uint32_t R = a.nregions;
  contain_init_kernel<<<blocks_for((uint64_t)R + 1), kThreads, 0, st>>>(R, s);
  contain_border_kernel<<<blocks_for(2 * ((uint64_t)a.width + a.height)), kThreads, 0, st>>>(a.regions, a.width,
                                                                                           a.height, R, s.depth);
  contain_roots_kernel<<<bounded_blocks(R), kThreads, 0, st>>>(R, a.area, s);
}

void launch_contain_level(const ContainArgs& a, uint32_t level, hipStream_t st) {
  const Scratch s = carve(a.scratch, a.nregions);
  contain_level_kernel<<<bounded_blocks(a.nedges), kThreads, 0, st>>>(a.nregions, a.nedges, a.edges, level, s.depth,
                                                                     s.counters);
}

void launch_contain_tree(const ContainArgs& a, uint32_t levels, uint32_t nroots, uint32_t reached, uint32_t area_bits,
                         hipStream_t st) {
  const Scratch s = carve(a.scratch, a.nregions);
  const uint32_t R = a.nregions;
  if (a.nedges) contain_parent_kernel<<<blocks_for(a.nedges), kThreads, 0, st>>>(R, a.nedges, a.edges, a.area, s.depth, s.key);
  contain_settle_kernel<<<blocks_for(R), kThreads, 0, st>>>(R, a.area, s);
  sort::launch(BySize{a.area, mask_of(area_bits)}, R, area_bits, s.bysize, s.sort, st);
  sort::launch(ByParent{s.bysize, s.depth, s.parent, R}, R, sort::bits_of(R + 1), s.seq, s.sort, st);
  const uint32_t nchildren = reached - nroots;
  if (nchildren) contain_rows_kernel<<<blocks_for(nchildren), kThreads, 0, st>>>(R, nroots, reached, s);
  scan::launch(scan::Words{s.childoff}, s.childoff, R + 1, s.sums, st);
  for (uint32_t level = levels; level-- > 1;)   // (levels > 1: there are children)
    contain_fold_kernel<<<blocks_for(nchildren), kThreads, 0, st>>>(R, level, nroots, reached, s);
  scan::launch(SubtreeOfSequence{s.seq, s.subtree, R}, s.S, R, s.sums, st);
  for (uint32_t level = 0; level < levels && reached != 0; ++level)   // (no region reached: a map of ids >= R)
    contain_place_kernel<<<blocks_for(reached), kThreads, 0, st>>>(R, level, nroots, reached, s);
}

// ---- the size order alone --------------------------------------------------
size_t size_scratch_bytes(uint32_t nregions) { return 4 * (sort::buffer_words(nregions) + (size_t)nregions + 1); }

const uint32_t* size_bits_word(const void* scratch) { return (const uint32_t*)scratch; }

void launch_size_bits(uint32_t nregions, const uint32_t* area, void* scratch, hipStream_t st) {
  size_zero_kernel<<<1, 64, 0, st>>>((uint32_t*)scratch);
  size_bits_kernel<<<bounded_blocks(nregions), kThreads, 0, st>>>(nregions, area, (uint32_t*)scratch);
}

void launch_size_order(uint32_t nregions, const uint32_t* area, uint32_t area_bits, uint32_t* order, uint32_t* rank,
                       void* scratch, hipStream_t st) {
  uint32_t* own = (uint32_t*)scratch + 1;
  const sort::Buffers b = sort::carve(own + nregions, nregions);
  uint32_t* dest = order ? order : own;
  sort::launch(BySize{area, mask_of(area_bits)}, nregions, area_bits, dest, b, st);
  if (rank) size_rank_kernel<<<blocks_for(nregions), kThreads, 0, st>>>(nregions, dest, rank);
}

}  // namespace dq
