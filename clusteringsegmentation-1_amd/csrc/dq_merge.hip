// dq_merge.hip -- merging regions over their adjacency graph on gfx950 (MI355X).
//
// Input: a map of n region ids < R, per region its area, first pixel, colour
// sums (and bounding box), and a list of id pairs that touch.  comp[r] is the
// component of region r, at first r itself; a component carries the summed
// stats of its regions.  One round (include/dq_hip.h, "region merge", has the
// full definition):
//   a component is RESTLESS when its area < min_area; its mean is the 8.8
//   fixed-point floor(256 * sum / area) per channel; d(A, B) = the sum of the
//   three |mean differences|.  Every edge between different components with
//   d <= max_dist offers each restless end the key (d << 32 | other end); a
//   component's best is the lowest key offered.  A restless A with a best
//   links to its target T unless T's best targets A and A < T (of a mutual
//   pair the lower id stays a root).  A round without a link ends the call.
//   Otherwise every component's stats are added into the root of its parent
//   chain and comp[] follows.
// The final components are numbered in increasing order of their first pixel.
// Every output is an integer that does not depend on scheduling.
//
// Kernels per round, all over regions or edges, never over pixels (no kernel
// waits for another workgroup; what atomics write in one launch only later
// launches read, by plain loads):
//   prep    comp[r] = rootof[comp[r]] (the fold of the round before); a live
//           root (comp[r] == r) gets its three means packed in one word with
//           the restless bit, best = none, parent = itself
//   choose  per edge: both ends through comp[], the distance from the packed
//           means, a 64-bit atomicMin into best[] of the restless ends
//   link    per live root: the rule above; the links are counted (one add per
//           workgroup of a bounded grid) and the host reads the count back:
//           4 bytes
//   fold    per live root: its root by a chase of the now read-only parent[]
//           (rootof[] = it); a non-root adds its stats into the root, first in
//           128 LDS slots per workgroup (slot free or already the root's, else
//           straight to global memory) flushed once: thousands of specks fold
//           into one background region in the same round
// The chase and not pointer doubling: a chain of L links costs its one thread L
// dependent loads, and doubling costs log2 L launches over all regions plus a
// converged-yet read-back; chains follow strictly the lowest key, so on frames
// they are a few links long, and the 2047-link chain of the test is one thread.
//
// Finish: a bitmap of n bits with the first pixels of the live roots set, the
// set bits per 1024-bit chunk, one workgroup's exclusive scan of those
// (dq_scan.h's top scan), and
// the new id of a root = its chunk's offset + the set bits below its own in
// the chunk (work over regions and n / 32 words; a pixel pass that counts
// first[comp[reg[p]]] == p would read the whole map once more).  Then
// remap[r] = newid[comp[r]] and one pixel pass out[p] = remap[regions[p]],
// 16 bytes per thread where both maps are 16-byte aligned.
// No floating point anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dq_merge.h"
#include "dq_scan.h"
#include "dq_stage.h"

namespace dq {
namespace {

using scan::chunks_of;   // (of the bitmap: scan::kChunk bits per count)

constexpr uint32_t kChunkWords = scan::kChunk / 32;
static_assert(kChunkWords == 32, "a count per half wave of bitmap words; chunk = first pixel >> 10");
constexpr unsigned long long kNoBest = ~0ull;     // no key equals it: d <= 195840
constexpr unsigned long long kRestless = 1ull << 63;
constexpr uint32_t kSlots = 128;                  // LDS slots of the fold pass
// -DDQ_MERGE_LDS_SLOTS=0 builds the fold pass without them (every non-root
// straight to global memory): the variant DESIGN.md 5a'''' measures against.
#ifndef DQ_MERGE_LDS_SLOTS
#define DQ_MERGE_LDS_SLOTS 1
#endif

struct Scratch {
  unsigned long long* sums;   // 3 per component
  unsigned long long* best;
  unsigned long long* mean;   // R | G << 16 | B << 32 | restless << 63
  uint32_t* area;
  uint32_t* first;
  uint32_t* comp;
  uint32_t* parent;           // (newid[] once the rounds are over)
  uint32_t* rootof;
  uint32_t* bbox;             // 4 per component, or nullptr
  uint32_t* newof;            // the caller's remap, or scratch
  uint32_t* bitmap;           // nchunks * 32 words
  uint32_t* counts;           // nchunks + 1
  uint32_t* links;
};

Scratch carve(const MergeArgs& a) {
  const size_t R = a.nregions, nchunks = chunks_of(a.n);
  Scratch s;
  s.sums = (unsigned long long*)a.scratch;
  s.best = s.sums + 3 * R;
  s.mean = s.best + R;
  s.area = (uint32_t*)(s.mean + R);
  s.first = s.area + R;
  s.comp = s.first + R;
  s.parent = s.comp + R;
  s.rootof = s.parent + R;
  uint32_t* p = s.rootof + R;
  s.bbox = a.bbox ? p : nullptr;
  if (a.bbox) p += 4 * R;
  s.newof = a.remap ? a.remap : p;
  if (!a.remap) p += R;
  s.bitmap = p;
  s.counts = s.bitmap + nchunks * kChunkWords;
  s.links = s.counts + nchunks + 1;
  return s;
}

// ---- init ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void merge_init_kernel(uint32_t R, const uint32_t* __restrict__ area,
                                                             const uint32_t* __restrict__ first,
                                                             const unsigned long long* __restrict__ sums,
                                                             const uint32_t* __restrict__ bbox, Scratch s) {
  const uint64_t r = global_thread();
  if (r >= R) return;
  s.comp[r] = s.rootof[r] = (uint32_t)r;
  s.area[r] = area[r];
  s.first[r] = first[r];
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) s.sums[3 * r + c] = sums[3 * r + c];
  if (bbox) {
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) s.bbox[4 * r + c] = bbox[4 * r + c];
  }
}

// ---- prep ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void merge_prep_kernel(uint32_t R, uint32_t min_area, Scratch s) {
  const uint64_t r = global_thread();
  if (r == 0) *s.links = 0;
  if (r >= R) return;
  const uint32_t c = s.rootof[s.comp[r]];
  s.comp[r] = c;
  if (c != (uint32_t)r) return;
  const uint32_t area = s.area[r];   // (> 0: the caller's areas are)
  unsigned long long m = area < min_area ? kRestless : 0ull;
  if (area != 0) {
#pragma unroll
    for (uint32_t ch = 0; ch < 3; ++ch) m |= ((s.sums[3 * r + ch] << 8) / area & 0xFFFFull) << (16 * ch);
  }
  s.mean[r] = m;
  s.best[r] = kNoBest;
  s.parent[r] = (uint32_t)r;
}

// ---- choose ----------------------------------------------------------------
__device__ __forceinline__ uint32_t mean_distance(unsigned long long x, unsigned long long y) {
  uint32_t d = 0;
#pragma unroll
  for (uint32_t ch = 0; ch < 3; ++ch) {
    const int dx = (int)((x >> (16 * ch)) & 0xFFFFu) - (int)((y >> (16 * ch)) & 0xFFFFu);
    d += (uint32_t)abs(dx);
  }
  return d;
}

__global__ __launch_bounds__(kThreads) void merge_choose_kernel(uint32_t R, uint32_t E,
                                                               const uint32_t* __restrict__ edges,
                                                               uint32_t max_dist, Scratch s) {
  const uint64_t i = global_thread();
  if (i >= E) return;
  const uint32_t a = edges[2 * i], b = edges[2 * i + 1];
  if (a >= R || b >= R) return;   // (not an id: the pair is skipped)
  const uint32_t A = s.comp[a], B = s.comp[b];
  if (A == B) return;             // (a stale pair: both ends in one component by now)
  const unsigned long long mA = s.mean[A], mB = s.mean[B];
  if (!((mA | mB) & kRestless)) return;
  const uint32_t d = mean_distance(mA, mB);
  if (d > max_dist) return;
  if (mA & kRestless) atomicMin(&s.best[A], ((unsigned long long)d << 32) | B);
  if (mB & kRestless) atomicMin(&s.best[B], ((unsigned long long)d << 32) | A);
}

// ---- link ------------------------------------------------------------------
// A grid of at most kLinkBlocks workgroups strides over the regions and each
// adds its links to the one global word once: a frame of specks has millions of
// regions, and one add per wave (127 000 adds to one address, one after the
// other) took longer than the rest of the pass.
constexpr uint32_t kLinkBlocks = 2048;
__global__ __launch_bounds__(kThreads) void merge_link_kernel(uint32_t R, Scratch s) {
  __shared__ uint32_t s_links;
  if (threadIdx.x == 0) s_links = 0;
  __syncthreads();
  uint32_t made = 0;
  for (uint64_t r = global_thread(); r < R; r += (uint64_t)gridDim.x * kThreads) {
    if (s.comp[r] != (uint32_t)r) continue;
    const unsigned long long b = s.best[r];
    if (b == kNoBest) continue;
    const uint32_t T = (uint32_t)b;
    const unsigned long long bT = s.best[T];
    const bool mutual = bT != kNoBest && (uint32_t)bT == (uint32_t)r;
    if (mutual && (uint32_t)r < T) continue;
    s.parent[r] = T;
    ++made;
  }
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) made += __shfl_xor(made, d);
  if ((threadIdx.x & 63u) == 0 && made) atomicAdd(&s_links, made);
  __syncthreads();
  if (threadIdx.x == 0 && s_links) atomicAdd(s.links, s_links);
}

// ---- fold ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void merge_fold_kernel(uint32_t R, Scratch s) {
  __shared__ uint32_t s_root[kSlots], s_area[kSlots], s_first[kSlots], s_bbox[4 * kSlots];
  __shared__ unsigned long long s_sums[3 * kSlots];
  const bool boxes = s.bbox != nullptr;   // (uniform over the grid)
  if (threadIdx.x < kSlots) {
    const uint32_t t = threadIdx.x;
    s_root[t] = kNoId;
    s_area[t] = 0;
    s_first[t] = kNoId;
    s_sums[3 * t] = s_sums[3 * t + 1] = s_sums[3 * t + 2] = 0;
    s_bbox[4 * t] = s_bbox[4 * t + 1] = kNoId;
    s_bbox[4 * t + 2] = s_bbox[4 * t + 3] = 0;
  }
  __syncthreads();
  const uint64_t r = global_thread();
  if (r < R && s.comp[r] == (uint32_t)r) {
    // parent[] is a forest (DESIGN.md 5a''''): the chase ends at a root; the
    // bound only keeps a broken forest from spinning.
    uint32_t root = (uint32_t)r;
    for (uint32_t k = 0; k < R; ++k) {
      const uint32_t p = s.parent[root];
      if (p == root) break;
      root = p;
    }
    s.rootof[r] = root;
    if (root != (uint32_t)r) {
      const uint32_t area = s.area[r], first = s.first[r];
      const unsigned long long s0 = s.sums[3 * r], s1 = s.sums[3 * r + 1], s2 = s.sums[3 * r + 2];
      uint32_t bb[4] = {0, 0, 0, 0};
      if (boxes) {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) bb[c] = s.bbox[4 * r + c];
      }
      const uint32_t slot = root % kSlots;
      // (the areas of a frame sum to n < 2^31: the u32 sum holds)
      if (DQ_MERGE_LDS_SLOTS && slot_claim(s_root, slot, kNoId, root)) {
        atomicAdd(&s_area[slot], area);
        atomicMin(&s_first[slot], first);
        atomicAdd(&s_sums[3 * slot], s0);
        atomicAdd(&s_sums[3 * slot + 1], s1);
        atomicAdd(&s_sums[3 * slot + 2], s2);
        if (boxes) {
          atomicMin(&s_bbox[4 * slot], bb[0]);
          atomicMin(&s_bbox[4 * slot + 1], bb[1]);
          atomicMax(&s_bbox[4 * slot + 2], bb[2]);
          atomicMax(&s_bbox[4 * slot + 3], bb[3]);
        }
      } else {
        atomicAdd(&s.area[root], area);
        atomicMin(&s.first[root], first);
        atomicAdd(&s.sums[3 * (size_t)root], s0);
        atomicAdd(&s.sums[3 * (size_t)root + 1], s1);
        atomicAdd(&s.sums[3 * (size_t)root + 2], s2);
        if (boxes) {
          atomicMin(&s.bbox[4 * (size_t)root], bb[0]);
          atomicMin(&s.bbox[4 * (size_t)root + 1], bb[1]);
          atomicMax(&s.bbox[4 * (size_t)root + 2], bb[2]);
          atomicMax(&s.bbox[4 * (size_t)root + 3], bb[3]);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kSlots && s_root[threadIdx.x] != kNoId) {
    const uint32_t t = threadIdx.x;
    const size_t root = s_root[t];
    atomicAdd(&s.area[root], s_area[t]);
    atomicMin(&s.first[root], s_first[t]);
    atomicAdd(&s.sums[3 * root], s_sums[3 * t]);
    atomicAdd(&s.sums[3 * root + 1], s_sums[3 * t + 1]);
    atomicAdd(&s.sums[3 * root + 2], s_sums[3 * t + 2]);
    if (boxes) {
      atomicMin(&s.bbox[4 * root], s_bbox[4 * t]);
      atomicMin(&s.bbox[4 * root + 1], s_bbox[4 * t + 1]);
      atomicMax(&s.bbox[4 * root + 2], s_bbox[4 * t + 2]);
      atomicMax(&s.bbox[4 * root + 3], s_bbox[4 * t + 3]);
    }
  }
}

// ---- finish ----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void merge_bits_kernel(uint32_t R, uint32_t n, Scratch s) {
  const uint64_t r = global_thread();
  if (r >= R || s.comp[r] != (uint32_t)r) return;
  const uint32_t f = s.first[r];
  if (f < n) atomicOr(&s.bitmap[f >> 5], 1u << (f & 31u));
}

// counts[chunk] = the set bits of the chunk's 32 words (one word per thread,
// summed over the 32 lanes of a half wave).
__global__ __launch_bounds__(kThreads) void merge_count_kernel(uint32_t nwords, const uint32_t* __restrict__ bitmap,
                                                              uint32_t* __restrict__ counts) {
  const uint64_t w = global_thread();   // (nwords is a multiple of 32, the grid of 256: whole half waves)
  uint32_t c = w < nwords ? (uint32_t)__popc(bitmap[w]) : 0u;
#pragma unroll
  for (uint32_t d = 16; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 31u) == 0 && w < nwords) counts[w >> 5] = c;
}

struct StatsOut {
  uint32_t cap;
  uint32_t* area;
  uint32_t* bbox;
  uint32_t* first;
  unsigned long long* sums;
};

__global__ __launch_bounds__(kThreads) void merge_number_kernel(uint32_t R, uint32_t n, Scratch s, StatsOut o) {
  const uint64_t r = global_thread();
  if (r >= R || s.comp[r] != (uint32_t)r) return;
  const uint32_t f = s.first[r];
  if (f >= n) return;
  const uint32_t chunk = f >> 10, word = (f >> 5) & 31u;
  const uint32_t* w = s.bitmap + (size_t)chunk * kChunkWords;
  uint32_t id = s.counts[chunk] + (uint32_t)__popc(w[word] & ((1u << (f & 31u)) - 1u));
  for (uint32_t k = 0; k < word; ++k) id += (uint32_t)__popc(w[k]);
  s.parent[r] = id;   // newid[]
  if (id >= o.cap) return;
  if (o.area) o.area[id] = s.area[r];
  if (o.first) o.first[id] = f;
  if (o.sums) {
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) o.sums[3 * (size_t)id + c] = s.sums[3 * r + c];
  }
  if (o.bbox) {
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) o.bbox[4 * (size_t)id + c] = s.bbox[4 * r + c];
  }
}

__global__ __launch_bounds__(kThreads) void merge_remap_kernel(uint32_t R, Scratch s) {
  const uint64_t r = global_thread();
  if (r < R) s.newof[r] = s.parent[s.comp[r]];
}

__device__ __forceinline__ uint32_t new_id(const uint32_t* __restrict__ newof, uint32_t R, uint32_t id) {
  return id < R ? newof[id] : id;   // (not an id: left as it is)
}

// out[p] = newof[reg[p]]; every thread reads its pixels before it writes them,
// so out may be reg.  VEC: both maps are 16-byte aligned, four pixels a thread.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void merge_pixels_kernel(const uint32_t* reg, uint32_t n, uint32_t R,
                                                               const uint32_t* __restrict__ newof, uint32_t* out) {
  const uint64_t p = 4 * global_thread();
  if (p >= n) return;
  if (VEC && p + 4 <= n) {
    uint4 v = *reinterpret_cast<const uint4*>(reg + p);
    v.x = new_id(newof, R, v.x);
    v.y = new_id(newof, R, v.y);
    v.z = new_id(newof, R, v.z);
    v.w = new_id(newof, R, v.w);
    *reinterpret_cast<uint4*>(out + p) = v;
  } else {
    uint32_t v[4];
    const uint32_t m = n - p < 4 ? (uint32_t)(n - p) : 4u;
    for (uint32_t k = 0; k < m; ++k) v[k] = new_id(newof, R, reg[p + k]);
    for (uint32_t k = 0; k < m; ++k) out[p + k] = v[k];
  }
}

}  // namespace

size_t merge_scratch_bytes(uint32_t n, uint32_t nregions, bool with_bbox, bool with_remap) {
  const size_t R = nregions, nchunks = chunks_of(n);
  return R * (60 + (with_bbox ? 16 : 0) + (with_remap ? 0 : 4)) + (nchunks * kChunkWords + nchunks + 2) * 4;
}

const uint32_t* merge_links_word(const MergeArgs& a) { return carve(a).links; }
const uint32_t* merge_count_word(const MergeArgs& a) { return carve(a).counts + chunks_of(a.n); }

void launch_merge_init(const MergeArgs& a, hipStream_t st) {
  const Scratch s = carve(a);
  merge_init_kernel<<<blocks_for(a.nregions), kThreads, 0, st>>>(a.nregions, a.area, a.first, a.sums, a.bbox, s);
}

void launch_merge_choose(const MergeArgs& a, hipStream_t st) {
  const Scratch s = carve(a);
  const uint32_t R = a.nregions;
  merge_prep_kernel<<<blocks_for(R), kThreads, 0, st>>>(R, a.min_area, s);
  merge_choose_kernel<<<blocks_for(a.nedges), kThreads, 0, st>>>(R, a.nedges, a.edges, a.max_dist, s);
  merge_link_kernel<<<std::min(blocks_for(R), kLinkBlocks), kThreads, 0, st>>>(R, s);
}

void launch_merge_fold(const MergeArgs& a, hipStream_t st) {
  merge_fold_kernel<<<blocks_for(a.nregions), kThreads, 0, st>>>(a.nregions, carve(a));
}

hipError_t launch_merge_finish(const MergeArgs& a, hipStream_t st) {
  const Scratch s = carve(a);
  const uint32_t R = a.nregions, n = a.n, nchunks = chunks_of(n), nwords = nchunks * kChunkWords;
  // (comp[] follows the last fold; min_area 0: nothing is restless, the means are not used)
  merge_prep_kernel<<<blocks_for(R), kThreads, 0, st>>>(R, 0u, s);
  const hipError_t filled = hipMemsetAsync(s.bitmap, 0, (size_t)nwords * 4, st);
  if (filled != hipSuccess) return filled;   // (no bitmap, no numbering: nothing more is launched)
  merge_bits_kernel<<<blocks_for(R), kThreads, 0, st>>>(R, n, s);
  merge_count_kernel<<<blocks_for(nwords), kThreads, 0, st>>>(nwords, s.bitmap, s.counts);
  // counts[nchunks] = R' (merged regions <= n <= 2^31 - 1: the saturating sums are the sums)
  scan::scan_top_kernel<<<1, 1024, 0, st>>>(s.counts, nchunks);
  const bool out_on = a.stats_cap != 0;
  StatsOut o{a.stats_cap, out_on ? a.out_area : nullptr, out_on && a.bbox ? a.out_bbox : nullptr,
             out_on ? a.out_first : nullptr, out_on ? a.out_sums : nullptr};
  merge_number_kernel<<<blocks_for(R), kThreads, 0, st>>>(R, n, s, o);
  merge_remap_kernel<<<blocks_for(R), kThreads, 0, st>>>(R, s);
  const bool vec = (((uintptr_t)a.regions | (uintptr_t)a.out_regions) & 15u) == 0;
  const uint32_t blocks = blocks_for(((uint64_t)n + 3) / 4);
  if (vec) merge_pixels_kernel<true><<<blocks, kThreads, 0, st>>>(a.regions, n, R, s.newof, a.out_regions);
  else merge_pixels_kernel<false><<<blocks, kThreads, 0, st>>>(a.regions, n, R, s.newof, a.out_regions);
  return hipSuccess;
}

}  // namespace dq
