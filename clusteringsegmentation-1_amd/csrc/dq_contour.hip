// dq_contour.hip -- the contours of all regions of a region map on gfx950
// (MI355X): border following as list ranking.
//
// Input: a width x height map of ids; an id < R is a region (its pixels need
// not be connected), an id >= R is background.  include/dq_hip.h, "region
// contours", has the full definition; in short: a neighbour of a pixel is on
// iff it lies in the frame and has the pixel's own id; a state is (p, d), a
// pixel with a direction whose neighbour is on; step(p, d) turns to the first
// on neighbour s after d, emits p with code s and goes to (p + delta[s], s + 4);
// the contour of a region is the cycle of `step` through its start state (its
// first pixel in raster order, the first on neighbour of E, SE, S, SW).
//
// `step` is a bijection on the states of a map, so the states fall into disjoint
// cycles and nothing but the cycle of a start ever reaches that start.  A traced
// contour passes only through border pixels (a 4-neighbour off), so only their
// states are numbered: base[p] + the rank of d among p's on neighbours.  With a
// start made a sink, its cycle is a chain that ends in it, and pointer jumping
// on (next, distance) words ranks the chain: the state after the start is the
// farthest one, so the chain is resolved as soon as that state points at the
// start, and len = its distance + 1.  A chain that never reaches a start (a
// hole's border, another component, the small cycles of the interior, a chain
// that leaves the border pixels) is jumped along with the rest and never written.
//
// Kernels (no kernel waits for another workgroup; every result is a function of
// the map alone):
//   mark     per pixel: the byte of its on neighbours; a pixel whose W, NW, N
//            and NE are off offers itself as its region's first (atomicMin)
//   (scan)   dq_scan.h over the states of every pixel -> base, and S
//   starts   per region: the start state, the state after it, len 0 and 1
//   links    per border pixel: the successor of each of its states into buffer 0,
//            (next, 1); a start (itself, 0); a successor off the border: (none, 1)
//   jump     per state: next <- next of next, distance summed, from one buffer
//            into the other; its first R threads look whether region r's chain
//            was resolved in the buffer read, and say so in the round's word
//   lengths  per region: len from the state after the start
//   (scan)   dq_scan.h over len -> offsets, and M
//   emit     per pixel: each of its states that points at its region's start
//            writes its point and code at len - distance (the start at 0), the
//            orientation folded into the index; visits = how many did
#include <hip/hip_runtime.h>

#include "dq_contour.h"
#include "dq_scan.h"
#include "dq_stage.h"

namespace dq {
namespace {

using u64 = unsigned long long;

// ---- neighbour bytes ---------------------------------------------------------
// Directions, y down: 0 = E, 1 = NE, 2 = N, 3 = NW, 4 = W, 5 = SW, 6 = S, 7 = SE.
__device__ __forceinline__ int dir_x(uint32_t d) { return (int)((0x83u >> d) & 1u) - (int)((0x38u >> d) & 1u); }
__device__ __forceinline__ int dir_y(uint32_t d) { return (int)((0xE0u >> d) & 1u) - (int)((0x0Eu >> d) & 1u); }
// A border pixel: one of E, N, W, S is off.
__device__ __forceinline__ bool border(uint32_t m) { return (m & 0x55u) != 0x55u; }
// The states of a pixel: one per on neighbour of a border pixel.
__device__ __forceinline__ uint32_t states_of(uint32_t m) { return border(m) ? (uint32_t)__popc(m) : 0u; }
// The place of direction d among the on neighbours m.
__device__ __forceinline__ uint32_t rank_of(uint32_t m, uint32_t d) { return (uint32_t)__popc(m & ((1u << d) - 1u)); }
// The first of d + 1, d + 2, .. (mod 8) that is on; m != 0.
__device__ __forceinline__ uint32_t next_on(uint32_t m, uint32_t d) {
  const uint32_t turned = ((m | (m << 8)) >> (d + 1u)) & 0xFFu;
  return (d + (uint32_t)__ffs((int)turned)) & 7u;
}

__device__ __forceinline__ u64 link(uint32_t next, uint32_t dist) { return (u64)next << 32 | dist; }
__device__ __forceinline__ uint32_t next_of(u64 w) { return (uint32_t)(w >> 32); }
__device__ __forceinline__ uint32_t dist_of(u64 w) { return (uint32_t)w; }

struct Parts {
  uint32_t* base;     // n: the number of the pixel's first state
  uint32_t* first;    // R: the region's first pixel, kNoId for an id with no pixel
  uint32_t* start;    // R: the start state, kNoId when len is 0 or 1
  uint32_t* after;    // R: the state after the start, kNoId when there is none
  uint32_t* sums;     // the top scans: of the states, then of len
  uint32_t* round;    // kContourMaxRounds
  uint8_t* mask;      // n: the on neighbours, bit d for direction d; 0 for background
  uint32_t nchunks_n, nchunks_r;
};

Parts carve(void* scratch, uint32_t width, uint32_t height, uint32_t nregions) {
  const size_t n = (size_t)width * height, R = nregions;
  Parts p;
  p.nchunks_n = scan::chunks_of((uint32_t)n), p.nchunks_r = scan::chunks_of(nregions);
  p.base = (uint32_t*)scratch;
  p.first = p.base + n;
  p.start = p.first + R;
  p.after = p.start + R;
  p.sums = p.after + R;
  p.round = p.sums + (size_t)max(p.nchunks_n, p.nchunks_r) + 1;
  p.mask = (uint8_t*)(p.round + kContourMaxRounds);
  return p;
}

// the states of pixel i, for the scan that numbers them
struct PixelStates {
  const uint8_t* mask;
  __device__ uint32_t operator()(uint32_t i) const { return states_of(mask[i]); }
};

// ---- mark ----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void contour_init_kernel(Parts p, uint32_t R) {
  const uint64_t i = global_thread();
  if (i < R) p.first[i] = kNoId;
  if (i < kContourMaxRounds) p.round[i] = 0;
}

__global__ __launch_bounds__(kThreads) void contour_mark_kernel(ContourArgs a, Parts p) {
  const uint64_t i = global_thread();
  if (i >= (uint64_t)a.width * a.height) return;
  const uint32_t W = a.width, H = a.height;
  const uint32_t y = (uint32_t)i / W, x = (uint32_t)i - y * W;
  const uint32_t id = a.regions[i];
  uint32_t m = 0;
  if (id < a.nregions) {
#pragma unroll
    for (uint32_t d = 0; d < 8; ++d) {
      const uint32_t qx = x + (uint32_t)dir_x(d), qy = y + (uint32_t)dir_y(d);   // (below 0 wraps past W, H)
      if (qx < W && qy < H && a.regions[(size_t)qy * W + qx] == id) m |= 1u << d;
    }
    // the first pixel of a region has no NE, N, NW, W of its own id: few pixels ask
    if ((m & 0x1Eu) == 0) atomicMin(&p.first[id], (uint32_t)i);
  }
  p.mask[i] = (uint8_t)m;
}

// ---- starts and links ------------------------------------------------------------
// The state (q, d) of a border pixel q; kNoId when q is no border pixel.
__device__ __forceinline__ uint32_t state_at(const Parts& p, uint32_t q, uint32_t d) {
  const uint32_t m = p.mask[q];
  return border(m) ? p.base[q] + rank_of(m, d) : kNoId;
}

// The state `step` goes to from (i, d), m the on neighbours of pixel i.
__device__ __forceinline__ uint32_t successor(const Parts& p, uint32_t W, uint32_t i, uint32_t m, uint32_t d) {
  const uint32_t s = next_on(m, d);
  const uint32_t q = (uint32_t)((int)i + dir_y(s) * (int)W + dir_x(s));   // (on: in the frame)
  return state_at(p, q, (s + 4u) & 7u);
}

__global__ __launch_bounds__(kThreads) void contour_starts_kernel(ContourArgs a, Parts p) {
  const uint64_t r = global_thread();
  if (r >= a.nregions) return;
  const uint32_t i = p.first[r];
  const uint32_t m = i == kNoId ? 0u : p.mask[i];
  uint32_t start = kNoId, after = kNoId;
  if (m != 0) {   // (W, NW, N, NE are off: a border pixel, and d0 is the first of E, SE, S, SW)
    const uint32_t d0 = (m & 0x01u) ? 0u : (m & 0x80u) ? 7u : (m & 0x40u) ? 6u : 5u;
    start = p.base[i] + rank_of(m, d0);
    after = successor(p, a.width, i, m, d0);
  }
  p.start[r] = start, p.after[r] = after;
  a.len[r] = i == kNoId ? 0u : m == 0 ? 1u : 0u;   // (the lengths pass has the others)
}

__global__ __launch_bounds__(kThreads) void contour_links_kernel(ContourArgs a, Parts p, u64* links) {
  const uint64_t i = global_thread();
  if (i >= (uint64_t)a.width * a.height) return;
  const uint32_t id = a.regions[i];
  if (id >= a.nregions) return;
  const uint32_t m = p.mask[i];
  if (!border(m)) return;
  const uint32_t start = p.start[id];
  uint32_t state = p.base[i];
  for (uint32_t left = m; left; left &= left - 1u, ++state) {
    const uint32_t d = (uint32_t)__ffs((int)left) - 1u;
    links[state] = state == start ? link(state, 0) : link(successor(p, a.width, (uint32_t)i, m, d), 1);
  }
}

// ---- list ranking ----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void contour_jump_kernel(Parts p, uint32_t S, uint32_t R, const u64* __restrict__ in,
                                                               u64* __restrict__ out, uint32_t* todo) {
  const uint64_t i = global_thread();
  if (i < S) {
    u64 w = in[i];
    const uint32_t nx = next_of(w);
    if (nx != kNoId && nx != i) {   // (a sink, or a chain that left the border, stays as it is)
      const u64 v = in[nx];
      w = link(next_of(v), dist_of(w) + dist_of(v));
    }
    out[i] = w;
  }
  if (i < R) {
    const uint32_t after = p.after[i];
    if (after != kNoId && next_of(in[after]) != p.start[i]) *todo = 1;
  }
}

__global__ __launch_bounds__(kThreads) void contour_lengths_kernel(ContourArgs a, Parts p, const u64* __restrict__ links) {
  const uint64_t r = global_thread();
  if (r >= a.nregions) return;
  const uint32_t after = p.after[r];
  if (after == kNoId) return;
  const u64 w = links[after];
  if (next_of(w) == p.start[r]) a.len[r] = dist_of(w) + 1u;
}

// ---- emit ------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void contour_emit_kernel(ContourArgs a, Parts p, const u64* __restrict__ links,
                                                               bool lists) {
  const uint64_t i = global_thread();
  if (i >= (uint64_t)a.width * a.height) return;
  const uint32_t id = a.regions[i];
  uint32_t visits = 0;
  if (id < a.nregions) {
    const uint32_t m = p.mask[i];
    const uint32_t y = (uint32_t)i / a.width, x = (uint32_t)i - y * a.width;
    const uint32_t coord = x | y << 16;
    if (m == 0) {   // a pixel alone: its region's contour iff it is the region's first
      if (p.first[id] == (uint32_t)i) {
        visits = 1;
        if (lists && a.points) a.points[a.offsets[id]] = coord;
        if (lists && a.codes) a.codes[a.offsets[id]] = 8;
      }
    } else if (border(m)) {
      const uint32_t start = p.start[id], len = a.len[id];
      const size_t at = lists ? a.offsets[id] : 0;
      uint32_t state = p.base[i];
      for (uint32_t left = m; left; left &= left - 1u, ++state) {
        const u64 w = links[state];
        if (next_of(w) != start || dist_of(w) >= len) continue;   // (start may be kNoId: no state is)
        ++visits;
        if (!lists) continue;
        const uint32_t j = dist_of(w) == 0 ? 0u : len - dist_of(w);   // the place as followed
        const uint32_t s = next_on(m, (uint32_t)__ffs((int)left) - 1u);
        // reversed: point j goes to len - 1 - j, and the step j -> j + 1 is walked back from there
        if (a.points) a.points[at + (a.orientation ? len - 1u - j : j)] = coord;
        if (a.codes) a.codes[at + (a.orientation ? (j + 1u == len ? len - 1u : len - 2u - j) : j)] =
            (uint8_t)(a.orientation ? (s + 4u) & 7u : s);
      }
    }
  }
  if (a.visits) a.visits[i] = (uint8_t)visits;
}

const u64* links_after(const ContourArgs& a, uint32_t states, uint32_t rounds) {
  return (const u64*)a.links + (size_t)(rounds & 1u) * states;
}

}  // namespace

size_t contour_scratch_bytes(uint32_t width, uint32_t height, uint32_t nregions) {
  const Parts p = carve(nullptr, width, height, nregions);
  const size_t n = (size_t)width * height;
  return 4 * (n + 3 * (size_t)nregions + max(p.nchunks_n, p.nchunks_r) + 1 + kContourMaxRounds) + n;
}

size_t contour_links_bytes(uint32_t states) { return 16 * (size_t)states; }

void launch_contour_mark(const ContourArgs& a, hipStream_t st) {
  const Parts p = carve(a.scratch, a.width, a.height, a.nregions);
  const uint32_t n = a.width * a.height;
  contour_init_kernel<<<blocks_for(max((uint64_t)a.nregions, (uint64_t)kContourMaxRounds)), kThreads, 0, st>>>(p, a.nregions);
  contour_mark_kernel<<<blocks_for(n), kThreads, 0, st>>>(a, p);
  scan::launch(PixelStates{p.mask}, p.base, n, p.sums, st);
}

const uint32_t* contour_states_word(const ContourArgs& a) {
  const Parts p = carve(a.scratch, a.width, a.height, a.nregions);
  return p.sums + p.nchunks_n;
}

void launch_contour_links(const ContourArgs& a, uint32_t states, hipStream_t st) {
  const Parts p = carve(a.scratch, a.width, a.height, a.nregions);
  contour_starts_kernel<<<blocks_for(a.nregions), kThreads, 0, st>>>(a, p);
  if (states) contour_links_kernel<<<blocks_for(a.width * a.height), kThreads, 0, st>>>(a, p, (u64*)a.links);
}

void launch_contour_jump(const ContourArgs& a, uint32_t states, uint32_t round, hipStream_t st) {
  const Parts p = carve(a.scratch, a.width, a.height, a.nregions);
  u64* bufs[2] = {(u64*)a.links, (u64*)a.links + states};
  contour_jump_kernel<<<blocks_for(max((uint64_t)states, (uint64_t)a.nregions)), kThreads, 0, st>>>(
      p, states, a.nregions, bufs[round & 1u], bufs[(round + 1u) & 1u], p.round + round);
}

const uint32_t* contour_round_words(const ContourArgs& a) {
  return carve(a.scratch, a.width, a.height, a.nregions).round;
}

void launch_contour_lengths(const ContourArgs& a, uint32_t states, uint32_t rounds, hipStream_t st) {
  const Parts p = carve(a.scratch, a.width, a.height, a.nregions);
  if (states) contour_lengths_kernel<<<blocks_for(a.nregions), kThreads, 0, st>>>(a, p, links_after(a, states, rounds));
  scan::scan_sums_kernel<scan::Words><<<p.nchunks_r, kThreads, 0, st>>>(scan::Words{a.len}, a.nregions, p.sums);
  scan::scan_top_kernel<<<1, 1024, 0, st>>>(p.sums, p.nchunks_r);
}

const uint32_t* contour_total_word(const ContourArgs& a) {
  const Parts p = carve(a.scratch, a.width, a.height, a.nregions);
  return p.sums + p.nchunks_r;
}

hipError_t launch_contour_emit(const ContourArgs& a, uint32_t states, uint32_t rounds, bool lists, hipStream_t st) {
  const Parts p = carve(a.scratch, a.width, a.height, a.nregions);
  scan::scan_apply_kernel<scan::Words><<<p.nchunks_r, kThreads, 0, st>>>(scan::Words{a.len}, a.offsets, a.nregions, p.sums);
  if (lists || a.visits)
    contour_emit_kernel<<<blocks_for(a.width * a.height), kThreads, 0, st>>>(a, p, links_after(a, states, rounds), lists);
  return hipMemcpyAsync(a.offsets + a.nregions, p.sums + p.nchunks_r, 4, hipMemcpyDeviceToDevice, st);
}

}  // namespace dq
