// dq_windows.hip -- the capture windows of a region map on gfx950 (MI355X).
//
// Input: a width x height row-major map of uint32 region ids, each < R, a block
// size d (1..8) and an expansion e (0..3).  The blocks of the d x d grid that
// hold a pixel of r are own(r); window(r) is every block of the grid at L1
// distance <= e from one of them (e dilations by the 3 x 3 cross).  The list of
// r: the blocks of window(r) in raster order of blocks, in each block its
// pixels in raster order, without the pixels outside the frame and the masked
// ones.  offsets[r] = the total length of the lists of the ids < r; the j-th
// pixel of the list of r is entry offsets[r] + j of every list array.  Every
// output is an integer that does not depend on scheduling.
//
// One pixel is in many lists, so the lists are not a permutation of the map:
// the unit of work is the pair (block b, member id r with b in window(r)), P of
// them, and m(b), the surviving pixels of b.  The position of a pair is split
// as (lengths of lower ids) + (m of the id's window blocks in block rows above)
// + (m of its window blocks to the left in the block row).  The first two are
// one table entry per (id, block row its window spans), laid out id-major; T is
// their number.  A connected region has a window block in every block row its
// window spans, so T <= P for the maps of the connected-regions and merge
// calls; the call refuses a map with T > P before it sizes the table.
//
// Passes (all on the caller's stream; no kernel waits for another workgroup,
// values written by atomics are otherwise read only in later launches):
//   1 blocks   one wave per block, a lane per pixel: m(b), the distinct ids of b
//              (one ballot round per id), per id the first and last block row by
//              atomicMin / atomicMax, gathered per workgroup in 128 LDS slots
//   2 members  one wave per block: the distinct ids of the blocks within L1
//              distance e (a lane per block of the ball reads its count; then 64
//              candidates at a time), deduplicated in an LDS hash set of the
//              wave, without the ids the area rule skips -> c(b); scan ->
//              pairbase[], P
//   3 spans    scan of the block rows each id's window spans -> rowbase[], T
//              (the host reads P and T back, 8 bytes)
//   4 pairs    pass 2 again, writing the pairs (id, block) at pairbase[b]
//   5 count    table[rowbase[r] + row - lo(r)] += m(b) per pair; scan in place:
//              entry (r, row) = the position of the first pixel of r's window in
//              that block row; M is the total (the host reads it back)
//   6 offsets  offsets[r] = table[rowbase[r]]
//   7 walk     one wave per block row, 64 pairs at a time in block order: the
//              lanes with equal ids form a group (ballots, as in dq_pixels.hip),
//              the group's lowest lane takes old = atomicAdd(&table[..], the
//              group's summed m) and a lane's pair starts at old + the m of the
//              lower lanes of its group.  A row's entries are touched by that
//              row's wave alone, one chunk after the other.
//   8 fill     per pair, the block's surviving pixels at the pair's position,
//              ranked in raster order; 64 / d^2 pairs per wave at a time
//
// Ids >= R (not allowed) found no block and are members of none; their pixels
// are pixels of the frame like any other.  No floating point anywhere.
#include <hip/hip_runtime.h>

#include "dq_pixels.h"
#include "dq_scan.h"
#include "dq_stage.h"
#include "dq_windows.h"

namespace dq {
namespace {

using scan::chunks_of;

constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kBlocksPerWave = 16;     // passes 1: consecutive blocks of a wave (its LDS slots serve 64 blocks)
constexpr uint32_t kRowSlots = 128;         // pass 1: LDS slots per workgroup
constexpr uint32_t kMembersPerWave = 8;     // passes 2, 4: consecutive blocks of a wave
constexpr uint32_t kMaxBlock = 8, kMaxExpand = 3;
constexpr uint32_t kMaxMembers = (2 * kMaxExpand * kMaxExpand + 2 * kMaxExpand + 1) * kMaxBlock * kMaxBlock;   // 1600
constexpr uint32_t kSetBits = 11;           // the hash set of a wave: 2048 slots for at most 1600 ids
constexpr uint32_t kSetSlots = 1u << kSetBits;
static_assert(kMaxMembers < kSetSlots, "the set never fills up");

constexpr uint32_t kNoRow = 0xFFFFFFFFu;   // the first block row of an id without a pixel
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

Grid grid_of(const WindowsArgs& a) { return block_grid(a.width, a.height, a.block); }

// the first block row of the window of an id whose first own block row is j0
__device__ __forceinline__ uint32_t window_lo(uint32_t j0, uint32_t e) { return j0 > e ? j0 - e : 0u; }

// ---- 1 blocks ------------------------------------------------------------------
// info[b] = m(b) | distinct ids << 16; ids[b * d^2 ..] = the distinct ids.
__global__ __launch_bounds__(kThreads) void windows_blocks_kernel(const uint32_t* __restrict__ reg,
                                                                 const uint8_t* __restrict__ mask, Grid g, uint32_t R,
                                                                 uint32_t* __restrict__ info, uint32_t* __restrict__ ids,
                                                                 uint32_t* y0, uint32_t* y1) {
  __shared__ uint32_t s_id[kRowSlots], s_lo[kRowSlots], s_hi[kRowSlots];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < kRowSlots) {
    s_id[threadIdx.x] = kNoId;
    s_lo[threadIdx.x] = kNoRow;   // (flushed as they are: a min with all ones, a max with 0 change nothing)
    s_hi[threadIdx.x] = 0;
  }
  __syncthreads();
  const uint32_t lx = lane % g.d, ly = lane / g.d;
#pragma unroll 1
  for (uint32_t k = 0; k < kBlocksPerWave; ++k) {
    const uint32_t b = (blockIdx.x * kWaves + wave) * kBlocksPerWave + k;
    if (b >= g.NB) break;   // (uniform in the wave; the barrier below is outside the loop)
    const uint32_t by = b / g.BW, bx = b - by * g.BW;
    const uint32_t x = bx * g.d + lx, y = by * g.d + ly;
    const bool in = lane < g.dd && x < g.W && y < g.H;
    const uint32_t p = in ? y * g.W + x : 0u;
    uint32_t id = in ? reg[p] : kNoId;
    if (id >= R) id = kNoId;
    const bool alive = in && !(mask && mask[p] != 0);
    const uint32_t m = (uint32_t)__popcll(__ballot(alive));
    uint32_t cnt = 0;
    unsigned long long todo = __ballot(id != kNoId);
    while (todo) {   // one round per distinct id
      const int l = __ffsll(todo) - 1;
      const uint32_t key = __shfl(id, l);
      todo &= ~__ballot(id == key);
      if (lane == (uint32_t)l) {
        ids[(size_t)b * g.dd + cnt] = key;
        const uint32_t slot = key % kRowSlots;
        if (slot_claim(s_id, slot, kNoId, key)) {
          atomicMin(&s_lo[slot], by);
          atomicMax(&s_hi[slot], by);
        } else {
          atomicMin(&y0[key], by);
          atomicMax(&y1[key], by);
        }
      }
      ++cnt;
    }
    if (lane == 0) info[b] = m | (cnt << 16);
  }
  __syncthreads();
  if (threadIdx.x < kRowSlots && s_id[threadIdx.x] != kNoId) {
    atomicMin(&y0[s_id[threadIdx.x]], s_lo[threadIdx.x]);
    atomicMax(&y1[s_id[threadIdx.x]], s_hi[threadIdx.x]);
  }
}

// ---- 2, 4 members --------------------------------------------------------------
// FILL false: counts[b] = |members(b)|.  FILL true: the pairs of b at pairbase[b],
// in the order the set took them (any order does: a block holds an id once).
template <bool FILL>
__global__ __launch_bounds__(kThreads) void windows_members_kernel(Grid g, uint32_t e,
                                                                  const uint32_t* __restrict__ info,
                                                                  const uint32_t* __restrict__ ids,
                                                                  const uint32_t* __restrict__ area, uint32_t min_area,
                                                                  uint32_t* counts, uint32_t P,
                                                                  uint32_t* __restrict__ pair_id,
                                                                  uint32_t* __restrict__ pair_block) {
  __shared__ uint32_t s_set[kWaves][kSetSlots];
  __shared__ uint16_t s_used[kWaves][kMaxMembers];
  __shared__ uint32_t s_start[kWaves][32], s_block[kWaves][32];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t* set = s_set[wave];   // this wave's alone (a wave's LDS accesses run in order)
  uint16_t* used = s_used[wave];
  uint32_t *start = s_start[wave], *block = s_block[wave];
  for (uint32_t j = lane; j < kSetSlots; j += 64) set[j] = kNoId;
  // lane t < 2 e^2 + 2 e + 1 (at most 25): the t-th offset of the L1 ball, row by row
  int dy = 0, dx = 0;
  bool ball = false;
  {
    int t = (int)lane;
    for (int yy = -(int)e; yy <= (int)e; ++yy) {
      const int reach = (int)e - (yy < 0 ? -yy : yy), width = 2 * reach + 1;
      if (t >= 0 && t < width) dy = yy, dx = t - reach, ball = true;
      t -= width;
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (uint32_t k = 0; k < kMembersPerWave; ++k) {
    const uint32_t b = (blockIdx.x * kWaves + wave) * kMembersPerWave + k;
    if (b >= g.NB) break;   // (uniform in the wave; the kernel has no workgroup barrier)
    const int by = (int)(b / g.BW), bx = (int)(b - (uint32_t)by * g.BW);
    const uint32_t base = FILL ? counts[b] : 0u;   // (counts is pairbase by then)
    // The candidates: the distinct ids of the ball's blocks, one after the other.  A lane per block
    // of the ball reads how many it has; their prefix sums say which block candidate c belongs to.
    const int ny = by + dy, nx = bx + dx;
    const bool there = ball && ny >= 0 && ny < (int)g.BH && nx >= 0 && nx < (int)g.BW;
    const uint32_t nb = there ? (uint32_t)ny * g.BW + (uint32_t)nx : 0u;
    const uint32_t have = there ? info[nb] >> 16 : 0u;
    uint32_t inc = have;
#pragma unroll
    for (uint32_t d = 1; d < 32; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    const uint32_t candidates = __shfl(inc, 31);   // (lanes 25 .. 31 have none)
    if (lane < 32) {
      start[lane] = inc - have;
      block[lane] = nb;
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t count = 0;
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < candidates; c0 += 64) {
      const uint32_t c = c0 + lane;
      uint32_t id = kNoId;
      if (c < candidates) {
        uint32_t t = 0;   // the last block of the ball that starts at or before c: it has candidate c
#pragma unroll
        for (uint32_t step = 16; step > 0; step >>= 1)
          if (start[t + step] <= c) t += step;
        id = ids[(size_t)block[t] * g.dd + (c - start[t])];
        if (area && area[id] <= min_area) id = kNoId;
      }
      bool fresh = false;
      uint32_t s = (id * 2654435761u) >> (32 - kSetBits);
      if (id != kNoId) {
        for (;;) {   // (ends: the set has more slots than a block has members)
          const uint32_t was = atomicCAS(&set[s], kNoId, id);
          if (was == kNoId) fresh = true;
          if (was == kNoId || was == id) break;
          s = (s + 1) & (kSetSlots - 1);
        }
      }
      const unsigned long long news = __ballot(fresh);
      const uint32_t at = count + (uint32_t)__popcll(news & ((1ull << lane) - 1ull));
      if (fresh && at < kMaxMembers) {
        used[at] = (uint16_t)s;
        if (FILL && base + at < P) {
          pair_id[base + at] = id;
          pair_block[base + at] = b;
        }
      }
      count += (uint32_t)__popcll(news);
    }
    __builtin_amdgcn_wave_barrier();
    for (uint32_t j = lane; j < count && j < kMaxMembers; j += 64) set[used[j]] = kNoId;   // (free for the next block)
    __builtin_amdgcn_wave_barrier();   // (start[] and block[] are the next block's from here on)
    if (!FILL && lane == 0) counts[b] = count;
  }
}

// ---- 3 spans -------------------------------------------------------------------
// Element r: the block rows the window of r spans, 0 for an id without a pixel
// or one the area rule skips.  y1 = the array scanned in place.
struct Spans {
  const uint32_t *y0, *y1, *area;
  uint32_t min_area, e, BH;
  __device__ uint32_t operator()(uint32_t r) const {
    const uint32_t j0 = y0[r];
    if (j0 == kNoRow || (area && area[r] <= min_area)) return 0u;
    const uint32_t j1 = y1[r], hi = j1 + e < BH ? j1 + e : BH - 1;
    return hi - window_lo(j0, e) + 1u;
  }
};

// ---- 5 count -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void windows_count_kernel(uint32_t P, uint32_t T, uint32_t e, uint32_t BW,
                                                                uint32_t NB, uint32_t R,
                                                                const uint32_t* __restrict__ pair_id,
                                                                const uint32_t* __restrict__ pair_block,
                                                                const uint32_t* __restrict__ info,
                                                                const uint32_t* __restrict__ y0,
                                                                const uint32_t* __restrict__ rowbase, uint32_t* table) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= P) return;
  const uint32_t id = pair_id[i], b = pair_block[i];
  if (id >= R || b >= NB) return;   // (never: pass 4 wrote every pair)
  const uint32_t m = info[b] & 0xFFFFu;
  if (m == 0) return;
  const uint32_t slot = rowbase[id] + (b / BW - window_lo(y0[id], e));
  if (slot < T) atomicAdd(&table[slot], m);
}

// ---- 7 walk --------------------------------------------------------------------
// pair_id[i] becomes the position of pair i.
__global__ __launch_bounds__(kThreads) void windows_walk_kernel(Grid g, uint32_t e, uint32_t R, uint32_t P, uint32_t T,
                                                               const uint32_t* __restrict__ pairbase,
                                                               uint32_t* pair_id, const uint32_t* __restrict__ pair_block,
                                                               const uint32_t* __restrict__ info,
                                                               const uint32_t* __restrict__ y0,
                                                               const uint32_t* __restrict__ rowbase, uint32_t* table) {
  __shared__ uint32_t s_slots[kWaves][kWalkSlots];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t by = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (by >= g.BH) return;   // (whole waves; the kernel has no barrier)
  uint32_t* slots = s_slots[threadIdx.x >> 6];   // this wave's alone
  for (uint32_t j = lane; j < kWalkSlots; j += 64) slots[j] = kNoId;
  __builtin_amdgcn_wave_barrier();
  const uint32_t first = pairbase[by * g.BW];
  uint32_t last = pairbase[by * g.BW + g.BW];   // (pairbase has NB + 1 entries)
  if (last > P) last = P;
#pragma unroll 1
  for (uint32_t i0 = first; i0 < last; i0 += 64) {
    const uint32_t i = i0 + lane;
    uint32_t id = kNoId, slot = kNoSlot, m = 0;
    if (i < last) {
      id = pair_id[i];
      const uint32_t b = pair_block[i];
      if (id < R && b < g.NB) {   // (always: pass 4 wrote every pair)
        m = info[b] & 0xFFFFu;
        slot = rowbase[id] + (by - window_lo(y0[id], e));
      }
    }
    const bool valid = slot < T;
    // Groups of equal ids (dq_stage.h).  A group's lanes are in block order (the pairs are
    // block-major, a block holds an id once): the start of a lane is the m of the group's lower
    // lanes, the group's size their sum; a lane in no round is alone with its id.
    uint32_t before = 0, size = m, leader = lane;
    wave_id_groups(slots, id, valid, [&](bool mine, unsigned long long group, int) {
      uint32_t inc = mine ? m : 0u;   // inclusive prefix sums of the group's m over the wave
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
      }
      const uint32_t sum = __shfl(inc, 63);
      if (mine) {
        before = inc - m;
        size = sum;
        leader = (uint32_t)(__ffsll(group) - 1);
      }
    });
    uint32_t old = 0;
    if (valid && leader == lane) old = atomicAdd(&table[slot], size);
    old = __shfl(old, (int)leader);
    if (valid) pair_id[i] = old + before;
  }
}

// ---- 8 fill --------------------------------------------------------------------
// One wave per block; lane = pair-in-flight * d^2 + pixel of the block.
__global__ __launch_bounds__(kThreads) void windows_fill_kernel(Grid g, uint32_t P, uint32_t M,
                                                               const uint8_t* __restrict__ mask,
                                                               const uint32_t* __restrict__ pairbase,
                                                               const uint32_t* __restrict__ pair_pos,
                                                               const uint32_t* __restrict__ pixels,
                                                               uint32_t* __restrict__ index, uint32_t* __restrict__ coords,
                                                               uint32_t* __restrict__ colors) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= g.NB) return;   // (whole waves; the kernel has no barrier)
  const uint32_t first = pairbase[b];
  uint32_t last = pairbase[b + 1];
  if (last > P) last = P;
  if (first >= last) return;
  const uint32_t by = b / g.BW, bx = b - by * g.BW;
  const uint32_t flight = 64u / g.dd, sub = lane / g.dd, l = lane - sub * g.dd;
  const uint32_t x = bx * g.d + l % g.d, y = by * g.d + l / g.d;
  const bool in = sub < flight && x < g.W && y < g.H;
  const uint32_t p = in ? y * g.W + x : 0u;
  const bool alive = in && !(mask && mask[p] != 0);
  // the rank of the pixel among the block's surviving ones: the lower lanes of its own copy of the block
  const unsigned long long copy = __ballot(alive) >> (sub * g.dd);
  const uint32_t rank = (uint32_t)__popcll(copy & ((1ull << l) - 1ull));
  const uint32_t px = (alive && colors) ? pixels[p] : 0u;
#pragma unroll 1
  for (uint32_t i0 = first; i0 < last; i0 += flight) {
    const uint32_t i = i0 + sub;
    if (!alive || i >= last) continue;
    const uint32_t pos = pair_pos[i] + rank;
    if (pos < M) {
      if (index) index[pos] = p;
      if (coords) coords[pos] = x | (y << 16);
      if (colors) colors[pos] = px;
    }
  }
}

// The scratch of the first part, in words: info | ids | counts (pairbase) | its sums | y0 | y1 (rowbase) | its sums
struct BlocksLayout {
  size_t info, ids, counts, csums, y0, y1, rsums, words;
};

BlocksLayout blocks_layout(const Grid& g, uint32_t R) {
  BlocksLayout l;
  l.info = 0;
  l.ids = l.info + g.NB;
  l.counts = l.ids + (size_t)g.NB * g.dd;
  l.csums = l.counts + (size_t)g.NB + 1;
  l.y0 = l.csums + chunks_of(g.NB + 1) + 1;
  l.y1 = l.y0 + R;
  l.rsums = l.y1 + R;
  l.words = l.rsums + chunks_of(R) + 1;
  return l;
}

}  // namespace

size_t windows_blocks_bytes(uint32_t width, uint32_t height, uint32_t block, uint32_t nregions) {
  WindowsArgs a{};
  a.width = width, a.height = height, a.block = block;
  return blocks_layout(grid_of(a), nregions).words * 4;
}

// pair ids (then positions) | pair blocks | the table | its sums
size_t windows_pairs_bytes(uint32_t npairs, uint32_t nrows) {
  const uint32_t t = nrows ? nrows : 1u;
  return ((size_t)npairs * 2 + t + chunks_of(t) + 1) * 4;
}

const uint32_t* windows_pairs_word(const WindowsArgs& a) {
  const Grid g = grid_of(a);
  return a.blocks + blocks_layout(g, a.nregions).csums + chunks_of(g.NB + 1);
}

const uint32_t* windows_rows_word(const WindowsArgs& a) {
  return a.blocks + blocks_layout(grid_of(a), a.nregions).rsums + chunks_of(a.nregions);
}

const uint32_t* windows_total_word(const WindowsArgs& a, uint32_t npairs, uint32_t nrows) {
  return a.pairs + (size_t)npairs * 2 + nrows + chunks_of(nrows);
}

void launch_windows_blocks(const WindowsArgs& a, hipStream_t st) {
  const Grid g = grid_of(a);
  const uint32_t R = a.nregions;
  const BlocksLayout l = blocks_layout(g, R);
  uint32_t *info = a.blocks + l.info, *ids = a.blocks + l.ids, *counts = a.blocks + l.counts;
  uint32_t *y0 = a.blocks + l.y0, *y1 = a.blocks + l.y1;
  (void)hipMemsetAsync(y0, 0xFF, (size_t)R * 4, st);
  (void)hipMemsetAsync(y1, 0, (size_t)R * 4, st);
  (void)hipMemsetAsync(counts + g.NB, 0, 4, st);   // (the scan's last entry: pairbase[NB] = P)
  const uint32_t per1 = kWaves * kBlocksPerWave, per2 = kWaves * kMembersPerWave;
  windows_blocks_kernel<<<(g.NB + per1 - 1) / per1, kThreads, 0, st>>>(a.regions, a.mask, g, R, info, ids, y0, y1);
  windows_members_kernel<false><<<(g.NB + per2 - 1) / per2, kThreads, 0, st>>>(g, a.expand, info, ids, a.area,
                                                                              a.min_area, counts, 0, nullptr, nullptr);
  scan::launch(scan::Words{counts}, counts, g.NB + 1, a.blocks + l.csums, st);   // counts is pairbase from here on
  scan::launch(Spans{y0, y1, a.area, a.min_area, a.expand, g.BH}, y1, R, a.blocks + l.rsums, st);   // y1 is rowbase
}

void launch_windows_count(const WindowsArgs& a, uint32_t P, uint32_t T, hipStream_t st) {
  if (P == 0 || T == 0) return;
  const Grid g = grid_of(a);
  const BlocksLayout l = blocks_layout(g, a.nregions);
  uint32_t *pair_id = a.pairs, *pair_block = pair_id + P, *table = pair_block + P;
  const uint32_t per2 = kWaves * kMembersPerWave;
  windows_members_kernel<true><<<(g.NB + per2 - 1) / per2, kThreads, 0, st>>>(
      g, a.expand, a.blocks + l.info, a.blocks + l.ids, a.area, a.min_area, a.blocks + l.counts, P, pair_id, pair_block);
  (void)hipMemsetAsync(table, 0, (size_t)T * 4, st);
  windows_count_kernel<<<(P - 1) / kThreads + 1, kThreads, 0, st>>>(P, T, a.expand, g.BW, g.NB, a.nregions, pair_id,
                                                                   pair_block,
                                                                   a.blocks + l.info, a.blocks + l.y0, a.blocks + l.y1,
                                                                   table);
  scan::launch(scan::Words{table}, table, T, table + T, st);
}

void launch_windows_offsets(const WindowsArgs& a, uint32_t P, uint32_t T, uint32_t M, hipStream_t st) {
  const BlocksLayout l = blocks_layout(grid_of(a), a.nregions);
  const uint32_t R = a.nregions;
  launch_list_offsets(R, P ? T : 0u, M, a.blocks + l.y1, a.pairs + (size_t)P * 2, a.offsets, st);   // 6 offsets
}

WindowsView windows_view(const WindowsArgs& a, uint32_t P) {
  const Grid g = grid_of(a);
  const BlocksLayout l = blocks_layout(g, a.nregions);
  return WindowsView{a.blocks + l.info, a.blocks + l.ids, a.blocks + l.counts, a.pairs, a.pairs + P, g.NB};
}

void launch_windows_walk(const WindowsArgs& a, uint32_t P, uint32_t T, hipStream_t st) {
  if (P == 0 || T == 0) return;
  const Grid g = grid_of(a);
  const BlocksLayout l = blocks_layout(g, a.nregions);
  uint32_t *pair_id = a.pairs, *pair_block = pair_id + P, *table = pair_block + P;
  windows_walk_kernel<<<(g.BH + kWaves - 1) / kWaves, kThreads, 0, st>>>(g, a.expand, a.nregions, P, T, a.blocks + l.counts,
                                                                        pair_id,
                                                                        pair_block, a.blocks + l.info, a.blocks + l.y0,
                                                                        a.blocks + l.y1, table);
}

void launch_windows_lists(const WindowsArgs& a, uint32_t P, uint32_t T, uint32_t M, hipStream_t st) {
  if (P == 0 || T == 0 || M == 0 || !(a.index || a.coords || a.colors)) return;
  const Grid g = grid_of(a);
  const BlocksLayout l = blocks_layout(g, a.nregions);
  uint32_t* pair_id = a.pairs;
  launch_windows_walk(a, P, T, st);
  windows_fill_kernel<<<(g.NB + kWaves - 1) / kWaves, kThreads, 0, st>>>(g, P, M, a.mask, a.blocks + l.counts, pair_id,
                                                                        a.pixels, a.index, a.coords, a.colors);
}

}  // namespace dq
