// dq_wtags.hip -- the tag histogram of every capture window of a region map, and
// the inside / outside votes of a window's quant, on gfx950 (MI355X).
//
// Tags.  With the lists of dq_windows.hip: for a region r with a window and an
// id s < R, c(r, s) = the entries of the list of r whose pixel has id s and
// f(r, s) = the first of them, relative to the start of the list.  Row r = the
// ids with c(r, s) > 0 in ascending f(r, s).  Every output is an integer that
// does not depend on scheduling.
//
// The lists are never built.  The unit of work is the contribution: a pair
// (block b, member id r) of the windows stage and an id s with a surviving pixel
// in b.  It carries n = the surviving pixels of s in b and pos = the pair's list
// position + the rank of the first surviving pixel of s among the surviving
// pixels of b (both ballots over the block's lanes).  c(r, s) is the sum of n and
// offsets[r] + f(r, s) the minimum of pos over the contributions of (r, s).  The
// first positions of two entries differ (a list position holds one pixel), so
// one bit per first position in a bitmap over the M list positions orders all
// entries at once: row-major, and in a row by f.  An entry's index is the rank
// of its bit, rows[r] the rank at offsets[r].
//
// Passes (all on the caller's stream; no kernel waits for another workgroup,
// values written by atomics are read only in later launches):
//   1 live     one wave per block, a lane per pixel: live(b) = the distinct ids
//              < R with a surviving pixel (one ballot round per id); Q = the sum
//              over the blocks of live(b) * members(b) by the scan's first two
//              kernels (the host reads Q back and sizes the table from it)
//   2 insert   one wave per block: the (s, n, rank) of its live ids, one per lane;
//              then 64 contributions at a time, each claiming or finding (r, s)
//              in an open-addressing table (64-bit atomicCAS, linear probing, at
//              most half full), count += n, first = min(first, pos); a workgroup
//              first gathers its contributions in 128 LDS slots (slot free or the
//              key's, else straight to the table) and flushes them once
//   3 entries  per slot in use: the bit of its first position (atomicOr), inside[r]
//              for s = r, else atomicMax(best[r], count << 32 | ~s): the largest
//              count, ties to the lowest id
//   4 rank     scan of the popcounts of the bitmap's words; E is the total (the
//              host reads it back and decides E <= cap)
//   5 rows     rows[r] = rank(offsets[r]); inside, best, best_count per region
//   6 emit     per slot in use: s, c, f at rank(first)
//
// Votes.  For entry j of the list of r: side = 0 if the pixel's id is r, else 1;
// i = the lowest i < k_outs[r] whose colortable entry equals the mapped colour in
// its low 24 bits; votes[(2 r + side) k + i] += 1.  A job is up to 2048
// consecutive entries of one list and belongs to one wave, which keeps the row of
// the colortable and its 2 k bins in LDS and flushes the bins with atomics: a
// long list is many jobs in many workgroups, short lists share a workgroup a wave
// each.  The first job of every region is a scan over the regions; a wave finds
// its region by bisection.
//
// No floating point anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dq_scan.h"
#include "dq_stage.h"
#include "dq_table.h"
#include "dq_windows.h"
#include "dq_wtags.h"

namespace dq {
namespace {

using scan::chunks_of;
using table::kNoKey;
using table::mix;

constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kBlocksPerWave = 8;      // passes 1, 2: consecutive blocks of a wave
constexpr uint32_t kSlots = 128;            // pass 2: LDS slots per workgroup
constexpr uint32_t kNoPos = 0xFFFFFFFFu;   // M <= 2^32 - 2: never a list position

// (nblocks is the grid's block count: the windows stage's view gave it)
Grid grid_of(const WtagsArgs& a) { return block_grid(a.width, a.height, a.block); }

// ---- 1 live --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wtags_live_kernel(const uint32_t* __restrict__ reg,
                                                             const uint8_t* __restrict__ mask, Grid g, uint32_t R,
                                                             uint32_t* __restrict__ live) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (uint32_t k = 0; k < kBlocksPerWave; ++k) {
    const uint32_t b = (blockIdx.x * kWaves + wave) * kBlocksPerWave + k;
    if (b >= g.NB) break;   // (uniform in the wave; the kernel has no barrier)
    uint32_t id;
    bool alive;
    block_pixel(reg, mask, g, R, b, lane, id, alive);
    uint32_t cnt = 0;
    unsigned long long todo = __ballot(alive && id != kNoId);
    while (todo) {   // one round per distinct id
      const uint32_t key = __shfl(id, __ffsll(todo) - 1);
      todo &= ~__ballot(id == key);
      ++cnt;
    }
    if (lane == 0) live[b] = cnt;
  }
}

// Element b: the contributions of block b (<= 64 * 1600).
struct Contribs {
  const uint32_t *live, *pairbase;
  __device__ uint32_t operator()(uint32_t b) const { return live[b] * (pairbase[b + 1] - pairbase[b]); }
};

// ---- 2 insert ------------------------------------------------------------------
struct Table {
  unsigned long long* key;   // kNoKey: free; else r << 32 | s
  uint32_t* first;           // starts as kNoPos
  uint32_t* count;           // starts as 0
  uint32_t slots;            // >= 2 Q (any number: a slot is a 32-bit hash scaled to it)
};

__device__ __forceinline__ uint32_t home_slot(const Table& t, unsigned long long key) {
  return (uint32_t)(((mix(key) & 0xFFFFFFFFull) * t.slots) >> 32);   // (the LDS slots take the top bits)
}

__device__ __forceinline__ void table_add(const Table& t, unsigned long long key, uint32_t n, uint32_t pos) {
  const uint32_t s = table::table_claim(t.key, t.slots, home_slot(t, key), key);
  atomicAdd(&t.count[s], n);
  atomicMin(&t.first[s], pos);
}

__global__ __launch_bounds__(kThreads) void wtags_insert_kernel(const uint32_t* __restrict__ reg,
                                                               const uint8_t* __restrict__ mask, Grid g, uint32_t R,
                                                               uint32_t P, uint32_t M,
                                                               const uint32_t* __restrict__ pairbase,
                                                               const uint32_t* __restrict__ pair_id,
                                                               const uint32_t* __restrict__ pair_pos, Table t) {
  __shared__ unsigned long long s_key[kSlots];
  __shared__ uint32_t s_count[kSlots], s_first[kSlots];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < kSlots) {
    s_key[threadIdx.x] = kNoKey;
    s_count[threadIdx.x] = 0;
    s_first[threadIdx.x] = kNoPos;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t k = 0; k < kBlocksPerWave; ++k) {
    const uint32_t b = (blockIdx.x * kWaves + wave) * kBlocksPerWave + k;
    if (b >= g.NB) break;   // (uniform in the wave; the barrier below is outside the loop)
    const uint32_t first = pairbase[b];
    uint32_t last = pairbase[b + 1];
    if (last > P) last = P;
    if (first >= last) continue;
    uint32_t id;
    bool alive;
    block_pixel(reg, mask, g, R, b, lane, id, alive);
    const unsigned long long living = __ballot(alive);
    // lane j keeps the j-th live id of the block: s, its surviving pixels and the rank of the first of them
    uint32_t my_s = kNoId, my_n = 0, my_rank = 0, cnt = 0;
    unsigned long long todo = __ballot(alive && id != kNoId);
    while (todo) {   // one round per distinct id, in the order of their first surviving pixels
      const int l = __ffsll(todo) - 1;
      const uint32_t key = __shfl(id, l);
      const unsigned long long group = __ballot(alive && id == key);
      if (lane == cnt) {
        my_s = key;
        my_n = (uint32_t)__popcll(group);
        my_rank = (uint32_t)__popcll(living & ((1ull << l) - 1ull));
      }
      todo &= ~group;
      ++cnt;
    }
    if (cnt == 0) continue;
    const uint32_t items = (last - first) * cnt;   // (<= 1600 * 64)
#pragma unroll 1
    for (uint32_t t0 = 0; t0 < items; t0 += 64) {   // (uniform: every lane takes part in the shuffles)
      const uint32_t it = t0 + lane;
      const bool on = it < items;
      const uint32_t pi = on ? it / cnt : 0u, si = on ? it - pi * cnt : 0u;
      const uint32_t s = __shfl(my_s, (int)si), n = __shfl(my_n, (int)si), rank = __shfl(my_rank, (int)si);
      if (!on) continue;
      const uint32_t r = pair_id[first + pi];
      const uint32_t pos = pair_pos[first + pi] + rank;
      if (r >= R || pos >= M) continue;   // (never: the windows stage wrote every pair)
      const unsigned long long key = ((unsigned long long)r << 32) | s;
      const uint32_t slot = (uint32_t)(mix(key) >> 57);   // (the table takes the low half)
      static_assert(kSlots == 128, "the top 7 bits of the hash");
      if (slot_claim(s_key, slot, kNoKey, key)) {   // (<= 32 blocks of 64 pixels a workgroup: the u32 sum holds)
        atomicAdd(&s_count[slot], n);
        atomicMin(&s_first[slot], pos);
      } else {
        table_add(t, key, n, pos);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kSlots && s_key[threadIdx.x] != kNoKey)
    table_add(t, s_key[threadIdx.x], s_count[threadIdx.x], s_first[threadIdx.x]);
}

// ---- 3 entries -----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wtags_mark_kernel(Table t, uint32_t R, uint32_t M,
                                                             uint32_t* __restrict__ bits, uint32_t* __restrict__ inside,
                                                             unsigned long long* __restrict__ best) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= t.slots) return;
  const unsigned long long key = t.key[i];
  if (key == kNoKey) return;
  const uint32_t r = (uint32_t)(key >> 32), s = (uint32_t)key, c = t.count[i], f = t.first[i];
  if (r >= R || f >= M) return;   // (never)
  atomicOr(&bits[f >> 5], 1u << (f & 31u));
  if (s == r)
    inside[r] = c;   // (one entry per key)
  else
    atomicMax(&best[r], ((unsigned long long)c << 32) | (uint32_t)~s);
}

// ---- 4 rank --------------------------------------------------------------------
struct Popcounts {
  const uint32_t* bits;
  __device__ uint32_t operator()(uint32_t i) const { return (uint32_t)__popc(bits[i]); }
};

// the set bits below list position p
__device__ __forceinline__ uint32_t rank_of(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ ranks,
                                            uint32_t p) {
  return ranks[p >> 5] + (uint32_t)__popc(bits[p >> 5] & ((1u << (p & 31u)) - 1u));
}

// ---- 5 rows --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wtags_rows_kernel(uint32_t R, uint32_t M,
                                                             const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ bits,
                                                             const uint32_t* __restrict__ ranks,
                                                             const uint32_t* __restrict__ inside,
                                                             const unsigned long long* __restrict__ best,
                                                             uint32_t* __restrict__ rows, uint32_t* __restrict__ out_inside,
                                                             uint32_t* __restrict__ out_best,
                                                             uint32_t* __restrict__ out_best_count) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r > R) return;
  uint32_t o = offsets[r];
  if (o > M) o = M;   // (never)
  rows[r] = rank_of(bits, ranks, o);
  if (r == R) return;
  const unsigned long long v = best[r];
  if (out_inside) out_inside[r] = inside[r];
  if (out_best) out_best[r] = v ? ~(uint32_t)v : kNoId;
  if (out_best_count) out_best_count[r] = (uint32_t)(v >> 32);
}

// ---- 6 emit --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wtags_emit_kernel(Table t, uint32_t R, uint32_t M, uint32_t E,
                                                             const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ bits,
                                                             const uint32_t* __restrict__ ranks,
                                                             uint32_t* __restrict__ ids, uint32_t* __restrict__ counts,
                                                             uint32_t* __restrict__ first) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= t.slots) return;
  const unsigned long long key = t.key[i];
  if (key == kNoKey) return;
  const uint32_t r = (uint32_t)(key >> 32), f = t.first[i];
  if (r >= R || f >= M) return;   // (never)
  const uint32_t at = rank_of(bits, ranks, f);
  if (at >= E) return;            // (never: E counts every bit)
  if (ids) ids[at] = (uint32_t)key;
  if (counts) counts[at] = t.count[i];
  if (first) first[at] = f - offsets[r];
}

// Twice the contributions (so at most half the slots are ever claimed), as a 32-bit count: from
// Q = 2^31 on the table is fuller than half, and still never full (Q <= 2^32 - 2 < slots).
uint32_t table_slots(uint32_t Q) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(2 * (uint64_t)Q, table::kMinTableSlots), 0xFFFFFFFFull);
}

uint32_t bit_words(uint32_t M) { return M / 32u + 2u; }   // (word M >> 5 exists, and one more: its rank is E)

// keys | firsts (both start as all ones) | counts | best | inside | bits (all four start as 0) |
// ranks | their sums
struct TableLayout {
  uint32_t slots;
  size_t key, first, count, best, inside, bits, ranks, sums, words;
};

TableLayout table_layout(uint32_t Q, uint32_t M, uint32_t R) {
  TableLayout l;
  l.slots = table_slots(Q);
  l.key = 0;
  l.first = l.key + 2 * (size_t)l.slots;
  l.count = l.first + l.slots;
  l.best = l.count + l.slots;   // (4 * slots words from the start: 8-byte aligned whatever slots is)
  l.inside = l.best + 2 * (size_t)R;
  l.bits = l.inside + R;
  l.ranks = l.bits + bit_words(M);
  l.sums = l.ranks + bit_words(M);
  l.words = l.sums + chunks_of(bit_words(M)) + 1;
  return l;
}

Table table_of(const WtagsArgs& a, const TableLayout& l) {
  return Table{(unsigned long long*)(a.table + l.key), a.table + l.first, a.table + l.count, l.slots};
}

// ---- votes ---------------------------------------------------------------------
// Element r: the jobs of the list of r (0 for offsets that are not a list's).
struct Jobs {
  const uint32_t* offsets;
  uint32_t R, total;
  __device__ uint32_t operator()(uint32_t r) const {
    if (r >= R) return 0u;
    const uint32_t lo = offsets[r], hi = offsets[r + 1];
    if (lo >= hi || hi > total) return 0u;
    return (hi - lo - 1) / kVotesSegment + 1u;
  }
};

__global__ __launch_bounds__(kThreads) void wvotes_kernel(WvotesArgs a, const uint32_t* __restrict__ jobbase,
                                                         unsigned long long* misses) {
  __shared__ uint32_t s_ct[kWaves][kVotesMaxK], s_bins[kWaves][2 * kVotesMaxK];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t R = a.nregions, k = a.k;
  const uint32_t j = blockIdx.x * kWaves + wave;
  if (j >= jobbase[R]) return;   // (whole waves; the kernel has no workgroup barrier)
  uint32_t r = 0, hi = R;        // the last r with jobbase[r] <= j: the one job j belongs to
  while (hi - r > 1) {
    const uint32_t mid = r + (hi - r) / 2;
    if (jobbase[mid] <= j)
      r = mid;
    else
      hi = mid;
  }
  const uint32_t start = a.offsets[r] + (j - jobbase[r]) * kVotesSegment;
  uint32_t len = a.offsets[r + 1] - start;   // this job's entries: start .. start + len
  if (len > kVotesSegment) len = kVotesSegment;
  uint32_t kout = a.k_outs[r];
  if (kout > k) kout = k;
  uint32_t *ct = s_ct[wave], *bins = s_bins[wave];   // this wave's alone (a wave's LDS accesses run in order)
  for (uint32_t i = lane; i < kout; i += 64) ct[i] = a.cts[(size_t)r * k + i] & 0xFFFFFFu;
  for (uint32_t i = lane; i < 2 * k; i += 64) bins[i] = 0;
  __builtin_amdgcn_wave_barrier();
  uint32_t missed = 0;
#pragma unroll 1
  for (uint32_t o0 = 0; o0 < len; o0 += 64) {   // (offsets into the job, not positions: start + 64 may pass 2^32)
    const uint32_t o = o0 + lane, e = start + o;
    bool miss = false;
    if (o < len) {
      const uint32_t p = a.index[e], v = a.mapped[e] & 0xFFFFFFu;
      uint32_t i = 0;
      while (i < kout && ct[i] != v) ++i;
      miss = i == kout || p >= a.n;   // (a pixel index outside the map: the entry is no list's)
      if (!miss) atomicAdd(&bins[(a.regions[p] == r ? 0u : k) + i], 1u);
    }
    missed += (uint32_t)__popcll(__ballot(miss));
  }
  __builtin_amdgcn_wave_barrier();
  uint32_t* out = a.votes + (size_t)r * 2 * k;
  for (uint32_t i = lane; i < 2 * k; i += 64)
    if (bins[i]) atomicAdd(&out[i], bins[i]);
  if (lane == 0 && missed) atomicAdd(misses, (unsigned long long)missed);
}

// best[2 r + side] = the lowest i with the largest non-zero count.
__global__ __launch_bounds__(kThreads) void wvotes_best_kernel(uint32_t R, uint32_t k,
                                                              const uint32_t* __restrict__ votes,
                                                              uint32_t* __restrict__ best) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2ull * R) return;
  const uint32_t* v = votes + (size_t)i * k;
  uint32_t at = kNoId, most = 0;
  for (uint32_t c = 0; c < k; ++c)
    if (v[c] > most) most = v[c], at = c;
  best[i] = at;
}

}  // namespace

size_t wtags_live_bytes(uint32_t nblocks) { return ((size_t)nblocks + chunks_of(nblocks) + 1) * 4; }

size_t wtags_table_bytes(uint32_t Q, uint32_t M, uint32_t R) { return table_layout(Q, M, R).words * 4; }

void launch_wtags_count(const WtagsArgs& a, hipStream_t st) {
  const Grid g = grid_of(a);
  const uint32_t per = kWaves * kBlocksPerWave, nchunks = chunks_of(g.NB);
  uint32_t* sums = a.live + g.NB;
  wtags_live_kernel<<<(g.NB + per - 1) / per, kThreads, 0, st>>>(a.regions, a.mask, g, a.nregions, a.live);
  const Contribs value{a.live, a.pairbase};
  scan::scan_sums_kernel<Contribs><<<nchunks, scan::kThreads, 0, st>>>(value, g.NB, sums);
  scan::scan_top_kernel<<<1, 1024, 0, st>>>(sums, nchunks);
}

const uint32_t* wtags_contribs_word(const WtagsArgs& a) { return a.live + a.nblocks + chunks_of(a.nblocks); }

void launch_wtags_fill(const WtagsArgs& a, uint32_t Q, hipStream_t st) {
  const Grid g = grid_of(a);
  const uint32_t R = a.nregions;
  const TableLayout l = table_layout(Q, a.total, R);
  const Table t = table_of(a, l);
  const uint32_t nbits = bit_words(a.total);
  uint32_t *bits = a.table + l.bits, *ranks = a.table + l.ranks;
  if (Q == 0) {
    (void)hipMemsetAsync(a.table + l.best, 0, (l.ranks - l.best) * 4, st);    // best | inside | bits
  } else {
    (void)hipMemsetAsync(t.key, 0xFF, (l.count - l.key) * 4, st);             // keys | firsts
    (void)hipMemsetAsync(t.count, 0, (l.ranks - l.count) * 4, st);            // counts | best | inside | bits
    const uint32_t per = kWaves * kBlocksPerWave;
    wtags_insert_kernel<<<(g.NB + per - 1) / per, kThreads, 0, st>>>(a.regions, a.mask, g, R, a.npairs, a.total,
                                                                    a.pairbase, a.pair_id, a.pair_pos, t);
    wtags_mark_kernel<<<(l.slots - 1) / kThreads + 1, kThreads, 0, st>>>(
        t, R, a.total, bits, a.table + l.inside, (unsigned long long*)(a.table + l.best));
  }
  scan::launch(Popcounts{bits}, ranks, nbits, a.table + l.sums, st);
}

const uint32_t* wtags_entries_word(const WtagsArgs& a, uint32_t Q) {
  const TableLayout l = table_layout(Q, a.total, a.nregions);
  return a.table + l.sums + chunks_of(bit_words(a.total));
}

void launch_wtags_rows(const WtagsArgs& a, uint32_t Q, hipStream_t st) {
  const uint32_t R = a.nregions;
  const TableLayout l = table_layout(Q, a.total, R);
  wtags_rows_kernel<<<R / kThreads + 1, kThreads, 0, st>>>(R, a.total, a.offsets, a.table + l.bits, a.table + l.ranks,
                                                          a.table + l.inside,
                                                          (const unsigned long long*)(a.table + l.best), a.rows,
                                                          a.inside, a.best, a.best_count);
}

void launch_wtags_entries(const WtagsArgs& a, uint32_t Q, uint32_t E, hipStream_t st) {
  if (Q == 0 || E == 0 || !(a.ids || a.counts || a.first)) return;
  const TableLayout l = table_layout(Q, a.total, a.nregions);
  wtags_emit_kernel<<<(l.slots - 1) / kThreads + 1, kThreads, 0, st>>>(
      table_of(a, l), a.nregions, a.total, E, a.offsets, a.table + l.bits, a.table + l.ranks, a.ids, a.counts, a.first);
}

size_t wvotes_jobs_bytes(uint32_t R) { return ((size_t)R + 1 + chunks_of(R + 1) + 1 + 3) * 4; }

const unsigned long long* wvotes_misses_word(const WvotesArgs& a) {
  const size_t at = (size_t)a.nregions + 1 + chunks_of(a.nregions + 1) + 1;
  return (const unsigned long long*)(a.jobs + ((at + 1) & ~(size_t)1));   // (8-byte aligned)
}

void launch_wvotes(const WvotesArgs& a, hipStream_t st) {
  const uint32_t R = a.nregions;
  uint32_t* jobbase = a.jobs;
  unsigned long long* misses = const_cast<unsigned long long*>(wvotes_misses_word(a));
  (void)hipMemsetAsync(misses, 0, 8, st);
  (void)hipMemsetAsync(a.votes, 0, (size_t)R * 2 * a.k * 4, st);
  scan::launch(Jobs{a.offsets, R, a.total}, jobbase, R + 1, a.jobs + R + 1, st);   // jobbase[R] = the jobs
  // at most one job per list that is not empty and one more per full segment of the entries
  const uint64_t most = (uint64_t)std::min<uint64_t>(R, a.total) + a.total / kVotesSegment;
  if (most != 0) wvotes_kernel<<<(uint32_t)((most + kWaves - 1) / kWaves), kThreads, 0, st>>>(a, jobbase, misses);
  wvotes_best_kernel<<<(uint32_t)((2ull * R + kThreads - 1) / kThreads), kThreads, 0, st>>>(R, a.k, a.votes, a.best);
}

}  // namespace dq
