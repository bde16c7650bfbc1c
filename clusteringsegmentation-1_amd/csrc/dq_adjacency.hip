// dq_adjacency.hip -- region adjacency graph of a region map on gfx950 (MI355X).
//
// Input: a width x height row-major map of uint32 region ids (any id map) and
// a connectivity (4 or 8).  A contact is a pair of pixel indexes p < q that are
// 4- / 8-neighbours with different ids; for one p the possible q are, in
// increasing order, direction 0 right (p + 1), 1 down-left (p + W - 1, 8 only),
// 2 down (p + W), 3 down-right (p + W + 1, 8 only).  With n <= 2^30 a contact is
// the word 4 * p + dir, and the order of these words is the order of (p, q).
// An edge is an unordered pair of ids {a, b}, a < b, with at least one contact;
// edges are numbered in the order of their first (lowest) contacts.  Every
// output is an integer that does not depend on scheduling.
//
// The lanes of a wave hold 64 consecutive pixels.  Per direction, a run of
// consecutive lanes with the same key (a << 32 | b) is one HEAD; the first
// contact of an edge is always the first lane of a head (were the contact one
// lane to the left of the same key, it would be lower).
//
// Passes (all on the caller's stream; no kernel waits for another workgroup,
// a probe loop ends because the table is at most half full):
//   1 count   the heads of every chunk of 1024 pixels, summed by dq_scan.h's top scan
//             (the host reads the total back and sizes the table from it,
//             never from 4 * n)
//   2 insert  each head claims or finds its key in an open-addressing table
//             (64-bit atomicCAS, linear probing) and adds its run length to the
//             border, its first contact by atomicMin, its colour steps to the
//             step sum; a workgroup first gathers its heads in 128 LDS slots
//             (slot free or already the key's, else straight to the table) and
//             flushes them once: a frame with few, long borders is the usual one
//   3 flag    a head whose contact word equals its entry's first contact is
//             the edge's first contact; their number per chunk of 1024 pixels
//   4 scan    one workgroup (dq_scan.h's top scan): exclusive prefix sum of the
//             chunk counts, total E
//   5 emit    pass 3 again (the key is looked up again: no per-pixel flag is
//             kept); edge id = chunk offset + rank in (p, dir) order; the
//             owning thread writes the edge's entries for ids < edge_cap and
//             adds 1 to the degree of both ends (through 128 LDS slots per
//             workgroup, like the insert pass)
//
// Extra device memory: 4 B per 1024 pixels + 4 B, and the table: 16 B (24 B
// with the step sums) per slot, slots = the power of two >= 2 * heads (>= 1024).
// No floating point anywhere.
#include <hip/hip_runtime.h>

#include "dq_adjacency.h"
#include "dq_scan.h"
#include "dq_stage.h"
#include "dq_table.h"

namespace dq {
namespace {

using scan::block_excl_scan;
using scan::chunks_of;
using table::kNoKey;   // (no a < b key equals it)
using table::mix;

constexpr uint32_t kNoContact = 0xFFFFFFFFu;   // (the last pixel has no down-right neighbour)
constexpr unsigned long long kNoSlot = ~0ull;   // table::table_find's "not there"
constexpr uint32_t kSlots = 128;               // LDS slots of the insert pass (and of the emit pass's degrees)
// -DDQ_ADJACENCY_LDS_SLOTS=0 builds the insert pass without them (every head
// straight to the table): the variant DESIGN.md 5a''' measures against.
#ifndef DQ_ADJACENCY_LDS_SLOTS
#define DQ_ADJACENCY_LDS_SLOTS 1
#endif

__device__ __forceinline__ unsigned long long edge_key(uint32_t a, uint32_t b) {
  if (a == b) return kNoKey;
  return a < b ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a;
}

// The keys of pixel i's four forward contacts (kNoKey: no neighbour there, the
// direction is not in the connectivity, or the ids are equal).
__device__ __forceinline__ void pixel_keys(const uint32_t* __restrict__ reg, uint32_t i, uint32_t n, uint32_t W,
                                           uint32_t H, int conn8, unsigned long long key[4]) {
  key[0] = key[1] = key[2] = key[3] = kNoKey;
  if (i >= n) return;
  const uint32_t y = i / W, x = i - y * W, a = reg[i];
  const bool right = x + 1 < W, down = y + 1 < H;
  if (right) key[0] = edge_key(a, reg[i + 1]);
  if (down) {
    key[2] = edge_key(a, reg[i + W]);
    if (conn8) {
      if (x > 0) key[1] = edge_key(a, reg[i + W - 1]);
      if (right) key[3] = edge_key(a, reg[i + W + 1]);
    }
  }
}

__device__ __forceinline__ uint32_t neighbour(uint32_t i, uint32_t dir, uint32_t W) {
  return dir == 0 ? i + 1 : i + W + dir - 2;
}

// Does a run of equal keys start at this lane?  (Every lane of the wave calls it.)
__device__ __forceinline__ bool run_start(unsigned long long key, uint32_t lane) {
  const unsigned long long prev = __shfl_up(key, 1);
  return lane == 0 || prev != key;
}

__device__ __forceinline__ uint32_t colour_step(uint32_t p, uint32_t q) {
  const int dr = (int)((p >> 16) & 0xFFu) - (int)((q >> 16) & 0xFFu);
  const int dg = (int)((p >> 8) & 0xFFu) - (int)((q >> 8) & 0xFFu);
  const int db = (int)(p & 0xFFu) - (int)(q & 0xFFu);
  return (uint32_t)(abs(dr) + abs(dg) + abs(db));
}

// ---- 1 count ---------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void adjacency_count_kernel(const uint32_t* __restrict__ reg, uint32_t n,
                                                                  uint32_t W, uint32_t H, int conn8,
                                                                  uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kThreads / 64];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t c = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    unsigned long long key[4];
    pixel_keys(reg, i, n, W, H, conn8, key);
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      const bool start = run_start(key[d], lane);
      c += start && key[d] != kNoKey ? 1u : 0u;
    }
  }
  uint32_t total;
  block_excl_scan<kThreads / 64>(c, wsum, total);
  // (one word per chunk and a scan: thousands of workgroups adding to ONE word took as long as the pass)
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ---- 2 insert --------------------------------------------------------------
struct Table {
  unsigned long long* key;    // kNoKey: free
  uint32_t* first;            // starts as kNoContact
  uint32_t* border;           // starts as 0
  unsigned long long* step;   // starts as 0; nullptr: not asked for
  unsigned long long slots;   // a power of two
};

// the home slot of a key: the hash's low bits
__device__ __forceinline__ unsigned long long home_slot(unsigned long long slots, unsigned long long key) {
  return mix(key) & (slots - 1);
}

__device__ __forceinline__ void table_add(const Table& t, unsigned long long key, uint32_t cnt, uint32_t contact,
                                          uint32_t step) {
  const unsigned long long s = table::table_claim(t.key, t.slots, home_slot(t.slots, key), key);
  atomicAdd(&t.border[s], cnt);
  atomicMin(&t.first[s], contact);
  if (t.step) atomicAdd(&t.step[s], (unsigned long long)step);
}

__global__ __launch_bounds__(kThreads) void adjacency_insert_kernel(const uint32_t* __restrict__ reg, uint32_t n,
                                                                   uint32_t W, uint32_t H, int conn8,
                                                                   const uint32_t* __restrict__ pixels, Table t) {
  __shared__ unsigned long long s_key[kSlots];
  __shared__ uint32_t s_first[kSlots], s_border[kSlots], s_step[kSlots];
  const uint32_t lane = threadIdx.x & 63u;
  const bool steps = t.step != nullptr;   // (uniform over the grid)
  if (threadIdx.x < kSlots) {
    s_key[threadIdx.x] = kNoKey;
    s_first[threadIdx.x] = kNoContact;
    s_border[threadIdx.x] = s_step[threadIdx.x] = 0;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    unsigned long long key[4];
    pixel_keys(reg, i, n, W, H, conn8, key);
    const uint32_t px = steps && i < n ? pixels[i] : 0u;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      const WaveRun run = wave_run(run_start(key[d], lane));
      uint32_t sv = 0;
      if (steps) {   // (uniform) the run's sum: <= 64 * 765
        if (key[d] != kNoKey) sv = colour_step(px, pixels[neighbour(i, d, W)]);
        sv = run_sum(sv, run);
      }
      if (run.tail && key[d] != kNoKey) {
        const uint32_t cnt = run.length(lane), contact = 4u * (i + 1 - cnt) + d;
        const uint32_t slot = (uint32_t)(mix(key[d]) >> 57);   // (the table takes the low bits)
        static_assert(kSlots == 128, "the top 7 bits of the hash");
        // (without the slots every head goes to the table; <= 4096 contacts a workgroup: the u32 sums hold)
        if (DQ_ADJACENCY_LDS_SLOTS && slot_claim(s_key, slot, kNoKey, key[d])) {
          atomicAdd(&s_border[slot], cnt);
          atomicMin(&s_first[slot], contact);
          if (steps) atomicAdd(&s_step[slot], sv);
        } else {
          table_add(t, key[d], cnt, contact, sv);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kSlots && s_key[threadIdx.x] != kNoKey)
    table_add(t, s_key[threadIdx.x], s_border[threadIdx.x], s_first[threadIdx.x], s_step[threadIdx.x]);
}

// ---- 3 flag, 5 emit --------------------------------------------------------
struct EdgeOut {
  uint32_t cap;
  uint32_t* edges;
  uint32_t* border;
  uint32_t* contact;
  unsigned long long* step;
  uint32_t* degree;
};

// One more edge at id: into the workgroup's LDS slot id % kSlots when that slot
// is free or already the id's, else straight to global memory (an id that
// touches thousands of others would otherwise take one global add per edge on
// one word).  kNoId: ids are < nregions <= 2^32 - 1 where a degree is asked for.
__device__ __forceinline__ void degree_add(uint32_t* s_id, uint32_t* s_cnt, uint32_t* degree, uint32_t id) {
  const uint32_t slot = id % kSlots;
  if (slot_claim(s_id, slot, kNoId, id)) atomicAdd(&s_cnt[slot], 1u);
  else atomicAdd(&degree[id], 1u);
}

// EMIT = false: counts[chunk] = the chunk's first contacts.  EMIT = true:
// counts[] holds the chunks' offsets and the edges are written.
template <bool EMIT>
__global__ __launch_bounds__(kThreads) void adjacency_first_kernel(
    const uint32_t* __restrict__ reg, uint32_t n, uint32_t W, uint32_t H, int conn8,
    const unsigned long long* __restrict__ t_key, const uint32_t* __restrict__ t_first,
    const uint32_t* __restrict__ t_border, const unsigned long long* __restrict__ t_step, unsigned long long slots,
    uint32_t* counts, EdgeOut o) {
  __shared__ uint32_t wsum[kThreads / 64];
  __shared__ uint32_t s_id[EMIT ? kSlots : 1], s_cnt[EMIT ? kSlots : 1];
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t carry = EMIT ? counts[blockIdx.x] : 0u, c = 0;
  if (EMIT && o.degree) {   // (uniform over the grid)
    if (threadIdx.x < kSlots) {
      s_id[threadIdx.x] = kNoId;
      s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
  }
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    unsigned long long key[4], slot[4];
    pixel_keys(reg, i, n, W, H, conn8, key);
    uint32_t firsts = 0;   // bit d: contact 4 * i + d is its edge's first
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      const bool start = run_start(key[d], lane);
      slot[d] = kNoSlot;
      if (start && key[d] != kNoKey) {
        // (every head's key is in the table; a free slot ends the probe all the same)
        const unsigned long long s = table::table_find(t_key, slots, home_slot(slots, key[d]), key[d]);
        if (s != kNoSlot && t_first[s] == 4u * i + d) {
          firsts |= 1u << d;
          slot[d] = s;
        }
      }
    }
    const uint32_t mine = (uint32_t)__popc(firsts);
    if (!EMIT) {
      c += mine;
      continue;
    }
    uint32_t total;
    uint32_t id = carry + block_excl_scan<kThreads / 64>(mine, wsum, total);
    carry += total;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      if (!((firsts >> d) & 1u)) continue;
      const uint32_t a = (uint32_t)(key[d] >> 32), b = (uint32_t)key[d];
      if (id < o.cap) {
        if (o.edges) {
          o.edges[2 * (size_t)id + 0] = a;
          o.edges[2 * (size_t)id + 1] = b;
        }
        if (o.border) o.border[id] = t_border[slot[d]];
        if (o.contact) {
          o.contact[2 * (size_t)id + 0] = i;
          o.contact[2 * (size_t)id + 1] = neighbour(i, d, W);
        }
        if (o.step) o.step[id] = t_step[slot[d]];
      }
      if (o.degree) {
        degree_add(s_id, s_cnt, o.degree, a);
        degree_add(s_id, s_cnt, o.degree, b);
      }
      ++id;
    }
  }
  if (!EMIT) {
    uint32_t total;
    block_excl_scan<kThreads / 64>(c, wsum, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
  } else if (o.degree) {
    __syncthreads();
    if (threadIdx.x < kSlots && s_id[threadIdx.x] != kNoId) atomicAdd(&o.degree[s_id[threadIdx.x]], s_cnt[threadIdx.x]);
  }
}

}  // namespace

size_t adjacency_count_words(uint32_t width, uint32_t height) { return (size_t)chunks_of(width * height) + 1; }

uint64_t adjacency_table_slots(uint32_t heads) {
  uint64_t slots = table::kMinTableSlots;
  while (slots < 2 * (uint64_t)heads) slots <<= 1;
  return slots;
}

size_t adjacency_scratch_bytes(uint32_t heads, bool with_step) {
  return (size_t)adjacency_table_slots(heads) * (with_step ? 24 : 16);
}

const uint32_t* adjacency_edges_word(const AdjacencyArgs& a) { return a.counts + chunks_of(a.width * a.height); }
// (the same word: the heads are read before the second half overwrites the counts)
const uint32_t* adjacency_heads_word(const AdjacencyArgs& a) { return adjacency_edges_word(a); }

void launch_adjacency_count(const AdjacencyArgs& a, hipStream_t st) {
  const uint32_t W = a.width, H = a.height, n = W * H, nchunks = chunks_of(n);
  adjacency_count_kernel<<<nchunks, kThreads, 0, st>>>(a.regions, n, W, H, a.connectivity == 8 ? 1 : 0, a.counts);
  // (heads < 4 n <= 2^32, DQ_HIP_ADJACENCY_MAX_PIXELS: the saturating sums are the sums)
  scan::scan_top_kernel<<<1, 1024, 0, st>>>(a.counts, nchunks);
}

void launch_adjacency_build(const AdjacencyArgs& a, uint32_t heads, hipStream_t st) {
  const uint32_t W = a.width, H = a.height, n = W * H, nchunks = chunks_of(n);
  const int conn8 = a.connectivity == 8 ? 1 : 0;
  const uint64_t slots = adjacency_table_slots(heads);
  // keys | first contacts (all ones), then borders | step sums (zero)
  Table t;
  t.key = (unsigned long long*)a.table;
  t.first = (uint32_t*)(t.key + slots);
  t.border = t.first + slots;
  t.step = a.step ? (unsigned long long*)(t.border + slots) : nullptr;   // (8-B aligned: 16 * slots bytes in)
  t.slots = slots;
  (void)hipMemsetAsync(t.key, 0xFF, (size_t)slots * 12, st);
  (void)hipMemsetAsync(t.border, 0, (size_t)slots * (a.step ? 12 : 4), st);
  const bool out_on = a.edge_cap != 0;
  EdgeOut o{a.edge_cap,
            out_on ? a.edges : nullptr,
            out_on ? a.border : nullptr,
            out_on ? a.contact : nullptr,
            out_on ? a.step : nullptr,
            a.degree};
  adjacency_insert_kernel<<<nchunks, kThreads, 0, st>>>(a.regions, n, W, H, conn8, a.pixels, t);
  adjacency_first_kernel<false><<<nchunks, kThreads, 0, st>>>(a.regions, n, W, H, conn8, t.key, t.first, t.border,
                                                             t.step, t.slots, a.counts, o);
  scan::scan_top_kernel<<<1, 1024, 0, st>>>(a.counts, nchunks);   // (E <= heads)
  adjacency_first_kernel<true><<<nchunks, kThreads, 0, st>>>(a.regions, n, W, H, conn8, t.key, t.first, t.border,
                                                            t.step, t.slots, a.counts, o);
}

}  // namespace dq
