// dq_pixels.hip -- the pixel lists of a region map on gfx950 (MI355X).
//
// Input: a width x height row-major map of uint32 region ids, each < R.  The
// output is the stable counting sort of the pixels by id: offsets[r] = the
// pixels with an id < r, and the j-th pixel of region r in raster order
// (increasing p = y * width + x) is entry offsets[r] + j of every list (the
// pixel index p, the Coord word x | y << 16, the frame's word at p).  Every
// output is an integer that does not depend on scheduling.
//
// The position of a pixel is split as (pixels of lower ids) + (pixels of its id
// in rows above) + (pixels of its id to the left in its row).  The first two
// are one table entry per (id, row the id spans), laid out id-major:
// entry rowbase[r] + y - y0[r].  T, the number of entries, is the sum over the
// ids present of (last row - first row + 1); a connected region has a pixel in
// every row it spans, so T <= n for the maps of the connected-regions and merge
// calls, and the call refuses a map with T > n before it sizes the table.
//
// Passes (all on the caller's stream; no kernel waits for another workgroup,
// values written by atomics are otherwise read only in later launches):
//   1 rows    y0[r], y1[r] by atomicMin / atomicMax, once per run of equal ids
//             in a wave whose pixel above (below) has another id, gathered
//             per workgroup in 128 LDS slots first
//   2 scan    heights y1 - y0 + 1 (0: id absent) -> rowbase[] and T, three
//             kernels (dq_scan.h: sums per 1024, one workgroup over the sums, apply);
//             the sums saturate at 2^32 - 1, so T > n is seen however large T is
//             (the host reads T back and allocates the table)
//   3 count   table[rowbase[r] + y - y0[r]] += run length, one add per run
//   4 scan    the table in place: entry (r, y) = the output position of the
//             first pixel of r in row y; offsets[r] = table[rowbase[r]]
//   5 walk    one wave per row, 64 pixels at a time in x order: the lanes with
//             equal ids form a group (not only neighbours: A B A is one group
//             of A; found by ballots, one round per id that an LDS slot per id
//             shows to be, or possibly be, shared), the group's lowest lane
//             takes old = atomicAdd(&table[..], group size) and every lane
//             writes at old + its rank.  A row's entries are touched by that
//             row's wave alone, one chunk after the other (the returned value
//             is used before the next chunk's add), so positions are
//             deterministic.  The returning atomic, not a load and a store: it
//             reads and writes at L2.
// A 65535 x 1 map is one wave's work in pass 5: correct and slow.
//
// Extra device memory: 8 B per region + 4 B per 1024 regions + 4 B, and after
// the read-back 4 B per table entry (T <= n) + 4 B per 1024 entries + 4 B.
// Ids >= R (not allowed) are skipped by every pass: their pixels are in no
// list, nothing is written out of bounds.  No floating point anywhere.
#include <hip/hip_runtime.h>

#include "dq_pixels.h"
#include "dq_scan.h"
#include "dq_stage.h"

namespace dq {
namespace {

constexpr uint32_t kRowsPerBlock = kThreads / 64;   // the walk: one wave per row
constexpr uint32_t kRowSlots = 128;                 // the rows pass: LDS slots per workgroup

constexpr uint32_t kNoRow = 0xFFFFFFFFu;   // y0 of an id without a pixel
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // T <= n <= 2^31 - 1: never a table entry

using scan::chunks_of;

// the scan over the regions: element i is y1[i] - y0[i] + 1 (0 when y0[i] is kNoRow) with y1 = v
struct Heights {
  const uint32_t *y0, *v;
  __device__ uint32_t operator()(uint32_t i) const {
    const uint32_t a = y0[i];
    return a == kNoRow ? 0u : v[i] - a + 1u;
  }
};

// ---- 1 rows ------------------------------------------------------------------
// A pixel whose upper neighbour has its id is not in the id's first row; of the
// others, one lane per run of equal ids in the wave (and in the row) is enough.
// A workgroup first gathers its rows in 128 LDS slots (slot id % 128 free or
// already the id's, else straight to global memory) and flushes them once: a
// few hundred large regions otherwise queue on a few hundred words.
__global__ __launch_bounds__(kThreads) void pixels_rows_kernel(const uint32_t* __restrict__ reg, uint32_t n, uint32_t W,
                                                              uint32_t H, uint32_t R, uint32_t* y0, uint32_t* y1) {
  __shared__ uint32_t s_id[kRowSlots], s_lo[kRowSlots], s_hi[kRowSlots];
  const uint32_t lane = threadIdx.x & 63u;
  if (threadIdx.x < kRowSlots) {
    s_id[threadIdx.x] = kNoId;
    s_lo[threadIdx.x] = kNoRow;   // (flushed as they are: a min with all ones, a max with 0 change nothing)
    s_hi[threadIdx.x] = 0;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    const bool in = i < n;
    const uint32_t id = in ? reg[i] : kNoId;
    const uint32_t y = in ? i / W : 0u, x = in ? i - y * W : 0u;
    const bool valid = id < R;
    const uint32_t prev = __shfl_up(id, 1);
    const bool head = lane == 0 || prev != id || x == 0;
    const bool top = valid && (y == 0 || reg[i - W] != id);
    const bool bot = valid && (y + 1 == H || reg[i + W] != id);
    const int ptop = __shfl_up((int)top, 1), pbot = __shfl_up((int)bot, 1);
    const bool lo = top && (head || !ptop), hi = bot && (head || !pbot);
    if (lo || hi) {
      const uint32_t slot = id % kRowSlots;
      if (slot_claim(s_id, slot, kNoId, id)) {
        if (lo) atomicMin(&s_lo[slot], y);
        if (hi) atomicMax(&s_hi[slot], y);
      } else {
        if (lo) atomicMin(&y0[id], y);
        if (hi) atomicMax(&y1[id], y);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kRowSlots && s_id[threadIdx.x] != kNoId) {
    atomicMin(&y0[s_id[threadIdx.x]], s_lo[threadIdx.x]);
    atomicMax(&y1[s_id[threadIdx.x]], s_hi[threadIdx.x]);
  }
}

// ---- 3 count -----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pixels_count_kernel(const uint32_t* __restrict__ reg, uint32_t n, uint32_t W,
                                                               uint32_t R, uint32_t T,
                                                               const uint32_t* __restrict__ y0,
                                                               const uint32_t* __restrict__ rowbase, uint32_t* table) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    const bool in = i < n;
    const uint32_t id = in ? reg[i] : kNoId;
    const uint32_t y = in ? i / W : 0u, x = in ? i - y * W : 0u;
    const uint32_t prev = __shfl_up(id, 1);
    const WaveRun run = wave_run(prev != id || x == 0);
    if (run.tail && id < R) {
      const uint32_t slot = rowbase[id] + (y - y0[id]);
      if (slot < T) atomicAdd(&table[slot], run.length(lane));
    }
  }
}

// ---- 4 offsets ---------------------------------------------------------------
// offsets[r] = table[rowbase[r]].  An id without a list has the rowbase of the
// next id with one (or T): its offset is that id's (or `total`, the pixels with
// a lower id, which is also offsets[R]).
__global__ __launch_bounds__(kThreads) void list_offsets_kernel(uint32_t R, uint32_t T, uint32_t total,
                                                               const uint32_t* __restrict__ rowbase,
                                                               const uint32_t* __restrict__ table,
                                                               uint32_t* __restrict__ offsets) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r > R) return;
  uint32_t o = total;
  if (r < R) {
    const uint32_t b = rowbase[r];
    if (b < T) o = table[b];
  }
  offsets[r] = o;
}

// ---- 5 walk ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pixels_walk_kernel(const uint32_t* __restrict__ reg, uint32_t W, uint32_t H,
                                                              uint32_t R, uint32_t T, uint32_t n,
                                                              const uint32_t* __restrict__ y0,
                                                              const uint32_t* __restrict__ rowbase, uint32_t* table,
                                                              const uint32_t* __restrict__ pixels,
                                                              uint32_t* __restrict__ index, uint32_t* __restrict__ coords,
                                                              uint32_t* __restrict__ colors) {
  __shared__ uint32_t s_slots[kRowsPerBlock][kWalkSlots];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t y = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (y >= H) return;   // (whole waves; the kernel has no barrier)
  uint32_t* slots = s_slots[threadIdx.x >> 6];   // this wave's alone (a wave's LDS accesses run in order)
  for (uint32_t j = lane; j < kWalkSlots; j += 64) slots[j] = kNoId;
  __builtin_amdgcn_wave_barrier();
  const uint32_t base = y * W;
  // the id at x and its table entry (kNoSlot: no pixel there, or an id >= R)
  auto fetch = [&](uint32_t x, uint32_t& id, uint32_t& slot) {
    id = x < W ? reg[base + x] : kNoId;
    slot = kNoSlot;
    if (id < R) slot = rowbase[id] + (y - y0[id]);
  };
  uint32_t id, slot;
  fetch(lane, id, slot);
#pragma unroll 1
  for (uint32_t x0 = 0; x0 < W; x0 += 64) {
    uint32_t nid = kNoId, nslot = kNoSlot;   // the next chunk's loads go out before this chunk's add
    if (x0 + 64 < W) fetch(x0 + 64 + lane, nid, nslot);
    const uint32_t x = x0 + lane, p = base + x;
    const bool valid = slot < T;
    const uint32_t px = (valid && colors) ? pixels[p] : 0u;
    // Groups of equal ids (dq_stage.h): rank, size and leader come from the round's ballot; a lane
    // in no round is alone with its id.
    uint32_t rank = 0, size = 1, leader = lane;
    wave_id_groups(slots, id, valid, [&](bool mine, unsigned long long group, int l) {
      if (mine) {
        rank = (uint32_t)__popcll(group & ((1ull << lane) - 1ull));
        size = (uint32_t)__popcll(group);
        leader = (uint32_t)l;
      }
    });
    uint32_t old = 0;
    if (valid && leader == lane) old = atomicAdd(&table[slot], size);
    old = __shfl(old, (int)leader);
    const uint32_t pos = old + rank;
    if (valid && pos < n) {
      if (index) index[pos] = p;
      if (coords) coords[pos] = x | (y << 16);
      if (colors) colors[pos] = px;
    }
    id = nid;
    slot = nslot;
  }
}

// ---- the inverse: values of a Coord list into a frame --------------------------
__global__ __launch_bounds__(kThreads) void scatter_coords_kernel(const uint32_t* __restrict__ values,
                                                                 const uint32_t* __restrict__ coords, uint32_t n,
                                                                 uint32_t W, uint32_t* __restrict__ frame) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = coords[i];
  frame[(size_t)(c >> 16) * W + (c & 0xFFFFu)] = values[i];
}

}  // namespace

// y0 | y1, then rowbase | the sums of the scan over the regions
size_t pixels_rows_bytes(uint32_t nregions) { return ((size_t)nregions * 2 + chunks_of(nregions) + 1) * 4; }

// the table | the sums of the scan over it
size_t pixels_table_bytes(uint32_t total) {
  const uint32_t t = total ? total : 1u;
  return ((size_t)t + chunks_of(t) + 1) * 4;
}

const uint32_t* pixels_total_word(const PixelsArgs& a) {
  return a.rows + (size_t)a.nregions * 2 + chunks_of(a.nregions);
}

void launch_pixels_rows(const PixelsArgs& a, hipStream_t st) {
  const uint32_t W = a.width, H = a.height, n = W * H, R = a.nregions;
  uint32_t *y0 = a.rows, *y1 = y0 + R, *sums = y1 + R;
  (void)hipMemsetAsync(y0, 0xFF, (size_t)R * 4, st);
  (void)hipMemsetAsync(y1, 0, (size_t)R * 4, st);
  pixels_rows_kernel<<<chunks_of(n), kThreads, 0, st>>>(a.regions, n, W, H, R, y0, y1);
  scan::launch(Heights{y0, y1}, y1, R, sums, st);   // y1 is rowbase from here on
}

void launch_pixels_lists(const PixelsArgs& a, uint32_t T, hipStream_t st) {
  const uint32_t W = a.width, H = a.height, n = W * H, R = a.nregions;
  const uint32_t *y0 = a.rows, *rowbase = y0 + R;
  uint32_t* table = a.table;
  if (T != 0) {
    (void)hipMemsetAsync(table, 0, (size_t)T * 4, st);
    pixels_count_kernel<<<chunks_of(n), kThreads, 0, st>>>(a.regions, n, W, R, T, y0, rowbase, table);
    scan::launch(scan::Words{table}, table, T, table + T, st);
  }
  launch_list_offsets(R, T, n, rowbase, table, a.offsets, st);
  if (T != 0 && (a.index || a.coords || a.colors))
    pixels_walk_kernel<<<(H + kRowsPerBlock - 1) / kRowsPerBlock, kThreads, 0, st>>>(
        a.regions, W, H, R, T, n, y0, rowbase, table, a.pixels, a.index, a.coords, a.colors);
}

void launch_list_offsets(uint32_t R, uint32_t T, uint32_t total, const uint32_t* rowbase, const uint32_t* table,
                         uint32_t* offsets, hipStream_t st) {
  list_offsets_kernel<<<R / kThreads + 1, kThreads, 0, st>>>(R, T, total, rowbase, table, offsets);
}

void launch_scatter_coords(const uint32_t* values, const uint32_t* coords, uint32_t n, uint32_t width, uint32_t* frame,
                           hipStream_t st) {
  if (n == 0) return;
  scatter_coords_kernel<<<(n - 1) / kThreads + 1, kThreads, 0, st>>>(values, coords, n, width, frame);
}

}  // namespace dq
