// dq_distance.hip -- the L1 distance transform, the centres and the cores of a
// region map on gfx950 (MI355X).
//
// Input: a width x height map of ids; an id < R is a region (its pixels need
// not be connected), an id >= R is background.  include/dq_hip.h, "region
// distance", has the full definition; in short: D(p) is the smallest
// |dx| + |dy| from p to a pixel of another id or to a position just outside the
// frame (0 on background); dmax[r] the highest D of r; thresh[r] = dmax[r]
// (rule 0) or the lowest d whose 8-bit scale value equals dmax's (rule 1);
// S[r] the pixels of r with D >= thresh[r]; the centre of r the centroid of S
// when it lies in S, else the pixel of S nearest to it (for |S| <= 2: the
// leftmost pixel of S's last row); the core of r the component of r's pixels
// that holds the centre.  Every output is an integer that does not depend on
// scheduling.
//
// D needs no segmented scan and no pass per region.  A HEAD is a pixel whose
// predecessor along a line has another id (or is outside the frame), a TAIL one
// whose successor has.  Along a column
//   g(x, y) = min(y - lastHeadAbove + 1, firstTailBelow - y + 1)
// is the distance to the nearest other id in the column, and along a row
//   D(x, y) = min(x - lh + 1, rt - x + 1,
//                 x + min_{x' <= x} (g(x', y) - x'), -x + min_{x' >= x} (g(x', y) + x')).
// The two min-plus scans run straight across other regions' pixels: g >= 1
// everywhere, so a term from beyond the row run [lh, rt] is at least the
// distance to the run's end plus 2, and the boundary term beats it.
//
// Kernels (no kernel waits for another workgroup; what atomics write in one
// launch only later launches read):
//   init     per region: dmax, bbox, count, sums, keys cleared
//   heads    per (band of kDistanceBand rows, column), lanes across x: the head
//            bits of the band's pixels in one word, and the band's last head
//            and first tail
//   carry    per column: the last head above and the first tail below every band
//   columns  per (band, column): g as u16 from the head bits and the carries
//            (the map is not read again)
//   rows     one wave per row, 64 pixels per step: left to right the heads by
//            ballot and the prefix min by shuffles with the carry in a register,
//            the half result parked in D; right to left the tails and the
//            suffix min, D as u16
//   stats    per run of equal ids along a wave: dmax and bbox  } through the workgroup's
//   sums     per pixel of S: count, the sums of x and y, the   } LDS slot cache (dq_stage.h): one
//            last-row key                                      } global atomic per region and workgroup
//   thresh   per region (between stats and sums): the threshold, FP64 for rule 1
//   decide   per region: the centre where no search is needed, else the
//            centroid c goes to want[r]
//   nearest  per pixel of S of a region with want[r]: one 64-bit atomicMin of
//            (dx^2 + dy^2) << 31 | raster index
//   settle   per region with want[r]: the centre from the key
//   cores    per pixel: the component of the pixel against the component of its
//            region's centre (components: dq_regions.hip on the map as labels)
// FP64 only in thresh (sqrt and /, correctly rounded; -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "dq_distance.h"
#include "dq_stage.h"

namespace dq {
namespace {

constexpr uint32_t kBand = kDistanceBand;
static_assert(kBand == 32, "one word of head bits per band");
constexpr uint32_t kSlots = 64;
constexpr int kFar = 0x3FFFFFFF;   // above every g +- x, below overflow when x is added
constexpr uint32_t kNoRow = 0xFFFFu;   // no tail in a band (rows are <= 65534)
// the search key: dx, dy <= 65534, so dx^2 + dy^2 < 2^33, and the raster index is < 2^31
static_assert(2ull * 65534ull * 65534ull < (1ull << 33), "the squared distance and the index share 64 bits");

struct Scratch {
  unsigned long long* sumx;   // R
  unsigned long long* sumy;   // R
  unsigned long long* near;   // R: the search key
  uint32_t* last;             // R: y << 16 | (65535 - x), max: the last row of S, its leftmost pixel
  uint32_t* want;             // R: the centroid of a region whose centre is searched, else kNoId
  uint32_t* bits;             // bands * W: the head bits
  uint32_t* carry;            // bands * W: last head + 1 | first tail << 16, then the carries into the band
  uint16_t* g;                // W * H: the column step's distances
};

uint32_t bands_of(uint32_t height) { return (height + kBand - 1) / kBand; }

Scratch carve(void* scratch, uint32_t width, uint32_t height, uint32_t nregions) {
  const size_t R = nregions, cells = (size_t)bands_of(height) * width;
  Scratch s;
  s.sumx = (unsigned long long*)scratch;
  s.sumy = s.sumx + R;
  s.near = s.sumy + R;
  s.last = (uint32_t*)(s.near + R);
  s.want = s.last + R;
  s.bits = s.want + R;
  s.carry = s.bits + cells;
  s.g = (uint16_t*)(s.carry + cells);
  return s;
}

__global__ __launch_bounds__(kThreads) void distance_init_kernel(DistanceArgs a, Scratch s) {
  const uint64_t r = global_thread();
  if (r >= a.nregions) return;
  a.dmax[r] = 0;
  a.bbox[4 * r + 0] = a.bbox[4 * r + 1] = 0xFFFFFFFFu;   // x0, y0: atomicMin
  a.bbox[4 * r + 2] = a.bbox[4 * r + 3] = 0;             // x1, y1: atomicMax
  a.count[r] = 0;
  s.sumx[r] = s.sumy[r] = 0;
  s.last[r] = 0;
}

// ---- columns ---------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void distance_heads_kernel(const uint32_t* __restrict__ regions, uint32_t W,
                                                                 uint32_t H, Scratch s) {
  const uint32_t x = blockIdx.x * kThreads + threadIdx.x, band = blockIdx.y;
  if (x >= W) return;
  const uint32_t y0 = band * kBand, rows = min(kBand, H - y0);
  uint32_t prev = y0 > 0 ? regions[(size_t)(y0 - 1) * W + x] : 0u;
  uint32_t m = y0 == 0 ? 1u : 0u;   // (row 0 is a head)
  for (uint32_t j = 0; j < rows; ++j) {
    const uint32_t id = regions[(size_t)(y0 + j) * W + x];
    if (id != prev) m |= 1u << j;
    prev = id;
  }
  // the head just below the band ends the band's last run (row H is one)
  const uint32_t below = y0 + rows == H || regions[(size_t)(y0 + rows) * W + x] != prev ? 1u : 0u;
  const unsigned long long tails = ((unsigned long long)m | (unsigned long long)below << rows) >> 1;   // bit j: a tail at y0 + j
  const uint32_t last_head = m ? y0 + (31u - (uint32_t)__clz((int)m)) + 1u : 0u;
  const uint32_t first_tail = tails ? y0 + (uint32_t)__ffsll((long long)tails) - 1u : kNoRow;
  const size_t cell = (size_t)band * W + x;
  s.bits[cell] = m;
  s.carry[cell] = last_head | first_tail << 16;
}

__global__ __launch_bounds__(kThreads) void distance_carry_kernel(uint32_t W, uint32_t bands, Scratch s) {
  const uint32_t x = blockIdx.x * kThreads + threadIdx.x;
  if (x >= W) return;
  uint32_t run = 0;   // the last head + 1 above the band (band 0 holds row 0's)
  for (uint32_t b = 0; b < bands; ++b) {
    const size_t cell = (size_t)b * W + x;
    const uint32_t w = s.carry[cell];
    s.carry[cell] = run | (w & 0xFFFF0000u);
    if (w & 0xFFFFu) run = w & 0xFFFFu;
  }
  run = kNoRow;       // the first tail below the band (the last band holds row H - 1's)
  for (uint32_t b = bands; b-- > 0;) {
    const size_t cell = (size_t)b * W + x;
    const uint32_t w = s.carry[cell];
    s.carry[cell] = (w & 0xFFFFu) | run << 16;
    if ((w >> 16) != kNoRow) run = w >> 16;
  }
}

__global__ __launch_bounds__(kThreads) void distance_columns_kernel(uint32_t W, uint32_t H, uint32_t bands, Scratch s,
                                                                   uint16_t* __restrict__ g) {
  const uint32_t x = blockIdx.x * kThreads + threadIdx.x, band = blockIdx.y;
  if (x >= W) return;
  const uint32_t y0 = band * kBand, rows = min(kBand, H - y0);
  const size_t cell = (size_t)band * W + x;
  const uint32_t m = s.bits[cell], c = s.carry[cell];
  const uint32_t below = band + 1 < bands ? s.bits[cell + W] & 1u : 1u;   // (a band that is not the last has kBand rows)
  const unsigned long long heads = (unsigned long long)m | (unsigned long long)below << rows;
  for (uint32_t j = 0; j < rows; ++j) {
    const uint32_t y = y0 + j;
    const uint32_t upto = m & (0xFFFFFFFFu >> (31u - j));
    const uint32_t last_head = upto ? y0 + (31u - (uint32_t)__clz((int)upto)) : (c & 0xFFFFu) - 1u;
    const unsigned long long after = heads >> (j + 1);   // bit i: a head at y + 1 + i, a tail at y + i
    const uint32_t first_tail = after ? y + (uint32_t)__ffsll((long long)after) - 1u : c >> 16;
    g[(size_t)y * W + x] = (uint16_t)min(y - last_head + 1u, first_tail - y + 1u);
  }
}

// ---- rows ------------------------------------------------------------------
// One wave per row.  D holds the left-to-right half between the two sweeps: a
// lane reads back only what it wrote itself.
__global__ __launch_bounds__(kThreads) void distance_rows_kernel(const uint32_t* __restrict__ regions, uint32_t W,
                                                                uint32_t H, uint32_t R,
                                                                const uint16_t* __restrict__ g, uint16_t* D) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t y = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (y >= H) return;   // (the whole wave)
  const uint32_t* id_row = regions + (size_t)y * W;
  const uint16_t* g_row = g + (size_t)y * W;
  uint16_t* d_row = D + (size_t)y * W;
  const uint32_t chunks = (W + 63u) / 64u;

  int carry_min = kFar;
  uint32_t carry_head = 0, edge_id = 0;
  for (uint32_t c = 0; c < chunks; ++c) {
    const uint32_t x = c * 64u + lane;
    const bool valid = x < W;
    const uint32_t id = valid ? id_row[x] : 0u;
    uint32_t left = __shfl_up(id, 1);
    if (lane == 0) left = edge_id;
    const unsigned long long heads = __ballot(valid && (x == 0 || id != left));
    const unsigned long long upto = heads & (~0ull >> (63u - lane));
    const uint32_t lh = upto ? c * 64u + 63u - (uint32_t)__clzll((long long)upto) : carry_head;
    int v = valid ? (int)g_row[x] - (int)x : kFar;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(v, d);
      if (lane >= d) v = min(v, t);
    }
    v = min(v, carry_min);
    if (valid) d_row[x] = (uint16_t)min((int)(x - lh + 1u), (int)x + v);
    carry_min = __shfl(v, 63);
    if (heads) carry_head = c * 64u + 63u - (uint32_t)__clzll((long long)heads);
    edge_id = __shfl(id, 63);
  }

  carry_min = kFar;
  uint32_t carry_tail = W - 1;
  for (uint32_t c = chunks; c-- > 0;) {
    const uint32_t x = c * 64u + lane;
    const bool valid = x < W;
    const uint32_t id = valid ? id_row[x] : 0u;
    uint32_t right = __shfl_down(id, 1);
    if (lane == 63) right = edge_id;
    const unsigned long long tails = __ballot(valid && (x == W - 1 || id != right));
    const unsigned long long from = tails & (~0ull << lane);
    const uint32_t rt = from ? c * 64u + (uint32_t)__ffsll((long long)from) - 1u : carry_tail;
    int v = valid ? (int)g_row[x] + (int)x : kFar;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const int t = __shfl_down(v, d);
      if (lane + d < 64) v = min(v, t);
    }
    v = min(v, carry_min);
    if (valid) {
      const int d = min(min((int)d_row[x], (int)(rt - x + 1u)), v - (int)x);
      d_row[x] = id < R ? (uint16_t)d : (uint16_t)0;
    }
    carry_min = __shfl(v, 0);
    if (tails) carry_tail = c * 64u + (uint32_t)__ffsll((long long)tails) - 1u;
    edge_id = __shfl(id, 0);
  }
}

// ---- per-region values -----------------------------------------------------
// The lanes of a wave hold consecutive pixels: each run of lanes with one region
// id adds once, from its last lane, into the workgroup's slot of the id.
__global__ __launch_bounds__(kThreads) void distance_stats_kernel(const uint32_t* __restrict__ regions, uint32_t n,
                                                                 uint32_t W, uint32_t R,
                                                                 const uint16_t* __restrict__ D, uint32_t* dmax,
                                                                 uint32_t* bbox) {
  __shared__ uint32_t s_key[kSlots], s_dmax[kSlots], s_xlo[kSlots], s_ylo[kSlots], s_xhi[kSlots], s_yhi[kSlots];
  if (threadIdx.x < kSlots) {
    s_key[threadIdx.x] = kNoId;
    s_dmax[threadIdx.x] = s_xhi[threadIdx.x] = s_yhi[threadIdx.x] = 0;
    s_xlo[threadIdx.x] = s_ylo[threadIdx.x] = 0xFFFFFFFFu;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {   // (every lane stays for the shuffles)
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;   // (n < 2^31: no wrap)
    const uint32_t id = i < n ? regions[i] : kNoId;
    const bool on = i < n && id < R;
    const uint32_t key = on ? id : kNoId;
    const WaveRun run = wave_run(__shfl_up(key, 1) != key);
    const uint32_t d = run_max(on ? (uint32_t)D[i] : 0u, run);
    if (run.tail && on) {   // (no lane leaves the loop's shuffles)
      const uint32_t i0 = i + 1 - run.length(lane);
      const uint32_t ya = i0 / W, xa = i0 - ya * W, yb = i / W, xb = i - yb * W;
      // a run that wraps to a later row holds the last pixel of one row and the first of another
      const uint32_t xlo = yb > ya ? 0u : xa, xhi = yb > ya ? W - 1 : xb;
      const uint32_t slot = id % kSlots;
      if (slot_claim(s_key, slot, kNoId, id)) {
        atomicMax(&s_dmax[slot], d);
        atomicMin(&s_xlo[slot], xlo);
        atomicMin(&s_ylo[slot], ya);
        atomicMax(&s_xhi[slot], xhi);
        atomicMax(&s_yhi[slot], yb);
      } else {
        atomicMax(&dmax[id], d);
        atomicMin(&bbox[4 * (size_t)id + 0], xlo);
        atomicMin(&bbox[4 * (size_t)id + 1], ya);
        atomicMax(&bbox[4 * (size_t)id + 2], xhi);
        atomicMax(&bbox[4 * (size_t)id + 3], yb);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kSlots && s_key[threadIdx.x] != kNoId) {
    const size_t id = s_key[threadIdx.x];
    atomicMax(&dmax[id], s_dmax[threadIdx.x]);
    atomicMin(&bbox[4 * id + 0], s_xlo[threadIdx.x]);
    atomicMin(&bbox[4 * id + 1], s_ylo[threadIdx.x]);
    atomicMax(&bbox[4 * id + 2], s_xhi[threadIdx.x]);
    atomicMax(&bbox[4 * id + 3], s_yhi[threadIdx.x]);
  }
}

// The reference's 8-bit scale of a distance: the normalised square root, FP64 in this order.
__device__ __forceinline__ uint32_t scale_byte(uint32_t d, double radius) {
  if (d == 1) return 1u;
  const double v = sqrt((double)d) / radius * 255.0 + 0.5;
  return max(1u, (uint32_t)v & 0xFFu);
}

__device__ __forceinline__ uint32_t isqrt64(unsigned long long v) {
  unsigned long long r = (unsigned long long)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return (uint32_t)r;
}

__global__ __launch_bounds__(kThreads) void distance_thresh_kernel(uint32_t R, int rule,
                                                                  const uint32_t* __restrict__ dmax,
                                                                  const uint32_t* __restrict__ bbox,
                                                                  uint32_t* __restrict__ thresh) {
  const uint64_t r = global_thread();
  if (r >= R) return;
  const uint32_t top = dmax[r];
  if (rule == 0 || top <= 1) {   // (an id with no pixel: dmax = thresh = 0)
    thresh[r] = top;
    return;
  }
  const unsigned long long bw = bbox[4 * r + 2] - bbox[4 * r + 0] + 3ull, bh = bbox[4 * r + 3] - bbox[4 * r + 1] + 3ull;
  const double radius = (double)(isqrt64((bw * bw + bh * bh) >> 2) + 1u);
  const uint32_t target = scale_byte(top, radius);
  uint32_t lo = 1, hi = top;   // scale_byte is monotone: the lowest d that reaches the target
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (scale_byte(mid, radius) >= target) hi = mid;
    else lo = mid + 1;
  }
  thresh[r] = lo;
}

__global__ __launch_bounds__(kThreads) void distance_sums_kernel(const uint32_t* __restrict__ regions, uint32_t n,
                                                                uint32_t W, uint32_t R,
                                                                const uint16_t* __restrict__ D,
                                                                const uint32_t* __restrict__ thresh, uint32_t* count,
                                                                Scratch s) {
  __shared__ uint32_t s_key[kSlots], s_cnt[kSlots], s_sx[kSlots], s_sy[kSlots], s_last[kSlots];
  if (threadIdx.x < kSlots) {
    s_key[threadIdx.x] = kNoId;
    s_cnt[threadIdx.x] = s_sx[threadIdx.x] = s_sy[threadIdx.x] = s_last[threadIdx.x] = 0;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;   // (n < 2^31: no wrap)
    if (i >= n) continue;
    const uint32_t id = regions[i];
    if (id >= R || (uint32_t)D[i] < thresh[id]) continue;
    const uint32_t y = i / W, x = i - y * W;
    const uint32_t key = y << 16 | (0xFFFFu - x);
    const uint32_t slot = id % kSlots;
    if (slot_claim(s_key, slot, kNoId, id)) {   // (<= 1024 pixels a workgroup: the u32 sums hold)
      atomicAdd(&s_cnt[slot], 1u);
      atomicAdd(&s_sx[slot], x);
      atomicAdd(&s_sy[slot], y);
      atomicMax(&s_last[slot], key);
    } else {
      atomicAdd(&count[id], 1u);
      atomicAdd(&s.sumx[id], (unsigned long long)x);
      atomicAdd(&s.sumy[id], (unsigned long long)y);
      atomicMax(&s.last[id], key);
    }
  }
  __syncthreads();
  if (threadIdx.x < kSlots && s_key[threadIdx.x] != kNoId) {
    const uint32_t id = s_key[threadIdx.x];
    atomicAdd(&count[id], s_cnt[threadIdx.x]);
    atomicAdd(&s.sumx[id], (unsigned long long)s_sx[threadIdx.x]);
    atomicAdd(&s.sumy[id], (unsigned long long)s_sy[threadIdx.x]);
    atomicMax(&s.last[id], s_last[threadIdx.x]);
  }
}

// ---- centres ---------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void distance_decide_kernel(DistanceArgs a, Scratch s) {
  const uint64_t r = global_thread();
  if (r >= a.nregions) return;
  const uint32_t cnt = a.count[r];
  uint32_t centre = kNoId, want = kNoId;
  if (cnt != 0 && cnt <= 2) {
    const uint32_t key = s.last[r];
    centre = (0xFFFFu - (key & 0xFFFFu)) | (key >> 16) << 16;
  } else if (cnt != 0) {
    const uint32_t cx = (uint32_t)(s.sumx[r] / cnt), cy = (uint32_t)(s.sumy[r] / cnt);   // (means of coordinates: inside the frame)
    const size_t i = (size_t)cy * a.width + cx;
    if (a.regions[i] == r && (uint32_t)a.dist[i] >= a.thresh[r]) centre = cx | cy << 16;
    else want = cx | cy << 16;
  }
  a.centre[r] = centre;
  s.want[r] = want;
  s.near[r] = ~0ull;
}

__global__ __launch_bounds__(kThreads) void distance_nearest_kernel(const uint32_t* __restrict__ regions, uint32_t n,
                                                                   uint32_t W, uint32_t R,
                                                                   const uint16_t* __restrict__ D,
                                                                   const uint32_t* __restrict__ thresh, Scratch s) {
  __shared__ uint32_t s_key[kSlots];
  __shared__ unsigned long long s_near[kSlots];
  if (threadIdx.x < kSlots) {
    s_key[threadIdx.x] = kNoId;
    s_near[threadIdx.x] = ~0ull;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;   // (n < 2^31: no wrap)
    if (i >= n) continue;
    const uint32_t id = regions[i];
    if (id >= R) continue;
    const uint32_t c = s.want[id];
    if (c == kNoId || (uint32_t)D[i] < thresh[id]) continue;
    const uint32_t y = i / W, x = i - y * W;
    const long long dx = (long long)x - (long long)(c & 0xFFFFu), dy = (long long)y - (long long)(c >> 16);
    const unsigned long long key = (unsigned long long)(dx * dx + dy * dy) << 31 | i;
    const uint32_t slot = id % kSlots;
    if (slot_claim(s_key, slot, kNoId, id)) atomicMin(&s_near[slot], key);
    else atomicMin(&s.near[id], key);
  }
  __syncthreads();
  if (threadIdx.x < kSlots && s_key[threadIdx.x] != kNoId) atomicMin(&s.near[s_key[threadIdx.x]], s_near[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void distance_settle_kernel(DistanceArgs a, Scratch s) {
  const uint64_t r = global_thread();
  if (r >= a.nregions || s.want[r] == kNoId) return;
  const uint32_t i = (uint32_t)(s.near[r] & 0x7FFFFFFFull);   // (S is not empty: some pixel wrote its key)
  const uint32_t y = i / a.width;
  a.centre[r] = (i - y * a.width) | y << 16;
}

// ---- cores -----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cores_init_kernel(CoresArgs a) {
  const uint64_t r = global_thread();
  if (r == 0) *a.kept = 0;
  if (r < a.nregions) a.core_area[r] = 0;
}

__global__ __launch_bounds__(kThreads) void cores_kernel(CoresArgs a) {
  __shared__ uint32_t s_key[kSlots], s_cnt[kSlots], s_kept;
  if (threadIdx.x < kSlots) {
    s_key[threadIdx.x] = kNoId;
    s_cnt[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) s_kept = 0;
  __syncthreads();
  const uint32_t n = a.width * a.height, lane = threadIdx.x & 63u;
  uint32_t kept = 0;   // (lane 0: the wave's)
#pragma unroll
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {   // (every lane stays for the shuffles)
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;   // (n < 2^31: no wrap)
    const uint32_t id = i < n ? a.regions[i] : kNoId;
    bool in = false;
    if (i < n && id < a.nregions) {
      const uint32_t c = a.centre[id];   // (the id has this pixel: it has a centre)
      in = c != kNoId && a.component[i] == a.component[(size_t)(c >> 16) * a.width + (c & 0xFFFFu)];
    }
    if (i < n && a.core) a.core[i] = in ? 1 : 0;
    if (i < n && a.cored) a.cored[i] = in ? id : kNoId;
    kept += (uint32_t)__popcll(__ballot(in));
    const uint32_t key = in ? id : kNoId;
    const WaveRun run = wave_run(__shfl_up(key, 1) != key);
    if (run.tail && in) {
      if (slot_claim(s_key, id % kSlots, kNoId, id)) atomicAdd(&s_cnt[id % kSlots], run.length(lane));
      else atomicAdd(&a.core_area[id], run.length(lane));
    }
  }
  if (lane == 0 && kept) atomicAdd(&s_kept, kept);
  __syncthreads();
  if (threadIdx.x < kSlots && s_key[threadIdx.x] != kNoId) atomicAdd(&a.core_area[s_key[threadIdx.x]], s_cnt[threadIdx.x]);
  if (threadIdx.x == 0 && s_kept) atomicAdd(a.kept, s_kept);
}

uint32_t chunk_blocks(uint32_t n) { return (n + kChunk - 1) / kChunk; }

}  // namespace

size_t distance_scratch_bytes(uint32_t width, uint32_t height, uint32_t nregions) {
  return 32 * (size_t)nregions + 8 * (size_t)bands_of(height) * width + 2 * (size_t)width * height;
}

void launch_region_distance(const DistanceArgs& a, hipStream_t st) {
  const Scratch s = carve(a.scratch, a.width, a.height, a.nregions);
  const uint32_t W = a.width, H = a.height, R = a.nregions, n = W * H, bands = bands_of(H);
  const dim3 cells(blocks_for(W), bands);
  distance_init_kernel<<<blocks_for(R), kThreads, 0, st>>>(a, s);
  distance_heads_kernel<<<cells, kThreads, 0, st>>>(a.regions, W, H, s);
  distance_carry_kernel<<<blocks_for(W), kThreads, 0, st>>>(W, bands, s);
  distance_columns_kernel<<<cells, kThreads, 0, st>>>(W, H, bands, s, s.g);
  distance_rows_kernel<<<(H + kThreads / 64 - 1) / (kThreads / 64), kThreads, 0, st>>>(a.regions, W, H, R, s.g, a.dist);
  distance_stats_kernel<<<chunk_blocks(n), kThreads, 0, st>>>(a.regions, n, W, R, a.dist, a.dmax, a.bbox);
  distance_thresh_kernel<<<blocks_for(R), kThreads, 0, st>>>(R, a.rule, a.dmax, a.bbox, a.thresh);
  distance_sums_kernel<<<chunk_blocks(n), kThreads, 0, st>>>(a.regions, n, W, R, a.dist, a.thresh, a.count, s);
  distance_decide_kernel<<<blocks_for(R), kThreads, 0, st>>>(a, s);
  distance_nearest_kernel<<<chunk_blocks(n), kThreads, 0, st>>>(a.regions, n, W, R, a.dist, a.thresh, s);
  distance_settle_kernel<<<blocks_for(R), kThreads, 0, st>>>(a, s);
}

void launch_region_cores(const CoresArgs& a, hipStream_t st) {
  cores_init_kernel<<<blocks_for(a.nregions), kThreads, 0, st>>>(a);
  cores_kernel<<<chunk_blocks(a.width * a.height), kThreads, 0, st>>>(a);
}

}  // namespace dq
