// dq_regions.hip -- connected regions of a label map on gfx950 (MI355X).
//
// Input: a width x height row-major label map (u8 / u16 / u32) and a
// connectivity (4 or 8).  Two pixels are in one region when a path of 4- /
// 8-neighbours with EQUAL label values joins them.  Regions are numbered in
// raster order of their first pixel (the lowest y * width + x), so the answer
// is unique: every output is an integer that does not depend on scheduling.
//
// Passes (all on the caller's stream, no kernel waits for another workgroup,
// every loop ends by the thread's own atomics: parent values only decrease):
//   1 tile     one workgroup per kRegionTile^2 tile: rows cut into runs by a
//              wave ballot of "differs from the left neighbour", union-find of
//              the tile in LDS, then parent[i] = GLOBAL linear index of i's
//              tile-local root.  A root is always the minimum index of its set.
//   2 seam     one thread per pixel on a tile border: lock-free union with the
//              neighbours across the border (find both roots, atomicMin the
//              larger root's parent to the smaller, retry on a lost race).
//   3 flatten  parent[i] = root of i; counts the roots (parent[i] == i) of
//              every chunk of kRegionChunk pixels.
//   4 scan     one workgroup (dq_scan.h's top scan): exclusive prefix sum of
//              the chunk counts, total.
//   5 number   roots get region id = chunk offset + rank in the chunk (raster
//              order); a root with id < stats_cap initialises its stats.
//   6 assign   regions[i] = regions[parent[i]]; area / bounding box / colour
//              sums by integer atomics: one LDS add per run of consecutive
//              lanes of a wave that share a region, one global add per region
//              and workgroup.
//
// Peak extra device memory: 4 B per pixel (parent) + 4 B per 1024 pixels
// (chunk counts) + 4 B: 4.004 B per pixel, stream-ordered and owned by the
// call.  No floating point anywhere.
#include <hip/hip_runtime.h>

#include "dq_regions.h"
#include "dq_scan.h"
#include "dq_stage.h"

namespace dq {
namespace {

using scan::block_excl_scan;
using scan::chunks_of;

constexpr uint32_t T = kRegionTile;
static_assert(T == 64, "one wave lane per tile column");

template <int LB> struct LabelOf;
template <> struct LabelOf<1> { using type = uint8_t; };
template <> struct LabelOf<2> { using type = uint16_t; };
template <> struct LabelOf<4> { using type = uint32_t; };

template <int LB>
__device__ __forceinline__ uint32_t label_at(const void* labels, uint32_t i) {
  return (uint32_t)((const typename LabelOf<LB>::type*)labels)[i];
}

// The 4 / LB labels of one little-endian word.
template <int LB>
__device__ __forceinline__ void unpack_word(uint32_t w, uint32_t* dst) {
  if (LB == 4) {
    dst[0] = w;
  } else if (LB == 2) {
    dst[0] = w & 0xFFFFu;
    dst[1] = w >> 16;
  } else {
    dst[0] = w & 0xFFu;
    dst[1] = (w >> 8) & 0xFFu;
    dst[2] = (w >> 16) & 0xFFu;
    dst[3] = w >> 24;
  }
}

// One wave loads `cols` (1..64) labels of a row into LDS words: 16-B loads when
// the row segment starts 16-B aligned, 4-B loads when it starts 4-B aligned
// (u8 / u16), and element-wise for the tail or a misaligned start.
template <int LB>
__device__ __forceinline__ void load_row(const unsigned char* p, uint32_t cols, uint32_t* dst, uint32_t lane) {
  const uint32_t nbytes = cols * LB;
  const uintptr_t addr = (uintptr_t)p;
  uint32_t done = 0;
  if ((addr & 15u) == 0) {
    const uint32_t nvec = nbytes >> 4;
    if (lane < nvec) {
      const uint4 v = ((const uint4*)p)[lane];
      uint32_t* d = dst + lane * (16 / LB);
      unpack_word<LB>(v.x, d);
      unpack_word<LB>(v.y, d + 4 / LB);
      unpack_word<LB>(v.z, d + 8 / LB);
      unpack_word<LB>(v.w, d + 12 / LB);
    }
    done = nvec * (16 / LB);
  } else if (LB < 4 && (addr & 3u) == 0) {
    const uint32_t nword = nbytes >> 2;
    if (lane < nword) unpack_word<LB>(((const uint32_t*)p)[lane], dst + lane * (4 / LB));
    done = nword * (4 / LB);
  }
  for (uint32_t e = done + lane; e < cols; e += 64) dst[e] = label_at<LB>(p, e);
}

// ---- union-find in LDS (the tile pass) -----------------------------------
__device__ __forceinline__ uint32_t lds_find(uint32_t* par, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;   // (p < x: ends)
  }
}

__device__ __forceinline__ void lds_unite(uint32_t* par, uint32_t a, uint32_t b) {
  for (;;) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(&par[a], b);
    if (old == a) return;   // a was still a root: linked under the smaller root
    a = old;                // lost a race: a's set goes on from its new parent (< a)
  }
}

template <int LB>
__global__ __launch_bounds__(kThreads) void region_tile_kernel(const void* __restrict__ labels, uint32_t W,
                                                              uint32_t H, int conn8,
                                                              uint32_t* __restrict__ parent) {
  __shared__ uint32_t lab[T * T];
  __shared__ uint32_t par[T * T];
  const uint32_t x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  const uint32_t cols = min(T, W - x0), rows = min(T, H - y0);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  constexpr uint32_t kWaves = kThreads / 64;
  const unsigned char* base = (const unsigned char*)labels;

  for (uint32_t y = wave; y < rows; y += kWaves)
    load_row<LB>(base + ((size_t)(y0 + y) * W + x0) * LB, cols, lab + y * T, lane);
  __syncthreads();

  // runs of equal labels along each row: every pixel points at its run's start
  for (uint32_t y = wave; y < rows; y += kWaves) {
    const bool valid = lane < cols;
    const uint32_t L = valid ? lab[y * T + lane] : 0u;
    const WaveRun run = wave_run(valid && (lane == 0 || lab[y * T + lane - 1] != L));
    if (valid) par[y * T + lane] = y * T + run.start;
  }
  __syncthreads();

  // unions with the row above.  A pair whose union follows from the pair one
  // column to the left (same runs in both rows) is skipped; a diagonal pair is
  // needed only when neither straight pair beside it joins the same pixels.
  for (uint32_t y = wave; y < rows; y += kWaves) {
    if (y == 0 || lane >= cols) continue;
    const uint32_t i = y * T + lane, u = i - T;
    const uint32_t L = lab[i];
    const bool left_same = lane > 0 && lab[i - 1] == L;
    if (lab[u] == L) {
      if (!(left_same && lab[u - 1] == L)) lds_unite(par, i, u);
    } else if (conn8) {
      if (lane > 0 && lab[u - 1] == L && !left_same) lds_unite(par, i, u - 1);
      if (lane + 1 < cols && lab[u + 1] == L && lab[i + 1] != L) lds_unite(par, i, u + 1);
    }
  }
  __syncthreads();

  // the tile's order of pixels is the frame's raster order restricted to the
  // tile, so the tile-local minimum is the global minimum of the local set
  for (uint32_t y = wave; y < rows; y += kWaves) {
    if (lane >= cols) continue;
    const uint32_t r = lds_find(par, y * T + lane);
    parent[(y0 + y) * W + x0 + lane] = (y0 + r / T) * W + x0 + (r % T);
  }
}

// ---- lock-free union-find in global memory (the seam pass) ---------------
// Every read of parent[] here is an agent-scope atomic load: other workgroups
// (on other XCDs, behind other L2s) lower these words while this one reads.
__device__ __forceinline__ uint32_t g_find(uint32_t* par, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void g_unite(uint32_t* par, uint32_t a, uint32_t b) {
  const uint32_t a0 = a, b0 = b;
  uint32_t root;
  for (;;) {
    a = g_find(par, a);
    b = g_find(par, b);
    if (a == b) {
      root = a;
      break;
    }
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(&par[a], b);
    if (old == a) {
      root = b;
      break;
    }
    a = old;
  }
  // shorten the two chains just walked (root is an ancestor of both: <= their parents)
  if (root != a0) atomicMin(&par[a0], root);
  if (root != b0) atomicMin(&par[b0], root);
}

// Thread s < nh: pixel x of the k-th horizontal seam (row (k + 1) * T) and the
// row above it; the others: pixel y of a vertical seam (column (k + 1) * T)
// and the column left of it.  A straight pair is skipped only when the pair
// one step back ALONG THE SEAM joins the same two runs inside the same two
// tiles; a diagonal pair only when a straight pair beside it does the work.
template <int LB>
__global__ __launch_bounds__(kThreads) void region_seam_kernel(const void* __restrict__ labels, uint32_t W,
                                                              uint32_t H, int conn8, uint32_t* parent,
                                                              uint32_t nh, uint32_t total) {
  uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= total) return;
  if (s < nh) {
    const uint32_t k = s / W, x = s - k * W, y = (k + 1) * T;
    const uint32_t i = y * W + x, u = i - W;
    const uint32_t L = label_at<LB>(labels, i);
    const bool left_same = x > 0 && label_at<LB>(labels, i - 1) == L;
    if (label_at<LB>(labels, u) == L) {
      if (!((x % T) != 0 && left_same && label_at<LB>(labels, u - 1) == L)) g_unite(parent, i, u);
    } else if (conn8) {
      if (x > 0 && label_at<LB>(labels, u - 1) == L && !left_same) g_unite(parent, i, u - 1);
      if (x + 1 < W && label_at<LB>(labels, u + 1) == L && label_at<LB>(labels, i + 1) != L)
        g_unite(parent, i, u + 1);
    }
  } else {
    s -= nh;
    const uint32_t k = s / H, y = s - k * H, x = (k + 1) * T;
    const uint32_t i = y * W + x, l = i - 1;
    const uint32_t L = label_at<LB>(labels, i);
    const bool up_same = y > 0 && label_at<LB>(labels, i - W) == L;
    if (label_at<LB>(labels, l) == L) {
      if (!((y % T) != 0 && up_same && label_at<LB>(labels, l - W) == L)) g_unite(parent, i, l);
    } else if (conn8) {
      if (y > 0 && label_at<LB>(labels, l - W) == L && !up_same) g_unite(parent, i, l - W);
      if (y + 1 < H && label_at<LB>(labels, l + W) == L && label_at<LB>(labels, i + W) != L)
        g_unite(parent, i, l + W);
    }
  }
}

// ---- linear passes --------------------------------------------------------
// The four parents of pixels base .. base + 3 (0xFFFFFFFF past n: never a root
// flag, since i < n there is never 0xFFFFFFFF).
__device__ __forceinline__ void load4(const uint32_t* parent, uint32_t base, uint32_t n, uint32_t p[4]) {
  if (base + 4 <= n) {
    const uint4 v = *(const uint4*)(parent + base);   // parent is 16-B aligned, base a multiple of 4
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) p[j] = base + j < n ? parent[base + j] : 0xFFFFFFFFu;
  }
}

// parent[i] = root of i.  Other threads shorten other entries meanwhile: a
// walk sees an entry's old or new value, both ancestors in the same set, and a
// root's entry never changes in this pass.
__global__ __launch_bounds__(kThreads) void region_flatten_kernel(uint32_t* parent, uint32_t n,
                                                                 uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kThreads / 64];
  const uint32_t base = blockIdx.x * kChunk + threadIdx.x * 4;
  uint32_t p[4];
  load4(parent, base, n, p);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t i = base + j;
    if (i >= n) continue;
    if (p[j] == i) {
      ++c;
      continue;
    }
    uint32_t r = p[j];
    for (;;) {
      const uint32_t q = __hip_atomic_load(&parent[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (q == r) break;
      r = q;
    }
    if (r != p[j]) __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  uint32_t total;
  block_excl_scan<kThreads / 64>(c, wsum, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// Roots get their region id; a root with id < cap starts its region's stats.
template <int LB>
__global__ __launch_bounds__(kThreads) void region_number_kernel(
    const uint32_t* __restrict__ parent, uint32_t n, uint32_t W, const uint32_t* __restrict__ offsets,
    const void* __restrict__ labels, uint32_t* __restrict__ regions, uint32_t cap, uint32_t* __restrict__ area,
    uint32_t* __restrict__ bbox, uint32_t* __restrict__ first, uint32_t* __restrict__ label,
    unsigned long long* __restrict__ sums) {
  __shared__ uint32_t wsum[kThreads / 64];
  const uint32_t base = blockIdx.x * kChunk + threadIdx.x * 4;
  uint32_t p[4];
  load4(parent, base, n, p);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) c += p[j] == base + j ? 1u : 0u;
  uint32_t total;
  uint32_t id = offsets[blockIdx.x] + block_excl_scan<kThreads / 64>(c, wsum, total);
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t i = base + j;
    if (p[j] != i) continue;
    regions[i] = id;
    if (id < cap) {
      const uint32_t y = i / W;
      if (area) area[id] = 0;
      if (bbox) {
        bbox[4 * (size_t)id + 0] = 0xFFFFFFFFu;   // x0: atomicMin
        bbox[4 * (size_t)id + 1] = y;             // y0: the first pixel's row
        bbox[4 * (size_t)id + 2] = 0;             // x1: atomicMax
        bbox[4 * (size_t)id + 3] = y;             // y1: atomicMax
      }
      if (first) first[id] = i;
      if (label) label[id] = label_at<LB>(labels, i);
      if (sums) {
        sums[3 * (size_t)id + 0] = 0;
        sums[3 * (size_t)id + 1] = 0;
        sums[3 * (size_t)id + 2] = 0;
      }
    }
    ++id;
  }
}

// One region's stats contribution to global memory.
__device__ __forceinline__ void stats_to_global(uint32_t id, uint32_t cnt, uint32_t xlo, uint32_t xhi, uint32_t yhi,
                                                uint32_t r, uint32_t g, uint32_t b, uint32_t* area, uint32_t* bbox,
                                                unsigned long long* sums) {
  if (area) atomicAdd(&area[id], cnt);
  if (bbox) {
    atomicMin(&bbox[4 * (size_t)id + 0], xlo);
    atomicMax(&bbox[4 * (size_t)id + 2], xhi);
    atomicMax(&bbox[4 * (size_t)id + 3], yhi);
  }
  if (sums) {
    atomicAdd(&sums[3 * (size_t)id + 0], (unsigned long long)r);
    atomicAdd(&sums[3 * (size_t)id + 1], (unsigned long long)g);
    atomicAdd(&sums[3 * (size_t)id + 2], (unsigned long long)b);
  }
}

// regions[i] = the id of i's root (written by the pass before; this pass
// writes non-root entries only).  Stats: the lanes of a wave hold consecutive
// pixels; each run of lanes with one region id adds once, from its last lane,
// into the workgroup's LDS slot id % kStatSlots when that slot is free or
// already the region's (one global add per region and workgroup at the end:
// a large region is met by every workgroup over it), else straight to global
// memory.  Integer adds, min and max: the result is the same either way.
constexpr uint32_t kStatSlots = 64, kNoRegion = 0xFFFFFFFFu;

__global__ __launch_bounds__(kThreads) void region_assign_kernel(
    const uint32_t* __restrict__ parent, uint32_t n, uint32_t W, uint32_t* regions, uint32_t cap,
    uint32_t* __restrict__ area, uint32_t* __restrict__ bbox, const uint32_t* __restrict__ pixels,
    unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_key[kStatSlots], s_cnt[kStatSlots], s_xlo[kStatSlots], s_xhi[kStatSlots],
      s_yhi[kStatSlots], s_r[kStatSlots], s_g[kStatSlots], s_b[kStatSlots];
  const uint32_t lane = threadIdx.x & 63u;
  const bool stats = cap != 0 && (area || bbox || sums);   // (uniform over the grid)
  if (stats) {
    if (threadIdx.x < kStatSlots) {
      s_key[threadIdx.x] = kNoRegion;
      s_cnt[threadIdx.x] = s_xhi[threadIdx.x] = s_yhi[threadIdx.x] = 0;
      s_r[threadIdx.x] = s_g[threadIdx.x] = s_b[threadIdx.x] = 0;
      s_xlo[threadIdx.x] = 0xFFFFFFFFu;
    }
    __syncthreads();
  }
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    const bool valid = i < n;
    uint32_t id = kNoRegion;
    if (valid) {
      const uint32_t p = parent[i];
      id = __hip_atomic_load(&regions[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p != i) regions[i] = id;
    }
    if (!stats) continue;
    const uint32_t prev = __shfl_up(id, 1);
    const WaveRun run = wave_run(prev != id || !valid);
    uint32_t rg = 0, b = 0;
    if (sums) {   // (uniform) the run's sums of R | G << 16 and of B: <= 64 * 255 each
      const uint32_t px = valid ? pixels[i] : 0u;
      rg = run_sum(((px >> 16) & 0xFFu) | (((px >> 8) & 0xFFu) << 16), run);
      b = run_sum(px & 0xFFu, run);
    }
    if (run.tail && valid && id < cap) {
      const uint32_t cnt = run.length(lane), i0 = i + 1 - cnt;
      const uint32_t ya = i0 / W, xa = i0 - ya * W, yb = i / W, xb = i - yb * W;
      // a run that wraps to the next row holds the last pixel of one row and the first of the next
      const uint32_t xlo = yb > ya ? 0u : xa, xhi = yb > ya ? W - 1 : xb;
      const uint32_t slot = id % kStatSlots;
      if (slot_claim(s_key, slot, kNoRegion, id)) {   // (<= 1024 pixels a workgroup: the u32 sums hold)
        atomicAdd(&s_cnt[slot], cnt);
        atomicMin(&s_xlo[slot], xlo);
        atomicMax(&s_xhi[slot], xhi);
        atomicMax(&s_yhi[slot], yb);
        atomicAdd(&s_r[slot], rg & 0xFFFFu);
        atomicAdd(&s_g[slot], rg >> 16);
        atomicAdd(&s_b[slot], b);
      } else {
        stats_to_global(id, cnt, xlo, xhi, yb, rg & 0xFFFFu, rg >> 16, b, area, bbox, sums);
      }
    }
  }
  if (stats) {
    __syncthreads();
    if (threadIdx.x < kStatSlots && s_key[threadIdx.x] != kNoRegion)
      stats_to_global(s_key[threadIdx.x], s_cnt[threadIdx.x], s_xlo[threadIdx.x], s_xhi[threadIdx.x],
                      s_yhi[threadIdx.x], s_r[threadIdx.x], s_g[threadIdx.x], s_b[threadIdx.x], area, bbox, sums);
  }
}

size_t parent_words(uint32_t n) { return ((size_t)n + 3) & ~(size_t)3; }

template <int LB>
void launch_lb(const RegionArgs& a, hipStream_t st) {
  const uint32_t W = a.width, H = a.height, n = W * H;
  const uint32_t tx = (W + T - 1) / T, ty = (H + T - 1) / T, nchunks = chunks_of(n);
  const int conn8 = a.connectivity == 8 ? 1 : 0;
  uint32_t* parent = a.scratch;
  uint32_t* counts = a.scratch + parent_words(n);
  const bool st_on = a.stats_cap != 0;
  uint32_t* area = st_on ? a.area : nullptr;
  uint32_t* bbox = st_on ? a.bbox : nullptr;
  uint32_t* first = st_on ? a.first : nullptr;
  uint32_t* label = st_on ? a.label : nullptr;
  unsigned long long* sums = st_on ? a.sums : nullptr;

  region_tile_kernel<LB><<<dim3(tx, ty), kThreads, 0, st>>>(a.labels, W, H, conn8, parent);
  const uint32_t nh = (ty - 1) * W, nv = (tx - 1) * H;
  if (nh + nv != 0)
    region_seam_kernel<LB><<<(nh + nv + kThreads - 1) / kThreads, kThreads, 0, st>>>(a.labels, W, H, conn8,
                                                                                    parent, nh, nh + nv);
  region_flatten_kernel<<<nchunks, kThreads, 0, st>>>(parent, n, counts);
  // (roots <= n <= 2^31 - 1: the saturating sums are the sums)
  scan::scan_top_kernel<<<1, 1024, 0, st>>>(counts, nchunks);
  region_number_kernel<LB><<<nchunks, kThreads, 0, st>>>(parent, n, W, counts, a.labels, a.regions, a.stats_cap,
                                                         area, bbox, first, label, sums);
  region_assign_kernel<<<nchunks, kThreads, 0, st>>>(parent, n, W, a.regions, a.stats_cap, area, bbox, a.pixels,
                                                     sums);
}

}  // namespace

size_t region_scratch_words(uint32_t width, uint32_t height) {
  const uint32_t n = width * height;
  return parent_words(n) + chunks_of(n) + 1;
}

const uint32_t* region_count_word(const RegionArgs& a) {
  const uint32_t n = a.width * a.height;
  return a.scratch + parent_words(n) + chunks_of(n);
}

void launch_label_regions(const RegionArgs& a, hipStream_t stream) {
  switch (a.label_bytes) {
    case 1: launch_lb<1>(a, stream); break;
    case 2: launch_lb<2>(a, stream); break;
    default: launch_lb<4>(a, stream); break;
  }
}

}  // namespace dq
