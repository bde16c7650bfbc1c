// dq_skeleton.hip -- the skeletons of all regions of a region map on gfx950
// (MI355X): Guo-Hall two-subiteration thinning on bit planes.
//
// Input: a width x height map of ids; an id < R is a region (its pixels need
// not be connected), an id >= R is background.  include/dq_hip.h, "region
// skeleton", has the full definition; in short: a pixel's neighbour n_k is on
// iff it lies in the frame, has the pixel's own id and is still alive; a
// subiteration deletes every alive pixel with C == 1, N in {2, 3} and its own
// side test, all decided from the state before it; an iteration is both
// subiterations; the run stops after the first iteration that deletes nothing.
// Regions are disjoint and a neighbour of another id is off, so every region
// thins exactly as its own mask would alone.
//
// The map is read once.  That pass leaves one bit per pixel in u64 words of 64
// pixels along x (bit i of word c of a row: x = 64 c + i; rows padded to whole
// words): the ALIVE plane (id < R) and four SAME planes (the neighbour to the E,
// SE, S, SW has the same id, and the id is < R).  The sameness towards W, N, NW,
// NE is the E, S, SE, SW bit of that neighbour: a shift of the word beside or above.
// A subiteration on 64 pixels is then word logic: the alive words of three rows
// shifted by a bit with the carries of the words beside them, ANDed with the
// eight same words; C == 1 and 2 <= min(N1, N2) <= 3 by bit-sliced adders.
//
// Kernels (no kernel waits for another workgroup):
//   init     the call's words: skel_area, thick, the tile flags, the launches' words
//   planes   one wave per row and 16 words: five ballots per 64 pixels, lane j
//            keeps word j, one store per plane; `when` cleared
//   thin     one workgroup per tile of kSkeletonTileWords x kSkeletonTileRows
//            (384 x 64 pixels) with a halo of one word (64 pixels) to either side and
//            2 * kSkeletonIters rows above and below, in LDS: up to kSkeletonIters
//            iterations, every subiteration from one LDS buffer into the other.
//            What lies beyond the halo is unknown, so subiteration s leaves ring s
//            of the halo wrong; after 2 * kSkeletonIters of them the core is still
//            right, and only the core is written, to the OTHER alive plane (no
//            workgroup reads a halo that a neighbour is overwriting).  `when` at
//            each deletion in the core.  A tile none of whose 3 x 3 tiles deleted
//            in the launch before does nothing (DESIGN.md has the proof); a tile
//            stops at its first iteration that changes nothing in its LDS.
//   outputs  per pixel: skel, skeled; per run of equal ids along a wave the alive
//            count and the highest `when` through the workgroup's LDS slot cache
//            (dq_stage.h); the pixels kept by ballot count
#include <hip/hip_runtime.h>

#include "dq_skeleton.h"
#include "dq_stage.h"

namespace dq {
namespace {

using u64 = unsigned long long;

constexpr uint32_t kSlots = 64;
constexpr uint32_t kPlaneWords = 16;   // the words of a row one wave of the planes pass makes
constexpr int kIters = (int)kSkeletonIters;
constexpr int kHaloRows = 2 * kIters;
constexpr int kTileW = (int)kSkeletonTileWords + 2;                 // the core and one halo word to either side
constexpr int kTileR = (int)kSkeletonTileRows + 2 * kHaloRows;
constexpr int kThinThreads = 512;                                  // of a thinning workgroup: two words each (measured
                                                                   // against 256 and 1024: DESIGN.md)
constexpr int kPer = kTileW * kTileR / kThinThreads;               // the words of a thread
constexpr int kRowStep = kThinThreads / kTileW;                    // a thread's words lie this many rows apart
constexpr int kStride = kTileW + 2;                                // an LDS row: a zero word before and behind
constexpr int kLdsWords = (kTileR + 2) * kStride;                  // a zero row above and below
static_assert(2 * kIters <= 64, "the halo to either side is one word");
static_assert(2 * kIters <= (int)kSkeletonTileRows && 2 * kIters <= 64 * (int)kSkeletonTileWords,
              "a tile's halo lies in its eight neighbour tiles (the tile-skip rule)");
static_assert(kTileW * kTileR == kPer * kThinThreads && kThinThreads % kTileW == 0, "every thread has kPer words of one column");
static_assert(kSkeletonMaxIters <= 0xFFFFu, "`when` is u16");

struct Planes {
  u64* alive[2];        // launch l reads alive[l % 2] and writes the other
  u64* same[4];         // E, SE, S, SW
  uint32_t* flag[2];    // per tile: it deleted in its core; launch l reads flag[l % 2] and writes the other
  uint32_t* last;       // kSkeletonMaxLaunches
  uint32_t* kept;
  uint32_t wpr, tiles_x, tiles_y;
};

uint32_t words_per_row(uint32_t width) { return (width + 63u) / 64u; }

Planes carve(void* scratch, uint32_t width, uint32_t height) {
  Planes p;
  p.wpr = words_per_row(width);
  p.tiles_x = (p.wpr + kSkeletonTileWords - 1) / kSkeletonTileWords;
  p.tiles_y = (height + kSkeletonTileRows - 1) / kSkeletonTileRows;
  const size_t words = (size_t)p.wpr * height, tiles = (size_t)p.tiles_x * p.tiles_y;
  u64* w = (u64*)scratch;
  p.alive[0] = w, p.alive[1] = w + words;
  for (int d = 0; d < 4; ++d) p.same[d] = w + (2 + d) * words;
  p.flag[0] = (uint32_t*)(w + 6 * words);
  p.flag[1] = p.flag[0] + tiles;
  p.last = p.flag[1] + tiles;
  p.kept = p.last + kSkeletonMaxLaunches;
  return p;
}

__global__ __launch_bounds__(kThreads) void skeleton_init_kernel(SkeletonArgs a, Planes p) {
  const uint64_t i = global_thread();
  if (i < a.nregions) {
    if (a.skel_area) a.skel_area[i] = 0;
    if (a.thick) a.thick[i] = 0;
  }
  if (i < (uint64_t)p.tiles_x * p.tiles_y) p.flag[0][i] = 1;   // (before the first launch every tile counts as changed)
  if (i < kSkeletonMaxLaunches) p.last[i] = 0;
  if (i == 0) *p.kept = 0;
}

// ---- planes ----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void skeleton_planes_kernel(SkeletonArgs a, Planes p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t y = blockIdx.y * (kThreads / 64) + (threadIdx.x >> 6);
  if (y >= a.height) return;   // (the whole wave)
  const uint32_t W = a.width, R = a.nregions, c0 = blockIdx.x * kPlaneWords;
  const uint32_t* row = a.regions + (size_t)y * W;
  const uint32_t* below = y + 1 < a.height ? row + W : nullptr;
  u64 alive = 0, e = 0, se = 0, s = 0, sw = 0;
  for (uint32_t j = 0; j < kPlaneWords && c0 + j < p.wpr; ++j) {   // (uniform)
    const uint32_t x = (c0 + j) * 64u + lane;
    const bool valid = x < W;
    const uint32_t id = valid ? row[x] : kNoId;
    const bool on = valid && id < R;
    const u64 b_alive = __ballot(on);
    const u64 b_e = __ballot(on && x + 1 < W && row[x + 1] == id);
    const u64 b_se = __ballot(on && below && x + 1 < W && below[x + 1] == id);
    const u64 b_s = __ballot(on && below && below[x] == id);
    const u64 b_sw = __ballot(on && below && x > 0 && below[x - 1] == id);
    if (lane == j) alive = b_alive, e = b_e, se = b_se, s = b_s, sw = b_sw;
    if (valid && a.when) a.when[(size_t)y * W + x] = 0;
  }
  if (lane < kPlaneWords && c0 + lane < p.wpr) {
    const size_t at = (size_t)y * p.wpr + c0 + lane;
    p.alive[0][at] = alive;
    p.same[0][at] = e, p.same[1][at] = se, p.same[2][at] = s, p.same[3][at] = sw;
  }
}

// ---- thinning ----------------------------------------------------------------
// Bit i of the result: bit i - 1 of x (the pixel to the W), the carry from the word `left` of it.
__device__ __forceinline__ u64 from_west(u64 left, u64 x) { return x << 1 | left >> 63; }
// Bit i of the result: bit i + 1 of x (the pixel to the E), the carry from the word `right` of it.
__device__ __forceinline__ u64 from_east(u64 x, u64 right) { return x >> 1 | right << 63; }

// The word (y, c) of a plane; 0 outside the frame.
__device__ __forceinline__ u64 plane_word(const u64* __restrict__ plane, int y, int c, const Planes& p, uint32_t H) {
  if (y < 0 || y >= (int)H || c < 0 || c >= (int)p.wpr) return 0;
  return plane[(size_t)y * p.wpr + c];
}

// The sameness of the 64 pixels of a word towards their eight neighbours.
struct Same {
  u64 nw, n, ne, e, se, s, sw, w;
};

__device__ __forceinline__ Same same_of(const Planes& p, uint32_t H, int y, int c) {
  const u64 *E = p.same[0], *SE = p.same[1], *S = p.same[2], *SW = p.same[3];
  Same m;
  m.e = plane_word(E, y, c, p, H), m.se = plane_word(SE, y, c, p, H);
  m.s = plane_word(S, y, c, p, H), m.sw = plane_word(SW, y, c, p, H);
  // W of p = E of the pixel to the W; N = S of the one above; NW = SE of the one above to the W; NE = SW of the one above to the E
  m.w = from_west(plane_word(E, y, c - 1, p, H), m.e);
  m.n = plane_word(S, y - 1, c, p, H);
  m.nw = from_west(plane_word(SE, y - 1, c - 1, p, H), plane_word(SE, y - 1, c, p, H));
  m.ne = from_east(plane_word(SW, y - 1, c, p, H), plane_word(SW, y - 1, c + 1, p, H));
  return m;
}

// (the four bits sum to at least 2, the four bits sum to 4)
__device__ __forceinline__ void count4(u64 b0, u64 b1, u64 b2, u64 b3, u64& ge2, u64& eq4) {
  const u64 x01 = b0 ^ b1, a01 = b0 & b1, x23 = b2 ^ b3, a23 = b2 & b3;
  ge2 = a01 | a23 | (x01 & x23);
  eq4 = a01 & a23;
}

// One subiteration on the word at `at` of the LDS tile `b`, whose own value is `mid`: the word after it.
__device__ __forceinline__ u64 thin_word(const u64* b, int at, u64 mid, const Same& m, bool second) {
  const u64 up = b[at - kStride], dn = b[at + kStride];
  const u64 n0 = from_west(b[at - kStride - 1], up) & m.nw;
  const u64 n1 = up & m.n;
  const u64 n2 = from_east(up, b[at - kStride + 1]) & m.ne;
  const u64 n3 = from_east(mid, b[at + 1]) & m.e;
  const u64 n4 = from_east(dn, b[at + kStride + 1]) & m.se;
  const u64 n5 = dn & m.s;
  const u64 n6 = from_west(b[at + kStride - 1], dn) & m.sw;
  const u64 n7 = from_west(b[at - 1], mid) & m.w;
  // C == 1: exactly one of the four 0 -> 1 patterns
  const u64 t1 = ~n1 & (n2 | n3), t2 = ~n3 & (n4 | n5), t3 = ~n5 & (n6 | n7), t4 = ~n7 & (n0 | n1);
  const u64 c_is_1 = ((t1 ^ t2) ^ (t3 ^ t4)) & ~((t1 & t2) | (t3 & t4));
  // 2 <= min(N1, N2) <= 3: both at least 2, not both 4
  u64 ge2_a, eq4_a, ge2_b, eq4_b;
  count4(n0 | n1, n2 | n3, n4 | n5, n6 | n7, ge2_a, eq4_a);
  count4(n1 | n2, n3 | n4, n5 | n6, n7 | n0, ge2_b, eq4_b);
  const u64 n_is_2_or_3 = ge2_a & ge2_b & ~(eq4_a & eq4_b);
  const u64 side = second ? (n5 | n6 | ~n0) & n7 : (n1 | n2 | ~n4) & n3;
  return mid & ~(c_is_1 & n_is_2_or_3 & ~side);
}

__global__ __launch_bounds__(kThinThreads) void skeleton_thin_kernel(Planes p, uint32_t W, uint32_t H, uint32_t launch,
                                                                uint32_t iters, uint16_t* when) {
  __shared__ u64 s_buf[2][kLdsWords];
  __shared__ uint32_t s_go, s_last;
  const uint32_t tx = blockIdx.x, ty = blockIdx.y, tile = ty * p.tiles_x + tx;
  const uint32_t* flag_in = p.flag[launch & 1u];
  uint32_t* flag_out = p.flag[(launch + 1u) & 1u];
  if (threadIdx.x == 0) s_go = 0, s_last = 0;
  __syncthreads();
  if (threadIdx.x < 9) {
    const int nx = (int)tx + (int)(threadIdx.x % 3) - 1, ny = (int)ty + (int)(threadIdx.x / 3) - 1;
    if (nx >= 0 && nx < (int)p.tiles_x && ny >= 0 && ny < (int)p.tiles_y && flag_in[(size_t)ny * p.tiles_x + nx])
      atomicOr(&s_go, 1u);
  }
  __syncthreads();
  if (!s_go) {   // (the whole workgroup) nothing in reach changed: the other plane holds this core already
    if (threadIdx.x == 0) flag_out[tile] = 0;
    return;
  }

  for (int i = threadIdx.x; i < kLdsWords; i += kThinThreads) s_buf[0][i] = s_buf[1][i] = 0;
  __syncthreads();

  const u64* src = p.alive[launch & 1u];
  u64* dst = p.alive[(launch + 1u) & 1u];
  const int c = threadIdx.x % kTileW, g = threadIdx.x / kTileW;
  const int wc = (int)(tx * kSkeletonTileWords) - 1 + c;
  const int y0 = (int)(ty * kSkeletonTileRows) - kHaloRows + g;
  const bool core_col = c >= 1 && c <= (int)kSkeletonTileWords;
  u64 cur[kPer];
  Same m[kPer];
  int at[kPer];
  bool core[kPer];   // the thread's word j is core iff its row and its column are
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int r = j * kRowStep + g;
    at[j] = (r + 1) * kStride + c + 1;
    core[j] = core_col && r >= kHaloRows && r < kHaloRows + (int)kSkeletonTileRows;
    cur[j] = plane_word(src, y0 + j * kRowStep, wc, p, H);
    m[j] = same_of(p, H, y0 + j * kRowStep, wc);
    s_buf[0][at[j]] = cur[j];
  }
  __syncthreads();

  const uint32_t first = launch * kSkeletonIters;
  uint32_t mine = 0;   // the last iteration of this launch in which one of the thread's core words lost a pixel
  for (uint32_t it = 1; it <= iters; ++it) {
    u64 half[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      half[j] = thin_word(s_buf[0], at[j], cur[j], m[j], false);
      s_buf[1][at[j]] = half[j];
    }
    __syncthreads();
    u64 changed = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const u64 v = thin_word(s_buf[1], at[j], half[j], m[j], true);
      s_buf[0][at[j]] = v;
      u64 gone = cur[j] & ~v;
      cur[j] = v;
      changed |= gone;
      if (core[j] && gone) {   // (alive bits lie in the frame)
        mine = it;
        if (when) {
          uint16_t* w = when + (size_t)(y0 + j * kRowStep) * W + (size_t)wc * 64u;
          for (; gone; gone &= gone - 1) w[__ffsll((long long)gone) - 1] = (uint16_t)(first + it);
        }
      }
    }
    if (!__syncthreads_or(changed != 0)) break;   // (the tile's LDS is at a fixed point: so is its core)
  }

#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int y = y0 + j * kRowStep;
    if (core[j] && y < (int)H && wc < (int)p.wpr) dst[(size_t)y * p.wpr + wc] = cur[j];
  }
  if (mine) atomicMax(&s_last, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    flag_out[tile] = s_last != 0;
    if (s_last) atomicMax(&p.last[launch], s_last);
  }
}

// ---- outputs ---------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void skeleton_outputs_kernel(SkeletonArgs a, Planes p, const u64* alive) {
  __shared__ uint32_t s_key[kSlots], s_cnt[kSlots], s_thick[kSlots], s_kept;
  if (threadIdx.x < kSlots) {
    s_key[threadIdx.x] = kNoId;
    s_cnt[threadIdx.x] = s_thick[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) s_kept = 0;
  __syncthreads();
  const uint32_t n = a.width * a.height, lane = threadIdx.x & 63u;
  const bool per_region = a.skel_area || a.thick;
  uint32_t kept = 0;   // (lane 0: the wave's)
#pragma unroll
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {   // (every lane stays for the shuffles)
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;   // (n < 2^31: no wrap)
    const uint32_t id = i < n ? a.regions[i] : kNoId;
    const bool region = i < n && id < a.nregions;
    bool in = false;
    if (region) {
      const uint32_t y = i / a.width, x = i - y * a.width;
      in = ((alive[(size_t)y * p.wpr + (x >> 6)] >> (x & 63u)) & 1ull) != 0;
    }
    if (i < n && a.skel) a.skel[i] = in ? 1 : 0;
    if (i < n && a.skeled) a.skeled[i] = in ? id : kNoId;
    kept += (uint32_t)__popcll(__ballot(in));
    if (!per_region) continue;   // (uniform)
    const uint32_t key = region ? id : kNoId;
    const WaveRun run = wave_run(__shfl_up(key, 1) != key);
    const uint32_t cnt = run_sum(in ? 1u : 0u, run);
    const uint32_t th = run_max(region && a.thick ? (uint32_t)a.when[i] : 0u, run);
    if (run.tail && region) {
      if (slot_claim(s_key, id % kSlots, kNoId, id)) {
        atomicAdd(&s_cnt[id % kSlots], cnt);
        atomicMax(&s_thick[id % kSlots], th);
      } else {
        if (a.skel_area) atomicAdd(&a.skel_area[id], cnt);
        if (a.thick) atomicMax(&a.thick[id], th);
      }
    }
  }
  if (lane == 0 && kept) atomicAdd(&s_kept, kept);
  __syncthreads();
  if (threadIdx.x < kSlots && s_key[threadIdx.x] != kNoId) {
    if (a.skel_area) atomicAdd(&a.skel_area[s_key[threadIdx.x]], s_cnt[threadIdx.x]);
    if (a.thick) atomicMax(&a.thick[s_key[threadIdx.x]], s_thick[threadIdx.x]);
  }
  if (threadIdx.x == 0 && s_kept) atomicAdd(p.kept, s_kept);
}

}  // namespace

size_t skeleton_scratch_bytes(uint32_t width, uint32_t height) {
  const Planes p = carve(nullptr, width, height);
  return 48 * (size_t)p.wpr * height + 8 * (size_t)p.tiles_x * p.tiles_y + 4 * (size_t)kSkeletonMaxLaunches + 8;
}

void launch_skeleton_planes(const SkeletonArgs& a, hipStream_t st) {
  const Planes p = carve(a.scratch, a.width, a.height);
  const uint64_t items = max(max((uint64_t)a.nregions, (uint64_t)p.tiles_x * p.tiles_y), (uint64_t)kSkeletonMaxLaunches);
  skeleton_init_kernel<<<blocks_for(items), kThreads, 0, st>>>(a, p);
  const dim3 grid((p.wpr + kPlaneWords - 1) / kPlaneWords, (a.height + kThreads / 64 - 1) / (kThreads / 64));
  skeleton_planes_kernel<<<grid, kThreads, 0, st>>>(a, p);
}

void launch_skeleton_thin(const SkeletonArgs& a, uint32_t launch, uint32_t iters, hipStream_t st) {
  const Planes p = carve(a.scratch, a.width, a.height);
  skeleton_thin_kernel<<<dim3(p.tiles_x, p.tiles_y), kThinThreads, 0, st>>>(p, a.width, a.height, launch, iters, a.when);
}

const uint32_t* skeleton_last_words(const SkeletonArgs& a) { return carve(a.scratch, a.width, a.height).last; }

void launch_skeleton_outputs(const SkeletonArgs& a, uint32_t launches, hipStream_t st) {
  const Planes p = carve(a.scratch, a.width, a.height);
  const uint32_t n = a.width * a.height;
  skeleton_outputs_kernel<<<(n + kChunk - 1) / kChunk, kThreads, 0, st>>>(a, p, p.alive[launches & 1u]);
}

const uint32_t* skeleton_kept_word(const SkeletonArgs& a) { return carve(a.scratch, a.width, a.height).kept; }

}  // namespace dq
