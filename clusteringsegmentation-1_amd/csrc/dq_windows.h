// dq_windows.h -- the capture windows of a region map (dq_windows.hip): the
// launchers behind dq_hip_region_windows_dev (include/dq_hip.h, "capture
// windows"; DESIGN.md 5a'''''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dq_stage.h"

namespace dq {

struct WindowsArgs {
  const uint32_t* regions;   // width * height region ids, each < nregions
  uint32_t width, height;    // <= 65535 each, width * height <= 2^31 - 1
  uint32_t nregions;         // 1 .. 2^31 - 1
  uint32_t block, expand;    // 1 .. 8, 0 .. 3
  const uint8_t* mask;       // optional: width * height bytes, nonzero = consumed
  const uint32_t* area;      // optional: nregions words; area[r] <= min_area: r is absent
  uint32_t min_area;
  uint32_t* offsets;         // nregions + 1
  uint32_t* coords;          // optional: Coord words x | y << 16
  uint32_t* index;           // optional: pixel indexes y * width + x
  const uint32_t* pixels;    // optional: the frame
  uint32_t* colors;          // optional (needs pixels): words of the frame
  uint32_t* blocks;          // windows_blocks_bytes(..) bytes, owned by the call
  uint32_t* pairs;           // windows_pairs_bytes(P, T) bytes, owned by the call
};

// The call has three parts with a small read-back after the first two:
//   launch_windows_blocks   per block its surviving pixels and distinct ids, per id
//                           its block rows; the members of every block counted and
//                           scanned (P pairs), the window rows per id scanned (T)
//   (the host reads P and T, refuses T > P and allocates the pairs and the table)
//   launch_windows_count    the pairs (block, id) block-major, the surviving pixels
//                           per (id, block row), their prefix sums (M)
//   (the host reads M and decides -3 and M <= cap)
//   launch_windows_offsets  the offsets
//   launch_windows_lists    a position per pair (one wave per block row), then the
//                           pixels of every pair at its position

// block^2 + 2 words per block (m and the id count, the distinct ids, the member count), 2 words per
// region (first and last block row), a word per 1024 of each and 3 more (the sums of the two scans).
size_t windows_blocks_bytes(uint32_t width, uint32_t height, uint32_t block, uint32_t nregions);
// 8 B per pair, 4 B per table entry (T <= P), 4 B per 1024 entries and 4 B.
size_t windows_pairs_bytes(uint32_t npairs, uint32_t nrows);

void launch_windows_blocks(const WindowsArgs& a, hipStream_t stream);
const uint32_t* windows_pairs_word(const WindowsArgs& a);   // P (saturates at 2^32 - 1)
const uint32_t* windows_rows_word(const WindowsArgs& a);    // T (saturates at 2^32 - 1)
void launch_windows_count(const WindowsArgs& a, uint32_t npairs, uint32_t nrows, hipStream_t stream);
const uint32_t* windows_total_word(const WindowsArgs& a, uint32_t npairs, uint32_t nrows);   // M (saturates)
void launch_windows_offsets(const WindowsArgs& a, uint32_t npairs, uint32_t nrows, uint32_t total, hipStream_t stream);
void launch_windows_lists(const WindowsArgs& a, uint32_t npairs, uint32_t nrows, uint32_t total, hipStream_t stream);

// For the stages that work on the pairs themselves (dq_wtags.hip): what the parts above leave in
// the call's scratch.  info[b] = m(b) | distinct ids << 16 and ids[b * block^2 ..] after
// launch_windows_blocks; pairbase[b] (nblocks + 1 entries) = the first pair of block b;
// pair_block[i] after launch_windows_count; pair_word[i] = the pair's id after
// launch_windows_count and its list position after launch_windows_walk.
struct WindowsView {
  const uint32_t *info, *ids, *pairbase, *pair_word, *pair_block;
  uint32_t nblocks;
};
WindowsView windows_view(const WindowsArgs& a, uint32_t npairs);
// The first half of launch_windows_lists alone (after launch_windows_offsets; once per call).
void launch_windows_walk(const WindowsArgs& a, uint32_t npairs, uint32_t nrows, hipStream_t stream);

// The d x d block grid of a frame, for the kernels of both stages: BW x BH = NB blocks of dd pixels.
struct Grid {
  uint32_t W, H, d, dd, BW, BH, NB;
};

inline Grid block_grid(uint32_t width, uint32_t height, uint32_t block) {
  Grid g;
  g.W = width, g.H = height, g.d = block, g.dd = block * block;
  g.BW = (g.W + g.d - 1) / g.d, g.BH = (g.H + g.d - 1) / g.d, g.NB = g.BW * g.BH;
  return g;
}

// The lane's pixel of block b: its id (kNoId outside the block or the frame, or
// for an id >= R) and whether it survives the mask.
__device__ __forceinline__ void block_pixel(const uint32_t* __restrict__ reg, const uint8_t* __restrict__ mask,
                                            const Grid& g, uint32_t R, uint32_t b, uint32_t lane, uint32_t& id,
                                            bool& alive) {
  const uint32_t by = b / g.BW, bx = b - by * g.BW;
  const uint32_t x = bx * g.d + lane % g.d, y = by * g.d + lane / g.d;
  const bool in = lane < g.dd && x < g.W && y < g.H;
  const uint32_t p = in ? y * g.W + x : 0u;
  id = in ? reg[p] : kNoId;
  if (id >= R) id = kNoId;
  alive = in && !(mask && mask[p] != 0);
}

}  // namespace dq
