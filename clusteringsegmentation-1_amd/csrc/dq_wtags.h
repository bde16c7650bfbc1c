// dq_wtags.h -- the tag histogram of every capture window and the inside /
// outside votes of a window's quant (dq_wtags.hip): the launchers behind
// dq_hip_window_tags_dev and dq_hip_window_votes_dev (include/dq_hip.h, "window
// tags"; DESIGN.md 5a''''''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

// ---- tags ------------------------------------------------------------------------
// The call runs the windows stage (dq_windows.h) up to the pair positions and
// works on its scratch: the pairs (block b, member id r), block-major.
struct WtagsArgs {
  const uint32_t* regions;     // width * height region ids
  uint32_t width, height, nregions, block;
  const uint8_t* mask;         // optional
  uint32_t nblocks;            // of the grid
  const uint32_t* pairbase;    // nblocks + 1: the first pair of a block
  const uint32_t* pair_id;     // npairs: the member id of a pair (a copy: the walk overwrites the windows stage's)
  const uint32_t* pair_pos;    // npairs: the list position of a pair's first pixel (after the walk)
  const uint32_t* offsets;     // nregions + 1: the windows call's
  uint32_t npairs, total;      // P, M
  uint32_t* live;              // wtags_live_bytes(nblocks) bytes, owned by the call
  uint32_t* table;             // wtags_table_bytes(Q, M, nregions) bytes, owned by the call
  // outputs (each may be NULL but rows)
  uint32_t *rows, *ids, *counts, *first, *inside, *best, *best_count;
};

// The call has three parts with a small read-back after the first two:
//   launch_wtags_count    per block the distinct ids with a surviving pixel, live(b);
//                         Q = the sum over the pairs of live(block of the pair); needs
//                         pairbase alone, so it follows launch_windows_blocks directly
//   (the host reads Q with P and T, decides -3 and, once M is known, allocates the table)
//   launch_wtags_fill     a contribution per (pair (b, r), id s alive in b): its pixels
//                         added and its first position min-ed into the entry (r, s) of
//                         a hash table; then per entry one bit at its first position,
//                         the inside count and the best other id; the ranks of the bits
//   (the host reads E and decides E <= cap)
//   launch_wtags_rows     rows[r] = the rank at offsets[r]; inside, best, best_count
//   launch_wtags_entries  entry (r, s) at the rank of its bit

// 4 B per block, 4 B per 1024 blocks and 4 B.
size_t wtags_live_bytes(uint32_t nblocks);
// 16 B per slot, slots = 2 Q (>= 1024, < 2^32); 8 B per 32 list entries
// (a bit per list position and the rank of every word of them) + 4 B per 32768 + 24 B;
// 12 B per region (the inside count, the best other id with its count).
size_t wtags_table_bytes(uint32_t ncontribs, uint32_t total, uint32_t nregions);

void launch_wtags_count(const WtagsArgs& a, hipStream_t stream);
const uint32_t* wtags_contribs_word(const WtagsArgs& a);   // Q (saturates at 2^32 - 1)
void launch_wtags_fill(const WtagsArgs& a, uint32_t ncontribs, hipStream_t stream);
const uint32_t* wtags_entries_word(const WtagsArgs& a, uint32_t ncontribs);   // E
void launch_wtags_rows(const WtagsArgs& a, uint32_t ncontribs, hipStream_t stream);
void launch_wtags_entries(const WtagsArgs& a, uint32_t ncontribs, uint32_t nentries, hipStream_t stream);

// ---- votes -----------------------------------------------------------------------
constexpr uint32_t kVotesMaxK = 256;      // the reference asserts <= 256 (ClusteringSegmentation.cpp:1962)
constexpr uint32_t kVotesSegment = 2048;  // list entries of one job (a wave's share of a list)

struct WvotesArgs {
  const uint32_t* regions;   // n region ids
  uint32_t n, nregions;
  const uint32_t *offsets, *index, *mapped;   // the windows call's offsets and index, the pipeline's mapped colours
  uint32_t total, k;
  const uint32_t *cts, *k_outs;   // device copies: nregions * k, nregions
  uint32_t* jobs;            // wvotes_jobs_bytes(nregions) bytes, owned by the call
  uint32_t *votes, *best;    // nregions * 2 * k, nregions * 2
};

// 4 B per region (the first job of a region), 4 B per 1024 regions and 16 B (the misses).
size_t wvotes_jobs_bytes(uint32_t nregions);
void launch_wvotes(const WvotesArgs& a, hipStream_t stream);
const unsigned long long* wvotes_misses_word(const WvotesArgs& a);

}  // namespace dq
