// dq_merge.h -- merging regions over their adjacency graph (dq_merge.hip): the
// launchers behind dq_hip_merge_regions_dev (include/dq_hip.h, "region merge";
// DESIGN.md 5a'''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

struct MergeArgs {
  const uint32_t* regions;   // n region ids, each < nregions
  uint32_t n, nregions;      // n <= 2^31 - 1, 1 <= nregions <= n
  const uint32_t* area;      // nregions (> 0 each)
  const uint32_t* first;     // nregions (distinct, < n)
  const unsigned long long* sums;   // nregions * 3 (R, G, B)
  const uint32_t* bbox;      // optional: nregions * 4 (x0, y0, x1, y1, inclusive)
  uint32_t nedges;
  const uint32_t* edges;     // nedges * 2 ids (any order, duplicates allowed)
  uint32_t min_area, max_dist;
  uint32_t* out_regions;     // n new ids (may be `regions`)
  uint32_t* remap;           // optional: nregions new ids
  uint32_t stats_cap;        // new regions with id >= stats_cap are left out of the stats
  uint32_t* out_area;        // optional: stats_cap
  uint32_t* out_bbox;        // optional (needs bbox): stats_cap * 4
  uint32_t* out_first;       // optional: stats_cap
  unsigned long long* out_sums;   // optional: stats_cap * 3
  void* scratch;             // merge_scratch_bytes(...) bytes, owned by the call
};

// The call is a loop on the host with one 4-byte read-back per round:
//   launch_merge_init
//   repeat: launch_merge_choose   links of the round -> the word merge_links_word(a)
//           (the host reads it; 0 links: the round does not count, the loop ends)
//           launch_merge_fold
//   launch_merge_finish           R' -> the word merge_count_word(a)
// With no edge or min_area == 0 the loop body is never launched.

// Per region 60 B (76 B with bbox, 4 B more without remap), one bit per pixel,
// 4 B per 1024 pixels, and two words.
size_t merge_scratch_bytes(uint32_t n, uint32_t nregions, bool with_bbox, bool with_remap);

void launch_merge_init(const MergeArgs& a, hipStream_t stream);
void launch_merge_choose(const MergeArgs& a, hipStream_t stream);
void launch_merge_fold(const MergeArgs& a, hipStream_t stream);
// (the status of the bitmap fill; nothing after a failed fill is launched)
hipError_t launch_merge_finish(const MergeArgs& a, hipStream_t stream);
const uint32_t* merge_links_word(const MergeArgs& a);
const uint32_t* merge_count_word(const MergeArgs& a);

}  // namespace dq
