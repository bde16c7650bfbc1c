// dq_regions.h -- connected regions of a label map (dq_regions.hip): the
// launcher behind dq_hip_label_regions_dev (include/dq_hip.h, "connected
// regions"; DESIGN.md 5a'').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

// The tile of the tile pass: kRegionTile x kRegionTile pixels per workgroup
// (DQ_HIP_REGION_TILE in include/dq_hip.h is the same number).
constexpr uint32_t kRegionTile = 64;
// Pixels per workgroup of the linear passes (flatten + count, number, assign)
// = pixels per entry of the root-count scan.
constexpr uint32_t kRegionChunk = 1024;

struct RegionArgs {
  const void* labels;      // width * height labels of label_bytes each
  int label_bytes;         // 1, 2, 4
  uint32_t width, height;  // <= 65535 each, width * height <= 2^31 - 1
  int connectivity;        // 4, 8
  uint32_t* regions;       // out: width * height region ids
  uint32_t stats_cap;      // regions with id >= stats_cap are left out of the stats
  uint32_t* area;          // optional: stats_cap
  uint32_t* bbox;          // optional: stats_cap * 4 (x0, y0, x1, y1, inclusive)
  uint32_t* first;         // optional: stats_cap
  uint32_t* label;         // optional: stats_cap
  const uint32_t* pixels;  // optional: the packed 0x00RRGGBB frame
  unsigned long long* sums;  // optional (needs pixels): stats_cap * 3 (R, G, B)
  uint32_t* scratch;       // region_scratch_words(width, height) words, owned by the call
};

// parent[] (one word per pixel) + the root counts of the chunks + the total.
size_t region_scratch_words(uint32_t width, uint32_t height);
// Enqueues every pass on `stream`; the region count is then the word
// region_count_word(a) (device memory inside the scratch).
void launch_label_regions(const RegionArgs& a, hipStream_t stream);
const uint32_t* region_count_word(const RegionArgs& a);

}  // namespace dq
