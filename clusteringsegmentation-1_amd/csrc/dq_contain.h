// dq_contain.h -- the containment tree of a region map (dq_contain.hip): the
// launchers behind dq_hip_region_containment_dev and dq_hip_regions_by_size_dev
// (include/dq_hip.h, "containment tree"; DESIGN.md 5a'''''''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

struct ContainArgs {
  const uint32_t* regions;   // width * height ids; an id >= nregions is passed over
  uint32_t width, height, nregions;
  const uint32_t* area;      // nregions
  uint32_t nedges;
  const uint32_t* edges;     // nedges * 2 ids (any order, duplicates allowed)
  void* scratch;             // contain_scratch_bytes(nregions) bytes, owned by the call
};

// The results, all in the scratch (the caller copies out what it wants).
struct ContainResults {
  const uint32_t* depth;           // R
  const uint32_t* parent;          // R
  const uint32_t* sequence;        // R: [roots | children grouped by parent | orphans], each group in size order
  const uint32_t* child_offsets;   // R + 1
  const uint32_t* subtree;         // R
  const unsigned long long* enclosed;   // R
  const uint32_t* order;           // reached
  const uint32_t* pos;             // R
};

// The call is a loop on the host with one 8-byte read-back per level:
//   launch_contain_roots          the roots -> word 0 of contain_counters(a), the OR of the areas -> word 1
//   L = 1, 2, ..: launch_contain_level(a, L)   the regions reached so far -> word 0
//           (the host reads it; no more than before: L - 1 was the deepest level, the loop ends)
//   launch_contain_tree(a, levels, nroots, reached, area_bits)   everything else, no read-back
// 68 B per region plus the sort's digit counts (1 KiB per 1024 regions), nothing per edge.
size_t contain_scratch_bytes(uint32_t nregions);
const uint32_t* contain_counters(const ContainArgs& a);
ContainResults contain_results(const ContainArgs& a);

void launch_contain_roots(const ContainArgs& a, hipStream_t stream);
void launch_contain_level(const ContainArgs& a, uint32_t level, hipStream_t stream);
void launch_contain_tree(const ContainArgs& a, uint32_t levels, uint32_t nroots, uint32_t reached, uint32_t area_bits,
                         hipStream_t stream);

// The key bits the size sort runs over, from the OR of the areas.
inline uint32_t sort_key_bits(uint32_t or_of_areas) {
  return or_of_areas == 0 ? 0u : 32u - (uint32_t)__builtin_clz(or_of_areas);
}

// The size order alone: order[i] = the id at position i of (area decreasing,
// id increasing), rank[id] = its position; either may be NULL.
//   launch_size_bits      the OR of the areas -> the word size_bits_word(scratch) (the host reads it)
//   launch_size_order     the sort over bits_of(that word) key bits
// 20 B per region plus the sort's digit counts.
size_t size_scratch_bytes(uint32_t nregions);
const uint32_t* size_bits_word(const void* scratch);
void launch_size_bits(uint32_t nregions, const uint32_t* area, void* scratch, hipStream_t stream);
void launch_size_order(uint32_t nregions, const uint32_t* area, uint32_t area_bits, uint32_t* order, uint32_t* rank,
                       void* scratch, hipStream_t stream);

}  // namespace dq
