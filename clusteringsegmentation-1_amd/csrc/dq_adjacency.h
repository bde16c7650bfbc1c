// dq_adjacency.h -- region adjacency graph of a region map (dq_adjacency.hip):
// the launcher behind dq_hip_region_adjacency_dev (include/dq_hip.h, "region
// adjacency"; DESIGN.md 5a''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

struct AdjacencyArgs {
  const uint32_t* regions;   // width * height region ids (any id map)
  uint32_t width, height;    // <= 65535 each, width * height <= 2^30
  int connectivity;          // 4, 8
  uint32_t edge_cap;         // edges with index >= edge_cap are left out of the edge arrays
  uint32_t* edges;           // optional: edge_cap * 2 (a < b)
  uint32_t* border;          // optional: edge_cap
  uint32_t* contact;         // optional: edge_cap * 2 (p < q)
  const uint32_t* pixels;    // optional: the packed 0x00RRGGBB frame
  unsigned long long* step;  // optional (needs pixels): edge_cap
  uint32_t* degree;          // optional: one word per region id, zeroed by the caller
  uint32_t* counts;          // adjacency_count_words(width, height) words, owned by the call
  void* table;               // adjacency_scratch_bytes(heads, step != nullptr) bytes, owned by the call
};

// The call has two halves with one small read-back between them, because the
// table is sized from the heads the first half counts, never from 4 * n:
//   launch_adjacency_count   heads -> the word adjacency_heads_word(a)
//   (the host reads it and allocates the table)
//   launch_adjacency_build   edges -> the arrays, E -> adjacency_edges_word(a)
// With 0 heads there is no edge and the second half is not launched.

// One count per chunk of 1024 pixels (heads, then edges) + their total.
size_t adjacency_count_words(uint32_t width, uint32_t height);
// Slots of the table: the power of two >= 2 * heads, at least 1024.
uint64_t adjacency_table_slots(uint32_t heads);
// The table: per slot an 8-B key, a 4-B first contact, a 4-B border and, with
// step, an 8-B step sum: 16 or 24 B times adjacency_table_slots(heads).
size_t adjacency_scratch_bytes(uint32_t heads, bool with_step);

void launch_adjacency_count(const AdjacencyArgs& a, hipStream_t stream);
void launch_adjacency_build(const AdjacencyArgs& a, uint32_t heads, hipStream_t stream);
const uint32_t* adjacency_heads_word(const AdjacencyArgs& a);
const uint32_t* adjacency_edges_word(const AdjacencyArgs& a);

}  // namespace dq
