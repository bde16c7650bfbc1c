// dq_table.h -- the 64-bit open-addressing table of the graph stages
// (dq_adjacency.hip: a key per edge; dq_wtags.hip: a key per (window, tag)):
// the hash and the two probes over the key array.  A stage keeps its own home
// slot (adjacency: the hash's low bits under a power-of-two mask; wtags: a
// 32-bit hash scaled to any slot count), its own payload arrays beside the keys
// and its own atomics on them.  Slot: the stage's slot index type (u64, u32).
// Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq {
namespace table {

constexpr unsigned long long kNoKey = ~0ull;   // a free slot; no stage's key equals it
constexpr uint64_t kMinTableSlots = 1024;      // (an empty call's table stays a table)

__device__ __forceinline__ unsigned long long mix(unsigned long long h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// The slot of `key`, claimed if the key was not there: linear probing from
// `home`.  Other workgroups (on other XCDs, behind other L2s) claim slots
// meanwhile: every read of a key during insertion is an agent-scope atomic.  A
// slot's key never changes once claimed, and at most half the slots are ever
// claimed, so the probe ends at the key or at a free slot this thread then
// claims.
template <class Slot>
__device__ __forceinline__ Slot table_claim(unsigned long long* keys, Slot nslots, Slot home,
                                            unsigned long long key) {
  Slot s = home;
  for (;;) {
    unsigned long long k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kNoKey) {
      k = atomicCAS(&keys[s], kNoKey, key);
      if (k == kNoKey) k = key;   // claimed
    }
    if (k == key) return s;
    s = s + 1 == nslots ? 0 : s + 1;
  }
}

// The slot of `key` in the finished table, or ~Slot(0): the key is not there (a
// free slot ends the probe).  Plain loads, and only because the insert kernel
// has ended.
template <class Slot>
__device__ __forceinline__ Slot table_find(const unsigned long long* __restrict__ keys, Slot nslots, Slot home,
                                           unsigned long long key) {
  Slot s = home;
  for (;;) {
    const unsigned long long k = keys[s];
    if (k == key) return s;
    if (k == kNoKey) return ~Slot(0);
    s = s + 1 == nslots ? 0 : s + 1;
  }
}

}  // namespace table
}  // namespace dq
