// dq_stage.h -- the device idioms the region-map stages share (dq_regions.hip,
// dq_adjacency.hip, dq_merge.hip, dq_pixels.hip, dq_windows.hip, dq_wtags.hip,
// dq_contain.hip, dq_distance.hip, dq_skeleton.hip, dq_contour.hip): the workgroup and chunk sizes, runs of
// equal keys along a wave, the workgroup's LDS slot cache and groups of equal ids in a wave.  Free
// functions of a few lines each; beside it dq_scan.h (prefix sums) and
// dq_table.h (the 64-bit hash table).
// Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dq_regions.h"

namespace dq {

constexpr int kThreads = 256;
constexpr uint32_t kChunk = kRegionChunk;   // items per workgroup of a flat pass = items per entry of a top scan
static_assert(kChunk == 4 * kThreads, "four rounds of one item per thread");

constexpr uint32_t kNoId = 0xFFFFFFFFu;   // never a valid id: ids are < R <= 2^32 - 1 wherever a stage keeps one

__device__ __forceinline__ uint64_t global_thread() { return (uint64_t)blockIdx.x * kThreads + threadIdx.x; }
inline uint32_t blocks_for(uint64_t items) { return (uint32_t)((items + kThreads - 1) / kThreads); }

// ---- runs of equal keys along a wave ---------------------------------------------
// The lanes of a wave hold consecutive items; a run is a stretch of lanes the
// caller's head predicate does not cut.  Every lane of the wave calls these.
struct WaveRun {
  uint32_t start;   // the first lane of this lane's run
  bool tail;        // this lane is the last of its run
  __device__ uint32_t length(uint32_t lane) const { return lane - start + 1; }   // at the tail: the run's
};

// head: a run starts at this lane (lane 0 always starts one).
__device__ __forceinline__ WaveRun wave_run(bool head) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long heads = __ballot(head || lane == 0);
  WaveRun run;
  run.start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
  run.tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0;
  return run;
}

// The sum of v over the run's lanes up to this one (the tail lane holds the run's sum).
template <class T>
__device__ __forceinline__ T run_sum(T v, const WaveRun& run) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const T t = __shfl_up(v, d);
    if (lane >= run.start + d) v += t;
  }
  return v;
}

// The highest v over the run's lanes up to this one (the tail lane holds the run's).
__device__ __forceinline__ uint32_t run_max(uint32_t v, const WaveRun& run) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d);
    if (lane >= run.start + d) v = max(v, t);
  }
  return v;
}

// ---- the workgroup's LDS slot cache ----------------------------------------------
// A workgroup gathers what it adds to a key in LDS slots and flushes them once.
// true: the slot was free (`none`) or already the key's, and the caller adds
// into the slot's LDS words; false: another key has it, and the caller adds
// straight to global memory.  Integer adds, min and max: the same result either way.
template <class Key>
__device__ __forceinline__ bool slot_claim(Key* s_key, uint32_t slot, Key none, Key key) {
  const Key was = atomicCAS(&s_key[slot], none, key);
  return was == none || was == key;
}

// ---- groups of equal ids in a wave -----------------------------------------------
// The lanes of a wave with equal ids form a group, not only neighbours: A B A is
// one group of A.  A valid lane first claims the wave's LDS slot of its id: the
// lane that finds the slot free and is in no round below is alone with its id
// (any other lane of that id finds the slot taken and asks for a round); a lane
// that finds it taken, by its id or by another, asks for a round, and a round
// settles every lane of its id.  Which lane claims does not matter.  One round
// per id asked for: 1 to 3 on a smooth map, a few (the slot collisions) instead
// of 64 on a map of specks.  round(mine, group, l): this lane is in the round's
// group, the ballot of the group, the lane the round took its id from.
// slots: kWalkSlots words of this wave alone, all kNoId (and again afterwards).
constexpr uint32_t kWalkSlotBits = 9;   // 512 LDS slots per wave (64 ids: ~4 share a slot)
constexpr uint32_t kWalkSlots = 1u << kWalkSlotBits;

template <class Round>
__device__ __forceinline__ void wave_id_groups(uint32_t* slots, uint32_t id, bool valid, Round round) {
  const uint32_t s = (id * 2654435761u) >> (32 - kWalkSlotBits);
  bool ask = false;
  if (valid) ask = atomicCAS(&slots[s], kNoId, id) != kNoId;
  unsigned long long todo = __ballot(ask);
  __builtin_amdgcn_wave_barrier();
  if (valid) slots[s] = kNoId;   // (free again for the next chunk)
  __builtin_amdgcn_wave_barrier();
  while (todo) {   // (uniform: every round takes at least the lane it reads the id of)
    const int l = __ffsll(todo) - 1;
    const uint32_t key = __shfl(id, l);
    const bool mine = valid && id == key;
    const unsigned long long group = __ballot(mine);
    round(mine, group, l);
    todo &= ~group;
  }
}

}  // namespace dq
