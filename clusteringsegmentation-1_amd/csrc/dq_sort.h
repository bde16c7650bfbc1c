// dq_sort.h -- the stable LSD radix sort of (u32 key, u32 value) pairs the
// graph stages share (dq_contain.hip), beside dq_scan.h: 8-bit digits, only
// over the key bits in use.  One pass over a digit is
//   count    per tile of 1024 pairs the pairs of every digit, digit-major:
//            counts[digit * ntiles + tile]
//   scan     dq_scan.h's exclusive prefix sum over those 256 * ntiles words:
//            where a tile's pairs of a digit begin in the output
//   scatter  a tile again: its pairs in order, 256 at a time; a pair's rank
//            among the equal digits of its wave from wave64 ballots (eight, one
//            per digit bit), the waves and rounds before it from 256 running
//            counts in LDS; out[begin + rank] = pair
// Pairs with equal digits keep their order in every pass, so the sort is
// stable and its result does not depend on scheduling: no atomic decides a
// position.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dq_scan.h"

namespace dq {
namespace sort {

constexpr uint32_t kTile = 1024;
constexpr int kThreads = 256;
constexpr uint32_t kRounds = kTile / kThreads;
constexpr uint32_t kDigitBits = 8;
constexpr uint32_t kDigits = 1u << kDigitBits;
static_assert(kDigits == (uint32_t)kThreads, "one running count per thread");

inline uint32_t tiles_of(uint32_t n) { return (uint32_t)(((uint64_t)n + kTile - 1) / kTile); }
inline uint32_t passes_of(uint32_t key_bits) { return key_bits == 0 ? 1u : (key_bits + kDigitBits - 1) / kDigitBits; }
inline uint32_t bits_of(uint32_t v) { return v == 0 ? 0u : 32u - (uint32_t)__builtin_clz(v); }

// The words of the counts and of their scan's sums, for n pairs.
inline size_t counts_words(uint32_t n) { return (size_t)kDigits * tiles_of(n); }
inline size_t sums_words(uint32_t n) { return (size_t)scan::chunks_of((uint32_t)counts_words(n)) + 1; }

// A Source is a small struct with `__device__ uint32_t key(uint32_t i) const`
// and `__device__ uint32_t value(uint32_t i) const`: pair i < n of the input.
struct Pairs {
  const uint32_t* k;
  const uint32_t* v;
  __device__ uint32_t key(uint32_t i) const { return k[i]; }
  __device__ uint32_t value(uint32_t i) const { return v[i]; }
};

template <class Source>
__global__ __launch_bounds__(kThreads) void sort_count_kernel(Source src, uint32_t n, uint32_t shift,
                                                             uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[kDigits];
  hist[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kRounds; ++k) {
    const uint32_t i = blockIdx.x * kTile + k * kThreads + threadIdx.x;
    if (i < n) atomicAdd(&hist[(src.key(i) >> shift) & (kDigits - 1)], 1u);
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

template <class Source>
__global__ __launch_bounds__(kThreads) void sort_scatter_kernel(Source src, uint32_t n, uint32_t shift,
                                                               const uint32_t* __restrict__ begins,
                                                               uint32_t* __restrict__ out_keys,
                                                               uint32_t* __restrict__ out_values) {
  __shared__ uint32_t running[kDigits];              // where the tile's next pair of a digit goes
  __shared__ uint32_t wave_count[kThreads / 64][kDigits];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  running[threadIdx.x] = begins[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
#pragma unroll
  for (uint32_t w = 0; w < kThreads / 64; ++w) wave_count[w][threadIdx.x] = 0;
  __syncthreads();
#pragma unroll 1
  for (uint32_t k = 0; k < kRounds; ++k) {
    const uint32_t i = blockIdx.x * kTile + k * kThreads + threadIdx.x;
    const bool live = i < n;
    const uint32_t key = live ? src.key(i) : 0u, value = live ? src.value(i) : 0u;
    const uint32_t digit = (key >> shift) & (kDigits - 1);
    // the lanes of this wave with the same digit (dead lanes match nobody)
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (uint32_t b = 0; b < kDigitBits; ++b) {
      const bool bit = (digit >> b) & 1u;
      const unsigned long long set = __ballot(bit);
      peers &= bit ? set : ~set;
    }
    const uint32_t before = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (live && before == 0) wave_count[wave][digit] = (uint32_t)__popcll(peers);   // (one lane per digit and wave)
    __syncthreads();
    uint32_t at = 0;
    if (live) {
      at = running[digit] + before;
      for (uint32_t w = 0; w < wave; ++w) at += wave_count[w][digit];
    }
    __syncthreads();
    {
      uint32_t add = 0;
#pragma unroll
      for (uint32_t w = 0; w < kThreads / 64; ++w) {
        add += wave_count[w][threadIdx.x];
        wave_count[w][threadIdx.x] = 0;
      }
      running[threadIdx.x] += add;
    }
    __syncthreads();
    if (live && at < n) {   // (at < n by construction: the bound keeps a broken count inside the arrays)
      if (out_keys) out_keys[at] = key;
      out_values[at] = value;
    }
  }
}

// One pass: the pairs of src in the order of the digit at `shift`, equal digits
// in their order in src.  counts: counts_words(n), sums: sums_words(n) words.
template <class Source>
void launch_pass(const Source& src, uint32_t n, uint32_t shift, uint32_t* out_keys, uint32_t* out_values,
                 uint32_t* counts, uint32_t* sums, hipStream_t st) {
  const uint32_t ntiles = tiles_of(n);
  sort_count_kernel<Source><<<ntiles, kThreads, 0, st>>>(src, n, shift, counts);
  scan::launch(scan::Words{counts}, counts, (uint32_t)counts_words(n), sums, st);
  sort_scatter_kernel<Source><<<ntiles, kThreads, 0, st>>>(src, n, shift, counts, out_keys, out_values);
}

// The buffers of a sort: two key and two value arrays of n words (pass p reads
// [p & 1] and writes the other; the last pass writes its values to `dest`
// and no keys), the counts and the sums.
struct Buffers {
  uint32_t* keys[2];
  uint32_t* values[2];
  uint32_t* counts;
  uint32_t* sums;
};

inline size_t buffer_words(uint32_t n) { return 4 * (size_t)n + counts_words(n) + sums_words(n); }

inline Buffers carve(uint32_t* p, uint32_t n) {
  Buffers b;
  b.keys[0] = p;
  b.keys[1] = p + n;
  b.values[0] = p + 2 * (size_t)n;
  b.values[1] = p + 3 * (size_t)n;
  b.counts = p + 4 * (size_t)n;
  b.sums = b.counts + counts_words(n);
  return b;
}

// dest[0 .. n) = the values of src in increasing order of the low key_bits
// bits of their keys, equal keys in their order in src.
template <class Source>
void launch(const Source& src, uint32_t n, uint32_t key_bits, uint32_t* dest, const Buffers& b, hipStream_t st) {
  const uint32_t passes = passes_of(key_bits);
  for (uint32_t p = 0; p < passes; ++p) {
    const bool last = p + 1 == passes;
    uint32_t* ok = last ? nullptr : b.keys[(p + 1) & 1u];
    uint32_t* ov = last ? dest : b.values[(p + 1) & 1u];
    if (p == 0) launch_pass(src, n, 0u, ok, ov, b.counts, b.sums, st);
    else launch_pass(Pairs{b.keys[p & 1u], b.values[p & 1u]}, n, p * kDigitBits, ok, ov, b.counts, b.sums, st);
  }
}

}  // namespace sort
}  // namespace dq
