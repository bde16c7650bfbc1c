// dq_scan.h -- the saturating exclusive prefix sum every region-map stage
// uses: three kernels over chunks of 1024 values (sums per chunk, one workgroup
// over the sums, apply).  The list and graph stages (dq_pixels.hip,
// dq_windows.hip, dq_wtags.hip, dq_contain.hip, dq_sort.h) run all three
// through launch(); dq_regions.hip, dq_adjacency.hip and dq_merge.hip write
// their chunk sums in a pass of their own, run scan_top_kernel over them and
// apply the offsets in their next pass, with block_excl_scan inside the chunk.
// Every sum saturates at 2^32 - 1 (min(sum, 2^32 - 1) is associative), so a
// total too large for a word is seen however large it is; where the true total
// fits a word the saturating sum is the sum.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dq_stage.h"

namespace dq {
namespace scan {

using dq::kChunk;     // values per entry of the top scan
using dq::kThreads;

__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) {
  const uint32_t s = a + b;
  return s < a ? 0xFFFFFFFFu : s;
}

// Exclusive prefix sum of v over the workgroup's threads (NW waves) and the
// workgroup's total, both saturating.  Every thread of the workgroup calls it.
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc = sat_add(inc, t);
  }
  uint32_t excl = __shfl_up(inc, 1);
  if (lane == 0) excl = 0;
  __syncthreads();   // (wsum may still be read from the previous call)
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)NW; ++w) {
    const uint32_t s = wsum[w];
    if (w < wave) off = sat_add(off, s);
    tot = sat_add(tot, s);
  }
  total = tot;
  return sat_add(off, excl);
}

// A Value is a small struct with `__device__ uint32_t operator()(uint32_t i)
// const`: element i < n of the sequence.  It may read out[i]: the apply kernel
// reads element i in the thread that then writes out[i].
template <class Value>
__global__ __launch_bounds__(kThreads) void scan_sums_kernel(Value value, uint32_t n, uint32_t* __restrict__ sums) {
  __shared__ uint32_t wsum[kThreads / 64];
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    c = sat_add(c, i < n ? value(i) : 0u);
  }
  uint32_t total;
  block_excl_scan<kThreads / 64>(c, wsum, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. nchunks) -> their exclusive prefix sums, sums[nchunks] = the total.
static __global__ __launch_bounds__(1024) void scan_top_kernel(uint32_t* sums, uint32_t nchunks) {
  __shared__ uint32_t wsum[16];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nchunks; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nchunks ? sums[i] : 0u;
    uint32_t total;
    const uint32_t excl = block_excl_scan<16>(v, wsum, total);
    if (i < nchunks) sums[i] = sat_add(carry, excl);
    carry = sat_add(carry, total);
  }
  if (threadIdx.x == 0) sums[nchunks] = carry;
}

template <class Value>
__global__ __launch_bounds__(kThreads) void scan_apply_kernel(Value value, uint32_t* out, uint32_t n,
                                                             const uint32_t* __restrict__ sums) {
  __shared__ uint32_t wsum[kThreads / 64];
  uint32_t carry = sums[blockIdx.x];
#pragma unroll 1
  for (uint32_t k = 0; k < kChunk / kThreads; ++k) {
    const uint32_t i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    const uint32_t val = i < n ? value(i) : 0u;   // (read by the thread that then writes out[i])
    uint32_t total;
    const uint32_t excl = block_excl_scan<kThreads / 64>(val, wsum, total);
    if (i < n) out[i] = sat_add(carry, excl);
    carry = sat_add(carry, total);
  }
}

inline uint32_t chunks_of(uint32_t n) { return (n + kChunk - 1) / kChunk; }

// out[i] = value(0) + .. + value(i - 1) for i < n (out may be what value reads:
// in place); sums: chunks_of(n) + 1 words, the last one the total.
template <class Value>
void launch(const Value& value, uint32_t* out, uint32_t n, uint32_t* sums, hipStream_t st) {
  const uint32_t nchunks = chunks_of(n);
  scan_sums_kernel<Value><<<nchunks, kThreads, 0, st>>>(value, n, sums);
  scan_top_kernel<<<1, 1024, 0, st>>>(sums, nchunks);
  scan_apply_kernel<Value><<<nchunks, kThreads, 0, st>>>(value, out, n, sums);
}

// the words of a sequence as they are
struct Words {
  const uint32_t* v;
  __device__ uint32_t operator()(uint32_t i) const { return v[i]; }
};

}  // namespace scan
}  // namespace dq
