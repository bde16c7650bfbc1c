// dq_skeleton.h -- the skeletons of all regions of a region map by Guo-Hall
// two-subiteration thinning (dq_skeleton.hip): the launchers behind
// dq_hip_region_skeleton_dev (include/dq_hip.h, "region skeleton"; DESIGN.md
// 5a'''''''''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

// The iterations one thinning launch runs on a tile held in LDS.  A subiteration
// spoils one more ring of the tile's halo, so the halo is 2 * kSkeletonIters pixels.
constexpr uint32_t kSkeletonIters = 16;
// The tile's core, the part a launch writes: words of 64 pixels along x, rows along y.
constexpr uint32_t kSkeletonTileWords = 6;
constexpr uint32_t kSkeletonTileRows = 64;
// The most iterations of a call (`when` is u16), and so the most launches.
constexpr uint32_t kSkeletonMaxIters = 65535;
constexpr uint32_t kSkeletonMaxLaunches = (kSkeletonMaxIters + kSkeletonIters - 1) / kSkeletonIters;

struct SkeletonArgs {
  const uint32_t* regions;   // width * height ids; an id >= nregions is background (may be `skeled`:
                             // read by the planes pass, then per pixel before the pixel's word is written)
  uint32_t width, height;    // <= 65535 each, width * height <= 2^31 - 1
  uint32_t nregions;
  uint32_t max_iters;        // 0: until stable
  uint8_t* skel;             // optional: width * height
  uint32_t* skeled;          // optional: width * height, the id or 0xFFFFFFFF
  uint16_t* when;            // width * height; required when `thick` is given (the entry points put scratch there)
  uint32_t* skel_area;       // optional: nregions
  uint32_t* thick;           // optional: nregions
  void* scratch;             // skeleton_scratch_bytes(width, height), owned by the call
};

// Six bit planes of one bit per pixel, rows padded to 64 pixels (two alive
// planes and the sameness towards E, SE, S and SW), two words per tile (did it
// delete in the last launch, in this one), one word per possible launch (the last
// iteration of the launch that deleted) and the pixels kept.  Nothing per region.
size_t skeleton_scratch_bytes(uint32_t width, uint32_t height);

// Two launches: the words of the call cleared; one pass over the map for the
// planes (and `when` cleared).
void launch_skeleton_planes(const SkeletonArgs& a, hipStream_t stream);
// Launch number `launch` (from 0) of the thinning: iterations first + 1 .. first + iters, iters <=
// kSkeletonIters and first = launch * kSkeletonIters.  It reads the alive plane launch % 2 and writes
// the other.
void launch_skeleton_thin(const SkeletonArgs& a, uint32_t launch, uint32_t iters, hipStream_t stream);
// Word `launch` (device memory): the highest iteration of that launch, counted from 1 within it, that
// deleted a pixel; 0 when none did.
const uint32_t* skeleton_last_words(const SkeletonArgs& a);
// One pass after `launches` thinning launches: skel, skeled, skel_area, thick and the pixels kept.
void launch_skeleton_outputs(const SkeletonArgs& a, uint32_t launches, hipStream_t stream);
const uint32_t* skeleton_kept_word(const SkeletonArgs& a);

}  // namespace dq
