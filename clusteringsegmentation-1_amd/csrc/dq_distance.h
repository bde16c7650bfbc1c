// dq_distance.h -- the L1 distance transform, the centres and the cores of a
// region map (dq_distance.hip): the launchers behind
// dq_hip_region_distance_dev and dq_hip_region_cores_dev (include/dq_hip.h,
// "region distance"; DESIGN.md 5a''''''''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

// The rows of a band of the column step: one word of head bits per (band, column).
constexpr uint32_t kDistanceBand = 32;

struct DistanceArgs {
  const uint32_t* regions;   // width * height ids; an id >= nregions is background
  uint32_t width, height;    // <= 65535 each, width * height <= 2^31 - 1
  uint32_t nregions;
  int rule;                  // 0: thresh = dmax; 1: the reference's 8-bit scale
  // Every array below is written; the entry points put scratch where the caller gave NULL.
  uint16_t* dist;            // width * height
  uint32_t* dmax;            // nregions
  uint32_t* bbox;            // nregions * 4 (x0, y0, x1, y1, inclusive)
  uint32_t* thresh;          // nregions
  uint32_t* count;           // nregions
  uint32_t* centre;          // nregions: x | y << 16, 0xFFFFFFFF for an id with no pixel
  void* scratch;             // distance_scratch_bytes(width, height, nregions), owned by the call
};

// The column step's distances (2 B per pixel), its head bits and carries (8 B
// per kDistanceBand pixels) and 32 B per region (the sums of the centre set, its last-row key, the
// centroid of a region whose centre is searched and the search key).
size_t distance_scratch_bytes(uint32_t width, uint32_t height, uint32_t nregions);
// Enqueues all eleven launches on `stream`; no read-back.
void launch_region_distance(const DistanceArgs& a, hipStream_t stream);

struct CoresArgs {
  const uint32_t* regions;     // width * height ids (may be `cored`: a pixel's id is read before it is written)
  uint32_t width, height, nregions;
  const uint32_t* component;   // width * height: launch_label_regions' ids of the map read as u32 labels
  const uint32_t* centre;      // nregions, from launch_region_distance
  uint8_t* core;               // optional: width * height
  uint32_t* cored;             // optional: width * height, the id or 0xFFFFFFFF
  uint32_t* core_area;         // nregions (scratch when the caller gave NULL)
  uint32_t* kept;              // one word: the pixels kept
};

// Two launches: core_area and the total cleared, then one pass over the map.
void launch_region_cores(const CoresArgs& a, hipStream_t stream);

}  // namespace dq
