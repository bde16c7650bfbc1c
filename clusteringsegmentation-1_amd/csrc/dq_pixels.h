// dq_pixels.h -- the pixel lists of a region map (dq_pixels.hip): the launchers
// behind dq_hip_region_pixels_dev and dq_hip_scatter_coords_dev
// (include/dq_hip.h, "pixel lists"; DESIGN.md 5a''''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

struct PixelsArgs {
  const uint32_t* regions;   // width * height region ids, each < nregions
  uint32_t width, height;    // <= 65535 each, width * height <= 2^31 - 1
  uint32_t nregions;         // 1 .. 2^31 - 1
  uint32_t* offsets;         // nregions + 1
  uint32_t* coords;          // optional: width * height Coord words x | y << 16
  uint32_t* index;           // optional: width * height pixel indexes y * width + x
  const uint32_t* pixels;    // optional: the frame
  uint32_t* colors;          // optional (needs pixels): width * height words of the frame
  uint32_t* rows;            // pixels_rows_bytes(nregions) bytes, owned by the call
  uint32_t* table;           // pixels_table_bytes(T) bytes, owned by the call
};

// The call has two halves with one small read-back between them, because the
// table is sized from T, the sum over the ids present of the rows they span:
//   launch_pixels_rows      first and last row per id, their prefix sums,
//                           T -> the word pixels_total_word(a) (saturates at 2^32 - 1)
//   (the host reads it, returns -2 when T > n and allocates the table)
//   launch_pixels_lists     run lengths per (id, row), their prefix sums, the
//                           offsets, and the row walk that writes the lists

// 8 B per region, 4 B per 1024 regions and 4 B.
size_t pixels_rows_bytes(uint32_t nregions);
// 4 B per table entry (T <= n of them; one for T = 0), 4 B per 1024 entries and 4 B.
size_t pixels_table_bytes(uint32_t total);

void launch_pixels_rows(const PixelsArgs& a, hipStream_t stream);
void launch_pixels_lists(const PixelsArgs& a, uint32_t total, hipStream_t stream);
const uint32_t* pixels_total_word(const PixelsArgs& a);

// offsets[r] = table[rowbase[r]] for r < nregions with rowbase[r] < nrows, else `total`
// (nregions + 1 offsets): the offsets of this stage's lists and of the capture windows'
// (dq_windows.hip), whose tables have the same shape.
void launch_list_offsets(uint32_t nregions, uint32_t nrows, uint32_t total, const uint32_t* rowbase,
                         const uint32_t* table, uint32_t* offsets, hipStream_t stream);

// frame[(c >> 16) * width + (c & 0xFFFF)] = values[i] for the n Coord words c.
void launch_scatter_coords(const uint32_t* values, const uint32_t* coords, uint32_t n, uint32_t width,
                           uint32_t* frame, hipStream_t stream);

}  // namespace dq
