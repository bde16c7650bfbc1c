// dq_contour.h -- the contours of all regions of a region map by border
// following as list ranking (dq_contour.hip): the launchers behind
// dq_hip_region_contours_dev (include/dq_hip.h, "region contours"; DESIGN.md
// 5a''''''''''').
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dq {

// A chain of fewer than 2^32 states is resolved after 32 pointer-jumping rounds;
// the round after the last one needed is the one that sees nothing left to do.
constexpr uint32_t kContourMaxRounds = 33;
// The most states a call can number (a state is a word; 0xFFFFFFFF is "none").
constexpr uint32_t kContourMaxStates = 0xFFFFFFFEu;

struct ContourArgs {
  const uint32_t* regions;   // width * height ids; an id >= nregions is background
  uint32_t width, height;    // <= 65535 each, width * height <= 2^31 - 1
  uint32_t nregions;
  int orientation;           // 0: as followed; 1: the list reversed
  unsigned long long point_cap;   // the entries of room in points and codes
  uint32_t* offsets;         // nregions + 1 (the entry points put scratch there when the caller has none)
  uint32_t* points;          // optional: point_cap Coord words
  uint8_t* codes;            // optional: point_cap
  uint32_t* len;             // nregions (the entry points put scratch there when the caller has none)
  uint8_t* visits;           // optional: width * height
  void* scratch;             // contour_scratch_bytes(width, height, nregions), owned by the call
  void* links;               // contour_links_bytes(states), owned by the call; NULL when there is no state
};

// Per pixel its neighbour byte and the number of its first state (5 B), per
// region its first pixel, its start state and the state after it (12 B), the
// sums of the scans and one word per round.
size_t contour_scratch_bytes(uint32_t width, uint32_t height, uint32_t nregions);
// Two buffers of one (next : 32 | distance : 32) word per state.
size_t contour_links_bytes(uint32_t states);

// Five launches: the words of the call cleared; one pass over the map for the
// neighbour bytes and the first pixels; the scan that numbers the states.
void launch_contour_mark(const ContourArgs& a, hipStream_t stream);
// The number of states S (device memory; 0xFFFFFFFF: more than kContourMaxStates).
const uint32_t* contour_states_word(const ContourArgs& a);
// Two launches: per region the start state, the state after it and the lengths
// 0 and 1; per border pixel the successor of each of its states (states > 0 only).
void launch_contour_links(const ContourArgs& a, uint32_t states, hipStream_t stream);
// Round `round` (from 0) of the pointer jumping: reads buffer round % 2, writes the other.
void launch_contour_jump(const ContourArgs& a, uint32_t states, uint32_t round, hipStream_t stream);
// Word `round` (device memory): non-zero when a start's chain was not yet
// resolved in the buffer that round read.
const uint32_t* contour_round_words(const ContourArgs& a);
// Three launches after `rounds` rounds: len, and the sums of the scan over it.
void launch_contour_lengths(const ContourArgs& a, uint32_t states, uint32_t rounds, hipStream_t stream);
// M, saturating at 2^32 - 1 (device memory).
const uint32_t* contour_total_word(const ContourArgs& a);
// Two launches and a word copied: offsets; points, codes (lists: there is room for all M) and visits.
hipError_t launch_contour_emit(const ContourArgs& a, uint32_t states, uint32_t rounds, bool lists, hipStream_t stream);

}  // namespace dq
