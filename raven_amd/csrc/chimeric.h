// chimeric.h — raven::Pile::ClearChimericRegions(median) (RavenLib/src/pile.cc:189-228) and the UpdateValidRegion it
// ends with (pile.cc:144-157) for ONE pile, as __host__ __device__ code: the part of ResolveChimericSequences
// (construct.cc:250-314) that resolve.hip runs per pile, and the same functions behind the host program of the tests
// (tests/host/resolve_pile.cpp).
//
// A chimeric region is a (first, second) pair of cells, both inclusive.  A region that leaves the valid region
// [begin_, end_] is skipped and dropped; a region with a cell whose clamp(coverage * 1.82) is at most the global median
// is RESOLVED: the read is cut there; every other region stays with the pile.  The longest stretch between resolved
// regions (the first of equal length) becomes the valid region.  All arithmetic is the reference's: uint32 differences
// that may wrap, the product in double, the clamp to 65535.
//
// clamp(x * 1.82) does not decrease when x grows, so a region is resolved exactly when its SMALLEST cell passes the
// test: the device takes the minimum of a region with the whole wave (chimeric_cell_resolves on the minimum) and walks
// the pile's handful of regions on one lane (clear_chimeric_walk); the host build tests cell by cell in the reference's
// order (chimeric_region_resolved).
#pragma once

#include "common.h"
#include "slopes.h"

namespace rvn {

constexpr double kChimericQ = 1.82;
constexpr u32 kMinValidCells = 1260 >> 4;  // UpdateValidRegion: 1260 >> kPSS

struct ChimericOutcome {
  u32 begin, end;    // Pile::begin_ / end_ afterwards (cells)
  u32 n_unresolved;  // regions left in the pile's slots
  bool chimeric;     // set_is_chimeric() happened
  bool invalid;      // UpdateValidRegion made the pile invalid (begin / end are then the old ones)
};

// the test of is_chimeric_region on one cell (pile.cc:192)
__host__ __device__ inline bool chimeric_cell_resolves(u16 cell, u16 median) {
  return slope_clamp(static_cast<double>(cell) * kChimericQ) <= static_cast<double>(median);
}

// is_chimeric_region (pile.cc:190-197), cell by cell
__host__ __device__ inline bool chimeric_region_resolved(const u16* data, u32 first, u32 second, u16 median) {
  for (u32 i = first; i <= second; ++i)
    if (chimeric_cell_resolves(data[i], median)) return true;
  return false;
}

// pile.cc:199-225 and the test of UpdateValidRegion (:145): walks regions[0 .. 2 * n) in order, leaves the unresolved
// ones at the front of the same array, returns the new valid region.  resolved(k, first, second) is asked once for every
// region inside [begin_, end_].
template <typename Resolved>
__host__ __device__ inline ChimericOutcome clear_chimeric_walk(u32 begin_, u32 end_, u32* regions, u32 n, Resolved resolved) {
  u32 begin = 0, end = 0, last = begin_, kept = 0;
  for (u32 k = 0; k < n; ++k) {
    const u32 first = regions[2 * k], second = regions[2 * k + 1];
    if (begin_ > first || end_ < second) continue;
    if (resolved(k, first, second)) {
      if (first - last > end - begin) {
        begin = last;
        end = first;
      }
      last = second;
    } else {
      regions[2 * kept] = first;
      regions[2 * kept + 1] = second;
      ++kept;
    }
  }
  if (end_ - last > end - begin) {
    begin = last;
    end = end_;
  }
  ChimericOutcome out;
  out.chimeric = begin != begin_ || end != end_;
  out.n_unresolved = kept;
  out.invalid = begin >= end || end - begin < kMinValidCells;
  out.begin = out.invalid ? begin_ : begin;
  out.end = out.invalid ? end_ : end;
  return out;
}

// the stores of UpdateValidRegion (pile.cc:149-154) for a pile that stays valid: cells [begin_, begin) and [end, end_)
__host__ __device__ inline void chimeric_zero_outside(u16* data, u32 begin_, u32 end_, u32 begin, u32 end) {
  for (u32 i = begin_; i < begin; ++i) data[i] = 0;
  for (u32 i = end; i < end_; ++i) data[i] = 0;
}

// ClearChimericRegions(median) of one pile over its coverage
__host__ __device__ inline ChimericOutcome clear_chimeric_regions(u16* data, u32 begin_, u32 end_, u32* regions, u32 n, u16 median) {
  const ChimericOutcome out = clear_chimeric_walk(begin_, end_, regions, n, [&](u32, u32 first, u32 second) {
    return chimeric_region_resolved(data, first, second, median);
  });
  if (!out.invalid) chimeric_zero_outside(data, begin_, end_, out.begin, out.end);
  return out;
}

}  // namespace rvn
