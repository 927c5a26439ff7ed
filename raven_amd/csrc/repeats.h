// repeats.h — raven::Pile::FindRepetitiveRegions(median) (RavenLib/src/pile.cc:230-317) and the per-overlap halves of
// Pile::UpdateRepetitiveRegions / CheckRepetitiveRegions (pile.cc:319-369) as __host__ __device__ code: the pieces of
// ResolveRepeatInducedOverlaps (construct.cc:493-559) that repeats.hip runs per pile and per overlap, and the same
// functions that tests/host/repeats_pile.cpp compiles for the host and runs through the whole loop on the CPU.
//
// FindRepetitiveRegions appends, in this order, (a) the groups of more than 12 k-mer cells at most 29 cells apart
// (kmers_), (b) for every up slope i and every later down slope j of FindSlopes(1.42) whose span is a coverage plateau
// well above the component's median, the span widened by a third of the two slopes; then MergeRegions and the clip to the
// valid region.  Every comparison is the reference's, in its types: uint32 arithmetic that may wrap, products in double,
// clamp to 65535 and truncation to uint16 / uint32 where the reference assigns.  A region is two uint32, (first, second)
// cells, and after the clip first = cell << 1 with bit 0 the flag that UpdateRepetitiveRegions sets.
#pragma once

#include "common.h"
#include "slopes.h"

namespace rvn {

constexpr double kRepeatQ = 1.42;

// appends one (first, second) pair; n counts every region, out holds the first cap of them
__host__ __device__ inline void repeat_push(u32* out, u32 cap, u32& n, u32 first, u32 second) {
  if (n < cap) {
    out[2 * n] = first;
    out[2 * n + 1] = second;
  }
  ++n;
}

// (a) pile.cc:232-259: groups of set k-mer cells (w = 479 >> kPSS, group = 12)
__host__ __device__ inline void repeat_kmer_groups(const u8* kmers, u32 nk, u32* out, u32 cap, u32& n) {
  const u32 w = 479 >> 4, group = 12;
  u32 rf = 0, rs = 0, count = 0;
  for (u32 i = 0; i < nk; ++i) {
    if (kmers[i] == 0) continue;
    if (count && i - rs <= w) {
      rs = i;
      ++count;
      continue;
    }
    if (count > group) repeat_push(out, cap, n, rf, rs);
    rf = rs = i;
    count = 1;
  }
  if (count > group) repeat_push(out, cap, n, rf, rs);
}

// the first test of is_repetitive_region (pile.cc:264-268): the midpoints of the two slopes, in uint32, at most
// 0.84 * (end_ - begin_) apart
__host__ __device__ inline bool repeat_span_short(const SlopeRegion& b, const SlopeRegion& e, u32 begin, u32 end) {
  const u32 d = ((e.first >> 1) + e.second) / 2 - ((b.first >> 1) + b.second) / 2;
  return !(static_cast<double>(d) > 0.84 * static_cast<double>(end - begin));
}
// clamp(1.42 * v) assigned to uint16 (pile.cc:270-272)
__host__ __device__ inline u16 repeat_threshold(u32 v) {
  return static_cast<u16>(slope_clamp(kRepeatQ * static_cast<double>(v)));
}
__host__ __device__ inline u16 repeat_peak(const u16* data, const SlopeRegion& b, const SlopeRegion& e) {
  const u16 x = data[b.second], y = data[e.first >> 1];
  return repeat_threshold(x > y ? x : y);
}
// the final test (pile.cc:283-285) on the counts over the cells strictly between the slopes
__host__ __device__ inline bool repeat_accept(bool found_peak, u32 num_valid, const SlopeRegion& b, const SlopeRegion& e) {
  return found_peak && !(static_cast<double>(num_valid) < 0.9 * static_cast<double>((e.first >> 1) - b.second));
}
// the region of an accepted pair (pile.cc:298-305): double values converted to uint32 as emplace_back does
__host__ __device__ inline void repeat_pair_region(const SlopeRegion& b, const SlopeRegion& e, u32* out, u32 cap, u32& n) {
  const double lo = static_cast<double>(b.second) - 0.336 * static_cast<double>(b.second - (b.first >> 1));
  const double hi = static_cast<double>(e.first >> 1) + 0.336 * static_cast<double>(e.second - (e.first >> 1));
  repeat_push(out, cap, n, static_cast<u32>(lo), static_cast<u32>(hi));
}

// is_repetitive_region (pile.cc:262-287), serially
__host__ __device__ inline bool repeat_is_region(const u16* data, const SlopeRegion& b, const SlopeRegion& e, u32 begin,
                                                 u32 end, u16 min_value) {
  if (!repeat_span_short(b, e, begin, end)) return false;
  const u16 peak = repeat_peak(data, b, e);
  bool found = false;
  u32 num_valid = 0;
  for (u32 i = b.second + 1; i < (e.first >> 1); ++i) {
    if (data[i] > min_value) ++num_valid;
    if (data[i] > peak) found = true;
  }
  return repeat_accept(found, num_valid, b, e);
}

// MergeRegions (pile.cc:373-400) on out[0, n) in place, then first = max(begin_, first) << 1, second = min(end_, second)
// (pile.cc:312-316).  The merged flag of pair j is bit 31 of its first (cells stay below 2^28); a merged region is
// written at position no <= i, which no later step reads.  Returns the number of regions left.
__host__ __device__ inline u32 repeat_merge_and_clip(u32* out, u32 n, u32 begin, u32 end) {
  const u32 kMerged = 1u << 31;
  u32 no = 0;
  for (u32 i = 0; i < n; ++i) {
    if (out[2 * i] & kMerged) continue;
    u32 f = out[2 * i], s = out[2 * i + 1];
    for (;;) {
      bool grew = false;
      for (u32 j = i + 1; j < n; ++j) {
        const u32 jf = out[2 * j], js = out[2 * j + 1];
        if (jf & kMerged) continue;
        if (f < js && s > jf) {
          grew = true;
          out[2 * j] = jf | kMerged;
          f = f < jf ? f : jf;
          s = s > js ? s : js;
        }
      }
      if (!grew) break;
    }
    out[2 * no] = (begin > f ? begin : f) << 1;
    out[2 * no + 1] = end < s ? end : s;
    ++no;
  }
  return no;
}

// Pile::FindRepetitiveRegions(median) on one pile, one thread: data[size] coverage, kmers[nk] (nk = 0: kmers_ empty),
// begin / end = begin_ / end_ in cells.  slopes: scratch of 2 * size regions (slopes.h), tmp: size cells.  *raw = the
// regions appended before MergeRegions (set_is_repetitive() happened iff *raw > 0); out holds cap pairs.  Returns the
// merged count when *raw <= cap; otherwise 0 and out is incomplete (the caller retries with cap = *raw).
// *slope_overflow: the slope scratch was too small (cannot happen with 2 * size: slopes.h).
__host__ __device__ inline u32 find_repetitive_regions(const u16* __restrict__ data, u32 size, const u8* __restrict__ kmers,
                                                       u32 nk, u32 begin, u32 end, u16 median, SlopeRegion* slopes,
                                                       u16* __restrict__ tmp, u32* __restrict__ out, u32 cap, u32* raw,
                                                       bool* slope_overflow) {
  u32 n = 0;
  repeat_kmer_groups(kmers, nk, out, cap, n);
  *slope_overflow = false;
  const u32 ns = find_slopes(data, static_cast<int>(size), kRepeatQ, slopes, 2 * size, tmp, slope_overflow);
  if (*slope_overflow) {
    *raw = n;
    return 0;
  }
  const u16 min_value = repeat_threshold(median);
  for (u32 i = 0; i + 1 < ns; ++i) {
    if (!(slopes[i].first & 1u)) continue;
    for (u32 j = i + 1; j < ns; ++j) {
      if (slopes[j].first & 1u) continue;
      if (repeat_is_region(data, slopes[i], slopes[j], begin, end, min_value)) repeat_pair_region(slopes[i], slopes[j], out, cap, n);
    }
  }
  *raw = n;
  return n <= cap ? repeat_merge_and_clip(out, n, begin, end) : 0;
}

// Pile::UpdateRepetitiveRegions(o) (pile.cc:319-342) for one region: true when the overlap, seen from this pile
// (coordinates ob / oe in bases; the lhs ones when the pile is o.lhs_id), sets the region's flag.  fuzz = 420 >> kPSS,
// offset = 0.1 * (end_ - begin_) truncated to uint32, the reference's unsigned comparisons.
__host__ __device__ inline bool repeat_update_hits(u32 rfirst, u32 rsecond, u32 ob, u32 oe, u32 begin, u32 end) {
  const u32 b = ob >> 4, e = oe >> 4, fuzz = 420 >> 4;
  const u32 offset = static_cast<u32>(0.1 * static_cast<double>(end - begin));
  const u32 rb = rfirst >> 1;
  if (!(b < rsecond && rb < e)) return false;
  if (rb < begin + offset && b - begin < end - e) return e >= rsecond + fuzz;
  if (rsecond > end - offset && b - begin > end - e) return b + fuzz <= rb;
  return false;
}
// Pile::CheckRepetitiveRegions(o) (pile.cc:344-369) for one region: true when the overlap is to be removed
__host__ __device__ inline bool repeat_check_hits(u32 rfirst, u32 rsecond, u32 ob, u32 oe, u32 begin, u32 end) {
  const u32 b = ob >> 4, e = oe >> 4, fuzz = 420 >> 4;
  const u32 offset = static_cast<u32>(0.1 * static_cast<double>(end - begin));
  const u32 rb = rfirst >> 1;
  if (!(b < rsecond && rb < e)) return false;
  if (rb < begin + offset) return e < rsecond + fuzz && (rfirst & 1u);
  if (rsecond > end - offset) return b + fuzz > rb && (rfirst & 1u);
  return false;
}

}  // namespace rvn
