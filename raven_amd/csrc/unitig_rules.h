// unitig_rules.h — the segment rules of node sequences as __host__ __device__ functions (unitigs.hip; the host build for
// the CPU tests is tests/host/unitig_rules_host.cpp).
// A node's sequence is never stored as bases on the device: it is a TILING, a list of segments (read, first base, length,
// strand) whose concatenation is the sequence; strand 1 = the reverse complement of that stretch of the read.  Node 2i of
// ConstructAssemblyGraph is one segment (pile, begin, end - begin, 0), node 2i + 1 the same stretch with strand 1, and a
// unitig (RavenLib/src/graph.cc:27-57: Edge::Label() = the first `length` bases of the tail, per member) is the
// concatenation of prefixes of its members' tilings — again a list of read segments.
//   segment_prefix    the first L bases of one segment
//   prefix_segments   the number of segments a prefix of a tiling keeps
//   tiling_word       one packed 64-bit word (32 bases, base x at bits 2x .. 2x + 1, zero above the last base) of a
//                     tiling's sequence from the 2-bit packed reads, reverse complement included
//   slice_length, segment_slice, slice_word    InflateData(i, len) of a node; edge_lhs_length / edge_rhs_length: the two
//                     slices of an edge's similarity (graph_repr.cc:248-249)
// Codes are A C G T = 0 1 2 3, so the complement of a code is code ^ 3.
#pragma once

#include "graph_rules.h"

namespace rvn {

struct Segment {
  u32 read, begin, length, strand;
};

// the first L <= s.length bases of s: the FRONT of the stretch on strand 0, its BACK (read backwards) on strand 1
__host__ __device__ inline Segment segment_prefix(const Segment& s, u32 L) {
  Segment p = s;
  p.length = L;
  if (s.strand) p.begin = s.begin + (s.length - L);
  return p;
}

// cum[i] = bases of the tiling in front of segment i (cum[0] = 0), n of them.  The prefix of L bases keeps every segment
// that starts in front of base L — the number of i with cum[i] < L — and cuts the last of them with segment_prefix to
// L - cum[last] bases (a segment of length 0 in front of base L is kept as it is; L = 0 keeps nothing).
__host__ __device__ inline u32 prefix_segments(const u32* cum, u32 n, u32 L) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (cum[mid] < L) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// segment i of the prefix of L bases (i < prefix_segments(cum, n, L))
__host__ __device__ inline Segment prefix_segment(const Segment* seg, const u32* cum, u32 i, u32 L) {
  const u32 left = L - cum[i];
  return left < seg[i].length ? segment_prefix(seg[i], left) : seg[i];
}

// the segment that holds base p of the tiling (p < its length): the last i with cum[i] <= p
__host__ __device__ inline u32 segment_of_base(const u32* cum, u32 n, u32 p) {
  u32 lo = 0, hi = n;  // the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (cum[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the 2-bit groups of a word in reverse order
__host__ __device__ inline u64 reverse_bases(u64 x) {
  x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
  x = ((x >> 8) & 0x00FF00FF00FF00FFULL) | ((x & 0x00FF00FF00FF00FFULL) << 8);
  x = ((x >> 16) & 0x0000FFFF0000FFFFULL) | ((x & 0x0000FFFF0000FFFFULL) << 16);
  return (x >> 32) | (x << 32);
}
__host__ __device__ inline u64 low_bases(u32 take) { return take >= 32 ? ~0ULL : (1ULL << (2 * take)) - 1; }

// `take` (1 .. 32) bases of a read from base `pos` on, in the low bits: at most two source words, funnel-shifted.  words =
// the read's first word; the second word is read only when the bases reach into it.
__host__ __device__ inline u64 read_bases(const u64* words, u32 pos, u32 take) {
  const u32 k = pos >> 5, sh = 2 * (pos & 31);
  u64 w = words[k] >> sh;
  if (sh != 0 && (pos & 31) + take > 32) w |= words[k + 1] << (64 - sh);
  return w & low_bases(take);
}
// bases [o, o + take) of segment s (o + take <= s.length, take 1 .. 32)
__host__ __device__ inline u64 segment_bases(const Segment& s, u32 o, u32 take, const u64* packed, const u64* word_off) {
  const u64* words = packed + word_off[s.read];
  if (!s.strand) return read_bases(words, s.begin + o, take);
  // base o of the reverse complement is the complement of base length - 1 - o of the stretch
  const u64 fwd = read_bases(words, s.begin + (s.length - o - take), take);
  return (reverse_bases(fwd) >> (2 * (32 - take))) ^ low_bases(take);
}

// The packed word of bases [first, first + 32) of a tiling of n segments and `length` bases (first < length): the
// covering segment by binary search, then piece by piece while the word spans several segments.
__host__ __device__ inline u64 tiling_word(const Segment* seg, const u32* cum, u32 n, u32 length, u32 first, const u64* packed,
                                           const u64* word_off) {
  const u32 left = length - first;
  const u32 end = first + (left < 32 ? left : 32);
  u32 i = segment_of_base(cum, n, first);
  u32 p = first;
  u64 w = 0;
  while (p < end && i < n) {
    const u32 o = p - cum[i];
    const u32 room = seg[i].length - o;
    const u32 take = room < end - p ? room : end - p;
    if (take) w |= segment_bases(seg[i], o, take, packed, word_off) << (2 * (p - first));
    p += take;
    ++i;
  }
  return w;
}

// ---- slices: biosoup::NucleicAcid::InflateData(i, len) on a tiling ----
// the bases of a node of `own` bases that InflateData(i, len) returns: [i, i + slice_length), nothing from i >= own on
__host__ __device__ inline u32 slice_length(u32 own, u32 i, u32 len) {
  if (i >= own) return 0;
  return len < own - i ? len : own - i;
}
// bases [o, o + L) of one segment (o + L <= s.length) as a segment of its own.  On strand 1 the segment reads its stretch
// backwards, so the slice is the reverse complement of the MIRRORED stretch: the L bases that end o bases in front of the
// stretch's end.  segment_slice(s, 0, L) == segment_prefix(s, L).
__host__ __device__ inline Segment segment_slice(const Segment& s, u32 o, u32 L) {
  Segment p = s;
  p.length = L;
  p.begin = s.strand ? s.begin + (s.length - o - L) : s.begin + o;
  return p;
}
// packed word w of the slice [i, i + L) of a tiling (L = slice_length(...), 32 w < L): the tiling's bases from i + 32 w on,
// cut at the slice's end — tiling_word of the tiling shortened to i + L bases, which is zero above the last base
__host__ __device__ inline u64 slice_word(const Segment* seg, const u32* cum, u32 n, u32 i, u32 L, u32 w, const u64* packed,
                                          const u64* word_off) {
  return tiling_word(seg, cum, n, i + L, i + 32u * w, packed, word_off);
}
// The two strings of an edge's similarity (RavenLib/src/graph_repr.cc:248-249): lhs = tail.InflateData(length), rhs =
// head.InflateData(0, lhs.size()).  A length at or beyond the tail's end (a wrapped one included) gives an empty lhs.
__host__ __device__ inline u32 edge_lhs_length(u32 tail_len, u32 edge_length) {
  return tail_len > edge_length ? tail_len - edge_length : 0;
}
__host__ __device__ inline u32 edge_rhs_length(u32 lhs_len, u32 head_len) { return lhs_len < head_len ? lhs_len : head_len; }

// ---- the sequence of a node path (RemoveBubbles' path_sequence, RavenLib/src/assemble.cc:225-237) ----
// what a member of `own` bases contributes: Edge::Label() = InflateData(0, label), which clamps a length beyond the
// sequence (a wrapped edge length gives the whole node); the last member is taken whole, whatever its label
__host__ __device__ inline u32 path_member_keep(u32 label, u32 own, bool last) { return last || label > own ? own : label; }

// ---- what CreateUnitigs decides per chain (RavenLib/src/common.cc:96-112, graph.cc:53) ----
// a chain of `nodes` nodes is made a unitig when it is circular or has 2 epsilon + 2 nodes (uint32 arithmetic, as there)
__host__ __device__ inline bool chain_is_kept(u32 nodes, bool circular, u32 epsilon) {
  return circular || nodes >= static_cast<u32>(2u * epsilon + 2u);
}
__host__ __device__ inline u16 unitig_coverage(u16 begin, u16 end) {
  return static_cast<u16>((static_cast<int>(begin) + static_cast<int>(end)) / 2);
}
__host__ __device__ inline bool unitig_is_unitig(u32 count, u32 length, u32 min_unitig_size) {
  return count > 5 && length > min_unitig_size;
}

}  // namespace rvn
