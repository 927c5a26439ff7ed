// graph_rules.h — the per-edge rules of the assembly graph as __host__ __device__ functions (graph.hip; the host build
// for the CPU tests is tests/host/graph_rules_host.cpp):
//   edge_record      the two edges ConstructAssemblyGraph makes of one finalized overlap (RavenLib/src/construct.cc:617-641)
//   is_comparable    the double comparison of RemoveTransitiveEdges (assemble.cc:27-31)
//   is_long_edge     the weight comparison of RemoveLongEdges' marking loop (assemble.cc:713-720)
// Lengths are the reference's std::uint32_t arithmetic (differences and sums wrap exactly as they do there); the
// comparisons are plain IEEE double — this header must not be compiled with fast-math.
#pragma once

#include "overlap_rules.h"

namespace rvn {

constexpr u32 kNoEdge = 0xFFFFFFFFu;  // tail of an empty edge slot (graph.edges[i] == nullptr); "no candidate"

// (a within 12 % of b) or (b within 12 % of a); 1 - eps and 1 + eps are double operations on the double 0.12, as in the
// reference (a compiler that folds them folds them to the same doubles)
__host__ __device__ inline bool is_comparable(double a, double b) {
  const double eps = 0.12;
  return (a >= b * (1 - eps) && a <= b * (1 + eps)) || (b >= a * (1 - eps) && b <= a * (1 + eps));
}
// the walk v -> x -> y (edges of lengths len_j, len_k) against the direct edge v -> y of length len_c: the sum wraps in
// 32 bits (jt->length + kt->length on std::uint32_t) before it becomes a double
__host__ __device__ inline bool is_transitive(u32 len_j, u32 len_k, u32 len_c) {
  return is_comparable(static_cast<double>(static_cast<u32>(len_j + len_k)), static_cast<double>(len_c));
}

// edge kt is long when another out-edge of its node has less than half its weight; min_other = the smallest weight
// among the node's OTHER out-edges (x * 2.0 is monotone, so the smallest decides)
__host__ __device__ inline bool is_long_edge(double min_other, double weight) { return min_other * 2.0 < weight; }

// The pair of edges of one FINALIZED overlap f (overlap_finalize returned true: score = 3 or 4, coordinates relative to
// the valid regions).  node_l / node_r: node of the lhs / rhs pile (even), len_l / len_r: Pile::length() = end - begin.
// The edge runs tail -> head with `length`, its pair head ^ 1 -> tail ^ 1 with `length_pair`.
struct EdgeRecord {
  u32 tail, head, length, length_pair;
};
__host__ __device__ inline EdgeRecord edge_record(const Overlap& f, u32 node_l, u32 node_r, u32 len_l, u32 len_r) {
  EdgeRecord r;
  r.tail = node_l;
  r.head = node_r + 1u - f.strand;
  r.length = f.lhs_begin - f.rhs_begin;
  r.length_pair = (len_r - f.rhs_end) - (len_l - f.lhs_end);
  if (f.score == 4) {
    const u32 t = r.tail;
    r.tail = r.head;
    r.head = t;
    r.length = 0u - r.length;
    r.length_pair = 0u - r.length_pair;
  }
  return r;
}

}  // namespace rvn
