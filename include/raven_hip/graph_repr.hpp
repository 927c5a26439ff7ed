// raven_hip/graph_repr.hpp — what printEdgeSimilarity makes raven's CSV emitters compute per edge
// (RavenLib/src/graph_repr.cc:247-258 in PrintCsv, :358-369 in getCsv) on the MI355X (rvn_graph_edge_similarity).
// Header-only; see INTEGRATION.md 3.1i and DESIGN.md 3.15.
//
// The reference inflates, for every edge and on one thread, the tail from `length` on and the head's prefix of the same
// size, aligns the two strings with edlib and prints 1 - editDistance / lhs.size().  Here the scores of all edges come
// from one call before the emitter's loop, which then prints similarity[it->id]; the text of the emitters stays Raven's.
//
// The facade never reads a node's sequence: the node type needs none.  GraphT needs nodes, edges (vectors of
// std::unique_ptr, entries may be null); per node id; per edge id, pair, tail, head, length.  The tiling holds the
// sequence of node i under i and has as many nodes as graph.nodes (raven_hip/unitigs.hpp: MakeTilings, CreateUnitigs).
#ifndef RAVEN_HIP_GRAPH_REPR_HPP_
#define RAVEN_HIP_GRAPH_REPR_HPP_

#include "raven_hip/assembly_graph.hpp"

namespace raven {

// similarity[id] = the score the reference prints for graph.edges[id]: NaN where its lhs is empty (0 / 0., as there) and
// for an empty slot, which the emitters skip.  Throws std::invalid_argument for an edge that does not sit at its id beside
// its pair, a node that does not sit at its id, a tiling whose node count is not the graph's, a read set other than the
// tiling's.
template <typename GraphT>
std::vector<double> EdgeSimilarity(rvn_engine* engine, const GraphT& graph, const rvn_tiling* tiling, const rvn_reads* reads) {
  graph_detail::Handle h;
  graph_detail::Flatten(engine, graph, false, &h);
  std::vector<double> similarity(graph.edges.size());
  graph_detail::Check(rvn_graph_edge_similarity(engine, h.g, tiling, reads, nullptr, nullptr, nullptr, similarity.data()));
  return similarity;
}

}  // namespace raven

#endif  // RAVEN_HIP_GRAPH_REPR_HPP_
