// raven_hip/assembly_graph.hpp — raven's ConstructAssemblyGraph (RavenLib/src/construct.cc:561-648), RemoveTransitiveEdges
// (assemble.cc:23-73) and the marking loop of RemoveLongEdges (assemble.cc:708-721) with the edge table made and reduced
// on the MI355X (rvn_construct_assembly_graph, rvn_graph_mark_transitive, rvn_graph_mark_long_edges).  Header-only; see
// INTEGRATION.md 3.1f.
//
// What stays on the host, exactly as there: node sequences (InflateData of the valid region, ReverseAndComplement), the
// factories' calls in the reference's order, the nodes' `transitive` sets, RemoveEdges (the caller's, found through the
// graph type's namespace), tips, bubbles.  Unitigs: raven_hip/unitigs.hpp.
//
// GraphT needs what the reference uses: nodes, edges (vectors of std::unique_ptr, entries may be null), node_factory /
// edge_factory with NextIndex() and MakeUnique(...); per node id, pair, coverage, outedges, transitive
// (std::unordered_set<std::uint32_t>); per edge id, pair, tail, head, length, weight.  Piles: id(), begin(), end(),
// median(), is_invalid().  Sequences: name, InflateData(begin, length), and a type constructible from (name, data) with
// ReverseAndComplement().  raven::Graph, raven::Pile and biosoup::NucleicAcid fit as they are.
#ifndef RAVEN_HIP_ASSEMBLY_GRAPH_HPP_
#define RAVEN_HIP_ASSEMBLY_GRAPH_HPP_

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "raven_hip.h"

namespace raven {

namespace graph_detail {

inline void Check(int rc) {
  if (rc == RVN_OK) return;
  if (rc == RVN_EINVAL) throw std::invalid_argument(rvn_last_error());
  throw std::runtime_error(rvn_last_error());
}

struct Handle {
  rvn_graph* g = nullptr;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() { rvn_graph_destroy(g); }
};

// graph.edges as the flat table of rvn_graph_from_edges.  The device takes the pair of edge i to be i ^ 1, node ids to
// be positions in graph.nodes, and (check_order) a node's out-edges to stand in ascending edge id.
template <typename GraphT>
void Flatten(rvn_engine* engine, const GraphT& graph, bool check_order, Handle* out) {
  const std::size_t n_edges = graph.edges.size();
  std::vector<std::uint32_t> tail(n_edges, 0xFFFFFFFFu), head(n_edges, 0), length(n_edges, 0);
  for (std::size_t i = 0; i < n_edges; ++i) {
    const auto& e = graph.edges[i];
    if (e == nullptr) continue;
    if (e->id != i || e->pair == nullptr || e->pair->id != (i ^ 1))
      throw std::invalid_argument("[raven_hip] assembly graph: edge " + std::to_string(i) +
                                  " does not sit at its id beside its pair (id ^ 1)");
    tail[i] = e->tail->id;
    head[i] = e->head->id;
    length[i] = e->length;
  }
  for (std::size_t v = 0; v < graph.nodes.size(); ++v) {
    const auto& node = graph.nodes[v];
    if (node == nullptr) continue;
    if (node->id != v) throw std::invalid_argument("[raven_hip] assembly graph: node " + std::to_string(v) + " does not sit at its id");
    if (!check_order) continue;
    for (std::size_t k = 1; k < node->outedges.size(); ++k)
      if (node->outedges[k - 1]->id >= node->outedges[k]->id)
        throw std::invalid_argument("[raven_hip] RemoveTransitiveEdges: the out-edges of node " + std::to_string(v) +
                                    " are not in ascending edge id (the order the device form reproduces)");
  }
  Check(rvn_graph_from_edges(engine, static_cast<std::uint32_t>(graph.nodes.size()), n_edges, tail.data(), head.data(),
                             length.data(), &out->g));
}

}  // namespace graph_detail

// overlaps.back() is finalized where it makes an edge (coordinates relative to the valid regions, score = 3 or 4), as
// OverlapFinalize leaves it; the overlaps that make none are left as they were (the reference stores their type in
// `score`, which nothing reads afterwards).
template <typename GraphT, typename PilesT, typename OverlapsT, typename SequencesT>
void ConstructAssemblyGraph(rvn_engine* engine, GraphT& graph, const PilesT& piles, OverlapsT& overlaps,
                            const SequencesT& sequences) {
  using SequenceT = typename SequencesT::value_type::element_type;
  const std::uint32_t n = static_cast<std::uint32_t>(piles.size());
  std::vector<std::uint32_t> begin(n), end(n);
  std::vector<std::uint16_t> median(n);
  std::vector<std::uint8_t> invalid(n);
  for (std::uint32_t i = 0; i < n; ++i) {
    if (piles[i]->id() != i) throw std::invalid_argument("[raven_hip] ConstructAssemblyGraph: pile " + std::to_string(i) + " does not sit at its id");
    begin[i] = piles[i]->begin();
    end[i] = piles[i]->end();
    median[i] = piles[i]->median();
    invalid[i] = piles[i]->is_invalid() ? 1 : 0;
  }
  auto& list = overlaps.back();
  std::vector<rvn_overlap> flat(list.size());
  for (std::size_t i = 0; i < list.size(); ++i)
    flat[i] = rvn_overlap{list[i].lhs_id, list[i].lhs_begin, list[i].lhs_end, list[i].rhs_id,
                          list[i].rhs_begin, list[i].rhs_end, list[i].score, list[i].strand ? 1u : 0u};
  graph_detail::Handle h;
  graph_detail::Check(rvn_construct_assembly_graph(engine, flat.data(), flat.size(), n, begin.data(), end.data(), median.data(),
                                                   invalid.data(), &h.g));
  std::uint32_t n_nodes = 0;
  std::uint64_t n_edges = 0;
  graph_detail::Check(rvn_graph_info(h.g, &n_nodes, &n_edges, nullptr));
  std::vector<std::int32_t> sequence_to_node(n);
  std::vector<std::uint32_t> tail(n_edges), head(n_edges), length(n_edges);
  std::vector<std::uint64_t> source(n_edges / 2);
  std::vector<rvn_overlap> finalized(n_edges / 2);
  graph_detail::Check(rvn_graph_fetch(h.g, sequence_to_node.data(), nullptr, nullptr, tail.data(), head.data(), length.data(),
                                      source.data(), finalized.data()));

  // The overlaps that made an edge go back finalized, each to its place in the caller's list.
  for (std::uint64_t j = 0; j < n_edges / 2; ++j) {
    auto& o = list[source[j]];
    o.lhs_begin = finalized[j].lhs_begin;
    o.lhs_end = finalized[j].lhs_end;
    o.rhs_begin = finalized[j].rhs_begin;
    o.rhs_end = finalized[j].rhs_end;
    o.score = finalized[j].score;
  }

  // Nodes: the two strands of every valid pile, in pile order, through the caller's factory.  The device numbered them
  // from 0 (sequence_to_node), which is also how the reference indexes the nodes it has just made: the factory has to
  // hand out exactly these ids.
  std::vector<decltype(graph.node_factory.MakeUnique(std::declval<SequenceT&>()))> nodes;
  nodes.reserve(n_nodes);
  for (std::uint32_t i = 0; i < n; ++i) {
    if (sequence_to_node[i] < 0) continue;
    const std::size_t first = static_cast<std::size_t>(sequence_to_node[i]);
    if (nodes.size() != first || static_cast<std::size_t>(graph.node_factory.NextIndex()) != first)
      throw std::invalid_argument("[raven_hip] ConstructAssemblyGraph: the node factory does not count from 0");
    const auto& pile = *piles[i];
    SequenceT strand{sequences[i]->name, sequences[i]->InflateData(pile.begin(), pile.end() - pile.begin())};
    for (int k = 0; k < 2; ++k) {
      if (k == 1) strand.ReverseAndComplement();
      nodes.emplace_back(graph.node_factory.MakeUnique(strand));
      nodes.back()->coverage = pile.median();
    }
    nodes[first]->pair = nodes[first + 1].get();
    nodes[first + 1]->pair = nodes[first].get();
  }

  // Edges: straight down the device table (slot e runs tail[e] -> head[e]; slots 2j and 2j + 1 are each other's pair, and
  // the table already holds the odd slot as the even one seen from the opposite strands).
  std::vector<decltype(graph.edge_factory.MakeUnique(nodes[0].get(), nodes[0].get(), std::uint32_t()))> edges;
  edges.reserve(n_edges);
  for (std::uint64_t e = 0; e < n_edges; ++e) {
    edges.emplace_back(graph.edge_factory.MakeUnique(nodes[tail[e]].get(), nodes[head[e]].get(), length[e]));
    if (e % 2 == 1) {
      edges[e]->pair = edges[e - 1].get();
      edges[e - 1]->pair = edges[e].get();
    }
  }
  graph.nodes = std::move(nodes);
  graph.edges = std::move(edges);
}

// Marks on the device, the rest of RemoveTransitiveEdges (assemble.cc:58-72) on the host.  The reference fills the nodes'
// `transitive` sets while it ITERATES its std::unordered_set of marked ids, so what has to be reproduced is that set's
// iteration order: the marked ids are inserted into a fresh set in the order in which the reference's set received them
// (rvn_graph_fetch_transitive), and the set is then walked.  The two node ids every odd marked edge contributes come
// from the device's pair list.  RemoveEdges(graph, marked) is the caller's, found through the graph type's namespace.
// Throws std::invalid_argument when a node's out-edges are not in ascending edge id.
template <typename GraphT>
std::uint32_t RemoveTransitiveEdges(rvn_engine* engine, GraphT& graph) {
  graph_detail::Handle h;
  graph_detail::Flatten(engine, graph, true, &h);
  std::uint64_t n_marked = 0, n_pairs = 0;
  graph_detail::Check(rvn_graph_mark_transitive(engine, h.g, &n_marked));
  std::vector<std::uint32_t> sequence(n_marked), ends(2 * n_marked);
  graph_detail::Check(rvn_graph_fetch_transitive(h.g, sequence.data(), ends.data(), &n_pairs));

  // odd marked id -> its position in the pair list (the list follows the sequence, odd ids only)
  std::vector<std::uint32_t> pair_at(graph.edges.size(), 0);
  std::uint32_t next_pair = 0;
  std::unordered_set<std::uint32_t> marked;
  for (const std::uint32_t id : sequence) {
    marked.insert(id);
    if (id % 2 == 1) pair_at[id] = next_pair++;
  }
  if (next_pair != n_pairs) throw std::runtime_error("[raven_hip] RemoveTransitiveEdges: pair list and marked ids disagree");
  for (const std::uint32_t id : marked) {
    if (id % 2 == 0) continue;
    const std::uint32_t a = ends[2 * pair_at[id]], b = ends[2 * pair_at[id] + 1];
    graph.nodes[a]->transitive.insert(b);
    graph.nodes[b]->transitive.insert(a);
  }
  RemoveEdges(graph, marked);
  return static_cast<std::uint32_t>(marked.size() / 2);
}

// The marked set of RemoveLongEdges' loop over the edges' current weights (ids in ascending order of insertion: what
// RemoveEdges does with the set does not depend on its order).  The loop around it, RemoveEdges and RemoveTips stay the
// caller's.
template <typename GraphT>
std::unordered_set<std::uint32_t> MarkLongEdges(rvn_engine* engine, const GraphT& graph) {
  graph_detail::Handle h;
  graph_detail::Flatten(engine, graph, false, &h);
  const std::size_t n_edges = graph.edges.size();
  std::vector<double> weight(n_edges, 0.0);
  for (std::size_t i = 0; i < n_edges; ++i)
    if (graph.edges[i] != nullptr) weight[i] = graph.edges[i]->weight;
  std::vector<std::uint8_t> flags(n_edges, 0);
  graph_detail::Check(rvn_graph_mark_long_edges(engine, h.g, weight.data(), flags.data(), nullptr));
  std::unordered_set<std::uint32_t> marked;
  for (std::size_t i = 0; i < n_edges; ++i)
    if (flags[i]) marked.insert(static_cast<std::uint32_t>(i));
  return marked;
}

}  // namespace raven

#endif  // RAVEN_HIP_ASSEMBLY_GRAPH_HPP_
