// raven_hip/unitigs.hpp — raven::CreateUnitigs (RavenLib/src/common.cc:32-225) with the chains found and the unitig
// sequences gathered on the MI355X (rvn_graph_create_unitigs, rvn_unitigs_as_reads).  Header-only; see INTEGRATION.md 3.1g.
//
// What stays on the host, exactly as there: the factories' calls in the reference's order, the new nodes' `transitive`
// sets (filled member by member, so that their iteration order is the reference's), node_updates, the
// original_node_sequence_names, RemoveEdges(graph, marked, true) (the caller's, found through the graph type's namespace)
// and the final remap of every node's `transitive`.
//
// GraphT needs what assembly_graph.hpp needs, and per node count, is_unitig, is_circular, sequence.name,
// original_node_sequence_names (a set of std::string); the node type is constructible through
// node_factory.MakeUnique(SequenceT{name, data}).  raven::Graph fits once Node has that constructor (raven's own
// Node(id, sequence) is it).
#ifndef RAVEN_HIP_UNITIGS_HPP_
#define RAVEN_HIP_UNITIGS_HPP_

#include <type_traits>

#include "raven_hip/assembly_graph.hpp"

namespace raven {

// Node sequences as read segments on the device.  Made once behind ConstructAssemblyGraph; every CreateUnitigs call
// appends its new nodes, so the tilings follow graph.nodes.
struct Tilings {
  rvn_tiling* t = nullptr;
  Tilings() = default;
  Tilings(const Tilings&) = delete;
  Tilings& operator=(const Tilings&) = delete;
  ~Tilings() { rvn_tiling_destroy(t); }
};

// The tilings of the graph ConstructAssemblyGraph has just made: nodes 2k and 2k + 1 are the k-th valid pile's valid region
// and its reverse complement.  reads = the device read set the piles belong to (pile i = read i).
template <typename PilesT>
void MakeTilings(rvn_engine* engine, const rvn_reads* reads, const PilesT& piles, Tilings* out) {
  const std::uint32_t n = static_cast<std::uint32_t>(piles.size());
  std::vector<std::uint32_t> begin(n), end(n), node_pile;
  for (std::uint32_t i = 0; i < n; ++i) {
    begin[i] = piles[i]->begin();
    end[i] = piles[i]->end();
    if (piles[i]->is_invalid()) continue;
    node_pile.push_back(i);
    node_pile.push_back(i);
  }
  rvn_tiling_destroy(out->t);
  out->t = nullptr;
  graph_detail::Check(rvn_tiling_from_piles(engine, reads, static_cast<std::uint32_t>(node_pile.size()), node_pile.data(), n,
                                            begin.data(), end.data(), &out->t));
}

namespace unitig_detail {

struct Tables {
  rvn_unitigs* u = nullptr;
  rvn_reads* sequences = nullptr;
  Tables() = default;
  Tables(const Tables&) = delete;
  Tables& operator=(const Tables&) = delete;
  ~Tables() {
    rvn_reads_destroy(sequences);
    rvn_unitigs_destroy(u);
  }
};

}  // namespace unitig_detail

// Returns the number of unitigs made (pairs of new nodes).  Throws std::invalid_argument when the factories do not
// continue graph.nodes / graph.edges, and for everything rvn_graph_create_unitigs refuses.
template <typename GraphT>
std::uint32_t CreateUnitigs(rvn_engine* engine, GraphT& graph, const rvn_reads* reads, Tilings& tilings, std::uint32_t epsilon = 0,
                            std::uint32_t min_unitig_size = 9999) {
  using NodeT = typename std::remove_reference<decltype(*graph.nodes[0])>::type;
  using SequenceT = decltype(std::declval<NodeT>().sequence);
  const std::size_t n_old = graph.nodes.size(), e_old = graph.edges.size();
  if (static_cast<std::size_t>(graph.node_factory.NextIndex()) != n_old || static_cast<std::size_t>(graph.edge_factory.NextIndex()) != e_old)
    throw std::invalid_argument("[raven_hip] CreateUnitigs: the factories do not continue graph.nodes / graph.edges");
  graph_detail::Handle h;
  graph_detail::Flatten(engine, graph, false, &h);
  std::vector<std::uint32_t> count(n_old, 0);
  std::vector<std::uint16_t> coverage(n_old, 0);
  for (std::size_t v = 0; v < n_old; ++v) {
    if (graph.nodes[v] == nullptr) continue;
    count[v] = graph.nodes[v]->count;
    coverage[v] = graph.nodes[v]->coverage;
  }
  unitig_detail::Tables t;
  graph_detail::Check(rvn_graph_create_unitigs(engine, h.g, tilings.t, count.data(), coverage.data(), epsilon, min_unitig_size, &t.u));
  std::uint32_t n_new = 0;
  std::uint64_t n_members = 0, n_new_edges = 0;
  graph_detail::Check(rvn_unitigs_info(t.u, nullptr, &n_new, &n_members, nullptr, &n_new_edges));
  std::vector<std::uint32_t> begin(n_new), end(n_new), cnt(n_new), members(n_members), e_tail(n_new_edges), e_head(n_new_edges),
      e_length(n_new_edges);
  std::vector<std::uint16_t> cov(n_new);
  std::vector<std::uint8_t> circular(n_new), is_unitig(n_new), flags(e_old);
  std::vector<std::uint64_t> member_off(static_cast<std::size_t>(n_new) + 1);
  graph_detail::Check(rvn_unitigs_fetch(t.u, begin.data(), end.data(), circular.data(), cnt.data(), nullptr, cov.data(), is_unitig.data(),
                                        member_off.data(), members.data(), flags.data(), e_tail.data(), e_head.data(), e_length.data()));

  // the new nodes' sequences: gathered on the device, inflated here
  graph_detail::Check(rvn_unitigs_as_reads(engine, t.u, tilings.t, reads, RVN_UNITIGS_ALL, &t.sequences));
  std::uint64_t n_words = 0;
  graph_detail::Check(rvn_reads_info(t.sequences, nullptr, &n_words, nullptr, nullptr, nullptr));
  std::vector<std::uint64_t> words(n_words), word_off(static_cast<std::size_t>(n_new) + 1);
  std::vector<std::uint32_t> length(n_new);
  graph_detail::Check(rvn_reads_fetch(t.sequences, words.data(), word_off.data(), length.data(), nullptr, nullptr));

  std::vector<decltype(graph.node_factory.MakeUnique(std::declval<SequenceT>()))> nodes;
  nodes.reserve(n_new);
  auto node_at = [&](std::uint32_t id) { return id < n_old ? graph.nodes[id].get() : nodes[id - n_old].get(); };
  for (std::uint32_t j = 0; j < n_new; ++j) {
    std::string data(length[j], 'A');
    for (std::uint32_t x = 0; x < length[j]; ++x) data[x] = "ACGT"[(words[word_off[j] + x / 32] >> (2 * (x % 32))) & 3];
    const std::uint32_t id = graph.node_factory.NextIndex();
    nodes.emplace_back(graph.node_factory.MakeUnique(SequenceT{(is_unitig[j] ? "Utg" : "Ctg") + std::to_string(id & ~1u), data}));
    NodeT& u = *nodes.back();
    u.count = cnt[j];
    u.is_circular = circular[j] != 0;
    u.is_unitig = is_unitig[j] != 0;
    u.coverage = cov[j];
    if (j % 2 == 1) {
      u.pair = nodes[j - 1].get();
      nodes[j - 1]->pair = &u;
    }
  }
  std::vector<decltype(graph.edge_factory.MakeUnique(node_at(0), node_at(0), std::uint32_t()))> edges;
  edges.reserve(n_new_edges);
  for (std::uint64_t x = 0; x < n_new_edges; ++x) {
    edges.emplace_back(graph.edge_factory.MakeUnique(node_at(e_tail[x]), node_at(e_head[x]), e_length[x]));
    if (x % 2 == 1) {
      edges[x]->pair = edges[x - 1].get();
      edges[x - 1]->pair = edges[x].get();
    }
  }

  // Per unitig what the reference's loop body leaves on the host side.  The names: the ends of every edge it marks for the
  // unitig (the members, the tail of begin's in-edge, the head of end's out-edge), and of their pairs for its pair.  The
  // transitive sets: member by member from begin up to, not including, end (all the way round a circular one).
  std::vector<std::uint32_t> node_updates(n_old, 0);
  for (std::uint32_t j = 0; j < n_new; j += 2) {
    NodeT& unitig = *nodes[j];
    NodeT& unitig_rc = *nodes[j + 1];
    const std::uint64_t first = member_off[j], last = member_off[j + 1];
    auto names = [&](NodeT* member) {
      unitig.original_node_sequence_names.insert(member->sequence.name);
      unitig_rc.original_node_sequence_names.insert(member->pair->sequence.name);
    };
    for (std::uint64_t k = first; k < last; ++k) names(graph.nodes[members[k]].get());
    if (!circular[j]) {
      NodeT* b = graph.nodes[begin[j]].get();
      NodeT* e = graph.nodes[end[j]].get();
      if (!b->inedges.empty()) names(b->inedges.front()->tail);
      if (!e->outedges.empty()) names(e->outedges.front()->head);
    }
    for (std::uint64_t k = first; k < (circular[j] ? last : last - 1); ++k) {
      const std::uint32_t even = members[k] & ~1u;
      node_updates[even] = unitig.id;
      unitig.transitive.insert(graph.nodes[even]->transitive.begin(), graph.nodes[even]->transitive.end());
    }
  }

  for (auto& n : nodes) graph.nodes.emplace_back(std::move(n));
  for (auto& e : edges) graph.edges.emplace_back(std::move(e));
  std::unordered_set<std::uint32_t> marked;
  for (std::size_t i = 0; i < e_old; ++i)
    if (flags[i]) marked.insert(static_cast<std::uint32_t>(i));
  RemoveEdges(graph, marked, true);
  for (const auto& it : graph.nodes) {
    if (it == nullptr) continue;
    std::unordered_set<std::uint32_t> valid;
    for (const std::uint32_t jt : it->transitive) valid.emplace(jt < n_old && node_updates[jt] != 0 ? node_updates[jt] : jt);
    it->transitive.swap(valid);
  }
  return n_new / 2;
}

}  // namespace raven

#endif  // RAVEN_HIP_UNITIGS_HPP_
