// raven_hip/layout.hpp — raven's CreateForceDirectedLayout (RavenLib/src/assemble.cc:357-627) with the layout itself on
// the MI355X: what the reference does to graph.edges[i]->weight, bit for bit, through one rvn_layout_force_directed call
// for all laid-out components.  Header-only; see INTEGRATION.md 3.1e.
//
// On the host, exactly as there: connected components over node pairs (breadth first from the lowest id), largest
// first, components with fewer than 6 members or without a junction skipped, every member's `transitive` pruned to the
// component, the static seed doubled per call, two draws per member in the iteration order of the component's
// std::unordered_set.  On the device: the 100 iterations.  Then the weights of the even-id edges and their pairs.
// The JSON dump of the reference's `path` argument is not provided.
//
// GraphT needs only what the reference uses: nodes, edges (vectors of smart pointers, entries may be null), and per node
// id, pair, inedges, outedges, transitive (std::unordered_set<std::uint32_t>), is_junction(); per edge id, pair, tail,
// head, weight.  raven::Graph fits as it is.
#ifndef RAVEN_HIP_LAYOUT_HPP_
#define RAVEN_HIP_LAYOUT_HPP_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <deque>
#include <random>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "raven_hip.h"

namespace raven {

namespace layout_detail {
// the reference's `static std::uint64_t seed = 21`, one per program
inline std::uint64_t& Seed() {
  static std::uint64_t seed = 21;
  return seed;
}
}  // namespace layout_detail

template <typename GraphT>
void CreateForceDirectedLayout(rvn_engine* engine, const GraphT& graph, std::uint32_t num_iterations = 100,
                               rvn_layout_stats* stats = nullptr) {
  std::vector<std::unordered_set<std::uint32_t>> components;
  {
    std::vector<char> is_visited(graph.nodes.size(), 0);
    for (std::uint32_t i = 0; i < graph.nodes.size(); ++i) {
      if (graph.nodes[i] == nullptr || is_visited[i]) continue;
      components.resize(components.size() + 1);
      std::deque<std::uint32_t> que = {i};
      while (!que.empty()) {
        const std::uint32_t j = que.front();
        que.pop_front();
        if (is_visited[j]) continue;
        const auto& node = graph.nodes[j];
        is_visited[node->id] = 1;
        is_visited[node->pair->id] = 1;
        components.back().emplace((node->id >> 1) << 1);
        for (auto it : node->inedges) que.emplace_back(it->tail->id);
        for (auto it : node->outedges) que.emplace_back(it->head->id);
      }
    }
  }
  std::sort(components.begin(), components.end(),
            [](const std::unordered_set<std::uint32_t>& lhs, const std::unordered_set<std::uint32_t>& rhs) {
              return lhs.size() > rhs.size();
            });

  std::uint64_t& seed = layout_detail::Seed();
  seed <<= 1;
  std::mt19937 generator(seed);
  std::uniform_real_distribution<> distribution(0., 1.);

  constexpr std::uint32_t kNone = 0xFFFFFFFFu;
  std::vector<std::uint32_t> point_of(graph.nodes.size(), kNone);  // node id -> point of the device call
  std::vector<std::uint32_t> offsets = {0}, adj;
  std::vector<std::uint64_t> adj_offsets = {0};
  std::vector<double> xy;
  std::vector<const std::unordered_set<std::uint32_t>*> laid_out;
  for (const auto& component : components) {
    if (component.size() < 6) continue;
    bool has_junctions = false;
    for (const auto& it : component) {
      if (graph.nodes[it]->is_junction()) {
        has_junctions = true;
        break;
      }
    }
    if (!has_junctions) continue;

    for (const auto& n : component) {
      std::unordered_set<std::uint32_t> valid;
      for (const auto& m : graph.nodes[n]->transitive)
        if (component.find(m) != component.end()) valid.emplace(m);
      graph.nodes[n]->transitive.swap(valid);
    }

    const std::uint32_t first = offsets.back();
    std::uint32_t next = first;
    for (const auto& it : component) {
      point_of[it] = next++;
      xy.push_back(distribution(generator));
      xy.push_back(distribution(generator));
    }
    offsets.push_back(next);
    auto neighbour = [&](std::uint32_t m) {
      if (m >= point_of.size() || point_of[m] == kNone || point_of[m] < first)
        throw std::invalid_argument("[raven_hip] CreateForceDirectedLayout: node " + std::to_string(m) +
                                    " is a neighbour of a component it is not a member of");
      adj.push_back(point_of[m]);
    };
    for (const auto& n : component) {
      for (auto e : graph.nodes[n]->inedges) neighbour((e->tail->id >> 1) << 1);
      for (auto e : graph.nodes[n]->outedges) neighbour((e->head->id >> 1) << 1);
      for (const auto& m : graph.nodes[n]->transitive) neighbour(m);
      adj_offsets.push_back(adj.size());
    }
    laid_out.push_back(&component);
  }
  if (stats) *stats = rvn_layout_stats{0, 0, 0};
  if (laid_out.empty()) return;

  std::vector<double> out(xy.size());
  if (rvn_layout_force_directed(engine, static_cast<std::uint32_t>(laid_out.size()), offsets.data(), xy.data(),
                                adj_offsets.data(), adj.data(), num_iterations, out.data(), stats) != RVN_OK)
    throw std::runtime_error(rvn_last_error());

  for (const auto& it : graph.edges) {
    if (it == nullptr || it->id & 1) continue;
    const std::uint32_t n = point_of[(it->tail->id >> 1) << 1], m = point_of[(it->head->id >> 1) << 1];
    if (n == kNone || m == kNone) continue;
    // (both in SOME laid-out component means both in the same one: an edge joins its ends' components)
    const double dx = out[2 * n] - out[2 * m], dy = out[2 * n + 1] - out[2 * m + 1];
    it->weight = std::sqrt(dx * dx + dy * dy);
    it->pair->weight = it->weight;
  }
}

}  // namespace raven

#endif  // RAVEN_HIP_LAYOUT_HPP_
