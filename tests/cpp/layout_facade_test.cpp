// TEST INFRASTRUCTURE: raven::CreateForceDirectedLayout<Graph> (include/raven_hip/layout.hpp) on a seeded graph double
// against the reference's whole function restated on the host in this program (components, filters, pruning, seed, draws:
// below; the loop: layout_restated.hpp), twice in a row — the static seed doubles per call, as in the reference.  Every
// edge weight must be == .  usage: layout_facade_test [graph seed]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>

#include "layout_doubles.hpp"
#include "layout_restated.hpp"
#include "raven_hip/layout.hpp"

namespace {

using layout_doubles::Graph;

// the host function: as the reference, component by component; returns the number of components laid out
std::uint32_t HostLayout(Graph& graph, std::uint64_t seed) {
  std::vector<std::unordered_set<std::uint32_t>> components;
  std::vector<char> seen(graph.nodes.size(), 0);
  for (std::uint32_t i = 0; i < graph.nodes.size(); ++i) {
    if (!graph.nodes[i] || seen[i]) continue;
    components.emplace_back();
    std::deque<std::uint32_t> todo = {i};
    while (!todo.empty()) {
      const std::uint32_t j = todo.front();
      todo.pop_front();
      if (seen[j]) continue;
      const auto& node = graph.nodes[j];
      seen[node->id] = seen[node->pair->id] = 1;
      components.back().emplace(node->id & ~1u);
      for (auto e : node->inedges) todo.emplace_back(e->tail->id);
      for (auto e : node->outedges) todo.emplace_back(e->head->id);
    }
  }
  std::sort(components.begin(), components.end(),
            [](const std::unordered_set<std::uint32_t>& a, const std::unordered_set<std::uint32_t>& b) { return a.size() > b.size(); });
  std::mt19937 generator(seed);
  std::uniform_real_distribution<> distribution(0., 1.);
  std::uint32_t laid_out = 0;
  for (const auto& component : components) {
    if (component.size() < 6) continue;
    if (std::none_of(component.begin(), component.end(), [&](std::uint32_t n) { return graph.nodes[n]->is_junction(); })) continue;
    for (std::uint32_t n : component) {
      std::unordered_set<std::uint32_t> valid;
      for (std::uint32_t m : graph.nodes[n]->transitive)
        if (component.count(m)) valid.emplace(m);
      graph.nodes[n]->transitive.swap(valid);
    }
    std::vector<std::uint32_t> local(graph.nodes.size(), 0);
    std::vector<layout_restated::Vec> pos;
    for (std::uint32_t n : component) {
      local[n] = static_cast<std::uint32_t>(pos.size());
      layout_restated::Vec v;
      v.x = distribution(generator);
      v.y = distribution(generator);
      pos.push_back(v);
    }
    std::vector<std::uint64_t> adj_off = {0};
    std::vector<std::uint32_t> adj;
    for (std::uint32_t n : component) {
      for (auto e : graph.nodes[n]->inedges) adj.push_back(local[e->tail->id & ~1u]);
      for (auto e : graph.nodes[n]->outedges) adj.push_back(local[e->head->id & ~1u]);
      for (std::uint32_t m : graph.nodes[n]->transitive) adj.push_back(local[m]);
      adj_off.push_back(adj.size());
    }
    layout_restated::LayOut(pos, 0, static_cast<std::uint32_t>(pos.size()), adj_off.data(), adj.data(), 100);
    for (const auto& e : graph.edges) {
      if (!e || (e->id & 1)) continue;
      const std::uint32_t n = e->tail->id & ~1u, m = e->head->id & ~1u;
      if (!component.count(n) || !component.count(m)) continue;
      const double dx = pos[local[n]].x - pos[local[m]].x, dy = pos[local[n]].y - pos[local[m]].y;
      e->weight = e->pair->weight = std::sqrt(dx * dx + dy * dy);
    }
    ++laid_out;
  }
  return laid_out;
}

}  // namespace

int main(int argc, char** argv) {
  const std::uint32_t graph_seed = argc > 1 ? static_cast<std::uint32_t>(std::atoi(argv[1])) : 7;
  rvn_engine* engine = nullptr;
  if (rvn_engine_create(&engine, 15, 5, 500, 4, 100, 10000, 0) != RVN_OK) {
    std::printf("%s\n", rvn_last_error());
    return 1;
  }
  Graph device_graph = layout_doubles::MakeGraph(graph_seed), host_graph = layout_doubles::MakeGraph(graph_seed);
  std::uint64_t seed = 21;
  int rc = 0;
  for (int call = 0; call < 2; ++call) {
    seed <<= 1;
    rvn_layout_stats stats;
    raven::CreateForceDirectedLayout(engine, device_graph, 100, &stats);
    const std::uint32_t laid_out = HostLayout(host_graph, seed);
    std::uint64_t edges = 0, weighted = 0, mismatches = 0;
    for (size_t i = 0; i < host_graph.edges.size(); ++i) {
      if (!host_graph.edges[i]) continue;
      ++edges;
      weighted += host_graph.edges[i]->weight != 0;
      mismatches += !(host_graph.edges[i]->weight == device_graph.edges[i]->weight);
    }
    std::printf("call %d components %u edges %llu weighted %llu mismatches %llu host_tree_iterations %llu\n", call, laid_out,
                static_cast<unsigned long long>(edges), static_cast<unsigned long long>(weighted),
                static_cast<unsigned long long>(mismatches), static_cast<unsigned long long>(stats.host_tree_iterations));
    if (mismatches) rc = 3;
  }
  rvn_engine_destroy(engine);
  return rc;
}
