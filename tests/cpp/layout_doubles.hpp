// TEST INFRASTRUCTURE: a stand-in for raven::Graph with the members CreateForceDirectedLayout uses (graph.h:97-193), and
// a seeded generator of pair-consistent graphs: node 2a / 2a + 1 are the two strands of piece a, an edge 2a -> 2b (even
// id) comes with its pair 2b + 1 -> 2a + 1 (odd id).
#pragma once

#include <cstdint>
#include <memory>
#include <random>
#include <unordered_set>
#include <utility>
#include <vector>

namespace layout_doubles {

struct Edge;

struct Node {
  std::uint32_t id = 0;
  Node* pair = nullptr;
  std::vector<Edge*> inedges, outedges;
  std::unordered_set<std::uint32_t> transitive;
  bool is_junction() const { return outedges.size() > 1 || inedges.size() > 1; }
};

struct Edge {
  std::uint32_t id = 0;
  Node* tail = nullptr;
  Node* head = nullptr;
  Edge* pair = nullptr;
  double weight = 0;
};

struct Graph {
  std::vector<std::unique_ptr<Node>> nodes;
  std::vector<std::unique_ptr<Edge>> edges;

  void AddPieces(std::uint32_t n) {
    for (std::uint32_t i = 0; i < n; ++i) {
      const std::uint32_t id = static_cast<std::uint32_t>(nodes.size());
      nodes.emplace_back(new Node());
      nodes.emplace_back(new Node());
      nodes[id]->id = id;
      nodes[id + 1]->id = id + 1;
      nodes[id]->pair = nodes[id + 1].get();
      nodes[id + 1]->pair = nodes[id].get();
    }
  }
  void Hole() {  // a removed piece: two null entries
    nodes.emplace_back(nullptr);
    nodes.emplace_back(nullptr);
  }
  // strand bits choose which strands the edge joins; its pair joins the opposite strands the other way round
  void Join(std::uint32_t a, std::uint32_t b, std::uint32_t strand_a = 0, std::uint32_t strand_b = 0) {
    const std::uint32_t id = static_cast<std::uint32_t>(edges.size());
    edges.emplace_back(new Edge());
    edges.emplace_back(new Edge());
    Edge *e = edges[id].get(), *p = edges[id + 1].get();
    e->id = id;
    p->id = id + 1;
    e->pair = p;
    p->pair = e;
    e->tail = nodes[2 * a + strand_a].get();
    e->head = nodes[2 * b + strand_b].get();
    p->tail = nodes[2 * b + (strand_b ^ 1)].get();
    p->head = nodes[2 * a + (strand_a ^ 1)].get();
    for (Edge* x : {e, p}) {
      x->tail->outedges.push_back(x);
      x->head->inedges.push_back(x);
    }
  }
};

// pieces [first, first + n): a chain, `chords` random extra edges (junctions), `transitive` random transitive neighbours,
// a few of them pointing outside the component (the layout prunes those)
inline void Tangle(Graph& g, std::mt19937& rng, std::uint32_t first, std::uint32_t n, std::uint32_t chords,
                   std::uint32_t transitive) {
  auto pick = [&](std::uint32_t m) { return static_cast<std::uint32_t>(rng() % m); };
  // (a chain that changes strands has junctions: two edges end in the same strand of a piece; chords == 0 keeps one strand)
  for (std::uint32_t i = 0; i + 1 < n; ++i) g.Join(first + i, first + i + 1, chords ? pick(2) : 0, chords ? pick(2) : 0);
  for (std::uint32_t c = 0; c < chords; ++c) g.Join(first + pick(n), first + pick(n), pick(2), pick(2));
  const std::uint32_t pieces = static_cast<std::uint32_t>(g.nodes.size() / 2);
  for (std::uint32_t t = 0; t < transitive; ++t) {
    const std::uint32_t a = first + pick(n);
    std::uint32_t b = (t % 5 == 4) ? pick(pieces) : first + pick(n);
    if (!g.nodes[2 * b]) b = a;
    g.nodes[2 * a]->transitive.emplace(2 * b);
  }
}

// a big tangled component, two mid-sized ones, a chain without a junction, components below six pieces, holes
inline Graph MakeGraph(std::uint32_t seed) {
  std::mt19937 rng(seed);
  Graph g;
  const std::pair<std::uint32_t, std::uint32_t> parts[] = {{3, 1}, {40, 6}, {700, 80}, {12, 0}, {5, 2}, {64, 9}, {1, 0}, {6, 1}};
  for (const auto& part : parts) {
    const std::uint32_t first = static_cast<std::uint32_t>(g.nodes.size() / 2);
    g.AddPieces(part.first);
    Tangle(g, rng, first, part.first, part.second, part.second ? part.first / 8 + 1 : 0);
    g.Hole();
  }
  g.edges.emplace_back(nullptr);
  g.edges.emplace_back(nullptr);
  return g;
}

}  // namespace layout_doubles
