// TEST DOUBLES (tests/cpp only) of what include/raven_hip/unitigs.hpp touches of Raven itself, on top of what
// graph_doubles.hpp has: a node with count, is_unitig, is_circular and original_node_sequence_names (graph.h:127-151),
// and RemoveEdges with remove_nodes (common.cc:5-30).  A Raven build uses its own.
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "graph_doubles.hpp"

namespace unitig_doubles {

using graph_doubles::IndexedFactory;
using graph_doubles::Pile;
using graph_doubles::Sequence;

struct Edge;
struct Node {
  Node(std::uint32_t id_, const Sequence& s) : id(id_), sequence(s) {}
  std::uint32_t outdegree() const { return static_cast<std::uint32_t>(outedges.size()); }
  std::uint32_t indegree() const { return static_cast<std::uint32_t>(inedges.size()); }
  bool is_junction() const { return outdegree() > 1 || indegree() > 1; }
  std::uint32_t id;
  Sequence sequence;
  std::uint32_t count = 1;
  std::uint16_t coverage = 0;
  bool is_unitig = false, is_circular = false;
  Node* pair = nullptr;
  std::vector<Edge*> inedges, outedges;
  std::unordered_set<std::uint32_t> transitive;
  std::unordered_set<std::string> original_node_sequence_names;
};
struct Edge {
  Edge(std::uint32_t id_, Node* tail_, Node* head_, std::uint32_t length_) : id(id_), tail(tail_), head(head_), length(length_) {
    tail->outedges.emplace_back(this);
    head->inedges.emplace_back(this);
  }
  std::string Label() const { return tail->sequence.InflateData(0, length); }
  std::uint32_t id;
  Node* tail;
  Node* head;
  Edge* pair = nullptr;
  std::uint32_t length;
  double weight = 0;
};

struct Graph {
  IndexedFactory<Node> node_factory;
  IndexedFactory<Edge> edge_factory;
  std::vector<std::unique_ptr<Node>> nodes;
  std::vector<std::unique_ptr<Edge>> edges;
};

inline void RemoveEdges(Graph& graph, const std::unordered_set<std::uint32_t>& indices, bool remove_nodes = false) {
  auto drop = [](std::vector<Edge*>& list, Edge* e) { list.erase(std::remove(list.begin(), list.end(), e), list.end()); };
  std::unordered_set<std::uint32_t> touched;
  for (auto i : indices) {
    Edge* e = graph.edges[i].get();
    if (remove_nodes) {
      touched.emplace(e->tail->id);
      touched.emplace(e->head->id);
    }
    drop(e->tail->outedges, e);
    drop(e->head->inedges, e);
  }
  for (auto i : touched)
    if (graph.nodes[i]->outdegree() == 0 && graph.nodes[i]->indegree() == 0) graph.nodes[i].reset();
  for (auto i : indices) graph.edges[i].reset();
}

}  // namespace unitig_doubles
