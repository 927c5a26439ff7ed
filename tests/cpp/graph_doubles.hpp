// TEST DOUBLES (tests/cpp only) of what include/raven_hip/assembly_graph.hpp touches of Raven itself: a sequence with
// InflateData / ReverseAndComplement, a pile's accessors, raven::Graph with its indexed factories (graph.h:55-193), Node,
// Edge and RemoveEdges (common.cc:5-30).  A Raven build uses its own; these exist so that the reference's call order can
// be exercised through the facade without the reference tree.
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

namespace graph_doubles {

struct Sequence {
  Sequence(const std::string& name_, const std::string& data_) : name(name_), data(data_) {}
  std::string InflateData(std::uint32_t i = 0, std::uint32_t len = 0xFFFFFFFFu) const { return i < data.size() ? data.substr(i, len) : std::string(); }
  void ReverseAndComplement() {
    std::reverse(data.begin(), data.end());
    for (auto& c : data) c = c == 'A' ? 'T' : (c == 'C' ? 'G' : (c == 'G' ? 'C' : 'A'));
  }
  std::string name, data;
};

struct Pile {
  std::uint32_t id_ = 0, begin_ = 0, end_ = 0;  // bases
  std::uint16_t median_ = 0;
  bool invalid_ = false;
  std::uint32_t id() const { return id_; }
  std::uint32_t begin() const { return begin_; }
  std::uint32_t end() const { return end_; }
  std::uint32_t length() const { return end_ - begin_; }
  std::uint16_t median() const { return median_; }
  bool is_invalid() const { return invalid_; }
};

struct Edge;
struct Node {
  Node(std::uint32_t id_, const Sequence& s) : id(id_), sequence(s) {}
  std::uint32_t outdegree() const { return static_cast<std::uint32_t>(outedges.size()); }
  std::uint32_t indegree() const { return static_cast<std::uint32_t>(inedges.size()); }
  std::uint32_t id;
  Sequence sequence;
  std::uint16_t coverage = 0;
  Node* pair = nullptr;
  std::vector<Edge*> inedges, outedges;
  std::unordered_set<std::uint32_t> transitive;
};
struct Edge {
  Edge(std::uint32_t id_, Node* tail_, Node* head_, std::uint32_t length_) : id(id_), tail(tail_), head(head_), length(length_) {
    tail->outedges.emplace_back(this);
    head->inedges.emplace_back(this);
  }
  std::uint32_t id;
  Node* tail;
  Node* head;
  Edge* pair = nullptr;
  std::uint32_t length;
  double weight = 0;
};

template <typename T>
struct IndexedFactory {
  std::uint32_t NextIndex() const { return next; }
  template <typename... Args>
  std::unique_ptr<T> MakeUnique(Args&&... args) {
    return std::unique_ptr<T>(new T(next++, std::forward<Args>(args)...));
  }
  std::uint32_t next = 0;
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

}  // namespace graph_doubles
