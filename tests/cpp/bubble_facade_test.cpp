// TEST INFRASTRUCTURE: raven::RemoveBubbles (include/raven_hip/bubbles.hpp) on a graph read from a file, over doubles of
// Raven's graph whose node sequence COUNTS every access: the facade must leave that count at zero.  The graph comes in
// the input format of tests/host/bubble_reference.cpp (tests/bubble_util.py writes both), so that tests/test_gpu_bubble_facade.py
// can hold the result against the restatement's: the return value, the surviving nodes and edges, the counters.
//   bubble_facade_test IN OUT [sites]      (sites: also the launches per kernel site of the edit-distance stage, on stdout)
//     OUT = u32 popped, u64 n_junctions, u64 n_checked, u64 n_predicted, u64 n_misses, u8 node_alive[n_nodes],
//           u8 edge_alive[E], u64 sequence_reads
// The device reads are the node sequences themselves (read i = node i), the tiling one whole-read segment per node.
// Exits 3 when a node's sequence was read, 2 when a call of the library failed.
#include <cstdio>
#include <fstream>

#include "raven_hip/bubbles.hpp"

// what the facade touches of Raven's graph (graph.h:127-193, common.cc:5-30), in the manner of graph_doubles.hpp
namespace bubble_doubles {

inline std::uint64_t& SequenceReads() {
  static std::uint64_t n = 0;
  return n;
}
class Sequence {  // the node's bases, behind an accessor that counts
 public:
  explicit Sequence(const std::string& data) : data_(data) {}
  std::string InflateData(std::uint32_t i = 0, std::uint32_t len = 0xFFFFFFFFu) const {
    ++SequenceReads();
    return i < data_.size() ? data_.substr(i, len) : std::string();
  }

 private:
  std::string data_;
};

struct Edge;
struct Node {
  Node(std::uint32_t id_, const Sequence& s) : id(id_), sequence(s) {}
  std::uint32_t outdegree() const { return static_cast<std::uint32_t>(outedges.size()); }
  std::uint32_t indegree() const { return static_cast<std::uint32_t>(inedges.size()); }
  std::uint32_t id;
  Sequence sequence;
  std::uint32_t count = 1;
  Node* pair = nullptr;
  std::vector<Edge*> inedges, outedges;
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
};
struct Graph {
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

}  // namespace bubble_doubles

namespace {

using bubble_doubles::Edge;
using bubble_doubles::Graph;
using bubble_doubles::Node;
using u8 = std::uint8_t;
using u32 = std::uint32_t;
using u64 = std::uint64_t;

template <typename T>
std::vector<T> Get(std::ifstream& in, std::size_t n) {
  std::vector<T> v(n);
  if (n) in.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input");
  return v;
}
template <typename T>
void Put(std::ofstream& out, const std::vector<T>& v) {
  out.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) return 2;
  const bool sites = argc == 4;
  std::ifstream in(argv[1], std::ios::binary);
  const u32 n = Get<u32>(in, 1)[0];
  const u64 E = Get<u64>(in, 1)[0];
  const auto tail = Get<u32>(in, E), head = Get<u32>(in, E), length = Get<u32>(in, E);
  const auto present = Get<u8>(in, n);
  const auto count = Get<u32>(in, n);
  const auto seq_off = Get<u64>(in, static_cast<std::size_t>(n) + 1);
  const auto bases = Get<u8>(in, seq_off[n]);

  Graph graph;
  graph.nodes.resize(n);
  for (u32 i = 0; i < n; ++i) {
    if (!present[i]) continue;
    std::string s(seq_off[i + 1] - seq_off[i], 'A');
    for (std::size_t x = 0; x < s.size(); ++x) s[x] = "ACGT"[bases[seq_off[i] + x] & 3];
    graph.nodes[i].reset(new Node(i, bubble_doubles::Sequence(s)));
    graph.nodes[i]->count = count[i];
  }
  for (u32 i = 0; i < n; ++i)
    if (graph.nodes[i] && (i ^ 1u) < n) graph.nodes[i]->pair = graph.nodes[i ^ 1u].get();
  graph.edges.resize(E);
  for (u64 i = 0; i < E; ++i)
    if (tail[i] != 0xFFFFFFFFu) graph.edges[i].reset(new Edge(static_cast<u32>(i), graph.nodes[tail[i]].get(), graph.nodes[head[i]].get(), length[i]));
  for (u64 i = 0; i < E; ++i)
    if (graph.edges[i]) graph.edges[i]->pair = graph.edges[i ^ 1].get();

  rvn_engine* engine = nullptr;
  rvn_reads* reads = nullptr;
  rvn_tiling* tiling = nullptr;
  auto failed = [&](const char* what) {
    std::fprintf(stderr, "%s: %s\n", what, rvn_last_error());
    return 2;
  };
  if (rvn_engine_create(&engine, 15, 5, 500, 4, 100, 10000, 0) != RVN_OK) return failed("engine");
  if (rvn_reads_upload_codes(engine, bases.data(), seq_off.data(), nullptr, n, &reads) != RVN_OK) return failed("reads");
  std::vector<u64> segment_off(static_cast<std::size_t>(n) + 1);
  std::vector<u32> s_read(n), s_begin(n, 0), s_length(n);
  std::vector<u8> s_strand(n, 0);
  for (u32 i = 0; i < n; ++i) {
    segment_off[i] = i;
    s_read[i] = i;
    s_length[i] = static_cast<u32>(seq_off[i + 1] - seq_off[i]);
  }
  segment_off[n] = n;
  if (rvn_tiling_from_segments(engine, reads, n, segment_off.data(), s_read.data(), s_begin.data(), s_length.data(), s_strand.data(), &tiling) != RVN_OK)
    return failed("tiling");

  if (sites) rvn_engine_set_kernel_timing(engine, 1);
  int rc = 0;
  raven::BubbleStats st;
  u32 popped = 0;
  try {
    popped = raven::RemoveBubbles(graph, engine, tiling, reads, &st);
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "RemoveBubbles: %s\n", ex.what());
    rc = 2;
  }
  if (sites && rc == 0) {  // which edit-distance stage the pairs took
    const int n_sites = rvn_engine_num_kernel_sites();
    std::vector<double> ms(n_sites);
    std::vector<u64> launches(n_sites);
    if (rvn_engine_kernel_ms(engine, ms.data(), launches.data(), n_sites) != RVN_OK) return failed("kernel sites");
    std::printf("sites");
    for (int i = 0; i < n_sites; ++i)
      if (std::string(rvn_engine_kernel_site_name(i)).rfind("edit_", 0) == 0)
        std::printf(" %s %llu %.3f", rvn_engine_kernel_site_name(i), static_cast<unsigned long long>(launches[i]), ms[i]);
    std::printf("\n");
  }
  rvn_tiling_destroy(tiling);
  rvn_reads_destroy(reads);
  rvn_engine_destroy(engine);
  if (rc) return rc;

  std::ofstream out(argv[2], std::ios::binary);
  std::vector<u8> node_alive, edge_alive;
  for (const auto& v : graph.nodes) node_alive.push_back(v ? 1 : 0);
  for (const auto& e : graph.edges) edge_alive.push_back(e ? 1 : 0);
  Put(out, std::vector<u32>{popped});
  Put(out, std::vector<u64>{st.n_junctions, st.n_checked, st.n_predicted, st.n_misses});
  Put(out, node_alive), Put(out, edge_alive);
  Put(out, std::vector<u64>{bubble_doubles::SequenceReads()});
  std::printf("popped %u junctions %llu checked %llu predicted %llu misses %llu sequence reads %llu\n", popped,
              static_cast<unsigned long long>(st.n_junctions), static_cast<unsigned long long>(st.n_checked),
              static_cast<unsigned long long>(st.n_predicted), static_cast<unsigned long long>(st.n_misses),
              static_cast<unsigned long long>(bubble_doubles::SequenceReads()));
  std::printf("seconds predict %.6f loop %.6f misses %.6f\n", st.predict_seconds, st.loop_seconds, st.miss_seconds);
  if (bubble_doubles::SequenceReads() != 0) return 3;
  return out ? 0 : 1;
}
