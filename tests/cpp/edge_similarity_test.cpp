// TEST INFRASTRUCTURE: raven::EdgeSimilarity (include/raven_hip/graph_repr.hpp) on a graph read from a file, over doubles of
// Raven's graph whose node sequence COUNTS every access: the facade must leave that count at zero.  The graph comes in
// the input format of tests/host/edge_similarity_reference.cpp (tests/edge_sim_util.py writes both), so that
// tests/test_gpu_edge_similarity_facade.py can hold the scores against the restatement's.
//   edge_similarity_test GRAPH OUT [TILING]
//     TILING = u32 n_reads, u64 read_off[n_reads + 1], u8 bases[]; u32 n_nodes, u64 seg_off[n_nodes + 1], u32 read[],
//              u32 begin[], u32 length[], u8 strand[]: the reads and the nodes' tilings.  Without it the device reads are the
//              node sequences themselves (read i = node i) and the tiling is one whole-read segment per node.
//     OUT = f64 score[E], u64 sequence_reads
// Exits 3 when a node's sequence was read, 2 when a call of the library failed.
#include <cstdio>
#include <fstream>

#include "raven_hip/graph_repr.hpp"

namespace similarity_doubles {

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
  std::uint32_t id;
  Sequence sequence;
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

}  // namespace similarity_doubles

namespace {

using similarity_doubles::Edge;
using similarity_doubles::Graph;
using similarity_doubles::Node;
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
  std::ifstream in(argv[1], std::ios::binary);
  const u32 n = Get<u32>(in, 1)[0];
  const u64 E = Get<u64>(in, 1)[0];
  const auto tail = Get<u32>(in, E), head = Get<u32>(in, E), length = Get<u32>(in, E);
  const auto seq_off = Get<u64>(in, static_cast<std::size_t>(n) + 1);
  const auto bases = Get<u8>(in, seq_off[n]);

  Graph graph;
  graph.nodes.resize(n);
  for (u32 i = 0; i < n; ++i) {
    std::string s(seq_off[i + 1] - seq_off[i], 'A');
    for (std::size_t x = 0; x < s.size(); ++x) s[x] = "ACGT"[bases[seq_off[i] + x] & 3];
    graph.nodes[i].reset(new Node(i, similarity_doubles::Sequence(s)));
  }
  for (u32 i = 0; i < n; ++i)
    if ((i ^ 1u) < n) graph.nodes[i]->pair = graph.nodes[i ^ 1u].get();
  graph.edges.resize(E);
  for (u64 i = 0; i < E; ++i)
    if (tail[i] != 0xFFFFFFFFu) graph.edges[i].reset(new Edge(static_cast<u32>(i), graph.nodes[tail[i]].get(), graph.nodes[head[i]].get(), length[i]));
  for (u64 i = 0; i < E; ++i)
    if (graph.edges[i]) graph.edges[i]->pair = graph.edges[i ^ 1].get();

  // the reads and the tiling: the caller's, or the node sequences as they are
  u32 n_reads = n;
  std::vector<u64> read_off = seq_off, segment_off(static_cast<std::size_t>(n) + 1);
  std::vector<u8> read_bases = bases, s_strand(n, 0);
  std::vector<u32> s_read(n), s_begin(n, 0), s_length(n);
  for (u32 i = 0; i < n; ++i) {
    segment_off[i] = i;
    s_read[i] = i;
    s_length[i] = static_cast<u32>(seq_off[i + 1] - seq_off[i]);
  }
  segment_off[n] = n;
  if (argc == 4) {
    std::ifstream tin(argv[3], std::ios::binary);
    n_reads = Get<u32>(tin, 1)[0];
    read_off = Get<u64>(tin, static_cast<std::size_t>(n_reads) + 1);
    read_bases = Get<u8>(tin, read_off[n_reads]);
    if (Get<u32>(tin, 1)[0] != n) return 2;
    segment_off = Get<u64>(tin, static_cast<std::size_t>(n) + 1);
    const u64 S = segment_off[n];
    s_read = Get<u32>(tin, S), s_begin = Get<u32>(tin, S), s_length = Get<u32>(tin, S);
    s_strand = Get<u8>(tin, S);
  }

  rvn_engine* engine = nullptr;
  rvn_reads* reads = nullptr;
  rvn_tiling* tiling = nullptr;
  auto failed = [&](const char* what) {
    std::fprintf(stderr, "%s: %s\n", what, rvn_last_error());
    return 2;
  };
  if (rvn_engine_create(&engine, 15, 5, 500, 4, 100, 10000, 0) != RVN_OK) return failed("engine");
  if (rvn_reads_upload_codes(engine, read_bases.data(), read_off.data(), nullptr, n_reads, &reads) != RVN_OK) return failed("reads");
  if (rvn_tiling_from_segments(engine, reads, n, segment_off.data(), s_read.data(), s_begin.data(), s_length.data(), s_strand.data(), &tiling) != RVN_OK)
    return failed("tiling");

  int rc = 0;
  std::vector<double> similarity;
  try {
    similarity = raven::EdgeSimilarity(engine, graph, tiling, reads);
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "EdgeSimilarity: %s\n", ex.what());
    rc = 2;
  }
  rvn_tiling_destroy(tiling);
  rvn_reads_destroy(reads);
  rvn_engine_destroy(engine);
  if (rc) return rc;

  std::ofstream out(argv[2], std::ios::binary);
  Put(out, similarity);
  Put(out, std::vector<u64>{similarity_doubles::SequenceReads()});
  std::printf("edges %llu sequence reads %llu\n", static_cast<unsigned long long>(E),
              static_cast<unsigned long long>(similarity_doubles::SequenceReads()));
  if (similarity_doubles::SequenceReads() != 0) return 3;
  return out ? 0 : 1;
}
