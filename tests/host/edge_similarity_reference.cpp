// The CPU statement that rvn_graph_edge_similarity and the facade include/raven_hip/graph_repr.hpp are compared with.  It
// says, in this project's own words and on one thread, what printEdgeSimilarity makes the CSV emitters compute per edge
// (RavenLib/src/graph_repr.cc:247-254): lhs = tail->sequence.InflateData(length), rhs = head->sequence.InflateData(0,
// lhs.size()), the global unit-cost edit distance of the two strings, 1 - distance / double(lhs.size()) — over node and
// edge objects with std::string sequences.  InflateData(i, len) is the one of tests/cpp/biosoup/nucleic_acid.hpp: nothing
// from i >= size on, len clamped to size - i.  The edit distance is Myers' bit-vector algorithm in 64-row blocks over whole
// columns (no band, no threshold), as tests/host/bubble_reference.cpp carries it.  tests/test_edge_similarity_rules.py pins
// it by results derived by hand.
//
//   edge_similarity_reference similarity IN OUT
//     IN  = u32 n_nodes, u64 n_edges, u32 tail[E] (0xFFFFFFFF: graph.edges[i] == nullptr), u32 head[E], u32 length[E],
//           u64 seq_off[n_nodes + 1], u8 bases[seq_off[n_nodes]] (codes 0 .. 3)
//     OUT = u32 lhs_length[E], u32 rhs_length[E], u32 distance[E], f64 score[E]; an empty slot: 0, 0, 0xFFFFFFFF, NaN
//   edge_similarity_reference distance IN OUT
//     IN  = u32 n_pairs, then per pair u64 l, u64 r, u8 a[l], u8 b[r];  OUT = u32 distance[n_pairs]
// Binary little-endian files; the loop's own time goes to stderr (tools/time_edge_similarity.py).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

using u8 = std::uint8_t;
using u32 = std::uint32_t;
using u64 = std::uint64_t;

// ---- global unit-cost edit distance: Myers' bit-vector recurrence, the pattern cut into blocks of 64 rows ----
struct Block {
  u64 plus = ~0ULL, minus = 0;  // vertical deltas +1 / -1 of the block's rows in the current column
};
// one column step of one block: `carry` is the horizontal delta that enters at its top row, the result the one that leaves
// at its bottom row
int Step(Block& b, u64 match, int carry) {
  const u64 diag = match | b.minus;
  if (carry < 0) match |= 1ULL;
  const u64 run = (((match & b.plus) + b.plus) ^ b.plus) | match;
  u64 hplus = b.minus | ~(run | b.plus);
  u64 hminus = b.plus & run;
  const int out = (hplus >> 63) ? 1 : ((hminus >> 63) ? -1 : 0);
  hplus <<= 1;
  hminus <<= 1;
  if (carry < 0) hminus |= 1ULL;
  else if (carry > 0) hplus |= 1ULL;
  b.plus = hminus | ~(diag | hplus);
  b.minus = hplus & diag;
  return out;
}
u32 Distance(const std::string& a, const std::string& b) {
  const u64 n = a.size(), m = b.size();
  if (n == 0) return static_cast<u32>(m);
  const u64 blocks = (n + 63) / 64;
  std::vector<u64> match(blocks * 4, 0);  // rows of the pattern that hold each of the four codes
  for (u64 i = 0; i < n; ++i) match[(i / 64) * 4 + (a[i] & 3)] |= 1ULL << (i % 64);
  std::vector<Block> col(blocks);
  long long bottom = static_cast<long long>(64 * blocks);  // the score under the last block's last row
  for (u64 j = 0; j < m; ++j) {
    int carry = 1;  // the first row of the matrix grows by one per column
    for (u64 k = 0; k < blocks; ++k) carry = Step(col[k], match[k * 4 + (b[j] & 3)], carry);
    bottom += carry;
  }
  // rows behind the pattern's end match nothing: take their vertical deltas off again
  const u64 used = n - 64 * (blocks - 1);
  const u64 pad = used >= 64 ? 0ULL : ~((1ULL << used) - 1ULL);
  bottom -= __builtin_popcountll(col[blocks - 1].plus & pad);
  bottom += __builtin_popcountll(col[blocks - 1].minus & pad);
  return static_cast<u32>(bottom);
}

// ---- the graph ----
struct Sequence {
  std::string bases;
  std::string InflateData(u32 i = 0, u32 len = 0xFFFFFFFFu) const {
    const u32 size = static_cast<u32>(bases.size());
    if (i >= size) return std::string();
    len = len < size - i ? len : size - i;
    return bases.substr(i, len);
  }
};
struct Vertex {
  u32 id = 0;
  Sequence sequence;
};
struct Link {
  u32 id = 0;
  Vertex* tail = nullptr;
  Vertex* head = nullptr;
  u32 length = 0;
};
struct Graph {
  std::vector<std::unique_ptr<Vertex>> nodes;
  std::vector<std::unique_ptr<Link>> edges;  // null: an empty slot
};

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

int Similarity(std::ifstream& in, std::ofstream& out) {
  const u32 n_nodes = Get<u32>(in, 1)[0];
  const u64 E = Get<u64>(in, 1)[0];
  const auto tail = Get<u32>(in, E), head = Get<u32>(in, E), length = Get<u32>(in, E);
  const auto seq_off = Get<u64>(in, static_cast<std::size_t>(n_nodes) + 1);
  const auto bases = Get<u8>(in, seq_off[n_nodes]);
  Graph graph;
  for (u32 u = 0; u < n_nodes; ++u) {
    graph.nodes.emplace_back(new Vertex());
    graph.nodes.back()->id = u;
    graph.nodes.back()->sequence.bases.assign(bases.begin() + static_cast<std::ptrdiff_t>(seq_off[u]),
                                              bases.begin() + static_cast<std::ptrdiff_t>(seq_off[u + 1]));
  }
  for (u64 i = 0; i < E; ++i) {
    if (tail[i] == 0xFFFFFFFFu) {
      graph.edges.emplace_back(nullptr);
      continue;
    }
    if (tail[i] >= n_nodes || head[i] >= n_nodes) throw std::runtime_error("an edge names an unknown node");
    graph.edges.emplace_back(new Link());
    Link& e = *graph.edges.back();
    e.id = static_cast<u32>(i);
    e.tail = graph.nodes[tail[i]].get();
    e.head = graph.nodes[head[i]].get();
    e.length = length[i];
  }
  std::vector<u32> lhs_len(E, 0), rhs_len(E, 0), distance(E, 0xFFFFFFFFu);
  std::vector<double> score(E, std::numeric_limits<double>::quiet_NaN());
  const auto t0 = std::chrono::steady_clock::now();
  for (const auto& it : graph.edges) {
    if (it == nullptr) continue;
    const std::string lhs{it->tail->sequence.InflateData(it->length)};
    const std::string rhs{it->head->sequence.InflateData(0, static_cast<u32>(lhs.size()))};
    const u32 d = Distance(lhs, rhs);
    lhs_len[it->id] = static_cast<u32>(lhs.size());
    rhs_len[it->id] = static_cast<u32>(rhs.size());
    distance[it->id] = d;
    score[it->id] = 1 - d / static_cast<double>(lhs.size());
  }
  std::fprintf(stderr, "similarity %.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  Put(out, lhs_len), Put(out, rhs_len), Put(out, distance), Put(out, score);
  return 0;
}

int Distances(std::ifstream& in, std::ofstream& out) {
  const u32 n = Get<u32>(in, 1)[0];
  std::vector<u32> d;
  for (u32 i = 0; i < n; ++i) {
    const u64 l = Get<u64>(in, 1)[0], r = Get<u64>(in, 1)[0];
    const auto a = Get<u8>(in, l), b = Get<u8>(in, r);
    d.push_back(Distance(std::string(a.begin(), a.end()), std::string(b.begin(), b.end())));
  }
  Put(out, d);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::ifstream in(argv[2], std::ios::binary);
  std::ofstream out(argv[3], std::ios::binary);
  int rc = 2;
  try {
    if (mode == "similarity") rc = Similarity(in, out);
    else if (mode == "distance") rc = Distances(in, out);
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "%s\n", ex.what());
    return 3;
  }
  if (rc) return rc;
  return out ? 0 : 1;
}
