// TEST INFRASTRUCTURE: the host build of raven_amd/csrc/graph_rules.h (with overlap_rules.h's overlap_finalize), in the
// file formats of graph_reference.cpp, for the CPU tests that compare the two (tests/test_graph_rules.py):
//   graph_rules_host construct IN OUT    the construct OUT of graph_reference.cpp up to the finalized overlaps (no MARKS)
//   graph_rules_host comparable IN OUT   verdict[i] = is_transitive(len_j, len_k, len_c)
//   graph_rules_host long IN OUT         IN = u64 n, n x (f64 min_other, f64 weight);  OUT = u8 is_long_edge[n]
#include <fstream>
#include <string>
#include <vector>

#include "graph_rules.h"

using namespace rvn;

namespace {

template <typename T>
void Get(std::ifstream& in, T* p, std::size_t n) {
  in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input");
}
template <typename T>
void Put(std::ofstream& out, const T* p, std::size_t n) {
  out.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
}

int Construct(std::ifstream& in, std::ofstream& out) {
  u32 n = 0;
  u64 m = 0;
  Get(in, &n, 1);
  Get(in, &m, 1);
  std::vector<Overlap> overlaps(m);
  Get(in, overlaps.data(), m);
  std::vector<u32> begin(n), end(n);
  std::vector<u16> median(n);
  std::vector<u8> invalid(n);
  Get(in, begin.data(), n);
  Get(in, end.data(), n);
  Get(in, median.data(), n);
  Get(in, invalid.data(), n);
  std::vector<i32> sequence_to_node(n, -1);
  std::vector<u32> node_pile;
  std::vector<u16> coverage;
  std::vector<PileRegion> reg(n);
  for (u32 i = 0; i < n; ++i) {
    reg[i] = PileRegion{begin[i], end[i], invalid[i] ? 1u : 0u};
    if (invalid[i]) continue;
    sequence_to_node[i] = static_cast<i32>(node_pile.size());
    for (int s = 0; s < 2; ++s) {
      node_pile.push_back(i);
      coverage.push_back(median[i]);
    }
  }
  std::vector<u32> tail, head, length;
  std::vector<u64> edge_overlap;
  std::vector<Overlap> finalized;
  for (u64 x = 0; x < m; ++x) {
    Overlap f = overlaps[x];
    const PileRegion &L = reg[f.lhs_id], &R = reg[f.rhs_id];
    if (!overlap_finalize(f, L, R)) continue;
    if (L.invalid || R.invalid) return 3;
    const EdgeRecord r = edge_record(f, static_cast<u32>(sequence_to_node[f.lhs_id]), static_cast<u32>(sequence_to_node[f.rhs_id]),
                                     L.end - L.begin, R.end - R.begin);
    tail.push_back(r.tail);
    head.push_back(r.head);
    length.push_back(r.length);
    tail.push_back(r.head ^ 1u);
    head.push_back(r.tail ^ 1u);
    length.push_back(r.length_pair);
    edge_overlap.push_back(x);
    finalized.push_back(f);
  }
  const u32 n_nodes = static_cast<u32>(node_pile.size());
  const u64 n_edges = tail.size();
  Put(out, &n_nodes, 1);
  Put(out, &n_edges, 1);
  Put(out, sequence_to_node.data(), n);
  Put(out, node_pile.data(), n_nodes);
  Put(out, coverage.data(), n_nodes);
  Put(out, tail.data(), n_edges);
  Put(out, head.data(), n_edges);
  Put(out, length.data(), n_edges);
  Put(out, edge_overlap.data(), edge_overlap.size());
  Put(out, finalized.data(), finalized.size());
  return 0;
}

int Comparable(std::ifstream& in, std::ofstream& out) {
  u64 n = 0;
  Get(in, &n, 1);
  std::vector<u32> t(3 * n);
  Get(in, t.data(), t.size());
  std::vector<u8> verdict(n);
  for (u64 i = 0; i < n; ++i) verdict[i] = is_transitive(t[3 * i], t[3 * i + 1], t[3 * i + 2]) ? 1 : 0;
  Put(out, verdict.data(), n);
  return 0;
}

int Long(std::ifstream& in, std::ofstream& out) {
  u64 n = 0;
  Get(in, &n, 1);
  std::vector<double> w(2 * n);
  Get(in, w.data(), w.size());
  std::vector<u8> verdict(n);
  for (u64 i = 0; i < n; ++i) verdict[i] = is_long_edge(w[2 * i], w[2 * i + 1]) ? 1 : 0;
  Put(out, verdict.data(), n);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::ifstream in(argv[2], std::ios::binary);
  std::ofstream out(argv[3], std::ios::binary);
  int rc = 2;
  if (mode == "construct") rc = Construct(in, out);
  else if (mode == "comparable") rc = Comparable(in, out);
  else if (mode == "long") rc = Long(in, out);
  if (rc) return rc;
  return out ? 0 : 1;
}
