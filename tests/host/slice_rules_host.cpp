// TEST INFRASTRUCTURE: the host build of the slice rule of rvn_tiling_slices_as_reads and of the edge rule of
// rvn_graph_edge_similarity (raven_amd/csrc/unitig_rules.h: slice_length, segment_slice, slice_word, edge_lhs_length,
// edge_rhs_length) for the CPU tests (tests/test_edge_similarity_rules.py).
//   slice_rules_host slices IN OUT
//     IN  = u32 n_reads, u64 read_off[n_reads + 1], u8 bases[] (codes 0 .. 3);
//           u32 n_nodes, u64 seg_off[n_nodes + 1], u32 read[], u32 begin[], u32 length[], u8 strand[] (the tiling);
//           u32 n_slices, u32 node[], u32 begin[], u32 length[]
//     OUT = u32 length[n_slices], u64 word_off[n_slices + 1], u64 words[] (slice_word),
//           u64 base_off[n_slices + 1], u8 bases[] (the same slices segment by segment: segment_slice of every segment the
//           slice touches, inflated by segment_bases)
//   slice_rules_host edges IN OUT
//     IN  = u32 n, u32 tail_length[n], u32 edge_length[n], u32 head_length[n];  OUT = u32 lhs_length[n], u32 rhs_length[n]
// The program has its own main, so it is also what a sanitizer build of the header runs.
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "unitig_rules.h"

using namespace rvn;

namespace {

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

int Slices(std::ifstream& in, std::ofstream& out) {
  const u32 n_reads = Get<u32>(in, 1)[0];
  const auto read_off = Get<u64>(in, static_cast<std::size_t>(n_reads) + 1);
  const auto bases = Get<u8>(in, read_off[n_reads]);
  std::vector<u64> word_off(static_cast<std::size_t>(n_reads) + 1, 0);
  for (u32 r = 0; r < n_reads; ++r) word_off[r + 1] = word_off[r] + (read_off[r + 1] - read_off[r] + 31) / 32;
  std::vector<u64> packed(word_off[n_reads], 0);  // (no pad word: slice_word must not need it)
  for (u32 r = 0; r < n_reads; ++r)
    for (u64 x = 0; x < read_off[r + 1] - read_off[r]; ++x)
      packed[word_off[r] + x / 32] |= static_cast<u64>(bases[read_off[r] + x] & 3u) << (2 * (x % 32));

  const u32 n_nodes = Get<u32>(in, 1)[0];
  const auto seg_off = Get<u64>(in, static_cast<std::size_t>(n_nodes) + 1);
  const u64 S = seg_off[n_nodes];
  const auto s_read = Get<u32>(in, S), s_begin = Get<u32>(in, S), s_length = Get<u32>(in, S);
  const auto s_strand = Get<u8>(in, S);
  std::vector<Segment> seg(S);
  std::vector<u32> cum(S), node_len(n_nodes, 0);
  for (u32 u = 0; u < n_nodes; ++u)
    for (u64 i = seg_off[u]; i < seg_off[u + 1]; ++i) {
      seg[i] = Segment{s_read[i], s_begin[i], s_length[i], s_strand[i]};
      cum[i] = node_len[u];
      node_len[u] += s_length[i];
    }

  const u32 n_slices = Get<u32>(in, 1)[0];
  const auto node = Get<u32>(in, n_slices), begin = Get<u32>(in, n_slices), length = Get<u32>(in, n_slices);
  std::vector<u32> lens;
  std::vector<u64> out_word_off(1, 0), words, base_off(1, 0);
  std::vector<u8> out_bases;
  for (u32 k = 0; k < n_slices; ++k) {
    const u32 u = node[k];
    const u64 s0 = seg_off[u];
    const u32 n = static_cast<u32>(seg_off[u + 1] - s0);
    const u32 L = slice_length(node_len[u], begin[k], length[k]);
    lens.push_back(L);
    for (u32 w = 0; 32ULL * w < L; ++w)
      words.push_back(slice_word(seg.data() + s0, cum.data() + s0, n, begin[k], L, w, packed.data(), word_off.data()));
    out_word_off.push_back(words.size());
    // the same bases through segment_slice: the part of every segment that lies in [begin, begin + L)
    const u64 lo = begin[k], hi = lo + L;
    for (u32 i = 0; i < n && L; ++i) {
      const u64 a = cum[s0 + i], z = a + seg[s0 + i].length;
      const u64 from = a > lo ? a : lo, to = z < hi ? z : hi;
      if (from >= to) continue;
      const Segment part = segment_slice(seg[s0 + i], static_cast<u32>(from - a), static_cast<u32>(to - from));
      for (u32 o = 0; o < part.length; ++o) out_bases.push_back(static_cast<u8>(segment_bases(part, o, 1, packed.data(), word_off.data())));
    }
    base_off.push_back(out_bases.size());
  }
  Put(out, lens), Put(out, out_word_off), Put(out, words), Put(out, base_off), Put(out, out_bases);
  return 0;
}

int Edges(std::ifstream& in, std::ofstream& out) {
  const u32 n = Get<u32>(in, 1)[0];
  const auto tail_len = Get<u32>(in, n), edge_len = Get<u32>(in, n), head_len = Get<u32>(in, n);
  std::vector<u32> lhs, rhs;
  for (u32 i = 0; i < n; ++i) {
    lhs.push_back(edge_lhs_length(tail_len[i], edge_len[i]));
    rhs.push_back(edge_rhs_length(lhs.back(), head_len[i]));
  }
  Put(out, lhs), Put(out, rhs);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::ifstream in(argv[2], std::ios::binary);
  std::ofstream out(argv[3], std::ios::binary);
  int rc = 2;
  if (mode == "slices") rc = Slices(in, out);
  else if (mode == "edges") rc = Edges(in, out);
  if (rc) return rc;
  return out ? 0 : 1;
}
