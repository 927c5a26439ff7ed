// TEST INFRASTRUCTURE: the host build of the path rule of rvn_tiling_paths_as_reads (raven_amd/csrc/unitig_rules.h:
// path_member_keep, prefix_segments, prefix_segment, tiling_word) and of the threshold of rvn_path_similarity_batch
// (raven_amd/csrc/overlap_rules.h: identity_kmax) for the CPU tests (tests/test_bubble_rules.py).
//   bubble_rules_host paths IN OUT
//     IN  = u32 n_reads, u64 read_off[n_reads + 1], u8 bases[] (codes 0 .. 3);
//           u32 n_nodes, u64 seg_off[n_nodes + 1], u32 read[], u32 begin[], u32 length[], u8 strand[] (the tiling);
//           u32 n_paths, u64 path_off[n_paths + 1], u32 node[], u32 label[]
//     OUT = u32 length[n_paths], u64 word_off[n_paths + 1], u64 words[]
//   bubble_rules_host kmax IN OUT
//     IN  = u32 n, f64 ratio, u32 maxlen[n];  OUT = u32 kmax[n]
// The program has its own main, so it is also what a sanitizer build of the headers runs.
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "overlap_rules.h"
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

int Paths(std::ifstream& in, std::ofstream& out) {
  const u32 n_reads = Get<u32>(in, 1)[0];
  const auto read_off = Get<u64>(in, static_cast<std::size_t>(n_reads) + 1);
  const auto bases = Get<u8>(in, read_off[n_reads]);
  std::vector<u64> word_off(static_cast<std::size_t>(n_reads) + 1, 0);
  for (u32 r = 0; r < n_reads; ++r) word_off[r + 1] = word_off[r] + (read_off[r + 1] - read_off[r] + 31) / 32;
  std::vector<u64> packed(word_off[n_reads], 0);  // (no pad word: tiling_word must not need it)
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

  const u32 n_paths = Get<u32>(in, 1)[0];
  const auto path_off = Get<u64>(in, static_cast<std::size_t>(n_paths) + 1);
  const auto node = Get<u32>(in, path_off[n_paths]), label = Get<u32>(in, path_off[n_paths]);
  std::vector<u32> lens;
  std::vector<u64> out_word_off(1, 0), words;
  for (u32 p = 0; p < n_paths; ++p) {
    std::vector<Segment> pseg;
    std::vector<u32> pcum;
    u32 length = 0;
    for (u64 k = path_off[p]; k < path_off[p + 1]; ++k) {
      const u32 u = node[k];
      const u64 s0 = seg_off[u];
      const u32 n = static_cast<u32>(seg_off[u + 1] - s0);
      const u32 keep = path_member_keep(label[k], node_len[u], k + 1 == path_off[p + 1]);
      const u32 kept = prefix_segments(cum.data() + s0, n, keep);
      for (u32 i = 0; i < kept; ++i) {
        pseg.push_back(prefix_segment(seg.data() + s0, cum.data() + s0, i, keep));
        pcum.push_back(length + cum[s0 + i]);
      }
      length += keep;
    }
    lens.push_back(length);
    for (u32 first = 0; first < length; first += 32)
      words.push_back(tiling_word(pseg.data(), pcum.data(), static_cast<u32>(pseg.size()), length, first, packed.data(), word_off.data()));
    out_word_off.push_back(words.size());
  }
  Put(out, lens), Put(out, out_word_off), Put(out, words);
  return 0;
}

int Kmax(std::ifstream& in, std::ofstream& out) {
  const u32 n = Get<u32>(in, 1)[0];
  const double ratio = Get<double>(in, 1)[0];
  const auto maxlen = Get<u32>(in, n);
  std::vector<u32> k;
  for (u32 x : maxlen) k.push_back(identity_kmax(x, ratio));
  Put(out, k);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::ifstream in(argv[2], std::ios::binary);
  std::ofstream out(argv[3], std::ios::binary);
  int rc = 2;
  if (mode == "paths") rc = Paths(in, out);
  else if (mode == "kmax") rc = Kmax(in, out);
  if (rc) return rc;
  return out ? 0 : 1;
}
