// TEST INFRASTRUCTURE: the case file of the layout test programs (tests/layout_util.py writes it).  Little-endian:
//   u32 n_components, n_points, n_iterations, n_snapshots; u64 n_adj; u32 off[n_components + 1]; f64 xy[2 n_points];
//   u64 adj_off[n_points + 1]; u32 adj[n_adj]; u32 snapshot[n_snapshots] (numbers of iterations done, ascending, 0 = start)
// Output: 2 n_points doubles per snapshot, in order.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct LayoutCase {
  std::uint32_t n_components = 0, n_points = 0, n_iterations = 0;
  std::vector<std::uint32_t> off, adj, snapshots;
  std::vector<double> xy;
  std::vector<std::uint64_t> adj_off;
};

template <typename T>
inline void layout_read(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short case file\n");
    std::exit(2);
  }
}

inline LayoutCase layout_case_read(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  LayoutCase c;
  std::vector<std::uint32_t> head;
  std::vector<std::uint64_t> n_adj;
  layout_read(f, head, 4);
  layout_read(f, n_adj, 1);
  c.n_components = head[0];
  c.n_points = head[1];
  c.n_iterations = head[2];
  layout_read(f, c.off, static_cast<size_t>(c.n_components) + 1);
  layout_read(f, c.xy, 2 * static_cast<size_t>(c.n_points));
  layout_read(f, c.adj_off, static_cast<size_t>(c.n_points) + 1);
  layout_read(f, c.adj, n_adj[0]);
  layout_read(f, c.snapshots, head[3]);
  std::fclose(f);
  if (c.off.back() != c.n_points || c.adj_off.back() != n_adj[0]) {
    std::fprintf(stderr, "inconsistent case file\n");
    std::exit(2);
  }
  return c;
}
