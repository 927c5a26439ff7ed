// TEST INFRASTRUCTURE: the yardstick of the layout tests — tests/cpp/layout_restated.hpp (the reference's loop restated:
// insertion-built recursive quadtree, recursive centres and forces) run on a case file (layout_case.h), one thread.
// usage: layout_reference case.in positions.out
#include <cstdio>

#include "../cpp/layout_restated.hpp"
#include "layout_case.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const LayoutCase c = layout_case_read(argv[1]);
  std::vector<layout_restated::Vec> pos(c.n_points);
  for (std::uint32_t i = 0; i < c.n_points; ++i) pos[i] = layout_restated::Vec{c.xy[2 * i], c.xy[2 * i + 1]};
  std::vector<std::vector<double>> shots(c.snapshots.size(), std::vector<double>(2 * static_cast<size_t>(c.n_points)));
  auto keep = [&](std::uint32_t done, std::uint32_t first, std::uint32_t n) {
    for (size_t s = 0; s < c.snapshots.size(); ++s)
      if (c.snapshots[s] == done)
        for (std::uint32_t i = first; i < first + n; ++i) {
          shots[s][2 * i] = pos[i].x;
          shots[s][2 * i + 1] = pos[i].y;
        }
  };
  for (std::uint32_t k = 0; k < c.n_components; ++k) {
    const std::uint32_t first = c.off[k], n = c.off[k + 1] - first;
    keep(0, first, n);
    layout_restated::LayOut(pos, first, n, c.adj_off.data(), c.adj.data(), c.n_iterations,
                            [&](std::uint32_t done) { keep(done, first, n); });
  }
  std::FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  for (const auto& s : shots) std::fwrite(s.data(), sizeof(double), s.size(), f);
  std::fclose(f);
  return 0;
}
