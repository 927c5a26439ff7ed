// ResolveRepeatInducedOverlaps (construct.cc:493-559) with the pieces the device runs — raven_amd/csrc/repeats.h and
// overlap_rules.h, the __host__ __device__ code of repeats.hip, compiled here for the host — on an input in the format
// of tests/host/repeats_reference.cpp: find_repetitive_regions as lane 0 runs it (a first try, then exactly the room
// the pile counted), repeat_update_hits over every overlap before any repeat_check_hits, overlap_type for the edges.
// What is the device's own (union-find, radix sort, compaction) is stated plainly here: a component search by
// relabelling, a sorted vector for the median, a copy of the survivors.  Regions are rebuilt from nothing in every
// iteration, as repeats.hip does.  Without overlaps every valid pile is a component of its own, judged with its own
// median.  Writes the same output format, so that the CPU suite compares the shared headers with the restatement
// without a GPU.
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "overlap_rules.h"
#include "repeats.h"

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

}  // namespace

int main(int argc, char** argv) {
  using namespace rvn;
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  std::uint32_t n = 0;
  std::uint64_t m = 0;
  Get(in, &n, 1);
  Get(in, &m, 1);
  std::vector<Overlap> overlaps(m);
  Get(in, overlaps.data(), m);
  std::vector<std::uint64_t> coff(n + 1), koff(n + 1);
  Get(in, coff.data(), n + 1);
  std::vector<std::uint16_t> cov(coff[n]);
  Get(in, cov.data(), cov.size());
  Get(in, koff.data(), n + 1);
  std::vector<std::uint8_t> kmers(koff[n]);
  Get(in, kmers.data(), kmers.size());
  std::vector<std::uint32_t> begin(n), end(n);
  std::vector<std::uint16_t> median(n);
  std::vector<std::uint8_t> invalid(n);
  Get(in, begin.data(), n);
  Get(in, end.data(), n);
  Get(in, median.data(), n);
  Get(in, invalid.data(), n);

  std::vector<PileRegion> reg(n);
  for (std::uint32_t i = 0; i < n; ++i) reg[i] = PileRegion{begin[i], end[i], invalid[i] ? 1u : 0u};
  std::vector<std::vector<std::uint32_t>> regions(n);  // (first, second) pairs of every pile
  std::vector<std::uint8_t> isrep(n, 0);
  std::uint32_t iterations = 0, components = 0;
  std::uint64_t removed = 0;
  for (;;) {
    ++iterations;
    // components: the smallest pile id reachable over overlaps of type > 2, by relabelling until nothing changes
    std::vector<std::uint32_t> comp(n);
    for (std::uint32_t i = 0; i < n; ++i) comp[i] = i;
    for (bool changed = true; changed;) {
      changed = false;
      for (const Overlap& o : overlaps) {
        if (overlap_type(o, reg[o.lhs_id], reg[o.rhs_id]) <= 2) continue;
        const std::uint32_t c = std::min(comp[o.lhs_id], comp[o.rhs_id]);
        if (comp[o.lhs_id] != c || comp[o.rhs_id] != c) changed = true;
        comp[o.lhs_id] = comp[o.rhs_id] = c;
      }
    }
    std::vector<std::uint8_t> has_valid(n, 0);
    for (std::uint32_t i = 0; i < n; ++i)
      if (!invalid[i]) has_valid[comp[i]] = 1;
    std::vector<std::vector<std::uint16_t>> medians(n);
    for (std::uint32_t i = 0; i < n; ++i)
      if (has_valid[comp[i]]) medians[comp[i]].push_back(median[i]);
    std::uint32_t count = 0;
    for (std::uint32_t c = 0; c < n; ++c) {
      if (medians[c].empty()) continue;
      ++count;
      std::sort(medians[c].begin(), medians[c].end());
    }
    if (iterations == 1) components = count;
    for (std::uint32_t i = 0; i < n; ++i) {
      regions[i].clear();
      if (!has_valid[comp[i]]) continue;
      const std::uint16_t med = medians[comp[i]][medians[comp[i]].size() / 2];
      const std::uint32_t len = static_cast<std::uint32_t>(coff[i + 1] - coff[i]);
      std::vector<SlopeRegion> slopes(2 * static_cast<std::size_t>(len) + 2);
      std::vector<std::uint16_t> tmp(static_cast<std::size_t>(len) + 1);
      std::uint32_t cap = 8, raw = 0;
      std::vector<std::uint32_t> out;
      std::uint32_t c = 0;
      for (;;) {  // as the device does: a first try, then exactly the room the pile counted
        out.assign(2 * static_cast<std::size_t>(cap) + 2, 0);
        bool overflow = false;
        c = find_repetitive_regions(cov.data() + coff[i], len, kmers.data() + koff[i],
                                    static_cast<std::uint32_t>(koff[i + 1] - koff[i]), begin[i] >> 4, end[i] >> 4, med,
                                    slopes.data(), tmp.data(), out.data(), cap, &raw, &overflow);
        if (overflow) return 3;
        if (raw <= cap) break;
        cap = raw;
      }
      if (raw) isrep[i] = 1;
      regions[i].assign(out.begin(), out.begin() + 2 * c);
    }
    // UpdateRepetitiveRegions of both piles of every overlap (once when lhs == rhs: the lhs coordinates both times)
    for (const Overlap& o : overlaps) {
      for (int side = 0; side < 2; ++side) {
        if (side == 1 && o.rhs_id == o.lhs_id) break;
        const std::uint32_t p = side ? o.rhs_id : o.lhs_id;
        const std::uint32_t ob = side ? o.rhs_begin : o.lhs_begin, oe = side ? o.rhs_end : o.lhs_end;
        std::vector<std::uint32_t>& r = regions[p];
        for (std::size_t k = 0; k < r.size(); k += 2)
          if (repeat_update_hits(r[k], r[k + 1], ob, oe, begin[p] >> 4, end[p] >> 4)) r[k] |= 1u;
      }
    }
    // CheckRepetitiveRegions of lhs, then of rhs; the survivors in order
    std::vector<Overlap> kept;
    for (const Overlap& o : overlaps) {
      bool hit = false;
      for (int side = 0; side < 2 && !hit; ++side) {
        const std::uint32_t p = side ? o.rhs_id : o.lhs_id;
        const bool lhs = p == o.lhs_id;
        const std::uint32_t ob = lhs ? o.lhs_begin : o.rhs_begin, oe = lhs ? o.lhs_end : o.rhs_end;
        const std::vector<std::uint32_t>& r = regions[p];
        for (std::size_t k = 0; k < r.size() && !hit; k += 2)
          hit = repeat_check_hits(r[k], r[k + 1], ob, oe, begin[p] >> 4, end[p] >> 4);
      }
      if (!hit) kept.push_back(o);
    }
    if (kept.size() == overlaps.size()) break;
    removed += overlaps.size() - kept.size();
    overlaps.swap(kept);
  }
  std::vector<std::uint32_t> roff(n + 1, 0), flat;
  for (std::uint32_t i = 0; i < n; ++i) {
    flat.insert(flat.end(), regions[i].begin(), regions[i].end());
    roff[i + 1] = static_cast<std::uint32_t>(flat.size() / 2);
  }

  std::ofstream out(argv[2], std::ios::binary);
  const std::uint64_t m_out = overlaps.size();
  Put(out, &iterations, 1);
  Put(out, &components, 1);
  Put(out, &removed, 1);
  Put(out, &m_out, 1);
  Put(out, overlaps.data(), overlaps.size());
  Put(out, roff.data(), roff.size());
  Put(out, flat.data(), flat.size());
  Put(out, isrep.data(), isrep.size());
  return out ? 0 : 1;
}
