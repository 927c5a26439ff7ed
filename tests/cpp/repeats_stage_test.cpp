// raven::ResolveRepeatInducedOverlaps through the C++ facade (include/raven_hip/find_overlaps.hpp) on the host state the
// reference holds after FindOverlapsAndRepetetiveRegions (construct.cc:690): piles (coverage, k-mer cells, valid region,
// median, validity) and overlaps.back(), read from a file in the input format of tests/host/repeats_reference.cpp.
// Writes that program's output format (the facade reports no loop counts: iterations = components = 0, removed = the
// overlaps it dropped), so that tests/test_gpu_repeats.py compares the two.
//   repeats_stage_test IN OUT
#include <fstream>
#include <stdexcept>
#include <string>

#include "raven_hip/find_overlaps.hpp"
#include "repeats_doubles.hpp"

std::atomic<std::uint32_t> biosoup::NucleicAcid::num_objects{0};

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
  if (argc != 3) return 2;
  try {
    std::ifstream in(argv[1], std::ios::binary);
    std::uint32_t n = 0;
    std::uint64_t m = 0;
    Get(in, &n, 1);
    Get(in, &m, 1);
    std::vector<rvn_overlap> flat(m);
    Get(in, flat.data(), m);
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

    raven_double::RepeatPiles piles;
    std::vector<std::unique_ptr<biosoup::NucleicAcid>> sequences;
    for (std::uint32_t i = 0; i < n; ++i) {
      piles.emplace_back(new raven_double::RepeatPile(i, static_cast<std::uint32_t>(coff[i + 1] - coff[i]) << 4));
      piles[i]->AdoptCoverage(cov.data() + coff[i], coff[i + 1] - coff[i]);
      piles[i]->AdoptAnnotation(begin[i] >> 4, end[i] >> 4, median[i], invalid[i] != 0);
      if (koff[i + 1] > koff[i]) piles[i]->AdoptKmers(kmers.data() + koff[i], koff[i + 1] - koff[i]);
    }
    std::vector<std::vector<biosoup::Overlap>> overlaps(n + 1);  // overlaps.back(): the second pass's list
    for (const auto& o : flat) overlaps.back().emplace_back(ram::detail::ToOverlap(o));

    raven::ResolveRepeatInducedOverlaps<raven_double::RepeatPile>(nullptr, piles, overlaps, sequences);

    std::ofstream out(argv[2], std::ios::binary);
    const std::uint32_t zero = 0;
    const std::uint64_t m_out = overlaps.back().size(), removed = m - m_out;
    Put(out, &zero, 1);
    Put(out, &zero, 1);
    Put(out, &removed, 1);
    Put(out, &m_out, 1);
    for (const auto& o : overlaps.back()) {
      const rvn_overlap r{o.lhs_id, o.lhs_begin, o.lhs_end, o.rhs_id, o.rhs_begin, o.rhs_end, o.score, o.strand ? 1u : 0u};
      Put(out, &r, 1);
    }
    std::vector<std::uint32_t> roff(n + 1, 0), regions;
    std::vector<std::uint8_t> isrep(n);
    for (std::uint32_t i = 0; i < n; ++i) {
      for (const auto& r : piles[i]->repetitive_regions) {
        regions.push_back(r.first);
        regions.push_back(r.second);
      }
      roff[i + 1] = static_cast<std::uint32_t>(regions.size() / 2);
      isrep[i] = piles[i]->is_repetitive() ? 1 : 0;
    }
    Put(out, roff.data(), roff.size());
    Put(out, regions.data(), regions.size());
    Put(out, isrep.data(), isrep.size());
    return out ? 0 : 1;
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
}
