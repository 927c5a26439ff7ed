// Pile::FindRepetitiveRegions(median) as the device runs it — raven_amd/csrc/repeats.h, the __host__ __device__ code
// of repeats.hip's lane-0 path, compiled here for the host — on every valid pile of an input in the format of
// tests/host/repeats_reference.cpp, with the pile's own median: what ResolveRepeatInducedOverlaps leaves when no
// overlap joins two piles (every valid pile is a component of its own, nothing is removed).  Writes the same output
// format, so that the CPU suite compares the shared header with the restatement without a GPU.
#include <cstdint>
#include <fstream>
#include <stdexcept>
#include <vector>

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

  std::vector<std::uint32_t> roff(n + 1, 0), regions;
  std::vector<std::uint8_t> isrep(n, 0);
  std::uint32_t components = 0;
  for (std::uint32_t i = 0; i < n; ++i) {
    roff[i + 1] = roff[i];
    if (invalid[i]) continue;
    ++components;
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
                                  static_cast<std::uint32_t>(koff[i + 1] - koff[i]), begin[i] >> 4, end[i] >> 4, median[i],
                                  slopes.data(), tmp.data(), out.data(), cap, &raw, &overflow);
      if (overflow) return 3;
      if (raw <= cap) break;
      cap = raw;
    }
    isrep[i] = raw ? 1 : 0;
    regions.insert(regions.end(), out.begin(), out.begin() + 2 * c);
    roff[i + 1] = roff[i] + c;
  }

  std::ofstream out(argv[2], std::ios::binary);
  const std::uint32_t iterations = 1;
  const std::uint64_t removed = 0, m_out = 0;
  Put(out, &iterations, 1);
  Put(out, &components, 1);
  Put(out, &removed, 1);
  Put(out, &m_out, 1);
  Put(out, roff.data(), roff.size());
  Put(out, regions.data(), regions.size());
  Put(out, isrep.data(), isrep.size());
  return out ? 0 : 1;
}
