// TEST DOUBLE (tests/cpp only): raven::Pile as raven::ResolveRepeatInducedOverlaps (include/raven_hip/find_overlaps.hpp)
// uses it — the members of raven_doubles.hpp's Pile plus the accessors and the adopter that INTEGRATION.md §3 adds to
// pile.h for this stage.  A Raven build uses its own pile.h.
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "raven_doubles.hpp"

namespace raven_double {

struct RepeatPile : Pile {
  using Pile::Pile;
  // accessors of Pile::data_ / kmers_ and the adopter of Pile::repetitive_regions_
  const std::vector<std::uint16_t>& coverage() const { return data; }
  std::size_t num_kmers() const { return kmers.size(); }
  bool kmer(std::size_t i) const { return kmers[i] != 0; }
  void AdoptRepetitiveRegions(const std::uint32_t* pairs, std::size_t n) {
    repetitive_regions.clear();
    for (std::size_t i = 0; i < n; ++i) repetitive_regions.emplace_back(pairs[2 * i], pairs[2 * i + 1]);
  }
  bool is_repetitive() const { return repetitive; }
  void set_is_repetitive() { repetitive = true; }

  std::vector<std::pair<std::uint32_t, std::uint32_t>> repetitive_regions;
  bool repetitive = false;
};

using RepeatPiles = std::vector<std::unique_ptr<RepeatPile>>;

}  // namespace raven_double
