// TEST DOUBLE (tests/cpp only) of raven::Pile as far as stage -5 of raven::ConstructGraph touches it once
// ResolveContainedReads and ResolveChimericSequences run on the device: state, the pile.h accessors and the hooks that
// include/raven_hip/find_overlaps.hpp asks for.  No rule of pile.cc or overlap_utils.cc is restated
// here: the stage program (resolve_stage_test.cpp) has none left to run on the host.
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

namespace resolve_double {

struct Pile {
  Pile(std::uint32_t id_, std::uint32_t len) : id(id_), data(len >> 4, 0), begin_(0), end_(len >> 4) {}
  // hooks of include/raven_hip/find_overlaps.hpp
  void AdoptCoverage(const std::uint16_t* d, std::size_t n) { data.assign(d, d + n); }
  void AdoptAnnotation(std::uint32_t b, std::uint32_t e, std::uint16_t m, bool inv) {
    begin_ = b;
    end_ = e;
    median_ = m;
    if (inv) invalid = true;
  }
  void AdoptChimericRegions(const std::uint32_t* pairs, std::size_t n) {
    regions.clear();
    for (std::size_t i = 0; i < n; ++i) regions.emplace_back(pairs[2 * i], pairs[2 * i + 1]);
  }
  const std::vector<std::uint16_t>& coverage() const { return data; }
  const std::vector<std::pair<std::uint32_t, std::uint32_t>>& chimeric_regions() const { return regions; }
  // pile.h accessors
  std::uint32_t begin() const { return begin_ << 4; }
  std::uint32_t end() const { return end_ << 4; }
  std::uint16_t median() const { return median_; }
  bool is_invalid() const { return invalid; }
  bool is_contained() const { return contained; }
  bool is_chimeric() const { return chimeric; }
  void set_is_invalid() { invalid = true; }
  void set_is_contained() { contained = true; }
  void set_is_chimeric() { chimeric = true; }

  std::uint32_t id;
  std::vector<std::uint16_t> data;
  std::vector<std::pair<std::uint32_t, std::uint32_t>> regions;
  std::uint32_t begin_, end_;
  std::uint16_t median_ = 0;
  bool invalid = false, contained = false, chimeric = false;
};

using Piles = std::vector<std::unique_ptr<Pile>>;

}  // namespace resolve_double
