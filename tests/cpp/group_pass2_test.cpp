// The overlap phase of raven::ConstructGraph (RavenLib/src/construct.cc:650-707) over a raven::DeviceGroup
// (include/raven_hip/multi_gpu.hpp) against the single-device path on the same input, stage by stage:
//   FindOverlapsAndCreatePiles (keeping the pass handles) -> TrimAndAnnotatePiles -> the identity filter of
//   ResolveContainedReads -> FindOverlapsAndRepetetiveRegions.
// The containment marking between the filter and the second pass is Raven's host logic: both paths mark the same piles
// (every lhs pile of a kept overlap that is type 1 in raven_doubles' rules) so that the second pass runs on invalid piles.
// Virtual ranks on the one GPU of the test box.  Prints one line per stage for tests/test_gpu_group_pass2.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "raven_doubles.hpp"
#include "raven_hip/find_overlaps.hpp"
#include "raven_hip/multi_gpu.hpp"

std::atomic<std::uint32_t> biosoup::NucleicAcid::num_objects{0};

using Sequences = std::vector<std::unique_ptr<biosoup::NucleicAcid>>;
using Lists = std::vector<std::vector<biosoup::Overlap>>;

namespace {

Sequences Load(const char* path) {
  biosoup::NucleicAcid::num_objects = 0;
  Sequences v;
  std::ifstream in(path);
  std::string line;
  while (std::getline(in, line))
    if (!line.empty()) v.emplace_back(new biosoup::NucleicAcid("r" + std::to_string(v.size()), line));
  return v;
}

bool Same(const biosoup::Overlap& a, const biosoup::Overlap& b) {
  return a.lhs_id == b.lhs_id && a.lhs_begin == b.lhs_begin && a.lhs_end == b.lhs_end && a.rhs_id == b.rhs_id &&
         a.rhs_begin == b.rhs_begin && a.rhs_end == b.rhs_end && a.score == b.score && a.strand == b.strand;
}

std::size_t DifferingLists(const Lists& a, const Lists& b) {
  if (a.size() != b.size()) return a.size() + b.size();
  std::size_t bad = 0;
  for (std::size_t i = 0; i < a.size(); ++i) {
    bool same = a[i].size() == b[i].size();
    for (std::size_t j = 0; same && j < a[i].size(); ++j) same = Same(a[i][j], b[i][j]);
    bad += same ? 0 : 1;
  }
  return bad;
}

std::size_t DifferingPiles(const raven_double::Piles& a, const raven_double::Piles& b) {
  std::size_t bad = 0;
  for (std::size_t i = 0; i < a.size(); ++i) {
    const auto &x = *a[i], &y = *b[i];
    bad += (x.data == y.data && x.begin_ == y.begin_ && x.end_ == y.end_ && x.median_ == y.median_ && x.invalid == y.invalid &&
            x.contained == y.contained && x.chimeric_regions == y.chimeric_regions && x.kmers == y.kmers)
               ? 0
               : 1;
  }
  return bad;
}

// the single-device identity filter: rvn_filter_overlaps_by_identity on one engine (what the group call must equal)
void SingleFilter(ram::MinimizerEngine& engine, const Sequences& sequences, const raven_double::Piles& piles, Lists& overlaps,
                  double identity) {
  const std::size_t n = sequences.size();
  std::vector<std::uint32_t> begin(n), end(n), off(n + 1, 0);
  std::vector<std::uint8_t> invalid(n);
  std::vector<rvn_overlap> flat;
  for (std::size_t i = 0; i < n; ++i) {
    begin[i] = piles[i]->begin();
    end[i] = piles[i]->end();
    invalid[i] = piles[i]->is_invalid() ? 1 : 0;
    for (const auto& o : overlaps[i]) flat.push_back(raven::detail::FromOverlap(o));
    off[i + 1] = static_cast<std::uint32_t>(flat.size());
  }
  ram::detail::ReadsHandle reads;
  reads.Upload(engine.handle(), sequences.begin(), sequences.end());
  ram::detail::Check(rvn_filter_overlaps_by_identity(engine.handle(), reads.h, flat.data(), off.data(), begin.data(),
                                                     end.data(), invalid.data(), identity));
  for (std::size_t i = 0; i < n; ++i) {
    overlaps[i].clear();
    for (std::uint32_t j = off[i]; j < off[i + 1]; ++j) overlaps[i].emplace_back(ram::detail::ToOverlap(flat[j]));
  }
}

void MarkContained(raven_double::Piles& piles, Lists& overlaps) {
  for (auto& list : overlaps)
    for (auto o : list)
      if (raven_double::OverlapUpdate(o, piles) && raven_double::GetOverlapType(o, piles) == 1) {
        piles[o.lhs_id]->set_is_contained();
        piles[o.lhs_id]->set_is_invalid();
      }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  try {
    auto sequences = Load(argv[1]);
    const int n_ranks = std::atoi(argv[2]);
    const double identity = std::atof(argv[3]);
    const std::uint64_t batch_bases = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : (1ULL << 30);
    const std::size_t n = sequences.size();
    raven_double::Piles p1, p2;
    Lists o1(n), o2(n);
    ram::MinimizerEngine engine{nullptr, 15, 5};
    raven::DeviceGroup group(std::vector<int>(n_ranks, 0));
    {
      raven::Pass1Handle h1;
      raven::FindOverlapsAndCreatePiles<raven_double::Pile>(nullptr, engine, sequences, 0.001, p1, o1, 32, false,
                                                            1ULL << 32, 1ULL << 30, &h1);
      raven::TrimAndAnnotatePiles(nullptr, p1, o1, h1);
    }
    {
      raven::GroupPass1Handles h2;
      raven::FindOverlapsAndCreatePiles<raven_double::Pile>(nullptr, group, sequences, 0.001, p2, o2, h2, 32, false);
      raven::TrimAndAnnotatePiles(nullptr, p2, o2, h2);
    }
    std::size_t n_invalid = 0;
    for (const auto& p : p1) n_invalid += p->is_invalid() ? 1 : 0;
    std::printf("ranks %u trim differing_piles %zu differing_lists %zu invalid %zu\n", group.size(), DifferingPiles(p1, p2),
                DifferingLists(o1, o2), n_invalid);
    std::size_t before = 0, after = 0;
    for (const auto& l : o1) before += l.size();
    if (identity != 0) SingleFilter(engine, sequences, p1, o1, identity);
    raven::FilterOverlapsByIdentity(group, sequences, p2, o2, identity);
    for (const auto& l : o1) after += l.size();
    std::printf("filter differing_lists %zu before %zu after %zu\n", DifferingLists(o1, o2), before, after);
    MarkContained(p1, o1);
    MarkContained(p2, o2);
    raven::FindOverlapsAndRepetetiveRegions<raven_double::Pile>(nullptr, engine, 0.001, 15, identity, p1, o1, sequences,
                                                                batch_bases);
    raven::FindOverlapsAndRepetetiveRegions<raven_double::Pile>(nullptr, group, 0.001, 15, identity, p2, o2, sequences,
                                                                batch_bases);
    std::size_t kmer_cells = 0;
    for (const auto& p : p1)
      for (auto c : p->kmers) kmer_cells += c;
    std::printf("pass2 overlaps %zu kmer_cells %zu differing_piles %zu differing_lists %zu\n", o1.back().size(), kmer_cells,
                DifferingPiles(p1, p2), DifferingLists(o1, o2));
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  return 0;
}
