// Stage -5 of raven::ConstructGraph (RavenLib/src/construct.cc:661-676) with every step on the device, through the facades
// of include/raven_hip/find_overlaps.hpp in the reference's order:
//   FindOverlapsAndCreatePiles -> TrimAndAnnotatePiles -> ResolveContainedReads -> ResolveChimericSequences
//   resolve_stage_test READS IDENTITY RESIDENT
// RESIDENT = 0: the two Resolve functions take the piles' host state (the reference's signatures); 1: they take the
// Pass1Handle and run on the lists and the coverage the first pass left in HBM.  Prints the pile dump and the list sizes
// after each of the two functions; tests/test_gpu_resolve.py compares them with the restatement's.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "raven_hip/find_overlaps.hpp"
#include "resolve_doubles.hpp"

std::atomic<std::uint32_t> biosoup::NucleicAcid::num_objects{0};

namespace {

using resolve_double::Pile;
using Sequences = std::vector<std::unique_ptr<biosoup::NucleicAcid>>;
using Overlaps = std::vector<std::vector<biosoup::Overlap>>;

void Dump(const char* tag, const resolve_double::Piles& piles, const Overlaps& overlaps) {
  for (const auto& p : piles) {
    std::uint64_t h = 0;
    for (auto v : p->data) h = h * 1000003ULL + v;
    std::printf("%s %u %u %u %u %d %d %d %zu %llu %zu\n", tag, p->id, p->begin_, p->end_, p->median_, p->invalid ? 1 : 0,
                p->contained ? 1 : 0, p->chimeric ? 1 : 0, p->regions.size(), static_cast<unsigned long long>(h),
                p->id < overlaps.size() ? overlaps[p->id].size() : static_cast<std::size_t>(0));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: resolve_stage_test READS IDENTITY RESIDENT\n");
    return 2;
  }
  try {
    Sequences sequences;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line))
      if (!line.empty()) sequences.emplace_back(new biosoup::NucleicAcid("r" + std::to_string(sequences.size()), line));
    const double identity = std::atof(argv[2]);
    const bool resident = std::atoi(argv[3]) != 0;

    ram::MinimizerEngine minimizer_engine{nullptr, 15, 5};
    Overlaps overlaps(sequences.size());
    resolve_double::Piles piles;
    raven::Pass1Handle pass;
    raven::FindOverlapsAndCreatePiles<Pile>(nullptr, minimizer_engine, sequences, 0.001, piles, overlaps, 32, false,
                                            1ULL << 32, 1ULL << 30, &pass);
    raven::TrimAndAnnotatePiles<Pile>(nullptr, piles, overlaps, pass);
    if (resident) raven::ResolveContainedReads<Pile>(piles, overlaps, sequences, nullptr, identity, pass);
    else raven::ResolveContainedReads<Pile>(piles, overlaps, sequences, nullptr, identity);
    Dump("C", piles, overlaps);
    std::size_t left = 0;
    for (const auto& it : overlaps) left += it.size();
    std::printf("resolved overlaps %zu\n", left);
    if (resident) raven::ResolveChimericSequences<Pile>(nullptr, piles, overlaps, sequences, pass);
    else raven::ResolveChimericSequences<Pile>(nullptr, piles, overlaps, sequences);
    Dump("D", piles, overlaps);
    std::printf("lists %zu\n", overlaps.size());
  } catch (const std::exception& ex) {
    std::printf("error: %s\n", ex.what());
    return 1;
  }
  return 0;
}
