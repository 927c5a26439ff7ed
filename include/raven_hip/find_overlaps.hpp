// raven_hip/find_overlaps.hpp — raven::FindOverlapsAndCreatePiles (RavenLib/src/construct.cc:14-121, decl
// RavenLib/include/raven/graph/construct.h:22-29) with the reference's signature and semantics, running the
// whole pass on the MI355X through one C-ABI call.  Header-only; see INTEGRATION.md.
//
// PileT must provide PileT(std::uint32_t id, std::uint32_t len) and
//   void AdoptCoverage(const std::uint16_t* data, std::size_t n)   // replaces Pile::data_ (n == len >> 4)
// (a two-line addition to raven::Pile; AddLayers itself is no longer called on this path).
//
// Optional: pass a raven::Pass1Handle to FindOverlapsAndCreatePiles and the coverage stays in HBM for
// raven::TrimAndAnnotatePiles(thread_pool, piles, overlaps, handle) below — construct.cc:123-152 (FindValidRegion(4),
// FindMedian, FindChimericRegions of every pile) on the device instead of Pile's host loops; PileT then also provides
//   void AdoptAnnotation(std::uint32_t begin, std::uint32_t end, std::uint16_t median, bool invalid)   // cells, as Pile::begin_ / end_
//   void AdoptChimericRegions(const std::uint32_t* pairs, std::size_t n)                                // Pile::chimeric_regions_
//
// raven::ResolveContainedReads and raven::ResolveChimericSequences (construct.cc:154-314) below run on the device too,
// on the piles' host state or — the overloads that take the Pass1Handle — on the lists and coverage the pass left in HBM.
#ifndef RAVEN_HIP_FIND_OVERLAPS_HPP_
#define RAVEN_HIP_FIND_OVERLAPS_HPP_

#include <algorithm>
#include <cstdint>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

#include "ram/minimizer_engine.hpp"

namespace raven {

// the first pass's result in HBM, kept alive between FindOverlapsAndCreatePiles and TrimAndAnnotatePiles
struct Pass1Handle {
  rvn_pass1* p = nullptr;
  rvn_engine* engine = nullptr;  // the engine of the pass (not owned): uploads the reads for an identity filter on the pass
  Pass1Handle() = default;
  Pass1Handle(const Pass1Handle&) = delete;
  Pass1Handle& operator=(const Pass1Handle&) = delete;
  ~Pass1Handle() { rvn_pass1_destroy(p); }
};

template <typename PileT>
void FindOverlapsAndCreatePiles(const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/,
                                ram::MinimizerEngine& minimizer_engine,
                                const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences, double freq,
                                std::vector<std::unique_ptr<PileT>>& piles,
                                std::vector<std::vector<biosoup::Overlap>>& overlaps,
                                std::size_t kMaxNumOverlaps = 32, bool useMinhash = false,
                                std::uint64_t index_batch_bases = 1ULL << 32, std::uint64_t flush_bases = 1ULL << 30,
                                Pass1Handle* keep = nullptr) {
  piles.reserve(sequences.size());
  for (const auto& it : sequences) piles.emplace_back(new PileT(it->id, it->inflated_len));
  if (sequences.empty()) return;
  if (overlaps.size() < sequences.size()) overlaps.resize(sequences.size());

  ram::detail::ReadsHandle reads;
  reads.Upload(minimizer_engine.handle(), sequences.begin(), sequences.end());
  rvn_pass1* p = nullptr;
  ram::detail::Check(rvn_find_overlaps_and_create_piles(minimizer_engine.handle(), reads.h, freq,
                                                        static_cast<std::uint32_t>(kMaxNumOverlaps), useMinhash,
                                                        index_batch_bases, flush_bases, &p));
  struct Guard {
    rvn_pass1* p;
    Pass1Handle* keep;
    rvn_engine* engine;
    ~Guard() {
      if (keep) {
        rvn_pass1_destroy(keep->p);
        keep->p = p;
        keep->engine = engine;
      } else {
        rvn_pass1_destroy(p);
      }
    }
  } guard{p, keep, minimizer_engine.handle()};

  const std::size_t n = sequences.size();
  std::vector<std::uint16_t> data(rvn_pass1_pile_words(p));
  std::vector<std::uint64_t> poff(n + 1);
  ram::detail::Check(rvn_pass1_fetch_piles(p, data.data(), poff.data()));
  for (std::size_t i = 0; i < n; ++i) piles[i]->AdoptCoverage(data.data() + poff[i], poff[i + 1] - poff[i]);

  std::vector<rvn_overlap> flat(rvn_pass1_num_overlaps(p));
  std::vector<std::uint32_t> ooff(n + 1);
  ram::detail::Check(rvn_pass1_fetch_overlaps(p, flat.data(), ooff.data()));
  for (std::size_t i = 0; i < n; ++i) {
    overlaps[i].clear();
    overlaps[i].reserve(ooff[i + 1] - ooff[i]);
    for (std::uint32_t j = ooff[i]; j < ooff[i + 1]; ++j) overlaps[i].emplace_back(ram::detail::ToOverlap(flat[j]));
  }
}

// raven::TrimAndAnnotatePiles (RavenLib/src/construct.cc:123-152) on the coverage arrays the first pass left in HBM:
// Pile::FindValidRegion(4) (+ UpdateValidRegion), FindMedian and FindChimericRegions of every pile in two device calls;
// overlaps[i] of an invalid pile is released as the reference does (:134-135).  The piles get their trimmed coverage,
// valid region, median, validity and chimeric regions through the Adopt* hooks (see the top of this file).
template <typename PileT>
void TrimAndAnnotatePiles(const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/,
                          const std::vector<std::unique_ptr<PileT>>& piles,
                          std::vector<std::vector<biosoup::Overlap>>& overlaps, Pass1Handle& pass) {
  const std::size_t n = piles.size();
  if (n == 0 || pass.p == nullptr) return;
  std::vector<std::uint32_t> begin(n), end(n), roff(n + 1);
  std::vector<std::uint16_t> median(n);
  std::vector<std::uint8_t> invalid(n);
  ram::detail::Check(rvn_pass1_trim_and_annotate(pass.p, 4, begin.data(), end.data(), median.data(), invalid.data()));
  std::uint32_t* regions = nullptr;
  ram::detail::Check(rvn_pass1_find_chimeric_regions(pass.p, invalid.data(), roff.data(), &regions));
  struct Free {
    void* p;
    ~Free() { rvn_free(p); }
  } free_regions{regions};
  std::vector<std::uint16_t> data(rvn_pass1_pile_words(pass.p));
  std::vector<std::uint64_t> poff(n + 1);
  ram::detail::Check(rvn_pass1_fetch_piles(pass.p, data.data(), poff.data()));
  for (std::size_t i = 0; i < n; ++i) {
    piles[i]->AdoptCoverage(data.data() + poff[i], poff[i + 1] - poff[i]);
    piles[i]->AdoptAnnotation(begin[i], end[i], median[i], invalid[i] != 0);
    piles[i]->AdoptChimericRegions(regions + 2 * static_cast<std::size_t>(roff[i]), roff[i + 1] - roff[i]);
    if (invalid[i]) std::vector<biosoup::Overlap>().swap(overlaps[i]);
  }
}

namespace detail {

using ram::detail::Check;
using ram::detail::ReadsHandle;
using ram::detail::ToOverlap;

// what rvn_resolved_fetch gives, handed to the piles and the lists: valid region, flags, remaining chimeric regions,
// coverage, overlaps[i] (phase 2 with a median: the reference's overlaps.clear(), construct.cc:310)
template <typename PileT>
void AdoptResolved(rvn_resolved* r, const std::uint16_t* coverage, const std::uint64_t* coff,
                   const std::vector<std::unique_ptr<PileT>>& piles, std::vector<std::vector<biosoup::Overlap>>& overlaps,
                   std::uint32_t phases) {
  const std::size_t n = piles.size();
  std::vector<std::uint32_t> begin(n), end(n), roff(n + 1), ooff(n + 1), regions(2 * rvn_resolved_num_regions(r));
  std::vector<std::uint8_t> invalid(n), contained(n), chimeric(n);
  std::vector<rvn_overlap> flat(rvn_resolved_num_overlaps(r));
  std::vector<std::uint16_t> own(rvn_resolved_coverage_words(r));
  std::uint16_t median = 0;
  Check(rvn_resolved_fetch(r, begin.data(), end.data(), invalid.data(), contained.data(), chimeric.data(), regions.data(),
                           roff.data(), &median, flat.data(), ooff.data(), own.data(), nullptr));
  if (!coverage) coverage = own.data();
  for (std::size_t i = 0; i < n; ++i) {
    PileT& p = *piles[i];
    p.AdoptCoverage(coverage + coff[i], coff[i + 1] - coff[i]);
    p.AdoptAnnotation(begin[i], end[i], p.median(), invalid[i] != 0);
    p.AdoptChimericRegions(regions.data() + 2 * static_cast<std::size_t>(roff[i]), roff[i + 1] - roff[i]);
    if (contained[i]) p.set_is_contained();
    if (chimeric[i]) p.set_is_chimeric();
  }
  if ((phases & 2u) && median != 0) {
    overlaps.clear();
    return;
  }
  for (std::size_t i = 0; i < n && i < overlaps.size(); ++i) {
    overlaps[i].clear();
    for (std::uint32_t j = ooff[i]; j < ooff[i + 1]; ++j) overlaps[i].emplace_back(ToOverlap(flat[j]));
    if (overlaps[i].empty()) std::vector<biosoup::Overlap>().swap(overlaps[i]);
  }
}

// the two functions on the piles' host state (rvn_resolve_contained_and_chimeric), an engine of their own on device 0
template <typename PileT>
void ResolveOnArrays(const std::vector<std::unique_ptr<PileT>>& piles, std::vector<std::vector<biosoup::Overlap>>& overlaps,
                     const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences, double identity,
                     std::uint32_t phases) {
  const std::size_t n = piles.size();
  if (n == 0) return;
  std::vector<std::uint32_t> ooff(n + 1, 0), roff(n + 1, 0), begin(n), end(n);
  std::vector<std::uint64_t> coff(n + 1, 0);
  for (std::size_t i = 0; i < n; ++i) {
    ooff[i + 1] = ooff[i] + static_cast<std::uint32_t>(i < overlaps.size() ? overlaps[i].size() : 0);
    roff[i + 1] = roff[i] + static_cast<std::uint32_t>(piles[i]->chimeric_regions().size());
    coff[i + 1] = coff[i] + piles[i]->coverage().size();
  }
  std::vector<rvn_overlap> flat(ooff[n]);
  std::vector<std::uint32_t> regions(2 * static_cast<std::size_t>(roff[n]));
  std::vector<std::uint16_t> coverage(coff[n]), median(n);
  std::vector<std::uint8_t> invalid(n);
  for (std::size_t i = 0; i < n; ++i) {
    const PileT& p = *piles[i];
    for (std::size_t j = 0; i < overlaps.size() && j < overlaps[i].size(); ++j) {
      const auto& o = overlaps[i][j];
      flat[ooff[i] + j] = rvn_overlap{o.lhs_id, o.lhs_begin, o.lhs_end, o.rhs_id, o.rhs_begin, o.rhs_end, o.score, o.strand ? 1u : 0u};
    }
    std::size_t k = 2 * static_cast<std::size_t>(roff[i]);
    for (const auto& reg : p.chimeric_regions()) {
      regions[k++] = reg.first;
      regions[k++] = reg.second;
    }
    std::copy(p.coverage().begin(), p.coverage().end(), coverage.begin() + coff[i]);
    begin[i] = p.begin() >> 4;  // Pile::begin_ / end_: cells
    end[i] = p.end() >> 4;
    median[i] = p.median();
    invalid[i] = p.is_invalid() ? 1 : 0;
  }
  struct Engine {
    rvn_engine* e = nullptr;
    ~Engine() { rvn_engine_destroy(e); }
  } engine;
  Check(rvn_engine_create(&engine.e, 15, 5, 500, 4, 100, 10000, 0));
  ReadsHandle reads;
  if (identity != 0 && (phases & 1u)) reads.Upload(engine.e, sequences.begin(), sequences.end());
  rvn_resolved* r = nullptr;
  Check(rvn_resolve_contained_and_chimeric(engine.e, reads.h, flat.data(), ooff.data(), static_cast<std::uint32_t>(n),
                                           coverage.data(), coff.data(), regions.data(), roff.data(), begin.data(),
                                           end.data(), median.data(), invalid.data(), identity, phases, &r));
  struct Guard {
    rvn_resolved* r;
    ~Guard() { rvn_resolved_destroy(r); }
  } guard{r};
  AdoptResolved<PileT>(r, nullptr, coff.data(), piles, overlaps, phases);
}

// ... on the lists and the coverage the first pass left in HBM (rvn_pass1_resolve): nothing is uploaded but the reads of
// an identity filter
template <typename PileT>
void ResolveOnPass(Pass1Handle& pass, const std::vector<std::unique_ptr<PileT>>& piles,
                   std::vector<std::vector<biosoup::Overlap>>& overlaps,
                   const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences, double identity, std::uint32_t phases) {
  const std::size_t n = piles.size();
  if (n == 0 || pass.p == nullptr) return;
  ReadsHandle reads;
  if (identity != 0 && (phases & 1u)) {
    if (!pass.engine) throw std::invalid_argument("[raven_hip] the identity filter on a pass needs the pass's engine");
    reads.Upload(pass.engine, sequences.begin(), sequences.end());
  }
  rvn_resolved* r = nullptr;
  Check(rvn_pass1_resolve(pass.p, reads.h, 4, identity, phases, &r));
  struct Guard {
    rvn_resolved* r;
    ~Guard() { rvn_resolved_destroy(r); }
  } guard{r};
  std::vector<std::uint16_t> data(rvn_pass1_pile_words(pass.p));
  std::vector<std::uint64_t> poff(n + 1);
  Check(rvn_pass1_fetch_piles(pass.p, data.data(), poff.data()));
  AdoptResolved<PileT>(r, data.data(), poff.data(), piles, overlaps, phases);
}

}  // namespace detail

// raven::ResolveContainedReads (RavenLib/src/construct.cc:154-248, decl construct.h) with the reference's signature: the
// identity filter loop when identity != 0, the containment marking of every overlap, contained piles made invalid with
// their lists emptied — one C-ABI call on the piles' host state (an engine of its own on device 0, as the signature
// names none).  overlaps[i] keeps its survivors with their updated coordinates, in order.
// PileT must provide begin(), end(), median(), is_invalid(), set_is_contained() (raven::Pile members), the hooks
// AdoptCoverage / AdoptAnnotation / AdoptChimericRegions of the top of this file, and
//   const std::vector<std::uint16_t>& coverage() const                                            // Pile::data_
//   const std::vector<std::pair<std::uint32_t, std::uint32_t>>& chimeric_regions() const         // Pile::chimeric_regions_
//   void set_is_chimeric()                                                                        // a raven::Pile member
template <typename PileT>
void ResolveContainedReads(const std::vector<std::unique_ptr<PileT>>& piles,
                           std::vector<std::vector<biosoup::Overlap>>& overlaps,
                           const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences,
                           const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/, double identity) {
  detail::ResolveOnArrays<PileT>(piles, overlaps, sequences, identity, 1);
}
// ... on the pass that FindOverlapsAndCreatePiles kept: the lists are not uploaded again
template <typename PileT>
void ResolveContainedReads(const std::vector<std::unique_ptr<PileT>>& piles,
                           std::vector<std::vector<biosoup::Overlap>>& overlaps,
                           const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences,
                           const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/, double identity,
                           Pass1Handle& pass) {
  detail::ResolveOnPass<PileT>(pass, piles, overlaps, sequences, identity, 1);
}

// raven::ResolveChimericSequences (RavenLib/src/construct.cc:250-314) with the reference's signature: the global median,
// Pile::ClearChimericRegions of every valid pile, the last OverlapUpdate / containment sweep, overlaps.clear().
// PileT: as for ResolveContainedReads, and set_is_invalid() is not needed (AdoptAnnotation carries the flag).
template <typename PileT>
void ResolveChimericSequences(const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/,
                              const std::vector<std::unique_ptr<PileT>>& piles,
                              std::vector<std::vector<biosoup::Overlap>>& overlaps,
                              const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences) {
  detail::ResolveOnArrays<PileT>(piles, overlaps, sequences, 0, 2);
}
template <typename PileT>
void ResolveChimericSequences(const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/,
                              const std::vector<std::unique_ptr<PileT>>& piles,
                              std::vector<std::vector<biosoup::Overlap>>& overlaps,
                              const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences, Pass1Handle& pass) {
  detail::ResolveOnPass<PileT>(pass, piles, overlaps, sequences, 0, 2);
}

// raven::FindOverlapsAndRepetetiveRegions (RavenLib/src/construct.cc:316-491, decl construct.h:49-54) with the
// reference's signature: the second all-vs-all pass on the valid reads, one C-ABI call.  The reference re-sorts
// `sequences` valid-first for the duration of the call and restores the id order before returning (construct.cc:324-332,
// :486-490); the device pass selects the valid reads itself, so `sequences` is left as it is (ids must equal positions,
// the invariant of construct.cc:25).  Effects, as in the reference: overlaps gets the extra slot overlaps.back(),
// contained piles are marked and set invalid, Pile::kmers_ of the valid piles is filled.
// PileT must provide begin(), end(), is_invalid(), set_is_contained(), set_is_invalid() (all raven::Pile members) and
//   void AdoptKmers(const std::uint8_t* cells, std::size_t n)      // replaces Pile::kmers_ (n == (len >> 4) + 1)
template <typename PileT>
void FindOverlapsAndRepetetiveRegions(const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/,
                                      ram::MinimizerEngine& minimizer_engine, double freq, std::uint8_t kmer_len,
                                      double identity, const std::vector<std::unique_ptr<PileT>>& piles,
                                      std::vector<std::vector<biosoup::Overlap>>& overlaps,
                                      std::vector<std::unique_ptr<biosoup::NucleicAcid>>& sequences,
                                      std::uint64_t batch_bases = 1ULL << 30) {
  const std::size_t n = sequences.size();
  overlaps.resize(n + 1);  // construct.cc:352
  if (n == 0) return;
  ram::detail::ReadsHandle reads;
  reads.Upload(minimizer_engine.handle(), sequences.begin(), sequences.end());
  std::vector<std::uint32_t> begin(n), end(n);
  std::vector<std::uint8_t> invalid(n);
  for (std::size_t i = 0; i < n; ++i) {
    begin[i] = piles[i]->begin();
    end[i] = piles[i]->end();
    invalid[i] = piles[i]->is_invalid() ? 1 : 0;
  }
  rvn_pass2* p = nullptr;
  ram::detail::Check(rvn_find_overlaps_and_repetitive_regions(minimizer_engine.handle(), reads.h, begin.data(), end.data(),
                                                              invalid.data(), freq, kmer_len, identity, batch_bases, &p));
  struct Guard {
    rvn_pass2* p;
    ~Guard() { rvn_pass2_destroy(p); }
  } guard{p};
  std::vector<rvn_overlap> flat(rvn_pass2_num_overlaps(p));
  std::vector<std::uint8_t> contained(n), kmers(rvn_pass2_kmer_cells(p));
  std::vector<std::uint64_t> koff(n + 1);
  ram::detail::Check(rvn_pass2_fetch(p, flat.data(), contained.data(), kmers.data(), koff.data()));
  for (std::size_t i = 0; i < n; ++i) {
    if (koff[i + 1] > koff[i]) piles[i]->AdoptKmers(kmers.data() + koff[i], koff[i + 1] - koff[i]);
    if (contained[i]) {  // construct.cc:438-441, :466-470
      piles[i]->set_is_contained();
      piles[i]->set_is_invalid();
    }
  }
  auto& back = overlaps.back();
  back.reserve(back.size() + flat.size());
  for (const auto& o : flat) back.emplace_back(ram::detail::ToOverlap(o));
}

// raven::ResolveRepeatInducedOverlaps (RavenLib/src/construct.cc:493-559, called at :690) with the reference's
// signature: the loop of ConnectedComponents, FindRepetitiveRegions(component median), UpdateRepetitiveRegions and the
// removal of the overlaps CheckRepetitiveRegions flags, on the device in one C-ABI call (an engine of its own on device
// 0, as the reference's signature names none).  Rewrites overlaps.back() (survivors in order) and hands every pile its
// final repetitive regions and is_repetitive flag.  `sequences` is not needed (ids equal positions, construct.cc:25).
// PileT must provide begin(), end(), median(), is_invalid(), set_is_repetitive() (all raven::Pile members) and
//   const std::vector<std::uint16_t>& coverage() const                         // Pile::data_
//   std::size_t num_kmers() const; bool kmer(std::size_t i) const             // Pile::kmers_
//   void AdoptRepetitiveRegions(const std::uint32_t* pairs, std::size_t n)    // replaces Pile::repetitive_regions_
template <typename PileT>
void ResolveRepeatInducedOverlaps(const std::shared_ptr<thread_pool::ThreadPool>& /*thread_pool*/,
                                  const std::vector<std::unique_ptr<PileT>>& piles,
                                  std::vector<std::vector<biosoup::Overlap>>& overlaps,
                                  const std::vector<std::unique_ptr<biosoup::NucleicAcid>>& /*sequences*/) {
  const std::size_t n = piles.size();
  if (overlaps.empty()) overlaps.resize(1);
  auto& back = overlaps.back();
  std::vector<rvn_overlap> flat(back.size());
  for (std::size_t i = 0; i < back.size(); ++i) {
    const auto& o = back[i];
    flat[i] = rvn_overlap{o.lhs_id, o.lhs_begin, o.lhs_end, o.rhs_id, o.rhs_begin, o.rhs_end, o.score, o.strand ? 1u : 0u};
  }
  std::vector<std::uint64_t> coff(n + 1, 0), koff(n + 1, 0);
  for (std::size_t i = 0; i < n; ++i) {
    coff[i + 1] = coff[i] + piles[i]->coverage().size();
    koff[i + 1] = koff[i] + piles[i]->num_kmers();
  }
  std::vector<std::uint16_t> coverage(coff[n]);
  std::vector<std::uint8_t> kmers(koff[n]), invalid(n);
  std::vector<std::uint32_t> begin(n), end(n);
  std::vector<std::uint16_t> median(n);
  for (std::size_t i = 0; i < n; ++i) {
    const auto& p = *piles[i];
    std::copy(p.coverage().begin(), p.coverage().end(), coverage.begin() + coff[i]);
    for (std::size_t k = 0; k < p.num_kmers(); ++k) kmers[koff[i] + k] = p.kmer(k) ? 1 : 0;
    begin[i] = p.begin();
    end[i] = p.end();
    median[i] = p.median();
    invalid[i] = p.is_invalid() ? 1 : 0;
  }
  struct Engine {
    rvn_engine* e = nullptr;
    ~Engine() { rvn_engine_destroy(e); }
  } engine;
  ram::detail::Check(rvn_engine_create(&engine.e, 15, 5, 500, 4, 100, 10000, 0));
  rvn_repeats* r = nullptr;
  ram::detail::Check(rvn_resolve_repeat_induced_overlaps(engine.e, flat.data(), flat.size(), static_cast<std::uint32_t>(n),
                                                         coverage.data(), coff.data(), kmers.data(), koff.data(),
                                                         begin.data(), end.data(), median.data(), invalid.data(), &r));
  struct Guard {
    rvn_repeats* r;
    ~Guard() { rvn_repeats_destroy(r); }
  } guard{r};
  flat.resize(rvn_repeats_num_overlaps(r));
  std::vector<std::uint32_t> regions(2 * rvn_repeats_num_regions(r)), roff(n + 1);
  std::vector<std::uint8_t> is_repetitive(n);
  ram::detail::Check(rvn_repeats_fetch(r, flat.data(), regions.data(), roff.data(), is_repetitive.data(), nullptr));
  back.clear();
  for (const auto& o : flat) back.emplace_back(ram::detail::ToOverlap(o));
  for (std::size_t i = 0; i < n; ++i) {
    piles[i]->AdoptRepetitiveRegions(regions.data() + 2 * static_cast<std::size_t>(roff[i]), roff[i + 1] - roff[i]);
    if (is_repetitive[i]) piles[i]->set_is_repetitive();
  }
}

}  // namespace raven

#endif  // RAVEN_HIP_FIND_OVERLAPS_HPP_
