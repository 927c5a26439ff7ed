// The CPU statement of raven::ResolveContainedReads and raven::ResolveChimericSequences (RavenLib/src/construct.cc:154-248,
// :250-314) that the device stage (raven_amd/csrc/resolve.hip) and the host build of chimeric.h are compared with:
// Pile::ClearChimericRegions and UpdateValidRegion (pile.cc:189-228, :144-157) restated over std::vector state,
// single-threaded, the loops in the reference's order, with the oracle's OverlapUpdate / GetOverlapType / identity score
// (oracle/raven_oracle.cpp, compiled into this program).
//
//   resolve_reference stage IN OUT    the stage: the phases and the identity threshold come from IN
//   resolve_reference piles IN OUT    Pile::ClearChimericRegions(median[i]) on every pile i that is not invalid, nothing else
// Binary little-endian files (tests/resolve_util.py).
// IN  = u32 n_piles, u32 phases, f64 identity, u32 offsets[n + 1], overlaps (8 x u32 each), u64 coverage_offsets[n + 1],
//       u16 coverage[], u32 region_offsets[n + 1], u32 regions[2 x total], u32 begin[n], u32 end[n] (cells), u16 median[n],
//       u8 invalid[n]; when identity != 0: u64 word_offsets[n + 1], u32 lengths[n], u64 packed[word_offsets[n] + 1].
// OUT = u32 begin[n], u32 end[n], u8 invalid[n], u8 contained[n], u8 chimeric[n], u32 region_offsets[n + 1],
//       u32 regions[2 x total], u16 global median, u64 n_overlaps, overlaps, u32 offsets[n + 1], u16 coverage[],
//       stats = u64 dropped_by_update[2], u64 dropped_by_filter, u64 dropped_by_containment, u32 contained[2], u32 cut,
//       u32 invalidated (rvn_resolve_stats).
#include <cstring>
#include <fstream>
#include <iostream>

#include "raven_oracle.cpp"

namespace {

using orc::Overlap;
using Region = orc::Region;
constexpr std::uint32_t kPSS = 4;

// the state of a raven::Pile that the two functions read and write (pile.h:130-141)
struct Pile {
  std::uint32_t id_ = 0, begin_ = 0, end_ = 0;
  std::uint16_t median_ = 0;
  bool is_invalid_ = false, is_contained_ = false, is_chimeric_ = false;
  std::vector<std::uint16_t> data_;
  std::vector<Region> chimeric_regions_;

  bool is_maybe_chimeric() const { return !chimeric_regions_.empty(); }

  // pile.cc:144-157
  void UpdateValidRegion(std::uint32_t begin, std::uint32_t end) {
    if (begin >= end || end - begin < 1260 >> kPSS) {
      is_invalid_ = true;
      return;
    }
    std::fill(data_.begin() + begin_, data_.begin() + begin, 0);
    std::fill(data_.begin() + end, data_.begin() + end_, 0);
    begin_ = begin;
    end_ = end;
  }

  // pile.cc:189-228
  void ClearChimericRegions(std::uint16_t median) {
    auto dips_to_median = [&](const Region& r) {
      for (std::uint32_t i = r.first; i <= r.second; ++i)
        if (orc::clamp16(data_[i] * 1.82) <= median) return true;
      return false;
    };
    std::uint32_t best_begin = 0, best_end = 0, last_cut = begin_;
    std::vector<Region> unresolved;
    for (const auto& r : chimeric_regions_) {
      if (begin_ > r.first || end_ < r.second) continue;  // leaves the valid region: dropped
      if (!dips_to_median(r)) {
        unresolved.emplace_back(r);
        continue;
      }
      if (r.first - last_cut > best_end - best_begin) {
        best_begin = last_cut;
        best_end = r.first;
      }
      last_cut = r.second;
    }
    if (end_ - last_cut > best_end - best_begin) {
      best_begin = last_cut;
      best_end = end_;
    }
    if (best_begin != begin_ || best_end != end_) is_chimeric_ = true;
    chimeric_regions_.swap(unresolved);
    UpdateValidRegion(best_begin, best_end);
  }
};

struct Stats {
  std::uint64_t dropped_by_update[2] = {0, 0}, dropped_by_filter = 0, dropped_by_containment = 0;
  std::uint32_t contained[2] = {0, 0}, cut = 0, invalidated = 0;
};

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
  if (argc != 4) return 2;
  const bool piles_only = std::strcmp(argv[1], "piles") == 0;
  std::ifstream in(argv[2], std::ios::binary);
  std::uint32_t n = 0, phases = 0;
  double identity = 0;
  Get(in, &n, 1);
  Get(in, &phases, 1);
  Get(in, &identity, 1);
  std::vector<std::uint32_t> off(n + 1), roff(n + 1), begin(n), end(n);
  Get(in, off.data(), n + 1);
  std::vector<Overlap> flat(off[n]);
  Get(in, flat.data(), flat.size());
  std::vector<std::uint64_t> coff(n + 1);
  Get(in, coff.data(), n + 1);
  std::vector<std::uint16_t> cov(coff[n]), median(n);
  Get(in, cov.data(), cov.size());
  Get(in, roff.data(), n + 1);
  std::vector<std::uint32_t> reg(2 * static_cast<std::size_t>(roff[n]));
  Get(in, reg.data(), reg.size());
  Get(in, begin.data(), n);
  Get(in, end.data(), n);
  Get(in, median.data(), n);
  std::vector<std::uint8_t> invalid(n);
  Get(in, invalid.data(), n);
  std::vector<std::uint64_t> word_off, packed;
  std::vector<std::uint32_t> lengths;
  std::vector<orc::Read> reads;
  if (identity != 0 && !piles_only) {
    word_off.resize(n + 1);
    lengths.resize(n);
    Get(in, word_off.data(), n + 1);
    Get(in, lengths.data(), n);
    packed.resize(word_off[n] + 1);
    Get(in, packed.data(), packed.size());
    reads = MakeReads(packed.data(), word_off.data(), lengths.data(), nullptr, n);
  }

  std::vector<Pile> piles(n);
  std::vector<std::vector<Overlap>> overlaps(n);
  std::vector<orc::PileView> views(n);
  auto sync = [&](std::uint32_t i) { views[i] = orc::PileView{piles[i].begin_ << kPSS, piles[i].end_ << kPSS, piles[i].is_invalid_}; };
  for (std::uint32_t i = 0; i < n; ++i) {
    Pile& p = piles[i];
    p.id_ = i;
    p.begin_ = begin[i];
    p.end_ = end[i];
    p.median_ = median[i];
    p.is_invalid_ = invalid[i] != 0;
    p.data_.assign(cov.begin() + coff[i], cov.begin() + coff[i + 1]);
    for (std::uint32_t k = roff[i]; k < roff[i + 1]; ++k) p.chimeric_regions_.emplace_back(reg[2 * k], reg[2 * k + 1]);
    overlaps[i].assign(flat.begin() + off[i], flat.begin() + off[i + 1]);
    sync(i);
  }
  Stats st;
  std::uint16_t global_median = 0;

  auto clear_one = [&](std::uint32_t i, std::uint16_t med) {
    const bool was = piles[i].is_chimeric_;
    piles[i].is_chimeric_ = false;
    piles[i].ClearChimericRegions(med);
    if (piles[i].is_chimeric_) ++st.cut;
    piles[i].is_chimeric_ = piles[i].is_chimeric_ || was;
    if (piles[i].is_invalid_) {
      ++st.invalidated;
      std::vector<Overlap>().swap(overlaps[i]);
    }
    sync(i);
  };

  if (piles_only) {
    for (std::uint32_t i = 0; i < n; ++i)
      if (!piles[i].is_invalid_) clear_one(i, median[i]);
  } else {
    if (phases & 1u) {  // ResolveContainedReads
      if (identity != 0) {  // construct.cc:162-217
        for (std::uint32_t i = 0; i < n; ++i) {
          std::uint32_t k = 0;
          for (std::uint32_t j = 0; j < overlaps[i].size(); ++j) {
            if (!orc::OverlapUpdate(overlaps[i][j], views) ||
                orc::IdentityScore(overlaps[i][j], reads[overlaps[i][j].lhs_id], reads[overlaps[i][j].rhs_id]) < identity) {
              ++st.dropped_by_filter;
              continue;
            }
            overlaps[i][k++] = overlaps[i][j];
          }
          overlaps[i].resize(k);
        }
      }
      for (std::uint32_t i = 0; i < n; ++i) {  // :221-237
        std::uint32_t k = 0;
        for (std::uint32_t j = 0; j < overlaps[i].size(); ++j) {
          Overlap& o = overlaps[i][j];
          if (!orc::OverlapUpdate(o, views)) {
            ++st.dropped_by_update[0];
            continue;
          }
          const std::uint32_t type = orc::GetOverlapType(o, views);
          if (type == 1 && !piles[o.rhs_id].is_maybe_chimeric()) {
            piles[i].is_contained_ = true;
            ++st.dropped_by_containment;
          } else if (type == 2 && !piles[i].is_maybe_chimeric()) {
            piles[o.rhs_id].is_contained_ = true;
            ++st.dropped_by_containment;
          } else {
            overlaps[i][k++] = o;
          }
        }
        overlaps[i].resize(k);
      }
      for (std::uint32_t i = 0; i < n; ++i) {  // :238-244
        if (!piles[i].is_contained_) continue;
        ++st.contained[0];
        piles[i].is_invalid_ = true;
        sync(i);
        std::vector<Overlap>().swap(overlaps[i]);
      }
    }
    if (phases & 2u) {  // ResolveChimericSequences
      std::vector<std::uint16_t> medians;
      for (const auto& p : piles)
        if (p.median_ != 0) medians.emplace_back(p.median_);
      // no non-zero median: the reference reads medians[0] of an empty vector.  There is no valid pile then (a valid pile's
      // median is at least the trim coverage), and the stage is stated to change nothing.
      if (!medians.empty()) {
        std::nth_element(medians.begin(), medians.begin() + medians.size() / 2, medians.end());
        global_median = medians[medians.size() / 2];
        for (std::uint32_t i = 0; i < n; ++i)  // :270-282
          if (!piles[i].is_invalid_) clear_one(i, global_median);
        for (std::uint32_t i = 0; i < n; ++i) {  // :287-295
          std::uint32_t k = 0;
          for (std::uint32_t j = 0; j < overlaps[i].size(); ++j) {
            if (orc::OverlapUpdate(overlaps[i][j], views)) overlaps[i][k++] = overlaps[i][j];
            else ++st.dropped_by_update[1];
          }
          overlaps[i].resize(k);
        }
        for (const auto& list : overlaps) {  // :297-308; GetOverlapType reads begin / end only, `views` may lag on invalid
          for (const auto& o : list) {
            const std::uint32_t type = orc::GetOverlapType(o, views);
            const std::uint32_t hit = type == 1 ? o.lhs_id : (type == 2 ? o.rhs_id : n);
            if (hit == n) continue;
            if (!piles[hit].is_contained_) ++st.contained[1];
            piles[hit].is_contained_ = true;
            piles[hit].is_invalid_ = true;
          }
        }
        for (auto& list : overlaps) list.clear();  // :310 (the per-pile slots stay for the second pass's extra one)
      }
    }
  }

  std::ofstream out(argv[3], std::ios::binary);
  std::vector<std::uint8_t> f_inv(n), f_con(n), f_chi(n);
  std::vector<std::uint32_t> o_roff(n + 1, 0), o_reg, o_off(n + 1, 0);
  std::vector<Overlap> o_flat;
  std::vector<std::uint16_t> o_cov;
  for (std::uint32_t i = 0; i < n; ++i) {
    begin[i] = piles[i].begin_;
    end[i] = piles[i].end_;
    f_inv[i] = piles[i].is_invalid_;
    f_con[i] = piles[i].is_contained_;
    f_chi[i] = piles[i].is_chimeric_;
    for (const auto& r : piles[i].chimeric_regions_) {
      o_reg.push_back(r.first);
      o_reg.push_back(r.second);
    }
    o_roff[i + 1] = static_cast<std::uint32_t>(o_reg.size() / 2);
    o_flat.insert(o_flat.end(), overlaps[i].begin(), overlaps[i].end());
    o_off[i + 1] = static_cast<std::uint32_t>(o_flat.size());
    o_cov.insert(o_cov.end(), piles[i].data_.begin(), piles[i].data_.end());
  }
  const std::uint64_t m = o_flat.size();
  Put(out, begin.data(), n);
  Put(out, end.data(), n);
  Put(out, f_inv.data(), n);
  Put(out, f_con.data(), n);
  Put(out, f_chi.data(), n);
  Put(out, o_roff.data(), n + 1);
  Put(out, o_reg.data(), o_reg.size());
  Put(out, &global_median, 1);
  Put(out, &m, 1);
  Put(out, o_flat.data(), o_flat.size());
  Put(out, o_off.data(), n + 1);
  Put(out, o_cov.data(), o_cov.size());
  Put(out, st.dropped_by_update, 2);
  Put(out, &st.dropped_by_filter, 1);
  Put(out, &st.dropped_by_containment, 1);
  Put(out, st.contained, 2);
  Put(out, &st.cut, 1);
  Put(out, &st.invalidated, 1);
  return out ? 0 : 1;
}
