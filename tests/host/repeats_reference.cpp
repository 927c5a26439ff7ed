// The CPU statement of raven::ResolveRepeatInducedOverlaps (RavenLib/src/construct.cc:493-559) that the device stage
// (raven_amd/csrc/repeats.hip) and its per-pile hook are compared with: ConnectedComponents (overlap_utils.cc:135-178,
// the BFS with its deque), nth_element of the members' medians, Pile::FindRepetitiveRegions / UpdateRepetitiveRegions /
// CheckRepetitiveRegions / ClearRepetitiveRegions (pile.cc:230-371) restated over std::vector state, single-threaded,
// with the oracle's FindSlopes / MergeRegions / GetOverlapType (oracle/raven_oracle.cpp, compiled into this program).
//
//   repeats_reference IN OUT      IN: the arguments of rvn_resolve_repeat_induced_overlaps, OUT: what it returns
// Binary little-endian files.  IN = u32 n_piles, u64 n_overlaps, overlaps (8 x u32 each), u64 coverage_offsets[n + 1],
// u16 coverage[], u64 kmers_offsets[n + 1], u8 kmers[], u32 begin[n], u32 end[n] (bases), u16 median[n], u8 invalid[n].
// OUT = u32 iterations, u32 components (first iteration), u64 removed, u64 n_overlaps, overlaps, u32 region_offsets[n + 1],
// u32 regions[2 x total], u8 is_repetitive[n].  The wall time of the loop goes to stderr.
#include <chrono>
#include <fstream>
#include <iostream>

#include "raven_oracle.cpp"

namespace {

using orc::Overlap;
using Region = orc::Region;
constexpr std::uint32_t kPSS = 4;

// the state of a raven::Pile that the stage reads and writes (pile.h:130-141)
struct Pile {
  std::uint32_t id_, begin_, end_;
  std::uint16_t median_;
  bool is_invalid_, is_repetitive_ = false;
  std::vector<std::uint16_t> data_;
  std::vector<bool> kmers_;
  std::vector<Region> repetitive_regions_;

  // pile.cc:230-317
  void FindRepetitiveRegions(std::uint16_t median) {
    if (!kmers_.empty()) {
      std::uint32_t w = 479 >> kPSS;
      std::uint32_t group = 12;
      Region region;
      std::size_t count = 0;
      for (std::uint32_t i = 0; i < kmers_.size(); ++i) {
        if (kmers_[i] == 0) continue;
        if (count && i - region.second <= w) {
          region.second = i;
          ++count;
          continue;
        }
        if (count > group) {
          repetitive_regions_.emplace_back(region);
          is_repetitive_ = true;
        }
        region = {i, i};
        count = 1;
      }
      if (count > group) {
        repetitive_regions_.emplace_back(region);
        is_repetitive_ = true;
      }
    }
    auto slopes = orc::FindSlopes(data_, 1.42);
    if (!slopes.empty()) {
      auto is_repetitive_region = [&](const Region& begin, const Region& end) -> bool {
        if (((end.first >> 1) + end.second) / 2 - ((begin.first >> 1) + begin.second) / 2 > 0.84 * (end_ - begin_))
          return false;
        bool found_peak = false;
        std::uint16_t peak_value = orc::clamp16(1.42 * std::max(data_[begin.second], data_[end.first >> 1]));
        std::uint16_t min_value = orc::clamp16(1.42 * median);
        std::uint32_t num_valid = 0;
        for (std::uint32_t i = begin.second + 1; i < (end.first >> 1); ++i) {
          if (data_[i] > min_value) ++num_valid;
          if (data_[i] > peak_value) found_peak = true;
        }
        return !(!found_peak || num_valid < 0.9 * ((end.first >> 1) - begin.second));
      };
      for (std::uint32_t i = 0; i < slopes.size() - 1; ++i) {
        if (!(slopes[i].first & 1)) continue;
        for (std::uint32_t j = i + 1; j < slopes.size(); ++j) {
          if (slopes[j].first & 1) continue;
          if (is_repetitive_region(slopes[i], slopes[j])) {
            repetitive_regions_.emplace_back(
                (slopes[i].second) - 0.336 * (slopes[i].second - (slopes[i].first >> 1)),
                (slopes[j].first >> 1) + 0.336 * (slopes[j].second - (slopes[j].first >> 1)));
            is_repetitive_ = true;
          }
        }
      }
    }
    repetitive_regions_ = orc::MergeRegions(repetitive_regions_);
    for (auto& it : repetitive_regions_) {
      it.first = std::max(begin_, it.first) << 1;
      it.second = std::min(end_, it.second);
    }
  }

  // pile.cc:319-342
  void UpdateRepetitiveRegions(const Overlap& o) {
    if (repetitive_regions_.empty() || (id_ != o.lhs_id && id_ != o.rhs_id)) return;
    std::uint32_t begin = (id_ == o.lhs_id ? o.lhs_begin : o.rhs_begin) >> kPSS;
    std::uint32_t end = (id_ == o.lhs_id ? o.lhs_end : o.rhs_end) >> kPSS;
    std::uint32_t fuzz = 420 >> kPSS;
    std::uint32_t offset = 0.1 * (end_ - begin_);
    for (auto& it : repetitive_regions_) {
      if (begin < it.second && (it.first >> 1) < end) {
        if ((it.first >> 1) < begin_ + offset && begin - begin_ < end_ - end) {
          if (end >= it.second + fuzz) it.first |= 1;
        } else if (it.second > end_ - offset && begin - begin_ > end_ - end) {
          if (begin + fuzz <= (it.first >> 1)) it.first |= 1;
        }
      }
    }
  }

  // pile.cc:344-369
  bool CheckRepetitiveRegions(const Overlap& o) const {
    if (repetitive_regions_.empty() || (id_ != o.lhs_id && id_ != o.rhs_id)) return false;
    std::uint32_t begin = (id_ == o.lhs_id ? o.lhs_begin : o.rhs_begin) >> kPSS;
    std::uint32_t end = (id_ == o.lhs_id ? o.lhs_end : o.rhs_end) >> kPSS;
    std::uint32_t fuzz = 420 >> kPSS;
    std::uint32_t offset = 0.1 * (end_ - begin_);
    for (const auto& it : repetitive_regions_) {
      if (begin < it.second && (it.first >> 1) < end) {
        if ((it.first >> 1) < begin_ + offset) {
          if (end < it.second + fuzz && (it.first & 1)) return true;
        } else if (it.second > end_ - offset) {
          if (begin + fuzz > (it.first >> 1) && (it.first & 1)) return true;
        }
      }
    }
    return false;
  }

  void ClearRepetitiveRegions() { repetitive_regions_.clear(); }
};

// overlap_utils.cc:135-178
std::vector<std::vector<std::uint32_t>> ConnectedComponents(const std::vector<Overlap>& overlaps,
                                                            const std::vector<Pile>& piles,
                                                            const std::vector<orc::PileView>& views) {
  std::vector<std::vector<std::uint32_t>> connections(piles.size());
  for (const auto& jt : overlaps) {
    if (orc::GetOverlapType(jt, views) > 2) {
      connections[jt.lhs_id].emplace_back(jt.rhs_id);
      connections[jt.rhs_id].emplace_back(jt.lhs_id);
    }
  }
  std::vector<std::vector<std::uint32_t>> dst;
  std::vector<bool> isVisited(piles.size(), false);
  for (std::uint32_t i = 0; i < connections.size(); ++i) {
    if (piles[i].is_invalid_ || isVisited[i]) continue;
    dst.resize(dst.size() + 1);
    std::deque<std::uint32_t> que = {i};
    while (!que.empty()) {
      std::uint32_t j = que.front();
      que.pop_front();
      if (isVisited[j]) continue;
      isVisited[j] = true;
      dst.back().emplace_back(j);
      for (const auto& it : connections[j]) que.emplace_back(it);
    }
  }
  return dst;
}

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

  std::vector<Pile> piles(n);
  std::vector<orc::PileView> views(n);
  for (std::uint32_t i = 0; i < n; ++i) {
    Pile& p = piles[i];
    p.id_ = i;
    p.begin_ = begin[i] >> kPSS;
    p.end_ = end[i] >> kPSS;
    p.median_ = median[i];
    p.is_invalid_ = invalid[i] != 0;
    p.data_.assign(cov.begin() + coff[i], cov.begin() + coff[i + 1]);
    p.kmers_.assign(kmers.begin() + koff[i], kmers.begin() + koff[i + 1]);
    views[i] = orc::PileView{begin[i], end[i], invalid[i] != 0};
  }

  // construct.cc:504-555
  const auto t0 = std::chrono::steady_clock::now();
  std::uint32_t iterations = 0, components = 0;
  std::uint64_t removed = 0;
  while (true) {
    ++iterations;
    auto comps = ConnectedComponents(overlaps, piles, views);
    if (iterations == 1) components = static_cast<std::uint32_t>(comps.size());
    for (const auto& it : comps) {
      std::vector<std::uint16_t> medians;
      for (const auto& jt : it) medians.emplace_back(piles[jt].median_);
      std::nth_element(medians.begin(), medians.begin() + medians.size() / 2, medians.end());
      std::uint16_t med = medians[medians.size() / 2];
      for (const auto& jt : it) piles[jt].FindRepetitiveRegions(med);
    }
    for (const auto& it : overlaps) {
      piles[it.lhs_id].UpdateRepetitiveRegions(it);
      piles[it.rhs_id].UpdateRepetitiveRegions(it);
    }
    bool is_changed = false;
    std::uint32_t j = 0;
    for (std::uint32_t i = 0; i < overlaps.size(); ++i) {
      const auto& it = overlaps[i];
      if (piles[it.lhs_id].CheckRepetitiveRegions(it) || piles[it.rhs_id].CheckRepetitiveRegions(it)) {
        is_changed = true;
      } else {
        overlaps[j++] = it;
      }
    }
    removed += overlaps.size() - j;
    overlaps.resize(j);
    if (!is_changed) break;
    for (const auto& it : comps)
      for (const auto& jt : it) piles[jt].ClearRepetitiveRegions();
  }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cerr << "repeats_reference: " << secs << " s, " << iterations << " iterations" << std::endl;

  std::ofstream out(argv[2], std::ios::binary);
  const std::uint64_t m_out = overlaps.size();
  Put(out, &iterations, 1);
  Put(out, &components, 1);
  Put(out, &removed, 1);
  Put(out, &m_out, 1);
  Put(out, overlaps.data(), overlaps.size());
  std::vector<std::uint32_t> roff(n + 1, 0), regions;
  std::vector<std::uint8_t> isrep(n);
  for (std::uint32_t i = 0; i < n; ++i) {
    for (const auto& r : piles[i].repetitive_regions_) {
      regions.push_back(r.first);
      regions.push_back(r.second);
    }
    roff[i + 1] = static_cast<std::uint32_t>(regions.size() / 2);
    isrep[i] = piles[i].is_repetitive_ ? 1 : 0;
  }
  Put(out, roff.data(), roff.size());
  Put(out, regions.data(), regions.size());
  Put(out, isrep.data(), isrep.size());
  return out ? 0 : 1;
}
