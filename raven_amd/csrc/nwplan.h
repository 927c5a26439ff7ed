// nwplan.h — the PLAN of the alignment-path stage (nwpath.hip: nw_breakpoints): everything the host decides about a call
// before a kernel is launched, as plain host arithmetic without a HIP call — which kernel variant and band a job gets,
// the order of a pass, its cut into chunks and their buffer sets, the threshold model fitted on the pilot, and where each
// array of a call lies in the stage's two device blocks.  The pass object of nwpath.hip turns a plan into launches; the
// same header compiles with g++ alone (tests/host/nw_plan_host.cpp, tests/test_nw_plan.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "nwpath.h"

namespace rvn {

// kernel variants: (blocks per lane R, lanes per alignment G); narrow rings share a wave (64 / G alignments).  Ordered by
// the band they hold (G (64 R + 1) - 64 R offsets), i.e. by alignment length.  Several blocks per lane are only used
// where one block per lane cannot hold the band: variants (2, 8) ... (4, 32) — fewer instructions per block step on
// paper — were measured and lost (C4 sweep 178 ms with R = 1 wherever possible, 187 ms allowing R = 2, 225 ms allowing
// R = 4: more registers = fewer waves, a coarser band, costlier ring events).
struct NwVariant {
  u32 R, G;
};
constexpr NwVariant kNwVariants[] = {{1, 4}, {1, 8}, {1, 16}, {1, 32}, {1, 64}, {2, 64}, {4, 64}, {8, 64}};
constexpr u32 kLevels = sizeof(kNwVariants) / sizeof(kNwVariants[0]);
// A band no variant's ring holds is swept in stripes (nwpath.h, NwGeo): the widest variant's R, stripes of nw_stripe_lanes
// super-blocks (default 64, a whole wave), a band of at most kNwMaxStripes such rings (262 144 rows with whole waves, 8 x
// the widest ring).  Striped jobs are a class of their own, above the variants.
constexpr NwVariant kNwStripedVariant = kNwVariants[kLevels - 1];
constexpr u32 kNwMaxStripes = 8;
constexpr u32 kStriped = kLevels;
constexpr u32 kClasses = kLevels + 1;
constexpr u32 kHeadMax = 4096;  // jobs of the pass of the longest alignments (nw_take_head)

// largest threshold whose band fits a ring of G lanes with R blocks each
inline u32 kcap_of(u32 n, u32 m, u32 R, u32 G) {
  const u32 d = n > m ? n - m : m - n;
  // nw_ring_lanes(lo, hi, R) <= G  <=>  64R + lo + hi <= G (64R + 1);  lo + hi = 2 floor((k - d) / 2) + d
  const u64 room = static_cast<u64>(G) * (64ULL * R + 1) - 64ULL * R;
  if (room < d) return 0;
  const u64 k = d + ((room - d) / 2) * 2 + 1;  // (k - d) / 2 floors: an odd surplus costs nothing
  return static_cast<u32>(std::min<u64>(k, static_cast<u64>(n) + m));
}

inline u32 level_of(const NwJob& J) {
  if (J.S) return kStriped;
  for (u32 x = 0; x < kLevels; ++x)
    if (kNwVariants[x].R == J.R && kNwVariants[x].G == J.G) return x;
  return kLevels - 1;
}

// plan: the narrowest variant whose ring holds the band of k; beyond the widest, stripes (a band of at most kNwMaxStripes
// rings whose stored hs + ck fit the budget; otherwise the job is not aligned).  stripe_lanes: the widest ring of one
// sweep (variants with wider rings are skipped) = the stripe size.
inline bool nw_plan(NwJob& J, u64 k, u32 stripe_lanes, u64 budget) {
  const u32 d = J.n > J.m ? J.n - J.m : J.m - J.n;
  k = std::max<u64>(std::max<u64>(k, d), 16);
  k = std::min<u64>(k, static_cast<u64>(J.n) + J.m);  // D(n, m) <= n + m: that threshold never fails
  J.S = 0;
  for (u32 lvl = 0; lvl < kLevels; ++lvl) {
    if (kNwVariants[lvl].G > stripe_lanes) continue;
    const u32 cap = kcap_of(J.n, J.m, kNwVariants[lvl].R, kNwVariants[lvl].G);
    if (cap >= k) {
      J.R = kNwVariants[lvl].R;
      J.G = kNwVariants[lvl].G;
      J.k = static_cast<u32>(k);
      J.kcap = cap;
      return true;
    }
  }
  const u32 cap = kcap_of(J.n, J.m, kNwStripedVariant.R, kNwMaxStripes * stripe_lanes);
  if (cap < k) return false;
  const NwGeo g = nw_geo_striped(J.n, J.m, static_cast<u32>(k), kNwStripedVariant.R, stripe_lanes);
  if (g.hs_words() * 4 + g.ck_entries() * 16 > budget) return false;
  J.R = kNwStripedVariant.R;
  J.G = kNwStripedVariant.G;
  J.S = stripe_lanes;
  J.k = static_cast<u32>(k);
  J.kcap = cap;
  return true;
}

// The order of a pass — longest jobs first: they go through the widest variants, and the pass ends with the walks of the
// shortest ones.  Descending by (variant, columns), ties in `todo` order: two counting passes (12 + 12 key bits) instead
// of a sort.
inline std::vector<u32> nw_order(const std::vector<NwJob>& jobs, const std::vector<u32>& todo) {
  const size_t nt = todo.size();
  std::vector<u32> key(nt), tmp(nt), idx(nt);
  parallel_for(nt, 16384, [&jobs, &todo, &key, &idx](size_t x0, size_t x1) {  // (the GPU waits for this planning: a few host threads)
    for (size_t x = x0; x < x1; ++x) {
      const NwJob& J = jobs[todo[x]];
      // 8-base resolution is plenty for the ordering; striped jobs by their number of stripes (each stripe launch takes
      // the jobs that have that stripe: a prefix of the class)
      const u32 mm = J.S ? std::min<u32>(nw_geo_job(J).n_stripes, (1u << 20) - 1) : std::min<u32>(J.m >> 3, (1u << 20) - 1);
      static_assert(kClasses <= 16, "4 bits of variant + 20 bits of length = the 24 key bits of the two passes");
      key[x] = 0xFFFFFFu - ((level_of(J) << 20) | mm);
      idx[x] = static_cast<u32>(x);
    }
  });
  for (int pass = 0; pass < 2; ++pass) {
    u32 cnt[4097] = {};
    const int sh = 12 * pass;
    for (size_t x = 0; x < nt; ++x) cnt[((key[idx[x]] >> sh) & 4095u) + 1]++;
    for (int c = 0; c < 4096; ++c) cnt[c + 1] += cnt[c];
    for (size_t x = 0; x < nt; ++x) tmp[cnt[(key[idx[x]] >> sh) & 4095u]++] = idx[x];
    idx.swap(tmp);
  }
  std::vector<u32> order(nt);
  for (size_t x = 0; x < nt; ++x) order[x] = todo[idx[x]];
  return order;
}

// Chunk layout of a pass: kOwnFirst — the first chunk (the longest alignments) on buffer set 3 with a twelfth of the
// budget, the others on sets 0-2 in rotation with a third each; kHeadOnly — that first chunk ALONE, what does not fit it
// is handed back in `left`; kRotating — sets 0-2 only (the jobs behind a head that is already running).
enum NwLayout { kOwnFirst, kHeadOnly, kRotating };

struct NwChunk {
  size_t c0, c1;  // its jobs: order[c0 .. c1)
  u64 hs_w, ck_e;
  u32 coff[kClasses + 1];  // offsets of the classes inside the chunk, from the widest variant down
};
struct NwChunks {
  std::vector<NwChunk> chunks;
  u64 slot_w = 0;       // (path form) words of the pass's slots
  u64 band_cells = 0;   // what the pass adds to NwStats::band_cells
  u64 store_bytes = 0;  // hs + ck bytes of its largest chunk
};

// chunk 0 -> set 3 (its own), chunk ci >= 1 -> set (ci - 1) % 3;  kRotating: chunk ci -> set ci % 3
inline int nw_set_of(size_t ci, NwLayout layout) {
  if (layout == kRotating) return static_cast<int>(ci % 3);
  return ci == 0 ? 3 : static_cast<int>((ci - 1) % 3);
}
// jobs of class x in the chunk: classes are laid out from the widest variant down
inline u32 nw_count_of(const NwChunk& C, u32 x) {
  const u32 next_off = x == 0 ? static_cast<u32>(C.c1 - C.c0) : C.coff[x - 1];
  return next_off - C.coff[x];
}

// Chunks of the order whose hs + ck fit a third of the budget (a job larger than that goes alone); every job's hs, ckpt
// and — slots: the path form — bp_off are set.  kHeadOnly: one chunk, the rest of `order` moves to `left`.  (Capping the
// jobs per chunk — an even eighth, or a third of what is left, so that the uncovered walk of the last chunk gets shorter —
// was measured at C4 and did not pay: every extra sweep launch brings its own ramp and tail, +19 ms of sweep time
// against ~20 ms less at the end; profiles/r05_nw_timeline.csv.)
inline NwChunks nw_chunks(std::vector<u32>& order, std::vector<NwJob>& jobs, u64 budget, NwLayout layout, bool slots,
                          std::vector<u32>* left) {
  NwChunks out;
  std::vector<NwChunk>& chunks = out.chunks;
  struct Need {
    u64 hw, ce, cells;
    u32 level;
  };
  std::vector<Need> need(order.size());  // what a job stores and computes: per job in parallel, summed up in order below
  parallel_for(order.size(), 16384, [&jobs, &order, &need](size_t x0, size_t x1) {
    for (size_t x = x0; x < x1; ++x) {
      const NwJob& J = jobs[order[x]];
      const NwGeo g = nw_geo_job(J);
      need[x] = Need{g.hs_words(), g.ck_entries(), static_cast<u64>(J.m) * (static_cast<u64>(g.lo) + g.hi + 1), level_of(J)};
    }
  });
  for (size_t c0 = 0; c0 < order.size();) {
    NwChunk C{};
    C.c0 = c0;
    size_t c1 = c0;
    while (c1 < order.size()) {
      NwJob& J = jobs[order[c1]];
      const u64 hw = need[c1].hw, ce = need[c1].ce;
      // three buffer sets in rotation + one of its own for the first chunk (the longest alignments: its walk is
      // latency-bound — 106 ms for 2 432 alignments at C4 — and a set shared with chunk 3 made that chunk's sweep wait
      // 17 ms for it), a quarter of a share
      const u64 share = (chunks.empty() && layout != kRotating) ? budget / 12 : budget / 3;
      if (c1 > c0 && (C.hs_w + hw) * 4 + (C.ck_e + ce) * 16 > share) break;
      J.hs = C.hs_w;
      J.ckpt = C.ck_e;
      if (slots) {
        J.bp_off = out.slot_w;
        out.slot_w += nw_slot_words(J.k);
      }
      C.hs_w += hw;
      C.ck_e += ce;
      out.band_cells += need[c1].cells;
      C.coff[need[c1].level + 1]++;
      ++c1;
    }
    // the order is by descending level: offsets of the classes inside the chunk, in that order
    u32 run_off = 0, cnt[kClasses];
    for (u32 x = 0; x < kClasses; ++x) cnt[x] = C.coff[x + 1];
    for (int x = static_cast<int>(kClasses) - 1; x >= 0; --x) {
      C.coff[x] = run_off;
      run_off += cnt[x];
    }
    C.coff[kClasses] = run_off;  // count of class x = offset of class x - 1 (or the chunk's end) - its own offset
    C.c1 = c1;
    out.store_bytes = std::max<u64>(out.store_bytes, C.hs_w * 4 + C.ck_e * 16);
    chunks.push_back(C);
    c0 = c1;
    if (layout == kHeadOnly) break;
  }
  if (layout == kHeadOnly && !chunks.empty() && chunks[0].c1 < order.size()) {  // what the head's share does not hold goes with the rest
    for (size_t x = chunks[0].c1; x < order.size(); ++x) left->push_back(order[x]);
    order.resize(chunks[0].c1);
  }
  return out;
}

// What a buffer set must hold for the chunks it serves (a lone job beyond its share enlarges one set, not all)
struct NwSetNeed {
  bool used;
  u64 hs_w, ck_e;
};
inline NwSetNeed nw_set_need(const std::vector<NwChunk>& chunks, NwLayout layout, int b) {
  NwSetNeed need{false, 0, 0};
  for (size_t ci = 0; ci < chunks.size(); ++ci) {
    if (nw_set_of(ci, layout) != b) continue;
    need.used = true;
    need.hs_w = std::max(need.hs_w, chunks[ci].hs_w);
    need.ck_e = std::max(need.ck_e, chunks[ci].ck_e);
  }
  return need;
}

// ---- thresholds ------------------------------------------------------------------------------------------------------
// A pilot sample (every call: the error level changes from round to round) is aligned with a generous band; its distances
// give the mean rate mu and the spread around mu x len as  var = a len + b len^2  (a: base-level noise, b: differences
// between reads).  Everyone gets  k = mu len + 4.5 sqrt(a len + b len^2) + 6 : with a normal spread a few alignments in a
// million are repeated (a repeat pass ends with lonely, latency-bound walks, so it is worth ~3 % more band to make it
// rare), against one in ten with a 90th-percentile rule.  The pilot is swept for its distances only and skips the longest
// quarter of the reads.  Small batches keep the previous call's estimate (rate).
struct NwObs {
  double len, d;
};
struct NwThresholdModel {
  double mu = -1, va = 0, vb = 0;
  // fewer than 256 observations: no model (mu < 0), threshold() goes by the rate
  void fit(const std::vector<NwObs>& obs) {
    if (obs.size() < 256) return;
    double sl = 0, sd = 0;
    for (const NwObs& o : obs) {
      sl += o.len;
      sd += o.d;
    }
    mu = sd / sl;
    // least squares of the squared residuals on (len, len^2), the 2 % largest standardised residuals left out
    std::vector<double> zs;
    for (const NwObs& o : obs) zs.push_back(std::fabs(o.d - mu * o.len) / std::sqrt(o.len));
    std::vector<double> zsorted = zs;
    std::sort(zsorted.begin(), zsorted.end());
    const double zcut = zsorted[static_cast<size_t>(zsorted.size() * 0.98)];
    double s11 = 0, s12 = 0, s22 = 0, t1 = 0, t2 = 0, sr = 0, sn = 0;
    for (size_t x = 0; x < obs.size(); ++x) {
      if (zs[x] > zcut) continue;
      const double L = obs[x].len * 1e-3, r2 = (obs[x].d - mu * obs[x].len) * (obs[x].d - mu * obs[x].len);
      s11 += L * L;
      s12 += L * L * L;
      s22 += L * L * L * L;
      t1 += r2 * L;
      t2 += r2 * L * L;
      sr += r2 / L;
      sn += 1;
    }
    const double det = s11 * s22 - s12 * s12;
    double a = -1, b = -1;
    if (det > 1e-9 * s11 * s22) {
      a = (t1 * s22 - t2 * s12) / det;
      b = (t2 * s11 - t1 * s12) / det;
    }
    if (!(a >= 0) || !(b >= 0)) {  // one length only, or a fit outside the model: all spread on the linear term
      a = sn > 0 ? sr / sn : mu * 1e3;
      b = 0;
    }
    va = std::max(a * 1e-3, 0.25 * mu);  // back to bases; never below a quarter of the Poisson level
    vb = b * 1e-6;
  }
  u64 threshold(double len, double rate) const {
    const double z = 4.5;
    return mu > 0 ? static_cast<u64>(mu * len + z * std::sqrt(va * len + vb * len * len)) + 6 : static_cast<u64>(rate * len) + 16;
  }
  // the pilot's own, generous threshold: from the previous call's rate
  static u64 pilot_threshold(double len, double rate) { return static_cast<u64>((rate * 1.25 + 0.02) * len) + 16; }
};

inline u32 nw_job_len(const NwJob& J) { return std::max(J.n, J.m); }

// The pilot sample of `valid` (4 096 jobs at least): every stride-th job, 1 024 at most, none from the longest quarter
inline std::vector<u32> nw_pilot_sample(const std::vector<NwJob>& jobs, const std::vector<u32>& valid) {
  std::vector<u32> lens;
  for (u32 i : valid) lens.push_back(nw_job_len(jobs[i]));
  std::nth_element(lens.begin(), lens.begin() + lens.size() * 3 / 4, lens.end());
  const u32 len_cap = lens[lens.size() * 3 / 4];
  std::vector<u32> pilot;
  const size_t stride = std::max<size_t>(valid.size() / 1400, 1);
  for (size_t x = 0; x < valid.size(); ++x)
    if (x % stride == stride / 2 && pilot.size() < 1024 && nw_job_len(jobs[valid[x]]) <= len_cap) pilot.push_back(valid[x]);
  return pilot;
}

// The head of a call: its min(kHeadMax, an eighth) longest jobs by (length descending, id ascending) move from `rest` to
// `head` (what is left of `rest` keeps no particular order)
inline void nw_take_head(const std::vector<NwJob>& jobs, std::vector<u32>& rest, std::vector<u32>& head) {
  const size_t n_head = std::min<size_t>(kHeadMax, rest.size() / 8);
  auto longer = [&jobs](u32 x, u32 y) {
    const u32 lx = nw_job_len(jobs[x]), ly = nw_job_len(jobs[y]);
    return lx != ly ? lx > ly : x < y;
  };
  std::nth_element(rest.begin(), rest.begin() + n_head, rest.end(), longer);
  head.assign(rest.begin(), rest.begin() + n_head);
  rest.erase(rest.begin(), rest.begin() + n_head);
}

// Rate estimate for the next call (the pilot's first threshold / small batches) from the distance / length of this call's
// alignments (reordered); fewer than 32: the previous one stays
inline double nw_next_rate(std::vector<double>& rates, double previous) {
  if (rates.size() < 32) return previous;
  const size_t at = std::min(rates.size() - 1, static_cast<size_t>(rates.size() * 0.9));
  std::nth_element(rates.begin(), rates.begin() + at, rates.end());  // (the order statistic a full sort gave: ~15 ms of host time per round)
  return rates[at] * 1.05 + 0.002;
}

// ---- the device arrays of a call ---------------------------------------------------------------------------------------
// A pass = a set of planned jobs queued together: its job records, order, results and states on the device.  The usual
// pass addresses them by job id; a COMPACT pass (the head, the early retry) has arrays of its own, addressed by position in
// its order.  All of them lie in two blocks (NwState::jobs: job records; NwState::res: u32 words); nw_dev_layout states
// where — offsets in elements, each array behind the one before — and how large the blocks are.
struct NwPassAt {
  size_t jobs, idx, res, status;
  size_t n;  // entries of each
  bool compact;
};
struct NwDevLayout {
  NwPassAt all, head, retry;
  size_t next;       // job counter of the sweeps on the main stream (4 words)
  size_t side_next;  // job counters of the sweeps launched beside the main stream, one per variant
  size_t n_words, n_jobs;  // sizes of the two blocks
};
inline NwDevLayout nw_dev_layout(u32 nj) {
  NwDevLayout L{};
  size_t words = 0, recs = 0;
  auto take = [](size_t& end, size_t n) {
    const size_t at = end;
    end += n;
    return at;
  };
  const size_t n_all = static_cast<size_t>(nj) + 1;
  L.all.n = n_all;
  L.all.compact = false;
  L.all.jobs = take(recs, n_all);
  L.all.res = take(words, n_all);
  L.all.status = take(words, n_all);
  L.all.idx = take(words, n_all);
  L.next = take(words, 4);
  for (NwPassAt* p : {&L.head, &L.retry}) {
    p->n = kHeadMax;
    p->compact = true;
    p->jobs = take(recs, kHeadMax);
    p->res = take(words, kHeadMax);
    p->status = take(words, kHeadMax);
    p->idx = take(words, kHeadMax);
  }
  L.side_next = take(words, kLevels);
  L.n_words = words;
  L.n_jobs = recs;
  return L;
}
// the same as pointers into the two blocks
struct NwPassDev {
  NwJob* jobs;
  u32 *idx, *res, *status;
  bool compact;
};
struct NwDevArrays {
  NwPassDev all, head, retry;
  u32 *next, *side_next;
};
inline NwDevArrays nw_dev_arrays(const NwDevLayout& L, NwJob* jobs_block, u32* words_block) {
  auto pass = [jobs_block, words_block](const NwPassAt& p) {
    return NwPassDev{jobs_block + p.jobs, words_block + p.idx, words_block + p.res, words_block + p.status, p.compact};
  };
  return NwDevArrays{pass(L.all), pass(L.head), pass(L.retry), words_block + L.next, words_block + L.side_next};
}

}  // namespace rvn
