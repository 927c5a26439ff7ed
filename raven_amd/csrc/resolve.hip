// resolve.hip — the tail of stage -5 of raven::ConstructGraph on the device:
//   raven::ResolveContainedReads      RavenLib/src/construct.cc:154-248   (phase 1)
//   raven::ResolveChimericSequences   RavenLib/src/construct.cc:250-314   (phase 2)
// with Pile::ClearChimericRegions / UpdateValidRegion (pile.cc:189-228, :144-157: chimeric.h) and the per-overlap rules
// of overlap_utils.cc (overlap_rules.h).  The piles' state, their coverage and the per-pile overlap lists stay in HBM
// from the first pass to the end of the stage (ResolveState, engine.h); the host reads back one count per compaction
// and, in phase 2, the global median with the number of piles that have work.
//
// Phase 1: [identity != 0: update_and_identity (pass2.hip) on the lists where they are, survivors compacted per pile in
//   order], then one thread per overlap: OverlapUpdate, GetOverlapType, the containment flags, keep flags; contained
//   piles become invalid; the lists are compacted per pile in order, those of invalid piles come out empty.
//   The marking does not depend on the order of the overlaps: OverlapUpdate reads is_invalid, begin and end, the loop
//   writes is_contained only, and is_invalid changes after the loop (construct.cc:238-244).
// Phase 2: the global median from a 65 536-bin histogram of the non-zero medians of ALL piles (a value, not a position:
//   exact), ClearChimericRegions by one wave per pile that has work, OverlapUpdate + GetOverlapType of what is left
//   (GetOverlapType reads begin / end only, so this sweep does not depend on the order either), the lists cleared.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "abi.h"
#include "chimeric.h"
#include "overlap_rules.h"
#include "wave.h"

namespace rvn {

namespace {

// counters of one call, in HBM
enum { kCntUpdate = 0, kCntContainment, kCntContained, kCntCut, kCntInvalidated, kCntNum = 8 };

__device__ __forceinline__ void count_flag(bool flag, u64* counter) {  // one atomic per wave
  const unsigned long long m = __ballot(flag);
  if (m && lane_id() == __builtin_ctzll(m)) atomicAdd(reinterpret_cast<unsigned long long*>(counter), static_cast<unsigned long long>(__popcll(m)));
}

__global__ void pile_regions_kernel(const u32* __restrict__ begin, const u32* __restrict__ end, const u8* __restrict__ invalid,
                                    u32 n, PileRegion* __restrict__ pr) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pr[i] = PileRegion{begin[i] << 4, end[i] << 4, invalid[i] ? 1u : 0u};  // Pile::begin() / end(): bases
}
__global__ void region_counts_kernel(const u32* __restrict__ roff, u32 n, u32* __restrict__ rcount) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rcount[i] = roff[i + 1] - roff[i];
}

// construct.cc:221-237 for one overlap: mark[] = set_is_contained of this phase (several writers, one value)
__global__ void contain_mark_kernel(Overlap* __restrict__ ovl, u64 m, const PileRegion* __restrict__ pr,
                                    const u32* __restrict__ rcount, u8* __restrict__ mark, u8* __restrict__ keep,
                                    u64* __restrict__ counters) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool dropped = false, marked = false;
  if (i < m) {
    Overlap o = ovl[i];
    const PileRegion L = pr[o.lhs_id], R = pr[o.rhs_id];
    u8 k = 0;
    if (!overlap_update(o, L, R)) {
      dropped = true;
    } else {
      const u32 type = overlap_type(o, L, R);
      if (type == 1 && rcount[o.rhs_id] == 0) {  // !is_maybe_chimeric(): no chimeric region left in the pile
        mark[o.lhs_id] = 1;
        marked = true;
      } else if (type == 2 && rcount[o.lhs_id] == 0) {
        mark[o.rhs_id] = 1;
        marked = true;
      } else {
        ovl[i] = o;
        k = 1;
      }
    }
    keep[i] = k;
  }
  count_flag(dropped, counters + kCntUpdate);
  count_flag(marked, counters + kCntContainment);
}

// construct.cc:287-308 for one overlap
// (the reference has emptied the lists of the piles ClearChimericRegions made invalid, work[] == 2, before this loop: their
// overlaps are not counted as dropped)
__global__ void final_mark_kernel(const Overlap* __restrict__ ovl, u64 m, const PileRegion* __restrict__ pr,
                                  const u8* __restrict__ work, u8* __restrict__ mark, u64* __restrict__ counters) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool dropped = false;
  if (i < m) {
    Overlap o = ovl[i];
    const PileRegion L = pr[o.lhs_id], R = pr[o.rhs_id];
    if (!overlap_update(o, L, R)) {
      dropped = work[o.lhs_id] != 2;
    } else {
      const u32 type = overlap_type(o, L, R);
      if (type == 1) mark[o.lhs_id] = 1;
      else if (type == 2) mark[o.rhs_id] = 1;
    }
  }
  count_flag(dropped, counters + kCntUpdate);
}

// the piles this phase marked become contained and invalid
__global__ void apply_marks_kernel(const u8* __restrict__ mark, u32 n, u8* __restrict__ contained, u8* __restrict__ invalid,
                                   PileRegion* __restrict__ pr, u64* __restrict__ counters) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool hit = i < n && mark[i] != 0;
  if (hit) {
    contained[i] = 1;
    invalid[i] = 1;
    pr[i].invalid = 1;
  }
  count_flag(hit, counters + kCntContained);
}

// lists of invalid piles come out empty (every entry of list i has lhs_id == i)
__global__ void keep_valid_kernel(const Overlap* __restrict__ ovl, u64 m, const u8* __restrict__ invalid, u8* __restrict__ keep) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < m && invalid[ovl[i].lhs_id]) keep[i] = 0;
}
// the new offsets are the scan read at the old ones (slot[m] = the survivors)
__global__ void new_offsets_kernel(const u32* __restrict__ off, const u32* __restrict__ slot, u32 n, u32* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) out[i] = slot[off[i]];
}

__global__ void median_hist_kernel(const u16* __restrict__ median, u32 n, u32* __restrict__ hist) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && median[i] != 0) atomicAdd(hist + median[i], 1u);
}
// nth_element(size / 2) of the non-zero medians = the value whose bin holds rank size / 2; out = {value, size}
__global__ __launch_bounds__(256) void median_select_kernel(const u32* __restrict__ hist, u32* __restrict__ out) {
  __shared__ u32 s4[4];
  const u32 t = threadIdx.x;
  u32 sum = 0;
  for (u32 b = 0; b < 256; ++b) sum += hist[t * 256 + b];
  u32 total = 0;
  const u32 before = block_exclusive_sum_256(sum, s4, &total);
  const u32 rank = total / 2;
  if (t == 0) out[1] = total;
  if (total == 0) {
    if (t == 0) out[0] = 0;
    return;
  }
  if (rank >= before && rank < before + sum) {
    u32 c = before;
    for (u32 b = 0; b < 256; ++b) {
      c += hist[t * 256 + b];
      if (rank < c) {
        out[0] = t * 256 + b;
        break;
      }
    }
  }
}

// piles ClearChimericRegions has work on: valid, and with a region or a valid region UpdateValidRegion rejects
__global__ void chimeric_work_kernel(const u8* __restrict__ invalid, const u32* __restrict__ rcount, const u32* __restrict__ begin,
                                     const u32* __restrict__ end, u32 n, u8* __restrict__ flag) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 b = begin[i], e = end[i];
  flag[i] = !invalid[i] && (rcount[i] != 0 || b >= e || e - b < kMinValidCells) ? 1 : 0;
}
__global__ void chimeric_list_kernel(const u8* __restrict__ flag, const u32* __restrict__ slot, u32 n, u32* __restrict__ list) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) list[slot[i]] = i;
}

struct ChimJob {
  const u32* list;
  u16* cov;
  const u64* cov_off;
  u32 *begin, *end;
  u8 *invalid, *chimeric;
  PileRegion* pr;
  const u32* roff;
  u32 *rcount, *regions;
  u8* rflag;  // per region slot: the region is resolved
  u8* work;   // per pile: 1 = listed; becomes 2 when the pile is made invalid here
  const u32* gmed;
  u64* counters;
};

// Pile::ClearChimericRegions(median) (chimeric.h): one wave per listed pile.  The minimum of every region inside the valid
// region is the wave's, over the coverage in HBM; the walk over the regions is lane 0's; the wave zeroes the coverage
// outside the new valid region.
__global__ __launch_bounds__(64) void clear_chimeric_kernel(ChimJob J) {
  const u32 p = J.list[blockIdx.x];
  const int lane = static_cast<int>(threadIdx.x);
  const u64 off = J.cov_off[p];
  const u32 len = static_cast<u32>(J.cov_off[p + 1] - off);
  u16* d = J.cov + off;
  const u32 b_ = J.begin[p], e_ = J.end[p];
  const u16 median = static_cast<u16>(J.gmed[0]);
  const u32 r0 = J.roff[p], nr = J.rcount[p];
  u32* reg = J.regions + 2ULL * r0;
  for (u32 k = 0; k < nr; ++k) {
    const u32 first = reg[2 * k], second = reg[2 * k + 1];
    if (b_ > first || e_ < second) continue;
    u32 mn = 0xFFFFu;
    for (u64 i = static_cast<u64>(first) + lane; i <= second && i < len; i += 64) {
      const u32 v = d[i];
      mn = v < mn ? v : mn;
    }
    mn = wave_min(mn);
    if (lane == 0) J.rflag[r0 + k] = chimeric_cell_resolves(static_cast<u16>(mn), median) ? 1 : 0;
  }
  u32 nb = 0, ne = 0, fl = 0;
  if (lane == 0) {
    const u8* rf = J.rflag + r0;
    const ChimericOutcome o = clear_chimeric_walk(b_, e_, reg, nr, [&](u32 k, u32, u32) { return rf[k] != 0; });
    nb = o.begin;
    ne = o.end;
    fl = (o.invalid ? 1u : 0u) | (o.chimeric ? 2u : 0u);
    J.rcount[p] = o.n_unresolved;
    if (o.chimeric) {
      J.chimeric[p] = 1;
      atomicAdd(reinterpret_cast<unsigned long long*>(J.counters + kCntCut), 1ULL);
    }
    if (o.invalid) {
      J.invalid[p] = 1;
      J.pr[p].invalid = 1;
      J.work[p] = 2;
      atomicAdd(reinterpret_cast<unsigned long long*>(J.counters + kCntInvalidated), 1ULL);
    } else {
      J.begin[p] = nb;
      J.end[p] = ne;
      J.pr[p] = PileRegion{nb << 4, ne << 4, 0u};
    }
  }
  nb = static_cast<u32>(__shfl(static_cast<int>(nb), 0, 64));
  ne = static_cast<u32>(__shfl(static_cast<int>(ne), 0, 64));
  fl = static_cast<u32>(__shfl(static_cast<int>(fl), 0, 64));
  if (fl & 1u) return;
  // UpdateValidRegion: cells [begin_, begin) and [end, end_)
  const u32 lim = e_ < len ? e_ : len;
  for (u64 i = static_cast<u64>(b_) + lane; i < nb && i < lim; i += 64) d[i] = 0;
  for (u64 i = static_cast<u64>(ne) + lane; i < lim; i += 64) d[i] = 0;
}

struct Scratch {
  DevBuf keep, slot, ovl2, off2, mark, counters, hist, gmed, flag, list, rflag;
};

u64* zero_counters(Engine& e, Scratch& S) {
  u64* c = S.counters.get<u64>(kCntNum);
  RVN_HIP(hipMemsetAsync(c, 0, kCntNum * 8, e.stream));
  return c;
}
void fetch_counters(Engine& e, const u64* d, u64* h) {
  RVN_HIP(hipMemcpyAsync(e.h_pin, d, kCntNum * 8, hipMemcpyDeviceToHost, e.stream));
  RVN_HIP(rvn_stream_sync(e.stream));
  std::memcpy(h, e.h_pin, kCntNum * 8);
}

// keep flags -> the lists compacted per pile in order; lists of invalid piles come out empty.  One count read back.
void compact_lists(Engine& e, ResolveState& st, Scratch& S, u8* d_keep) {
  hipStream_t s = e.stream;
  const u64 m = st.n_overlaps;
  const u32 n = st.n;
  if (m == 0) return;
  keep_valid_kernel<<<div_up(m, 256), 256, 0, s>>>(st.ovl.as<Overlap>(), m, st.invalid.as<u8>(), d_keep);
  RVN_LAUNCH_CHECK();
  st.n_overlaps = compact_overlap_list(e, st.ovl, m, d_keep, S.slot, S.ovl2);
  u32* d_off2 = S.off2.get<u32>(static_cast<size_t>(n) + 2);
  new_offsets_kernel<<<div_up(static_cast<u64>(n) + 1, 256), 256, 0, s>>>(st.off.as<u32>(), S.slot.as<u32>(), n, d_off2);
  RVN_LAUNCH_CHECK();
  st.off.swap(S.off2);
}

void apply_marks(Engine& e, ResolveState& st, const u8* d_mark, u64* d_cnt) {
  apply_marks_kernel<<<div_up(st.n, 256), 256, 0, e.stream>>>(d_mark, st.n, st.contained.as<u8>(), st.invalid.as<u8>(),
                                                              st.pr.as<PileRegion>(), d_cnt);
  RVN_LAUNCH_CHECK();
}

// ResolveContainedReads (construct.cc:154-248)
void phase_contained(Engine& e, ResolveState& st, Scratch& S, const ReadsDev* R, double identity) {
  hipStream_t s = e.stream;
  const u32 n = st.n;
  u8* d_keep = S.keep.get<u8>(st.n_overlaps + 16);
  if (identity != 0 && st.n_overlaps) {  // :162-217
    const u64 before = st.n_overlaps;
    update_and_identity(e, *R, st.ovl.as<Overlap>(), st.n_overlaps, st.pr.as<PileRegion>(), nullptr, identity, d_keep);  // ids are indices
    compact_lists(e, st, S, d_keep);
    st.stats.dropped_by_filter += before - st.n_overlaps;
  }
  u64* d_cnt = zero_counters(e, S);
  u8* d_mark = S.mark.get<u8>(static_cast<size_t>(n) + 16);
  RVN_HIP(hipMemsetAsync(d_mark, 0, n, s));
  const u64 m = st.n_overlaps;
  if (m) {
    contain_mark_kernel<<<div_up(m, 256), 256, 0, s>>>(st.ovl.as<Overlap>(), m, st.pr.as<PileRegion>(), st.rcount.as<u32>(), d_mark,
                                                       d_keep, d_cnt);
    RVN_LAUNCH_CHECK();
  }
  apply_marks(e, st, d_mark, d_cnt);  // :238-244
  compact_lists(e, st, S, d_keep);
  u64 c[kCntNum];
  fetch_counters(e, d_cnt, c);
  st.stats.dropped_by_update[0] += c[kCntUpdate];
  st.stats.dropped_by_containment += c[kCntContainment];
  st.stats.contained[0] += static_cast<u32>(c[kCntContained]);
}

// ResolveChimericSequences (construct.cc:250-314)
void phase_chimeric(Engine& e, ResolveState& st, Scratch& S) {
  hipStream_t s = e.stream;
  const u32 n = st.n;
  // :259-267
  u32* d_hist = S.hist.get<u32>(65536);
  u32* d_gmed = S.gmed.get<u32>(4);
  RVN_HIP(hipMemsetAsync(d_hist, 0, 65536 * 4, s));
  median_hist_kernel<<<div_up(n, 256), 256, 0, s>>>(st.median.as<u16>(), n, d_hist);
  median_select_kernel<<<1, 256, 0, s>>>(d_hist, d_gmed);
  RVN_LAUNCH_CHECK();
  // the piles with work, as a list
  u8* d_flag = S.flag.get<u8>(static_cast<size_t>(n) + 16);
  u32* d_slot = S.slot.get<u32>(static_cast<size_t>(n) + 2);
  chimeric_work_kernel<<<div_up(n, 256), 256, 0, s>>>(st.invalid.as<u8>(), st.rcount.as<u32>(), st.begin.as<u32>(), st.end.as<u32>(), n, d_flag);
  RVN_LAUNCH_CHECK();
  exclusive_scan_u8_u32(d_flag, d_slot, n, e.scratch.scan_tmp, s);
  e.h_pin[0] = e.h_pin[1] = 0;
  RVN_HIP(hipMemcpyAsync(e.h_pin, d_gmed, 8, hipMemcpyDeviceToHost, s));
  RVN_HIP(hipMemcpyAsync(e.h_pin + 1, d_slot + n, 4, hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));
  u32 gm[2];
  std::memcpy(gm, e.h_pin, 8);
  const u32 n_work = static_cast<u32>(e.h_pin[1]);
  if (gm[1] == 0) return;  // no pile has a median: no pile is valid, the reference reads an empty vector; nothing changes
  st.global_median = static_cast<u16>(gm[0]);
  u64* d_cnt = zero_counters(e, S);
  u8* d_mark = S.mark.get<u8>(static_cast<size_t>(n) + 16);  // (every allocation of this phase is made before the coverage changes)
  if (n_work) {  // :270-282
    u32* d_list = S.list.get<u32>(n_work);
    chimeric_list_kernel<<<div_up(n, 256), 256, 0, s>>>(d_flag, d_slot, n, d_list);
    RVN_LAUNCH_CHECK();
    ChimJob J{d_list, st.cov, st.cov_off, st.begin.as<u32>(), st.end.as<u32>(), st.invalid.as<u8>(), st.chimeric.as<u8>(),
              st.pr.as<PileRegion>(), st.roff.as<u32>(), st.rcount.as<u32>(), st.regions.as<u32>(),
              S.rflag.get<u8>(static_cast<size_t>(st.regions_total) + 16), d_flag, d_gmed, d_cnt};
    clear_chimeric_kernel<<<n_work, 64, 0, s>>>(J);
    RVN_LAUNCH_CHECK();
  }
  // :287-308
  RVN_HIP(hipMemsetAsync(d_mark, 0, n, s));
  if (st.n_overlaps) {
    final_mark_kernel<<<div_up(st.n_overlaps, 256), 256, 0, s>>>(st.ovl.as<Overlap>(), st.n_overlaps, st.pr.as<PileRegion>(), d_flag, d_mark, d_cnt);
    RVN_LAUNCH_CHECK();
  }
  apply_marks(e, st, d_mark, d_cnt);
  // :310
  st.n_overlaps = 0;
  RVN_HIP(hipMemsetAsync(st.off.ptr, 0, (static_cast<size_t>(n) + 1) * 4, s));
  u64 c[kCntNum];
  fetch_counters(e, d_cnt, c);
  st.stats.dropped_by_update[1] += c[kCntUpdate];
  st.stats.contained[1] += static_cast<u32>(c[kCntContained]);
  st.stats.cut += static_cast<u32>(c[kCntCut]);
  st.stats.invalidated += static_cast<u32>(c[kCntInvalidated]);
}

void run_phases(Engine& e, ResolveState& st, const ReadsDev* R, double identity, u32 phases) {
  Scratch S;
  if (st.n) {
    if (phases & 1u) phase_contained(e, st, S, R, identity);
    if (phases & 2u) phase_chimeric(e, st, S);
  }
  st.phases_done |= phases;
  RVN_HIP(rvn_stream_sync(e.stream));
}

void derive_state(Engine& e, ResolveState& st) {
  const u32 n = st.n;
  hipStream_t s = e.stream;
  RVN_HIP(hipMemsetAsync(st.contained.get<u8>(static_cast<size_t>(n) + 16), 0, static_cast<size_t>(n) + 16, s));
  RVN_HIP(hipMemsetAsync(st.chimeric.get<u8>(static_cast<size_t>(n) + 16), 0, static_cast<size_t>(n) + 16, s));
  st.pr.get<PileRegion>(static_cast<size_t>(n) + 1);
  st.rcount.get<u32>(static_cast<size_t>(n) + 1);
  if (n == 0) return;
  pile_regions_kernel<<<div_up(n, 256), 256, 0, s>>>(st.begin.as<u32>(), st.end.as<u32>(), st.invalid.as<u8>(), n, st.pr.as<PileRegion>());
  region_counts_kernel<<<div_up(n, 256), 256, 0, s>>>(st.roff.as<u32>(), n, st.rcount.as<u32>());
  RVN_LAUNCH_CHECK();
}

template <typename T>
void copy_dd(DevBuf& dst, const DevBuf& src, size_t count, hipStream_t s) {
  T* d = dst.get<T>(count + 16);
  if (count) RVN_HIP(hipMemcpyAsync(d, src.ptr, count * sizeof(T), hipMemcpyDeviceToDevice, s));
}

}  // namespace

// The state of a first pass whose lists and coverage are in HBM: TrimAndAnnotatePiles (construct.cc:123-152) when the pass
// has not been trimmed yet, FindChimericRegions with the CSR left on the device, a working copy of the lists.
std::shared_ptr<ResolveState> resolve_state_of_pass(Engine& e, PileState& ps, u32 coverage) {
  hipStream_t s = e.stream;
  const u32 n = ps.n;
  if (!ps.trimmed && n) piles_trim_and_median(e, ps, coverage, nullptr, nullptr, nullptr, nullptr);
  auto st = std::make_shared<ResolveState>();
  st->n = n;
  copy_dd<u32>(st->begin, ps.ann_begin, n, s);
  copy_dd<u32>(st->end, ps.ann_end, n, s);
  copy_dd<u16>(st->median, ps.ann_median, n, s);
  copy_dd<u8>(st->invalid, ps.ann_invalid, n, s);
  st->regions_total = piles_find_chimeric_regions_dev(e, ps, st->invalid.as<u8>(), st->roff, st->regions);
  st->n_overlaps = ps.kept_total;
  copy_dd<Overlap>(st->ovl, ps.kept, ps.kept_total, s);
  copy_dd<u32>(st->off, ps.kept_off, static_cast<size_t>(n) + 1, s);
  st->cov = ps.pile_data.as<u16>();
  st->cov_off = ps.pile_off.as<u64>();
  st->cov_words = ps.pile_words;
  derive_state(e, *st);
  RVN_HIP(rvn_stream_sync(s));
  return st;
}

// The same state from the caller's host arrays (begin / end in cells)
std::shared_ptr<ResolveState> resolve_state_of_arrays(Engine& e, const Overlap* ovl, const u32* off, u32 n, const u16* cov,
                                                      const u64* cov_off, const u32* regions, const u32* roff,
                                                      const u32* begin, const u32* end, const u16* median, const u8* invalid) {
  hipStream_t s = e.stream;
  auto st = std::make_shared<ResolveState>();
  st->n = n;
  upload(st->begin, begin, n, s);
  upload(st->end, end, n, s);
  upload(st->median, median, n, s);
  upload(st->invalid, invalid, n, s);
  upload(st->roff, roff, static_cast<size_t>(n) + 1, s);
  st->regions_total = roff[n];
  upload(st->regions, regions, 2ULL * roff[n], s);
  st->n_overlaps = off[n];
  upload(st->ovl, ovl, off[n], s);
  upload(st->off, off, static_cast<size_t>(n) + 1, s);
  upload(st->own_cov, cov, cov_off[n], s);
  upload(st->own_cov_off, cov_off, static_cast<size_t>(n) + 1, s);
  st->cov = st->own_cov.as<u16>();
  st->cov_off = st->own_cov_off.as<u64>();
  st->cov_words = cov_off[n];
  derive_state(e, *st);
  RVN_HIP(rvn_stream_sync(s));
  return st;
}

}  // namespace rvn

// ---- C ABI (include/raven_hip.h) -----------------------------------------------------------------------------------
using namespace rvn;

// The per-pile result on the host (a snapshot of the call that made it); the lists stay in HBM with the state.
struct rvn_resolved {
  Engine* e = nullptr;
  std::weak_ptr<int> engine_life;
  std::shared_ptr<ResolveState> st;
  u32 phases_done = 0;  // of the state when this result was made: the lists are its lists only as long as that holds
  u32 n = 0;
  std::vector<u32> begin, end, roff, regions;
  std::vector<u8> invalid, contained, chimeric;
  u64 n_overlaps = 0;
  u16 median = 0;
  ResolveStats stats;
};

namespace {

std::unique_ptr<rvn_resolved> snapshot(Engine& e, const std::shared_ptr<ResolveState>& st) {
  std::unique_ptr<rvn_resolved> r(new rvn_resolved());
  const u32 n = st->n;
  r->e = &e;
  r->engine_life = e.life;
  r->st = st;
  r->phases_done = st->phases_done;
  r->n = n;
  r->n_overlaps = st->n_overlaps;
  r->median = st->global_median;
  r->stats = st->stats;
  r->begin.assign(n, 0);
  r->end.assign(n, 0);
  r->invalid.assign(n, 0);
  r->contained.assign(n, 0);
  r->chimeric.assign(n, 0);
  r->roff.assign(static_cast<size_t>(n) + 1, 0);
  if (n == 0) return r;
  std::vector<u32> slots_off(static_cast<size_t>(n) + 1), rcount(n), slots(2ULL * st->regions_total);
  RVN_HIP(hipMemcpy(r->begin.data(), st->begin.ptr, n * 4ULL, hipMemcpyDeviceToHost));
  RVN_HIP(hipMemcpy(r->end.data(), st->end.ptr, n * 4ULL, hipMemcpyDeviceToHost));
  RVN_HIP(hipMemcpy(r->invalid.data(), st->invalid.ptr, n, hipMemcpyDeviceToHost));
  RVN_HIP(hipMemcpy(r->contained.data(), st->contained.ptr, n, hipMemcpyDeviceToHost));
  RVN_HIP(hipMemcpy(r->chimeric.data(), st->chimeric.ptr, n, hipMemcpyDeviceToHost));
  RVN_HIP(hipMemcpy(slots_off.data(), st->roff.ptr, (n + 1ULL) * 4, hipMemcpyDeviceToHost));
  RVN_HIP(hipMemcpy(rcount.data(), st->rcount.ptr, n * 4ULL, hipMemcpyDeviceToHost));
  if (!slots.empty()) RVN_HIP(hipMemcpy(slots.data(), st->regions.ptr, slots.size() * 4, hipMemcpyDeviceToHost));
  for (u32 i = 0; i < n; ++i) {  // the regions in use, as a CSR without gaps
    r->roff[i + 1] = r->roff[i] + rcount[i];
    r->regions.insert(r->regions.end(), slots.begin() + 2ULL * slots_off[i], slots.begin() + 2ULL * (slots_off[i] + rcount[i]));
  }
  return r;
}

}  // namespace

int rvn_pass1_resolve(rvn_pass1* p, const rvn_reads* rr, uint32_t coverage, double identity, uint32_t phases,
                      rvn_resolved** out) {
  return guarded(p ? p->e : nullptr, [&]() -> int {
    if (!p || !out) return fail(RVN_EINVAL, "[raven_hip] rvn_pass1_resolve: NULL argument");
    *out = nullptr;
    if (phases == 0 || phases > 3) return fail(RVN_EINVAL, "[raven_hip] rvn_pass1_resolve: phases must be 1, 2 or 3");
    if (coverage > 65535) return fail(RVN_EINVAL, "[raven_hip] coverage threshold above 65535");
    if (identity != 0 && (phases & 1u)) {
      if (!rr) return fail(RVN_EINVAL, "[raven_hip] rvn_pass1_resolve: the identity filter needs the reads");
      if (rr->r.n != p->ps.n || !rr->r.ids_are_indices)
        return fail(RVN_EINVAL, "[raven_hip] rvn_pass1_resolve: the reads are not the ones of this pass (ids[i] == i)");
    }
    PileState& ps = p->ps;
    if (ps.resolve && (ps.resolve->phases_done & phases))
      return fail(RVN_EINVAL, "[raven_hip] rvn_pass1_resolve: this phase has already run on this pass");
    if (ps.resolve && (phases & 1u))
      return fail(RVN_EINVAL, "[raven_hip] rvn_pass1_resolve: ResolveContainedReads cannot follow ResolveChimericSequences");
    Engine& e = *p->e;
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    const bool fresh = !ps.resolve;
    if (fresh) ps.resolve = resolve_state_of_pass(e, ps, coverage);
    try {
      run_phases(e, *ps.resolve, rr ? &rr->r : nullptr, identity, phases);
    } catch (const DeviceOutOfMemory& ex) {
      // guarded() repeats a call that ran out of device memory.  A state made by this call is made again; one that
      // an earlier call left holds that call's result and is kept (phase 2 allocates before it changes anything).
      if (fresh) {
        ps.resolve.reset();
        throw;
      }
      throw HipError(std::string(ex.what()) + " (the state of the earlier phase is kept: call again)");
    }
    *out = snapshot(e, ps.resolve).release();
    return RVN_OK;
  });
}

int rvn_resolve_contained_and_chimeric(rvn_engine* h, const rvn_reads* rr, const rvn_overlap* overlaps, const uint32_t* offsets,
                                       uint32_t n_piles, const uint16_t* coverage, const uint64_t* coverage_offsets,
                                       const uint32_t* regions, const uint32_t* region_offsets, const uint32_t* begin,
                                       const uint32_t* end, const uint16_t* median, const uint8_t* invalid, double identity,
                                       uint32_t phases, rvn_resolved** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    const char* who = "[raven_hip] rvn_resolve_contained_and_chimeric: ";
    auto bad = [&](const char* what) {
      return fail(RVN_EINVAL, std::string(who) + what);
    };
    if (!h || !out || !offsets || !coverage_offsets || !region_offsets ||
        (n_piles && (!begin || !end || !median || !invalid)) || (offsets[n_piles] && !overlaps) ||
        (coverage_offsets[n_piles] && !coverage) || (region_offsets[n_piles] && !regions))
      return bad("NULL argument");
    *out = nullptr;
    if (phases == 0 || phases > 3) return bad("phases must be 1, 2 or 3");
    if (identity != 0 && (phases & 1u)) {
      if (!rr) return bad("the identity filter needs the reads");
      if (rr->r.n != n_piles || !rr->r.ids_are_indices) return bad("the reads are not the ones of these piles (ids[i] == i)");
    }
    const char* csr = csr_offsets_error(offsets, n_piles, kNoCsrLimit);
    if (!csr) csr = csr_offsets_error(coverage_offsets, n_piles, kMaxPileCells);
    if (!csr) csr = csr_offsets_error(region_offsets, n_piles, kNoCsrLimit);
    if (csr) return bad(csr);
    for (u32 i = 0; i < n_piles; ++i) {
      const u64 len = coverage_offsets[i + 1] - coverage_offsets[i];
      if (begin[i] > end[i] || end[i] > len) return bad("a valid region outside its pile");
      for (u32 k = region_offsets[i]; k < region_offsets[i + 1]; ++k)
        if (regions[2 * k] > regions[2 * k + 1] || regions[2 * k + 1] >= len) return bad("a chimeric region outside its pile");
      for (u32 x = offsets[i]; x < offsets[i + 1]; ++x) {
        if (overlaps[x].lhs_id != i) return bad("an entry of list i whose lhs_id is not i");
        if (overlaps[x].rhs_id >= n_piles) return bad("overlap of an unknown pile");
      }
    }
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    auto st = resolve_state_of_arrays(e, reinterpret_cast<const Overlap*>(overlaps), offsets, n_piles, coverage, coverage_offsets,
                                      regions, region_offsets, begin, end, median, invalid);
    run_phases(e, *st, rr ? &rr->r : nullptr, identity, phases);
    *out = snapshot(e, st).release();
    return RVN_OK;
  });
}

uint64_t rvn_resolved_num_overlaps(const rvn_resolved* r) { return r ? r->n_overlaps : 0; }
uint64_t rvn_resolved_num_regions(const rvn_resolved* r) { return r ? r->regions.size() / 2 : 0; }
uint64_t rvn_resolved_coverage_words(const rvn_resolved* r) { return r && r->st->own_cov.ptr ? r->st->cov_words : 0; }

int rvn_resolved_fetch(const rvn_resolved* r, uint32_t* begin, uint32_t* end, uint8_t* invalid, uint8_t* contained,
                       uint8_t* chimeric, uint32_t* regions, uint32_t* region_offsets, uint16_t* median, rvn_overlap* overlaps,
                       uint32_t* offsets, uint16_t* coverage, rvn_resolve_stats* stats) {
  if (!r) return fail(RVN_EINVAL, "[raven_hip] NULL resolved result");
  const u32 n = r->n;
  if (begin && n) std::memcpy(begin, r->begin.data(), n * 4ULL);
  if (end && n) std::memcpy(end, r->end.data(), n * 4ULL);
  if (invalid && n) std::memcpy(invalid, r->invalid.data(), n);
  if (contained && n) std::memcpy(contained, r->contained.data(), n);
  if (chimeric && n) std::memcpy(chimeric, r->chimeric.data(), n);
  if (regions && !r->regions.empty()) std::memcpy(regions, r->regions.data(), r->regions.size() * 4);
  if (region_offsets) std::memcpy(region_offsets, r->roff.data(), r->roff.size() * 4);
  if (median) *median = r->median;
  if (stats) {
    static_assert(sizeof(rvn_resolve_stats) == sizeof(ResolveStats), "stats layout");
    std::memcpy(stats, &r->stats, sizeof(ResolveStats));
  }
  if (!overlaps && !offsets && !coverage) return RVN_OK;
  if (r->engine_life.expired()) return fail(RVN_EINVAL, "[raven_hip] the engine of this result is gone");
  return guarded(r->e, [&]() -> int {
    const ResolveState& st = *r->st;
    if ((overlaps || offsets) && st.phases_done != r->phases_done)
      return fail(RVN_EINVAL, "[raven_hip] rvn_resolved_fetch: a later phase on the same pass has consumed these lists");
    RVN_HIP(hipSetDevice(r->e->device));
    if (overlaps && st.n_overlaps)
      RVN_HIP(hipMemcpy(overlaps, st.ovl.ptr, st.n_overlaps * sizeof(Overlap), hipMemcpyDeviceToHost));
    if (offsets) {
      if (n) RVN_HIP(hipMemcpy(offsets, st.off.ptr, (n + 1ULL) * 4, hipMemcpyDeviceToHost));
      else offsets[0] = 0;
    }
    if (coverage && st.own_cov.ptr && st.cov_words)
      RVN_HIP(hipMemcpy(coverage, st.own_cov.ptr, st.cov_words * 2, hipMemcpyDeviceToHost));
    return RVN_OK;
  });
}

void rvn_resolved_destroy(rvn_resolved* r) { delete r; }
