// chain.hip — the chain stage of ram::MinimizerEngine::Map (ram's Chain + LongestSubsequence): a read's matches, already in
// e.map.m_grp[0] / m_pos[0] and segmented per read, -> its overlaps.  Entered through chain_matches, by the entry points of
// map.hip behind their match stage and by rvn_shard_chain (abi_shard.hip) on matches shipped from another GPU.
//
// Kernels (all integer, HBM/L2- or latency-bound; no MFMA):
//   seg_sort (segsort.h)       both sorts — a read's matches by group, an interval's by positions (keys only): segments
//                              binned by size, a workgroup per segment in LDS sized for the class, a wave beyond the table
//   intervals                  one wave per read segment; ram's sequential (i, j) sweep restated as
//                              a per-element binary search + wave max-scan
//   chain_small                intervals of <= kChainSmallCap matches: one lane each, insertion sort + LIS in LDS
//   chain                      one wave per larger interval, by the position sort's size classes (sizeclass.h): ram's exact
//                              patience/binary-search LIS replayed on ballots, gap split, covered-bases score
//   compact_*                  overlap slots -> (read, emission) order
#include <algorithm>

#include "engine.h"
#include "segsort.h"
#include "sizeclass.h"
#include "wave.h"

namespace rvn {

namespace {

// ---- diagonal-band intervals (ram Chain, first loop) ------------------------------------------
// One wave per read segment. Slots: segment [b, e) may hold at most (e-b)/4 intervals, stored at
// slot ceil(b/4)+id (disjoint across segments).
__global__ __launch_bounds__(256) void intervals_kernel(const u64* __restrict__ grp, const u64* __restrict__ seg_off,
                                                       u32 n_seg, u64 bandwidth, u64* __restrict__ slot_begin,
                                                       u64* __restrict__ slot_end, u32* __restrict__ iv_cnt) {
  const u32 seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= n_seg) return;
  const int lane = lane_id();
  const u64 b = seg_off[seg], e = seg_off[seg + 1];
  const long long n = static_cast<long long>(e - b);
  if (n < 4) {
    if (lane == 0) iv_cnt[seg] = 0;
    return;
  }
  const u64 slot_base = (b + 3) >> 2;
  const u64* g = grp + b;
  long long carry_prev = -1;  // local index (end) of the last valid candidate so far
  u32 n_iv = 0;
  const unsigned long long lt = lanemask_lt();
  for (long long base = 1; base <= n; base += 64) {
    const long long il = base + lane;
    const bool in = il <= n;
    long long lprev = 0;
    bool cand = false;
    if (in) {
      const u64 g_prev = g[il - 1];
      long long lo = 0, hi = il - 1;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (g_prev - g[mid] <= bandwidth) hi = mid;
        else lo = mid + 1;
      }
      lprev = lo;
      const u64 gi = il == n ? ~0ULL : g[il];
      cand = (gi - g[lprev] > bandwidth) && (il - lprev >= 4);
    }
    const long long mine = cand ? il : -1;
    const long long incl = wave_inclusive_max(mine);
    long long excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = -1;
    excl = excl > carry_prev ? excl : carry_prev;
    const bool is_new = cand && !(excl > lprev);
    const unsigned long long newmask = __ballot(is_new);
    if (is_new) {
      const u32 id = n_iv + __popcll(newmask & lt);
      slot_begin[slot_base + id] = b + static_cast<u64>(lprev);
      if (excl >= 0) slot_end[slot_base + id - 1] = b + static_cast<u64>(excl);
    }
    const long long wmax = __shfl(incl, 63, 64);
    carry_prev = wmax > carry_prev ? wmax : carry_prev;
    n_iv += __popcll(newmask);
  }
  if (lane == 0) {
    if (n_iv) slot_end[slot_base + n_iv - 1] = b + static_cast<u64>(carry_prev);
    iv_cnt[seg] = n_iv;
  }
}

__global__ __launch_bounds__(256) void intervals_gather_kernel(const u64* __restrict__ slot_begin,
                                                              const u64* __restrict__ slot_end,
                                                              const u64* __restrict__ seg_off,
                                                              const u32* __restrict__ iv_off, u32 n_seg,
                                                              u64* __restrict__ iv_begin, u64* __restrict__ iv_end,
                                                              u32* __restrict__ iv_read) {
  const u32 seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= n_seg) return;
  const u32 o0 = iv_off[seg], o1 = iv_off[seg + 1];
  const u64 slot_base = (seg_off[seg] + 3) >> 2;
  for (u32 i = lane_id(); i < o1 - o0; i += 64) {
    iv_begin[o0 + i] = slot_begin[slot_base + i];
    iv_end[o0 + i] = slot_end[slot_base + i];
    iv_read[o0 + i] = seg;
  }
}

// ---- LIS chain + overlap emission (ram Chain second loop + LongestSubsequence) ----------------
// ram Chain: split the chain where consecutive lhs positions differ by more than `gap`, score each piece by
// covered bases, emit the overlaps.  cp(m) = packed positions of chain element m (ascending).
template <typename CP>
__device__ __forceinline__ void chain_emit(CP cp, u32 longest, bool strand, u64 g0, u32 lhs_id, u32 k, u32 chain,
                                           u32 min_matches, u32 gap, Overlap* __restrict__ slots,
                                           u8* __restrict__ slot_flags, bool writer,
                                           u64* __restrict__ anchors /* region of this interval or null */,
                                           u64 anchor_base, u64* __restrict__ slot_aoff,
                                           u32* __restrict__ slot_acnt) {
  u32 emitted = 0;
  u32 l = 0;
  for (u32 kk = 1; kk <= longest; ++kk) {
    const u32 lhs_k = kk < longest ? static_cast<u32>(cp(kk) >> 32) : 0xFFFFFFFFu;
    const u32 lhs_km1 = static_cast<u32>(cp(kk - 1) >> 32);
    if (lhs_k - lhs_km1 > gap) {
      if (kk - l < chain) {
        l = kk;
        continue;
      }
      u32 lhs_matches = 0, lhs_begin = 0, lhs_end = 0;
      u32 rhs_matches = 0, rhs_begin = 0, rhs_end = 0;
      for (u32 m = l; m < kk; ++m) {
        const u64 mm = cp(m);
        const u32 lhs_pos = static_cast<u32>(mm >> 32);
        if (lhs_pos > lhs_end) {
          lhs_matches += lhs_end - lhs_begin;
          lhs_begin = lhs_pos;
        }
        lhs_end = lhs_pos + k;
        u32 rhs_pos = static_cast<u32>(mm);
        rhs_pos = strand ? rhs_pos : (1U << 31) - (rhs_pos + k - 1);
        if (rhs_pos > rhs_end) {
          rhs_matches += rhs_end - rhs_begin;
          rhs_begin = rhs_pos;
        }
        rhs_end = rhs_pos + k;
      }
      lhs_matches += lhs_end - lhs_begin;
      rhs_matches += rhs_end - rhs_begin;
      const u32 score = lhs_matches < rhs_matches ? lhs_matches : rhs_matches;
      if (score < min_matches) {
        l = kk;
        continue;
      }
      if (writer) {
        const u64 ml = cp(l), mr = cp(kk - 1);
        Overlap o;
        o.lhs_id = lhs_id;
        o.lhs_begin = static_cast<u32>(ml >> 32);
        o.lhs_end = k + static_cast<u32>(mr >> 32);
        o.rhs_id = static_cast<u32>(g0 >> 33);
        o.rhs_begin = strand ? static_cast<u32>(ml) : static_cast<u32>(mr);
        o.rhs_end = k + (strand ? static_cast<u32>(mr) : static_cast<u32>(ml));
        o.score = score;
        o.strand = strand ? 1u : 0u;
        slots[emitted] = o;
        slot_flags[emitted] = 1;
        if (anchors) {  // the chain pieces are disjoint sub-ranges of [0, longest): store them in place
          for (u32 m = l; m < kk; ++m) anchors[m] = cp(m);
          slot_aoff[emitted] = anchor_base + l;
          slot_acnt[emitted] = kk - l;
        }
      }
      ++emitted;
      l = kk;
    }
  }
}

// The same for a WAVE that holds the chain (chain_wave): the pieces from ballots of the gap test, a piece's covered bases
// summed by all lanes — the serial loop above adds up the measure of the union of the k-mers [pos, pos + k) of ascending
// positions, which is sum over consecutive pairs of min(k, difference) + k.
template <typename CP>
__device__ __forceinline__ void chain_emit_wave(CP cp, u32 longest, bool strand, u64 g0, u32 lhs_id, u32 k, u32 chain,
                                                u32 min_matches, u32 gap, Overlap* __restrict__ slots,
                                                u8* __restrict__ slot_flags, u64* __restrict__ anchors, u64 anchor_base,
                                                u64* __restrict__ slot_aoff, u32* __restrict__ slot_acnt) {
  const int lane = lane_id();
  auto rhs_of = [&](u64 mm) -> u32 {
    const u32 rhs_pos = static_cast<u32>(mm);
    return strand ? rhs_pos : (1U << 31) - (rhs_pos + k - 1);
  };
  u32 emitted = 0;
  u32 l = 0;
  for (u32 base = 1; base <= longest; base += 64) {
    const u32 kk_mine = base + static_cast<u32>(lane);
    bool brk = false;
    if (kk_mine <= longest) {
      const u32 lhs_k = kk_mine < longest ? static_cast<u32>(cp(kk_mine) >> 32) : 0xFFFFFFFFu;
      const u32 lhs_km1 = static_cast<u32>(cp(kk_mine - 1) >> 32);
      brk = lhs_k - lhs_km1 > gap;
    }
    unsigned long long pieces = __ballot(brk);
    while (pieces) {
      const u32 kk = base + static_cast<u32>(__builtin_ctzll(pieces));
      pieces &= pieces - 1;
      if (kk - l >= chain) {
        u32 lsum = 0, rsum = 0;
        for (u32 m = l + static_cast<u32>(lane); m + 1 < kk; m += 64) {
          const u64 a = cp(m), b = cp(m + 1);
          const u32 dl = static_cast<u32>(b >> 32) - static_cast<u32>(a >> 32), dr = rhs_of(b) - rhs_of(a);
          lsum += dl < k ? dl : k;
          rsum += dr < k ? dr : k;
        }
        const u32 lhs_matches = wave_sum(lsum) + k, rhs_matches = wave_sum(rsum) + k;
        const u32 score = lhs_matches < rhs_matches ? lhs_matches : rhs_matches;
        if (score >= min_matches) {
          if (lane == 0) {
            const u64 ml = cp(l), mr = cp(kk - 1);
            Overlap o;
            o.lhs_id = lhs_id;
            o.lhs_begin = static_cast<u32>(ml >> 32);
            o.lhs_end = k + static_cast<u32>(mr >> 32);
            o.rhs_id = static_cast<u32>(g0 >> 33);
            o.rhs_begin = strand ? static_cast<u32>(ml) : static_cast<u32>(mr);
            o.rhs_end = k + (strand ? static_cast<u32>(mr) : static_cast<u32>(ml));
            o.score = score;
            o.strand = strand ? 1u : 0u;
            slots[emitted] = o;
            slot_flags[emitted] = 1;
            if (anchors) {
              slot_aoff[emitted] = anchor_base + l;
              slot_acnt[emitted] = kk - l;
            }
          }
          if (anchors)  // the chain pieces are disjoint sub-ranges of [0, longest): stored in place
            for (u32 m = l + static_cast<u32>(lane); m < kk; m += 64) anchors[m] = cp(m);
          ++emitted;
        }
      }
      l = kk;
    }
  }
}

// Small intervals (chain <= n <= kChainSmallCap): one LANE per interval, every array private to the lane in LDS
// ([element][lane] layout: bank = lane, conflict-free), no cross-lane traffic at all.
__global__ __launch_bounds__(64) void chain_small_kernel(const u64* __restrict__ grp, const u64* __restrict__ pos,
                                                        const u64* __restrict__ iv_begin,
                                                        const u64* __restrict__ iv_end,
                                                        const u32* __restrict__ iv_read, u32 n_iv,
                                                        const u32* __restrict__ ids, u32 first, u32 k, u32 chain,
                                                        u32 min_matches, u32 gap, u32 slot_div,
                                                        Overlap* __restrict__ slots, u8* __restrict__ slot_flags,
                                                        u64* __restrict__ anchors, u64* __restrict__ slot_aoff,
                                                        u32* __restrict__ slot_acnt) {
  __shared__ u64 s_pos[kChainSmallCap][64];
  __shared__ u64 s_tail[kChainSmallCap + 1][64];
  __shared__ u8 s_tidx[kChainSmallCap + 1][64];
  __shared__ u8 s_pred[kChainSmallCap][64];
  const u32 lane = threadIdx.x;
  const u32 t = blockIdx.x * 64 + lane;
  if (t >= n_iv) return;
  const u64 b = iv_begin[t];
  const u64 n64 = iv_end[t] - b;
  if (n64 < chain || n64 > kChainSmallCap) return;  // larger intervals: chain_kernel
  const u32 n = static_cast<u32>(n64);
  const u64* p = pos + b;
  const u64 g0 = grp[b];
  const bool strand = (g0 >> 32) & 1;
#pragma unroll 8
  for (u32 i = 0; i < kChainSmallCap; ++i)
    if (i < n) s_pos[i][lane] = p[i];
  // ram sorts the interval by positions before the LIS: <= 32 elements, private to the lane -> insertion sort
  // (positions are distinct, so the result is the unique sorted order)
  for (u32 i = 1; i < n; ++i) {
    const u64 key = s_pos[i][lane];
    u32 j = i;
    while (j > 0 && s_pos[j - 1][lane] > key) {
      s_pos[j][lane] = s_pos[j - 1][lane];
      --j;
    }
    s_pos[j][lane] = key;
  }
  u32 longest = 0;
  for (u32 it = 0; it < n; ++it) {
    const u64 cur = s_pos[it][lane];
    const u32 lhs = static_cast<u32>(cur >> 32), rhs = static_cast<u32>(cur);
    u32 lo = 1, hi = longest;
    while (lo <= hi) {
      const u32 mid = lo + (hi - lo) / 2;
      const u64 q = s_tail[mid][lane];
      const u32 ql = static_cast<u32>(q >> 32), qr = static_cast<u32>(q);
      if (ql < lhs && (strand ? qr < rhs : qr > rhs)) lo = mid + 1;
      else hi = mid - 1;
    }
    s_pred[it][lane] = lo > 1 ? s_tidx[lo - 1][lane] : static_cast<u8>(0);
    s_tidx[lo][lane] = static_cast<u8>(it);
    s_tail[lo][lane] = cur;
    longest = longest > lo ? longest : lo;
  }
  if (longest < chain) return;
  {
    u32 j = s_tidx[longest][lane];
    for (u32 i = 0; i < longest; ++i) {
      const u32 nj = s_pred[j][lane];
      s_tidx[longest - 1 - i][lane] = static_cast<u8>(j);
      j = nj;
    }
    for (u32 m = 0; m < longest; ++m) s_tail[m][lane] = s_pos[s_tidx[m][lane]][lane];
  }
  const u64 slot_base = (b + slot_div - 1) / slot_div;
  chain_emit([&](u32 m) { return s_tail[m][lane]; }, longest, strand, g0, ids[first + iv_read[t]], k, chain,
             min_matches, gap, slots + slot_base, slot_flags + slot_base, true, anchors ? anchors + b : nullptr, b,
             slot_aoff ? slot_aoff + slot_base : nullptr, slot_acnt ? slot_acnt + slot_base : nullptr);
}

// One WAVE per interval.  ram's patience LIS is sequential over the elements, but its binary search only
// needs the predicate "tail[len] precedes cur" at the probed lengths: all 64 lanes evaluate the predicate
// for 64 lengths at once (tails live in LDS), a ballot turns it into a bit mask and the *same* probe
// sequence ram would follow is then replayed on the mask with scalar ALU only.  Intervals of up to
// kChainBigCap matches run entirely out of LDS; larger ones use the same code on global scratch.

template <bool GLOBAL>
__device__ __forceinline__ void chain_sync() {
  if (GLOBAL) __threadfence_block();  // lane 0's global stores must be visible to the other lanes' loads
  __builtin_amdgcn_wave_barrier();
}

template <typename IdxT, bool GLOBAL>
__device__ void chain_wave(const u64* __restrict__ p, u32 n, bool strand, u64 g0, u32 lhs_id, u32 k, u32 chain,
                           u32 min_matches, u32 gap, u64* tail_pos, IdxT* tail_idx, IdxT* pred, u64* maskbuf,
                           Overlap* __restrict__ slots, u8* __restrict__ slot_flags, u64* __restrict__ anchors,
                           u64 anchor_base, u64* __restrict__ slot_aoff, u32* __restrict__ slot_acnt) {
  const int lane = lane_id();
  u32 longest = 0;
  for (u32 base = 0; base < n; base += 64) {
    const u64 mine = (base + lane < n) ? p[base + lane] : 0;
    const u32 cnt = min(64u, n - base);
    // A colinear stretch is a run of elements that each EXTEND the longest chain: ram's search for such an element
    // answers "precedes" at every probe, and both the probed lengths and the tails found there are then known in
    // advance for the whole run (element t of the run meets the chain at length longest + t: its probes see old tails
    // and the run's own earlier elements).  So the run is tried as a whole: lanes t0 .. cnt-1 store their elements at
    // the lengths they would get, every lane replays its own ~log2(longest) probes against that speculated tail array,
    // and one ballot gives the first lane whose search would have turned: the elements before it are appended at once
    // (exactly the state the one-by-one loop below would leave), that element goes through the general replay.  A run
    // is tried at the start of a block and after every element that extended the chain.
    bool try_run = true;
    for (u32 t = 0; t < cnt;) {
      if (try_run && cnt - t >= 2) {
        const bool active = static_cast<u32>(lane) >= t && static_cast<u32>(lane) < cnt;
        const u32 my_long = longest + (static_cast<u32>(lane) - t);  // the chain length this lane's element meets
        const IdxT first_pred = longest ? tail_idx[longest] : static_cast<IdxT>(0);
        if (active) tail_pos[my_long + 1] = mine;
        chain_sync<GLOBAL>();
        bool turned = false;
        if (active) {
          const u32 lhs = static_cast<u32>(mine >> 32), rhs = static_cast<u32>(mine);
          for (u32 a = my_long; a >= 1 && !turned; a >>= 1) {
            const u64 q = tail_pos[my_long + 1 - a + ((a - 1) >> 1)];
            const u32 ql = static_cast<u32>(q >> 32), qr = static_cast<u32>(q);
            turned = !(ql < lhs && (strand ? qr < rhs : qr > rhs));
          }
        }
        const unsigned long long bad = __ballot(turned);
        const u32 stop = bad ? static_cast<u32>(__builtin_ctzll(bad)) : cnt;  // first lane whose search turns
        if (active && static_cast<u32>(lane) < stop) {
          tail_idx[my_long + 1] = static_cast<IdxT>(base + lane);
          pred[base + lane] = static_cast<u32>(lane) == t ? first_pred : static_cast<IdxT>(base + lane - 1);
        }
        chain_sync<GLOBAL>();
        longest += stop - t;
        t = stop;
        try_run = false;
        if (t >= cnt) break;
      }
      const u64 cur = __shfl(mine, static_cast<int>(t), 64);
      const u32 lhs = static_cast<u32>(cur >> 32), rhs = static_cast<u32>(cur);
      u32 lo = 1, hi = longest;
      bool appended = false;
      if (longest > 64) {
        // The common case of a colinear interval: cur extends the longest chain.  ram's search then answers "precedes" at
        // every probe, and that probe path is known in advance — probe i looks at length
        // longest + 1 - a + (a - 1) / 2 with a = longest >> i, while a >= 1 — so lane i tests probe i, and one ballot
        // says whether the search ends at longest + 1.  (Any failed probe: the general replay below.)
        const u32 a = lane < 32 ? longest >> lane : 0u;
        bool fail = false;
        if (a >= 1) {
          const u64 q = tail_pos[longest + 1 - a + ((a - 1) >> 1)];
          const u32 ql = static_cast<u32>(q >> 32), qr = static_cast<u32>(q);
          fail = !(ql < lhs && (strand ? qr < rhs : qr > rhs));
        }
        if (!__ballot(fail)) {
          lo = longest + 1;
          appended = true;
        }
      }
      if (appended) {
      } else if (longest > 512) {
        // Long chains: ram's binary search probes ~log2(longest) tails, one after the other.  Here six levels of its
        // search tree are evaluated at once: lane h (heap index 1..63) derives the (lo, hi) range ram would have at tree
        // node h from the current range, tests the predicate at that node's midpoint, a ballot collects the 63 answers
        // and the walk down the six levels is scalar bit tests — ram's exact probe sequence (the predicate need not be
        // monotone), two round trips to the tails for chains of up to 4096 instead of twelve dependent reads.
        while (lo <= hi) {
          const u32 h = static_cast<u32>(lane);
          u32 l = lo, r = hi;
          bool valid = h >= 1;
          if (valid) {
            const int depth = 31 - __clz(static_cast<int>(h));
            for (int d = depth - 1; d >= 0; --d) {
              if (l > r) break;
              const u32 mid = l + (r - l) / 2;
              if ((h >> d) & 1u) l = mid + 1;
              else r = mid - 1;
            }
            valid = l <= r;
          }
          bool ok = false;
          if (valid) {
            const u64 q = tail_pos[l + (r - l) / 2];
            const u32 ql = static_cast<u32>(q >> 32), qr = static_cast<u32>(q);
            ok = ql < lhs && (strand ? qr < rhs : qr > rhs);
          }
          const unsigned long long m = __ballot(ok);
          u32 node = 1;
          for (int level = 0; level < 6 && lo <= hi; ++level) {
            const u32 mid = lo + (hi - lo) / 2;
            const u32 bit = static_cast<u32>((m >> node) & 1ULL);
            if (bit) lo = mid + 1;
            else hi = mid - 1;
            node = 2 * node + bit;
          }
        }
      } else if (longest <= 64) {
        bool ok = false;
        if (static_cast<u32>(lane) < longest) {
          const u64 q = tail_pos[lane + 1];
          const u32 ql = static_cast<u32>(q >> 32), qr = static_cast<u32>(q);
          ok = ql < lhs && (strand ? qr < rhs : qr > rhs);
        }
        const unsigned long long m = __ballot(ok);
        while (lo <= hi) {
          const u32 mid = lo + (hi - lo) / 2;
          if ((m >> (mid - 1)) & 1ULL) lo = mid + 1;
          else hi = mid - 1;
        }
      } else {
        const u32 nchunks = (longest + 63) >> 6;
        for (u32 c = 0; c < nchunks; ++c) {
          const u32 len = c * 64 + lane + 1;
          bool ok = false;
          if (len <= longest) {
            const u64 q = tail_pos[len];
            const u32 ql = static_cast<u32>(q >> 32), qr = static_cast<u32>(q);
            ok = ql < lhs && (strand ? qr < rhs : qr > rhs);
          }
          const unsigned long long m = __ballot(ok);
          if (lane == 0) maskbuf[c] = m;
        }
        chain_sync<GLOBAL>();
        while (lo <= hi) {
          const u32 mid = lo + (hi - lo) / 2;
          if ((maskbuf[(mid - 1) >> 6] >> ((mid - 1) & 63)) & 1ULL) lo = mid + 1;
          else hi = mid - 1;
        }
      }
      const u32 it = base + t;
      const IdxT prev = lo > 1 ? tail_idx[lo - 1] : static_cast<IdxT>(0);  // minimal[0] == 0 in ram
      chain_sync<GLOBAL>();  // every lane has read maskbuf / tail_idx before lane 0 overwrites
      if (lane == 0) {
        pred[it] = prev;
        tail_idx[lo] = static_cast<IdxT>(it);
        tail_pos[lo] = cur;
      }
      chain_sync<GLOBAL>();
      try_run = lo > longest;  // it extended the chain: the next ones may well do so too
      longest = longest > lo ? longest : lo;
      ++t;
    }
  }
  if (longest < chain) return;
  {
    // backtrack: chain indices ascending into tail_idx[0 .. longest).  Rounds 1-5 followed pred[] one element at a time out
    // of LDS — `longest` dependent reads of ~100 cycles, every lane doing the same — and the emission below ran two more
    // serial loops over the chain on all 64 lanes: for the long colinear intervals of HiFi reads (4 500 matches per read in a
    // polishing round's mapping, one wave per CU in that size class) the three were ~95 % of the stage (round 6: 0.63 ms per
    // interval of which ~0.02 ms the LIS itself).  Now: the walk back goes 64 elements at a time out of REGISTERS (a block's
    // predecessors, one per lane; a run of elements that each follow the one before is taken in one step from a ballot),
    // leaving one membership mask per block, and the indices are written block by block from the masks.
    const u32 nblk = (n + 63) >> 6;
    for (u32 b2 = lane; b2 < nblk; b2 += 64) maskbuf[b2] = 0;
    u32 j = tail_idx[longest];
    chain_sync<GLOBAL>();
    u32 left = longest;
    for (int b2 = static_cast<int>(j >> 6); b2 >= 0 && left; --b2) {
      const u32 idx = (static_cast<u32>(b2) << 6) + static_cast<u32>(lane);
      const u32 pr = idx < n ? static_cast<u32>(pred[idx]) : 0u;
      // bit i: element i of the block follows element i - 1 of the block
      const unsigned long long cont = __ballot(lane > 0 && idx < n && pr + 1 == idx);
      unsigned long long m = 0;
      while (left && static_cast<int>(j >> 6) == b2) {
        const u32 l = j & 63u;
        const unsigned long long upto = l == 63 ? ~0ULL : ((2ULL << l) - 1ULL);
        const unsigned long long stops = ~cont & upto;                                   // (bit 0 is always one of them)
        u32 r = 63u - static_cast<u32>(__builtin_clzll(stops));                           // the run l, l - 1, .., r
        if (l - r + 1 > left) r = l + 1 - left;
        m |= upto & ~((1ULL << r) - 1ULL);
        left -= l - r + 1;
        j = static_cast<u32>(__shfl(static_cast<int>(pr), static_cast<int>(r), 64));       // where element r came from
      }
      if (lane == 0) maskbuf[b2] = m;
    }
    chain_sync<GLOBAL>();
    u32 at = 0;
    for (u32 b2 = 0; b2 < nblk; ++b2) {
      const unsigned long long m = maskbuf[b2];
      if ((m >> lane) & 1ULL) tail_idx[at + static_cast<u32>(__popcll(m & ((1ULL << lane) - 1ULL)))] = static_cast<IdxT>((b2 << 6) + lane);
      at += static_cast<u32>(__popcll(m));
    }
    chain_sync<GLOBAL>();
    // positions of the chain elements into tail_pos[0 .. longest)
    for (u32 m = lane; m < longest; m += 64) tail_pos[m] = p[tail_idx[m]];
    chain_sync<GLOBAL>();
  }
  chain_emit_wave([&](u32 m) { return tail_pos[m]; }, longest, strand, g0, lhs_id, k, chain, min_matches, gap, slots,
                  slot_flags, anchors, anchor_base, slot_aoff, slot_acnt);
}

// dynamic LDS of chain_kernel for a class of kChainClassTable (sizeclass.h)
inline size_t chain_class_lds(u32 cap) {
  return static_cast<size_t>(cap + 1) * 8 + (cap / 64 + 2) * 8 + static_cast<size_t>(cap + 2) * 2 + static_cast<size_t>(cap) * 2 + 64;
}

__global__ __launch_bounds__(64) void chain_kernel(const u64* __restrict__ grp, const u64* __restrict__ pos,
                                                  const u64* __restrict__ iv_begin, const u64* __restrict__ iv_end,
                                                  const u32* __restrict__ iv_read, const u32* __restrict__ list,
                                                  u32 n_list, u32 cap, const u32* __restrict__ ids, u32 first, u32 k,
                                                  u32 chain, u32 min_matches, u32 gap, u32 slot_div,
                                                  u64* __restrict__ g_tail_pos, u32* __restrict__ g_tail_idx,
                                                  u32* __restrict__ g_pred, u64* __restrict__ g_mask,
                                                  Overlap* __restrict__ slots, u8* __restrict__ slot_flags,
                                                  u64* __restrict__ anchors, u64* __restrict__ slot_aoff,
                                                  u32* __restrict__ slot_acnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char chain_smem[];
  if (blockIdx.x >= n_list) return;
  const u32 t = list[blockIdx.x];
  const u64 b = iv_begin[t];
  const u32 n = static_cast<u32>(iv_end[t] - b);
  const u64 g0 = grp[b];
  const bool strand = (g0 >> 32) & 1;
  const u32 lhs_id = ids[first + iv_read[t]];
  const u64 slot_base = (b + slot_div - 1) / slot_div;
  if (cap) {
    u64* tail_pos = reinterpret_cast<u64*>(chain_smem);
    u64* maskbuf = tail_pos + (cap + 1);
    u16* tail_idx = reinterpret_cast<u16*>(maskbuf + (cap / 64 + 2));
    u16* pred = tail_idx + (cap + 2);
    chain_wave<u16, false>(pos + b, n, strand, g0, lhs_id, k, chain, min_matches, gap, tail_pos, tail_idx, pred, maskbuf,
                           slots + slot_base, slot_flags + slot_base, anchors ? anchors + b : nullptr, b,
                           slot_aoff ? slot_aoff + slot_base : nullptr, slot_acnt ? slot_acnt + slot_base : nullptr);
  } else {
    chain_wave<u32, true>(pos + b, n, strand, g0, lhs_id, k, chain, min_matches, gap, g_tail_pos + b + t,
                          g_tail_idx + b + t, g_pred + b, g_mask + (b >> 6) + t, slots + slot_base,
                          slot_flags + slot_base, anchors ? anchors + b : nullptr, b,
                          slot_aoff ? slot_aoff + slot_base : nullptr, slot_acnt ? slot_acnt + slot_base : nullptr);
  }
}

__global__ void compact_overlaps_kernel(const Overlap* __restrict__ slots, const u8* __restrict__ flags,
                                        const u32* __restrict__ scan, u64 n_slots, Overlap* __restrict__ out) {
  u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n_slots && flags[i]) out[scan[i]] = slots[i];
}

__global__ void compact_aux_kernel(const u64* __restrict__ slot_aoff, const u32* __restrict__ slot_acnt,
                                   const u8* __restrict__ flags, const u32* __restrict__ scan, u64 n_slots,
                                   u64* __restrict__ aoff, u32* __restrict__ acnt) {
  u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n_slots && flags[i]) {
    aoff[scan[i]] = slot_aoff[i];
    acnt[scan[i]] = slot_acnt[i];
  }
}

__global__ void read_ovl_off_kernel(const u64* __restrict__ seg_off, const u32* __restrict__ scan, u32 slot_div,
                                    u32 n, u32* __restrict__ out) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = scan[(seg_off[i] + slot_div - 1) / slot_div];
}

}  // namespace

// The largest classes of both sorts and of chain_kernel are launched with more than 64 KB of dynamic LDS, which a kernel
// has to be allowed on the device it runs on: called once for every engine, on its device, where the engine is created.
void chain_allow_big_lds() {
  seg_sort_allow_lds<true>(kSegClassTable.cap[kSegClassTable.n_classes - 1]);
  seg_sort_allow_lds<false>(kChainBigCap);
  RVN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(chain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(chain_class_lds(kChainBigCap))));
}

// Chain stage: matches of reads [first, last) are in e.map.m_grp[0] / e.map.m_pos[0] (both ping-pong sides reserved for
// H + 1 entries: MapState::reserve_matches), segmented per read by e.map.seg_off[nr + 1] -> overlaps in (read, emission)
// order in `out`.  (ram Map after the index probes: sort by group, diagonal bands, per-band LIS, overlap emission.)
void chain_matches(Engine& e, const ReadsDev& r, u32 first, u32 last, u64 H, MapOut& out) {
  hipStream_t s = e.stream;
  const u32 nr = last - first;
  u32* ovl_read_off = out.ovl_read_off.get<u32>(static_cast<size_t>(nr) + 1);
  u64* seg_off = e.map.seg_off.as<u64>();
  if (H == 0) {
    RVN_HIP(hipMemsetAsync(ovl_read_off, 0, (static_cast<size_t>(nr) + 1) * 4, s));
    return;
  }
  u64* g0 = e.map.m_grp[0].as<u64>();
  u64* g1 = e.map.m_grp[1].as<u64>();
  u64* p0 = e.map.m_pos[0].as<u64>();
  u64* p1 = e.map.m_pos[1].as<u64>();
  {
    StageTimer t(e, StageTimes::kSegSort);
    seg_sort<true>(e, kKSegSortGroup, kSegClassTable, kSegClassMin, seg_off, seg_off + 1, nr, g0, g1, p0, p1);
    t.stop();
  }
  u32 NI = 0;
  const u64 n_slots4 = (H + 3) / 4 + 1;
  {
    StageTimer t(e, StageTimes::kIntervals);
    u64* slot_begin = e.map.iv_slot_begin.get<u64>(n_slots4 + 1);
    u64* slot_end = e.map.iv_slot_end.get<u64>(n_slots4 + 1);
    u32* iv_cnt = e.map.iv_cnt.get<u32>(static_cast<size_t>(nr) + 1);
    u32* iv_off = e.map.iv_off.get<u32>(static_cast<size_t>(nr) + 2);
    RVN_KLAUNCH(kKIntervals, intervals_kernel<<<div_up(nr, 4), 256, 0, s>>>(g0, seg_off, nr, e.bandwidth, slot_begin, slot_end, iv_cnt));
    exclusive_scan_u32_u32(iv_cnt, iv_off, nr, e.scratch.scan_tmp, s);
    NI = static_cast<u32>(read_back(e, iv_off + nr, 4));
    out.n_intervals = NI;
    if (NI) {
      u64* iv_begin = e.map.iv_begin.get<u64>(static_cast<size_t>(NI) + 1);
      u64* iv_end = e.map.iv_end.get<u64>(static_cast<size_t>(NI) + 1);
      u32* iv_read = e.scratch.tmp_b.get<u32>(static_cast<size_t>(NI) + 1);
      RVN_KLAUNCH(kKIntervalsGather, intervals_gather_kernel<<<div_up(nr, 4), 256, 0, s>>>(
                                         slot_begin, slot_end, seg_off, iv_off, nr, iv_begin, iv_end, iv_read));
    }
    t.stop();
  }
  if (NI == 0) {
    RVN_HIP(hipMemsetAsync(ovl_read_off, 0, (static_cast<size_t>(nr) + 1) * 4, s));
    return;
  }
  const u32 slot_div = std::max(1u, std::min(4u, e.chain));
  const u64 n_slots = (H + slot_div - 1) / slot_div + 1;
  Overlap* slots = e.map.ovl_slots.get<Overlap>(n_slots + 1);
  u8* slot_flags = e.map.ovl_flags.get<u8>(n_slots + 1);
  {
    StageTimer t(e, StageTimes::kChain);
    u64* iv_begin = e.map.iv_begin.as<u64>();
    u64* iv_end = e.map.iv_end.as<u64>();
    u32* iv_read = e.scratch.tmp_b.as<u32>();
    // Position sort of every interval that chain_kernel will take, KEYS ONLY — the payload of rounds 1-5, the group words,
    // is the same (target, strand) for every match of an interval and nothing behind this sort reads a group word's diagonal
    // (the chain kernels take target and strand from the interval's first word), so it stays where it is.  The chain
    // kernels below go by the same lists and counts: one classification, one read-back for the stage.
    const SegClasses cls = seg_sort<false>(e, kKSegSortPos, kChainClassTable, chain_class_min(e.chain), iv_begin, iv_end, NI,
                                           p0, p1, nullptr, nullptr);
    u32* lis_min = e.map.lis_min.get<u32>(H + NI + 1);
    u32* lis_pred = e.map.lis_pred.get<u32>(H + 1);
    u64* lis_tail = e.map.lis_tail.get<u64>(H + NI + 1);
    u64* lis_mask = e.map.lis_mask.get<u64>((H >> 6) + NI + 2);
    RVN_HIP(hipMemsetAsync(slot_flags, 0, n_slots + 1, s));
    u64* anchors = nullptr;
    u64* slot_aoff = nullptr;
    u32* slot_acnt = nullptr;
    if (e.map.keep_anchors) {
      anchors = out.anchors.get<u64>(H + 1);
      slot_aoff = e.map.anc_slot_off.get<u64>(n_slots + 1);
      slot_acnt = e.map.anc_slot_cnt.get<u32>(n_slots + 1);
    }
    RVN_KLAUNCH(kKChainSmall, chain_small_kernel<<<div_up(NI, 64), 64, 0, s>>>(
                                  g0, p0, iv_begin, iv_end, iv_read, NI, r.id.as<u32>(), first, e.k, e.chain, e.matches,
                                  e.gap, slot_div, slots, slot_flags, anchors, slot_aoff, slot_acnt));
    // largest classes first: their waves run longest
    for (int c = kChainClassTable.n_classes; c >= 0; --c) {
      if (!cls.count[c]) continue;
      const u32 cap = c < kChainClassTable.n_classes ? kChainClassTable.cap[c] : 0u;
      const size_t lds = cap ? chain_class_lds(cap) : 0;
      RVN_KLAUNCH(kKChain, chain_kernel<<<cls.count[c], 64, lds, s>>>(g0, p0, iv_begin, iv_end, iv_read, cls.list(c),
                                                                      cls.count[c], cap, r.id.as<u32>(), first, e.k, e.chain,
                                                                      e.matches, e.gap, slot_div, lis_tail, lis_min, lis_pred,
                                                                      lis_mask, slots, slot_flags, anchors, slot_aoff, slot_acnt));
    }
    t.stop();
  }
  {
    StageTimer t(e, StageTimes::kCompact);
    u32* scan = e.map.ovl_scan.get<u32>(n_slots + 2);
    exclusive_scan_u8_u32(slot_flags, scan, n_slots, e.scratch.scan_tmp, s);
    const u32 O = static_cast<u32>(read_back(e, scan + n_slots, 4));
    out.n_overlaps = O;
    e.c_overlaps += O;
    Overlap* ovl = out.ovl.get<Overlap>(static_cast<size_t>(O) + 1);
    RVN_KLAUNCH(kKCompactOverlaps, compact_overlaps_kernel<<<div_up(n_slots, 256), 256, 0, s>>>(slots, slot_flags, scan, n_slots, ovl));
    out.has_anchors = e.map.keep_anchors;
    if (e.map.keep_anchors) {
      u64* aoff = out.anchor_off.get<u64>(static_cast<size_t>(O) + 1);
      u32* acnt = out.anchor_cnt.get<u32>(static_cast<size_t>(O) + 1);
      RVN_KLAUNCH(kKCompactOverlaps, compact_aux_kernel<<<div_up(n_slots, 256), 256, 0, s>>>(
                                         e.map.anc_slot_off.as<u64>(), e.map.anc_slot_cnt.as<u32>(), slot_flags, scan, n_slots,
                                         aoff, acnt));
    }
    RVN_KLAUNCH(kKGather, read_ovl_off_kernel<<<div_up(nr + 1, 256), 256, 0, s>>>(seg_off, scan, slot_div, nr + 1, ovl_read_off));
    t.stop();
  }
}

}  // namespace rvn

