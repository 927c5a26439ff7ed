// map.hip — batched ram::MinimizerEngine::Map (call site RavenLib/src/construct.cc:59-64, :377-381): the entry points and
// the MATCH stage, for a whole batch of query reads at once — query sketch -> index probe or self-join -> the reads'
// matches in e.map.m_grp[0] / m_pos[0], segmented per read by e.map.seg_off.  The chain stage takes them from there
// (chain.hip: sort by group -> diagonal-band intervals -> per-interval sort by positions -> LIS chain -> overlaps).
// Output order equals the reference's "for each query read in order, Map() output order".
//
// Kernels (all integer, HBM/L2-bound; no MFMA):
//   match_count / match_emit   one lane per query minimizer: direct-address entry, or bucket table + binary search
//   join<false> / join<true>   one lane per run of equal values of the sorted index: count, then emit (no probe at all)
#include <stdexcept>

#include "engine.h"
#include "wave.h"

namespace rvn {

namespace {

template <typename V>
__device__ __forceinline__ bool index_find(const V* __restrict__ u_val, const u32* __restrict__ u_start,
                                           const u32* __restrict__ table, int shift, V v, u32* start, u32* count) {
  const u32 b = static_cast<u32>(static_cast<u64>(v) >> shift);
  u32 lo = table[b], hi = table[b + 1];
  const u32 end = hi;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (u_val[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  if (lo < end && u_val[lo] == v) {
    *start = u_start[lo];
    *count = u_start[lo + 1] - *start;
    return true;
  }
  return false;
}

template <typename V>
__global__ void match_count_kernel(const V* __restrict__ q_val, const u64* __restrict__ q_org, u64 nq,
                                   const V* __restrict__ u_val, const u32* __restrict__ u_start,
                                   const u32* __restrict__ table, int shift, u32 n_keys,
                                   const u64* __restrict__ s_org, u32 occurrence, int avoid_equal,
                                   int avoid_symmetric, u32* __restrict__ q_start, u32* __restrict__ q_n,
                                   u32* __restrict__ q_cnt, u8* __restrict__ filtered, const u64* __restrict__ direct) {
  u64 q = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const V v = q_val[q];
  const u32 qid = origin_id(q_org[q]);
  u32 start = 0, count = 0, cnt = 0;
  u8 filt = 0;
  bool found;
  if (direct) {  // (index.hip: every value addressed directly — the same start / count the search below finds)
    const u64 ent = direct[static_cast<u64>(v)];
    count = static_cast<u32>(ent >> 32);
    found = count != 0;
    start = found ? static_cast<u32>(ent) : 0u;
  } else {
    found = n_keys && index_find<V>(u_val, u_start, table, shift, v, &start, &count);
  }
  if (found) {
    if (count > occurrence) {
      filt = 1;
      count = 0;
    } else {
      for (u32 j = 0; j < count; ++j) {
        const u32 rid = origin_id(s_org[start + j]);
        if (avoid_equal && qid == rid) continue;
        if (avoid_symmetric && qid > rid) continue;
        ++cnt;
      }
    }
  }
  q_start[q] = start;
  q_n[q] = count;
  q_cnt[q] = cnt;
  if (filtered) filtered[q] = filt;
}

__global__ void match_emit_kernel(const u64* __restrict__ q_org, u64 nq, const u64* __restrict__ s_org,
                                  const u32* __restrict__ q_start, const u32* __restrict__ q_n,
                                  const u64* __restrict__ m_off, int avoid_equal, int avoid_symmetric,
                                  u64* __restrict__ m_grp, u64* __restrict__ m_pos) {
  u64 q = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const u32 count = q_n[q];
  if (count == 0) return;
  const u64 qo = q_org[q];
  const u32 qid = origin_id(qo);
  const u64 lhs_pos = static_cast<u32>(qo) >> 1;
  const u32 qstrand = static_cast<u32>(qo) & 1u;
  const u32 start = q_start[q];
  u64 o = m_off[q];
  for (u32 j = 0; j < count; ++j) {
    const u64 ro = s_org[start + j];
    const u32 rid = origin_id(ro);
    if (avoid_equal && qid == rid) continue;
    if (avoid_symmetric && qid > rid) continue;
    const u64 rhs_pos = static_cast<u32>(ro) >> 1;
    const u64 strand = (qstrand == (static_cast<u32>(ro) & 1u)) ? 1 : 0;
    const u64 diagonal = !strand ? rhs_pos + lhs_pos : rhs_pos - lhs_pos + (3ULL << 30);
    m_grp[o] = (((static_cast<u64>(rid) << 1) | strand) << 32) | diagonal;
    m_pos[o] = (lhs_pos << 32) | rhs_pos;
    ++o;
  }
}

// ---- self-join over the sorted index ----------------------------------------------------------------
// When the query reads are exactly the indexed reads, every query minimizer is itself an index entry
// (flagged kQueryFlag), so Map's probes become one streaming pass over the runs of equal value: for each
// flagged entry of a run (count <= occurrence), every other entry of the run is a match.  No table, no random
// access (the probe path fetched ~3 GB of cache lines per pass, profiles/r01_c_pmc_fetch_size.csv).
// Matches of one read land in that read's segment in arbitrary order; the result does not depend on it
// because the following sorts are total orders (group, then positions).
template <bool EMIT>
__global__ __launch_bounds__(256) void join_kernel(const u32* __restrict__ u_start, u32 n_runs,
                                                  const u64* __restrict__ s_org, u32 occurrence, int all_query,
                                                  int avoid_equal, int avoid_symmetric, u32 first, u32 q_lo, u32 q_hi,
                                                  u32* __restrict__ read_cnt, const u64* __restrict__ seg_off,
                                                  u32* __restrict__ cursor, u64* __restrict__ m_grp,
                                                  u64* __restrict__ m_pos) {
  const u32 run = blockIdx.x * blockDim.x + threadIdx.x;
  if (run >= n_runs) return;
  const u32 s = u_start[run];
  const u32 c = u_start[run + 1] - s;
  // entries [0, f) of the run are queries of reads outside this index batch (kForeignFlag): no members of the index
  const u32 f = run_foreign_prefix(s_org, s, c);
  if (c - f > occurrence || c == f) return;
  if (c == 1 && avoid_equal) return;
  for (u32 i = 0; i < c; ++i) {
    const u64 qo = s_org[s + i];
    if (!all_query && !(qo & kQueryFlag)) continue;
    const u32 qid = origin_id(qo);
    if (qid < q_lo || qid >= q_hi) continue;  // query reads of another flush window (sharded pass)
    u32 cnt = 0;
    for (u32 j = f; j < c; ++j) {
      const u32 rid = origin_id(s_org[s + j]);
      if (avoid_equal && qid == rid) continue;
      if (avoid_symmetric && qid > rid) continue;
      ++cnt;
    }
    if (cnt == 0) continue;
    if (!EMIT) {
      atomicAdd(&read_cnt[qid - first], cnt);
    } else {
      u64 o = seg_off[qid - first] + atomicAdd(&cursor[qid - first], cnt);
      const u64 lhs_pos = static_cast<u32>(qo) >> 1;
      const u32 qstrand = static_cast<u32>(qo) & 1u;
      for (u32 j = f; j < c; ++j) {
        const u64 ro = s_org[s + j];
        const u32 rid = origin_id(ro);
        if (avoid_equal && qid == rid) continue;
        if (avoid_symmetric && qid > rid) continue;
        const u64 rhs_pos = static_cast<u32>(ro) >> 1;
        const u64 strand = (qstrand == (static_cast<u32>(ro) & 1u)) ? 1 : 0;
        const u64 diagonal = !strand ? rhs_pos + lhs_pos : rhs_pos - lhs_pos + (3ULL << 30);
        m_grp[o] = (((static_cast<u64>(rid) << 1) | strand) << 32) | diagonal;
        m_pos[o] = (lhs_pos << 32) | rhs_pos;
        ++o;
      }
    }
  }
}

__global__ void gather_u64_by_u32_kernel(const u64* __restrict__ src, const u32* __restrict__ idx,
                                         u64* __restrict__ dst, u32 n) {
  u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}


template <typename V>
u64 match_probe_impl(Engine& e, const Sketch& qs, u32 nr, bool avoid_equal, bool avoid_symmetric, u8* filt, u64* seg_off) {
  hipStream_t s = e.stream;
  Index& ix = e.sketch.index;
  index_build_table(e);
  const u64 nq = qs.count;
  StageTimer t(e, StageTimes::kMatch);
  u32* q_start = e.map.q_start.get<u32>(nq + 1);
  u32* q_n = e.scratch.tmp_a.get<u32>(nq + 1);
  u32* q_cnt = e.map.q_cnt.get<u32>(nq + 1);
  u64* m_off = e.map.m_off.get<u64>(nq + 2);
  RVN_KLAUNCH(kKMatchCount, match_count_kernel<V><<<div_up(nq, 256), 256, 0, s>>>(
      qs.val.as<V>(), qs.org.as<u64>(), nq, ix.u_val.as<V>(), ix.u_start.as<u32>(), ix.table.as<u32>(), ix.shift,
      static_cast<u32>(ix.u), ix.s_org[ix.cur].as<u64>(), ix.occurrence, avoid_equal, avoid_symmetric, q_start, q_n,
      q_cnt, filt, ix.direct_built ? ix.direct.as<u64>() : nullptr));
  exclusive_scan_u32_u64(q_cnt, m_off, nq, e.scratch.scan_tmp, s);
  const u64 H = read_back(e, m_off + nq, 8);
  if (H) {
    e.map.reserve_matches(H);
    RVN_KLAUNCH(kKMatchEmit, match_emit_kernel<<<div_up(nq, 256), 256, 0, s>>>(
                                 qs.org.as<u64>(), nq, ix.s_org[ix.cur].as<u64>(), q_start, q_n, m_off, avoid_equal,
                                 avoid_symmetric, e.map.m_grp[0].as<u64>(), e.map.m_pos[0].as<u64>()));
    RVN_KLAUNCH(kKGather, gather_u64_by_u32_kernel<<<div_up(nr + 1, 256), 256, 0, s>>>(
                              e.map.m_off.as<u64>(), qs.read_off.as<u32>(), seg_off, nr + 1));
  }
  t.stop();
  return H;
}

// The self-join: segment i of the result holds the matches of the query read with id id_base + i.
struct JoinArgs {
  u32 n_seg;
  u32 id_base;
  u32 q_lo, q_hi;  // only query reads with q_lo <= id < q_hi (all: 0, 0xFFFFFFFF)
  bool all_query;  // every entry of the index is a query, flagged or not
  bool avoid_equal, avoid_symmetric;
};

// Its host sequence, stated once for the first pass (map_batch), the sharded pass (join_index_matches) and the polishing
// round (map_batch_query_only): matches per query read counted over the runs, scanned into e.map.seg_off[n_seg + 1], the
// match buffers reserved, the matches emitted into e.map.m_grp[0] / m_pos[0].  Returns their number H (added to e.c_matches).
// e.map.seg_off[0 .. n_seg] is written in every case: by the scan when the launches run — so nobody clears it ahead of
// them — and by a memset when they are skipped, which is when the index has no run or no member (H = 0, every segment
// empty; a grid of no blocks is no launch).  H == 0 skips the emit launch and leaves the match buffers as they are.
u64 self_join(Engine& e, const JoinArgs& a) {
  hipStream_t s = e.stream;
  Index& ix = e.sketch.index;
  StageTimer t(e, StageTimes::kMatch);
  u64* seg_off = e.map.seg_off.get<u64>(static_cast<size_t>(a.n_seg) + 2);
  const u32 n_runs = static_cast<u32>(ix.u);
  if (ix.m == 0 || n_runs == 0) {
    RVN_HIP(hipMemsetAsync(seg_off, 0, (static_cast<size_t>(a.n_seg) + 1) * 8, s));
    t.stop();
    return 0;
  }
  u32* read_cnt = e.map.q_cnt.get<u32>(2 * (static_cast<size_t>(a.n_seg) + 1));
  u32* cursor = read_cnt + a.n_seg + 1;
  RVN_HIP(hipMemsetAsync(read_cnt, 0, 2 * (static_cast<size_t>(a.n_seg) + 1) * 4, s));
  const u64* sorg = ix.s_org[ix.cur].as<u64>();
  RVN_KLAUNCH(kKJoinCount, join_kernel<false><<<div_up(n_runs, 256), 256, 0, s>>>(
                               ix.u_start.as<u32>(), n_runs, sorg, ix.occurrence, a.all_query, a.avoid_equal,
                               a.avoid_symmetric, a.id_base, a.q_lo, a.q_hi, read_cnt, nullptr, nullptr, nullptr, nullptr));
  exclusive_scan_u32_u64(read_cnt, seg_off, a.n_seg, e.scratch.scan_tmp, s);
  const u64 H = read_back(e, seg_off + a.n_seg, 8);
  e.c_matches += H;
  if (H) {
    e.map.reserve_matches(H);
    RVN_KLAUNCH(kKJoinEmit, join_kernel<true><<<div_up(n_runs, 256), 256, 0, s>>>(
                                ix.u_start.as<u32>(), n_runs, sorg, ix.occurrence, a.all_query, a.avoid_equal,
                                a.avoid_symmetric, a.id_base, a.q_lo, a.q_hi, nullptr, seg_off, cursor,
                                e.map.m_grp[0].as<u64>(), e.map.m_pos[0].as<u64>()));
  }
  t.stop();
  return H;
}

}  // namespace

// The probe branch of Map's match stage: every minimizer of the query sketch qs (nq = qs.count > 0 minimizers of nr reads,
// qs.read_off their per-read offsets) looked up in the engine's index (m > 0; its table is built here if it is not yet).
// The matches land in e.map.m_grp[0] / e.map.m_pos[0] in (query minimizer, run) order, their per-read offsets in seg_off[nr + 1]
// (not written when there is no match); filt (nullable): per-minimizer "skipped by the occurrence filter".  Returns the
// number of matches.  Called by map_batch and by the test hook rvn_test_match_probe (test_hooks.hip).
u64 match_probe(Engine& e, const Sketch& qs, u32 nr, bool avoid_equal, bool avoid_symmetric, u8* filt, u64* seg_off) {
  return e.val64 ? match_probe_impl<u64>(e, qs, nr, avoid_equal, avoid_symmetric, filt, seg_off)
                 : match_probe_impl<u32>(e, qs, nr, avoid_equal, avoid_symmetric, filt, seg_off);
}

void map_batch(Engine& e, const ReadsDev& r, u32 first, u32 last, bool avoid_equal, bool avoid_symmetric,
               bool minhash, bool want_filtered, MapOut& out) {
  hipStream_t s = e.stream;
  Index& ix = e.sketch.index;
  const u32 nr = last - first;
  out.first = first;
  out.last = last;
  out.n_query = out.n_matches = out.n_intervals = out.n_overlaps = 0;
  u32* ovl_read_off = out.ovl_read_off.get<u32>(static_cast<size_t>(nr) + 1);
  u64* seg_off = e.map.seg_off.get<u64>(static_cast<size_t>(nr) + 2);
  for (u32 i = first; i < last; ++i) e.c_query_bases += r.h_len[i];
  u64 H = 0;
  // self-join path: queries == indexed reads, flags in the index, bounded run lengths, ids == read indices
  const bool join = minhash && !want_filtered && ix.m != 0 && ix.first == first && ix.last == last &&
                    (ix.has_query_flags || ix.all_query) && ix.occurrence <= 4096 && r.ids_are_indices;
  if (join) {
    e.sketch.query_ready = {};
    out.n_query = ix.all_query ? ix.m : e.sketch.join_query_count;
    e.c_query_min += out.n_query;
    // (ids are read indices: read `first` has id `first`)
    H = self_join(e, JoinArgs{nr, first, 0u, 0xFFFFFFFFu, ix.all_query, avoid_equal, avoid_symmetric});
  } else {
    Sketch& qs = e.sketch.query_sketch;
    {
      StageTimer t(e, StageTimes::kQuery);
      const SketchState::QueryReady& q = e.sketch.query_ready;
      const bool ready = q.valid && q.first == first && q.last == last && q.minhash == minhash;
      e.sketch.query_ready = {};
      if (!ready) sketch_range(e, r, first, last, minhash, qs);
      t.stop();
    }
    const u64 nq = qs.count;
    out.n_query = nq;
    e.c_query_min += nq;
    if (nq == 0 || ix.m == 0) {
      RVN_HIP(hipMemsetAsync(ovl_read_off, 0, (static_cast<size_t>(nr) + 1) * 4, s));
      if (want_filtered) {
        u8* f = out.filtered.get<u8>(nq + 1);
        RVN_HIP(hipMemsetAsync(f, 0, nq + 1, s));
      }
      return;
    }
    H = match_probe(e, qs, nr, avoid_equal, avoid_symmetric, want_filtered ? out.filtered.get<u8>(nq + 1) : nullptr, seg_off);
    e.c_matches += H;
  }
  out.n_matches = H;
  chain_matches(e, r, first, last, H, out);
}

// Self-join of the whole (shard of the) index for query read ids 0..n_reads-1 (ids are global read indices):
// matches land in e.map.m_grp[0] / e.map.m_pos[0], segmented by query id through e.map.seg_off[n_reads + 1].  The hash-owner
// side of the sharded pass: the owner of a hash class joins its runs and ships every read's matches
// to the GPU that owns the read.  Returns the number of matches.
u64 join_index_matches(Engine& e, u32 n_reads, bool avoid_equal, bool avoid_symmetric, u32 q_lo, u32 q_hi) {
  const Index& ix = e.sketch.index;
  if (ix.m != 0 && ix.u != 0 && !(ix.has_query_flags || ix.all_query))
    throw std::invalid_argument("[raven_hip] join: index has no query flags");
  return self_join(e, JoinArgs{n_reads, 0u, q_lo, q_hi, ix.all_query, avoid_equal, avoid_symmetric});
}

// Map() of the reads [first, last) against an index in which their OWN minimizers sit as query-only entries (kQueryFlag |
// kForeignFlag, ahead of the members of every run: the polishing round's mapping, polish.hip).  One streaming pass over the
// runs instead of one random probe per query minimizer — what the first pass does when the queries are the indexed reads
// (join_kernel above), extended to queries that are not members.  n_query: the query-only entries (statistics).
void map_batch_query_only(Engine& e, const ReadsDev& r, u32 first, u32 last, u64 n_query, MapOut& out) {
  const u32 nr = last - first;
  out.first = first;
  out.last = last;
  out.n_query = n_query;
  out.n_matches = out.n_intervals = out.n_overlaps = 0;
  e.sketch.query_ready = {};
  for (u32 i = first; i < last; ++i) e.c_query_bases += r.h_len[i];
  e.c_query_min += n_query;
  const u64 H = self_join(e, JoinArgs{nr, r.h_id[first], 0u, 0xFFFFFFFFu, false, false, false});
  out.n_matches = H;
  chain_matches(e, r, first, last, H, out);
}

}  // namespace rvn
