// abi_shard.hip — C ABI (include/raven_hip.h): stage-level entry points of the sharded single-genome pass (SURVEY §8(e);
// host side raven_amd/sharded.py).  Where an entry point exists for host pointers and for device pointers (rvn_*_dev: the
// exchange buffers stay in HBM, torch tensors), both are wrappers of one function.
#include <cstring>
#include <memory>

#include "abi.h"

using namespace rvn;

// (every entry point below is declared extern "C" by raven_hip.h; the helpers between them are templates and file-local)

int rvn_shard_sketch(rvn_engine* h, const rvn_reads* rr, int index_minhash, uint64_t* count) {
  return guarded(h, h && rr && count, "[raven_hip] rvn_shard_sketch: NULL argument", [&](Engine& e) -> int {
    const ReadsDev& r = rr->r;
    StageTimer t(e, StageTimes::kSketch);
    e.sketch.query_ready = {};
    sketch_raw(e, r, 0, r.n, e.sketch.raw_sketch);
    if (index_minhash) {
      sketch_minhash(e, r, e.sketch.raw_sketch, e.sketch.index_sketch);
      e.sketch.shard_sketch_minhash = true;
      *count = e.sketch.index_sketch.count;
    } else {
      e.sketch.join_query_count = sketch_flag_queries(e, r, e.sketch.raw_sketch);  // minhash-selected entries get kQueryFlag
      e.sketch.shard_sketch_minhash = false;
      *count = e.sketch.raw_sketch.count;
    }
    for (u32 i = 0; i < r.n; ++i) e.c_index_bases += r.h_len[i];
    t.stop();
    RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

namespace {
__global__ void or_flags_kernel(u64* __restrict__ org, u64 n, u64 flags) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) org[i] |= flags;
}
}  // namespace

int rvn_shard_sketch_range(rvn_engine* h, const rvn_reads* rr, uint32_t first, uint32_t last, int index_minhash, int foreign,
                           uint64_t* count) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !rr || !count) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_sketch_range: NULL argument");
    Engine& e = h->e;
    const ReadsDev& r = rr->r;
    if (first > last || last > r.n) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_sketch_range: range beyond the read set");
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    StageTimer t(e, StageTimes::kSketch);
    e.sketch.query_ready = {};
    *count = 0;
    e.sketch.shard_sketch_minhash = (index_minhash != 0) || (foreign != 0);
    Sketch& res = e.sketch.shard_sketch_minhash ? e.sketch.index_sketch : e.sketch.raw_sketch;
    res.count = 0;
    if (first == last) {
      t.stop();
      return RVN_OK;
    }
    if (foreign) {
      // reads of an EARLIER index batch: only what Map() would look up for them — their minhash-selected minimizers — as
      // query-only entries.  The prefix [0, f_hi) of a late batch has no bound of its own (>= 12.9 Gbases at w = 5
      // are >= 2^32 raw minimizers, and the sketch's offsets are 32-bit), so it is sketched in pieces of <= kForeignPieceBases
      // and the minhash-selected entries (at most len / k per read) are appended: what comes out is bounded by its own
      // count only, which the index build checks against 2^32 (index.hip).
      u64 piece_bases = kForeignPieceBases;
#if defined(RVN_DEBUG_KNOBS)
      if (const char* pb = knob("RVN_FOREIGN_PIECE_BASES")) piece_bases = std::strtoull(pb, nullptr, 10);  // (tests: several pieces on a small set)
#endif
      std::vector<u32> cuts{first};
      u64 acc = 0, bound = 0;
      for (u32 i = first; i < last; ++i) {
        if (acc && acc + r.h_len[i] > piece_bases) {
          cuts.push_back(i);
          acc = 0;
        }
        acc += r.h_len[i];
        bound += r.h_len[i] / static_cast<u32>(e.k) + 1;
      }
      cuts.push_back(last);
      if (cuts.size() == 2) {
        sketch_raw(e, r, first, last, e.sketch.raw_sketch);
        sketch_minhash(e, r, e.sketch.raw_sketch, e.sketch.index_sketch);
      } else {
        const size_t vb = e.val64 ? 8 : 4;
        unsigned char* av = e.sketch.foreign_val.get<unsigned char>((bound + 1) * vb);
        u64* ao = e.sketch.foreign_org.get<u64>(bound + 1);
        u64 n_acc = 0;
        for (size_t c = 0; c + 1 < cuts.size(); ++c) {
          sketch_raw(e, r, cuts[c], cuts[c + 1], e.sketch.raw_sketch);
          sketch_minhash(e, r, e.sketch.raw_sketch, e.sketch.index_sketch);
          const u64 n = e.sketch.index_sketch.count;
          if (n_acc + n > bound) throw HipError("[raven_hip] rvn_shard_sketch_range: more selected minimizers than len / k per read");
          if (n) {
            RVN_HIP(hipMemcpyAsync(av + n_acc * vb, e.sketch.index_sketch.val.ptr, n * vb, hipMemcpyDeviceToDevice, e.stream));
            RVN_HIP(hipMemcpyAsync(ao + n_acc, e.sketch.index_sketch.org.ptr, n * 8, hipMemcpyDeviceToDevice, e.stream));
          }
          n_acc += n;
        }
        RVN_HIP(rvn_stream_sync(e.stream));
        e.sketch.index_sketch.val.swap(e.sketch.foreign_val);
        e.sketch.index_sketch.org.swap(e.sketch.foreign_org);
        e.sketch.index_sketch.first = first;
        e.sketch.index_sketch.last = last;
        e.sketch.index_sketch.count = n_acc;  // (read_off of the pieces is not kept: nothing downstream of a query-only sketch reads it)
      }
      const u64 n = e.sketch.index_sketch.count;
      if (n) {
        or_flags_kernel<<<static_cast<u32>((n + 255) / 256), 256, 0, e.stream>>>(e.sketch.index_sketch.org.as<u64>(), n, kQueryFlag | kForeignFlag);
        RVN_LAUNCH_CHECK();
      }
    } else if (index_minhash) {
      sketch_raw(e, r, first, last, e.sketch.raw_sketch);
      sketch_minhash(e, r, e.sketch.raw_sketch, e.sketch.index_sketch);
    } else {
      sketch_raw(e, r, first, last, e.sketch.raw_sketch);
      e.sketch.join_query_count = sketch_flag_queries(e, r, e.sketch.raw_sketch);  // minhash-selected entries get kQueryFlag
    }
    *count = res.count;
    if (!foreign)
      for (u32 i = first; i < last; ++i) e.c_index_bases += r.h_len[i];
    t.stop();
    RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

namespace {
__global__ void widen_u32_u64_kernel(const u32* __restrict__ src, u64* __restrict__ dst, u64 n) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
__global__ void narrow_u64_u32_kernel(const u64* __restrict__ src, u32* __restrict__ dst, u64 n) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = static_cast<u32>(src[i]);
}

int shard_sketch_fetch(rvn_engine* h, uint64_t* values, uint64_t* origins, hipMemcpyKind kind) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    Sketch& s = e.sketch.shard_sketch_minhash ? e.sketch.index_sketch : e.sketch.raw_sketch;
    RVN_HIP(hipSetDevice(e.device));
    if (kind == hipMemcpyDeviceToDevice) {
      if (s.count == 0) return RVN_OK;
      if (!values || !origins) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_sketch_fetch_dev: NULL argument");
      if (e.val64) put(e, values, s.val.ptr, s.count * 8, kind);
      else widen_u32_u64_kernel<<<static_cast<u32>((s.count + 255) / 256), 256, 0, e.stream>>>(s.val.as<u32>(), values, s.count);
    } else {
      fetch_values(e, s.val, s.count, values);
    }
    if (origins && s.count) put(e, origins, s.org.ptr, s.count * 8, kind);
    if (kind == hipMemcpyDeviceToDevice) RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

// n_flagged: the entries of `origins` that carry kQueryFlag
int shard_index_build(rvn_engine* h, const uint64_t* values, const uint64_t* origins, uint64_t n, int all_query, uint64_t n_flagged,
                      hipMemcpyKind kind, const char* what) {
  return guarded(h, h && !(n && (!values || !origins)), what, [&](Engine& e) -> int {
    Sketch& sk = e.sketch.index_sketch;
    sk.first = 0;
    sk.last = 0;
    sk.count = n;
    if (e.val64) {
      u64* dv = sk.val.get<u64>(n + 1);
      if (n) put(e, dv, values, n * 8, kind);
    } else if (kind == hipMemcpyHostToDevice) {
      std::vector<u32> tmp(n);
      for (u64 i = 0; i < n; ++i) tmp[i] = static_cast<u32>(values[i]);
      u32* dv = sk.val.get<u32>(n + 1);
      if (n) put(e, dv, tmp.data(), n * 4, kind);
    } else {
      u32* dv = sk.val.get<u32>(n + 1);
      if (n) narrow_u64_u32_kernel<<<static_cast<u32>((n + 255) / 256), 256, 0, e.stream>>>(values, dv, n);
    }
    u64* dorg = sk.org.get<u64>(n + 1);
    if (n) put(e, dorg, origins, n * 8, kind);
    e.c_index_min += n;
    index_build(e, sk, false);
    e.c_index_keys += e.sketch.index.u;
    e.sketch.index.has_query_flags = !all_query;
    e.sketch.index.all_query = all_query != 0;
    e.sketch.join_query_count = all_query ? n : n_flagged;
    RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}
}  // namespace

int rvn_shard_sketch_fetch(rvn_engine* h, uint64_t* values, uint64_t* origins) {
  return shard_sketch_fetch(h, values, origins, hipMemcpyDeviceToHost);
}
int rvn_shard_sketch_fetch_dev(rvn_engine* h, uint64_t* d_values, uint64_t* d_origins) {
  return shard_sketch_fetch(h, d_values, d_origins, hipMemcpyDeviceToDevice);
}

int rvn_shard_index_build(rvn_engine* h, const uint64_t* values, const uint64_t* origins, uint64_t n, int all_query) {
  u64 flagged = 0;
  if (origins)
    for (u64 i = 0; i < n; ++i) flagged += (origins[i] & kQueryFlag) ? 1 : 0;
  return shard_index_build(h, values, origins, n, all_query, flagged, hipMemcpyHostToDevice,
                           "[raven_hip] rvn_shard_index_build: NULL argument");
}
int rvn_shard_index_build_dev(rvn_engine* h, const uint64_t* d_values, const uint64_t* d_origins, uint64_t n,
                              int all_query, uint64_t n_flagged) {
  return shard_index_build(h, d_values, d_origins, n, all_query, n_flagged, hipMemcpyDeviceToDevice,
                           "[raven_hip] rvn_shard_index_build_dev: NULL argument");
}

int rvn_shard_key_counts(rvn_engine* h, uint32_t* counts) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    const u64 u = e.sketch.index.u;
    if (u == 0) return RVN_OK;
    if (!counts) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_key_counts: NULL argument");
    RVN_HIP(hipSetDevice(e.device));
    std::vector<u32> st(u + 1);
    RVN_HIP(hipMemcpy(st.data(), e.sketch.index.u_start.ptr, (u + 1) * 4, hipMemcpyDeviceToHost));
    // (members only: query-only entries of reads outside the index batch, kForeignFlag, are the front of their run; a run
    // without members reports 0 and the caller drops it)
    std::vector<u64> so(e.sketch.index.m);
    if (e.sketch.index.m) RVN_HIP(hipMemcpy(so.data(), e.sketch.index.s_org[e.sketch.index.cur].ptr, e.sketch.index.m * 8, hipMemcpyDeviceToHost));
    for (u64 i = 0; i < u; ++i) counts[i] = st[i + 1] - st[i] - run_foreign_prefix(so.data(), st[i], st[i + 1] - st[i]);
    return RVN_OK;
  });
}

int rvn_shard_key_histogram(rvn_engine* h, uint64_t* hist, uint32_t* over, uint32_t over_cap, uint32_t* n_over) {
  return guarded(h, h && hist && n_over, "[raven_hip] rvn_shard_key_histogram: NULL argument", [&](Engine& e) -> int {
    std::vector<u64> hv;
    std::vector<u32> ov;
    index_key_histogram(e, hv, ov);
    for (size_t i = 0; i < hv.size(); ++i) hist[i] = hv[i];
    *n_over = static_cast<u32>(ov.size());
    if (ov.size() > over_cap) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_key_histogram: overflow list does not fit");
    for (size_t i = 0; i < ov.size(); ++i) over[i] = ov[i];
    return RVN_OK;
  });
}

int rvn_shard_join(rvn_engine* h, uint32_t n_reads_total, int avoid_equal, int avoid_symmetric, uint64_t* n_matches) {
  return rvn_shard_join_range(h, n_reads_total, avoid_equal, avoid_symmetric, 0, n_reads_total, n_matches);
}

int rvn_shard_join_range(rvn_engine* h, uint32_t n_reads_total, int avoid_equal, int avoid_symmetric, uint32_t query_first,
                         uint32_t query_last, uint64_t* n_matches) {
  return guarded(h, h && n_matches, "[raven_hip] rvn_shard_join: NULL argument", [&](Engine& e) -> int {
    e.map.shard_join_reads = n_reads_total;
    e.map.shard_join_matches = join_index_matches(e, n_reads_total, avoid_equal != 0, avoid_symmetric != 0, query_first, query_last);
    *n_matches = e.map.shard_join_matches;
    RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

namespace {
int shard_join_fetch(rvn_engine* h, uint64_t* grp, uint64_t* pos, uint64_t* seg_off, hipMemcpyKind kind) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    const u64 H = e.map.shard_join_matches;
    if (H && grp) put(e, grp, e.map.m_grp[0].ptr, H * 8, kind);
    if (H && pos) put(e, pos, e.map.m_pos[0].ptr, H * 8, kind);
    if (seg_off) put(e, seg_off, e.map.seg_off.ptr, (static_cast<size_t>(e.map.shard_join_reads) + 1) * 8, kind);
    if (kind == hipMemcpyDeviceToDevice) RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

// n_matches == nullptr: seg_off is a host array and names the number of matches itself
int shard_chain(rvn_engine* h, const rvn_reads* own, const uint64_t* grp, const uint64_t* pos, const uint64_t* seg_off,
                const uint64_t* n_matches, uint64_t* n_overlaps, hipMemcpyKind kind, const char* who) {
  const std::string what = std::string("[raven_hip] ") + who;
  return guarded(h, h && own && seg_off && n_overlaps, (what + ": NULL argument").c_str(), [&](Engine& e) -> int {
    const ReadsDev& r = own->r;
    const u32 nr = r.n;
    const u64 H = n_matches ? *n_matches : seg_off[nr];
    if (H && (!grp || !pos)) return fail(RVN_EINVAL, what + ": NULL matches");
    u64* d_seg = e.map.seg_off.get<u64>(static_cast<size_t>(nr) + 2);
    put(e, d_seg, seg_off, (static_cast<size_t>(nr) + 1) * 8, kind);
    e.map.reserve_matches(H);
    if (H) {
      put(e, e.map.m_grp[0].as<u64>(), grp, H * 8, kind);
      put(e, e.map.m_pos[0].as<u64>(), pos, H * 8, kind);
    }
    MapOut& out = e.map.out;
    out.first = 0;
    out.last = nr;
    out.n_query = 0;
    out.n_matches = H;
    out.n_intervals = out.n_overlaps = 0;
    for (u32 i = 0; i < nr; ++i) e.c_query_bases += r.h_len[i];
    chain_matches(e, r, 0, nr, H, out);
    e.c_intervals += out.n_intervals;
    RVN_HIP(rvn_stream_sync(e.stream));
    *n_overlaps = out.n_overlaps;
    return RVN_OK;
  });
}
}  // namespace

int rvn_shard_join_fetch(rvn_engine* h, uint64_t* grp, uint64_t* pos, uint64_t* seg_off) {
  return shard_join_fetch(h, grp, pos, seg_off, hipMemcpyDeviceToHost);
}
int rvn_shard_join_fetch_dev(rvn_engine* h, uint64_t* d_grp, uint64_t* d_pos, uint64_t* d_seg_off) {
  return shard_join_fetch(h, d_grp, d_pos, d_seg_off, hipMemcpyDeviceToDevice);
}

int rvn_shard_chain(rvn_engine* h, const rvn_reads* own, const uint64_t* grp, const uint64_t* pos,
                    const uint64_t* seg_off, uint64_t* n_overlaps) {
  return shard_chain(h, own, grp, pos, seg_off, nullptr, n_overlaps, hipMemcpyHostToDevice, "rvn_shard_chain");
}
int rvn_shard_chain_dev(rvn_engine* h, const rvn_reads* own, const uint64_t* d_grp, const uint64_t* d_pos,
                        const uint64_t* d_seg_off, uint64_t n_matches, uint64_t* n_overlaps) {
  return shard_chain(h, own, d_grp, d_pos, d_seg_off, &n_matches, n_overlaps, hipMemcpyDeviceToDevice, "rvn_shard_chain_dev");
}

int rvn_shard_piles_create(rvn_engine* h, const uint32_t* lengths, uint32_t n_reads_total, rvn_pass1** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !lengths || !out) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_piles_create: NULL argument");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    std::unique_ptr<rvn_pass1> p(new rvn_pass1(e));
    // metadata-only read set: piles need lengths and ids (== indices), not bases
    p->meta.reset(new ReadsDev());
    ReadsDev& meta = *p->meta;
    meta.n = n_reads_total;
    meta.h_len.assign(lengths, lengths + n_reads_total);
    meta.h_id.resize(n_reads_total);
    for (u32 i = 0; i < n_reads_total; ++i) meta.h_id[i] = i;
    meta.ids_are_indices = true;
    u32* d_len = meta.len.get<u32>(static_cast<size_t>(n_reads_total) + 1);
    u32* d_id = meta.id.get<u32>(static_cast<size_t>(n_reads_total) + 1);
    if (n_reads_total) {
      RVN_HIP(hipMemcpy(d_len, meta.h_len.data(), static_cast<size_t>(n_reads_total) * 4, hipMemcpyHostToDevice));
      RVN_HIP(hipMemcpy(d_id, meta.h_id.data(), static_cast<size_t>(n_reads_total) * 4, hipMemcpyHostToDevice));
    }
    piles_init(e, meta, p->ps);
    *out = p.release();
    return RVN_OK;
  });
}

namespace {
// One flush (construct.cc:79-110) of a sharded pass: merge the Map outputs of the window into the piles, AddLayers, truncate.
// fill(e, mo, n_reads_total) puts the window's overlaps (grouped by lhs read) and their per-read offsets into mo.
template <typename Fill>
int shard_piles_merge(rvn_pass1* p, bool args_ok, const char* what, uint32_t kmax, Fill fill) {
  return guarded(p ? p->e : nullptr, [&]() -> int {
    if (!args_ok) return fail(RVN_EINVAL, what);
    Engine& e = *p->e;
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    const u32 n_reads_total = p->meta->n;
    MapOut mo;
    mo.first = 0;
    mo.last = n_reads_total;
    const int rc = fill(e, mo, n_reads_total);
    if (rc != RVN_OK) return rc;
    piles_merge(e, *p->meta, mo, kmax, p->ps);
    RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

// rvn_shard_piles / _dev: a pass created, one merge, the pass destroyed again if the merge fails
template <typename Merge>
int shard_piles(rvn_engine* h, const uint32_t* lengths, uint32_t n_reads_total, rvn_pass1** out, const char* what, Merge merge) {
  if (!out) return fail(RVN_EINVAL, what);
  rvn_pass1* p = nullptr;
  int rc = rvn_shard_piles_create(h, lengths, n_reads_total, &p);
  if (rc != RVN_OK) return rc;
  rc = merge(p);
  if (rc != RVN_OK) {
    rvn_pass1_destroy(p);
    return rc;
  }
  *out = p;
  return RVN_OK;
}
}  // namespace

int rvn_shard_piles_merge(rvn_pass1* p, const rvn_overlap* overlaps, uint64_t n, uint32_t kmax) {
  return shard_piles_merge(p, p && p->meta && !(n && !overlaps), "[raven_hip] rvn_shard_piles_merge: bad handle or NULL overlaps", kmax,
                           [&](Engine&, MapOut& mo, u32 n_reads_total) -> int {
    // overlaps arrive in (query read k, emission) order; per-k offsets as Map would have produced them
    std::vector<u32> off(static_cast<size_t>(n_reads_total) + 1, 0);
    const Overlap* ov = reinterpret_cast<const Overlap*>(overlaps);
    u32 prev = 0;
    for (u64 i = 0; i < n; ++i) {
      if (ov[i].lhs_id >= n_reads_total || ov[i].rhs_id >= n_reads_total || ov[i].lhs_id < prev)
        return fail(RVN_EINVAL, "[raven_hip] rvn_shard_piles: overlaps must be ordered by lhs_id and ids < n_reads");
      // pile_build_kernel puts every reversed overlap of a pile before the pile's own: construct.cc:72-77 only when the
      // reversed ones come from earlier queries (Map with avoid_equal and avoid_symmetric)
      if (ov[i].lhs_id >= ov[i].rhs_id)
        return fail(RVN_EINVAL, "[raven_hip] rvn_shard_piles: every overlap must have lhs_id < rhs_id");
      prev = ov[i].lhs_id;
      ++off[ov[i].lhs_id + 1];
    }
    for (u32 i = 0; i < n_reads_total; ++i) off[i + 1] += off[i];
    mo.n_overlaps = n;
    Overlap* d_ov = mo.ovl.get<Overlap>(n + 1);
    if (n) RVN_HIP(hipMemcpy(d_ov, ov, n * sizeof(Overlap), hipMemcpyHostToDevice));
    u32* d_off = mo.ovl_read_off.get<u32>(off.size());
    RVN_HIP(hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    return RVN_OK;
  });
}

int rvn_shard_piles_merge_dev(rvn_pass1* p, const rvn_overlap* d_overlaps, const uint32_t* d_ovl_read_off, uint64_t n,
                              uint32_t kmax) {
  return shard_piles_merge(p, p && p->meta && d_ovl_read_off && !(n && !d_overlaps),
                           "[raven_hip] rvn_shard_piles_merge_dev: bad handle or NULL argument", kmax,
                           [&](Engine& e, MapOut& mo, u32 n_reads_total) -> int {
    mo.n_overlaps = n;
    Overlap* d_ov = mo.ovl.get<Overlap>(n + 1);
    if (n) RVN_HIP(hipMemcpyAsync(d_ov, d_overlaps, n * sizeof(Overlap), hipMemcpyDeviceToDevice, e.stream));
    u32* d_off = mo.ovl_read_off.get<u32>(static_cast<size_t>(n_reads_total) + 1);
    RVN_HIP(hipMemcpyAsync(d_off, d_ovl_read_off, (static_cast<size_t>(n_reads_total) + 1) * 4, hipMemcpyDeviceToDevice,
                           e.stream));
    return RVN_OK;
  });
}

int rvn_shard_piles_merge_parts_dev(rvn_pass1* p, uint32_t n_parts, const rvn_overlap* const* d_parts,
                                    const uint64_t* n_per_part, uint32_t kmax) {
  return shard_piles_merge(p, p && p->meta && !(n_parts && (!d_parts || !n_per_part)),
                           "[raven_hip] rvn_shard_piles_merge_parts_dev: bad handle or NULL argument", kmax,
                           [&](Engine& e, MapOut& mo, u32 n_reads_total) -> int {
    u64 n = 0;
    for (u32 i = 0; i < n_parts; ++i) n += n_per_part[i];
    mo.n_overlaps = n;
    Overlap* d_ov = mo.ovl.get<Overlap>(n + 1);
    u64 at = 0;
    for (u32 i = 0; i < n_parts; ++i) {  // parts in ascending lhs-owner order: the list stays grouped by lhs read
      if (n_per_part[i])
        RVN_HIP(hipMemcpyAsync(d_ov + at, d_parts[i], n_per_part[i] * sizeof(Overlap), hipMemcpyDeviceToDevice, e.stream));
      at += n_per_part[i];
    }
    u32* d_off = mo.ovl_read_off.get<u32>(static_cast<size_t>(n_reads_total) + 1);
    shard_lhs_offsets(e, d_ov, n, n_reads_total, d_off);
    return RVN_OK;
  });
}

int rvn_shard_piles(rvn_engine* h, const uint32_t* lengths, uint32_t n_reads_total, const rvn_overlap* overlaps,
                    uint64_t n, uint32_t kmax, rvn_pass1** out) {
  return shard_piles(h, lengths, n_reads_total, out, "[raven_hip] rvn_shard_piles: NULL argument",
                     [&](rvn_pass1* p) { return rvn_shard_piles_merge(p, overlaps, n, kmax); });
}
int rvn_shard_piles_dev(rvn_engine* h, const uint32_t* lengths, uint32_t n_reads_total, const rvn_overlap* d_overlaps,
                        const uint32_t* d_ovl_read_off, uint64_t n, uint32_t kmax, rvn_pass1** out) {
  return shard_piles(h, lengths, n_reads_total, out, "[raven_hip] rvn_shard_piles_dev: NULL argument",
                     [&](rvn_pass1* p) { return rvn_shard_piles_merge_dev(p, d_overlaps, d_ovl_read_off, n, kmax); });
}

// ---- partition / regroup steps of the sharded pass on device pointers (shard.hip) ----
int rvn_shard_split_minimizers_dev(rvn_engine* h, const uint64_t* d_values, const uint64_t* d_origins, uint64_t n,
                                   uint32_t world, uint64_t* d_values_out, uint64_t* d_origins_out, uint64_t* counts) {
  const bool ok = h && counts && world != 0 && world <= 16 && !(n && (!d_values || !d_origins || !d_values_out || !d_origins_out));
  return guarded(h, ok, "[raven_hip] rvn_shard_split_minimizers_dev: bad argument", [&](Engine& e) -> int {
    shard_split_minimizers(e, d_values, d_origins, n, world, d_values_out, d_origins_out, counts);
    return RVN_OK;
  });
}

int rvn_shard_split_overlaps_dev(rvn_engine* h, const rvn_overlap* d_overlaps, uint64_t n, const uint32_t* bounds,
                                 uint32_t world, uint32_t self, rvn_overlap* d_out, uint64_t* counts) {
  const bool ok = h && counts && bounds && world != 0 && world <= 16 && self < world && !(n && (!d_overlaps || !d_out));
  return guarded(h, ok, "[raven_hip] rvn_shard_split_overlaps_dev: bad argument", [&](Engine& e) -> int {
    shard_split_overlaps(e, reinterpret_cast<const Overlap*>(d_overlaps), n, bounds, world, self,
                         reinterpret_cast<Overlap*>(d_out), counts);
    return RVN_OK;
  });
}

int rvn_shard_count_flagged_dev(rvn_engine* h, const uint64_t* d_origins, uint64_t n, uint64_t* count) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !count || (n && !d_origins)) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_count_flagged_dev: bad argument");
    RVN_HIP(hipSetDevice(h->e.device));
    *count = shard_count_flagged(h->e, d_origins, n);
    return RVN_OK;
  });
}

int rvn_shard_adjacent_diff_dev(rvn_engine* h, const uint64_t* d_seg_off, uint64_t n, uint64_t* d_counts) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || (n && (!d_seg_off || !d_counts))) return fail(RVN_EINVAL, "[raven_hip] rvn_shard_adjacent_diff_dev: bad argument");
    RVN_HIP(hipSetDevice(h->e.device));
    shard_adjacent_diff(h->e, d_seg_off, n, d_counts);
    RVN_HIP(rvn_stream_sync(h->e.stream));
    return RVN_OK;
  });
}

int rvn_shard_regroup_dev(rvn_engine* h, uint32_t world, const uint64_t* const* d_counts, const uint64_t* const* d_group,
                          const uint64_t* const* d_positions, const uint64_t* n_per_source, uint32_t n_reads,
                          uint64_t* d_seg_off, uint64_t* d_group_out, uint64_t* d_positions_out) {
  const bool ok = h && world != 0 && world <= 16 && d_counts && d_group && d_positions && n_per_source && d_seg_off;
  return guarded(h, ok, "[raven_hip] rvn_shard_regroup_dev: bad argument", [&](Engine& e) -> int {
    shard_regroup(e, world, d_counts, d_group, d_positions, n_per_source, n_reads, d_seg_off, d_group_out, d_positions_out);
    RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

