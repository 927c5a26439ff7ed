// abi_overlap.hip — C ABI (include/raven_hip.h): Minimize / Filter / Map, the first and second pass of ConstructGraph,
// the identity filter and the pile hooks.
#include <chrono>
#include <cstring>
#include <memory>

#include "abi.h"
#include "overlap_rules.h"

using namespace rvn;

extern "C" {

int rvn_engine_minimize(rvn_engine* h, const rvn_reads* r, uint32_t first, uint32_t last, int minhash) {
  return guarded(h, h && r && first <= last && last <= r->r.n, "[raven_hip] rvn_engine_minimize: bad range", [&](Engine& e) -> int {
    engine_minimize(e, r->r, first, last, minhash != 0);
    RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}

int rvn_engine_filter(rvn_engine* h, double f) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    if (!(0 <= f && f <= 1)) return fail(RVN_EINVAL, "[ram::MinimizerEngine::Filter] error: invalid frequency");
    RVN_HIP(hipSetDevice(h->e.device));
    UseTimers ut(h->e);
    index_filter(h->e, f);
    return RVN_OK;
  });
}

uint32_t rvn_engine_occurrence(const rvn_engine* h) { return h ? h->e.sketch.index.occurrence : 0; }

int rvn_engine_set_occurrence(rvn_engine* h, uint32_t occurrence) {
  if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
  h->e.sketch.index.occurrence = occurrence;
  return RVN_OK;
}

int rvn_engine_map_batch(rvn_engine* h, const rvn_reads* r, uint32_t first, uint32_t last, int avoid_equal,
                         int avoid_symmetric, int minhash, int want_filtered, uint64_t* n_overlaps) {
  return guarded(h, h && r && first <= last && last <= r->r.n, "[raven_hip] rvn_engine_map_batch: bad range", [&](Engine& e) -> int {
    map_batch(e, r->r, first, last, avoid_equal != 0, avoid_symmetric != 0, minhash != 0, want_filtered != 0, e.map.out);
    e.c_intervals += e.map.out.n_intervals;
    RVN_HIP(rvn_stream_sync(e.stream));
    if (n_overlaps) *n_overlaps = e.map.out.n_overlaps;
    return RVN_OK;
  });
}

namespace {
// the last Map result out of the engine: to the host, or to device buffers of the caller's
int map_fetch(rvn_engine* h, rvn_overlap* overlaps, uint32_t* read_offsets, hipMemcpyKind kind) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    MapOut& m = e.map.out;
    RVN_HIP(hipSetDevice(e.device));
    if (overlaps && m.n_overlaps) put(e, overlaps, m.ovl.ptr, m.n_overlaps * sizeof(Overlap), kind);
    if (read_offsets) put(e, read_offsets, m.ovl_read_off.ptr, (static_cast<size_t>(m.last - m.first) + 1) * 4, kind);
    if (kind == hipMemcpyDeviceToDevice) RVN_HIP(rvn_stream_sync(e.stream));
    return RVN_OK;
  });
}
}  // namespace

int rvn_engine_map_fetch(rvn_engine* h, rvn_overlap* overlaps, uint32_t* read_offsets) {
  return map_fetch(h, overlaps, read_offsets, hipMemcpyDeviceToHost);
}
int rvn_engine_map_fetch_dev(rvn_engine* h, rvn_overlap* d_overlaps, uint32_t* d_read_offsets) {
  return map_fetch(h, d_overlaps, d_read_offsets, hipMemcpyDeviceToDevice);
}

int rvn_engine_map_fetch_filtered(rvn_engine* h, uint32_t* positions, uint32_t* read_offsets, uint64_t* total) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    MapOut& m = e.map.out;
    RVN_HIP(hipSetDevice(e.device));
    const u64 nq = m.n_query;
    const u32 nr = m.last - m.first;
    std::vector<u8> flags(nq);
    std::vector<u64> org(nq);
    std::vector<u32> roff(static_cast<size_t>(nr) + 1, 0);
    if (nq) {
      RVN_HIP(hipMemcpy(flags.data(), m.filtered.ptr, nq, hipMemcpyDeviceToHost));
      RVN_HIP(hipMemcpy(org.data(), e.sketch.query_sketch.org.ptr, nq * 8, hipMemcpyDeviceToHost));
    }
    RVN_HIP(hipMemcpy(roff.data(), e.sketch.query_sketch.read_off.ptr, roff.size() * 4, hipMemcpyDeviceToHost));
    u64 tot = 0;
    for (u32 i = 0; i < nr; ++i) {
      if (read_offsets) read_offsets[i] = static_cast<u32>(tot);
      for (u32 q = roff[i]; q < roff[i + 1]; ++q) {
        if (flags[q]) {
          if (positions) positions[tot] = static_cast<u32>(org[q]) >> 1;
          ++tot;
        }
      }
    }
    if (read_offsets) read_offsets[nr] = static_cast<u32>(tot);
    if (total) *total = tot;
    return RVN_OK;
  });
}

int rvn_engine_map_collect(rvn_engine* h, const rvn_reads* r, uint32_t first, uint32_t last, int avoid_equal,
                           int avoid_symmetric, int minhash, int want_filtered, rvn_overlap** overlaps,
                           uint32_t** read_offsets, uint32_t** filtered, uint32_t** filtered_offsets) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !r || !overlaps || !read_offsets || first > last || last > r->r.n)
      return fail(RVN_EINVAL, "[raven_hip] rvn_engine_map_collect: bad argument");
    if (want_filtered && (!filtered || !filtered_offsets))
      return fail(RVN_EINVAL, "[raven_hip] rvn_engine_map_collect: filtered requested without output pointers");
    *overlaps = nullptr;
    *read_offsets = nullptr;
    if (filtered) *filtered = nullptr;
    if (filtered_offsets) *filtered_offsets = nullptr;
    uint64_t n = 0;
    int rc = rvn_engine_map_batch(h, r, first, last, avoid_equal, avoid_symmetric, minhash, want_filtered, &n);
    if (rc != RVN_OK) return rc;
    const size_t nr = last - first;
    auto* ov = static_cast<rvn_overlap*>(std::malloc((n + 1) * sizeof(rvn_overlap)));
    auto* off = static_cast<uint32_t*>(std::malloc((nr + 1) * 4));
    uint32_t *fp = nullptr, *fo = nullptr;
    auto drop = [&]() {
      std::free(ov);
      std::free(off);
      std::free(fp);
      std::free(fo);
    };
    if (!ov || !off) {
      drop();
      return fail(RVN_ENOMEM, "[raven_hip] out of host memory");
    }
    rc = rvn_engine_map_fetch(h, ov, off);
    if (rc == RVN_OK && want_filtered) {
      uint64_t total = 0;
      rc = rvn_engine_map_fetch_filtered(h, nullptr, nullptr, &total);
      if (rc == RVN_OK) {
        fp = static_cast<uint32_t*>(std::malloc((total + 1) * 4));
        fo = static_cast<uint32_t*>(std::malloc((nr + 1) * 4));
        if (!fp || !fo) {
          drop();
          return fail(RVN_ENOMEM, "[raven_hip] out of host memory");
        }
        rc = rvn_engine_map_fetch_filtered(h, fp, fo, &total);
      }
    }
    if (rc != RVN_OK) {
      drop();
      return rc;
    }
    *overlaps = ov;
    *read_offsets = off;
    if (want_filtered) {
      *filtered = fp;
      *filtered_offsets = fo;
    }
    return RVN_OK;
  });
}

int rvn_find_overlaps_and_create_piles(rvn_engine* h, const rvn_reads* rr, double freq, uint32_t kmax,
                                       int use_minhash, uint64_t index_batch_bases, uint64_t flush_bases,
                                       rvn_pass1** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !rr || !out) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    if (!(0 <= freq && freq <= 1)) return fail(RVN_EINVAL, "[ram::MinimizerEngine::Filter] error: invalid frequency");
    Engine& e = h->e;
    const ReadsDev& r = rr->r;
    const bool dbg = knob("RVN_DEBUG_PASS1") != nullptr;  // host wall time per stage (synchronising)
    auto t_last = std::chrono::steady_clock::now();
    for (u32 i = 0; i < r.n; ++i)
      if (r.h_id[i] != i) return fail(RVN_EINVAL, "[raven_hip] FindOverlapsAndCreatePiles requires ids[i] == i");
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    if (dbg) std::fprintf(stderr, "[raven_hip] pass1: %-12s %8.1f ms\n", "timers",
                          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_last).count());
    engine_release_scratch_if_tight(e, 0);
    auto lap = [&](const char* what) {
      if (!dbg) return;
      (void)rvn_stream_sync(e.stream);
      const auto now = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[raven_hip] pass1: %-12s %8.1f ms\n", what,
                   std::chrono::duration<double, std::milli>(now - t_last).count());
      t_last = now;
    };
    std::unique_ptr<rvn_pass1> p(new rvn_pass1(e));
    lap("handle");
    piles_init(e, r, p->ps);
    lap("piles_init");
    const u32 n = r.n;
    // construct.cc:32-120
    u64 bytes = 0;
    for (u32 i = 0, j = 0; i < n; ++i) {
      bytes += r.h_len[i];
      if (i != n - 1 && bytes < index_batch_bases) continue;
      bytes = 0;
      // does the first query flush cover exactly the index range [j, i+1)?  (always true for one batch)
      bool prefetch = false;
      if (j == 0) {
        u64 fb = 0;
        u32 kk = 0;
        for (; kk < i + 1; ++kk) {
          fb += r.h_len[kk];
          if (kk != i && fb < flush_bases) continue;
          break;
        }
        prefetch = (kk == i);
      }
      engine_minimize(e, r, j, i + 1, use_minhash != 0, prefetch);
      lap("minimize");
      index_filter(e, freq);
      lap("filter");
      u32 flush_first = 0;
      for (u32 k = 0; k < i + 1; ++k) {
        bytes += r.h_len[k];
        if (k != i && bytes < flush_bases) continue;
        bytes = 0;
        map_batch(e, r, flush_first, k + 1, true, true, true, false, e.map.out);
        lap("map_batch");
        e.c_intervals += e.map.out.n_intervals;
        piles_merge(e, r, e.map.out, kmax, p->ps);
        lap("piles_merge");
        flush_first = k + 1;
      }
      j = i + 1;
    }
    RVN_HIP(rvn_stream_sync(e.stream));
    *out = p.release();
    return RVN_OK;
  });
}

uint64_t rvn_pass1_pile_words(const rvn_pass1* p) { return p ? p->ps.pile_words : 0; }
uint64_t rvn_pass1_num_overlaps(const rvn_pass1* p) { return p ? p->ps.kept_total : 0; }

int rvn_pass1_fetch_piles(const rvn_pass1* p, uint16_t* data, uint64_t* offsets) {
  return guarded(p ? p->e : nullptr, [&]() -> int {
    if (!p) return fail(RVN_EINVAL, "[raven_hip] NULL pass1");
    RVN_HIP(hipSetDevice(p->e->device));
    if (data && p->ps.pile_words)
      RVN_HIP(hipMemcpy(data, p->ps.pile_data.ptr, p->ps.pile_words * 2, hipMemcpyDeviceToHost));
    if (offsets)
      RVN_HIP(hipMemcpy(offsets, p->ps.pile_off.ptr, (static_cast<size_t>(p->ps.n) + 1) * 8, hipMemcpyDeviceToHost));
    return RVN_OK;
  });
}

int rvn_pass1_trim_and_annotate(rvn_pass1* p, uint32_t coverage, uint32_t* begin, uint32_t* end, uint16_t* median,
                                uint8_t* invalid) {
  return guarded(p ? p->e : nullptr, [&]() -> int {
    if (!p) return fail(RVN_EINVAL, "[raven_hip] NULL pass1");
    if (coverage > 65535) return fail(RVN_EINVAL, "[raven_hip] coverage threshold above 65535");
    RVN_HIP(hipSetDevice(p->e->device));
    UseTimers ut(*p->e);
    piles_trim_and_median(*p->e, p->ps, coverage, begin, end, median, invalid);
    return RVN_OK;
  });
}

int rvn_pass1_find_chimeric_regions(rvn_pass1* p, const uint8_t* invalid, uint32_t* region_offsets, uint32_t** regions) {
  return guarded(p ? p->e : nullptr, [&]() -> int {
    if (!p || !invalid || !region_offsets || !regions) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    *regions = nullptr;
    RVN_HIP(hipSetDevice(p->e->device));
    UseTimers ut(*p->e);
    std::vector<u32> off, reg;
    piles_find_chimeric_regions(*p->e, p->ps, invalid, off, reg);
    std::memcpy(region_offsets, off.data(), off.size() * 4);
    auto* out = static_cast<uint32_t*>(std::malloc((reg.size() + 1) * 4));
    if (!out) return fail(RVN_ENOMEM, "[raven_hip] out of host memory");
    if (!reg.empty()) std::memcpy(out, reg.data(), reg.size() * 4);
    *regions = out;
    return RVN_OK;
  });
}

int rvn_pass1_fetch_overlaps(const rvn_pass1* p, rvn_overlap* overlaps, uint32_t* offsets) {
  return guarded(p ? p->e : nullptr, [&]() -> int {
    if (!p) return fail(RVN_EINVAL, "[raven_hip] NULL pass1");
    RVN_HIP(hipSetDevice(p->e->device));
    if (overlaps && p->ps.kept_total)
      RVN_HIP(hipMemcpy(overlaps, p->ps.kept.ptr, p->ps.kept_total * sizeof(Overlap), hipMemcpyDeviceToHost));
    if (offsets)
      RVN_HIP(hipMemcpy(offsets, p->ps.kept_off.ptr, (static_cast<size_t>(p->ps.n) + 1) * 4, hipMemcpyDeviceToHost));
    return RVN_OK;
  });
}

void rvn_pass1_destroy(rvn_pass1* p) { delete p; }

int rvn_find_overlaps_and_repetitive_regions(rvn_engine* h, const rvn_reads* rr, const uint32_t* pile_begin,
                                             const uint32_t* pile_end, const uint8_t* pile_invalid, double freq,
                                             uint32_t kmer_len, double identity, uint64_t batch_bases, rvn_pass2** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !rr || !out || (rr->r.n && (!pile_begin || !pile_end || !pile_invalid)))
      return fail(RVN_EINVAL, "[raven_hip] rvn_find_overlaps_and_repetitive_regions: NULL argument");
    if (!(0 <= freq && freq <= 1)) return fail(RVN_EINVAL, "[ram::MinimizerEngine::Filter] error: invalid frequency");
    if (kmer_len == 0 || kmer_len > 32) return fail(RVN_EINVAL, "[raven_hip] kmer_len must be in [1, 32]");
    if (batch_bases == 0) return fail(RVN_EINVAL, "[raven_hip] batch_bases must be positive");
    Engine& e = h->e;
    const ReadsDev& r = rr->r;
    for (u32 i = 0; i < r.n; ++i)
      if (r.h_id[i] != i) return fail(RVN_EINVAL, "[raven_hip] FindOverlapsAndRepetetiveRegions requires ids[i] == i");
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    engine_release_scratch_if_tight(e, 1);
    std::unique_ptr<rvn_pass2> p(new rvn_pass2());
    p->e = &e;
    p->engine_life = e.life;
    second_pass(e, r, pile_begin, pile_end, pile_invalid, freq, kmer_len, identity, batch_bases, p->st);
    *out = p.release();
    return RVN_OK;
  });
}

uint64_t rvn_pass2_num_overlaps(const rvn_pass2* p) { return p ? p->st.n_overlaps : 0; }
uint64_t rvn_pass2_kmer_cells(const rvn_pass2* p) { return p ? p->st.kmers_total : 0; }

int rvn_pass2_fetch(const rvn_pass2* p, rvn_overlap* overlaps, uint8_t* contained, uint8_t* kmers, uint64_t* kmers_offsets) {
  if (!p) return fail(RVN_EINVAL, "[raven_hip] NULL pass2");
  if (p->engine_life.expired()) return fail(RVN_EINVAL, "[raven_hip] the engine of this result is gone");
  return guarded(p->e, [&]() -> int {
    RVN_HIP(hipSetDevice(p->e->device));
    const Pass2State& st = p->st;
    if (overlaps && st.n_overlaps)
      RVN_HIP(hipMemcpy(overlaps, st.ovl.ptr, st.n_overlaps * sizeof(Overlap), hipMemcpyDeviceToHost));
    if (contained && st.n) RVN_HIP(hipMemcpy(contained, st.contained.ptr, st.n, hipMemcpyDeviceToHost));
    if (kmers && st.kmers_total) RVN_HIP(hipMemcpy(kmers, st.kmers.ptr, st.kmers_total, hipMemcpyDeviceToHost));
    if (kmers_offsets) std::memcpy(kmers_offsets, st.h_kmers_off.data(), st.h_kmers_off.size() * 8);
    return RVN_OK;
  });
}

void rvn_pass2_destroy(rvn_pass2* p) { delete p; }

int rvn_filter_overlaps_by_identity(rvn_engine* h, const rvn_reads* rr, rvn_overlap* overlaps, uint32_t* offsets,
                                    const uint32_t* pile_begin, const uint32_t* pile_end, const uint8_t* pile_invalid,
                                    double identity) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !rr || !offsets || !pile_begin || !pile_end || !pile_invalid || (offsets[rr->r.n] && !overlaps))
      return fail(RVN_EINVAL, "[raven_hip] rvn_filter_overlaps_by_identity: NULL argument");
    const ReadsDev& r = rr->r;
    for (u32 i = 0; i < r.n; ++i)
      if (r.h_id[i] != i) return fail(RVN_EINVAL, "[raven_hip] the identity filter requires ids[i] == i");
    for (u64 x = 0; x < offsets[r.n]; ++x)
      if (overlaps[x].lhs_id >= r.n || overlaps[x].rhs_id >= r.n)
        return fail(RVN_EINVAL, "[raven_hip] rvn_filter_overlaps_by_identity: overlap of an unknown read");
    RVN_HIP(hipSetDevice(h->e.device));
    UseTimers ut(h->e);
    identity_filter_lists(h->e, r, reinterpret_cast<Overlap*>(overlaps), offsets, pile_begin, pile_end, pile_invalid, identity);
    return RVN_OK;
  });
}

int rvn_overlap_update_and_type(rvn_overlap* overlaps, uint64_t n, const uint32_t* pile_begin, const uint32_t* pile_end,
                                const uint8_t* pile_invalid, uint32_t n_piles, uint8_t* ok, uint32_t* type) {
  if (!overlaps || !pile_begin || !pile_end || !pile_invalid || !ok || !type) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
  for (uint64_t i = 0; i < n; ++i) {
    Overlap& o = reinterpret_cast<Overlap*>(overlaps)[i];
    if (o.lhs_id >= n_piles || o.rhs_id >= n_piles) return fail(RVN_EINVAL, "[raven_hip] overlap names a pile beyond n_piles");
    const PileRegion L{pile_begin[o.lhs_id], pile_end[o.lhs_id], pile_invalid[o.lhs_id] ? 1u : 0u};
    const PileRegion R{pile_begin[o.rhs_id], pile_end[o.rhs_id], pile_invalid[o.rhs_id] ? 1u : 0u};
    ok[i] = overlap_update(o, L, R) ? 1 : 0;
    type[i] = ok[i] ? overlap_type(o, L, R) : 0xFFFFFFFFu;
  }
  return RVN_OK;
}

int rvn_pile_add_layers(rvn_engine* h, uint16_t* data, uint32_t cells, uint32_t id, const rvn_overlap* overlaps,
                        uint64_t n) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || (cells && !data) || (n && !overlaps)) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    if (n == 0 || cells == 0) return RVN_OK;
    if (n >= (1ULL << 31)) return fail(RVN_EINVAL, "[raven_hip] too many overlaps");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    // a one-pile PileState whose "new list" is the caller's overlaps
    ReadsDev r;
    r.n = 1;
    r.h_len = {cells << 4};
    r.h_id = {id};
    u32* d_id = r.id.get<u32>(1);
    RVN_HIP(hipMemcpy(d_id, &id, 4, hipMemcpyHostToDevice));
    PileState ps;
    piles_init(e, r, ps);
    RVN_HIP(hipMemcpy(ps.pile_data.ptr, data, static_cast<size_t>(cells) * 2, hipMemcpyHostToDevice));
    pile_add_layers_single(e, ps, d_id, reinterpret_cast<const Overlap*>(overlaps), static_cast<u32>(n));
    RVN_HIP(hipMemcpy(data, ps.pile_data.ptr, static_cast<size_t>(cells) * 2, hipMemcpyDeviceToHost));
    return RVN_OK;
  });
}

int rvn_pile_add_kmers_batch(rvn_engine* h, const rvn_reads* r, uint32_t first_read, uint32_t n_reads,
                             const uint32_t* positions, const uint64_t* position_offsets, uint8_t* kmers,
                             const uint64_t* kmers_offsets) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !r || (n_reads && (!position_offsets || !kmers || !kmers_offsets)))
      return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    const ReadsDev& rd = r->r;
    if (static_cast<u64>(first_read) + n_reads > rd.n) return fail(RVN_EINVAL, "[raven_hip] bad read range");
    for (uint32_t i = 0; i < n_reads; ++i) {
      const u32 len = rd.h_len[first_read + i];
      if (kmers_offsets[i + 1] - kmers_offsets[i] < (static_cast<u64>(len) >> 4) + 1)
        return fail(RVN_EINVAL, "[raven_hip] rvn_pile_add_kmers_batch: kmers buffer smaller than (len >> 4) + 1");
      for (uint64_t q = position_offsets[i]; q < position_offsets[i + 1]; ++q)
        if (static_cast<u64>(positions[q]) + h->e.k > len)
          return fail(RVN_EINVAL, "[raven_hip] rvn_pile_add_kmers_batch: k-mer position outside its read");
    }
    RVN_HIP(hipSetDevice(h->e.device));
    UseTimers ut(h->e);
    pile_add_kmers_batch(h->e, rd, positions, position_offsets, n_reads, first_read, kmers, kmers_offsets);
    return RVN_OK;
  });
}

int rvn_edit_distance_batch(rvn_engine* h, const rvn_reads* r, const rvn_ed_pair* pairs, uint32_t n_pairs,
                            uint32_t* distances, double* device_ms, uint64_t* cells) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !r || (n_pairs && (!pairs || !distances))) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    const ReadsDev& rd = r->r;
    if (const char* what = ed_pairs_error(rd, pairs, n_pairs))
      return fail(RVN_EINVAL, std::string("[raven_hip] rvn_edit_distance_batch: ") + what);
    RVN_HIP(hipSetDevice(h->e.device));
    UseTimers ut(h->e);
    static_assert(sizeof(rvn_ed_pair) == 32, "pair layout");
    edit_distance_batch(h->e, rd, reinterpret_cast<const u32*>(pairs), n_pairs, distances, device_ms, cells);
    return RVN_OK;
  });
}

int rvn_engine_sketch(rvn_engine* h, const rvn_reads* r, uint32_t first, uint32_t last, int minhash, uint64_t* count) {
  return guarded(h, h && r && first <= last && last <= r->r.n, "[raven_hip] rvn_engine_sketch: bad range", [&](Engine& e) -> int {
    sketch_range(e, r->r, first, last, minhash != 0, e.sketch.query_sketch);
    RVN_HIP(rvn_stream_sync(e.stream));
    if (count) *count = e.sketch.query_sketch.count;
    return RVN_OK;
  });
}

int rvn_engine_sketch_fetch(rvn_engine* h, uint64_t* values, uint64_t* origins, uint32_t* read_offsets) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    Sketch& s = e.sketch.query_sketch;
    RVN_HIP(hipSetDevice(e.device));
    fetch_values(e, s.val, s.count, values);
    if (origins && s.count) RVN_HIP(hipMemcpy(origins, s.org.ptr, s.count * 8, hipMemcpyDeviceToHost));
    if (read_offsets)
      RVN_HIP(hipMemcpy(read_offsets, s.read_off.ptr, (static_cast<size_t>(s.last - s.first) + 1) * 4,
                        hipMemcpyDeviceToHost));
    return RVN_OK;
  });
}

int rvn_engine_index_size(const rvn_engine* h, uint64_t* n_minimizers, uint64_t* n_keys) {
  if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
  if (n_minimizers) *n_minimizers = h->e.sketch.index.m;
  if (n_keys) *n_keys = h->e.sketch.index.u;
  return RVN_OK;
}

int rvn_engine_index_fetch(rvn_engine* h, uint64_t* values, uint64_t* origins) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    Index& ix = e.sketch.index;
    RVN_HIP(hipSetDevice(e.device));
    fetch_values(e, ix.s_val[ix.cur], ix.m, values);
    if (origins && ix.m) {
      RVN_HIP(hipMemcpy(origins, ix.s_org[ix.cur].ptr, ix.m * 8, hipMemcpyDeviceToHost));
      // (both flag bits: after a multi-batch shard build the index also holds query-only entries of earlier batches'
      // reads — they come back as plain id << 32 | pos << 1 | strand like the members)
      for (u64 i = 0; i < ix.m; ++i) origins[i] &= ~(kQueryFlag | kForeignFlag);
    }
    return RVN_OK;
  });
}

}  // extern "C"
