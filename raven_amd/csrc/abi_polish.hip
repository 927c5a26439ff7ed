// abi_polish.hip — C ABI (include/raven_hip.h): polishing rounds, the window-consensus batch and the alignment paths of
// the polishing front end as a batch call of their own.
#include <algorithm>
#include <cstring>

#include "abi.h"
#ifdef RVN_TEST_HOOKS
#include "../../include/raven_hip_test.h"
#endif
#include "nwpath.h"
#include "poa.h"

using namespace rvn;

struct rvn_paths {
  rvn::Engine* e = nullptr;
  std::weak_ptr<int> engine_life;  // a handle may outlive its engine
  rvn::NwPaths p;
};

extern "C" {

int rvn_polish_round_range(rvn_engine* h, rvn_reads* targets, rvn_reads* reads, const uint8_t* read_quals,
                           const uint64_t* qual_offsets, double q, double err, uint32_t w, int trim, int match,
                           int mismatch, int gap, uint64_t window_first, uint64_t window_last, uint8_t* out_codes,
                           const uint64_t* out_offsets, uint32_t* out_len, double* ratio, uint32_t* n_windows,
                           uint32_t* n_polished, rvn_polish_stats* stats) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !targets || !reads || !out_codes || !out_offsets || !out_len)
      return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    if (w == 0) return fail(RVN_EINVAL, "[racon::Polisher::Create] error: invalid window length!");
    if (read_quals && !qual_offsets) return fail(RVN_EINVAL, "[raven_hip] qualities without offsets");
    RVN_HIP(hipSetDevice(h->e.device));
    UseTimers ut(h->e);
    engine_release_scratch_if_tight(h->e, 2);
    std::vector<std::vector<u8>> polished;
    std::vector<double> rt;
    PolishStats st;
    std::vector<u32> wc, wp;
    // (the consensus goes from the page-locked read-back buffer straight into the caller's — usually never touched — pages, on a
    // few threads: 100 MB at C4; a buffer too small for a target fails the call with RVN_EINVAL)
    std::vector<u64> lens(targets->r.n, 0);
    const PolishDirectOut direct{out_codes, out_offsets, lens.data()};
    polish_round(h->e, targets->r, reads->r, read_quals, qual_offsets, q, err, w, trim != 0, match, mismatch, gap,
                 polished, rt, st, window_first, window_last, &wc, &wp, &direct);
    for (u32 t = 0; t < targets->r.n; ++t) {
      out_len[t] = static_cast<uint32_t>(lens[t]);
      if (ratio) ratio[t] = rt[t];
      if (n_windows) n_windows[t] = wc[t];
      if (n_polished) n_polished[t] = wp[t];
    }
    if (stats) {
      stats->n_overlaps = st.n_overlaps;
      stats->n_reads_used = st.n_reads_used;
      stats->n_layers = st.n_layers;
      stats->n_windows = st.n_windows;
      stats->n_polished_windows = st.n_polished_windows;
      stats->n_failed_windows = st.n_failed_windows;
      stats->poa_ms = st.poa_ms;
      stats->map_ms = st.map_ms;
      stats->host_ms = st.host_ms;
      stats->total_ms = st.total_ms;
      stats->n_dropped_layers = st.n_dropped_layers;
      stats->align_ms = st.align_ms;
      stats->n_aligned = st.n_aligned;
      stats->n_align_retries = st.n_align_retries;
      stats->align_band_cells = st.align_band_cells;
      stats->align_store_bytes = st.align_store_bytes;
    }
    return RVN_OK;
  });
}

int rvn_poa_consensus_batch(rvn_engine* h, const uint8_t* codes, const uint8_t* quals, const uint64_t* layer_offsets,
                            const uint32_t* begins, const uint32_t* ends, const uint32_t* has_qual,
                            const uint32_t* window_offsets, uint32_t n_windows, int match, int mismatch, int gap,
                            int trim, uint8_t* consensus, const uint64_t* consensus_offsets, uint32_t* consensus_len,
                            uint32_t* status, double* device_ms) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || (n_windows && (!codes || !layer_offsets || !begins || !ends || !window_offsets || !consensus ||
                             !consensus_offsets || !consensus_len || !status)))
      return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    for (uint32_t w = 0; w < n_windows; ++w) {
      const uint32_t f = window_offsets[w], l = window_offsets[w + 1];
      if (l <= f) return fail(RVN_EINVAL, "[raven_hip] rvn_poa_consensus_batch: window without a backbone");
      const uint64_t blen = layer_offsets[f + 1] - layer_offsets[f];
      for (uint32_t i = f + 1; i < l; ++i)  // racon Window::AddLayer checks
        if (layer_offsets[i + 1] > layer_offsets[i] && (begins[i] >= ends[i] || ends[i] >= blen))
          return fail(RVN_EINVAL, "[racon::Window::AddLayer] error: layer begin and end positions are invalid!");
    }
    RVN_HIP(hipSetDevice(h->e.device));
    UseTimers ut(h->e);
    poa_consensus_batch(h->e, codes, quals, layer_offsets, begins, ends, has_qual, window_offsets, n_windows, match,
                        mismatch, gap, trim, consensus, consensus_offsets, consensus_len, status, device_ms);
    return RVN_OK;
  });
}

int rvn_polish_map_best(rvn_engine* h, rvn_reads* targets, rvn_reads* reads, uint32_t read_first, uint32_t read_last,
                        double err, rvn_overlap* best, uint32_t* best_target, uint64_t* n_overlaps) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !targets || !reads || !best || !best_target) return fail(RVN_EINVAL, "[raven_hip] rvn_polish_map_best: NULL argument");
    if (read_first > read_last || read_last > reads->r.n) return fail(RVN_EINVAL, "[raven_hip] rvn_polish_map_best: bad read range");
    RVN_HIP(hipSetDevice(h->e.device));
    UseTimers ut(h->e);
    engine_release_scratch_if_tight(h->e, 3);
    std::vector<Overlap> b;
    std::vector<u32> bt;
    u64 n = 0;
    polish_map_best(h->e, targets->r, reads->r, read_first, read_last, err, b, bt, &n);
    if (!b.empty()) std::memcpy(best, b.data(), b.size() * sizeof(Overlap));
    if (!bt.empty()) std::memcpy(best_target, bt.data(), bt.size() * 4);
    if (n_overlaps) *n_overlaps = n;
    return RVN_OK;
  });
}

int rvn_polish_set_best(rvn_engine* h, const rvn_overlap* best, const uint32_t* best_target, uint32_t n_reads) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || (n_reads && (!best || !best_target))) return fail(RVN_EINVAL, "[raven_hip] rvn_polish_set_best: NULL argument");
    Engine& e = h->e;
    e.polish.given_best.resize(n_reads);
    e.polish.given_best_t.assign(best_target, best_target + n_reads);
    if (n_reads) std::memcpy(e.polish.given_best.data(), best, static_cast<size_t>(n_reads) * sizeof(Overlap));
    e.polish.given_valid = true;
    return RVN_OK;
  });
}

int rvn_polish_round(rvn_engine* h, rvn_reads* targets, rvn_reads* reads, const uint8_t* read_quals,
                     const uint64_t* qual_offsets, double q, double err, uint32_t w, int trim, int match, int mismatch,
                     int gap, uint8_t* out_codes, const uint64_t* out_offsets, uint32_t* out_len, double* ratio,
                     rvn_polish_stats* stats) {
  return rvn_polish_round_range(h, targets, reads, read_quals, qual_offsets, q, err, w, trim, match, mismatch, gap, 0,
                                ~0ULL, out_codes, out_offsets, out_len, ratio, nullptr, nullptr, stats);
}

// rvn_align_path_batch; jobs_after (the test hook): the job records as the stage left them, every job's final plan
static int align_path_batch(rvn_engine* h, const rvn_reads* queries, const rvn_reads* targets, const rvn_align_pair* pairs,
                            uint32_t n_pairs, rvn_paths** out, std::vector<NwJob>* jobs_after) {
  return guarded(h, h && queries && targets && out && (pairs || !n_pairs), "[raven_hip] rvn_align_path_batch: NULL argument",
                 [&](Engine& e) -> int {
    static_assert(sizeof(rvn_align_pair) == 32, "pair layout");
    const ReadsDev& Q = queries->r;
    const ReadsDev& T = targets->r;
    std::vector<NwJob> jobs(n_pairs);
    for (uint32_t i = 0; i < n_pairs; ++i) {
      const rvn_align_pair& p = pairs[i];
      if (p.query_read >= Q.n || p.target_read >= T.n)
        return fail(RVN_EINVAL, "[raven_hip] rvn_align_path_batch: read index outside its set");
      const u32 qlen = Q.h_len[p.query_read];
      if (static_cast<u64>(p.query_begin) + p.query_len > qlen ||
          static_cast<u64>(p.target_begin) + p.target_len > T.h_len[p.target_read])
        return fail(RVN_EINVAL, "[raven_hip] rvn_align_path_batch: span outside its read");
      const bool rc = p.strand == 0;
      NwJob& J = jobs[i];
      J = NwJob{};
      J.t_word = T.h_word_off[p.target_read];
      J.r_word = Q.h_word_off[p.query_read];
      J.t_begin = p.target_begin;
      J.n = p.target_len;
      J.q_begin = rc ? qlen - p.query_begin - p.query_len : p.query_begin;  // (in the orientation it is aligned in)
      J.m = p.query_len;
      J.r_len = qlen;
      J.rc = rc ? 1 : 0;
      J.read = p.query_read;
      J.target = p.target_read;
      J.n_windows = 1;
    }
    std::unique_ptr<rvn_paths> res(new rvn_paths());
    res->e = &e;
    res->engine_life = e.life;
    nw_align_paths(e, T, Q, jobs, res->p);
    if (jobs_after) jobs_after->swap(jobs);
    *out = res.release();
    return RVN_OK;
  });
}

int rvn_align_path_batch(rvn_engine* h, const rvn_reads* queries, const rvn_reads* targets, const rvn_align_pair* pairs,
                         uint32_t n_pairs, rvn_paths** out) {
  return align_path_batch(h, queries, targets, pairs, n_pairs, out, nullptr);
}

#ifdef RVN_TEST_HOOKS
int rvn_test_align_path_batch(rvn_engine* h, const rvn_reads* queries, const rvn_reads* targets, const rvn_align_pair* pairs,
                              uint32_t n_pairs, rvn_paths** out, uint32_t* plans, uint64_t* stats) {
  if (!plans || !stats) return fail(RVN_EINVAL, "[raven_hip] rvn_test_align_path_batch: NULL argument");
  std::vector<NwJob> jobs;
  const int r = align_path_batch(h, queries, targets, pairs, n_pairs, out, &jobs);
  if (r != RVN_OK) return r;
  for (size_t i = 0; i < jobs.size(); ++i) {
    const NwJob& J = jobs[i];
    const u32 plan[5] = {J.k, J.kcap, J.R, J.G, J.S};
    std::memcpy(plans + 5 * i, plan, sizeof(plan));
  }
  const NwStats& st = h->e.nw.last;
  const u64 counted[6] = {st.n_aligned, st.n_retries, st.n_unaligned, st.n_batches, st.band_cells, st.store_bytes};
  std::memcpy(stats, counted, sizeof(counted));
  return RVN_OK;
}
#endif

int rvn_paths_info(const rvn_paths* p, uint32_t* n_pairs, uint64_t* n_runs, uint64_t* n_ops, uint32_t* n_not_aligned) {
  if (!p) return fail(RVN_EINVAL, "[raven_hip] rvn_paths_info: NULL handle");
  if (n_pairs) *n_pairs = p->p.n;
  if (n_runs) *n_runs = p->p.n_runs;
  if (n_ops) *n_ops = p->p.n_ops;
  if (n_not_aligned) *n_not_aligned = p->p.n_not_aligned;
  return RVN_OK;
}

int rvn_paths_fetch(const rvn_paths* p, uint32_t* distances, uint64_t* run_offsets, uint32_t* runs) {
  if (!p || p->engine_life.expired()) return fail(RVN_EINVAL, "[raven_hip] rvn_paths_fetch: NULL handle, or its engine is gone");
  return guarded(p->e, [&]() -> int {
    const NwPaths& P = p->p;
    RVN_HIP(hipSetDevice(p->e->device));
    if (distances && P.n) std::memcpy(distances, P.distances.data(), static_cast<size_t>(P.n) * 4);
    if (run_offsets) RVN_HIP(hipMemcpy(run_offsets, P.run_off.ptr, (static_cast<size_t>(P.n) + 1) * 8, hipMemcpyDeviceToHost));
    if (runs && P.n_runs) RVN_HIP(hipMemcpy(runs, P.runs.ptr, static_cast<size_t>(P.n_runs) * 4, hipMemcpyDeviceToHost));
    return RVN_OK;
  });
}

int rvn_paths_fetch_ops(const rvn_paths* p, uint64_t* op_offsets, uint8_t* ops) {
  if (!p || p->engine_life.expired()) return fail(RVN_EINVAL, "[raven_hip] rvn_paths_fetch_ops: NULL handle, or its engine is gone");
  return guarded(p->e, [&]() -> int {
    const NwPaths& P = p->p;
    Engine& e = *p->e;
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    if (op_offsets) RVN_HIP(hipMemcpy(op_offsets, P.op_off.ptr, (static_cast<size_t>(P.n) + 1) * 8, hipMemcpyDeviceToHost));
    if (ops && P.n_ops) {
      DevBuf d_ops;
      u8* d = d_ops.get<u8>(static_cast<size_t>(P.n_ops));
      nw_paths_expand(e, P, d);
      RVN_HIP(hipMemcpyAsync(ops, d, static_cast<size_t>(P.n_ops), hipMemcpyDeviceToHost, e.stream));
      RVN_HIP(rvn_stream_sync(e.stream));
    }
    return RVN_OK;
  });
}

void rvn_paths_destroy(rvn_paths* p) { delete p; }

uint64_t rvn_polish_set_chunk_windows(rvn_engine* h, uint64_t windows) {
  if (!h) return 0;
  const uint64_t prev = h->e.polish_chunk_windows;
  h->e.polish_chunk_windows = windows;
  return prev;
}

int rvn_polish_target_reads(const rvn_engine* h, uint32_t* counts, uint32_t n_targets) {
  if (!h || !counts || n_targets != h->e.polish.target_reads.size())
    return fail(RVN_EINVAL, "[raven_hip] rvn_polish_target_reads: no polishing round with that many targets");
  for (uint32_t i = 0; i < n_targets; ++i) counts[i] = h->e.polish.target_reads[i];
  return RVN_OK;
}

void rvn_poa_phase_cycles(const rvn_engine* h, uint64_t out[6]) {
  for (int i = 0; i < 6; ++i) out[i] = h ? h->e.poa.phase_cycles[i] : 0;
}

int rvn_poa_set_mode(rvn_engine* h, int mode) {
  if (!h) return -1;
  const int prev = h->e.poa.mode;
  if ((mode >= 0 && mode <= 4) || mode == 9) h->e.poa.mode = mode;
  return prev;
}

uint32_t rvn_poa_fallback_windows(const rvn_engine* h) { return h ? h->e.poa.fallback_windows : 0; }
uint32_t rvn_poa_wide_windows(const rvn_engine* h) { return h ? h->e.poa.wide_windows : 0; }
uint32_t rvn_poa_narrow_windows(const rvn_engine* h) { return h ? h->e.poa.narrow_windows : 0; }

int rvn_polish_fetch_layers(rvn_engine* h, uint32_t* out, uint64_t cap, uint64_t* n_out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !n_out) return fail(RVN_EINVAL, "[raven_hip] rvn_polish_fetch_layers: NULL argument");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    const u32 nw = e.polish.last_layers.windows;
    const u64 nl = e.polish.last_layers.layers;
    std::vector<PoaWindow> wins(nw);
    std::vector<PoaLayer> lays(nl);
    std::vector<u8> ok(nl, 1);
    if (nw) RVN_HIP(hipMemcpy(wins.data(), e.polish.wins.ptr, nw * sizeof(PoaWindow), hipMemcpyDeviceToHost));
    if (nl) RVN_HIP(hipMemcpy(lays.data(), e.polish.lays.ptr, nl * sizeof(PoaLayer), hipMemcpyDeviceToHost));
    if (nl && e.polish.last_layers.has_ok) RVN_HIP(hipMemcpy(ok.data(), e.polish.ok.ptr, nl, hipMemcpyDeviceToHost));
    const std::vector<u64>& ro = e.polish.last_layers.read_off;
    u64 n = 0;
    for (u32 i = 0; i < nw; ++i) {
      for (u32 x = 1; x < wins[i].n_layers; ++x) {  // layer 0 = backbone
        const u64 li = static_cast<u64>(wins[i].layer_first) + x;
        if (!ok[li]) continue;
        const PoaLayer& L = lays[li];
        if (out && n < cap) {
          const u64 read = static_cast<u64>(std::upper_bound(ro.begin(), ro.end(), L.code_off) - ro.begin()) - 1;
          uint32_t* o = out + 7 * n;
          o[0] = static_cast<uint32_t>(e.polish.last_layers.w0 + i);
          o[1] = static_cast<uint32_t>(read);
          o[2] = L.q_begin;
          o[3] = L.len;
          o[4] = L.begin;
          o[5] = L.end;
          o[6] = (L.flags & kLayerRc) ? 1u : 0u;
        }
        ++n;
      }
    }
    *n_out = n;
    return RVN_OK;
  });
}

}  // extern "C"
