// engine.hip — the engine itself: create / destroy, options, Minimize, the scratch-release policy, stats and timers.
#include <chrono>
#include <memory>

#include "abi.h"
#include "poa.h"

using namespace rvn;

static_assert(sizeof(rvn_overlap) == sizeof(rvn::Overlap), "overlap layout");

namespace {

thread_local std::string g_err;

const char* kStageNames[StageTimes::kNum] = {"sketch", "sort", "index", "filter", "query_sketch", "match",
                                             "seg_sort", "intervals", "chain", "compact", "merge", "pile",
                                             "truncate"};

}  // namespace

namespace rvn {

void set_last_error(const std::string& msg) { g_err = msg; }
const std::string& last_error() { return g_err; }

// Sketch [first,last) and build the index.  With prefetch_query the minhash QUERY sketch of the same
// range (construct.cc:62 always maps with minhash=true) is derived from the same raw sketch before the
// index sort consumes it, so map_batch over that range does not sketch again.
void engine_minimize(Engine& e, const ReadsDev& r, u32 first, u32 last, bool minhash, bool prefetch_query) {
  bool raw_handed_over = false;
  {
    StageTimer t(e, StageTimes::kSketch);
    e.sketch.query_ready = {};
    Index& ix = e.sketch.index;
    ix.has_query_flags = false;
    ix.all_query = false;
    sketch_raw(e, r, first, last, e.sketch.raw_sketch);
    const bool join = prefetch_query && r.ids_are_indices;  // map_batch will self-join instead of probing
    if (join && !minhash) {
      e.sketch.join_query_count = sketch_flag_queries(e, r, e.sketch.raw_sketch);
      ix.has_query_flags = true;
    } else if (prefetch_query && !join) {
      sketch_minhash(e, r, e.sketch.raw_sketch, e.sketch.query_sketch);
      e.sketch.query_ready = {true, first, last, true};
    }
    Sketch& is = e.sketch.index_sketch;
    if (join && minhash) {
      sketch_minhash(e, r, e.sketch.raw_sketch, is);
      ix.all_query = true;
    } else if (!minhash) {
      is.val.swap(e.sketch.raw_sketch.val);
      is.org.swap(e.sketch.raw_sketch.org);
      is.read_off.swap(e.sketch.raw_sketch.read_off);
      is.first = first;
      is.last = last;
      is.count = e.sketch.raw_sketch.count;
      e.sketch.raw_sketch.count = 0;
      raw_handed_over = true;
    } else if (prefetch_query) {
      const Sketch& qs = e.sketch.query_sketch;
      const size_t vb = e.val64 ? 8 : 4;
      is.first = first;
      is.last = last;
      is.count = qs.count;
      is.val.reserve((qs.count + 1) * vb);
      is.org.reserve((qs.count + 1) * 8);
      if (qs.count) {
        RVN_HIP(hipMemcpyAsync(is.val.ptr, qs.val.ptr, qs.count * vb, hipMemcpyDeviceToDevice, e.stream));
        RVN_HIP(hipMemcpyAsync(is.org.ptr, qs.org.ptr, qs.count * 8, hipMemcpyDeviceToDevice, e.stream));
      }
    } else {
      sketch_minhash(e, r, e.sketch.raw_sketch, is);
    }
    t.stop();
  }
  for (u32 i = first; i < last; ++i) e.c_index_bases += r.h_len[i];
  e.c_index_min += e.sketch.index_sketch.count;
  index_build(e, e.sketch.index_sketch, !(e.sketch.index.has_query_flags || e.sketch.index.all_query));
  e.c_index_keys += e.sketch.index.u;
  // index_build adopted the sketch's buffers and left the ones it displaced in index_sketch: they go back to the raw
  // sketch, so that TWO sets circulate (raw sketch <-> index side 0) and the second pass already finds its buffers —
  // left alone, three sets rotate through the three owners and every one of them is grown once (0.5 s at C4).
  if (raw_handed_over) {
    if (e.sketch.raw_sketch.val.cap < e.sketch.index_sketch.val.cap) e.sketch.raw_sketch.val.swap(e.sketch.index_sketch.val);
    if (e.sketch.raw_sketch.org.cap < e.sketch.index_sketch.org.cap) e.sketch.raw_sketch.org.swap(e.sketch.index_sketch.org);
  }
}

void fetch_values(Engine& e, const DevBuf& val, u64 n, u64* values) {
  if (!values || n == 0) return;
  if (e.val64) {
    RVN_HIP(hipMemcpy(values, val.ptr, n * 8, hipMemcpyDeviceToHost));
  } else {
    std::vector<u32> tmp(n);
    RVN_HIP(hipMemcpy(tmp.data(), val.ptr, n * 4, hipMemcpyDeviceToHost));
    for (u64 i = 0; i < n; ++i) values[i] = tmp[i];
  }
}

const char* engine_option_names() {
  return "nw_budget_mb, nw_group_walk, nw_stripe_lanes, ed_wide_lanes, edge_slices_budget_kb, index_direct_min_keys, poa_rows_min_windows, io_threads, io_slab_mb, io_ring, io_zlib, arena_mb, arena_margin_mb, "
         "no_arena, release_always, polish_join, polish_sketch_cache_mb";
}
long long* engine_option(EngineOptions& o, const char* name) {
  const std::string n(name ? name : "");
  if (n == "nw_budget_mb") return &o.nw_budget_mb;
  if (n == "nw_group_walk") return &o.nw_group_walk;
  if (n == "nw_stripe_lanes") return &o.nw_stripe_lanes;
  if (n == "ed_wide_lanes") return &o.ed_wide_lanes;
  if (n == "edge_slices_budget_kb") return &o.edge_slices_budget_kb;
  if (n == "index_direct_min_keys") return &o.index_direct_min_keys;
  if (n == "poa_rows_min_windows") return &o.poa_rows_min_windows;
  if (n == "io_threads") return &o.io_threads;
  if (n == "io_slab_mb") return &o.io_slab_mb;
  if (n == "io_ring") return &o.io_ring;
  if (n == "io_zlib") return &o.io_zlib;
  if (n == "arena_mb") return &o.arena_mb;
  if (n == "arena_margin_mb") return &o.arena_margin_mb;
  if (n == "no_arena") return &o.no_arena;
  if (n == "release_always") return &o.release_always;
  if (n == "polish_join") return &o.polish_join;
  if (n == "polish_sketch_cache_mb") return &o.polish_sketch_cache_mb;
  return nullptr;
}

void engine_release_scratch(Engine& e) {
  if (e.stream) (void)rvn_stream_sync(e.stream);
  e.for_each_group([](auto& group) { group.release(); });
  delete e.pile_pool;
  e.pile_pool = nullptr;
}
void engine_release_scratch_if_tight(Engine& e, int stage_kind) {
  e.stage_kind = stage_kind;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
  const bool trace = knob("RVN_DEBUG_MEM") != nullptr;
  if (devpool::active()) {
    // the arena is on (the workload did not fit once): a stage starts from an empty arena when less than a quarter of it
    // is free, or when this kind of stage has run out of memory before with the other phase's scratch alive
    const size_t afree = devpool::free_total(), asize = devpool::size();
    const bool tight = afree * 4 < asize || ((e.oom_mask >> stage_kind) & 1u) || e.opt.release_always != 0;
    if (trace)
      std::fprintf(stderr, "[raven_hip] stage entry (kind %d): arena %.1f GB free of %.1f GB, driver %.1f GB free%s\n", stage_kind,
                   afree / 1e9, asize / 1e9, free_b / 1e9, tight ? " -> scratch released" : "");
    if (tight) engine_release_scratch(e);
    return;
  }
  // (a quarter, not a third: a C4 step settles at ~220 GB of grow-only stage buffers on a 309 GB device — alignment
  // store, window-consensus chunk, sort scratch — and handing them back costs seconds of re-allocation in the next step)
  const bool tight = free_b * 4 < total_b || e.opt.release_always != 0;  // (the latter: tests of this path)
  if (trace)
    std::fprintf(stderr, "[raven_hip] stage entry (kind %d): %.1f GB free of %.1f GB%s\n", stage_kind, free_b / 1e9, total_b / 1e9,
                 tight ? " -> scratch released, arena started" : "");
  if (!tight) return;
  engine_release_scratch(e);
  // From here on the scratch lives in one arena (common.h: devpool): everything that is free now except a margin for
  // the driver's own needs, the buffers that stay outside (reads, pile handles in use) and other users of the device.
  if (e.opt.no_arena) return;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
  size_t margin = std::max<size_t>(12ULL << 30, total_b / 16);
  if (e.opt.arena_margin_mb > 0) margin = static_cast<size_t>(e.opt.arena_margin_mb) << 20;
  if (e.opt.arena_mb > 0) margin = free_b > (static_cast<size_t>(e.opt.arena_mb) << 20) ? free_b - (static_cast<size_t>(e.opt.arena_mb) << 20) : free_b;
  if (free_b > margin + (1ULL << 30)) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = devpool::start(free_b - margin);
    if (trace)
      std::fprintf(stderr, "[raven_hip] arena of %.1f GB %s (%.0f ms)\n", (free_b - margin) / 1e9, ok ? "started" : "refused",
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
}
}  // namespace rvn

extern "C" {

const char* rvn_last_error(void) { return last_error().c_str(); }

int rvn_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rvn_engine_create(rvn_engine** out, uint32_t k, uint32_t w, uint32_t bandwidth, uint32_t chain, uint32_t matches,
                      uint32_t gap, int device) {
  return guarded([&]() -> int {
    if (!out) return fail(RVN_EINVAL, "[raven_hip] rvn_engine_create: out == NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
      return fail(RVN_ENODEVICE, "[raven_hip] no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= n) return fail(RVN_EINVAL, "[raven_hip] invalid device ordinal");
    if (w == 0 || w > static_cast<uint32_t>(kMaxWindow))
      return fail(RVN_EINVAL, "[raven_hip] window length must be in [1, 256]");
    if (chain == 0) return fail(RVN_EINVAL, "[raven_hip] chain must be >= 1");
    RVN_HIP(hipSetDevice(device));
    chain_allow_big_lds();
    std::unique_ptr<rvn_engine> h(new rvn_engine());
    Engine& e = h->e;
    e.k = std::min(std::max(k, 1u), 31u);  // as ram's constructor
    e.w = w;
    e.bandwidth = bandwidth;
    e.chain = chain;
    e.matches = matches;
    e.gap = gap;
    e.device = device;
    e.val64 = 2 * e.k >= 32;
    RVN_HIP(hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking));
    RVN_HIP(hipEventCreate(&e.ev0));
    RVN_HIP(hipEventCreate(&e.ev1));
    RVN_HIP(hipHostMalloc(reinterpret_cast<void**>(&e.h_pin), 4096, hipHostMallocDefault));
    *out = h.release();
    return RVN_OK;
  });
}

void rvn_engine_destroy(rvn_engine* h) {
  if (!h) return;
  (void)hipSetDevice(h->e.device);
  if (h->e.stream) (void)rvn_stream_sync(h->e.stream);
  if (h->e.ev0) (void)hipEventDestroy(h->e.ev0);
  if (h->e.ev1) (void)hipEventDestroy(h->e.ev1);
  if (h->e.stream) (void)hipStreamDestroy(h->e.stream);
  if (h->e.h_pin) (void)hipHostFree(h->e.h_pin);
  delete h->e.pile_pool;
  h->e.pile_pool = nullptr;
  delete h;
  devpool::stop();
}

void rvn_free(void* p) { std::free(p); }

int rvn_engine_release_scratch(rvn_engine* h) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    RVN_HIP(hipSetDevice(h->e.device));
    engine_release_scratch(h->e);
    devpool::stop();  // the caller asked for the memory itself (the arena goes if nothing of it is in use)
    return RVN_OK;
  });
}

int rvn_engine_set_option(rvn_engine* h, const char* name, int64_t value, int64_t* previous) {
  if (!h) return fail(RVN_EINVAL, "[raven_hip] rvn_engine_set_option: engine == NULL");
  long long* slot = engine_option(h->e.opt, name);
  // -1 = "the built-in default" for every option (the one way to get poa_rows_min_windows' default back: its 0 means
  // "every batch"); any other negative value is refused
  if (!slot || value < -1)
    return fail(RVN_EINVAL, std::string("[raven_hip] rvn_engine_set_option: unknown option or value below -1 (options: ") +
                                engine_option_names() + ")");
  const bool is_rows = slot == &h->e.opt.poa_rows_min_windows;
  if (slot == &h->e.opt.io_ring && value == 1)
    return fail(RVN_EINVAL, "[raven_hip] rvn_engine_set_option: io_ring needs at least 2 slabs in flight (0 or -1: the default)");
  if (slot == &h->e.opt.ed_wide_lanes && value > 1 && (value < 64 || value > 512 || value % 64 != 0))
    return fail(RVN_EINVAL, "[raven_hip] rvn_engine_set_option: ed_wide_lanes is 64 .. 512 in steps of 64, or 1 (no workgroup ring); 0 or -1: the default");
  std::lock_guard<std::recursive_mutex> lk(h->e.mu);
  if (previous) *previous = *slot < 0 ? (is_rows ? static_cast<int>(kPoaRowsMinWindowsDefault) : -1) : *slot;  // (the value the default stands for where it has one)
  *slot = value == -1 ? ((is_rows || slot == &h->e.opt.polish_sketch_cache_mb) ? -1 : 0) : value;
  return RVN_OK;
}

int rvn_engine_counters(const rvn_engine* h, uint64_t out[8]) {
  if (!h || !out) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
  const Engine& e = h->e;
  out[0] = e.c_index_bases;
  out[1] = e.c_index_min;
  out[2] = e.c_index_keys;
  out[3] = e.c_query_bases;
  out[4] = e.c_query_min;
  out[5] = e.c_matches;
  out[6] = e.c_overlaps;
  out[7] = e.c_intervals;
  return RVN_OK;
}

int rvn_engine_num_stages(void) { return StageTimes::kNum; }
const char* rvn_engine_stage_name(int s) { return (s >= 0 && s < StageTimes::kNum) ? kStageNames[s] : ""; }

int rvn_engine_stage_ms(const rvn_engine* h, double* ms, uint64_t* launches, int n) {
  if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
  for (int i = 0; i < n && i < StageTimes::kNum; ++i) {
    if (ms) ms[i] = h->e.times.ms[i];
    if (launches) launches[i] = h->e.times.launches[i];
  }
  return RVN_OK;
}

void rvn_engine_reset_stats(rvn_engine* h) {
  if (!h) return;
  Engine& e = h->e;
  e.times = StageTimes();
  e.ktimers.reset();
  e.c_index_bases = e.c_index_min = e.c_index_keys = e.c_query_bases = e.c_query_min = e.c_matches = e.c_overlaps =
      e.c_intervals = 0;
  e.poa.cells_full = e.poa.cells_band = e.poa.calls = 0;
}

void rvn_poa_work(const rvn_engine* h, uint64_t out[3]) {
  if (!h || !out) return;
  out[0] = h->e.poa.cells_full;
  out[1] = h->e.poa.cells_band;
  out[2] = h->e.poa.calls;
}

void rvn_engine_set_timing(rvn_engine* h, int enabled) {
  if (h) h->e.timing = enabled != 0;
}

void rvn_engine_set_kernel_timing(rvn_engine* h, int enabled) {
  if (h) h->e.ktimers.enabled = enabled != 0;
}
int rvn_engine_num_kernel_sites(void) { return kKNumSites; }
const char* rvn_engine_kernel_site_name(int i) { return (i >= 0 && i < kKNumSites) ? kKernelSiteNames[i] : ""; }
int rvn_engine_kernel_ms(rvn_engine* h, double* ms, uint64_t* launches, int n) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h) return fail(RVN_EINVAL, "[raven_hip] NULL engine");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    RVN_HIP(rvn_stream_sync(e.stream));
    e.ktimers.resolve();
    for (int i = 0; i < n && i < kKNumSites; ++i) {
      if (ms) ms[i] = e.ktimers.ms[i];
      if (launches) launches[i] = e.ktimers.launches[i];
    }
    return RVN_OK;
  });
}

}  // extern "C"
