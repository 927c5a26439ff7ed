// nwpath.hip — kernels and host driver of the alignment-path stage of a polishing round (see nwpath.h): for every
// read's best overlap, the global alignment path against its target span and racon's per-window breakpoints
// (racon Overlap::find_breaking_points, reached from RavenLib/src/polish.cc:51).
//
//   nw_sweep_kernel<R, G>   the forward sweep (nwsweep.h).  A wave is split into 64 / G lane groups; every group owns one
//                           alignment (its ring of L <= G lanes, R blocks per lane), the groups of a wave take a bundle
//                           of 64 / G jobs of similar length and step in lockstep.  Persistent waves, longest jobs
//                           first.  Block state in registers, match masks in LDS; per step one ds_bpermute, one LDS
//                           read, the Myers update.  Leaves the exact distance (if <= k), the hs stream and the
//                           checkpoints.
//   nw_sweep_kernel<8, 64, true>   one stripe of the alignments whose band is wider than one wave's ring (nwpath.h, NwGeo:
//                           the band in horizontal stripes of super-blocks, successive launches, the top input of a stripe
//                           from the hs stream of the one above).
//   nw_trace_kernel         the backward walk (nwtrace.h), one lane per alignment, strip of <= 33 columns in LDS.
//
// Host side: threshold k from the running error-rate estimate of the engine (first call: a generous default), the
// narrowest kernel variant whose ring holds the band of k; alignments whose distance exceeds k are repeated with 2k —
// the result is always the exact optimal path, the estimate only decides how much band is computed.  hs + ck of a launch
// are budgeted (RVN_NW_BUDGET_MB, default: a quarter of the free HBM, at most 64 GB); more jobs than fit go in chunks.
#include <algorithm>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <type_traits>
#include <vector>

#include "engine.h"
#include "nwpath.h"
#include "nwplan.h"
#include "nwsweep.h"
#include "nwtrace.h"
#include "wave.h"

namespace rvn {

namespace {

constexpr int kNwLaneStripCols = 16;        // columns a walker's strip keeps in LDS (nw_trace_kernel<true>)
constexpr int kNwGroupLanes = 16;           // lanes per alignment of the group walk (four alignments per wave)
constexpr u32 kNwGroupWalkMaxJobs = 8192;  // a walk launch of at most this many alignments takes the group walk (two rounds of the
                                           // machine's 4 096 resident groups: beyond that a group's ~3x shorter latency per column loses
                                           // to the lane walk's sixteen times as many alignments in flight — tools/walk_ab.sh)
constexpr u32 kSideSweepMaxWaves = 2048;    // a sweep launch of at most this many waves goes beside the main stream's (enqueue)
// (the kernel variants, the striped class above them and everything the host plans with them: nwplan.h)

template <int G>
__device__ __forceinline__ u32 group_max(u32 v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const u32 o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

template <int R>
constexpr int sweep_waves_per_simd() {
  return R == 1 ? 8 : (R == 2 ? 6 : (R == 4 ? 4 : 2));
}

// STRIPED: stripe `stripe` of every (striped) job of the launch — one super-block per lane, the stripe's steps only, the
// top input from the stripe above (NwTopIn); the last stripe of a job leaves its result
template <int R, int G, bool STRIPED = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sweep_waves_per_simd<R>())))
void nw_sweep_kernel(const NwJob* __restrict__ jobs, const u32* __restrict__ idx, u32 n_idx,
                     const u64* __restrict__ t_words, const u64* __restrict__ r_words, u32* __restrict__ hs,
                     NwPm* __restrict__ ck, u32* __restrict__ result, u32* __restrict__ status, u32* __restrict__ next,
                     int stripe) {
  constexpr int NG = 64 / G;
  static_assert(!STRIPED || G == 64, "a stripe's loop range is per job: one job per wave");
  __shared__ u64 s_peq[4][R * 4 * 64];
  const int lane = lane_id();
  const int group = lane / G, lig = lane % G, gbase = group * G;
  u64* peq = s_peq[threadIdx.x >> 6];
  for (;;) {
    // every lane takes part in the fetch (lane 0 adds the bundle size, the others 0; the compiler folds it into one
    // wave-level atomic): with the usual `if (lane == 0)` around it hipcc 7.2 threaded the G = 64 variant's control flow
    // through the readfirstlane and left lanes 1..63 spinning on bundle 0
    u32 q0 = atomicAdd(next, lane == 0 ? static_cast<u32>(NG) : 0u);
    q0 = static_cast<u32>(__builtin_amdgcn_readfirstlane(static_cast<int>(q0)));
    if (q0 >= n_idx) break;
    const u32 q = q0 + static_cast<u32>(group);
    const bool has = q < n_idx;
    NwSweepLane<R, 64, STRIPED> ln;
    u32 ji = 0, k = 0;
    int L = 0, n_steps = 0;
    u32* hs_j = hs;
    NwPm* ck_j = ck;
    // striped: first step of the loop, the stripe's stores (groups g0 .., checkpoints q0 ..), the top input, the step at
    // which the score the next stripe enters with is taken, whether this is the job's last stripe
    int t0 = 1, g0 = 0, qc0 = 0, gps = 0, qps = 0, t_hand = kNwNever, sc_in = 0, sc_hand = 0, lig_hand = -1;
    bool is_top = false, last = true;
    NwTopIn top;
    if (has) {
      ji = idx[q];
      const NwJob J = jobs[ji];
      NwGeo geo = STRIPED ? nw_geo_job(J) : nw_geo(J.n, J.m, J.k, R);
      n_steps = geo.n_steps;
      if (STRIPED) {
        geo.s0 = stripe * geo.S;
        geo.s1 = geo.s0 + geo.S < geo.n_super ? geo.s0 + geo.S : geo.n_super;
        t0 = geo.st_t0(stripe);
        g0 = (t0 - 1) >> 4;
        qc0 = (t0 - 1) >> 5;
        gps = geo.gps;
        qps = geo.qps;
        n_steps = geo.je(geo.s1 - 1) + geo.s1;  // the retirement of its last super-block
        last = geo.s1 == geo.n_super;
        if (!last && geo.ja(geo.s1) > 1) {
          t_hand = geo.ja(geo.s1) + geo.s1;
          lig_hand = geo.s1 - 1 - geo.s0;
        }
        is_top = lig == 0 && stripe > 0;
        if (is_top) {
          top.init(hs + J.hs, geo, t0);
          sc_in = static_cast<int>(hs[J.hs + geo.hand_at(stripe - 1)]);
        }
      }
      ln.init(J, t_words, r_words, geo, lig, peq, lane);
      L = geo.L;
      k = J.k;
      hs_j = hs + J.hs + (STRIPED ? static_cast<u64>(stripe) * geo.stripe_hs_words() : 0ULL);
      ck_j = ck + J.ckpt + (STRIPED ? static_cast<u64>(stripe) * geo.stripe_ck_entries() : 0ULL);
    } else {
      ln.init_idle(peq, lane);
    }
    int n_steps_w = n_steps;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(n_steps_w, off, 64);
      n_steps_w = o > n_steps_w ? o : n_steps_w;
    }
    n_steps_w = __builtin_amdgcn_readfirstlane((n_steps_w + 15) & ~15);
    const int prev = lig == 0 ? gbase + (L > 0 ? L - 1 : 0) : lane - 1;
    const bool st_ok = has && lig < L;
    int n_g = (n_steps + kNwHsSteps - 1) / kNwHsSteps, n_q = n_steps / kNwCkSteps;
    if (STRIPED) {  // (the stripe's region: gps groups from g0, qps checkpoints from qc0)
      n_g = g0 + gps;
      n_q = qc0 + qps;
    }
    const u64 row = static_cast<u64>(L) * R;
    for (int t = t0; t <= n_steps_w; ++t) {
      int x = __shfl(ln.xf, prev, 64);
      if (STRIPED) {
        if (is_top) x = top.x(t);
        if (t == t_hand) sc_hand = ln.sc;  // (after step t - 1: what the ring's next lane would read at t)
      }
      if (__ballot(ln.has_event(t)) != 0) {
        int sp = __shfl(ln.sc, prev, 64);
        if (STRIPED && is_top) sp = sc_in;
        if (ln.has_event(t)) ln.event(t, x, sp);
      }
      ln.step(t, x);
      if ((t & 15) == 0) {
        const int gi = (t >> 4) - 1;
        if (st_ok && gi < n_g) {
          u32* p = hs_j + static_cast<u64>(gi - g0) * row + static_cast<u64>(lig) * R;
#pragma unroll
          for (int r = 0; r < R; ++r) p[r] = ln.acc[r];
        }
        if ((t & 31) == 0) {
          const int qi = (t >> 5) - 1;
          if (st_ok && qi < n_q) {
            NwPm* p = ck_j + static_cast<u64>(qi - qc0) * row + static_cast<u64>(lig) * R;
#pragma unroll
            for (int r = 0; r < R; ++r) p[r] = NwPm{ln.Pv[r], ln.Mv[r]};
          }
        }
        ln.next_group(t);
        if (STRIPED && is_top) top.next_group(t);
      }
    }
    if (STRIPED && has && lig == lig_hand) hs_j[row * static_cast<u64>(gps)] = static_cast<u32>(sc_hand);  // (NwGeo::hand_at)
    const u32 res1 = group_max<G>(ln.result);  // exactly one lane of the group holds D(n, m) + 1
    if (has && lig == 0 && last) {
      const u32 res = res1 - 1u;
      result[ji] = res;
      status[ji] = (res1 != 0 && res <= k) ? 0u : 2u;  // 2: beyond the threshold, the host repeats the job with 2k
    }
  }
}

// STRIP_LDS: the walker's strip in LDS (33 KB per wave: four waves per CU) or in a per-wave scratch in HBM / L2
// ([column][lane], coalesced; occupancy limited by registers only)
// Out: what the walk leaves — NwWindowRec, the window records of polishing (recs[J.bp_off ..]), or u32, the path form:
// the walker's runs in the job's slot (out[J.bp_off ..], nw_slot_words(J.k) words, filled from the back: NwRunSink)
template <bool STRIP_LDS, int SC, class Out = NwWindowRec>
__global__ __launch_bounds__(64) void nw_trace_kernel(const NwJob* __restrict__ jobs, const u32* __restrict__ idx, u32 n_idx,
                                                      const u64* __restrict__ t_words, const u64* __restrict__ r_words,
                                                      const u32* __restrict__ hs, const NwPm* __restrict__ ck,
                                                      const u32* __restrict__ result, u32* __restrict__ status, u32 w,
                                                      Out* __restrict__ recs, u64* __restrict__ scratch) {
  // (SC = 16: a strip keeps sixteen columns, 17.4 KB of LDS per wave, nine waves per CU instead of four — nwtrace.h; for
  // launches of more waves than the machine holds with whole strips.  A walker pays ~15 % for the second visit of a
  // checkpoint interval, so launches that fit keep whole strips.)
  __shared__ u64 s_pv[STRIP_LDS ? (SC + 1) * 64 : 1];
  __shared__ u64 s_mv[STRIP_LDS ? (SC + 1) * 64 : 1];
  // one lane per alignment, a long dependent chain per column: these waves run beside the next chunk's sweep (which keeps
  // the VALUs full) and must not queue behind it for every instruction
  __builtin_amdgcn_s_setprio(3);
  const u32 q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_idx) return;
  const u32 ji = idx[q];
  if (status[ji] != 0) return;
  const NwJob J = jobs[ji];
  const NwGeo geo = nw_geo_job(J);
  u64* g_pv = scratch + static_cast<u64>(blockIdx.x) * (2 * kNwStripCols * 64);
  const NwStripMem<64> mem{STRIP_LDS ? s_pv : g_pv, STRIP_LDS ? s_mv : g_pv + kNwStripCols * 64, static_cast<int>(threadIdx.x)};
  if constexpr (std::is_same<Out, u32>::value) {
    NwRunSink sink;
    sink.init(recs + J.bp_off, nw_slot_words(J.k));
    status[ji] = static_cast<u32>(nw_trace_job<64, SC, NwRunSink>(J, geo, t_words, r_words, hs + J.hs, ck + J.ckpt, mem, result[ji], w,
                                                                  nullptr, sink));
  } else {
    status[ji] = static_cast<u32>(nw_trace_job<64, SC>(J, geo, t_words, r_words, hs + J.hs, ck + J.ckpt, mem, result[ji], w, recs));
  }
}

// The group walk (nwtrace.h: NwGroupWalk): GL lanes per alignment, 64 / GL alignments per wave; strips in the same LDS
// array as nw_trace_kernel's (column = lane), the heads beside it: 36.9 KB per wave, four waves per CU.
template <int GL, class Out = NwWindowRec>
__global__ __launch_bounds__(64) void nw_trace_group_kernel(const NwJob* __restrict__ jobs, const u32* __restrict__ idx, u32 n_idx,
                                                            const u64* __restrict__ t_words, const u64* __restrict__ r_words,
                                                            const u32* __restrict__ hs, const NwPm* __restrict__ ck,
                                                            const u32* __restrict__ result, u32* __restrict__ status, u32 w,
                                                            Out* __restrict__ recs) {
  constexpr int NG = 64 / GL;
  __shared__ u64 s_pv[kNwStripCols * 64];
  __shared__ u64 s_mv[kNwStripCols * 64];
  __shared__ NwStripHead s_heads[64];
  __builtin_amdgcn_s_setprio(3);
  const int lane = static_cast<int>(threadIdx.x), grp = lane / GL, t = lane % GL;
  const u32 q = blockIdx.x * NG + static_cast<u32>(grp);
  if (q >= n_idx) return;
  const u32 ji = idx[q];
  if (status[ji] != 0) return;
  const NwJob J = jobs[ji];
  const NwGeo geo = nw_geo_job(J);
  constexpr bool kPath = std::is_same<Out, u32>::value;
  NwGroupWalk<64, GL, typename std::conditional<kPath, NwRunSink, NwNoSink>::type> G;
  if constexpr (kPath) {
    NwRunSink sink;
    sink.init(recs + J.bp_off, nw_slot_words(J.k));
    G.init(J, t_words, r_words, NwStripMem<64>{s_pv, s_mv, grp * GL}, s_heads + grp * GL, result[ji], w, nullptr, sink);
  } else {
    G.init(J, t_words, r_words, NwStripMem<64>{s_pv, s_mv, grp * GL}, s_heads + grp * GL, result[ji], w, recs);
  }
  int bad = 0;
  while (!G.done()) {
    G.fill(J, geo, hs + J.hs, ck + J.ckpt, t);
    __threadfence_block();  // (one wave: the strips and heads of the group's lanes, visible to all of them)
    __builtin_amdgcn_wave_barrier();
    bad = G.walk_batch(geo, t == 0);
    __threadfence_block();  // (the next batch overwrites them)
    __builtin_amdgcn_wave_barrier();
    if (bad) break;
  }
  const int rcode = bad ? 1 : G.wk.finish(t == 0);
  if (t == 0) status[ji] = static_cast<u32>(rcode);
}

template <int R, int G, bool STRIPED = false>
void launch_sweep(Engine& e, hipStream_t s, const NwJob* d_jobs, const u32* d_idx, u32 n_idx, const ReadsDev& T, const ReadsDev& Rd,
                  u32* d_hs, NwPm* d_ck, u32* d_result, u32* d_status, u32* d_next, int stripe = 0) {
  if (n_idx == 0) return;
  constexpr u32 NG = 64 / G;
  const u32 bundles = (n_idx + NG - 1) / NG;
  // persistent waves: not every slot of the machine — the walks of the previous chunk run beside this sweep on the other
  // stream and need wave slots (and LDS) of their own; the sweep is VALU-bound long before its last two waves per SIMD
  const u32 per_simd = static_cast<u32>(sweep_waves_per_simd<R>());
  const u32 waves = std::min<u32>(bundles, 256u * 4u * (per_simd > 4 ? per_simd - 2 : per_simd));
  RVN_HIP(hipMemsetAsync(d_next, 0, 4, s));
  RVN_KLAUNCH_ON(kKNwForward, s, (nw_sweep_kernel<R, G, STRIPED><<<(waves + 3) / 4, 256, 0, s>>>(
                               d_jobs, d_idx, n_idx, T.packed.as<u64>(), Rd.packed.as<u64>(), d_hs, d_ck, d_result,
                               d_status, d_next, stripe)));
}


}  // namespace

// The stage's streams and events, on first use.  HIP multiplexes its streams over a handful of hardware queues (four by
// default): two walk streams that land on the same queue run one after the other, and the ~100-ms walk of the longest
// alignments held the walk queued behind it — and with it the sweep waiting for that walk's buffer set
// (profiles/r05_nw_timeline.csv: a walk starting the moment the long one ended).  Streams of another PRIORITY get hardware
// queues of their own: the long pole's stream (set 3) is created at the highest priority, which also suits a kernel of 38
// latency-bound waves.  ([4], the upload stream, must not share a hardware queue with the engine's stream either: its
// copies run while a pass queued before is sweeping there.)  All or nothing: a creation that throws half-way must not
// leave streams[0] set with the others null — the next call would skip this and launch walks on the null stream.
void NwState::open() {
  try {
    int prio_least = 0, prio_greatest = 0;
    RVN_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    for (int b = 0; b < 8; ++b) {
      hipStream_t& st2 = b < 5 ? streams[b] : side[b - 5];
      if (b >= 3 && prio_greatest != prio_least) RVN_HIP(hipStreamCreateWithPriority(&st2, hipStreamNonBlocking, prio_greatest));
      else RVN_HIP(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
    }
    for (hipEvent_t& x : ev) RVN_HIP(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    for (hipEvent_t& x : side_ev) RVN_HIP(hipEventCreateWithFlags(&x, hipEventDisableTiming));
  } catch (...) {
    close();
    throw;
  }
}
void NwState::close() {
  auto drop = [](auto& all, auto destroy) {
    for (auto& x : all) {
      if (x) (void)destroy(x);
      x = nullptr;
    }
  };
  drop(ev, hipEventDestroy);
  drop(streams, hipStreamDestroy);
  drop(side_ev, hipEventDestroy);
  drop(side, hipStreamDestroy);
}

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); }

// an error in the middle of a pass (a walk that left its band, an allocation that failed) must not leave walks running
// on the side streams against buffers the next call hands out again
struct WalkGuard {
  Engine& e;
  ~WalkGuard() {
    if (!std::uncaught_exceptions()) return;
    for (hipStream_t st2 : e.nw.streams)
      if (st2) (void)hipStreamSynchronize(st2);
    for (hipStream_t st2 : e.nw.side)
      if (st2) (void)hipStreamSynchronize(st2);
    (void)hipStreamSynchronize(e.stream);
  }
};

// hs + ck of the stage's buffer sets: a quarter of the free HBM (at most 64 GB), or engine option nw_budget_mb
u64 nw_budget(Engine& e) {
  size_t free_b = 0, total_b = 0;
  RVN_HIP(hipMemGetInfo(&free_b, &total_b));
  u64 held = 0;
  for (const NwState::Set& set : e.nw.sets) held += set.hs.cap + set.ck.cap;
  u64 budget = std::min<u64>((static_cast<u64>(free_b) + devpool::free_total()) / 4 + held, 64ULL << 30);  // parked blocks count as free
  if (e.opt.nw_budget_mb > 0) budget = static_cast<u64>(e.opt.nw_budget_mb) << 20;
  return std::max<u64>(budget, 64ULL << 20);
}

// One call of nw_breakpoints: what its passes share, and the stream and event protocol that turns a plan (nwplan.h) into
// launches.  Schedule: the jobs of a pass go in chunks whose hs + ck fit half the budget, longest jobs first.  The sweeps
// run on the engine's stream, the walk of chunk i on a second stream beside the sweeps of chunk i + 1 (two buffer sets): a
// walk is one lane per alignment and latency-bound (~1 us per column), a sweep fills the VALUs — together they cost the
// time of the sweeps plus the walk of the last, shortest jobs.
//
// path (the path form, nw_align_paths below): the walks leave their runs instead of window records (d_recs = nullptr).
// Every pass of walks gets a block of slots of its own, a job's slot there at its bp_off (nw_slot_words of its threshold:
// known when it is queued); path->slot_end[job] = the device address of the word behind the runs of the job's last walk.
// Planning, thresholds, retries, chunks, stripes and the choice of the walk are the same code.
struct NwRun {
  Engine& e;
  const ReadsDev& T;
  const ReadsDev& Rd;
  std::vector<NwJob>& jobs;
  const u32 w;
  NwWindowRec* const d_recs;
  NwPathSlots* const path;
  NwStats& st;
  std::vector<u32>* const distances;
  const hipStream_t s;
  const u32 nj;
  const u64 budget;
  // engine option nw_stripe_lanes: the widest ring of one sweep (variants with wider rings are skipped) = the stripe size
  const u32 stripe_lanes;
  const bool trace_lds;
  // which walk a launch takes (engine option nw_group_walk): 1 the lane per alignment with whole strips, 2 the group of lanes
  // per alignment, 3 the lane per alignment with strips of sixteen kept columns, otherwise by the number of alignments in the launch
  const int group_walk;
  const bool one_stream, dbg_sync;
  const NwDevArrays dev;  // (dev.side_next: behind the compact passes' arrays)
  bool side_pending[3] = {false, false, false};  // sweeps on a side stream that the main stream has not waited for yet
  bool set_used[4] = {false, false, false, false};  // a walk queued since the last collect() holds the buffer set
  struct Queued {  // what collect() reads back
    std::vector<u32> order;
    NwPassDev dev;
    bool sweep_only;
    std::vector<u32> res, status;  // (compact passes)
  };
  std::vector<Queued> queued;
  std::vector<u8> early;  // job was handed to retry_early(): its state in the pass that found it stays "above the threshold"
  std::vector<u32> h_result, h_status;
  std::vector<double> rates;
  std::vector<NwObs> obs;  // (length, distance) of the jobs of sweep-only passes: the pilot
  double h_plan = 0, h_order = 0, h_up = 0, h_res = 0;  // host milliseconds between the launches (RVN_NW_DEBUG)

  // the budget is taken before the call's arrays: it follows the free memory
  NwRun(Engine& e_, const ReadsDev& T_, const ReadsDev& Rd_, std::vector<NwJob>& jobs_, u32 w_, NwWindowRec* d_recs_, NwPathSlots* path_,
        NwStats& st_, std::vector<u32>* distances_)
      : e(e_), T(T_), Rd(Rd_), jobs(jobs_), w(w_), d_recs(d_recs_), path(path_), st(st_), distances(distances_), s(e_.stream),
        nj(static_cast<u32>(jobs_.size())), budget(nw_budget(e_)),
        stripe_lanes(e_.opt.nw_stripe_lanes > 0 && e_.opt.nw_stripe_lanes < 64 ? static_cast<u32>(e_.opt.nw_stripe_lanes) : 64u),
        trace_lds(!(knob("RVN_NW_TRACE_MEM") && std::atoi(knob("RVN_NW_TRACE_MEM")) == 1)),
        group_walk(static_cast<int>(e_.opt.nw_group_walk)), one_stream(knob("RVN_NW_ONE_STREAM") != nullptr),
        dbg_sync(knob("RVN_NW_DEBUG") && std::atoi(knob("RVN_NW_DEBUG")) >= 2), dev(arrays(e_, nj)), h_result(nj), h_status(nj) {
    rates.reserve(nj);  // (growing it inside collect() cost milliseconds of page faults with the GPU idle)
  }
  static NwDevArrays arrays(Engine& e, u32 nj) {
    const NwDevLayout at = nw_dev_layout(nj);
    NwJob* d_jobs = e.nw.jobs.get<NwJob>(at.n_jobs);
    return nw_dev_arrays(at, d_jobs, e.nw.res.get<u32>(at.n_words));
  }

  bool plan(NwJob& J, u64 k) const { return nw_plan(J, k, stripe_lanes, budget); }

  void join_side() {
    for (int x = 0; x < 3; ++x) {
      if (side_pending[x]) RVN_HIP(hipStreamWaitEvent(s, e.nw.side_ev[x], 0));
      side_pending[x] = false;
    }
  }

  // a chunk's buffers and arrays, as its launches see them
  struct ChunkDev {
    const NwPassDev& dev;
    int b;  // buffer set
    u32* hs;
    NwPm* ck;
    u64* d_strip;
    u32* d_slots;
  };

  template <class Out, class... Tail>
  void launch_walk_kernel(void (*kernel)(const NwJob*, const u32*, u32, const u64*, const u64*, const u32*, const NwPm*, const u32*, u32*, u32,
                                         Out*, Tail...),
                          u32 per_block, const ChunkDev& c, Out* d_out, hipStream_t wst, const u32* idx_w, u32 n_w, Tail... tail) {
    RVN_KLAUNCH_ON(kKNwTraceback, wst, (kernel<<<(n_w + per_block - 1) / per_block, 64, 0, wst>>>(
                                           c.dev.jobs, idx_w, n_w, T.packed.as<u64>(), Rd.packed.as<u64>(), c.hs, c.ck, c.dev.res,
                                           c.dev.status, w, d_out, tail...)));
  }
  // Out — NwWindowRec: polishing; u32: the path form's slots
  template <class Out>
  void launch_walk_to(Out* d_out, const ChunkDev& c, hipStream_t wst, const u32* idx_w, u32 n_w) {
    if (group_walk == 2 || (group_walk != 1 && n_w <= kNwGroupWalkMaxJobs)) {
      // few alignments: a group of lanes each (nwtrace.h) — the walk of a few thousand alignments costs its longest one's
      // latency, and a group walks a column in a fraction of a lane's time
      launch_walk_kernel<Out>(nw_trace_group_kernel<kNwGroupLanes, Out>, 64 / kNwGroupLanes, c, d_out, wst, idx_w, n_w);
    } else if (trace_lds && (group_walk == 3 || (group_walk != 1 && n_w > 64u * 4u * 256u))) {
      // more waves than four per CU hold: strips of sixteen kept columns, nine waves per CU (C4: the walk of the last
      // chunk's 140 000 shortest alignments, alone on the GPU, 18 -> 13 ms; align_ms 185 -> 174)
      launch_walk_kernel<Out, u64*>(nw_trace_kernel<true, kNwLaneStripCols, Out>, 64, c, d_out, wst, idx_w, n_w, nullptr);
    } else if (trace_lds) {
      launch_walk_kernel<Out, u64*>(nw_trace_kernel<true, kNwCkSteps, Out>, 64, c, d_out, wst, idx_w, n_w, nullptr);
    } else {
      launch_walk_kernel<Out, u64*>(nw_trace_kernel<false, kNwCkSteps, Out>, 64, c, d_out, wst, idx_w, n_w,
                                    c.d_strip + static_cast<size_t>(c.b) * ((e.nw.strip.cap / 32) & ~size_t(63)));
    }
  }
  void launch_walk(const ChunkDev& c, hipStream_t wst, const u32* idx_w, u32 n_w) {
    if (path) launch_walk_to(c.d_slots, c, wst, idx_w, n_w);
    else launch_walk_to(d_recs, c, wst, idx_w, n_w);
  }

  // the sweep of the chunk's jobs of variant X, beside the main stream where side[X] says so
  template <u32 X>
  void launch_variant(const ChunkDev& c, const NwChunk& C, const u32* idx_c, const bool* side) {
    constexpr int R = static_cast<int>(kNwVariants[X].R), G = static_cast<int>(kNwVariants[X].G);
    const u32 n = nw_count_of(C, X);
    launch_sweep<R, G>(e, side[X] ? e.nw.side[X % 3] : s, c.dev.jobs, idx_c + C.coff[X], n, T, Rd, c.hs, c.ck, c.dev.res, c.dev.status,
                       side[X] ? dev.side_next + X : dev.next);
    if (dbg_sync && n) {
      RVN_HIP(hipStreamSynchronize(s));
      std::fprintf(stderr, "[raven_hip] nw: sweep R=%d G=%d done, %u jobs\n", R, G, n);
    }
  }
  template <u32 X = kLevels - 1>  // every variant of the table, widest first
  void launch_variants(const ChunkDev& c, const NwChunk& C, const u32* idx_c, const bool* side) {
    launch_variant<X>(c, C, idx_c, side);
    if constexpr (X > 0) launch_variants<X - 1>(c, C, idx_c, side);
  }

  // Queues the sweeps and walks of `todo` (already planned) and returns; collect() waits for everything queued and reads
  // the results.  layout: nwplan.h (kHeadOnly hands what does not fit back in `left`).  up: the stream of the uploads (the
  // host waits for them: not the engine's stream when a pass queued before is sweeping on it).
  void enqueue(const std::vector<u32>& todo, bool sweep_only, NwLayout layout, const NwPassDev& pd, hipStream_t up, std::vector<u32>* left) {
    if (todo.empty()) return;
    auto t_h = clk::now();
    std::vector<u32> order = nw_order(jobs, todo);
    const NwChunks cut = nw_chunks(order, jobs, budget, layout, path && !sweep_only, left);
    const std::vector<NwChunk>& chunks = cut.chunks;
    st.band_cells += cut.band_cells;
    st.store_bytes = std::max<u64>(st.store_bytes, cut.store_bytes);
    // every get() of the pass before any pointer into the blocks is taken: a get may move the block
    for (int b = 0; b < 4; ++b) {
      // sized for the chunks the set serves (a lone job beyond its share enlarges one set, not all)
      const NwSetNeed need = nw_set_need(chunks, layout, b);
      if (!need.used) continue;
      (void)e.nw.sets[b].hs.get<u32>(need.hs_w + 4 * 64 * 8 + 16);  // + slack: the walk reads up to two words past a job's last one
      (void)e.nw.sets[b].ck.get<NwPm>(need.ck_e + 16);
    }
    u64* d_strip = nullptr;
    if (!trace_lds) {
      size_t mc = 0;
      for (const NwChunk& C : chunks) mc = std::max(mc, C.c1 - C.c0);
      d_strip = e.nw.strip.get<u64>(static_cast<size_t>((mc + 63) / 64) * 2 * kNwStripCols * 64 * 4 + 64);
    }
    u32* d_slots = nullptr;
    if (path && !sweep_only) {
      path->blocks.emplace_back(new DevBuf());
      d_slots = path->blocks.back()->get<u32>(cut.slot_w + 16);
      for (u32 i : order) path->slot_end[i] = reinterpret_cast<u64>(d_slots + jobs[i].bp_off + nw_slot_words(jobs[i].k) - 1);
    }
    h_order += since(t_h);
    t_h = clk::now();
    if (pd.compact) {  // records in the order of the pass, addressed by position
      std::vector<NwJob> hj(order.size());
      std::vector<u32> iota(order.size());
      for (size_t x = 0; x < order.size(); ++x) {
        hj[x] = jobs[order[x]];
        iota[x] = static_cast<u32>(x);
      }
      RVN_HIP(hipMemcpyAsync(pd.jobs, hj.data(), hj.size() * sizeof(NwJob), hipMemcpyHostToDevice, up));
      RVN_HIP(hipMemcpyAsync(pd.idx, iota.data(), iota.size() * 4, hipMemcpyHostToDevice, up));
      RVN_HIP(rvn_stream_sync(up));  // (locals)
    } else {
      RVN_HIP(hipMemcpyAsync(pd.jobs, jobs.data(), static_cast<size_t>(nj) * sizeof(NwJob), hipMemcpyHostToDevice, up));
      RVN_HIP(hipMemcpyAsync(pd.idx, order.data(), order.size() * 4, hipMemcpyHostToDevice, up));
      RVN_HIP(rvn_stream_sync(up));  // `jobs` / `order` are pageable: the copies must be done before the host goes on
    }
    h_up += since(t_h);
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
      const NwChunk& C = chunks[ci];
      const int b = nw_set_of(ci, layout);
      const ChunkDev c{pd, b, e.nw.sets[b].hs.as<u32>(), e.nw.sets[b].ck.as<NwPm>(), d_strip, d_slots};
      const u32* idx_c = pd.idx + C.c0;
      const u32 cn = static_cast<u32>(C.c1 - C.c0);
      // the walk that used this buffer set before (three chunks back in the rotation) is done with it
      if (set_used[b]) RVN_HIP(hipStreamWaitEvent(s, e.nw.ev[b], 0));
      // one walk stream per buffer set: the walk of the longest alignments (chunk 0: few waves, tens of milliseconds of
      // latency) must not hold back the walks of the chunks behind it
      hipStream_t ts = one_stream ? s : e.nw.streams[b];
      // A variant's launch of few waves — the pilot's five, the several-blocks-per-lane variants of a round's longest
      // alignments (a few hundred jobs whose sweep is tens of thousands of dependent steps: 14-18 ms on 60-300 of the
      // machine's 6 000 wave slots) — runs BESIDE the others on a side stream instead of in front of them; the walk (and
      // whoever reads the states) waits for all of them, the main stream goes on with the next chunk.
      bool side[kLevels] = {};
      bool side_used[3] = {false, false, false};
      {
        u32 n_levels = 0;
        for (u32 x = 0; x < kLevels; ++x) n_levels += nw_count_of(C, x) ? 1u : 0u;
        if (n_levels >= 2 && !one_stream && !dbg_sync)
          for (u32 x = 0; x < kLevels; ++x) {
            const u32 per_wave = 64 / kNwVariants[x].G;
            const u32 bundles = (nw_count_of(C, x) + per_wave - 1) / per_wave;
            side[x] = nw_count_of(C, x) && bundles <= kSideSweepMaxWaves;
            if (side[x]) side_used[x % 3] = true;
          }
        if (side_used[0] || side_used[1] || side_used[2]) {
          RVN_HIP(hipEventRecord(e.nw.side_ev[3], s));
          for (int y = 0; y < 3; ++y)
            if (side_used[y]) RVN_HIP(hipStreamWaitEvent(e.nw.side[y], e.nw.side_ev[3], 0));
        }
      }
      if (const u32 n_str = nw_count_of(C, kStriped)) {
        // the striped jobs (the widest class: first in the chunk), stripe after stripe on the engine's stream — launch st
        // takes the jobs that have a stripe st, a prefix of the class (ordered by number of stripes)
        const u32* idx_s = idx_c + C.coff[kStriped];
        std::vector<u32> n_stripes(n_str);
        for (u32 x = 0; x < n_str; ++x) n_stripes[x] = static_cast<u32>(nw_geo_job(jobs[order[C.c0 + C.coff[kStriped] + x]]).n_stripes);
        for (u32 stp = 0;; ++stp) {
          u32 n_st = 0;
          while (n_st < n_str && n_stripes[n_st] > stp) ++n_st;
          if (n_st == 0) break;
          launch_sweep<static_cast<int>(kNwStripedVariant.R), static_cast<int>(kNwStripedVariant.G), true>(
              e, s, pd.jobs, idx_s, n_st, T, Rd, c.hs, c.ck, pd.res, pd.status, dev.next, static_cast<int>(stp));
          if (dbg_sync) {
            RVN_HIP(hipStreamSynchronize(s));
            std::fprintf(stderr, "[raven_hip] nw: stripe %u done, %u jobs\n", stp, n_st);
          }
        }
      }
      launch_variants(c, C, idx_c, side);
      for (int y = 0; y < 3; ++y)
        if (side_used[y]) {
          RVN_HIP(hipEventRecord(e.nw.side_ev[y], e.nw.side[y]));
          side_pending[y] = true;
        }
      ++st.n_batches;
      if (sweep_only) continue;
      if (!one_stream) {
        RVN_HIP(hipEventRecord(e.nw.ev[4], s));
        RVN_HIP(hipStreamWaitEvent(ts, e.nw.ev[4], 0));
        for (int y = 0; y < 3; ++y)
          if (side_used[y]) RVN_HIP(hipStreamWaitEvent(ts, e.nw.side_ev[y], 0));
      }
      launch_walk(c, ts, idx_c, cn);
      if (!one_stream) {
        RVN_HIP(hipEventRecord(e.nw.ev[b], ts));
        set_used[b] = true;
      }
      if (dbg_sync) {
        RVN_HIP(hipStreamSynchronize(ts));
        std::fprintf(stderr, "[raven_hip] nw: trace done, %u jobs\n", cn);
      }
    }
    queued.push_back(Queued{std::move(order), pd, sweep_only, {}, {}});
  }

  // Waits for everything queued, reads the results; the jobs beyond their thresholds come back in `again` (planned with
  // twice the band and the variant that holds it).
  void collect(std::vector<u32>& again) {
    again.clear();
    join_side();
    for (int b = 0; b < 4; ++b) {  // (an event stands for the LAST walk recorded on its set)
      if (set_used[b]) RVN_HIP(hipStreamWaitEvent(s, e.nw.ev[b], 0));
      set_used[b] = false;
    }
    for (Queued& q : queued) {
      if (q.dev.compact) {
        q.res.resize(q.order.size());
        q.status.resize(q.order.size());
        RVN_HIP(hipMemcpyAsync(q.res.data(), q.dev.res, q.order.size() * 4, hipMemcpyDeviceToHost, s));
        RVN_HIP(hipMemcpyAsync(q.status.data(), q.dev.status, q.order.size() * 4, hipMemcpyDeviceToHost, s));
      }
    }
    RVN_HIP(hipMemcpyAsync(h_result.data(), dev.all.res, static_cast<size_t>(nj) * 4, hipMemcpyDeviceToHost, s));
    RVN_HIP(hipMemcpyAsync(h_status.data(), dev.all.status, static_cast<size_t>(nj) * 4, hipMemcpyDeviceToHost, s));
    RVN_HIP(rvn_stream_sync(s));
    auto t_h = clk::now();
    for (const Queued& q : queued)
      if (q.dev.compact)
        for (size_t x = 0; x < q.order.size(); ++x) {
          h_result[q.order[x]] = q.res[x];
          h_status[q.order[x]] = q.status[x];
        }
    for (size_t qi = 0; qi < queued.size(); ++qi) {
      const Queued& q = queued[qi];
      const bool is_early_retry = q.dev.jobs == dev.retry.jobs;
      // the aligned jobs of a pass (all but a handful) are only counted: on a few threads — the pass order is by length,
      // i.e. random in the 28 MB of job records, and one thread's cache misses were ~10 ms with the GPU idle
      std::vector<u32> rest_of;  // everything that is not a plain "aligned"
      if (q.sweep_only) {
        rest_of = q.order;
      } else {
        std::mutex mu_;
        parallel_for(q.order.size(), 16384, [this, &q, &mu_, &rest_of, is_early_retry](size_t x0, size_t x1) {
          u64 n_al = 0, sum_d = 0;
          std::vector<double> rr;
          std::vector<u32> other;
          rr.reserve(x1 - x0);
          for (size_t x = x0; x < x1; ++x) {
            const u32 i = q.order[x];
            if (!is_early_retry && !early.empty() && early[i]) continue;  // its result is the early retry pass's
            if (h_status[i] != 0) {
              other.push_back(i);
              continue;
            }
            const NwJob& J = jobs[i];
            ++n_al;
            sum_d += h_result[i];
            if (distances) (*distances)[i] = h_result[i];  // (distinct jobs per thread)
            rr.push_back(static_cast<double>(h_result[i]) / std::max(J.n, J.m));
          }
          std::lock_guard<std::mutex> lk(mu_);
          st.n_aligned += n_al;
          st.sum_distance += sum_d;
          rates.insert(rates.end(), rr.begin(), rr.end());
          rest_of.insert(rest_of.end(), other.begin(), other.end());
        });
        std::sort(rest_of.begin(), rest_of.end());  // (the threads finish in any order)
      }
      for (u32 i : rest_of) {
        NwJob& J = jobs[i];
        if (h_status[i] == 2) {  // distance above the threshold: twice the band (and the variant that holds it)
          ++st.n_retries;
          if (J.k >= static_cast<u64>(J.n) + J.m || !plan(J, static_cast<u64>(J.k) * 2)) ++st.n_unaligned;
          else again.push_back(i);
        } else if (h_status[i] != 0) {
          throw HipError("[raven_hip] alignment path: the walk left the stored band (internal error)");
        } else {  // (a sweep-only pass: the pilot)
          obs.push_back(NwObs{static_cast<double>(std::max(J.n, J.m)), static_cast<double>(h_result[i])});
        }
      }
    }
    early.clear();
    queued.clear();
    h_res += since(t_h);
  }

  // Whether an alignment is beyond its threshold is known when its SWEEP is done: the states are read once the sweeps of
  // everything queued are through — the last walks still run on their streams — and the few jobs above their thresholds
  // (two or three of 295 000 at C4) are planned again and queued at once, as a compact pass on the head's buffer set,
  // instead of as a pass of their own behind the last walk (~9 ms per round of sweep + lonely walk + host round trips,
  // profiles/r05_nw_timeline.csv).  A job handed on here is skipped by collect() in the pass that found it.
  void retry_early() {
    if (one_stream || queued.empty()) return;
    join_side();
    for (Queued& q : queued)
      if (q.dev.compact) {
        q.status.resize(q.order.size());
        RVN_HIP(hipMemcpyAsync(q.status.data(), q.dev.status, q.order.size() * 4, hipMemcpyDeviceToHost, s));
      }
    RVN_HIP(hipMemcpyAsync(h_status.data(), dev.all.status, static_cast<size_t>(nj) * 4, hipMemcpyDeviceToHost, s));
    RVN_HIP(rvn_stream_sync(s));  // (the sweeps; not the walks)
    std::vector<u32> todo;
    for (const Queued& q : queued)
      for (size_t x = 0; x < q.order.size(); ++x) {
        const u32 i = q.order[x];
        if ((q.dev.compact ? q.status[x] : h_status[i]) != 2) continue;
        if (todo.size() >= kHeadMax) break;  // (a wrong rate estimate: the ordinary repeat pass takes them)
        NwJob& J = jobs[i];
        if (J.k >= static_cast<u64>(J.n) + J.m) continue;  // (collect() counts it as unaligned)
        const NwJob before = J;
        if (!plan(J, static_cast<u64>(J.k) * 2)) {
          J = before;
          continue;
        }
        todo.push_back(i);
      }
    if (todo.empty()) return;
    early.assign(nj, 0);
    for (u32 i : todo) early[i] = 1;
    st.n_retries += todo.size();
    std::vector<u32> left;
    // (set 3 may have to grow for a doubled band, and growing hands the old block back: the walk on it — the head's, queued
    // long before — must be through)
    if (set_used[3]) RVN_HIP(hipEventSynchronize(e.nw.ev[3]));
    enqueue(todo, false, kHeadOnly, dev.retry, e.nw.streams[4], &left);
    for (u32 i : left) early[i] = 0;  // (beyond the set's share: their doubled plan stands, collect() doubles it once more)
    st.n_retries -= left.size();
  }

  // aligns every job of `todo` (already planned), repeating the ones beyond their threshold with twice the band
  void run(std::vector<u32> todo, bool sweep_only) {
    while (!todo.empty()) {
      enqueue(todo, sweep_only, kOwnFirst, dev.all, s, nullptr);
      std::vector<u32> again;
      collect(again);
      todo.swap(again);
    }
  }
};

}  // namespace

// Fills the band fields of `jobs` (k, kcap, R, G, hs, ckpt) and produces every job's window records in d_recs
// (records of a job start at its bp_off; jobs that cannot be aligned keep all-invalid records and are counted).
// What is decided here is in nwplan.h, how it is launched in NwRun above; this is the schedule of a call.
void nw_breakpoints(Engine& e, const ReadsDev& T, const ReadsDev& Rd, std::vector<NwJob>& jobs, u32 w,
                    NwWindowRec* d_recs, u64 n_recs, NwStats& st, std::vector<u32>* distances, NwPathSlots* path) {
  st = NwStats();
  const u32 nj = static_cast<u32>(jobs.size());
  if (distances) distances->assign(nj, ~0u);
  if (path) path->slot_end.assign(nj, 0);
  hipStream_t s = e.stream;
  if (n_recs) RVN_HIP(hipMemsetAsync(d_recs, 0xFF, n_recs * sizeof(NwWindowRec), s));
  e.nw.last = st;
  if (nj == 0) return;
  RVN_HIP(hipEventRecord(e.ev0, s));
  if (!e.nw.streams[0]) e.nw.open();
  WalkGuard walk_guard{e};
  double rate = e.nw.rate > 0 ? e.nw.rate : 0.13;  // first call: ONT-like; too small only costs a repeat
  if (const char* ev = knob("RVN_NW_RATE")) rate = std::atof(ev);  // (debug builds: force repeats)
  std::vector<u32> valid;
  for (u32 i = 0; i < nj; ++i) {
    const NwJob& J = jobs[i];
    if (J.n == 0 || J.m == 0 || J.n >= (1u << 30) || J.m >= (1u << 30)) ++st.n_unaligned;
    else valid.push_back(i);
  }
  NwRun pass(e, T, Rd, jobs, w, d_recs, path, st, distances);  // (the budget, the call's device arrays)

  // Thresholds (nwplan.h: NwThresholdModel): a pilot sample, swept for its distances only, gives the model everyone's
  // threshold comes from.  Small batches keep the previous call's estimate.
  std::vector<u32> rest, head;
  NwThresholdModel model;
  if (valid.size() >= 4096 && !knob("RVN_NW_RATE")) {
    rest = valid;  // the pilot is swept for its distances only; its jobs are aligned with everyone else
    std::vector<u32> ok;
    for (u32 i : nw_pilot_sample(jobs, valid))
      if (pass.plan(jobs[i], NwThresholdModel::pilot_threshold(nw_job_len(jobs[i]), rate))) ok.push_back(i);
    pass.enqueue(ok, true, kOwnFirst, pass.dev.all, s, nullptr);
    // (while the pilot is swept) the longest alignments: they go first and by themselves, see below
    if (!pass.one_stream) nw_take_head(jobs, rest, head);
    {
      std::vector<u32> again;
      pass.collect(again);
      pass.run(again, true);
    }
    model.fit(pass.obs);
  } else {
    rest = valid;
  }
  {
    auto t_h = clk::now();
    // The longest alignments are a pass of their own, queued the moment the thresholds exist: planning, ordering and
    // uploading 300 000 jobs took the host ~20 ms in which the GPU did nothing (profiles/r05_nw_timeline.csv: 6.6 -> 28.7 ms),
    // every round; now the head's sweeps (~23 ms at C4) run in that time, and its walk — the long pole, one lane per
    // alignment — starts that much earlier.  (Results do not depend on which pass or chunk a job is in.)
    std::vector<u32> ok_head, left;
    for (u32 i : head) {
      if (pass.plan(jobs[i], model.threshold(nw_job_len(jobs[i]), rate))) ok_head.push_back(i);
      else ++st.n_unaligned;
    }
    const bool split = !ok_head.empty();
    if (split) pass.enqueue(ok_head, false, kHeadOnly, pass.dev.head, s, &left);
    std::vector<u8> planned(rest.size());
    parallel_for(rest.size(), 16384, [&jobs, &rest, &planned, &model, rate, sl = pass.stripe_lanes, budget = pass.budget](size_t x0, size_t x1) {
      for (size_t x = x0; x < x1; ++x) {
        NwJob& J = jobs[rest[x]];
        planned[x] = nw_plan(J, model.threshold(nw_job_len(J), rate), sl, budget) ? 1 : 0;
      }
    });
    std::vector<u32> ok;
    ok.reserve(rest.size() + left.size());
    for (size_t x = 0; x < rest.size(); ++x) {
      if (planned[x]) ok.push_back(rest[x]);
      else ++st.n_unaligned;
    }
    ok.insert(ok.end(), left.begin(), left.end());
    pass.h_plan += since(t_h);
    pass.enqueue(ok, false, split ? kRotating : kOwnFirst, pass.dev.all, split ? e.nw.streams[4] : s, nullptr);
    pass.retry_early();
    std::vector<u32> again;
    pass.collect(again);
    pass.run(again, false);
  }
  RVN_HIP(hipEventRecord(e.ev1, s));
  e.nw.rate = nw_next_rate(pass.rates, e.nw.rate);
  RVN_HIP(hipEventSynchronize(e.ev1));
  float ms = 0;
  RVN_HIP(hipEventElapsedTime(&ms, e.ev0, e.ev1));
  st.ms = ms;
  e.nw.last = st;
  if (knob("RVN_NW_DEBUG"))
    std::fprintf(stderr, "[raven_hip] nw host: plan %.1f ms, order + chunks %.1f ms, uploads %.1f ms, results %.1f ms\n", pass.h_plan, pass.h_order,
                 pass.h_up, pass.h_res);
  if (knob("RVN_NW_DEBUG"))
    std::fprintf(stderr, "[raven_hip] nw: %u jobs, %llu aligned, %llu retries, %llu chunks, %.3e band cells, %.1f MB hs + ck, %.1f ms; pilot mu %.4f a %.4f b %.3e\n", nj,
                 static_cast<unsigned long long>(st.n_aligned), static_cast<unsigned long long>(st.n_retries),
                 static_cast<unsigned long long>(st.n_batches), static_cast<double>(st.band_cells),
                 st.store_bytes / 1048576.0, ms, model.mu, model.va, model.vb);
}

// ---- the path form: the walkers' runs, dense and in pair order; edlib's one byte per op ----------------------------------
namespace {

constexpr u32 kNwPathWindow = 1u << 30;  // one window for the whole span (spans are shorter): the walker's window logic idles

// pairs 0 .. n (entry n: 0, so that the scan's last entry is the total): runs of the pair — what its walker counted, one
// for a pair with an empty span (synth = its run), none for a pair that was not aligned or is empty on both sides
__global__ __launch_bounds__(256) void nw_path_count_kernel(const u64* __restrict__ slot_end, const u32* __restrict__ synth,
                                                            u32 n, u32* __restrict__ cnt) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  u32 c = 0;
  if (i < n) {
    const u32* end = reinterpret_cast<const u32*>(slot_end[i]);
    c = end ? *end : (synth[i] ? 1u : 0u);
  }
  cnt[i] = c;
}

// one wave per pair: the used tail of its slot to runs[run_off[pair] ..] (coalesced both ways), the ops its runs stand for
// (the sum of their counts) to op_cnt[pair]; op_cnt[n] = 0
__global__ __launch_bounds__(256) void nw_path_pack_kernel(const u64* __restrict__ slot_end, const u32* __restrict__ synth,
                                                           const u64* __restrict__ run_off, u32 n, u32* __restrict__ runs,
                                                           u32* __restrict__ op_cnt) {
  const u32 pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = lane_id();
  if (pair > n) return;
  if (pair == n) {
    if (lane == 0) op_cnt[n] = 0;
    return;
  }
  const u64 o = run_off[pair];
  const u32 c = static_cast<u32>(run_off[pair + 1] - o);
  const u32* end = reinterpret_cast<const u32*>(slot_end[pair]);
  const u32 one = synth[pair];
  u32 sum = 0;
  for (u32 x = static_cast<u32>(lane); x < c; x += 64) {
    const u32 v = end ? end[static_cast<long long>(x) - static_cast<long long>(c)] : one;
    runs[o + x] = v;
    sum += v >> 2;
  }
  sum = wave_sum(sum);
  if (lane == 0) op_cnt[pair] = sum;
}

// one workgroup per pair: its runs in tiles of 256 — the tile's run lengths are scanned in LDS, then the 256 threads write
// the tile's stretch of output side by side (consecutive threads, consecutive bytes), each finding its run by bisection
__global__ __launch_bounds__(256) void nw_path_expand_kernel(const u64* __restrict__ run_off, const u32* __restrict__ runs,
                                                             const u64* __restrict__ op_off, u8* __restrict__ ops) {
  __shared__ u32 s_incl[256];
  __shared__ u8 s_op[256];
  __shared__ u32 s_w[4];
  const u32 pair = blockIdx.x;
  const u64 r0 = run_off[pair], r1 = run_off[pair + 1];
  u8* out = ops + op_off[pair];
  for (u64 base = r0; base < r1; base += 256) {
    const u64 x = base + threadIdx.x;
    const u32 v = x < r1 ? runs[x] : 0u;
    u32 total = 0;
    const u32 excl = block_exclusive_sum_256<u32>(v >> 2, s_w, &total);
    s_incl[threadIdx.x] = excl + (v >> 2);
    s_op[threadIdx.x] = static_cast<u8>(v & 3u);
    __syncthreads();
    for (u32 pos = threadIdx.x; pos < total; pos += 256) {
      u32 lo = 0, hi = 255;  // the first run whose inclusive sum is above pos
      while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (s_incl[mid] > pos) hi = mid;
        else lo = mid + 1;
      }
      out[pos] = s_op[lo];
    }
    out += total;
    __syncthreads();
  }
}

}  // namespace

void nw_align_paths(Engine& e, const ReadsDev& T, const ReadsDev& Q, std::vector<NwJob>& jobs, NwPaths& out) {
  const u32 n = static_cast<u32>(jobs.size());
  hipStream_t s = e.stream;
  out.n = n;
  out.n_not_aligned = 0;
  out.n_runs = out.n_ops = 0;
  NwPathSlots slots;
  NwStats st;
  nw_breakpoints(e, T, Q, jobs, kNwPathWindow, nullptr, 0, st, &out.distances, &slots);
  out.device_ms = st.ms;
  // a pair with an empty span has one run and no walk: the other span's bases, query only ('I') or target only ('D')
  std::vector<u32> synth(static_cast<size_t>(n) + 1, 0);
  for (u32 i = 0; i < n; ++i) {
    const NwJob& J = jobs[i];
    if (J.n == 0 || J.m == 0) {
      out.distances[i] = J.n + J.m;
      if (J.n + J.m) synth[i] = ((J.n + J.m) << 2) | (J.m ? kNwOpInsert : kNwOpDelete);
    } else if (out.distances[i] == ~0u) {
      ++out.n_not_aligned;
      slots.slot_end[i] = 0;
    }
  }
  slots.slot_end.push_back(0);
  DevBuf d_end_b, d_synth_b, d_cnt_b;
  u64* d_end = d_end_b.get<u64>(static_cast<size_t>(n) + 1);
  u32* d_synth = d_synth_b.get<u32>(static_cast<size_t>(n) + 1);
  u32* d_cnt = d_cnt_b.get<u32>(static_cast<size_t>(n) + 1);
  u64* d_run_off = out.run_off.get<u64>(static_cast<size_t>(n) + 1);
  u64* d_op_off = out.op_off.get<u64>(static_cast<size_t>(n) + 1);
  RVN_HIP(hipEventRecord(e.ev0, s));
  RVN_HIP(hipMemcpyAsync(d_end, slots.slot_end.data(), (static_cast<size_t>(n) + 1) * 8, hipMemcpyHostToDevice, s));
  RVN_HIP(hipMemcpyAsync(d_synth, synth.data(), (static_cast<size_t>(n) + 1) * 4, hipMemcpyHostToDevice, s));
  RVN_KLAUNCH(kKNwTraceback, nw_path_count_kernel<<<n / 256 + 1, 256, 0, s>>>(d_end, d_synth, n, d_cnt));
  exclusive_scan_u32_u64(d_cnt, d_run_off, static_cast<u64>(n) + 1, e.scratch.scan_tmp, s);
  u64 total = 0;
  RVN_HIP(hipMemcpyAsync(&total, d_run_off + n, 8, hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));  // (also: `synth` and the slot addresses are pageable)
  out.n_runs = total;
  u32* d_runs = out.runs.get<u32>(static_cast<size_t>(total) + 1);
  RVN_KLAUNCH(kKNwTraceback, nw_path_pack_kernel<<<n / 4 + 1, 256, 0, s>>>(d_end, d_synth, d_run_off, n, d_runs, d_cnt));
  exclusive_scan_u32_u64(d_cnt, d_op_off, static_cast<u64>(n) + 1, e.scratch.scan_tmp, s);
  RVN_HIP(hipMemcpyAsync(&total, d_op_off + n, 8, hipMemcpyDeviceToHost, s));
  RVN_HIP(hipEventRecord(e.ev1, s));
  RVN_HIP(rvn_stream_sync(s));  // (the slots go back when this returns)
  out.n_ops = total;
  float ms = 0;
  RVN_HIP(hipEventElapsedTime(&ms, e.ev0, e.ev1));
  out.device_ms += ms;
}

void nw_paths_expand(Engine& e, const NwPaths& p, u8* d_ops) {
  if (p.n == 0 || p.n_ops == 0) return;
  RVN_KLAUNCH(kKNwTraceback, nw_path_expand_kernel<<<p.n, 256, 0, e.stream>>>(p.run_off.as<u64>(), p.runs.as<u32>(), p.op_off.as<u64>(), d_ops));
}

#ifdef RVN_TEST_HOOKS
// ---- CPU stepper of the same code (test hook rvn_test_nw_breakpoints): 64 emulated lanes, host arrays --------------
static u64 g_group_batches_store = 0;
static u64* const g_group_batches = &g_group_batches_store;  // batches of the hook's last group walk (band[3] when a group walk is asked for)
static int walk_host(const NwJob& J, const NwGeo& g, const u64* t_words, const u64* r_words, const std::vector<u32>& hs,
                     const std::vector<NwPm>& ck, u32 res, u32 w, NwWindowRec* recs, u32* band, int walk_gl);
template <int R>
static int emulate_job(NwJob J, u32 G, const u64* t_words, const u64* r_words, u32 w, NwWindowRec* recs, u32* distance,
                       u32* band, int walk_gl) {
  std::vector<u64> peq(static_cast<size_t>(R) * 4 * 64);
  std::vector<NwSweepLane<R, 64>> lanes(64);
  std::vector<int> xp(64), sp(64);
  std::vector<u32> hs;
  std::vector<NwPm> ck;
  NwGeo g;
  u32 res = 0;
  for (;;) {
    g = nw_geo(J.n, J.m, J.k, R);
    if (static_cast<u32>(g.L) > G) return -3;  // beyond this variant's ring
    hs.assign(g.hs_words() + 4 * 64 * 8 + 16, 0xA5A5A5A5u);
    ck.assign(g.ck_entries() + 16, NwPm{0x1234567887654321ULL, 0x0FEDCBA99ABCDEF0ULL});
    for (int l = 0; l < 64; ++l) {
      if (l < static_cast<int>(G)) lanes[l].init(J, t_words, r_words, g, l, peq.data(), l);
      else lanes[l].init_idle(peq.data(), l);
    }
    const int n_steps_w = (g.n_steps + 15) & ~15;
    const int n_g = (g.n_steps + kNwHsSteps - 1) / kNwHsSteps, n_q = g.n_steps / kNwCkSteps;
    const u64 row = static_cast<u64>(g.L) * R;
    for (int t = 1; t <= n_steps_w; ++t) {
      for (int l = 0; l < 64; ++l) {  // the shuffles read the previous lane's values of the previous step
        const int src = l == 0 ? g.L - 1 : l - 1;
        xp[l] = lanes[src].xf;
        sp[l] = lanes[src].sc;
      }
      for (int l = 0; l < 64; ++l)
        if (lanes[l].has_event(t)) lanes[l].event(t, xp[l], sp[l]);
      for (int l = 0; l < 64; ++l) lanes[l].step(t, xp[l]);
      if ((t & 15) == 0) {
        const int gi = (t >> 4) - 1;
        for (int l = 0; l < g.L; ++l) {
          if (gi < n_g)
            for (int r = 0; r < R; ++r) hs[static_cast<u64>(gi) * row + static_cast<u64>(l) * R + r] = lanes[l].acc[r];
          if ((t & 31) == 0 && (t >> 5) - 1 < n_q)
            for (int r = 0; r < R; ++r)
              ck[static_cast<u64>((t >> 5) - 1) * row + static_cast<u64>(l) * R + r] = NwPm{lanes[l].Pv[r], lanes[l].Mv[r]};
        }
        for (int l = 0; l < 64; ++l) lanes[l].next_group(t);
      }
    }
    u32 res1 = 0;
    for (int l = 0; l < 64; ++l) res1 = std::max(res1, lanes[l].result);
    if (res1 == 0) return -5;
    res = res1 - 1u;
    if (res <= J.k) break;
    if (J.k >= J.n + J.m) return -5;
    J.k = static_cast<u32>(std::min<u64>(2ULL * J.k, static_cast<u64>(J.n) + J.m));
  }
  *distance = res;
  if (band) {
    band[0] = J.k;
    band[1] = static_cast<u32>(g.L);
    band[2] = R;
  }
  return walk_host(J, g, t_words, r_words, hs, ck, res, w, recs, band, walk_gl);
}

// the walk of an emulated sweep, in the form the hook asks for
static int walk_host(const NwJob& J, const NwGeo& g, const u64* t_words, const u64* r_words, const std::vector<u32>& hs,
                     const std::vector<NwPm>& ck, u32 res, u32 w, NwWindowRec* recs, u32* band, int walk_gl) {
  if (walk_gl == 16) return nw_trace_group_host<16>(J, g, t_words, r_words, hs.data(), ck.data(), res, w, recs, band ? g_group_batches : nullptr);
  if (walk_gl == 64) return nw_trace_group_host<64>(J, g, t_words, r_words, hs.data(), ck.data(), res, w, recs, band ? g_group_batches : nullptr);
  if (walk_gl == 4) return nw_trace_group_host<4>(J, g, t_words, r_words, hs.data(), ck.data(), res, w, recs, band ? g_group_batches : nullptr);
  if (walk_gl == 1) {  // the lane walk as nw_trace_kernel<true> runs it: strips of sixteen kept columns
    u64 pv16[kNwLaneStripCols + 1], mv16[kNwLaneStripCols + 1];
    const NwStripMem<1> mem16{pv16, mv16, 0};
    return nw_trace_job<1, kNwLaneStripCols>(J, g, t_words, r_words, hs.data(), ck.data(), mem16, res, w, recs);
  }
  if (walk_gl != 0) return -2;
  u64 pv[kNwStripCols], mv[kNwStripCols];
  const NwStripMem<1> mem{pv, mv, 0};
  return nw_trace_job<1>(J, g, t_words, r_words, hs.data(), ck.data(), mem, res, w, recs);
}

// The striped sweep as nw_sweep_kernel<R, 64, true> runs it, stripe after stripe (one launch each), then the walk.
// band: {k, lanes one ring would need, R, group-walk batches, stripes}
template <int R>
static int emulate_striped(NwJob J, u32 S, const u64* t_words, const u64* r_words, u32 w, NwWindowRec* recs, u32* distance,
                           u32* band, int walk_gl) {
  std::vector<u64> peq(static_cast<size_t>(R) * 4 * 64);
  std::vector<NwSweepLane<R, 64, true>> lanes(64);
  std::vector<int> xp(64), sp(64);
  std::vector<u32> hs;
  std::vector<NwPm> ck;
  NwGeo g;
  u32 res = 0;
  J.R = R;
  J.G = 64;
  J.S = S;
  for (;;) {
    g = nw_geo_job(J);
    if (nw_ring_lanes(static_cast<u32>(g.lo), static_cast<u32>(g.hi), R) > kNwMaxStripes * S) return -3;  // refused
    hs.assign(g.hs_words() + 4 * 64 * 8 + 16, 0xA5A5A5A5u);
    ck.assign(g.ck_entries() + 16, NwPm{0x1234567887654321ULL, 0x0FEDCBA99ABCDEF0ULL});
    u32 res1 = 0;
    const u64 row = static_cast<u64>(S) * R;
    for (int st = 0; st < g.n_stripes; ++st) {
      NwGeo gs = g;
      gs.s0 = st * g.S;
      gs.s1 = std::min(g.n_super, gs.s0 + g.S);
      const int t0 = g.st_t0(st), g0 = (t0 - 1) >> 4, q0 = (t0 - 1) >> 5;
      const int n_steps_w = (gs.je(gs.s1 - 1) + gs.s1 + 15) & ~15;
      const bool last = gs.s1 == g.n_super;
      int t_hand = kNwNever, lig_hand = -1, sc_hand = 0, sc_in = 0;
      if (!last && gs.ja(gs.s1) > 1) {
        t_hand = gs.ja(gs.s1) + gs.s1;
        lig_hand = gs.s1 - 1 - gs.s0;
      }
      NwTopIn top;
      if (st > 0) {
        top.init(hs.data(), gs, t0);
        sc_in = static_cast<int>(hs[g.hand_at(st - 1)]);
      }
      u32* hs_j = hs.data() + static_cast<u64>(st) * g.stripe_hs_words();
      NwPm* ck_j = ck.data() + static_cast<u64>(st) * g.stripe_ck_entries();
      for (int l = 0; l < 64; ++l) {
        if (l < static_cast<int>(S)) lanes[l].init(J, t_words, r_words, gs, l, peq.data(), l);
        else lanes[l].init_idle(peq.data(), l);
      }
      for (int t = t0; t <= n_steps_w; ++t) {
        for (int l = 0; l < 64; ++l) {
          const int src = l == 0 ? g.L - 1 : l - 1;
          xp[l] = lanes[src].xf;
          sp[l] = lanes[src].sc;
        }
        if (st > 0) {
          xp[0] = top.x(t);
          sp[0] = sc_in;
        }
        if (t == t_hand) sc_hand = lanes[lig_hand].sc;
        for (int l = 0; l < 64; ++l)
          if (lanes[l].has_event(t)) lanes[l].event(t, xp[l], sp[l]);
        for (int l = 0; l < 64; ++l) lanes[l].step(t, xp[l]);
        if ((t & 15) == 0) {
          const int gi = (t >> 4) - 1;
          for (int l = 0; l < g.L; ++l) {
            if (gi - g0 < g.gps)
              for (int r = 0; r < R; ++r) hs_j[static_cast<u64>(gi - g0) * row + static_cast<u64>(l) * R + r] = lanes[l].acc[r];
            if ((t & 31) == 0 && (t >> 5) - 1 - q0 < g.qps)
              for (int r = 0; r < R; ++r)
                ck_j[static_cast<u64>((t >> 5) - 1 - q0) * row + static_cast<u64>(l) * R + r] = NwPm{lanes[l].Pv[r], lanes[l].Mv[r]};
          }
          for (int l = 0; l < 64; ++l) lanes[l].next_group(t);
          if (st > 0) top.next_group(t);
        }
      }
      if (lig_hand >= 0) hs_j[row * static_cast<u64>(g.gps)] = static_cast<u32>(sc_hand);
      if (last)
        for (int l = 0; l < 64; ++l) res1 = std::max(res1, lanes[l].result);
    }
    if (res1 == 0) return -5;
    res = res1 - 1u;
    if (res <= J.k) break;
    if (J.k >= J.n + J.m) return -5;
    J.k = static_cast<u32>(std::min<u64>(2ULL * J.k, static_cast<u64>(J.n) + J.m));
  }
  *distance = res;
  if (band) {
    band[0] = J.k;
    band[1] = nw_ring_lanes(static_cast<u32>(g.lo), static_cast<u32>(g.hi), R);
    band[2] = R;
    band[4] = static_cast<u32>(g.n_stripes);
  }
  return walk_host(J, g, t_words, r_words, hs, ck, res, w, recs, band, walk_gl);
}

// force_R > 0: that many blocks per lane (whole-wave ring); force_R < 0: R = 1 with a ring of at most -force_R lanes
// (the lane groups of the narrow variants); force_R >= 1000: the variant (R, G) = (force_R / 1000, force_R % 1000);
// 0: the narrowest variant that holds k, the next one on overflow
int nw_breakpoints_host(const u64* t_words, u32 t_len, const u64* r_words, u32 r_len, u32 t_begin, u32 n, u32 q_begin,
                        u32 m, int rc, u32 w, u32 k, int force_R, NwWindowRec* recs, u32* distance, u32* band) {
  (void)t_len;
  const int walk_gl = (rc >> 8) & 0xFF;  // bits 8-15 of rc: lanes per alignment of the group walk (0: the lane walk)
  const u32 stripe_lanes = static_cast<u32>(rc >> 16) & 0xFFu;  // bits 16-23: lanes per stripe of a striped sweep (0: none)
  rc &= 1;
  g_group_batches_store = 0;
  if (n == 0 || m == 0) return -1;
  NwJob J{};
  J.t_begin = t_begin;
  J.n = n;
  J.q_begin = q_begin;
  J.m = m;
  J.r_len = r_len;
  J.rc = rc ? 1 : 0;
  J.n_windows = (t_begin + n - 1) / w - t_begin / w + 1;
  for (u32 x = 0; x < J.n_windows; ++x) {
    recs[x].first_t = recs[x].first_q = recs[x].last_t = recs[x].last_q = 0xFFFFFFFFu;
    for (int g = 0; g < 8; ++g) recs[x].grid[g] = 0xFFFFu;
  }
  const u32 d = n > m ? n - m : m - n;
  u64 kk = std::min<u64>(std::max<u64>(std::max<u64>(k, d), 1), static_cast<u64>(n) + m);
  if (stripe_lanes) {  // striped, whatever the band: R = force_R (1 / 2 / 4 / 8; default 1)
    if (stripe_lanes > 64) return -2;
    J.k = static_cast<u32>(kk);
    int rcode;
    switch (force_R) {
      case 0:
      case 1: rcode = emulate_striped<1>(J, stripe_lanes, t_words, r_words, w, recs, distance, band, walk_gl); break;
      case 2: rcode = emulate_striped<2>(J, stripe_lanes, t_words, r_words, w, recs, distance, band, walk_gl); break;
      case 4: rcode = emulate_striped<4>(J, stripe_lanes, t_words, r_words, w, recs, distance, band, walk_gl); break;
      case 8: rcode = emulate_striped<8>(J, stripe_lanes, t_words, r_words, w, recs, distance, band, walk_gl); break;
      default: return -2;
    }
    if (walk_gl && band && rcode >= 0) band[3] = static_cast<u32>(g_group_batches_store);
    return rcode;
  }
  u32 lvl = 0;
  if (force_R >= 1000) {  // R * 1000 + G: one particular variant
    while (lvl < kLevels && !(kNwVariants[lvl].R == static_cast<u32>(force_R / 1000) && kNwVariants[lvl].G == static_cast<u32>(force_R % 1000))) ++lvl;
    if (lvl == kLevels) return -2;
  } else if (force_R > 0) {  // that many blocks per lane, whole-wave ring
    while (lvl < kLevels && !(kNwVariants[lvl].R == static_cast<u32>(force_R) && kNwVariants[lvl].G == 64)) ++lvl;
    if (lvl == kLevels) return -2;
  } else if (force_R < 0) {  // one block per lane, ring of at most -force_R lanes
    while (lvl < kLevels && !(kNwVariants[lvl].R == 1 && kNwVariants[lvl].G == static_cast<u32>(-force_R))) ++lvl;
    if (lvl == kLevels) return -2;
  }
  for (; lvl < kLevels; ++lvl) {
    const u32 cap = kcap_of(n, m, kNwVariants[lvl].R, kNwVariants[lvl].G);
    if (cap < kk) {
      if (force_R) return -2;
      continue;
    }
    J.R = kNwVariants[lvl].R;
    J.G = kNwVariants[lvl].G;
    J.k = static_cast<u32>(kk);
    J.kcap = cap;
    int rcode;
    switch (J.R) {
      case 1: rcode = emulate_job<1>(J, J.G, t_words, r_words, w, recs, distance, band, walk_gl); break;
      case 2: rcode = emulate_job<2>(J, J.G, t_words, r_words, w, recs, distance, band, walk_gl); break;
      case 4: rcode = emulate_job<4>(J, J.G, t_words, r_words, w, recs, distance, band, walk_gl); break;
      default: rcode = emulate_job<8>(J, J.G, t_words, r_words, w, recs, distance, band, walk_gl); break;
    }
    if (walk_gl && band) band[3] = static_cast<u32>(g_group_batches_store);
    if (rcode == -3 && !force_R) {  // the doubled threshold no longer fits this variant's ring
      kk = std::min<u64>(static_cast<u64>(cap) + 1, static_cast<u64>(n) + m);
      continue;
    }
    return rcode;
  }
  return -3;
}

#endif  // RVN_TEST_HOOKS

}  // namespace rvn
