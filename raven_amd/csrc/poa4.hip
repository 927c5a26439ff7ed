// poa4.hip — banded POA window kernel with the graph ROWS ON THE LANES: the first attempt of rvn_poa_consensus_batch / of
// a polishing round's consensus stage (racon Window::GenerateConsensus over spoa, as driven by raven::Polish,
// RavenLib/src/polish.cc:43-51; scores RavenLib/include/raven/graph/polish.hpp:13-17).  Same algorithm, graph layout, tie
// rules and escalation as poa2.hip (a window whose alignment touches the 32-column band goes on to poa2's 64 / 128 /
// 256 columns and the full-matrix kernel); what changes is how the NW of a layer sits on the wave.
//
// poa2 advances ONE graph row per loop iteration (64 lanes = 64 columns): every iteration is a dependent chain
// (ring write -> ring read -> candidates -> 6-step prefix maximum -> ring write) behind ~90 scalar instructions of row
// decode, and the kernel waits more than it issues.  Here a window owns 16 lanes, a lane owns a whole graph row and
// walks it left to right, two columns per step, so
//   * the horizontal gap chain is two max instructions inside the lane (no cross-lane prefix),
//   * a predecessor row is read from the window's LDS ring where another lane left it >= 1 step earlier (one aligned
//     32-bit read per in-edge and step: the static schedule below guarantees the cells exist), and a row's descriptor
//     (band start, match mask against the layer, LDS addresses of up to 8 predecessor rows) is one 32-byte record built
//     by a per-layer pre-pass, so the step loop decodes nothing,
//   * in-edges are folded with v_max on (score << 8 | diagonal << 3 | 7 - in-edge) keys: spoa's tie rule (diagonal
//     before vertical, first in-edge first) is the maximum's and the backpointer falls out of its low bits: FOUR bits per
//     cell.  0 = horizontal AND "vertical through the eighth in-edge" (tag 7 - 7): for the rows that have eight in-edges
//     (2.5 % of C4-like windows have one) the NW leaves one bit per column beside the row saying which of the two a code 0
//     is (Poa4Slot::v7; round 5 sent the window to poa2 when a walk met the case: 836 windows and a second kernel per round),
//   * backpointers leave as ONE coalesced 8-byte store per lane and 8 steps into a time-major stream (step, lane); the
//     traceback maps (row, column) -> (step, lane) through the descriptor.
// Schedule (all band starts even and non-decreasing along the topological order): row rho of the layer's rank range
// runs on lane rho % 16 during steps S - 1 .. S + 15, S = rho + rho / 16 + (b_rho - b_0) / 2 + 1 (step S - 1 only reads:
// it loads the cell left of the first column), computing columns b + 2k, b + 2k + 1 at step S + k.  A predecessor pi
// < rho with band start b_pi <= b_rho has written column j by step S_pi + (j - b_pi) / 2 <= S_rho + (j - b_rho) / 2 - 1:
// one step before it is read.  Sixteen lanes are always busy except for the (b - b_0) / 2 drift (~20 % of the steps).
//
// How a batch runs (round 5): ONE launch of persistent waves.  A wave takes a group of four windows (scheduling order =
// by decreasing layer count) from an atomic counter and carries it from the backbone graphs to the consensus: per layer the
// graph side of each window in turn (all 64 lanes on one window: graph update with the previous alignment, the next
// layer's set-up, its row descriptors), then NW and traceback of the four side by side.  Round 4 ran every phase as a
// kernel of its own over a chunk of windows in lock step (five launches per layer round on four streams): the rounds'
// barriers left ~45 % of the wave slots idle and every phase met its window's data cold (poa4_persistent below).
//
// Integer VALU + LDS bound; no MFMA.  Written against sv:: (simt.h): the same source runs under the host wavefront
// emulator (tests/test_poa4_emulation.py -> rvn_poa_banded_emulate: variant 5 = the persistent kernel, variant 4 = the
// same phase functions stepped wave by wave in lock step).
//
// This file is the translation unit: the thin phase functions, the LDS unions, the persistent driver, the kernel, its
// launch and the emulator entry.  The rest, one header per concern, included here only and in this order:
//   poa4_limits.h  the kernel's limits (struct P4); plain C++, also read by tests/test_poa4_limits.py
//   poa4_layout.h  LDS of the NW, batch description, a window's scratch slot, the state record (Poa4Win, Poa4Ctx)
//   poa4_ops.h     one-instruction helpers and compiler fences with their host twins: where GPU and emulator part
//   poa4_nw.h      the NW step (poa4_dp): the part that is fragile under the compiler (tests/test_poa4_isa.py)
//   poa4_tb.h      the traceback
//   poa4_graph.h   backbone graph and phase 0, graph update, consensus
//   poa4_desc.h    layer set-up, subgraph sweep, band guide, row descriptors
//   poa4_esc.h     the in-launch escalation queue and the far call to poa2's window function (behind Poa4LdsAll, below)
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poa4_limits.h"
#include "poa4_layout.h"
#include "poa4_ops.h"
#include "poa4_nw.h"
#include "poa4_tb.h"
#include "poa4_graph.h"
#include "poa4_desc.h"

namespace rvn {
namespace {

// phase B: the NW
template <class K, class SC>
__host__ __device__ inline void poa4_phase_dp(const Poa4Args& A, const Poa4Ctx& C, Poa4Lds& S, u32 wave) {
  const int lane = sv::lane();
  const int q = lane / K::GS;
  const unsigned long long t0 = sv::clock();
  const u32 my_rec = poa4_my_record(C, wave, q);
  u32 act = 0, t_end = 0, len = 0, li = 0;
  if (my_rec != 0xFFFFFFFFu) {
    Poa4Win& w = C.st[my_rec];
    act = (w.phase == kRunning && w.act) ? 1u : 0u;
    t_end = w.t_end;
    len = w.len;
    li = w.li;
    if (act && (w.dflag || t_end + 8u > poa4_steps(A.nmax, A.lmax))) {
      // beyond this kernel's limits (in-degree, in-edge length, band step): the 64-column kernel's job
      if ((lane & (K::GS - 1)) == 0) {
        w.phase = kFailed;
        // (bits 24-27: why, for the statistics of the debug build — 1..7 a limit of this kernel: 3 in-degree, 7 band step along
        // an in-edge, 1 steps; 9 the last column in no end node's band; 10 the walk came near a band's edge; 11 the walk met
        // a backpointer it cannot follow)
        w.status = kPoaBandHit | (li << 8) | ((w.dflag ? (w.dflag & 7u) : 1u) << 24);
        w.act = 0;
      }
      act = 0;
    }
  }
  if (!sv::any(act != 0)) return;
  u32 best_rho1 = 0;
  poa4_dp<K, SC>(A, S, poa4_slot_of(A, C, wave, q), act != 0, t_end, len, best_rho1);
  if (act && (lane & (K::GS - 1)) == 0) {
    Poa4Win& w = C.st[my_rec];
    w.best_rho1 = best_rho1;
    if (best_rho1 == 0) {  // the last column is in no end node's band
      w.phase = kFailed;
      w.status = kPoaBandHit | (li << 8) | (9u << 24);
      w.act = 0;
    }
  }
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[1], sv::clock() - t0);
}

// phase C: the traceback
template <class K>
__host__ __device__ inline void poa4_phase_tb(const Poa4Args& A, const Poa4Ctx& C, Poa4LdsTb& S, u32 wave) {
  const int lane = sv::lane();
  const int q = lane / K::GS;
  const unsigned long long t0 = sv::clock();
  const u32 my_rec = poa4_my_record(C, wave, q);
  u32 act = 0, r_lo = 0, n_rows = 0, full = 0, len = 0, best = 0, li = 0;
  if (my_rec != 0xFFFFFFFFu) {
    const Poa4Win& w = C.st[my_rec];
    act = (w.phase == kRunning && w.act) ? 1u : 0u;
    r_lo = w.r_lo;
    n_rows = w.n_rows;
    full = w.full;
    len = w.len;
    best = w.best_rho1;
    li = w.li;
  }
  if (!sv::any(act != 0)) return;
  u32 bad = 0, band_hit = 0;
  poa4_traceback<K>(A, S, poa4_slot_of(A, C, wave, q), act != 0, r_lo, n_rows, full != 0, len, best, bad, band_hit);
  if (act && (bad || band_hit) && (lane & (K::GS - 1)) == 0) {
    Poa4Win& w = C.st[my_rec];
    w.phase = kFailed;
    w.status = (bad ? bad : kPoaBandHit) | (li << 8) | ((bad ? 11u : 10u) << 24);
    w.act = 0;
  }
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[2], sv::clock() - t0);
}

// phase D: the graph update, one window per wave
constexpr int kUpdPer = 2;  // sequence positions per lane and iteration of the graph update (4: 117 registers instead of 80 in a
                            // kernel of its own; inside the persistent kernel's 128 registers the two-position form is faster)
struct alignas(16) Poa4LdsUpd {
  u16 nslot[kPoa2MaxSeq + 16];  // order slots of the layer's new nodes
  u32 seq2[64];                 // the layer, 2 bits per base
};
template <int UP>
__host__ __device__ inline void poa4_phase_update(const Poa4Args& A, const Poa4Ctx& C, Poa4LdsUpd& S, u32 rec) {
  const int lane = sv::lane();
  const u32 wave_dp = rec / P4::G;
  const int q = static_cast<int>(rec % P4::G);
  if (poa4_my_record(C, wave_dp, q) == 0xFFFFFFFFu) return;
  Poa4Win me = C.st[rec];
  if (me.phase != kRunning) return;
  const bool act = me.act != 0;
  unsigned char* const my_slot = poa4_slot_of(A, C, wave_dp, q);
  if (act && lane < 60) S.seq2[lane] = poa4_carve(my_slot, A.nmax, A.lmax).seq2g[lane];  // the layer's packed codes back into LDS
  lds_order();
  unsigned long long t_add = 0, t_ord = 0;
  u32 nn = me.nn;
  bool flip = me.flip != 0;
  const PoaLayer* Lp = A.layers;
  if (act) Lp = A.layers + A.windows[me.wi].layer_first + me.li;
  const u32 why = poa4_update_graph<64, UP>(A, S.nslot, S.seq2, my_slot, act, Lp, me.len, me.lb, nn, flip, t_add, t_ord);
  if (lane == 0) {
    if (act && why) {
      me.phase = kFailed;
      me.status = why;
    } else if (act) {
      me.nn = nn;
      me.flip = flip ? 1u : 0u;
    }
    me.li = me.li + 1;
    me.act = 0;
    C.st[rec] = me;
  }
  if (A.phase_cycles && lane == 0) {
    sv::atomic_add(&A.phase_cycles[3], t_add);
    sv::atomic_add(&A.phase_cycles[4], t_ord);
  }
}

// last phase: consensus (or the backbone of a window that failed), status
__host__ __device__ inline void poa4_phase_final(const Poa4Args& A, const Poa4Ctx& C, Poa4Lds& S, u32 wave) {
  const int lane = sv::lane();
  const unsigned long long t0 = sv::clock();
  for (int q2 = 0; q2 < P4::G; ++q2) {
    const u32 rec = poa4_my_record(C, wave, q2);
    if (rec == 0xFFFFFFFFu) continue;
    const Poa4Win w = C.st[rec];
    if (w.phase == kHandedOn) continue;  // (result and status: the wave that takes the window off the queue)
    PoaWindow wq = A.windows[w.wi];
    u32 st = w.status;
    if (w.phase == kFailed || w.phase == kRunning) {  // (still running: the host stopped the rounds early — never)
      poa4_copy_backbone(A, wq, A.layers[wq.layer_first], A.out + wq.out_off, A.out_len + w.wi);
      if (w.phase == kRunning) st = 5;
    } else if (w.phase == kLayersDone) {
      Poa2Slot g = poa4_graph(poa4_slot_of(A, C, wave, q2), A.nmax, A.lmax, w.flip != 0);
      wq.n_layers = w.n_eff;
      poa4_consensus(g, poa4_carve(poa4_slot_of(A, C, wave, q2), A.nmax, A.lmax).rb, w.nn, A.nmax, wq, A.trim, S, A.out + wq.out_off,
                     A.out_len + w.wi);
      sv::sync();
      st = 1;
    }
    if (lane == 0) {
      A.status[w.wi] = st;
      if (A.phase_cycles) {
        sv::atomic_add(&A.phase_cycles[6], static_cast<unsigned long long>(w.cells_full));
        sv::atomic_add(&A.phase_cycles[7], static_cast<unsigned long long>(w.cells_band));
      }
    }
  }
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[5], sv::clock() - t0);
}

// ---- the two sides of a layer ----------------------------------------------------------------------------------------------
// Phases of the same SHAPE follow each other directly: the graph side (one window on the wave's 64 lanes: update with the
// previous alignment -> the next layer's set-up -> its row descriptors) and the alignment side (the wave's four windows
// side by side: NW -> traceback).  Between two phases the wave's stores are ordered at workgroup scope (sv::phase_fence):
// the next phase reads what this wave just wrote, through the CU's own L1 / the XCD's L2.
struct alignas(16) Poa4LdsGraph {
  union {
    Poa4LdsUpd upd;
    Poa4LdsDesc desc;
  } u;
};
template <class K, int UP>
__host__ __device__ inline void poa4_phase_graph(const Poa4Args& A, const Poa4Ctx& C, Poa4LdsGraph& S, u32 rec) {
  const u32 wave_dp = rec / P4::G;
  const int q = static_cast<int>(rec % P4::G);
  if (poa4_my_record(C, wave_dp, q) == 0xFFFFFFFFu) return;
  {
    const Poa4Win me = C.st[rec];
    sv::sync();  // (every lane has the record as the previous round left it before any phase below rewrites it)
    if (me.phase != kRunning) return;
    if (me.act) {  // the layer aligned in the previous round goes into the graph
      poa4_phase_update<UP>(A, C, S.u.upd, rec);
      sv::phase_fence();
    }
  }
  poa4_phase_setup<K>(A, C, S.u.desc, rec);
  sv::phase_fence();
  poa4_phase_desc_onewave<K>(A, C, S.u.desc, rec);
}
struct alignas(16) Poa4LdsNw {
  union {
    Poa4Lds dp;
    Poa4LdsTb tb;
  } u;
};
template <class K, class SC>
__host__ __device__ inline void poa4_phase_nw(const Poa4Args& A, const Poa4Ctx& C, Poa4LdsNw& S, u32 wave) {
  poa4_phase_dp<K, SC>(A, C, S.u.dp, wave);
  sv::phase_fence();  // backpointer stream and the windows' records: written above, read below
  poa4_phase_tb<K>(A, C, S.u.tb, wave);
}

// ---- one launch for the whole batch: persistent waves (round 5) ------------------------------------------------------------
// Per-round launches (round 4: five phase kernels; first half of round 5: two) keep every window of a chunk in lock step: a
// round ends when its slowest wave ends, and the busy wave-cycles of a C4-like batch added up to ~55 % of the slots x time
// the launches occupied (tools/bench_poa.py phase counters; 918 / 841 ms per C4 round against 739 here).  Here a wave takes a GROUP of four windows (scheduling order = by decreasing layer count, so the four have
// about the same number of layers) from an atomic counter and carries it from the backbone graph to the consensus without
// waiting for anybody else: per layer the graph side of each of its windows in turn (all 64 lanes on one window), then
// the alignment side of the four side by side.  Scratch and state records belong to the WAVE (blockIdx), not to the
// windows: a launch of n resident waves needs 4 n slots whatever the batch size (~10 GB instead of 30 GB per chunk), no
// chunks, no layer histogram, no host round trip.
struct alignas(16) Poa4LdsAll {
  union {
    Poa4LdsGraph g;
    Poa4LdsNw n;
    Poa4Lds f;
    p2::Poa2Lds<1> w64;  // the 64-column window function (poa2_window.h), for a window taken off the queue
    p2::Poa2Lds<2> w128; // and the 128-column one behind it
  } u;
};
static_assert(sizeof(Poa4LdsAll) <= 10240, "sixteen waves per CU");

}  // namespace
}  // namespace rvn
#include "poa4_esc.h"
namespace rvn {
namespace {

template <class K, int UP, class SC>
__host__ __device__ inline void poa4_persistent(const Poa4Args& A, const Poa4Ctx& C0, Poa4LdsAll& S, u32 pw) {
  const int lane = sv::lane();
  const u32 n_quads = (C0.count + poa4_group_windows(C0) - 1) / poa4_group_windows(C0);
  for (;;) {
    if (A.esc) {  // windows handed on by anybody's first attempt since this wave last looked
      for (;;) {
        const u32 wi = poa4_esc_pop(A);
        if (wi == kEscEmpty) break;
        poa4_esc_window(S, pw, wi);
        sv::phase_fence();
      }
    }
    // (every lane takes part in the fetch — lane 0 adds one, the others nothing: see nwpath.hip on why not `if (lane == 0)`)
    u32 quad = sv::atomic_add(A.next, lane == 0 ? 1u : 0u);
    quad = static_cast<u32>(sv::rfl(static_cast<int>(quad)));
    if (quad >= n_quads) break;
    Poa4Ctx C = C0;
    C.quad_delta = quad - pw;  // (modulo 2^32: position = first + (pw + delta) * 4 + q)
    poa4_phase_init(A, C, pw);
    sv::phase_fence();
    for (;;) {
      for (int q = 0; q < P4::G; ++q) {
        poa4_phase_graph<K, UP>(A, C, S.u.g, pw * P4::G + static_cast<u32>(q));
        sv::phase_fence();
      }
      bool any_layer = false;
      for (int q = 0; q < P4::G; ++q) {
        const u32 rec = poa4_my_record(C, pw, q);
        if (rec != 0xFFFFFFFFu) {
          const Poa4Win& w = C.st[rec];
          any_layer = any_layer || (w.phase == kRunning && w.act != 0);
          // a window that just failed with a band hit (or beyond a limit of this kernel that the 64-column function does not have):
          // into the queue right away, the rest of the group goes on
          if (A.esc && w.phase == kFailed && (w.status & 0xFFu) == kPoaBandHit) {
            const bool queued = poa4_esc_push(A, w.wi);
            if (queued && lane == 0) C.st[rec].phase = kHandedOn;
          }
        }
      }
      sv::sync();  // (the records are read by every lane before the alignment side rewrites them)
      if (!any_layer) break;
      poa4_phase_nw<K, SC>(A, C, S.u.n, pw);
      sv::phase_fence();
    }
    poa4_phase_final(A, C, S.u.f, pw);
    sv::phase_fence();
  }
}

// ---- the kernel: one wave per workgroup, resident waves = the grid ---------------------------------------------------------
// (four waves per SIMD: 128 registers, 9.7 KB of LDS.  Measured at C4 on one box: three waves per SIMD with 168 registers
// 869 ms per round, four 766 ms, five — 96 registers, a 19-row score ring = 8 KB of LDS — 844 ms: profiles/r05_poa_occupancy.txt)
template <int UP, class SC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void poa4_persistent_kernel(const Poa4Args A, const Poa4Ctx C) {
  __shared__ Poa4LdsAll lds;
  poa4_persistent<P4, UP, SC>(A, C, lds, blockIdx.x);
}
__host__ __device__ inline bool poa4_racon_scores(const Poa4Args& A) {
  return A.m == Poa4ScoresRacon::m && A.n_ == Poa4ScoresRacon::n && A.gp == Poa4ScoresRacon::g;
}

Poa4Args args_of4(const PoaBatchDev& b, unsigned char* scratch, size_t slot_bytes) {
  Poa4Args A{};
  A.windows = b.wins;
  A.n_windows = b.n_windows;
  A.layers = b.layers;
  A.src = b.src;
  A.scratch = scratch;
  A.slot_bytes = slot_bytes;
  A.nmax = b.nmax;
  A.lmax = b.lmax;
  A.m = b.m;
  A.n_ = b.n;
  A.gp = b.g;
  A.trim = b.trim;
  A.out = b.out;
  A.out_len = b.out_len;
  A.status = b.status;
  A.phase_cycles = b.phase_cycles;
  A.sched = b.sched;
  A.next = b.next;
  A.esc = nullptr;
  A.esc_cap = 0;
  A.esc_wide = 0;
  return A;
}

}  // namespace

// One launch, persistent waves (poa4_persistent).  Resident waves = 16 per CU (four per SIMD); fewer when the batch is
// small or the scratch does not fit.
void poa_v4_launch(Engine& e, const PoaBatchDev& b) {
  if (b.n_windows == 0) return;
  const size_t slot_bytes = poa4_slot_bytes(b.nmax, b.lmax);
  int dev = 0, cus = 256;
  RVN_HIP(hipGetDevice(&dev));
  RVN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  // windows per group: four, or two for a batch that leaves more than half of the wave slots empty even then (measured on
  // tools/small_batch_survey.sh: 2 500 windows 28.3 -> 24.6 ms, 5 000 windows 32.0 -> 29.9 ms; one per group is no better
  // than two, three no better than four at 10 000)
  u32 gw = b.n_windows > 2u * static_cast<u32>(cus) * 16u ? static_cast<u32>(P4::G) : 2u;
  if (const char* ev = knob("RVN_POA_GW")) gw = std::min<u32>(P4::G, std::max(1, std::atoi(ev)));  // (debug builds: A/B)
  const u32 n_quads = (b.n_windows + gw - 1) / gw;
  size_t free_b = 0, total_b = 0;
  RVN_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t per_wave = P4::G * (slot_bytes + sizeof(Poa4Win));
  // (a buffer handed back to the block pool at a stage entry is still there for the taking)
  const size_t budget = std::max(e.poa.scratch2.cap, devpool::free_largest()) + free_b / 2;
  u32 n_waves = std::min<u32>(n_quads, static_cast<u32>(cus) * 16u);
  if (static_cast<size_t>(n_waves) * per_wave + 1024 > budget) n_waves = static_cast<u32>(std::max<size_t>(1, (budget - 1024) / per_wave));
  const size_t slots = static_cast<size_t>(n_waves) * P4::G;
  unsigned char* d_scratch = e.poa.scratch2.get<unsigned char>(slots * (slot_bytes + sizeof(Poa4Win)) + 512);
  Poa4Win* d_st = reinterpret_cast<Poa4Win*>(d_scratch + slots * slot_bytes + 256);
  Poa4Args A = args_of4(b, d_scratch, slot_bytes);
  if (b.esc && poa2_slot_bytes(b.nmax, b.lmax, 64) <= P4::G * slot_bytes) {  // (the wave's four slots as the 64-column function's one)
    A.esc = b.esc;
    A.esc_cap = b.esc_cap;
    A.esc_wide = poa2_slot_bytes(b.nmax, b.lmax, 128) <= P4::G * slot_bytes ? 1u : 0u;
  }
  hipStream_t s = e.stream;
  RVN_HIP(hipMemsetAsync(b.next, 0, 4, s));
  const Poa4Ctx C{d_st, 0, b.n_windows, 0, gw};
  // (two sequence positions per lane and turn of the graph update: the kernel's 128 registers hold it without the spills the
  // four-position variant brings — 739 against 829 ms per C4 round)
  if (poa4_racon_scores(A)) {
    RVN_KLAUNCH_ON(kKPoaRows, s, (poa4_persistent_kernel<kUpdPer, Poa4ScoresRacon><<<n_waves, 64, 0, s>>>(A, C)));
  } else {
    RVN_KLAUNCH_ON(kKPoaRows, s, (poa4_persistent_kernel<kUpdPer, Poa4ScoresAny><<<n_waves, 64, 0, s>>>(A, C)));
  }
}

#ifdef RVN_TEST_HOOKS
// The same phase functions on the host, wave by wave under the wavefront emulator (simt_emu): windows / layers /
// sources are host arrays.  TEST INFRASTRUCTURE (rvn_poa_banded_emulate); first attempt only — a window that needs a
// wider band comes back flagged.
namespace {
struct EmuCall4 {
  const Poa4Args* A;
  const Poa4Ctx* C;
  Poa4Lds* S;
  Poa4LdsGraph* SG;
  Poa4LdsNw* SN;
  Poa4LdsAll* SA;
  u32 wave;
  int phase;
};
void emu_entry4(void* p) {
  EmuCall4* c = static_cast<EmuCall4*>(p);
  switch (c->phase) {
    case 0: poa4_phase_init(*c->A, *c->C, c->wave); break;
    case 1: poa4_phase_graph<P4, kUpdPer>(*c->A, *c->C, *c->SG, c->wave); break;
    case 2:
      if (poa4_racon_scores(*c->A)) poa4_phase_nw<P4, Poa4ScoresRacon>(*c->A, *c->C, *c->SN, c->wave);
      else poa4_phase_nw<P4, Poa4ScoresAny>(*c->A, *c->C, *c->SN, c->wave);
      break;
    case 9:
      if (poa4_racon_scores(*c->A)) poa4_persistent<P4, kUpdPer, Poa4ScoresRacon>(*c->A, *c->C, *c->SA, c->wave);
      else poa4_persistent<P4, kUpdPer, Poa4ScoresAny>(*c->A, *c->C, *c->SA, c->wave);
      break;
    default: poa4_phase_final(*c->A, *c->C, *c->S, c->wave); break;
  }
}
}  // namespace

void poa_v4_emulate(const std::vector<PoaWindow>& wins, const std::vector<PoaLayer>& lays, const PoaSrc& src, u32 max_bb,
                    u32 max_len, int m, int n, int g, int trim, u8* out, u32* out_len, u32* status, bool persistent) {
  if (wins.empty()) return;
  PoaBatchDev b{};
  b.lmax = std::min<u32>(kPoaMaxSeq, std::max<u32>(64, ((max_len + 63) / 64) * 64));
  b.nmax = std::min<u32>(8192, std::max<u32>(512, max_bb * 6));
  const size_t slot_bytes = poa4_slot_bytes(b.nmax, b.lmax);
  const u32 count = static_cast<u32>(wins.size());
  const u32 n_waves = (count + P4::G - 1) / P4::G;
  std::vector<unsigned char> scratch(slot_bytes * std::max<u32>(n_waves, 2) * P4::G + 256, 0);
  std::vector<Poa4Win> st(static_cast<size_t>(std::max<u32>(n_waves, 2)) * P4::G);
  unsigned long long phase[16] = {};
  u32 next = 0;
  b.wins = wins.data();
  b.n_windows = count;
  b.layers = lays.data();
  b.src = src;
  b.m = m;
  b.n = n;
  b.g = g;
  b.trim = trim;
  b.out = out;
  b.out_len = out_len;
  b.status = status;
  b.phase_cycles = phase;
  b.sched = nullptr;
  b.next = &next;
  const Poa4Args A = args_of4(b, scratch.data(), slot_bytes);
  const Poa4Ctx C{st.data(), 0, count, 0};
  std::vector<Poa4Lds> lds(1);
  std::vector<Poa4LdsGraph> ldsg(1);
  std::vector<Poa4LdsNw> ldsn(1);
  if (persistent) {
    // two "resident" waves; the emulator runs a wave to its end, so wave 1 (started first) takes every group of windows —
    // with a group index below AND above its own — and wave 0 finds the counter exhausted
    std::vector<Poa4LdsAll> ldsa(1);
    const Poa4Ctx CP{st.data(), 0, count, 0};
    for (u32 pw : {1u, 0u}) {
      std::memset(static_cast<void*>(ldsa.data()), 0, sizeof(Poa4LdsAll));
      EmuCall4 call{&A, &CP, lds.data(), ldsg.data(), ldsn.data(), ldsa.data(), pw, 9};
      simt_emu::run_wave(&emu_entry4, &call);
    }
    return;
  }
  u32 max_layers = 0;
  for (const PoaWindow& w : wins) max_layers = std::max(max_layers, w.n_layers);
  auto run = [&](int ph) {
    const u32 waves = ph == 1 ? n_waves * P4::G : n_waves;
    for (u32 wv = 0; wv < waves; ++wv) {
      if (ph == 1 && (wv >= count || st[wv].phase != kRunning)) continue;  // (waves that would return at once: not worth 64 fibres each)
      std::memset(static_cast<void*>(lds.data()), 0, sizeof(Poa4Lds));  // (a fresh workgroup's LDS holds anything: zeros here)
      std::memset(static_cast<void*>(ldsg.data()), 0, sizeof(Poa4LdsGraph));
      std::memset(static_cast<void*>(ldsn.data()), 0, sizeof(Poa4LdsNw));
      EmuCall4 call{&A, &C, lds.data(), ldsg.data(), ldsn.data(), nullptr, wv, ph};
      simt_emu::run_wave(&emu_entry4, &call);
    }
  };
  run(0);
  for (u32 round = 1; round <= max_layers; ++round) {  // as poa_v4_launch: graph side, then (while layers remain) the alignment side
    run(1);
    if (round < max_layers) run(2);
  }
  run(5);
}

#endif  // RVN_TEST_HOOKS

}  // namespace rvn
