// poa4_nw.h — banded NW of one layer per window, rows on lanes (the schedule: poa4.hip).
#pragma once
#include "poa4_ops.h"
namespace rvn {
namespace {
// Outputs (group-uniform): best_rho1 = 1 + row (rho) of the end node with the best score in the last column, 0: the last
// column is in no end node's band.
//
// The step (round 6).  Counters of round 5 (SQ_* count quad-cycles: 33 G VALU instructions against ~44-51 G SIMD quad-cycles of
// the launch) say the kernel keeps the vector ALUs busy 65-75 % of the time at four waves per SIMD: a wave's step does not
// wait for LDS, it waits for the other waves' instructions — so the step is priced in instructions, and round 5's ~88
// vector instructions for 2 x 64 cells are now ~50:
//   * the lane's row descriptor is read from LDS a step ahead (Poa4Lds::qa / qm); the end of a row flips a pointer (rounds 4-5:
//     ~28 instructions under a lane mask in 98 % of the steps: seven register copies, the end-node test, the schedule test);
//   * keys are score << 8 | tag: both cells return to a packed pair of int16 with one v_perm_b32;
//   * the horizontal chain stays in the key domain (tag 0 = "horizontal"): a cell is max3(diagonal, vertical, horizontal) and
//     its backpointer code the key's low nibble — no score / code selects;
//   * the step's column pair comes from the step counter and a per-row constant ((qm + 8 t) & 0x78), the row's own step number
//     (k) is only compared; the match bits of the step are two sign-extending bit-field extracts;
//   * the end-node score is looked at by the service point after the row's last pair has been stored, the schedule is
//     checked where descriptors are fetched (consecutive rows of a lane start >= 17 steps apart): neither in the step.
// The scores of the NW: racon's defaults as raven::Polish passes them (m = 3, n = -5, g = -4: RavenLib/include/raven/graph/
// polish.hpp:13-17) are literals of a specialised instance — the persistent kernel keeps ~100 scalar registers live across the
// NW, and round 5's step fetched its score constants out of spilled scalar registers (v_readlane) every time; any other
// scores take the instance that reads them from the batch.
struct Poa4ScoresAny {
  i32 m, n, g;
  __host__ __device__ explicit Poa4ScoresAny(const Poa4Args& A) : m(A.m), n(A.n_), g(A.gp) {}
};
struct Poa4ScoresRacon {
  static constexpr i32 m = 3, n = -5, g = -4;
  __host__ __device__ explicit Poa4ScoresRacon(const Poa4Args&) {}
};
template <class K, class SC>
__host__ __device__ inline void poa4_dp(const Poa4Args A, Poa4Lds& S, unsigned char* slot_mem, bool act, u32 t_end, u32 len,
                                        u32& best_rho1) {
  P4_ASSUME_GLOBAL(slot_mem);
  P4_ASSUME_LDS(&S);
  const int lane = sv::lane();
  const int gl = lane & 15, q = lane >> 4;
  const Poa4Slot sl = poa4_carve(slot_mem, A.nmax, A.lmax);
  // the rings start as -inf (the union is reused by the layer set-up and by the traceback), the wave's -inf cells
  {
    const u32 neg = pack16(kNegInf16, kNegInf16);
    for (int idx = gl; idx < K::kRing * kRowW4; idx += 16) lds_st32(S, poa4_ring_byte(q, static_cast<u32>(idx)), neg);
    if (lane < 40) S.neg[lane] = neg;
    ring_fill_knob<K>(S, gl, q, len);
  }
  const SC sc(A);
  const i32 xD = sc.n * 256 + 8, dD = (sc.m - sc.n) * 256, gK = sc.g * 256;  // keys = score * 256 + tag; the diagonal's tag bit rides on the score term
  const i32 gp = sc.g;
  const u32 neg_off = poa4_neg_byte(q);
  const u32 neg2 = neg_off | (neg_off << 16);
  const u32 negpair = pack16(kNegInf16, kNegInf16);
  // a descriptor as the desc pass left it (2 x 16 bytes) into one of the lane's two slots; `on` = false: a row that never starts
  // (l16 = 16 x lane: the lane's place in a slot.  The loop derives it from its slot pointer where it parks: as three lane-derived
  // LDS addresses of their own (qa, qm / qc, qe) the compiler kept two in registers across the NW and one in scratch memory, reloaded
  // — behind a wait for everything outstanding — at every service point)
  auto park = [&](u32 l16, u32 par, uint4 da, uint4 db, bool on) __attribute__((always_inline)) {
    const u32 s2 = on ? (da.x & 0xFFFFu) : kInactiveS;
    const u32 c1 = on ? da.y : 0u;
    const u32 np = (c1 >> 26) & 15u;
    // bytes of the band's first column pair in a ring row, minus 8 S: the pair of step t is (this + 8 t) & 0x78
    const u32 r0 = (((c1 >> 14) & 0x78u) - 4u * s2) & 0x78u;
    const bool rare = on && s2 != kInactiveS && (np == 0u || np > 4u);
    unsigned char* const base = reinterpret_cast<unsigned char*>(&S);
    const u32 a16 = l16 + par * (64u * 16u);
    *reinterpret_cast<uint4*>(base + offsetof(Poa4Lds, qa) + a16) =
        uint4{on ? da.x : (kInactiveS | (neg_off << 16)), on ? da.w : neg2, on ? db.x : neg2, db.w};
    *reinterpret_cast<u32*>(base + offsetof(Poa4Lds, qm) + (a16 >> 2)) = r0 | ((c1 >> 31) << 8) | (np << 24) | (rare ? 0x80000000u : 0u);
    *reinterpret_cast<uint2*>(base + offsetof(Poa4Lds, qe) + (a16 >> 1)) = uint2{on ? db.y : neg2, on ? db.z : neg2};
    *reinterpret_cast<u32*>(base + offsetof(Poa4Lds, qc) + (a16 >> 2)) = c1;
  };
  bool sched_bad = false;
  u32 ld_rho = static_cast<u32>(gl) + 16u;  // the last row whose descriptor went to LDS
  u32 ld_s2;                                // its 2 S
  {
    const uint4 a = sl.desc[2 * static_cast<size_t>(gl)], b = sl.desc[2 * static_cast<size_t>(gl) + 1];
    const uint4 a2 = sl.desc[2 * static_cast<size_t>(gl + 16)], b2 = sl.desc[2 * static_cast<size_t>(gl + 16) + 1];
    park(static_cast<u32>(lane) * 16u, 0, a, b, act);  // (a group without a layer in this round has no descriptors: it idles on -inf cells)
    park(static_cast<u32>(lane) * 16u, 1, a2, b2, act);
    const u32 s0 = act ? (a.x & 0xFFFFu) : kInactiveS;
    ld_s2 = act ? (a2.x & 0xFFFFu) : kInactiveS;
    // consecutive rows of a lane start at least 17 steps apart (band starts do not decrease along the order)
    if (act && s0 != kInactiveS && ld_s2 < s0 + 34u) sched_bad = true;
  }
  lds_order();
  // the lane's slot as bytes into qa (qm = bytes / 4, qe = bytes / 2); the words of the step to come
  u32 ptr = static_cast<u32>(offsetof(Poa4Lds, qa)) + static_cast<u32>(lane) * 16u;
  constexpr u32 kFlip = 64u * 16u;
  uint4 cw = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(&S) + ptr);
  u32 cm = lds_ld32(S, static_cast<u32>(offsetof(Poa4Lds, qm)) + (ptr >> 2));
  uint4 lA = uint4{0, 0, 0, 0}, lB = uint4{0, 0, 0, 0};
  bool ld_pending = false;
  i32 Am1 = 0, UK = kNegU;
  u32 v7m = 0;
  i32 best_score = -0x7FFFFFFF;
  u32 best_row = 0;
  const u32 T = static_cast<u32>(sv::wave_max(act ? static_cast<int>(t_end) : 0));
  // An end node's score in the layer's last column, looked at by the first service point after the row's last pair was
  // stored: the row's descriptor is still in the lane's other slot (the next fetch parks 8 steps after it was issued, and it
  // is issued here at the earliest), and its cells are still in the ring — the row kRing rows on, which takes the ring slot
  // over, stores its first pair >= kRing + 1 steps after this row stored its first, i.e. >= 8 steps after this row's last:
  // not before the step this service point precedes.
  static_assert(K::kRing >= 16 + K::kU - 2, "an end node's cells outlive the row by a service interval");
  auto end_check = [&](u32 t0) __attribute__((always_inline)) {
    const u32 optr = ptr ^ kFlip;
    const u32 px = lds_ld32(S, optr), pm = lds_ld32(S, static_cast<u32>(offsetof(Poa4Lds, qm)) + (optr >> 2));
    const i32 fin2 = static_cast<i32>(2u * t0) - static_cast<i32>(px & 0xFFFFu) - 30;  // 2 x steps since the row's last pair
    const bool hit = (pm & 0x100u) != 0 && fin2 >= 2 && fin2 <= 2 * K::kU;
    if (sv::any(hit)) {
      const u32 c1 = lds_ld32(S, static_cast<u32>(offsetof(Poa4Lds, qc)) + (optr >> 2));
      const i32 idx = static_cast<i32>(len) - static_cast<i32>((c1 >> 16) & 0x3FFu);
      if (hit && idx >= 0 && idx < K::kBand) {
        const u32 cb3 = (c1 >> 14) & 0x78u;
        const i32 sce = lds_ld16(S, (px >> 16) + ((cb3 + 8u * (static_cast<u32>(idx) >> 1)) & 0x78u) + 2u * (static_cast<u32>(idx) & 1u));
        const u32 rho = ((cw.x & 0xFFFFu) == ld_s2 ? ld_rho : ld_rho - 16u) - 16u;  // (the lane is at the last row parked, or at the one before)
        const u32 cand = ((c1 & 0xFFFFu) << 16) | (rho + 1u);  // node id | 1 + row: equal scores -> smallest node id
        if (sce > best_score || (sce == best_score && cand < best_row)) {
          best_score = sce;
          best_row = cand;
        }
      }
    }
  };
  u32 t0 = 0, accp0 = 0, accp1 = 0;
  uint2* bp = sl.bps + gl;  // where the backpointers of the eight steps before go: [step / 8][lane of the window]
#if defined(RVN_DEBUG_KNOBS)
  unsigned long long t_sp = 0;
#endif
  for (; t0 < T; t0 += K::kU) {
#if defined(RVN_DEBUG_KNOBS)
    const unsigned long long sp0 = sv::clock();
#endif
    end_check(t0);
    // ---- service point: the descriptor fetched 8 steps ago goes into the slot of the row the lane finished last; a lane
    // that has moved on to the last row it holds fetches the one after (needed 17 steps after that switch at the earliest:
    // fetched <= 8 steps after it, parked <= 16 steps after it).  The backpointers of the PREVIOUS eight steps leave here,
    // after the two: the only wait for vector memory in the loop that finds anything outstanding is the one in front of the
    // parking, and what it finds — the fetch and the store of the service point before — was issued eight steps ago.  (Rounds 4-5
    // stored at the end of the eight steps: the wait at the top of the next eight then sat behind a store issued a moment
    // ago, every time, for the length of a write to HBM.) ----
    await_v((lA.x | lA.y | lA.z) | (lA.w | lB.x | lB.y) | (lB.z | lB.w));  // (the loads of the service point before: waited for behind the branch below, it is behind the store issued a moment before)
    if (ld_pending) {
      const u32 rho = ld_rho + 16u;
      const u32 l16 = pin_v(ptr & (kFlip - 1u));  // (from the slot pointer, here: not a value kept since before the loop)
      park(l16, (rho >> 4) & 1u, lA, lB, true);
      const u32 s2 = lA.x & 0xFFFFu;
      if (ld_s2 != kInactiveS && s2 < ld_s2 + 34u) sched_bad = true;  // the row's first step would be over: band starts decreased along the order
      ld_s2 = s2;
      ld_rho = rho;
    }
    {
      // (every lane loads at every service point — those with nothing to fetch the wave's first descriptor, one request for all of
      // them: a load under a lane mask makes its registers a merge of two definitions around the loop, and the compiler then
      // shuffles — and waits for — the loaded registers right behind the load)
      const bool want = !ld_pending && act && ld_s2 != kInactiveS && (cw.x & 0xFFFFu) == ld_s2;  // (a lane's rows have increasing S: the row it is at IS the last one parked)
      const uint4* src = sl.desc + (want ? 2 * static_cast<size_t>(ld_rho + 16) : 0);
      lA = src[0];
      lB = src[1];
      ld_pending = want;
    }
    // (the store BEHIND the loads: the compiler re-waits for "everything" in front of the loads whatever was waited for above
    // — free when nothing is outstanding, the length of a write to HBM behind a store)
    if (act && t0 != 0) *bp = uint2{accp0, accp1};
#if defined(RVN_DEBUG_KNOBS)
    t_sp += sv::clock() - sp0;
#endif
    u32 acc0 = 0, acc1 = 0;
#pragma unroll
    for (int u = 0; u < K::kU; ++u) {
      P4_MARK("step_begin");
      const u32 t = t0 + static_cast<u32>(u);
      const i32 k2 = static_cast<i32>(2u * t) - static_cast<i32>(cw.x & 0xFFFFu);  // 2 k: -2 = the pair left of the band, 0 .. 30 the band
      // the step's column pair as a byte offset into ANY ring row (interleaved rings: a pair is 8 bytes on)
      const u32 off4 = (cm + 8u * t) & 0x78u;
      // ---- in-edges: one aligned pair of predecessor cells each (columns j, j + 1 of this step).  A row's unused in-edges
      // point at -inf cells: in-edges 1..3 are read whether the row has them or not, so the four reads are in flight together
      // (issuing them under the exec mask of the lanes that have the in-edge was measured in round 5: slower) ----
      u32 wd = lds_ld32(S, add_half<false>(off4, cw.y));
      const u32 w1 = lds_ld32(S, add_half<true>(off4, cw.y));
      const u32 w2 = lds_ld32(S, add_half<false>(off4, cw.z));
      const u32 w3 = lds_ld32(S, add_half<true>(off4, cw.z));
      // ---- the words of the next step: the same row's, or — after the row's last pair — the other slot's ----
      const u32 nptr = k2 == 30 ? ptr ^ kFlip : ptr;
      const uint4 nw = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(&S) + nptr);
      const u32 nm = lds_ld32(S, static_cast<u32>(offsetof(Poa4Lds, qm)) + (nptr >> 2));
      i32 A0, A1;
      bool wave_has8 = false;  // (wave-uniform: some lane's row has eight in-edges)
      if (sv::any(static_cast<i32>(cm) < 0)) {  // rows without an in-edge inside the subgraph, rows with more than four (1 % of the rows)
        P4_MARK("rare_begin");
        const uint2 ce = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(&S) + offsetof(Poa4Lds, qe) + (ptr >> 1));
        const u32 np = (cm >> 24) & 15u;
        if (sv::any(np == 0)) {  // the virtual start row H[0][j] = j * g
          const u32 c1 = lds_ld32(S, static_cast<u32>(offsetof(Poa4Lds, qc)) + (ptr >> 2));
          const i32 j0 = static_cast<i32>((c1 >> 16) & 0x3FFu) + k2;
          u32 vp = pack16(j0 * gp, (j0 + 1) * gp);
          if (j0 < 0) vp = negpair;
          wd = np == 0 ? vp : wd;
        }
        A0 = cell_key<false, 7>(wd);
        A1 = cell_key<true, 7>(wd);
#define P4_EDGE(E, REG, HI)                                        \
  {                                                                \
    const u32 we = lds_ld32(S, add_half<HI>(off4, REG));           \
    A0 = imax(A0, cell_key<false, 7 - E>(we));                     \
    A1 = imax(A1, cell_key<true, 7 - E>(we));                      \
  }
        if (sv::any(np > 4)) {
          P4_EDGE(4, ce.x, false)
          if (sv::any(np > 5)) {
            P4_EDGE(5, ce.x, true)
            if (sv::any(np > 6)) {
              P4_EDGE(6, ce.y, false)
              P4_EDGE(7, ce.y, true)
              wave_has8 = sv::any(np > 7);
            }
          }
        }
#undef P4_EDGE
        P4_MARK("rare_end");
      } else {
        A0 = cell_key<false, 7>(wd);
        A1 = cell_key<true, 7>(wd);
      }
      A0 = imax3(A0, cell_key<false, 6>(w1), cell_key<false, 5>(w2));
      A1 = imax3(A1, cell_key<true, 6>(w1), cell_key<true, 5>(w2));
      A0 = imax(A0, cell_key<false, 4>(w3));
      A1 = imax(A1, cell_key<true, 4>(w3));
      // ---- the two cells: spoa's priority diagonal (first in-edge reaching the maximum), vertical, horizontal — the order of
      // the tags (8 | 7 - e, 7 - e, 0); equal keys are "vertical through the eighth in-edge" and "horizontal": code 0 for both ----
      const u32 cs = cw.w >> (static_cast<u32>(k2) & 31u);
      const i32 m0 = static_cast<i32>(cs << 31) >> 31, m1 = static_cast<i32>(cs << 30) >> 31;  // -1: the row's base matches the column's
      i32 M0 = imax3(Am1 + xD + (m0 & dD), A0 + gK, UK + gK);
      const i32 U0K = M0 & ~0xFF;
      i32 M1 = imax3(A0 + xD + (m1 & dD), A1 + gK, U0K + gK);
      const bool in_band = k2 >= 0;
      if (in_band) lds_st32(S, add_half<true>(off4, cw.x), clamp_pair(keys_to_pair(M0, M1)));
      UK = in_band ? (M1 & ~0xFF) : kNegU;
      if (wave_has8) {
        // A row of eight in-edges (a tenth of the 2.5 % of C4-like windows that have one): "vertical through the eighth" has
        // tag 0, the code of "horizontal".  Which of the two a code 0 of such a row means goes into a 32-bit mask beside the
        // row, one bit per column (round 5 handed the window to the 64-column kernel when a walk met the case: 836 windows and
        // 59 ms of a second kernel per C4 round).  The vertical candidate wins a tie with the horizontal one (max3's key
        // order), and a diagonal of the same score would have left a tag >= 8.
        P4_MARK("rare_begin");
        const u32 npc = (cm >> 24) & 15u;
        const bool has8 = npc > 7u;
        u32 b0 = (in_band && (M0 & 0xFF) == 0 && M0 == A0 + gK) ? 1u : 0u;
        u32 b1 = (in_band && (M1 & 0xFF) == 0 && M1 == A1 + gK) ? 1u : 0u;
        if (sv::any(npc > 8u)) {
          // A row of 9..15 in-edges (241 of the 244 windows a C4 round of round 6 still handed to the 64-column kernel had one:
          // a launch of 38 ms behind the persistent kernel for a thousandth of the windows).  In-edges 7..14 are a second group
          // with tags of their own (7 - (e - 7)): their cells of this step's pair and of the pair before come out of the ring here
          // (addresses: the row's overflow record, a global load — on this path only), the group's two cells are folded like the
          // first group's, and a cell takes the second group's key where that one is better by spoa's order — higher score, then
          // diagonal before vertical before horizontal; the first group has the earlier in-edges and keeps a tie inside a class.
          // The row's mask (v7: such a row keeps no eighth in-edge in its descriptor, code 0 is "horizontal") says per column which
          // group the code counts in.  The cells were stored above with the first group's values: stored again here, same lane,
          // before any other lane reads them (a step later at the earliest).
          const bool has9 = npc > 8u;
          const u32 rho_c = (cw.x & 0xFFFFu) == ld_s2 ? ld_rho : ld_rho - 16u;
          // (a loop that is NOT unrolled, one in-edge per turn, its ring bytes fetched as the 16 bits they are: this path runs
          // for one row in ~1 000 windows and must not cost the step's common path a register — unrolled over the record's four
          // words it pushed the descriptor pointer of the service point into scratch memory: two reloads and two waits for
          // "everything outstanding" per eight steps, +35 % on the whole NW)
          const u16* const ovp = reinterpret_cast<const u16*>(reinterpret_cast<const unsigned char*>(sl.v7) + poa4_v7_bytes(A.nmax)) +
                                 8u * static_cast<size_t>(has9 ? rho_c : 0u);
          const u32 offp = (off4 - 8u) & 0x78u;
          i32 B0 = kNegU, B1 = kNegU, Bm1 = kNegU;
          P4_NO_UNROLL
          for (i32 e = 0; e < 8; ++e) {
            const u32 rb = has9 ? static_cast<u32>(ovp[e]) : neg_off;
            const u32 wc = lds_ld32(S, rb + off4), wp = lds_ld32(S, rb + offp);
            const i32 tag = 7 - e;
            B0 = imax(B0, sext16(wc) * 256 + tag);
            B1 = imax(B1, sext16(wc >> 16) * 256 + tag);
            Bm1 = imax(Bm1, sext16(wp >> 16) * 256 + tag);
          }
          // class of a key: 2 diagonal, 1 vertical, 0 horizontal (first group: tag 0 — its vertical tags are 7..1 in such a row)
          auto better = [](i32 kb, i32 ka) -> bool {
            const i32 ca = (ka & 8) ? 2 : ((ka & 7) ? 1 : 0), cb = (kb & 8) ? 2 : 1;
            return ((kb & ~0xFF) | cb) > ((ka & ~0xFF) | ca);
          };
          const i32 N0 = imax(Bm1 + xD + (m0 & dD), B0 + gK);
          const bool t0b = has9 && better(N0, M0);
          const i32 M0n = t0b ? N0 : M0;
          const i32 M1a = imax3(A0 + xD + (m1 & dD), A1 + gK, (M0n & ~0xFF) + gK);
          const i32 N1 = imax(B0 + xD + (m1 & dD), B1 + gK);
          const bool t1b = has9 && better(N1, M1a);
          const i32 M1n = t1b ? N1 : M1a;
          if (has9) {
            M0 = M0n;
            M1 = M1n;
            if (in_band) lds_st32(S, add_half<true>(off4, cw.x), clamp_pair(keys_to_pair(M0, M1)));
            UK = in_band ? (M1 & ~0xFF) : kNegU;
            b0 = (in_band && t0b) ? 1u : 0u;
            b1 = (in_band && t1b) ? 1u : 0u;
          }
        }
        v7m = (k2 <= 0 ? 0u : v7m) | ((b0 | (b1 << 1)) << (static_cast<u32>(k2) & 31u));
        if (has8 && k2 == 30) sl.v7[(cw.x & 0xFFFFu) == ld_s2 ? ld_rho : ld_rho - 16u] = v7m;
        P4_MARK("rare_end");
      }
      Am1 = A1;
      // (byte 0: code of the pair; the rest is dropped by put_byte)
      const u32 cp = pin_v((static_cast<u32>(M0) & 15u) | (static_cast<u32>(M1) << 4));  // computed here: sunk to the store it would keep the step's two keys alive for eight steps
      if (u == 0) acc0 = put_byte<0>(acc0, cp);
      else if (u == 1) acc0 = put_byte<1>(acc0, cp);
      else if (u == 2) acc0 = put_byte<2>(acc0, cp);
      else if (u == 3) acc0 = put_byte<3>(acc0, cp);
      else if (u == 4) acc1 = put_byte<0>(acc1, cp);
      else if (u == 5) acc1 = put_byte<1>(acc1, cp);
      else if (u == 6) acc1 = put_byte<2>(acc1, cp);
      else acc1 = put_byte<3>(acc1, cp);
      lds_order();
      ptr = nptr;
      cw = nw;
      cm = nm;
      P4_MARK("step_end");
    }
    hold_v(accp0, accp1, bp);  // (the backpointer store of this turn's service point)
    accp0 = acc0;
    accp1 = acc1;
    if (t0 != 0) bp += 16;
  }
  if (act && t0 != 0) *bp = uint2{accp0, accp1};
  end_check(t0);  // rows that finished in the loop's last steps
#if defined(RVN_DEBUG_KNOBS)
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[9], t_sp);
#endif
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[14], static_cast<unsigned long long>((T + K::kU - 1) / K::kU * K::kU));
  // among the end nodes with the best score the one with the SMALLEST NODE ID (a rule that does not depend on the order of
  // the rows: spoa takes the first in ITS rank order, which is not the device's), as poa2 / poa pick it
  {
    const i32 gs = group_max_i(best_score);
    const u32 cand = (best_score == gs && best_row != 0) ? best_row : 0xFFFFFFFFu;
    const u32 br = group_min_u(cand);
    best_rho1 = (act && br != 0xFFFFFFFFu) ? (br & 0xFFFFu) : 0u;
    if (sv::any(sched_bad)) {
      const u32 any_bad = static_cast<u32>(sv::ballot(sched_bad) >> (lane & ~15)) & 0xFFFFu;
      if (any_bad) best_rho1 = 0;  // (reported as a band miss: the 64-column kernel takes the window)
    }
  }
}
}  // namespace
}  // namespace rvn
