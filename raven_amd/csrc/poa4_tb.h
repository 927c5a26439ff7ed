// poa4_tb.h — traceback of the wave's windows through the NW's backpointer stream, round-synchronous.
#pragma once
#include "poa4_ops.h"
namespace rvn {
namespace {
// k-th in-edge (among those inside the subgraph) of v as a rank
__host__ __device__ inline u32 poa4_nth_pred_rank(const Poa4Slot& sl, u32 v, u32 k, bool full) {
  const Poa2Slot& g = sl.g;
  const u32 c = g.in_cnt[v];
  u32 seen = 0;
  for (u32 i = 0; i < c; ++i) {
    const u32 t = g.in_tail[v * kPoaMaxIn + i];
    if (full || g.mark[t]) {
      if (seen == k) return sl.rb[t] & 0xFFFFu;
      ++seen;
    }
  }
  return 0;
}

// A round = every window walks through kTbG blocks of 16 rows.  Lane l of a window fetches rows 16 * block + l of the
// round — three descriptor words and the 24 bytes of the backpointer stream that hold the row's 32 four-bit codes (its 16
// steps lie in at most three 8-step blocks of the stream) — a round AHEAD into registers, descriptors two rounds ahead (the
// codes' addresses come out of them), and parks them in the window's LDS when the round begins.  The walk itself is the
// same for all 16 lanes of a window (every lane reads the same two LDS addresses per step: the current row's descriptor,
// then the code under column j): no cross-lane traffic, no select trees.  All four windows change rounds at the same
// point of the loop, so the wait there is for loads issued a round ago, not for another window's prefetch of a moment
// ago (the memory counter is the wave's, not the window's).
constexpr int kTbG = 2;
struct alignas(16) Poa4LdsTb {
  // per row of the round: the 16 code bytes of its 32 columns ALIGNED TO THE COLUMN (byte (j >> 1) & 15 holds the codes of
  // columns j, j + 1: where the code of (row, j) lies does not depend on the row's band start, so the walk reads it beside
  // the row's record, not behind it), then {band start | edge flags | in-edges, node, rank distances of in-edges 0..5, -}
  uint4 row[P4::G][16 * kTbG][2];
};
// the 16 code bytes of a row (its steps 0 .. 15 start at byte S % 8 of the 24 the lane fetched) rotated so that the byte of
// columns (j, j + 1) sits at index (j >> 1) & 15; bt = the row's (even) band start
__host__ __device__ __forceinline__ uint4 poa4_align_codes(u32 c0, u32 c1, u32 c2, u32 c3, u32 c4, u32 c5, u32 S, u32 bt) {
  const u32 sb = S & 7u;
  const bool hi = sb >= 4u;
  const u32 w0 = hi ? c1 : c0, w1 = hi ? c2 : c1, w2 = hi ? c3 : c2, w3 = hi ? c4 : c3, w4 = hi ? c5 : c4;
  const u32 sh = 8u * (sb & 3u);
  const u32 b0 = funnel_shr(w1, w0, sh), b1 = funnel_shr(w2, w1, sh), b2 = funnel_shr(w3, w2, sh), b3 = funnel_shr(w4, w3, sh);
  // rotate the 128-bit ring left by r bytes: byte k goes to (k + r) & 15
  const u32 r = (bt >> 1) & 15u, rw = r >> 2, rs = 8u * (r & 3u);
  const u32 o0 = rw == 0 ? b0 : (rw == 1 ? b3 : (rw == 2 ? b2 : b1));
  const u32 o1 = rw == 0 ? b1 : (rw == 1 ? b0 : (rw == 2 ? b3 : b2));
  const u32 o2 = rw == 0 ? b2 : (rw == 1 ? b1 : (rw == 2 ? b0 : b3));
  const u32 o3 = rw == 0 ? b3 : (rw == 1 ? b2 : (rw == 2 ? b1 : b0));
  if (rs == 0) return uint4{o0, o1, o2, o3};
  const u32 back = 32u - rs;
  return uint4{funnel_shr(o0, o3, back), funnel_shr(o1, o0, back), funnel_shr(o2, o1, back), funnel_shr(o3, o2, back)};
}
template <class K>
__host__ __device__ inline void poa4_traceback(const Poa4Args A, Poa4LdsTb& S, unsigned char* slot_mem, bool act, u32 r_lo,
                                               u32 n_rows, bool full, u32 len, u32 best_rho1, u32& bad, u32& band_hit) {
  P4_ASSUME_GLOBAL(slot_mem);
  P4_ASSUME_LDS(&S);
  (void)n_rows;
  const int lane = sv::lane();
  const int gl = lane & 15, q = lane >> 4;
  const Poa4Slot sl = poa4_carve(slot_mem, A.nmax, A.lmax);
  const uint4* const dsc = sl.desc;
  // (the backpointer stream's address is formed from the descriptors' where the codes are fetched, once per round of 32 rows: as a
  // pointer of its own it lived — with the descriptors' — in scratch memory across the walk, reloaded at every change of round)
  const size_t bps_off = static_cast<size_t>(poa4_desc_rows(A.nmax)) * 32 + 2 * ((static_cast<size_t>(A.nmax) * 4 + 255) & ~size_t(255));  // (poa4_carve)
  // (likewise the position -> node table: a scalar distance from the descriptors, the address formed where a block of sixteen leaves)
  const i32 pn_off = sv::rfl(static_cast<i32>(reinterpret_cast<const unsigned char*>(sl.g.pos_node) - reinterpret_cast<const unsigned char*>(sl.desc)));
  auto pos_node_at = [&](u32 idx) __attribute__((always_inline)) -> u16* {
    const i32 po = pin_s(pn_off);
    return reinterpret_cast<u16*>(const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(dsc)) + static_cast<ptrdiff_t>(po)) + idx;
  };
  const u32 w = len + 1;
  bad = 0;
  band_hit = 0;
  u32 i = act ? best_rho1 : 0;  // 1 + rho of the current row; 0 = the virtual start row
  i32 j = static_cast<i32>(w) - 1;
  bool done = !act || i == 0;
  u32 steps = 0, n_switch = 0;
  unsigned long long t_change = 0;
  u32 pbuf = kNone4, pblk = 0xFFFFFFFFu;  // the node of position 16 pblk + lane-of-the-window, for the block the walk is in
  // the next round (descriptors and codes in flight), the round after (descriptors in flight)
  u32 nd0[kTbG] = {}, nd1[kTbG] = {}, nd7[kTbG] = {}, fd0[kTbG] = {}, fd1[kTbG] = {}, fd7[kTbG] = {};
  // (native vectors, not HIP's uint4 class: arrays of the latter stay in scratch memory when passed by reference)
  typedef u32 v2u __attribute__((ext_vector_type(2)));
  v2u na[kTbG] = {}, nb[kTbG] = {}, nc[kTbG] = {};
  u32 c_rnd = 0xFFFFFFFFu, n_rnd = 0xFFFFFFFFu, f_rnd = 0xFFFFFFFFu;  // rounds LDS / the two register sets hold
  auto load_desc = [&](u32 rnd, u32 (&d0)[kTbG], u32 (&d1)[kTbG], u32 (&d7)[kTbG]) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < kTbG; ++h) {
      const size_t rho = (static_cast<size_t>(rnd) * kTbG + h) * 16 + static_cast<size_t>(gl);
      const uint4 da = dsc[2 * rho];
      d0[h] = da.x;
      d1[h] = da.y;
      d7[h] = da.z;
    }
  };
  auto load_codes = [&](const u32 (&d0)[kTbG], v2u (&a)[kTbG], v2u (&b)[kTbG], v2u (&c)[kTbG]) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < kTbG; ++h) {
      const u32 s2 = d0[h] & 0xFFFFu;
      const size_t tb = s2 == kInactiveS ? 0u : (s2 >> 1) / K::kU;
      const size_t bo = pin_s(bps_off);
      const v2u* src = reinterpret_cast<const v2u*>(reinterpret_cast<const unsigned char*>(dsc) + bo) + tb * 16 + static_cast<size_t>(gl);
      a[h] = src[0];
      b[h] = src[16];
      c[h] = src[32];
    }
  };
  while (sv::any(!done)) {
    // ---- change of round, all windows at once ----
    const u32 rnd = done ? c_rnd : (i - 1) / (16 * kTbG);
    const bool change = !done && rnd != c_rnd;
    // (the step and cycle counters of this function stay in the product build: without them — nothing else changed — the
    // kernel measured 18 % SLOWER on the same box, 700 against 592 ms per C4 round, at every setting of the block alignment;
    // the generated code differs by the two s_memtime reads and a handful of register moves.  Not understood)
    const unsigned long long tc0 = sv::clock();
    if (sv::any(change)) {
      lds_order();  // the walks of the previous round have read their last row
      if (change) {
        ++n_switch;
        if (rnd != n_rnd) {  // the first round of the walk (or a jump the sets do not cover): both levels right here
          load_desc(rnd, nd0, nd1, nd7);
          load_codes(nd0, na, nb, nc);
          f_rnd = 0xFFFFFFFFu;
        }
#pragma unroll
        for (int h = 0; h < kTbG; ++h) {
          uint4* dst = S.row[q][16 * h + gl];
          dst[0] = poa4_align_codes(na[h].x, na[h].y, nb[h].x, nb[h].y, nc[h].x, nc[h].y, (nd0[h] & 0xFFFFu) >> 1, (nd1[h] >> 16) & 0x3FFu);
          const u32 bt = (nd1[h] >> 16) & 0x3FFu;
          dst[1] = uint4{bt | (bt != 0 ? 0x10000u : 0u) | (bt + K::kBand < w ? 0x20000u : 0u) | (((nd1[h] >> 26) & 15u) << 20),
                         nd1[h] & 0xFFFFu, nd7[h], 0u};
        }
        c_rnd = rnd;
        if (rnd >= 1) {
          if (f_rnd == rnd - 1) {
#pragma unroll
            for (int h = 0; h < kTbG; ++h) {
              nd0[h] = fd0[h];
              nd1[h] = fd1[h];
              nd7[h] = fd7[h];
            }
          } else {
            load_desc(rnd - 1, nd0, nd1, nd7);
          }
          load_codes(nd0, na, nb, nc);
          n_rnd = rnd - 1;
        } else {
          n_rnd = 0xFFFFFFFFu;
        }
        if (rnd >= 2) {
          load_desc(rnd - 2, fd0, fd1, fd7);
          f_rnd = rnd - 2;
        } else {
          f_rnd = 0xFFFFFFFFu;
        }
      }
      lds_order();
    }
    t_change += sv::clock() - tc0;
    // ---- the walk through the round's rows: every lane of the window does the same ----
    // One step = the row's record and the code under column j out of LDS (two dependent reads), then straight-line
    // selects: the four windows of a wave are in different cases at every step, so any branch here is taken by somebody
    // and all of them would be executed anyway.  Every step lowers i + j, so the walk ends without a step counter.
    bool in_round = !done;
    while (sv::any(in_round)) {
      P4_MARK("tb_step_begin");
      const u32 l = (i - 1) & (16 * kTbG - 1);
      // the row's record and the code under column j: ONE round trip to LDS (rounds 4-5 read the rank distances behind a
      // test of the in-degree, a third dependent read); the code of column j is byte (j >> 1) & 15 of the row whatever its
      // band start
      const uint4 d = S.row[q][l][1];
      const u32 byte = pin_v(reinterpret_cast<const u8*>(S.row[q][l])[(static_cast<u32>(j) >> 1) & 15u], d);  // (all of it is wanted here, not where a branch first asks for it)
      const u32 code = (byte >> (4u * (static_cast<u32>(j) & 1u))) & 15u;  // 0: horizontal; else diagonal << 3 | 7 - in-edge
      // d.x: band start | (band start != 0) << 16 | (the matrix goes on right of the band) << 17 | in-edges << 20; d.y: node
      const u32 bt = d.x & 0xFFFFu, np = (d.x >> 20) & 15u, node = d.y;
      const u32 idx = static_cast<u32>(j) - bt;
      const bool oob = idx >= static_cast<u32>(K::kBand);  // the path left the stored band
      bool isH = code == 0u;
      const u32 k = (~code) & 7u;
      u32 ni = np ? i - ((d.z >> ((5u * k) & 31u)) & 31u) : 0u;  // (k >= 6: corrected below; the shift count as the GPU's shifter takes it)
      if (sv::any(in_round && np >= 7)) {  // rows of seven or eight in-edges (1 % of the windows have one)
        // code 0 in a row of eight in-edges is "horizontal" or "vertical through the eighth": the NW left the answer in the
        // row's v7 mask; in-edges 6 and 7: their ranks come from the graph
        // A row of 9..15 in-edges: the mask says which columns took their move through the second group (in-edges 7..14, counted
        // from 7 by the code's low bits; the descriptor of such a row has no eighth in-edge, code 0 outside the mask is "horizontal")
        u32 kk = k;
        if (in_round && !oob && np >= 8u && (isH || np >= 9u)) {
          const u32 m7 = poa4_carve(opaque(slot_mem), A.nmax, A.lmax).v7[i - 1];
          if ((m7 >> idx) & 1u) {
            isH = false;  // (np = 8: k = (~0) & 7 = 7, the eighth in-edge; code >> 3 = 0: no column is left)
            if (np >= 9u) kk = k + 7u;
          }
        }
        if (in_round && !oob && !isH && kk >= 6)
          ni = poa4_nth_pred_rank(poa4_carve(opaque(slot_mem), A.nmax, A.lmax), node, kk, full) - r_lo + 1;
      }
      // (a diagonal or horizontal code in column 0 — never on a consistent stream — leaves the band in the next step)
      const bool ok = in_round && !oob;
      // ---- the node a diagonal move aligns position j - 1 to: sixteen positions are collected in the window's lanes (lane =
      // position mod 16) and leave as one 32-byte store when the walk enters another block of sixteen; a position the walk
      // passes horizontally stays kNone, as the set-up left every position (rounds 4-5: one 2-byte store per diagonal step) ----
      const bool diag = ok && (code & 8u) != 0 && j > 0;
      const u32 p = static_cast<u32>(j) - 1u;
      if (sv::any(diag && (p >> 4) != pblk)) {
        const bool fl = diag && (p >> 4) != pblk;
        if (fl && pblk != 0xFFFFFFFFu) *pos_node_at(16u * pblk + static_cast<u32>(gl)) = static_cast<u16>(pbuf);
        if (fl) {
          pbuf = kNone4;
          pblk = p >> 4;
        }
      }
      pbuf = (diag && (p & 15u) == static_cast<u32>(gl)) ? node : pbuf;
      // ---- how near the path comes to an edge of the band beyond which the matrix goes on: within two cells = a band hit ----
      if (sv::any(ok && (idx - 2u) > static_cast<u32>(K::kBand - 5))) {
        if (ok && ((idx < 2u && (d.x & 0x10000u)) || (idx > static_cast<u32>(K::kBand - 3) && (d.x & 0x20000u)))) band_hit = 1;
      }
      if (in_round && oob) band_hit = 1;
      steps += in_round ? 1u : 0u;
      j -= ok ? static_cast<i32>(isH ? 1u : (code >> 3)) : 0;
      const bool row_move = ok && !isH;
      i = row_move ? ni : i;
      done = done || (in_round && (!ok || (row_move && ni == 0)));  // on the virtual row only insertions remain
      in_round = !done && (i - 1) / (16 * kTbG) == c_rnd;
      P4_MARK("tb_step_end");
    }
  }
  if (pblk != 0xFFFFFFFFu) *pos_node_at(16u * pblk + static_cast<u32>(gl)) = static_cast<u16>(pbuf);  // the positions of the last block
  if (A.phase_cycles && gl == 0 && act) {
    sv::atomic_add(&A.phase_cycles[11], static_cast<unsigned long long>(steps));
    sv::atomic_add(&A.phase_cycles[12], static_cast<unsigned long long>(n_switch));
  }
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[13], t_change);
}
}  // namespace
}  // namespace rvn
