// poa4_desc.h — what the window kernel (poa4.hip) prepares per layer: the layer's set-up with its subgraph sweep, the band
// guide, and the row descriptors the NW runs on.
#pragma once
#include "poa4_ops.h"
namespace rvn {
namespace {
// The row descriptors of a layer, flat over the nodes.  One wave = 256 nodes of one window (a launch gives a window ceil(nmax / 256) waves; those beyond its graph return at
// once).  Everything a node contributes is a coalesced load (rb[] holds rank and backbone coordinate of a node in one
// word), only its in-edges' tails are gathered; band starts come from the layer's guide through per-segment reciprocals
// kept in LDS.  The descriptor of every node whose rank lies in the rank range [r_lo, r_hi) of the layer's subgraph is
// written at its row rho = rank - r_lo; the steps of the layer's NW, the "beyond this kernel's limits" flag and the work
// counter are folded into the window's record with atomics.

struct alignas(16) Poa4LdsDesc {
  u32 segtab[32];  // the layer's band guide: {x0, wa, wb - wa, magic(x1 - x0)} per segment
  u32 seq2[60];    // the layer, 2 bits per base
  u8 bytes[1024];  // (set-up kernel: one-byte codes before they are packed; then 8192 rank-indexed bits of the subgraph sweep)
};

// the layer's band guide as eight segments in LDS (lanes 0..7), and the band start of a backbone coordinate from it
__host__ __device__ inline void poa4_guide_to_lds(Poa4LdsDesc& S, const PoaLayer* Lp, u32 len, i32 span) {
  const int lane = sv::lane();
  if (lane < 8) {
    const i32 sg = lane;
    const i32 x0 = (sg * span) / 8, x1 = ((sg + 1) * span) / 8;
    const i32 wa = sg == 0 ? 0 : static_cast<i32>(Lp->way[sg - 1]);
    const i32 wb = sg == 7 ? static_cast<i32>(len) : static_cast<i32>(Lp->way[sg]);
    S.segtab[4 * sg] = static_cast<u32>(x0);
    S.segtab[4 * sg + 1] = static_cast<u32>(wa);
    S.segtab[4 * sg + 2] = static_cast<u32>(wb - wa);
    S.segtab[4 * sg + 3] = magic_of(static_cast<u32>(x1 > x0 ? x1 - x0 : 1));
  }
}
template <class K>
__host__ __device__ __forceinline__ i32 poa4_band_start(const Poa4LdsDesc& S, i32 bpos, i32 lb, i32 span, u32 span_magic, u32 len) {
  // even, in [0, max(0, w - 31)]; = poa_layer_center(bpos - lb) - 16 clamped
  i32 x = bpos - lb;
  x = x < 0 ? 0 : (x > span ? span : x);
  const u32 seg = div_magic(static_cast<u32>(x) * 8u, span_magic);
  const u32 sg = seg > 7u ? 7u : seg;
  const uint4 st = *reinterpret_cast<const uint4*>(&S.segtab[4 * sg]);
  const i32 dw = static_cast<i32>(st.z);
  const u32 num = static_cast<u32>(x - static_cast<i32>(st.x)) * static_cast<u32>(dw < 0 ? -dw : dw);
  const i32 qn = static_cast<i32>(div_magic(num, st.w));
  i32 b = static_cast<i32>(st.y) + (dw < 0 ? -qn : qn) - K::kBand / 2;
  const i32 bmax = static_cast<i32>(len) + 1 - K::kBand;
  b = b > bmax ? bmax : b;
  b = b < 0 ? 0 : b;
  // even; at the right limit rounded UP, so that the band still holds the layer's last column
  return (b == bmax && bmax > 0) ? (b + 1) & ~1 : b & ~1;
}

// spoa Graph::Subgraph as marks, for one window by one wave: the ancestors (through in-edges and aligned nodes) of
// backbone node `end` among the nodes with id >= begin; sub_out = out-degree inside the subgraph; returns the rank range
// [r_lo, r_hi) that holds the marked nodes.  poa.h's version walks the graph with a stack on lane 0 — a chain of
// dependent global loads per node.  Here the nodes are swept in DECREASING rank, 64 ranks at a time: the lanes fetch
// their node's in-edges and aligned group and turn them into rank distances (everything a block needs is in flight
// together), then the wave walks the block's 64 nodes in order on 64-bit masks of marks kept in scalar registers (this
// block, the one above, the one below; a push further down goes through a bit array in LDS).  A node is marked iff its
// id is >= begin and it, or a member of its aligned group, was reached through an in-edge of a marked node: members of
// a column are reached only from later columns, which the sweep has left behind by then.
__host__ __device__ inline void poa4_subgraph_marks(Poa2Slot& g, const u32* rb, const u16* order, u32* pend, u32 n_nodes,
                                                    u32 begin, u32 end, u32& r_lo_out, u32& r_hi_out) {
  const int lane = sv::lane();
  for (u32 i = lane; i < n_nodes; i += 64) {
    g.mark[i] = 0;
    g.sub_out[i] = 0;
  }
  for (u32 i = lane; i < 256; i += 64) pend[i] = 0;  // rank-indexed bits for pushes beyond the block below
  lds_order();
  const u32 end_rank = rb[end] & 0xFFFFu;
  // (the sweep starts three ranks above `end`: the other letters of its column are reached from it and rank behind it)
  const u32 top_rank = end_rank + 3 < n_nodes ? end_rank + 3 : n_nodes - 1;
  unsigned long long w_cur = 0, w_above = 0, w_low = 0;
  u32 r_lo = 0xFFFFFFFFu, r_hi = 0;
  const i32 top_blk = static_cast<i32>(top_rank >> 6);
  if ((end_rank >> 6) == static_cast<u32>(top_blk)) w_cur = 1ULL << (end_rank & 63u);
  else w_low = 1ULL << (end_rank & 63u);
  for (i32 blk = top_blk; blk >= 0; --blk) {
    const u32 r0 = static_cast<u32>(blk) << 6;
    const u32 r = r0 + static_cast<u32>(lane);
    const bool in = r < n_nodes && r <= top_rank;
    const u32 v = in ? order[r] : 0u;
    u32 c = in ? g.in_cnt[v] : 0u;
    const u32 ac = in ? g.al_cnt[v] : 0u;
    const uint4 ta = *reinterpret_cast<const uint4*>(g.in_tail + static_cast<size_t>(v) * kPoaMaxIn);
    const uint2 al2 = *reinterpret_cast<const uint2*>(g.al + static_cast<size_t>(v) * 4);
    const bool ok = in && v >= begin;
    // rank distances of the first eight in-edges' tails (0: none, or a tail below `begin`) and of the aligned nodes
    u32 rec_a = 0, rec_b = 0, rec_f = ok ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const u32 wd = k < 2 ? ta.x : (k < 4 ? ta.y : (k < 6 ? ta.z : ta.w));
      const u32 t = static_cast<u32>(k) < c ? (wd >> (16 * (k & 1))) & 0xFFFFu : 0u;
      const u32 rt = rb[t] & 0xFFFFu;
      u32 lb = (static_cast<u32>(k) < c && t >= begin) ? r - rt : 0u;
      if (lb > 254u) {  // (a very long in-edge: through the slow path below)
        lb = 0;
        rec_f |= 2u;
      }
      if (k < 4) rec_a |= lb << (8 * k);
      else rec_b |= lb << (8 * (k - 4));
    }
    if (c > 8) rec_f |= 2u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const u32 m = k == 0 ? al2.x & 0xFFFFu : (k == 1 ? al2.x >> 16 : al2.y & 0xFFFFu);
      const bool has = static_cast<u32>(k) < ac;
      const u32 rm = rb[has ? m : 0u] & 0xFFFFu;
      const i32 d = has ? static_cast<i32>(rm) - static_cast<i32>(r) : 0;  // |d| <= 3: a column's nodes are rank-contiguous
      const u32 enc = (has && d >= -7 && d <= 7 && d != 0) ? static_cast<u32>(d + 8) : 0u;
      if (has && enc == 0) rec_f |= 2u;
      rec_f |= enc << (4 + 4 * k);
    }
    const int top_l = blk == top_blk ? static_cast<int>(top_rank & 63u) : 63;
    for (int l = top_l; l >= 0; --l) {
      const u32 f = static_cast<u32>(sv::rl(static_cast<int>(rec_f), l));
      bool reached = ((w_cur >> l) & 1ULL) != 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const u32 enc = (f >> (4 + 4 * k)) & 15u;
        if (enc) {
          const int pos = l + static_cast<int>(enc) - 8;
          const bool bit = pos >= 64 ? ((w_above >> (pos - 64)) & 1ULL) != 0
                                     : (pos >= 0 ? ((w_cur >> pos) & 1ULL) != 0 : ((w_low >> (pos + 64)) & 1ULL) != 0);
          reached = reached || bit;
        }
      }
      if (f & 2u) {  // slow path: a far tail, more than eight in-edges, or an aligned node out of place
        const u32 vs = order[r0 + static_cast<u32>(l)];
        const u32 as = g.al_cnt[vs];
        for (u32 k = 0; k < as; ++k) reached = reached || g.mark[g.al[vs * 4 + k]] != 0 ||
                                                 ((pend[(rb[g.al[vs * 4 + k]] & 0xFFFFu) >> 5] >> (rb[g.al[vs * 4 + k]] & 31u)) & 1u) != 0;
      }
      const bool marked = (f & 1u) != 0 && (reached || ((pend[(r0 + l) >> 5] >> ((r0 + l) & 31u)) & 1u) != 0);
      if (marked) {
        w_cur |= 1ULL << l;
        const u32 a = static_cast<u32>(sv::rl(static_cast<int>(rec_a), l)), b = static_cast<u32>(sv::rl(static_cast<int>(rec_b), l));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const u32 lb = ((k < 4 ? a : b) >> (8 * (k & 3))) & 0xFFu;
          if (lb) {
            const int pos = l - static_cast<int>(lb);
            if (pos >= 0) w_cur |= 1ULL << pos;
            else if (pos >= -64) w_low |= 1ULL << (pos + 64);
            else if (lane == 0) pend[(r0 + l - lb) >> 5] |= 1u << ((r0 + l - lb) & 31u);
          }
        }
        if (f & 2u) {  // slow path: every in-edge straight from the graph
          const u32 vs = order[r0 + static_cast<u32>(l)];
          const u32 cs = g.in_cnt[vs];
          for (u32 k = 0; k < cs; ++k) {
            const u32 t = g.in_tail[vs * kPoaMaxIn + k];
            if (t < begin) continue;
            const u32 rt = rb[t] & 0xFFFFu;
            if (rt >= r0) w_cur |= 1ULL << (rt - r0);
            else if (rt + 64 >= r0) w_low |= 1ULL << (rt + 64 - r0);
            else if (lane == 0) pend[rt >> 5] |= 1u << (rt & 31u);
          }
        }
        lds_order();
      } else {
        w_cur &= ~(1ULL << l);
      }
    }
    if (in && ((w_cur >> lane) & 1ULL)) {
      g.mark[v] = 1;
      r_lo = r < r_lo ? r : r_lo;
      r_hi = r + 1 > r_hi ? r + 1 : r_hi;
    }
    w_above = w_cur;
    w_cur = w_low;
    w_low = 0;
  }
  sv::sync();
  for (u32 v = lane; v < n_nodes; v += 64) {
    if (!g.mark[v]) continue;
    const u32 c = g.in_cnt[v];
    for (u32 k = 0; k < c; ++k) {
      const u32 t = g.in_tail[v * kPoaMaxIn + k];
      if (g.mark[t]) sv::atomic_add(reinterpret_cast<unsigned int*>(g.sub_out) + (t >> 1), (t & 1) ? 0x10000u : 1u);
    }
  }
  {
    const i32 lo_neg = sv::wave_max(r_lo == 0xFFFFFFFFu ? -0x7FFFFFFF : -static_cast<i32>(r_lo));
    const i32 hi = sv::wave_max(static_cast<i32>(r_hi));
    r_lo_out = lo_neg == -0x7FFFFFFF ? 0u : static_cast<u32>(-lo_neg);
    r_hi_out = lo_neg == -0x7FFFFFFF ? 0u : static_cast<u32>(hi);
  }
  sv::sync();
}

// phase A1 of a round, one window per wave: the window's next layer (codes packed 2 bits per base into the window's
// scratch, alignment results reset, subgraph marks and the rank range of the subgraph for a partial layer)
template <class K>
__host__ __device__ inline void poa4_phase_setup(const Poa4Args& A, const Poa4Ctx& C, Poa4LdsDesc& S, u32 rec) {
  const int lane = sv::lane();
  const u32 wave_dp = rec / P4::G;
  const int q = static_cast<int>(rec % P4::G);
  if (poa4_my_record(C, wave_dp, q) == 0xFFFFFFFFu) return;
  Poa4Win me = C.st[rec];
  sv::sync();  // (read by every lane before lane 0 stores the new state)
  if (me.phase != kRunning) return;
  const unsigned long long t0 = sv::clock();
  const PoaWindow wq = A.windows[me.wi];
  u32 liq = me.li;
  while (liq < wq.n_layers &&
         (A.layers[wq.layer_first + liq].len == 0 || (A.src.layer_ok && !A.src.layer_ok[wq.layer_first + liq])))
    ++liq;
  me.act = 0;
  me.li = liq;
  if (liq >= wq.n_layers) {
    me.phase = kLayersDone;
    if (lane == 0) C.st[rec] = me;
    return;
  }
  const PoaLayer L = A.layers[wq.layer_first + liq];
  if (L.len > A.lmax || L.len > static_cast<u32>(kPoa2MaxSeq)) {
    me.phase = kFailed;
    me.status = 4;
    if (lane == 0) C.st[rec] = me;
    return;
  }
  const Poa4Slot sl = poa4_carve(poa4_slot_of(A, C, wave_dp, q), A.nmax, A.lmax);
  Poa2Slot g = sl.g;
  for (u32 i = lane; i < L.len; i += 64) {
    S.bytes[i] = static_cast<u8>(poa_layer_code(A.src, L, i));
    g.pos_node[i] = static_cast<u16>(kNone4);
  }
  lds_order();
  if (lane < 60) {
    u32 x = 0;
    for (u32 c = 0; c < 16; ++c) {
      const i32 p = static_cast<i32>(static_cast<u32>(lane) * 16 + c) - 1;
      if (p >= 0 && p < static_cast<i32>(L.len)) x |= static_cast<u32>(S.bytes[p] & 3u) << (2 * c);
    }
    sl.seq2g[lane] = x;
  }
  const u32 blen = A.layers[wq.layer_first].len;
  const u32 offset = static_cast<u32>(0.01 * blen);
  const bool full = L.begin < offset && L.end > blen - offset;
  u32 r_lo = 0, r_hi = me.nn;
  if (!full) {
    lds_order();  // (the byte codes are packed: their LDS becomes the sweep's bit array)
    poa4_subgraph_marks(g, sl.rb, me.flip ? g.order2 : g.order, reinterpret_cast<u32*>(S.bytes), me.nn, L.begin, L.end, r_lo, r_hi);
  }
  const i32 lb = static_cast<i32>(L.begin), span = static_cast<i32>(L.end) - static_cast<i32>(L.begin) + 1;
  poa4_guide_to_lds(S, A.layers + wq.layer_first + liq, L.len, span);
  lds_order();
  if (lane < 32) sl.seq2g[64 + lane] = S.segtab[lane];
  u32 b_first = 0;
  if (r_hi > r_lo) {
    const u32 v0 = (me.flip ? g.order2 : g.order)[r_lo];
    b_first = static_cast<u32>(poa4_band_start<K>(S, static_cast<i32>(sl.rb[v0] >> 16), lb, span,
                                                   magic_of(static_cast<u32>(span > 0 ? span : 1)), L.len));
  }
  me.act = 1;
  me.full = full ? 1u : 0u;
  me.len = L.len;
  me.lb = L.begin;
  me.span = static_cast<u32>(span);
  me.r_lo = r_lo;
  me.n_rows = r_hi - r_lo;
  me.t_end = 0;
  me.best_rho1 = 0;
  me.b_first = b_first;
  me.dflag = 0;
  if (lane == 0) C.st[rec] = me;
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[0], sv::clock() - t0);
}

// The row descriptors of a layer, by the window's wave in two passes over the nodes (64 x kDescPer nodes per turn).  Pass 1
// streams over the nodes and leaves rank | band start of every node for THIS layer in rbl[]; pass 2 builds the
// descriptors: everything that depends only on (window, node) is a coalesced load (rb[] holds rank and backbone coordinate
// of a node in one word), an in-edge tail's rank and band start come from rbl[] with one gather (round 4 re-evaluated the
// guide per edge: nine evaluations per node), and in-edges beyond the largest in-degree of the 256 nodes in flight are not
// looked at at all.  The descriptor of every node whose rank lies in the rank range [r_lo, r_hi) of the layer's subgraph
// is written at its row rho = rank - r_lo.
constexpr int kDescPer = 4;
template <class K>
__host__ __device__ inline void poa4_phase_desc_onewave(const Poa4Args& A, const Poa4Ctx& C, Poa4LdsDesc& S, u32 rec) {
  const int lane = sv::lane();
  const u32 wave_dp = rec / P4::G;
  const int q = static_cast<int>(rec % P4::G);
  if (poa4_my_record(C, wave_dp, q) == 0xFFFFFFFFu) return;
  const Poa4Slot sl = poa4_carve(poa4_slot_of(A, C, wave_dp, q), A.nmax, A.lmax);
  const Poa2Slot& g = sl.g;
  const Poa4Win me = C.st[rec];
  if (me.phase != kRunning || !me.act) return;
  const unsigned long long t_desc0 = sv::clock();
  const u32 nn = me.nn;
  const bool full = me.full != 0;
  const u32 len = me.len, r_lo = me.r_lo, n_rows = me.n_rows, r_hi = r_lo + n_rows;
  const i32 lb = static_cast<i32>(me.lb), span = static_cast<i32>(me.span), b_first = static_cast<i32>(me.b_first);
  const u32 span_magic = magic_of(static_cast<u32>(span > 0 ? span : 1));
  const u32 dump_off = poa4_dump_byte(q);
  const u32 neg_off = poa4_neg_byte(q);
  const u32 neg2 = neg_off | (neg_off << 16);
  u32 flag = 0, marked_rows = 0;
  i32 t_end = 0;
  {  // the layer's packed codes and guide into LDS
    const u32 gw = sl.seq2g[lane < 60 ? lane : 64 + (lane - 60)];
    const u32 gw2 = lane < 28 ? sl.seq2g[68 + lane] : 0u;
    if (lane < 60) S.seq2[lane] = gw;
    else S.segtab[lane - 60] = gw;
    if (lane < 28) S.segtab[4 + lane] = gw2;
  }
  lds_order();
  // ---- pass 1: rank | band start of every node ----
  for (u32 v0 = 0; v0 < nn; v0 += 64 * kDescPer) {
    u32 rbv[kDescPer];
#pragma unroll
    for (int u = 0; u < kDescPer; ++u) {
      const u32 v = v0 + static_cast<u32>(u) * 64 + static_cast<u32>(lane);
      rbv[u] = v < nn ? sl.rb[v] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kDescPer; ++u) {
      const u32 v = v0 + static_cast<u32>(u) * 64 + static_cast<u32>(lane);
      if (v < nn) {
        const i32 b = poa4_band_start<K>(S, static_cast<i32>(rbv[u] >> 16), lb, span, span_magic, len);
        sl.rbl[v] = (rbv[u] & 0xFFFFu) | (static_cast<u32>(b) << 16);
      }
    }
  }
  sv::sync();  // rbl[]: written above by this wave, gathered below
  // ---- pass 2: the descriptors ----
  for (u32 v0 = 0; v0 < nn; v0 += 64 * kDescPer) {
    u32 vv[kDescPer], rbv[kDescPer], cc[kDescPer], code[kDescPer], outc_f[kDescPer], outc_s[kDescPer], mk[kDescPer];
    uint4 tl[kDescPer];
#pragma unroll
    for (int u = 0; u < kDescPer; ++u) {
      vv[u] = v0 + static_cast<u32>(u) * 64 + static_cast<u32>(lane);
      const u32 vq = vv[u] < nn ? vv[u] : 0u;
      rbv[u] = sl.rbl[vq];
      cc[u] = g.in_cnt[vq];
      code[u] = g.code[vq];
      outc_f[u] = g.out_cnt[vq];
      outc_s[u] = full ? 0u : g.sub_out[vq];
      mk[u] = full ? 1u : g.mark[vq];
      tl[u] = *reinterpret_cast<const uint4*>(g.in_tail + static_cast<size_t>(vq) * kPoaMaxIn);
    }
    bool ok[kDescPer], marked[kDescPer];
    u32 cmax = 0;
#pragma unroll
    for (int u = 0; u < kDescPer; ++u) {
      const u32 r = rbv[u] & 0xFFFFu;
      ok[u] = vv[u] < nn && r >= r_lo && r < r_hi;
      marked[u] = ok[u] && mk[u] != 0;
      if (!marked[u]) cc[u] = 0;
      cmax = cc[u] > cmax ? cc[u] : cmax;
    }
    cmax = static_cast<u32>(sv::wave_max(static_cast<i32>(cmax)));  // in-edges anybody of this turn has (uniform)
    u32 trb[kDescPer][8], tmk[kDescPer][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (static_cast<u32>(k) < cmax) {
#pragma unroll
        for (int u = 0; u < kDescPer; ++u) {
          const u32 wd = k < 2 ? tl[u].x : (k < 4 ? tl[u].y : (k < 6 ? tl[u].z : tl[u].w));
          const u32 t = static_cast<u32>(k) < cc[u] ? (wd >> (16 * (k & 1))) & 0xFFFFu : 0u;
          trb[u][k] = sl.rbl[t];
          tmk[u][k] = full ? 1u : g.mark[t];
        }
      } else {
#pragma unroll
        for (int u = 0; u < kDescPer; ++u) {
          trb[u][k] = 0;
          tmk[u][k] = 0;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kDescPer; ++u) {
      const u32 v = vv[u];
      const u32 r = rbv[u] & 0xFFFFu;
      const i32 b = static_cast<i32>(rbv[u] >> 16);
      const u32 rho = r - r_lo;
      u32 ep[4] = {neg2, neg2, neg2, neg2};
      u32 np = 0, lbw = 0, lbk7 = 0;
      auto edge = [&](u32 rbt, bool inside) {
        if (!inside) return;
        const u32 lbk = r - (rbt & 0xFFFFu);
        const i32 d = b - static_cast<i32>(rbt >> 16);
        if (lbk < 1 || lbk > static_cast<u32>(K::kRing - 1) || lbk > rho || d < 0 || d > K::kMaxD) {
          flag = 7;
        } else if (np < static_cast<u32>(K::kEdges)) {
          // (the row of the tail's ring slot: where a column lies in it does not depend on either band start)
          const u32 e = poa4_ring_byte(q, ((rho - lbk) % static_cast<u32>(K::kRing)) * static_cast<u32>(kRowW4));
          const u32 idx = np >> 1;
          const u32 keep = (np & 1) ? 0x0000FFFFu : 0xFFFF0000u;
          const u32 put = (np & 1) ? e << 16 : e;
#pragma unroll
          for (u32 i = 0; i < 4; ++i) ep[i] = i == idx ? ((ep[i] & keep) | put) : ep[i];
          if (np < 6) lbw |= lbk << (5 * np);
          if (np == 7) lbk7 = lbk;
        } else if (np < static_cast<u32>(K::kEdgesMax)) {
          // a ninth .. fifteenth in-edge (only the loop over in-edges 8.. below gets here: one row in ~1 000 windows).  The row's
          // overflow record takes in-edges 7..14 — the eighth moves out of the descriptor, so that code 0 of such a row is
          // "horizontal" and nothing else — and the NW's rare path reads their cells of the column pair BEFORE the step's as well
          // (it keeps no "cell left of this step's" for them), a step later than the descriptor's in-edges are read: one step less
          // of the margin before the ring slot's next owner stores, i.e. in-edges of at most kRing - 2 ranks.
          const u32 e = poa4_ring_byte(q, ((rho - lbk) % static_cast<u32>(K::kRing)) * static_cast<u32>(kRowW4));
          u16* const o16 = reinterpret_cast<u16*>(sl.ovf + rho);
          if (np == static_cast<u32>(K::kEdges)) {
            sl.ovf[rho] = uint4{(ep[3] >> 16) | (neg_off << 16), neg2, neg2, neg2};
            ep[3] = (ep[3] & 0xFFFFu) | (neg_off << 16);
            if (lbk7 > static_cast<u32>(K::kRing - 2)) flag = 7;
          }
          o16[np - 7] = static_cast<u16>(e);
          if (lbk > static_cast<u32>(K::kRing - 2)) flag = 7;
        }
        ++np;
      };
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (static_cast<u32>(k) < cmax) edge(trb[u][k], static_cast<u32>(k) < cc[u] && tmk[u][k] != 0);
      for (u32 k = 8; k < cc[u]; ++k) {  // rare
        const u32 t = g.in_tail[static_cast<size_t>(v) * kPoaMaxIn + k];
        edge(sl.rbl[t], full || g.mark[t] != 0);
      }
      if (np > static_cast<u32>(K::kEdgesMax)) flag = 3;
      if (ok[u]) {
        // match mask of the row's 32 columns against the layer
        u32 mm = 0;
        {
          const u32 wi = static_cast<u32>(b) >> 4, sh = 2u * (static_cast<u32>(b) & 15u);
          const u32 x0 = S.seq2[wi], x1 = S.seq2[wi + 1], x2 = S.seq2[wi + 2];
          const u32 pat = code[u] * 0x55555555u;
          const u32 elo = funnel_shr(x1, x0, sh) ^ pat, ehi = funnel_shr(x2, x1, sh) ^ pat;
          auto even_bits = [](u32 y) -> u32 {
            y = ~(y | (y >> 1)) & 0x55555555u;
            y = (y | (y >> 1)) & 0x33333333u;
            y = (y | (y >> 2)) & 0x0F0F0F0Fu;
            y = (y | (y >> 4)) & 0x00FF00FFu;
            y = (y | (y >> 8)) & 0x0000FFFFu;
            return y;
          };
          mm = even_bits(elo) | (even_bits(ehi) << 16);
        }
        i32 sdiff = b - b_first;
        if (sdiff < 0) {  // (never: a node's backbone coordinate does not decrease along the order)
          flag = 7;
          sdiff = 0;
        }
        const u32 Srow = rho + (rho >> 4) + (static_cast<u32>(sdiff) >> 1) + 1u;
        const u32 own = marked[u] ? poa4_ring_byte(q, (rho % static_cast<u32>(K::kRing)) * static_cast<u32>(kRowW4)) : dump_off;
        const bool endn = marked[u] && (full ? outc_f[u] : outc_s[u]) == 0;
        uint4 da, db;
        da.x = (2u * Srow) | (own << 16);
        da.y = v | (static_cast<u32>(b) << 16) | ((np > 15u ? 15u : np) << 26) | (marked[u] ? 1u << 30 : 0u) | (endn ? 1u << 31 : 0u);
        da.z = lbw;
        da.w = ep[0];
        db.x = ep[1];
        db.y = ep[2];
        db.z = ep[3];
        db.w = mm;
        sl.desc[2 * static_cast<size_t>(rho)] = da;
        sl.desc[2 * static_cast<size_t>(rho) + 1] = db;
        t_end = static_cast<i32>(Srow) + 17 > t_end ? static_cast<i32>(Srow) + 17 : t_end;
        if (marked[u]) ++marked_rows;
      }
    }
  }
  // rows beyond the last one: what the lanes' descriptor prefetch runs into
  if (lane < 32) {
    const size_t rho = static_cast<size_t>(n_rows) + static_cast<size_t>(lane);
    sl.desc[2 * rho] = uint4{kInactiveS | (dump_off << 16), 0u, 0u, neg2};
    sl.desc[2 * rho + 1] = uint4{neg2, neg2, neg2, 0u};
  }
  t_end = sv::wave_max(t_end);
  flag = static_cast<u32>(sv::wave_max(static_cast<i32>(flag)));
  marked_rows = sv::wave_sum(marked_rows);
  if (lane == 0) {  // (one wave per window: plain stores)
    Poa4Win& w = C.st[rec];
    w.t_end = static_cast<u32>(t_end);
    w.dflag = flag;
    w.cells_full += marked_rows * len;
    w.cells_band += marked_rows * (len + 1 < 32u ? len + 1 : 32u);
  }
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[10], sv::clock() - t_desc0);
}
}  // namespace
}  // namespace rvn
