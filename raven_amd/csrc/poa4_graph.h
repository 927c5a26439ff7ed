// poa4_graph.h — the graph side of the window kernel (poa4.hip), wave-wide per-window steps as in poa2.hip: backbone graph
// and state record (phase 0), graph update with a layer's alignment, consensus of a finished window.
#pragma once
#include "poa4_ops.h"
namespace rvn {
namespace {
__host__ __device__ inline void poa4_copy_backbone(const Poa4Args& A, const PoaWindow& win, const PoaLayer& bb, u8* out,
                                                   u32* out_len) {
  const int lane = sv::lane();
  const u32 n = bb.len < win.out_cap ? bb.len : win.out_cap;
  for (u32 i = lane; i < n; i += 64) out[i] = static_cast<u8>(poa_layer_code(A.src, bb, i));
  if (lane == 0) *out_len = n;
}

// window set-up: 0 = backbone returned (< 3 sequences), 4 = beyond a length limit (backbone returned), 1 = graph built
__host__ __device__ inline u32 poa4_init_window(const Poa4Args& A, const PoaWindow& win, Poa2Slot& g, u32* rb, u32 wi,
                                                u32& n_nodes, u32& n_eff) {
  const int lane = sv::lane();
  const PoaLayer bb = A.layers[win.layer_first];
  const u32 blen = bb.len;
  n_eff = win.n_layers;
  if (A.src.layer_ok) {  // layers dropped by racon's mean-quality filter do not count as sequences of the window
    u32 cnt = 0;
    for (u32 i = 1 + lane; i < win.n_layers; i += 64) cnt += A.src.layer_ok[win.layer_first + i] ? 1u : 0u;
    n_eff = 1 + sv::wave_sum(cnt);
  }
  n_nodes = 0;
  if (n_eff < 3) {
    poa4_copy_backbone(A, win, bb, A.out + win.out_off, A.out_len + wi);
    return 0;
  }
  if (blen == 0 || blen > A.nmax || blen > A.lmax) {
    poa4_copy_backbone(A, win, bb, A.out + win.out_off, A.out_len + wi);
    return 4;
  }
  // backbone graph (spoa AddAlignment with an empty alignment)
  n_nodes = blen;
  for (u32 i = lane; i < blen; i += 64) {
    g.code[i] = static_cast<u8>(poa_layer_code(A.src, bb, i));
    g.al_cnt[i] = 0;
    g.visits[i] = blen >= 2 ? 1 : 0;
    g.order[i] = static_cast<u16>(i);
    rb[i] = i | (i << 16);  // (rank and backbone coordinate of a node live in rb[] alone here: poa2's rank_of[] / bpos[] are not kept)
    const i32 wgt = poa_layer_weight(A.src, bb, i);
    if (i > 0) {
      const i32 wp = poa_layer_weight(A.src, bb, i - 1);
      g.in_cnt[i] = 1;
      g.in_tail[i * kPoaMaxIn] = static_cast<u16>(i - 1);
      g.in_w[i * kPoaMaxIn] = wp + wgt;
    } else {
      g.in_cnt[i] = 0;
    }
    g.out_cnt[i] = i + 1 < blen ? 1 : 0;
  }
  // nodes to come: poa4_update_graph counts on zero in-degree / out-degree / visits of an id it hands out
  for (u32 i = blen + lane; i < A.nmax; i += 64) {
    g.in_cnt[i] = 0;
    g.out_cnt[i] = 0;
    g.visits[i] = 0;
  }
  sv::sync();
  return 1;
}

template <class GT>
__host__ __device__ __forceinline__ u32 poa4_letter(const GT& Sg, u32 p) {
  return (Sg.seq2[(p + 1) >> 4] >> (2 * ((p + 1) & 15u))) & 3u;
}

// ---- graph update of the wave's windows side by side: spoa AddAlignment + the incremental order rebuild ---------------
// Sixteen lanes per window, four sequence positions per lane and iteration, every level of the gather chain
// (position -> aligned node -> its aligned group -> the node the position lands on) issued for all four positions before
// any is consumed.  A path visits distinct nodes of distinct columns, so target lookup, node creation, group updates and
// the edge (p - 1 -> p) are conflict-free between positions; new ids and order slots come from ballots / prefix counts
// in path order, identical to the serial order of creation.  in_cnt / out_cnt / visits of every node id are zero from
// the window's set-up on, so creating a node writes only what is not zero, and an edge's weight and its tail's
// out-degree are added with atomics (no read-modify-write round trip).  The new nodes' order slots stay in the group's
// LDS (the DP ring is free); ranks move by a binary search there, and the order array is rebuilt into the window's
// second order buffer (`flip` says which of the two is current).  Returns 0 or the failure code (group-uniform).
__host__ __device__ __forceinline__ Poa2Slot poa4_graph(unsigned char* slot_mem, u32 nmax, u32 lmax, bool flip) {
  Poa2Slot g = poa4_carve(slot_mem, nmax, lmax).g;
  if (flip) {
    u16* t = g.order;
    g.order = g.order2;
    g.order2 = t;
  }
  return g;
}


// GW = lanes per window: 64 (one window per wave, 256 positions per iteration — the update kernel) or 16.
template <int GW, int UP>
__host__ __device__ inline u32 poa4_update_graph(const Poa4Args A, u16* nslot, const u32* seq2, unsigned char* slot_mem, bool act,
                                                 const PoaLayer* Lp, u32 len, u32 lb, u32& nn, bool& flip,
                                                 unsigned long long& t_add, unsigned long long& t_ord) {
  P4_ASSUME_GLOBAL(slot_mem);
  P4_ASSUME_GLOBAL(Lp);
  P4_ASSUME_LDS(nslot);
  P4_ASSUME_LDS(seq2);
  const int lane = sv::lane();
  const int gl = lane & (GW - 1), gbase = lane & ~(GW - 1);
  constexpr unsigned long long kGMask = GW == 64 ? ~0ULL : ((1ULL << (GW & 63)) - 1ULL);
  auto shift1 = [&](int v, int fill) -> int {  // value of the lane below in the window; its first lane gets `fill`
    if constexpr (GW == 16) {
      return sv::row_shr<1>(v, fill);
    } else {
      const int t = sv::bperm(v, lane - 1);
      return gl == 0 ? fill : t;
    }
  };
  auto gmax = [&](i32 v) -> i32 {
    if constexpr (GW == 16) return group_max_i(v);
    else return sv::wave_max(v);
  };
  const Poa2Slot g = poa4_graph(slot_mem, A.nmax, A.lmax, flip);
  // rank and backbone coordinate of a node are ONE word (rb[v] = rank | coordinate << 16): one gather where poa2's separate
  // rank_of[] / bpos[] arrays took two, one scattered store per node in the order rebuild instead of two
  const u32* const rb32 = poa4_carve(slot_mem, A.nmax, A.lmax).rb;
  u16* const rb16 = reinterpret_cast<u16*>(poa4_carve(slot_mem, A.nmax, A.lmax).rb);  // [2 v] rank, [2 v + 1] backbone coordinate
  const PoaLayer L = *Lp;
  const u32 nmax = A.nmax, lmax = A.lmax;
  unsigned long long t0 = sv::clock();
  const u32 n_old = nn;
  const u32 max_len = static_cast<u32>(sv::wave_max(act ? static_cast<int>(len) : 0));
  auto gballot = [&](bool p) -> unsigned long long { return (sv::ballot(p) >> gbase) & kGMask; };
  auto letter_at = [&](u32 p) -> u32 { return (seq2[(p + 1) >> 4] >> (2 * ((p + 1) & 15u))) & 3u; };
  // ---- the first aligned position: the unaligned prefix goes before all members of its column ----
  u32 first_p = 0xFFFFFFFFu;
  for (u32 p0 = 0; p0 < max_len; p0 += UP * GW) {
    if (!sv::any(act && first_p == 0xFFFFFFFFu && p0 < len)) break;
    u32 pn[UP];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const u32 p = p0 + static_cast<u32>(GW) * static_cast<u32>(u) + static_cast<u32>(gl);
      pn[u] = (act && p < len) ? g.pos_node[p] : kNone4;
    }
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const unsigned long long bal = gballot(pn[u] != kNone4);
      if (first_p == 0xFFFFFFFFu && bal) first_p = p0 + static_cast<u32>(GW) * static_cast<u32>(u) + static_cast<u32>(__builtin_ctzll(bal));
    }
  }
  u32 carry_slot = n_old, carry_b = lb;
  if (act && first_p != 0xFFFFFFFFu) {
    const u32 an = g.pos_node[first_p];
    const u32 rb_an = rb32[an];
    u32 r = rb_an & 0xFFFFu;
    const u32 ac = g.al_cnt[an];
    const uint2 al2 = *reinterpret_cast<const uint2*>(g.al + static_cast<size_t>(an) * 4);
    const u32 a0 = al2.x & 0xFFFFu, a1 = al2.x >> 16, a2 = al2.y & 0xFFFFu;
    const u32 r0 = rb32[ac > 0 ? a0 : an] & 0xFFFFu, r1 = rb32[ac > 1 ? a1 : an] & 0xFFFFu, r2 = rb32[ac > 2 ? a2 : an] & 0xFFFFu;
    r = r0 < r ? r0 : r;
    r = r1 < r ? r1 : r;
    r = r2 < r ? r2 : r;
    carry_slot = r;
    carry_b = rb_an >> 16;
  }
  u32 total_new = 0;
  u32 why = 0;  // != 0: the window has failed; its lanes keep step with the wave without touching the graph
  u32 prev_tgt = kNone4;   // node of position p0 - 1 (the last position of the previous iteration)
  i32 prev_w = 0;          // its weight
  for (u32 p0 = 0; p0 < max_len; p0 += UP * GW) {
    const bool go = act && why == 0;
    u32 p[UP], an[UP], letter[UP];
    bool valid[UP], has[UP];
    // level 1: the nodes the positions are aligned to
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      p[u] = p0 + static_cast<u32>(GW) * static_cast<u32>(u) + static_cast<u32>(gl);
      valid[u] = go && p[u] < len;
      an[u] = valid[u] ? g.pos_node[p[u]] : kNone4;
      letter[u] = valid[u] ? letter_at(p[u]) : 0u;
    }
    // level 2: those nodes
    u32 c_an[UP], ac[UP], rk_an[UP], bp_an[UP];
    uint2 al2[UP];
    i32 wgt[UP];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      has[u] = valid[u] && an[u] != kNone4;
      const u32 a = has[u] ? an[u] : 0u;
      c_an[u] = g.code[a];
      ac[u] = g.al_cnt[a];
      const u32 rba = rb32[a];
      rk_an[u] = rba & 0xFFFFu;
      bp_an[u] = rba >> 16;
      al2[u] = *reinterpret_cast<const uint2*>(g.al + static_cast<size_t>(a) * 4);
      wgt[u] = valid[u] ? static_cast<i32>(static_cast<u8>(poa_layer_weight(A.src, L, p[u]))) : 0;
    }
    // level 3: their aligned groups (at most three other letters)
    u32 kt[UP][3], c_kt[UP][3], rk_kt[UP][3];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      if (!has[u]) ac[u] = 0;
      kt[u][0] = al2[u].x & 0xFFFFu;
      kt[u][1] = al2[u].x >> 16;
      kt[u][2] = al2[u].y & 0xFFFFu;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const u32 t = static_cast<u32>(k) < ac[u] ? kt[u][k] : 0u;
        c_kt[u][k] = g.code[t];
        rk_kt[u][k] = rb32[t] & 0xFFFFu;
      }
    }
    // where every position lands; order slot / backbone coordinate of the last aligned position at or before it
    u32 tgt[UP], id_new[UP];
    bool is_new[UP];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      u32 t = kNone4, rmax = rk_an[u];
      if (has[u]) {
        if (c_an[u] == letter[u]) t = an[u];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (static_cast<u32>(k) < ac[u]) {
            rmax = rk_kt[u][k] > rmax ? rk_kt[u][k] : rmax;
            if (t == kNone4 && c_kt[u][k] == letter[u]) t = kt[u][k];
          }
        }
      }
      const u32 gslot = rmax + 1, gb = bp_an[u];
      const unsigned long long bal = gballot(has[u]);
      const unsigned long long below = bal & (gl == 63 ? ~0ULL : ((2ULL << gl) - 1ULL));
      const int src = below ? 63 - __builtin_clzll(below) : 0;
      const u32 s_sh = static_cast<u32>(sv::bperm(static_cast<int>(gslot), gbase | src));
      const u32 b_sh = static_cast<u32>(sv::bperm(static_cast<int>(gb), gbase | src));
      const u32 fslot = below ? s_sh : carry_slot;
      const u32 fb = below ? b_sh : carry_b;
      {
        const int top = bal ? 63 - __builtin_clzll(bal) : 0;
        const u32 cs = static_cast<u32>(sv::bperm(static_cast<int>(gslot), gbase | top));
        const u32 cb = static_cast<u32>(sv::bperm(static_cast<int>(gb), gbase | top));
        if (bal) {
          carry_slot = cs;
          carry_b = cb;
        }
      }
      is_new[u] = valid[u] && t == kNone4;
      const unsigned long long nb = gballot(is_new[u]);
      const u32 cnt = static_cast<u32>(__builtin_popcountll(nb));
      if (go && why == 0 && (n_old + total_new + cnt > nmax || total_new + cnt > lmax)) why = 2;
      id_new[u] = 0;
      if (is_new[u] && why == 0) {
        const u32 tn = total_new + static_cast<u32>(__builtin_popcountll(nb & ((1ULL << gl) - 1ULL)));
        const u32 id = n_old + tn;
        id_new[u] = id;
        t = id;
        nslot[tn] = static_cast<u16>(fslot);
        g.code[id] = static_cast<u8>(letter[u]);
        rb16[2 * static_cast<size_t>(id) + 1] = static_cast<u16>(fb);
        u32 c2 = 0;
        uint2 mine = uint2{0, 0};
        if (has[u]) {  // joins an's aligned group: every member lists every other one
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            if (static_cast<u32>(k) < ac[u]) {
              g.al[static_cast<size_t>(kt[u][k]) * 4 + ac[u]] = static_cast<u16>(id);
              g.al_cnt[kt[u][k]] = static_cast<u8>(ac[u] + 1);
              if (c2 == 0) mine.x = kt[u][k];
              else if (c2 == 1) mine.x |= kt[u][k] << 16;
              else mine.y = kt[u][k];
              ++c2;
            }
          }
          if (ac[u] < 4) {
            g.al[static_cast<size_t>(an[u]) * 4 + ac[u]] = static_cast<u16>(id);
            g.al_cnt[an[u]] = static_cast<u8>(ac[u] + 1);
          }
          if (c2 == 0) mine.x = an[u];
          else if (c2 == 1) mine.x |= an[u] << 16;
          else if (c2 == 2) mine.y = an[u];
          else mine.y |= an[u] << 16;
          ++c2;
        }
        *reinterpret_cast<uint2*>(g.al + static_cast<size_t>(id) * 4) = mine;
        g.al_cnt[id] = static_cast<u8>(c2);
      }
      if (why == 0) total_new += cnt;
      tgt[u] = t;
    }
    // level 4: the in-edge lists of the nodes the positions land on (a new node's is empty)
    u32 icnt[UP];
    uint4 ta[UP], tb[UP];
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      const bool old = valid[u] && why == 0 && !is_new[u];
      const u32 t = old ? tgt[u] : 0u;
      icnt[u] = old ? g.in_cnt[t] : 0u;
      ta[u] = old ? *reinterpret_cast<const uint4*>(g.in_tail + static_cast<size_t>(t) * kPoaMaxIn) : uint4{0, 0, 0, 0};
      tb[u] = old ? *reinterpret_cast<const uint4*>(g.in_tail + static_cast<size_t>(t) * kPoaMaxIn + 8) : uint4{0, 0, 0, 0};
    }
    // the edges (p - 1 -> p)
#pragma unroll
    for (int u = 0; u < UP; ++u) {
      // node and weight of position p - 1: the lane below; lane 0 takes the last lane of the previous quarter
      const u32 last_t = static_cast<u32>(sv::bperm(static_cast<int>(u == 0 ? prev_tgt : tgt[u > 0 ? u - 1 : 0]), gbase | (GW - 1)));
      const i32 last_w = sv::bperm(u == 0 ? prev_w : wgt[u > 0 ? u - 1 : 0], gbase | (GW - 1));
      const u32 tail = static_cast<u32>(shift1(static_cast<int>(tgt[u]), static_cast<int>(last_t)));
      const i32 tw = shift1(wgt[u], last_w);
      if (valid[u] && why == 0) {
        const u32 head = tgt[u];
        if (len >= 2) {
          if (is_new[u]) g.visits[head] = 1;
          else atomic_inc_u16(g.visits, head);
        }
        if (p[u] >= 1) {
          const i32 weight = tw + wgt[u];
          const u32 c = icnt[u];
          u32 found = 0xFFu;
#pragma unroll
          for (int i2 = 0; i2 < 16; ++i2) {
            const uint4& src4 = i2 < 8 ? ta[u] : tb[u];
            const u32 wd = (i2 & 7) < 2 ? src4.x : ((i2 & 7) < 4 ? src4.y : ((i2 & 7) < 6 ? src4.z : src4.w));
            const u32 tt = (wd >> (16 * (i2 & 1))) & 0xFFFFu;
            if (static_cast<u32>(i2) < c && tt == tail && found == 0xFFu) found = static_cast<u32>(i2);
          }
          if (found != 0xFFu) {
            atomic_add_i32(g.in_w + static_cast<size_t>(head) * kPoaMaxIn + found, weight);
          } else if (c >= static_cast<u32>(kPoaMaxIn)) {
            why = 3;
          } else {
            g.in_tail[static_cast<size_t>(head) * kPoaMaxIn + c] = static_cast<u16>(tail);
            g.in_w[static_cast<size_t>(head) * kPoaMaxIn + c] = weight;
            g.in_cnt[head] = static_cast<u8>(c + 1);
            atomic_inc_u16(g.out_cnt, tail);
          }
        }
      }
    }
    // a failure anywhere in the window stops the whole window
    {
      const u32 wmax = static_cast<u32>(gmax(static_cast<i32>(why)));
      why = wmax;
    }
    prev_tgt = static_cast<u32>(sv::bperm(static_cast<int>(tgt[UP - 1]), gbase | (GW - 1)));
    prev_w = sv::bperm(wgt[UP - 1], gbase | (GW - 1));
  }
  t_add += sv::clock() - t0;
  t0 = sv::clock();
  const u32 n_new = total_new;
  lds_order();  // nslot
  // ---- order rebuild: old rank r -> r + #(new slots <= r); t-th new node -> slot_t + t ----
  const bool doit = act && why == 0 && n_new != 0;
  if (sv::any(doit)) {
    const u32 max_old = static_cast<u32>(sv::wave_max(doit ? static_cast<int>(n_old) : 0));
    for (u32 r0 = 0; r0 < max_old; r0 += UP * GW) {
      u32 rr[UP], vv[UP];
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        rr[u] = r0 + static_cast<u32>(GW) * static_cast<u32>(u) + static_cast<u32>(gl);
        vv[u] = (doit && rr[u] < n_old) ? g.order[rr[u]] : 0u;
      }
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        if (doit && rr[u] < n_old) {
          u32 lo = 0, hi = n_new;  // upper_bound(nslot, r)
          while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (nslot[mid] <= rr[u]) lo = mid + 1;
            else hi = mid;
          }
          g.order2[rr[u] + lo] = static_cast<u16>(vv[u]);
          rb16[2 * static_cast<size_t>(vv[u])] = static_cast<u16>(rr[u] + lo);
        }
      }
    }
    const u32 max_new = static_cast<u32>(sv::wave_max(doit ? static_cast<int>(n_new) : 0));
    for (u32 t = static_cast<u32>(gl); t < max_new; t += GW) {
      if (doit && t < n_new) {
        const u32 r = static_cast<u32>(nslot[t]) + t;
        g.order2[r] = static_cast<u16>(n_old + t);
        rb16[2 * static_cast<size_t>(n_old + t)] = static_cast<u16>(r);
      }
    }
    if (doit) flip = !flip;
  }
  if (act && why == 0) nn = n_old + n_new;
  sv::sync();
  t_ord += sv::clock() - t0;
  return why;
}

// Consensus of a finished window: spoa's heaviest bundle with the node scores in the WAVE's LDS (the DP of every window
// of the wave is over by now), first four in-edges of 64 nodes at a time in registers (as poa2_consensus), then branch
// completion + racon's coverage trim on lane 0 and a parallel output copy.
__host__ __device__ inline void poa4_consensus_general(Poa2Slot& g, u32 n_nodes, u32 nmax, const PoaWindow& win, int trim, Poa4Lds& S,
                                               u8* out, u32* out_len) {
  const int lane = sv::lane();
  // (the lane-0 code shared with poa2.hip wants a node's rank in rank_of[], which this kernel does not keep per layer)
  for (u32 r = lane; r < n_nodes; r += 64) g.rank_of[g.order[r]] = static_cast<u16>(r);
  constexpr u32 kCap = sizeof(Poa4Lds) / 4;
  i32* lsc = reinterpret_cast<i32*>(&S);
  i32 maxn = -1;
  if (n_nodes > kCap) {
    if (lane == 0) maxn = poa_consensus_scores_lane0(g, n_nodes);
    maxn = sv::rfl(maxn);
  } else {
    i32 max_sc = 0;
    const u32 nn = n_nodes;
    for (u32 r0 = 0; r0 < nn; r0 += 64) {
      const u32 rows = nn - r0 < 64 ? nn - r0 : 64;
      int m_it = 0, m_c = 0, m_t01 = 0, m_t23 = 0, m_w0 = 0, m_w1 = 0, m_w2 = 0, m_w3 = 0;
      if (static_cast<u32>(lane) < rows) {
        m_it = g.order[r0 + lane];
        m_c = g.in_cnt[m_it];
        const u16* tp = g.in_tail + static_cast<size_t>(m_it) * kPoaMaxIn;
        const i32* wp = g.in_w + static_cast<size_t>(m_it) * kPoaMaxIn;
        m_t01 = static_cast<int>(static_cast<u32>(tp[0]) | (static_cast<u32>(tp[1]) << 16));
        m_t23 = static_cast<int>(static_cast<u32>(tp[2]) | (static_cast<u32>(tp[3]) << 16));
        m_w0 = wp[0];
        m_w1 = wp[1];
        m_w2 = wp[2];
        m_w3 = wp[3];
      }
      for (u32 l = 0; l < rows; ++l) {
        const int li = static_cast<int>(l);
        const u32 it = static_cast<u32>(sv::rl(m_it, li));
        const u32 c = static_cast<u32>(sv::rl(m_c, li));
        const u32 t01 = static_cast<u32>(sv::rl(m_t01, li)), t23 = static_cast<u32>(sv::rl(m_t23, li));
        const i32 w0 = sv::rl(m_w0, li), w1 = sv::rl(m_w1, li), w2 = sv::rl(m_w2, li), w3 = sv::rl(m_w3, li);
        i32 sc = -1, pd = -1, pd_sc = 0;
        for (u32 k = 0; k < c; ++k) {
          i32 wgt, t;
          if (k < 4) {
            t = static_cast<i32>(((k < 2 ? t01 : t23) >> (16 * (k & 1))) & 0xFFFFu);
            wgt = k == 0 ? w0 : (k == 1 ? w1 : (k == 2 ? w2 : w3));
          } else {
            wgt = g.in_w[static_cast<size_t>(it) * kPoaMaxIn + k];
            t = static_cast<i32>(g.in_tail[static_cast<size_t>(it) * kPoaMaxIn + k]);
          }
          const i32 st = lsc[t];
          if (sc < wgt || (sc == wgt && pd_sc <= st)) {
            sc = wgt;
            pd = t;
            pd_sc = st;
          }
        }
        if (pd != -1) sc += pd_sc;
        lds_order();  // every lane has read the scores it needs before this node's is written
        if (lane == 0) {
          lsc[it] = sc;
          g.scores[it] = sc;
          g.preds[it] = pd;
        }
        lds_order();
        if (maxn == -1 || max_sc < sc) {
          maxn = static_cast<i32>(it);
          max_sc = sc;
        }
      }
    }
  }
  sv::sync();  // scores / predecessors in HBM visible to lane 0's branch completion and traceback
  u32 cl = 0;
  i32 begin = 0, end = -1;
  if (lane == 0) poa_consensus_trace_lane0(g, n_nodes, nmax, win, trim, maxn, &cl, &begin, &end);
  cl = static_cast<u32>(sv::rfl(static_cast<int>(cl)));
  begin = sv::rfl(begin);
  end = sv::rfl(end);
  sv::sync();  // g.stack
  i32 n_out = end - begin + 1;
  if (n_out < 0) n_out = 0;
  if (static_cast<u32>(n_out) > win.out_cap) n_out = static_cast<i32>(win.out_cap);
  for (i32 p = lane; p < n_out; p += 64) out[p] = g.code[g.stack[cl - 1 - static_cast<u32>(begin + p)]];
  if (lane == 0) *out_len = static_cast<u32>(n_out);
}

// The same for the common case, with nothing but registers and LDS between the graph and the consensus (round 5; the
// general form above took 10 % of the kernel's wave cycles: every node's score went through LDS and the walk back along
// the predecessors was ~600 dependent loads from global memory on lane 0).  Along the rank order a node's in-edges reach
// back a few ranks (at most 23 inside any layer's subgraph), so the scores of the last 64 ranks live in ONE vector register
// — lane = rank mod 64, read with v_readlane, written with v_writelane: the serial loop over the nodes is scalar code with
// no memory access at all —, the predecessors go to LDS (u16 per node) where the walk back follows them, and the stack of
// the consensus nodes stays in LDS for the output copy.  A window beyond what this form holds (more than 2 436 nodes, an
// in-edge reaching back more than 63 ranks) or whose heaviest path does not end in an end node (spoa's branch completion
// rewrites scores) takes the general form.  Same tie rules, same results.
__host__ __device__ inline void poa4_consensus(Poa2Slot& g, const u32* rb, u32 n_nodes, u32 nmax, const PoaWindow& win, int trim,
                                               Poa4Lds& S, u8* out, u32* out_len) {
  const int lane = sv::lane();
  constexpr u32 kCapNodes = sizeof(Poa4Lds) / 4;  // u16 predecessor per node + u16 stack entry per consensus node
  u16* lpred = reinterpret_cast<u16*>(&S);
  u16* lstack = lpred + kCapNodes;
  bool general = n_nodes > kCapNodes;
  i32 maxn = -1, max_sc = 0;
  if (!general) {
    int ring = 0;  // lane l: score of the last node computed at a rank = l (mod 64)
    u32 bad = 0;
    for (u32 r0 = 0; r0 < n_nodes; r0 += 64) {
      const u32 rows = n_nodes - r0 < 64 ? n_nodes - r0 : 64;
      int m_it = 0, m_c = 0, m_lb = 0, m_t01 = 0, m_t23 = 0, m_w0 = 0, m_w1 = 0, m_w2 = 0, m_w3 = 0;
      if (static_cast<u32>(lane) < rows) {
        const u32 r = r0 + static_cast<u32>(lane);
        m_it = g.order[r];
        m_c = g.in_cnt[m_it];
        const u16* tp = g.in_tail + static_cast<size_t>(m_it) * kPoaMaxIn;
        const i32* wp = g.in_w + static_cast<size_t>(m_it) * kPoaMaxIn;
        const uint2 t4 = *reinterpret_cast<const uint2*>(tp);
        const int4 w4 = *reinterpret_cast<const int4*>(wp);
        m_t01 = static_cast<int>(t4.x);
        m_t23 = static_cast<int>(t4.y);
        m_w0 = w4.x;
        m_w1 = w4.y;
        m_w2 = w4.z;
        m_w3 = w4.w;
        u32 lb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // how many ranks the first four in-edges reach back
          const u32 t = ((k < 2 ? t4.x : t4.y) >> (16 * (k & 1))) & 0xFFFFu;
          const u32 d = static_cast<u32>(k) < static_cast<u32>(m_c) ? r - (rb[t] & 0xFFFFu) : 1u;
          if (d < 1 || d > 63) bad = 1;
          lb |= (d & 63u) << (8 * k);
        }
        m_lb = static_cast<int>(lb);
      }
      int predv = 0xFFFF;
      for (u32 l = 0; l < rows; ++l) {
        const int li = static_cast<int>(l);
        const u32 r = r0 + l;
        const u32 it = static_cast<u32>(sv::rl(m_it, li));
        const u32 c = static_cast<u32>(sv::rl(m_c, li));
        const u32 lb = static_cast<u32>(sv::rl(m_lb, li));
        const u32 t01 = static_cast<u32>(sv::rl(m_t01, li)), t23 = static_cast<u32>(sv::rl(m_t23, li));
        const i32 w0 = sv::rl(m_w0, li), w1 = sv::rl(m_w1, li), w2 = sv::rl(m_w2, li), w3 = sv::rl(m_w3, li);
        i32 sc = -1, pd = -1, pd_sc = 0;
        for (u32 k = 0; k < c; ++k) {
          i32 wgt, t;
          u32 d;
          if (k < 4) {
            t = static_cast<i32>(((k < 2 ? t01 : t23) >> (16 * (k & 1))) & 0xFFFFu);
            wgt = k == 0 ? w0 : (k == 1 ? w1 : (k == 2 ? w2 : w3));
            d = (lb >> (8 * k)) & 0xFFu;
          } else {  // (1 % of the nodes)
            wgt = g.in_w[static_cast<size_t>(it) * kPoaMaxIn + k];
            t = static_cast<i32>(g.in_tail[static_cast<size_t>(it) * kPoaMaxIn + k]);
            d = r - (rb[t] & 0xFFFFu);
            if (d < 1 || d > 63) {
              bad = 1;
              d = 1;
            }
          }
          const i32 st = sv::rl(ring, static_cast<int>((r - d) & 63u));
          if (sc < wgt || (sc == wgt && pd_sc <= st)) {
            sc = wgt;
            pd = t;
            pd_sc = st;
          }
        }
        if (pd != -1) sc += pd_sc;
        ring = sv::wl(ring, sc, li);
        predv = sv::wl(predv, pd == -1 ? 0xFFFF : pd, li);
        if (maxn == -1 || max_sc < sc) {
          maxn = static_cast<i32>(it);
          max_sc = sc;
        }
      }
      if (static_cast<u32>(lane) < rows) lpred[m_it] = static_cast<u16>(predv);
    }
    general = sv::any(bad != 0) || (maxn >= 0 && g.out_cnt[maxn] != 0);  // (the latter: spoa's branch completion)
  }
  if (general) {
    sv::sync();
    poa4_consensus_general(g, n_nodes, nmax, win, trim, S, out, out_len);
    return;
  }
  lds_order();  // lpred
  u32 cl = 0;
  i32 begin = 0, end = -1;
  if (lane == 0) {
    // the walk back along the predecessors (reverse order into the stack), then racon's coverage trim — as
    // poa_consensus_trace_lane0 (poa.h), everything it follows in LDS
    u32 cur = maxn < 0 ? 0xFFFFu : static_cast<u32>(maxn);
    while (cur != 0xFFFFu && cl < kCapNodes) {
      lstack[cl++] = static_cast<u16>(cur);
      cur = lpred[cur];
    }
    end = static_cast<i32>(cl) - 1;
    if (trim) {
      const u32 avg = (win.n_layers - 1) / 2;
      auto cov = [&](i32 pos) -> u32 {  // coverage of a consensus node = visits of the node + of its aligned nodes
        const u32 v = lstack[cl - 1 - static_cast<u32>(pos)];
        u32 c = g.visits[v];
        for (u32 k = 0; k < g.al_cnt[v]; ++k) c += g.visits[g.al[v * 4 + k]];
        return c;
      };
      for (; begin < static_cast<i32>(cl); ++begin)
        if (cov(begin) >= avg) break;
      for (; end >= 0; --end)
        if (cov(end) >= avg) break;
      if (begin >= end) {  // racon: warning only, consensus kept untrimmed
        begin = 0;
        end = static_cast<i32>(cl) - 1;
      }
    }
  }
  cl = static_cast<u32>(sv::rfl(static_cast<int>(cl)));
  begin = sv::rfl(begin);
  end = sv::rfl(end);
  lds_order();  // lstack
  i32 n_out = end - begin + 1;
  if (n_out < 0) n_out = 0;
  if (static_cast<u32>(n_out) > win.out_cap) n_out = static_cast<i32>(win.out_cap);
  for (i32 p = lane; p < n_out; p += 64) out[p] = g.code[lstack[cl - 1 - static_cast<u32>(begin + p)]];
  if (lane == 0) *out_len = static_cast<u32>(n_out);
}

// phase 0: graph of the backbone, state record
__host__ __device__ inline void poa4_phase_init(const Poa4Args& A, const Poa4Ctx& C, u32 wave) {
  const int lane = sv::lane();
  const unsigned long long t_init0 = sv::clock();
  for (int q2 = 0; q2 < P4::G; ++q2) {
    const u32 rec = poa4_my_record(C, wave, q2);
    if (rec == 0xFFFFFFFFu) continue;
    const u32 pos = poa4_position(C, wave, q2);
    const u32 wi = A.sched ? A.sched[pos] : pos;
    const PoaWindow wq = A.windows[wi];
    const Poa4Slot sl2 = poa4_carve(poa4_slot_of(A, C, wave, q2), A.nmax, A.lmax);
    Poa2Slot g = sl2.g;
    u32 nn2 = 0, ne2 = 0;
    const u32 r = poa4_init_window(A, wq, g, sl2.rb, wi, nn2, ne2);
    if (lane == 0) {
      Poa4Win w{};
      w.wi = wi;
      w.phase = r == 1 ? kRunning : kFinal;
      w.status = r == 1 ? 0u : r;
      w.nn = nn2;
      w.n_eff = ne2;
      w.li = 1;
      C.st[rec] = w;
    }
  }
  if (A.phase_cycles && lane == 0) sv::atomic_add(&A.phase_cycles[15], sv::clock() - t_init0);
}
}  // namespace
}  // namespace rvn
