// unitigs.hip — raven::CreateUnitigs (RavenLib/src/common.cc:32-225, the unitig constructor graph.cc:27-57) on the edge
// table, and node sequences as tilings of the reads (engine.h: TilingDev, UnitigTables; rules: unitig_rules.h).
// The reference walks every non-branching chain node by node; the only state its loop carries is is_visited, which decides
// which node of a chain gets to create it.  Here the chains are the paths and cycles of a successor function on the
// non-junction nodes:
//   degrees      atomics over the edge table; a node of degree 1 keeps the id of its one in-edge and its one out-edge.  The
//                same pass checks that the table is pair-symmetric (the chain of a node's pair is then the paired chain).
//   successor    succ[u] where u and the head of its only out-edge are both non-junctions.
//   ranking      pointer jumping over succ: steps to the chain's end, the end, the smallest id on the way.  ceil(log2 n) + 1
//                rounds finish every path; a node whose pointer is still live then lies on a cycle, and the smallest id of
//                the cycle is its creating node (graph.nodes is walked in ascending id).  Cycles are cut in front of that
//                node and ranked once more, as paths that start there.
//   numbering    a chain and its paired chain hold the ids {x, x ^ 1}; the smallest of them all is even, and the chain that
//                holds it is the orientation that creates.  Flags at those ids, scan.hip: creation order.
//   members      every node finds its unitig through its chain's end and its place from its rank; prefix lengths, segment
//                counts and counts go through exclusive scans over the member table (the differences are the segmented sums).
//   packing      by destination: one lane per packed 64-bit word (tiling_word), coalesced stores.
// No kernel loop's trip count depends on a cycle being absent: the jumping rounds are counted on the host, the segment
// loops by the tiling's offsets.
#include <cstring>
#include <vector>

#include "abi.h"
#include "unitig_rules.h"

namespace rvn {

namespace {

constexpr u32 kNone = 0xFFFFFFFFu;
constexpr u32 kMaxEpsilon = 1u << 30;  // 2 epsilon + 2 stays below 2^32

__global__ void degrees_kernel(const u32* __restrict__ tail, const u32* __restrict__ head, u64 n_edges, u32* indeg, u32* outdeg,
                               u32* in_e, u32* out_e, unsigned long long* first_bad) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  const u32 t = tail[i];
  if (t == kNoEdge) return;
  const u32 h = head[i];
  if (tail[i ^ 1] != (h ^ 1u) || head[i ^ 1] != (t ^ 1u)) atomicMin(first_bad, static_cast<unsigned long long>(i));
  atomicAdd(outdeg + t, 1u);
  atomicAdd(indeg + h, 1u);
  out_e[t] = static_cast<u32>(i);  // (the one edge, where the degree is 1: nobody reads it otherwise)
  in_e[h] = static_cast<u32>(i);
}

// cls: 1 = the node is no junction.  succ / has-pred as the reference's two walks see them.
__global__ void successor_kernel(u32 n, const u32* __restrict__ indeg, const u32* __restrict__ outdeg, const u32* __restrict__ in_e,
                                 const u32* __restrict__ out_e, const u32* __restrict__ tail, const u32* __restrict__ head,
                                 u32* __restrict__ succ, u8* __restrict__ cls) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  const bool plain = indeg[u] <= 1 && outdeg[u] <= 1;
  u32 s = kNone;
  u8 c = plain ? 1 : 0;
  if (plain && outdeg[u] == 1) {
    const u32 v = head[out_e[u]];
    if (indeg[v] <= 1 && outdeg[v] <= 1) s = v;
  }
  if (plain && indeg[u] == 1) {
    const u32 p = tail[in_e[u]];
    if (indeg[p] <= 1 && outdeg[p] <= 1) c |= 2;  // has a predecessor in its chain
  }
  succ[u] = s;
  cls[u] = c;
}

// the cut in front of a cycle's creating node (its smallest id): that node loses its predecessor, the node before it its successor
__global__ void cut_cycles_kernel(u32 n, const u8* __restrict__ cyc, const u32* __restrict__ mn, u32* __restrict__ succ,
                                  u8* __restrict__ cls) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n || !cyc[u]) return;
  if (succ[u] == mn[u]) succ[u] = kNone;
  if (u == mn[u]) cls[u] &= 1;
}

struct Rank {
  u32 *ptr, *dist, *endn, *mn;
};
// ptr = the node `dist` steps on, or kNone when the chain ended `dist` steps on at `endn`; mn = the smallest id among the
// nodes the steps passed (the end included once it is reached)
__global__ void rank_init_kernel(u32 n, const u32* __restrict__ succ, Rank r) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  const u32 s = succ[u];
  r.ptr[u] = s;
  r.dist[u] = s != kNone ? 1u : 0u;
  r.endn[u] = u;
  r.mn[u] = u;
}
__global__ void rank_jump_kernel(u32 n, Rank a, Rank b) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  const u32 p = a.ptr[u];
  u32 d = a.dist[u], en = a.endn[u], m = a.mn[u], q = p;
  if (p != kNone) {
    q = a.ptr[p];
    d += a.dist[p];
    en = a.endn[p];
    const u32 mp = a.mn[p];
    m = mp < m ? mp : m;
  }
  b.ptr[u] = q;
  b.dist[u] = d;
  b.endn[u] = en;
  b.mn[u] = m;
}
__global__ void live_kernel(u32 n, const u32* __restrict__ ptr, u8* __restrict__ cyc, u32* n_live) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  const bool live = ptr[u] != kNone;
  cyc[u] = live ? 1 : 0;
  if (live) atomicAdd(n_live, 1u);
}

// the first node of every chain decides for the chain: kept or not, and whether this orientation creates (it holds the
// smallest id of the chain and its pair, which is even)
__global__ void chains_kernel(u32 n, const u8* __restrict__ cls, const u8* __restrict__ cyc, const u32* __restrict__ dist,
                              const u32* __restrict__ mn, u32 epsilon, u8* __restrict__ flag, u32* __restrict__ cbegin) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n || cls[u] != 1) return;  // a junction, or a node with a predecessor
  const u32 nodes = dist[u] + 1;
  const bool circular = cyc[u] != 0;
  if (!circular && nodes < 2) return;
  if (!chain_is_kept(nodes, circular, epsilon)) return;
  const u32 m = mn[u];
  if (m & 1u) return;
  flag[m] = 1;
  cbegin[m] = u;
}

struct ChainView {
  const u32 *succ, *dist, *endn;
  const u8 *cls, *cyc;
};
__global__ void unitig_chains_kernel(u32 n, const u8* __restrict__ flag, const u32* __restrict__ slot, const u32* __restrict__ cbegin,
                                     ChainView c, u32 epsilon, u32* __restrict__ mcount, u8* __restrict__ ucirc,
                                     u32* __restrict__ chain_of_end, u32* __restrict__ chain_len) {
  const u32 m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n || !flag[m]) return;
  const u32 j = 2u * slot[m];
  const u32 b = cbegin[m];
  const u32 nodes = c.dist[b] + 1;
  const bool circular = c.cyc[b] != 0;
  const u32 members = circular ? nodes : nodes - 2u * epsilon;
  mcount[j] = mcount[j + 1] = members;
  ucirc[j] = ucirc[j + 1] = circular ? 1 : 0;
  const u32 end = c.endn[b];
  // the paired chain runs from end ^ 1 to b ^ 1; the paired cycle starts at b ^ 1, so it ends with the pair of b's successor
  const u32 end_rc = (circular && nodes > 1 ? c.succ[b] : b) ^ 1u;
  chain_of_end[end] = j;
  chain_of_end[end_rc] = j + 1;
  chain_len[end] = chain_len[end_rc] = nodes;
}

struct TilingView {
  const u64* seg_off;
  const Segment* seg;
  const u32* cum;
  const u32* len;
};
struct EdgeView {
  const u32 *tail, *head, *length, *indeg, *outdeg, *in_e, *out_e;
};
struct MemberTable {
  u32 *node, *unitig, *len, *seg, *cnt;
};

// every node of a kept chain finds its unitig through the chain's end, its place from its rank
__global__ void members_kernel(u32 n, ChainView c, const u32* __restrict__ chain_of_end, const u32* __restrict__ chain_len,
                               const u8* __restrict__ ucirc, const u64* __restrict__ moff, u32 epsilon, EdgeView g, TilingView t,
                               const u32* __restrict__ count, MemberTable mt, u8* mark, unsigned long long* bad_edge) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n || !(c.cls[u] & 1)) return;
  const u32 end = c.endn[u];
  const u32 jj = chain_of_end[end];
  if (jj == kNone) return;
  const u32 nodes = chain_len[end];
  const u32 pos = nodes - 1 - c.dist[u];
  const bool circular = ucirc[jj] != 0;
  u32 idx = pos, members = nodes;
  if (!circular) {
    if (pos < epsilon || pos >= nodes - epsilon) return;  // a node near a junction
    idx = pos - epsilon;
    members = nodes - 2u * epsilon;
  }
  const u64 at = moff[jj] + idx;
  const bool last = !circular && idx == members - 1;
  const u32 own = t.len[u];
  u32 keep = own;
  if (!last) {
    const u32 oe = g.out_e[u];
    keep = g.length[oe];
    if (keep > own) {
      atomicMin(bad_edge, static_cast<unsigned long long>(oe));
      keep = own;
    }
    mark[oe] = 1;
    mark[oe ^ 1u] = 1;
  } else if (g.outdeg[u]) {
    const u32 oe = g.out_e[u];
    mark[oe] = 1;
    mark[oe ^ 1u] = 1;
  }
  if (!circular && idx == 0 && g.indeg[u]) {
    const u32 ie = g.in_e[u];
    mark[ie] = 1;
    mark[ie ^ 1u] = 1;
  }
  const u64 s0 = t.seg_off[u];
  mt.node[at] = u;
  mt.unitig[at] = jj;
  mt.len[at] = keep;
  mt.seg[at] = prefix_segments(t.cum + s0, static_cast<u32>(t.seg_off[u + 1] - s0), keep);
  mt.cnt[at] = count[u];
}

struct UnitigDev {
  u32 *begin, *end, *count, *length;
  u16* coverage;
  u8* is_unitig;
};
// per pair of new nodes: the segmented sums as differences of the scans, what the constructor and the loop body set, and
// the number of connecting edges
__global__ void unitig_tables_kernel(u32 n_pairs, const u64* __restrict__ moff, const u32* __restrict__ member, const u64* __restrict__ lenscan,
                                     const u64* __restrict__ cntscan, const u8* __restrict__ ucirc, const u16* __restrict__ cov,
                                     const u32* __restrict__ indeg, const u32* __restrict__ outdeg, u32 min_unitig_size, UnitigDev ud,
                                     u32* __restrict__ ecnt, unsigned long long* bad_len) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_pairs) return;
  const bool circular = ucirc[2 * k] != 0;
  for (u32 jj = 2 * k; jj < 2 * k + 2; ++jj) {
    const u64 a = moff[jj], z = moff[jj + 1];
    const u64 bases = lenscan[z] - lenscan[a];
    if (bases > 0xFFFFFFFFULL) atomicMin(bad_len, static_cast<unsigned long long>(jj));
    ud.length[jj] = static_cast<u32>(bases);
    ud.count[jj] = static_cast<u32>(cntscan[z] - cntscan[a]);  // (the difference mod 2^32 is the sum in uint32)
    ud.begin[jj] = member[a];
    ud.end[jj] = circular ? member[a] : member[z - 1];
    ud.is_unitig[jj] = unitig_is_unitig(ud.count[jj], ud.length[jj], min_unitig_size) ? 1 : 0;
  }
  const u32 b = ud.begin[2 * k], en = ud.end[2 * k];
  ud.coverage[2 * k] = ud.coverage[2 * k + 1] = unitig_coverage(cov[b], cov[en]);  // (rc_unitig->coverage = coverage)
  ecnt[k] = circular ? 0u : (indeg[b] ? 2u : 0u) + (outdeg[en] ? 2u : 0u);
}

// the connecting edges in factory order (common.cc:128-164): the in-edge, its pair, the out-edge, its pair
__global__ void connect_kernel(u32 n_pairs, u32 first_node, const u8* __restrict__ ucirc, UnitigDev ud, EdgeView g, const u32* __restrict__ node_len,
                               const u32* __restrict__ eoff, u32* __restrict__ etail, u32* __restrict__ ehead, u32* __restrict__ elen) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_pairs || ucirc[2 * k]) return;
  const u32 b = ud.begin[2 * k], en = ud.end[2 * k];
  const u32 id = first_node + 2 * k, id_rc = id + 1;
  u32 x = eoff[k];
  if (g.indeg[b]) {
    const u32 ie = g.in_e[b];
    etail[x] = g.tail[ie];
    ehead[x] = id;
    elen[x] = g.length[ie];
    etail[x + 1] = id_rc;
    ehead[x + 1] = g.head[ie ^ 1u];
    elen[x + 1] = g.length[ie ^ 1u] + ud.length[2 * k + 1] - node_len[b ^ 1u];
    x += 2;
  }
  if (g.outdeg[en]) {
    const u32 oe = g.out_e[en];
    etail[x] = id;
    ehead[x] = g.head[oe];
    elen[x] = g.length[oe] + ud.length[2 * k] - node_len[en];
    etail[x + 1] = g.tail[oe ^ 1u];
    ehead[x + 1] = id_rc;
    elen[x + 1] = g.length[oe ^ 1u];
  }
}

// the new nodes' segment lists: per member the prefix of its own list, behind the members in front of it
__global__ void append_segments_kernel(u64 n_members, MemberTable mt, const u64* __restrict__ moff, const u64* __restrict__ lenscan,
                                       const u64* __restrict__ segscan, TilingView t, u64 old_segs, Segment* __restrict__ seg_out,
                                       u32* __restrict__ cum_out) {
  const u64 at = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (at >= n_members) return;
  const u32 u = mt.node[at];
  const u32 keep = mt.len[at], segs = mt.seg[at];
  const u32 base = static_cast<u32>(lenscan[at] - lenscan[moff[mt.unitig[at]]]);
  const u64 s0 = t.seg_off[u];
  const u64 d0 = old_segs + segscan[at];
  for (u32 i = 0; i < segs; ++i) {
    seg_out[d0 + i] = prefix_segment(t.seg + s0, t.cum + s0, i, keep);
    cum_out[d0 + i] = base + t.cum[s0 + i];
  }
}
__global__ void append_nodes_kernel(u32 n_new, u32 first_node, const u64* __restrict__ moff, const u64* __restrict__ segscan, u64 old_segs,
                                    const u32* __restrict__ ulen, u64* __restrict__ seg_off, u32* __restrict__ len) {
  const u32 jj = blockIdx.x * blockDim.x + threadIdx.x;
  if (jj > n_new) return;
  seg_off[static_cast<u64>(first_node) + jj] = old_segs + segscan[moff[jj]];
  if (jj < n_new) len[static_cast<u64>(first_node) + jj] = ulen[jj];
}

// per member of a node path: the bases it contributes (path_member_keep) and the number of its segments they keep
__global__ void path_members_kernel(u64 n_members, const u32* __restrict__ node, const u32* __restrict__ label, const u32* __restrict__ path,
                                    const u64* __restrict__ moff, TilingView t, u32* __restrict__ mlen, u32* __restrict__ mseg) {
  const u64 at = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (at >= n_members) return;
  const u32 u = node[at];
  const u32 keep = path_member_keep(label[at], t.len[u], at + 1 == moff[path[at] + 1]);
  const u64 s0 = t.seg_off[u];
  mlen[at] = keep;
  mseg[at] = prefix_segments(t.cum + s0, static_cast<u32>(t.seg_off[u + 1] - s0), keep);
}

// one lane per packed word of the output read set: read i = node nodes[i]
__global__ void pack_tilings_kernel(const u32* __restrict__ nodes, const u64* __restrict__ woff, u32 n_reads, u64 n_words, TilingView t,
                                    const u64* __restrict__ packed, const u64* __restrict__ read_word_off, u64* __restrict__ out) {
  const u64 wi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (wi >= n_words) return;
  u32 lo = 0, hi = n_reads;  // the read of this word: the last i with woff[i] <= wi
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (woff[mid] <= wi) lo = mid;
    else hi = mid;
  }
  const u32 u = nodes[lo];
  const u64 s0 = t.seg_off[u];
  out[wi] = tiling_word(t.seg + s0, t.cum + s0, static_cast<u32>(t.seg_off[u + 1] - s0), t.len[u], static_cast<u32>(wi - woff[lo]) * 32u,
                        packed, read_word_off);
}

// one lane per packed word of slices [first, first + count) of the lists: slice s = InflateData(begin[s], length[s]) of
// node[s] with length[s] already clamped (slice_length); woff[s] = its first word, base = woff[first]
__global__ void pack_slices_kernel(const u32* __restrict__ node, const u32* __restrict__ begin, const u32* __restrict__ length,
                                   const u64* __restrict__ woff, u64 first, u64 count, u64 n_words, TilingView t,
                                   const u64* __restrict__ packed, const u64* __restrict__ read_word_off, u64* __restrict__ out) {
  const u64 wi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (wi >= n_words) return;
  const u64 at = woff[first] + wi;
  u64 lo = first, hi = first + count;  // the slice of this word: the last s with woff[s] <= at (slices of no words own none)
  while (hi - lo > 1) {
    const u64 mid = lo + (hi - lo) / 2;
    if (woff[mid] <= at) lo = mid;
    else hi = mid;
  }
  const u32 u = node[lo];
  const u64 s0 = t.seg_off[u];
  out[wi] = slice_word(t.seg + s0, t.cum + s0, static_cast<u32>(t.seg_off[u + 1] - s0), begin[lo], length[lo], static_cast<u32>(at - woff[lo]),
                       packed, read_word_off);
}

int rounds_for(u32 n) {  // ceil(log2 n) + 1
  int r = 0;
  while (r < 32 && (1ULL << r) < n) ++r;
  return r + 1;
}

// steps to the end, the end and the smallest id of every node's way along succ; returns which of the two sets holds them
int rank_chains(Engine& e, u32 n, const u32* d_succ) {
  UnitigScratch& S = e.unitig;
  hipStream_t s = e.stream;
  Rank r[2];
  for (int i = 0; i < 2; ++i)
    r[i] = Rank{S.ptr[i].get<u32>(n), S.dist[i].get<u32>(n), S.endn[i].get<u32>(n), S.mn[i].get<u32>(n)};
  rank_init_kernel<<<div_up(n, 256), 256, 0, s>>>(n, d_succ, r[0]);
  RVN_LAUNCH_CHECK();
  int a = 0;
  for (int round = 0; round < rounds_for(n); ++round, a ^= 1) {
    rank_jump_kernel<<<div_up(n, 256), 256, 0, s>>>(n, r[a], r[a ^ 1]);
    RVN_LAUNCH_CHECK();
  }
  return a;
}

TilingView view_of(const TilingDev& T) { return TilingView{T.seg_off.as<u64>(), T.seg.as<Segment>(), T.cum.as<u32>(), T.len.as<u32>()}; }

template <typename V>
void fetch_vec(std::vector<V>& dst, const void* d_src, size_t count, hipStream_t s) {
  dst.resize(count);
  if (count) RVN_HIP(hipMemcpyAsync(dst.data(), d_src, count * sizeof(V), hipMemcpyDeviceToHost, s));
}

// host arrays -> the tiling on the device; seg / cum / len are complete and checked
void tiling_upload(Engine& e, const ReadsDev& R, const std::vector<u64>& seg_off, const std::vector<Segment>& seg, const std::vector<u32>& cum,
                   std::vector<u32>&& len, TilingDev& T) {
  hipStream_t s = e.stream;
  const u32 n = static_cast<u32>(len.size());
  upload(T.seg_off, seg_off.data(), seg_off.size(), s);
  upload(T.seg, seg.data(), seg.size(), s);
  upload(T.cum, cum.data(), cum.size(), s);
  upload(T.len, len.data(), len.size(), s);
  RVN_HIP(rvn_stream_sync(s));
  T.n_nodes = n;
  T.n_segs = seg.size();
  T.reads_serial = R.serial;
  T.h_len = std::move(len);
}

}  // namespace

void tiling_from_segments(Engine& e, const ReadsDev& R, u32 n_nodes, const u64* h_seg_off, const u32* h_read, const u32* h_begin,
                          const u32* h_length, const u8* h_strand, TilingDev& T) {
  const std::string who = "[raven_hip] rvn_tiling_from_segments: ";
  if (h_seg_off[0] != 0) throw std::invalid_argument(who + "offsets must start at 0");
  for (u32 u = 0; u < n_nodes; ++u)
    if (h_seg_off[u + 1] < h_seg_off[u]) throw std::invalid_argument(who + "offsets must not decrease");
  const u64 S = h_seg_off[n_nodes];
  std::vector<Segment> seg(S);
  std::vector<u32> cum(S), len(n_nodes);
  for (u32 u = 0; u < n_nodes; ++u) {
    u64 bases = 0;
    for (u64 i = h_seg_off[u]; i < h_seg_off[u + 1]; ++i) {
      if (h_read[i] >= R.n) throw std::invalid_argument(who + "segment " + std::to_string(i) + " names an unknown read");
      if (static_cast<u64>(h_begin[i]) + h_length[i] > R.h_len[h_read[i]])
        throw std::invalid_argument(who + "segment " + std::to_string(i) + " runs past its read");
      if (h_strand[i] > 1) throw std::invalid_argument(who + "segment " + std::to_string(i) + " has a strand other than 0 or 1");
      seg[i] = Segment{h_read[i], h_begin[i], h_length[i], h_strand[i]};
      cum[i] = static_cast<u32>(bases);
      bases += h_length[i];
      if (bases > 0xFFFFFFFFULL) throw std::invalid_argument(who + "node " + std::to_string(u) + " has 2^32 bases or more");
    }
    len[u] = static_cast<u32>(bases);
  }
  tiling_upload(e, R, std::vector<u64>(h_seg_off, h_seg_off + n_nodes + 1), seg, cum, std::move(len), T);
}

void tiling_from_piles(Engine& e, const ReadsDev& R, u32 n_nodes, const u32* h_node_pile, u32 n_piles, const u32* h_begin,
                       const u32* h_end, TilingDev& T) {
  const std::string who = "[raven_hip] rvn_tiling_from_piles: ";
  if (n_piles > R.n) throw std::invalid_argument(who + "more piles than reads (pile i is read i)");
  std::vector<u64> seg_off(static_cast<size_t>(n_nodes) + 1);
  std::vector<Segment> seg(n_nodes);
  std::vector<u32> cum(n_nodes, 0), len(n_nodes);
  for (u32 u = 0; u < n_nodes; ++u) {
    const u32 p = h_node_pile[u];
    if (p >= n_piles) throw std::invalid_argument(who + "node " + std::to_string(u) + " names an unknown pile");
    if (h_end[p] < h_begin[p] || h_end[p] > R.h_len[p])
      throw std::invalid_argument(who + "the segment of node " + std::to_string(u) + " runs past its read");
    seg_off[u] = u;
    seg[u] = Segment{p, h_begin[p], h_end[p] - h_begin[p], u & 1u};
    len[u] = seg[u].length;
  }
  seg_off[n_nodes] = n_nodes;
  tiling_upload(e, R, seg_off, seg, cum, std::move(len), T);
}

void tiling_fetch(const TilingDev& T, u64* seg_off, u32* read, u32* begin, u32* length, u8* strand, u32* node_length) {
  if (seg_off) RVN_HIP(hipMemcpy(seg_off, T.seg_off.ptr, (static_cast<size_t>(T.n_nodes) + 1) * 8, hipMemcpyDeviceToHost));
  if (node_length && T.n_nodes) std::memcpy(node_length, T.h_len.data(), static_cast<size_t>(T.n_nodes) * 4);
  if (!T.n_segs || !(read || begin || length || strand)) return;
  std::vector<Segment> seg(T.n_segs);
  RVN_HIP(hipMemcpy(seg.data(), T.seg.ptr, T.n_segs * sizeof(Segment), hipMemcpyDeviceToHost));
  for (u64 i = 0; i < T.n_segs; ++i) {
    if (read) read[i] = seg[i].read;
    if (begin) begin[i] = seg[i].begin;
    if (length) length[i] = seg[i].length;
    if (strand) strand[i] = static_cast<u8>(seg[i].strand);
  }
}

void graph_create_unitigs(Engine& e, const GraphDev& g, TilingDev& T, const u32* h_count, const u16* h_coverage, u32 epsilon,
                          u32 min_unitig_size, UnitigTables& out) {
  const std::string who = "[raven_hip] rvn_graph_create_unitigs: ";
  hipStream_t s = e.stream;
  UnitigScratch& S = e.unitig;
  const u32 n = g.n_nodes;
  const u64 E = g.n_edges;
  if (T.n_nodes < n) throw std::invalid_argument(who + "the tiling has fewer nodes (" + std::to_string(T.n_nodes) + ") than the graph");
  if (T.n_nodes > n)
    throw std::invalid_argument(who + "the tiling has more nodes (" + std::to_string(T.n_nodes) + ") than the graph: the new nodes' ids would not be theirs");
  if (epsilon > kMaxEpsilon) throw std::invalid_argument(who + "epsilon above 2^30");
  out = UnitigTables();
  out.first_node = n;
  out.first_edge = E;
  out.marked.assign(E, 0);
  out.member_off.assign(1, 0);
  if (n == 0 || g.n_live == 0) return;

  // degrees, the one in- and out-edge, pair symmetry
  const size_t n2 = static_cast<size_t>(n) + 2;
  u32* d_indeg = S.indeg.get<u32>(n2);
  u32* d_outdeg = S.outdeg.get<u32>(n2);
  u32* d_in_e = S.in_e.get<u32>(n2);
  u32* d_out_e = S.out_e.get<u32>(n2);
  unsigned long long* d_err = S.err.get<unsigned long long>(4);  // asymmetric edge, long chain edge, long unitig, live pointers
  RVN_HIP(hipMemsetAsync(d_indeg, 0, n2 * 4, s));
  RVN_HIP(hipMemsetAsync(d_outdeg, 0, n2 * 4, s));
  RVN_HIP(hipMemsetAsync(d_err, 0xFF, 24, s));
  RVN_HIP(hipMemsetAsync(d_err + 3, 0, 8, s));
  degrees_kernel<<<div_up(E, 256), 256, 0, s>>>(g.tail.as<u32>(), g.head.as<u32>(), E, d_indeg, d_outdeg, d_in_e, d_out_e, d_err);
  RVN_LAUNCH_CHECK();
  const u64 asym = read_back(e, d_err, 8);
  if (asym != ~0ULL)
    throw std::invalid_argument(who + "edge " + std::to_string(asym) + " and its pair slot are not a pair (tail[e ^ 1] != head[e] ^ 1 or head[e ^ 1] != tail[e] ^ 1)");
  const EdgeView G{g.tail.as<u32>(), g.head.as<u32>(), g.length.as<u32>(), d_indeg, d_outdeg, d_in_e, d_out_e};

  // chains: successor, ranking, cycles cut at their creating node and ranked again
  u32* d_succ = S.succ.get<u32>(n2);
  u8* d_cls = S.cls.get<u8>(n2);
  u8* d_cyc = S.cyc.get<u8>(n2);
  u8* d_flag = S.flag.get<u8>(n2 + 16);
  successor_kernel<<<div_up(n, 256), 256, 0, s>>>(n, d_indeg, d_outdeg, d_in_e, d_out_e, G.tail, G.head, d_succ, d_cls);
  RVN_LAUNCH_CHECK();
  int a = rank_chains(e, n, d_succ);
  u32* d_live = reinterpret_cast<u32*>(d_err + 3);
  live_kernel<<<div_up(n, 256), 256, 0, s>>>(n, S.ptr[a].as<u32>(), d_cyc, d_live);
  RVN_LAUNCH_CHECK();
  if (read_back(e, d_live, 4) != 0) {
    cut_cycles_kernel<<<div_up(n, 256), 256, 0, s>>>(n, d_cyc, S.mn[a].as<u32>(), d_succ, d_cls);
    RVN_LAUNCH_CHECK();
    a = rank_chains(e, n, d_succ);
    RVN_HIP(hipMemsetAsync(d_live, 0, 4, s));
    live_kernel<<<div_up(n, 256), 256, 0, s>>>(n, S.ptr[a].as<u32>(), d_flag, d_live);
    RVN_LAUNCH_CHECK();
    if (read_back(e, d_live, 4) != 0) throw std::runtime_error(who + "a chain did not end after its cycle was cut");
  }
  const ChainView C{d_succ, S.dist[a].as<u32>(), S.endn[a].as<u32>(), d_cls, d_cyc};

  // creation order: the creating nodes of the kept chains, numbered in ascending id
  u32* d_cbegin = S.cbegin.get<u32>(n2);
  RVN_HIP(hipMemsetAsync(d_flag, 0, n, s));
  chains_kernel<<<div_up(n, 256), 256, 0, s>>>(n, d_cls, d_cyc, C.dist, S.mn[a].as<u32>(), epsilon, d_flag, d_cbegin);
  RVN_LAUNCH_CHECK();
  const KeptSlots ks = kept_slots(e, d_flag, n, S.slot);
  const u32 n_pairs = static_cast<u32>(ks.kept);
  if (n_pairs == 0) return;
  const u32 U = 2 * n_pairs;
  if (static_cast<u64>(n) + U > (1ULL << 31)) throw std::invalid_argument(who + "more than 2^31 nodes with the new ones");

  u32* d_mcount = S.mcount.get<u32>(static_cast<size_t>(U) + 2);
  u64* d_moff = S.moff.get<u64>(static_cast<size_t>(U) + 2);
  u8* d_ucirc = S.ucirc.get<u8>(static_cast<size_t>(U) + 2);
  u32* d_chain_of_end = S.chain_of_end.get<u32>(n2);
  u32* d_chain_len = S.chain_len.get<u32>(n2);
  RVN_HIP(hipMemsetAsync(d_chain_of_end, 0xFF, n2 * 4, s));
  unitig_chains_kernel<<<div_up(n, 256), 256, 0, s>>>(n, d_flag, ks.slot, d_cbegin, C, epsilon, d_mcount, d_ucirc, d_chain_of_end, d_chain_len);
  RVN_LAUNCH_CHECK();
  exclusive_scan_u32_u64(d_mcount, d_moff, U, e.scratch.scan_tmp, s);
  const u64 M = read_back(e, d_moff + U, 8);

  // members, their prefixes, the marks
  const u32* d_count = upload(S.count, h_count, n, s);
  const u16* d_cov = upload(S.cov, h_coverage, n, s);
  const MemberTable mt{S.members.get<u32>(M + 1), S.mnode.get<u32>(M + 1), S.mlen.get<u32>(M + 1), S.mseg.get<u32>(M + 1), S.mcnt.get<u32>(M + 1)};
  u8* d_mark = S.mark.get<u8>(E + 16);
  RVN_HIP(hipMemsetAsync(d_mark, 0, E, s));
  const TilingView tv = view_of(T);
  members_kernel<<<div_up(n, 256), 256, 0, s>>>(n, C, d_chain_of_end, d_chain_len, d_ucirc, d_moff, epsilon, G, tv, d_count, mt, d_mark, d_err + 1);
  RVN_LAUNCH_CHECK();
  u64* d_lenscan = S.lenscan.get<u64>(M + 1);
  u64* d_segscan = S.segscan.get<u64>(M + 1);
  u64* d_cntscan = S.cntscan.get<u64>(M + 1);
  exclusive_scan_u32_u64(mt.len, d_lenscan, M, e.scratch.scan_tmp, s);
  exclusive_scan_u32_u64(mt.seg, d_segscan, M, e.scratch.scan_tmp, s);
  exclusive_scan_u32_u64(mt.cnt, d_cntscan, M, e.scratch.scan_tmp, s);
  const u64 long_edge = read_back(e, d_err + 1, 8);
  if (long_edge != ~0ULL) throw std::invalid_argument(who + "chain edge " + std::to_string(long_edge) + " is longer than its tail's sequence");

  // the new nodes' tables and the connecting edges
  const UnitigDev ud{S.ubegin.get<u32>(U), S.uend.get<u32>(U), S.ucount.get<u32>(U), S.ulen.get<u32>(U), S.ucov.get<u16>(U), S.uis.get<u8>(U)};
  u32* d_ecnt = S.ecnt.get<u32>(static_cast<size_t>(n_pairs) + 1);
  u32* d_eoff = S.eoff.get<u32>(static_cast<size_t>(n_pairs) + 1);
  unitig_tables_kernel<<<div_up(n_pairs, 256), 256, 0, s>>>(n_pairs, d_moff, mt.node, d_lenscan, d_cntscan, d_ucirc, d_cov, d_indeg, d_outdeg,
                                                            min_unitig_size, ud, d_ecnt, d_err + 2);
  RVN_LAUNCH_CHECK();
  exclusive_scan_u32_u32(d_ecnt, d_eoff, n_pairs, e.scratch.scan_tmp, s);
  const u64 long_unitig = read_back(e, d_err + 2, 8);
  if (long_unitig != ~0ULL)
    throw std::invalid_argument(who + "new node " + std::to_string(static_cast<u64>(n) + long_unitig) + " would have 2^32 bases or more");
  const u64 NE = read_back(e, d_eoff + n_pairs, 4);
  if (E + NE >= 0xFFFFFFFFULL) throw std::invalid_argument(who + "2^32 edge slots or more with the new ones");
  u32* d_etail = S.etail.get<u32>(NE + 1);
  u32* d_ehead = S.ehead.get<u32>(NE + 1);
  u32* d_elen = S.elen.get<u32>(NE + 1);
  connect_kernel<<<div_up(n_pairs, 256), 256, 0, s>>>(n_pairs, n, d_ucirc, ud, G, tv.len, d_eoff, d_etail, d_ehead, d_elen);
  RVN_LAUNCH_CHECK();

  // the tables to the host
  fetch_vec(out.begin, ud.begin, U, s);
  fetch_vec(out.end, ud.end, U, s);
  fetch_vec(out.count, ud.count, U, s);
  fetch_vec(out.length, ud.length, U, s);
  fetch_vec(out.coverage, ud.coverage, U, s);
  fetch_vec(out.is_unitig, ud.is_unitig, U, s);
  fetch_vec(out.is_circular, d_ucirc, U, s);
  fetch_vec(out.member_off, d_moff, static_cast<size_t>(U) + 1, s);
  fetch_vec(out.members, mt.node, M, s);
  fetch_vec(out.marked, d_mark, E, s);
  fetch_vec(out.edge_tail, d_etail, NE, s);
  fetch_vec(out.edge_head, d_ehead, NE, s);
  fetch_vec(out.edge_length, d_elen, NE, s);
  const u64 new_segs = read_back(e, d_segscan + M, 8);  // (synchronises: the tables are complete)

  // the new nodes' segment lists behind the tiling's: from here on nothing is refused
  const u64 old_segs = T.n_segs;
  T.seg.grow_keeping(old_segs * sizeof(Segment), (old_segs + new_segs + 1) * sizeof(Segment), s);
  T.cum.grow_keeping(old_segs * 4, (old_segs + new_segs + 1) * 4, s);
  T.seg_off.grow_keeping((static_cast<size_t>(n) + 1) * 8, (static_cast<size_t>(n) + U + 2) * 8, s);
  T.len.grow_keeping(static_cast<size_t>(n) * 4, (static_cast<size_t>(n) + U + 1) * 4, s);
  const TilingView grown = view_of(T);
  append_segments_kernel<<<div_up(M, 256), 256, 0, s>>>(M, mt, d_moff, d_lenscan, d_segscan, grown, old_segs, T.seg.as<Segment>(), T.cum.as<u32>());
  RVN_LAUNCH_CHECK();
  append_nodes_kernel<<<div_up(static_cast<u64>(U) + 1, 256), 256, 0, s>>>(U, n, d_moff, d_segscan, old_segs, ud.length, T.seg_off.as<u64>(), T.len.as<u32>());
  RVN_LAUNCH_CHECK();
  RVN_HIP(rvn_stream_sync(s));
  T.n_nodes = n + U;
  T.n_segs = old_segs + new_segs;
  T.h_len.insert(T.h_len.end(), out.length.begin(), out.length.end());
}

void tiling_as_reads(Engine& e, const TilingDev& T, const ReadsDev& R, const u32* h_nodes, u32 n, ReadsDev& out) {
  const std::string who = "[raven_hip] rvn_tiling_as_reads: ";
  hipStream_t s = e.stream;
  UnitigScratch& S = e.unitig;
  if (T.reads_serial != R.serial) throw std::invalid_argument(who + "the tiling was made for another read set");
  std::vector<u64> woff(static_cast<size_t>(n) + 1, 0);
  std::vector<u32> lens(n);
  u64 total = 0;
  for (u32 i = 0; i < n; ++i) {
    if (h_nodes[i] >= T.n_nodes) throw std::invalid_argument(who + "node " + std::to_string(h_nodes[i]) + " is not in the tiling");
    lens[i] = T.h_len[h_nodes[i]];
    total += lens[i];
    woff[i + 1] = woff[i] + (static_cast<u64>(lens[i]) + 31) / 32;
  }
  const u64 n_words = woff[n];
  u64* d_packed = out.packed.get<u64>(n_words + 2);
  if (n_words) {
    const u32* d_nodes = upload(S.nodes, h_nodes, n, s);
    const u64* d_woff = upload(S.woff, woff.data(), woff.size(), s);
    pack_tilings_kernel<<<div_up(n_words, 256), 256, 0, s>>>(d_nodes, d_woff, n, n_words, view_of(T), R.packed.as<u64>(), R.word_off.as<u64>(), d_packed);
    RVN_LAUNCH_CHECK();
  }
  RVN_HIP(hipMemsetAsync(d_packed + n_words, 0, 16, s));
  RVN_HIP(rvn_stream_sync(s));
  reads_finish_device_set(e, out, woff, lens, nullptr, total);
}

void pack_slices_dev(Engine& e, const TilingDev& T, const ReadsDev& R, const u32* d_node, const u32* d_begin, const u32* d_length,
                     const u64* d_woff, u64 first, u64 count, u64 n_words, u64* d_out) {
  if (n_words == 0) return;
  RVN_KLAUNCH(kKSlicePack, pack_slices_kernel<<<div_up(n_words, 256), 256, 0, e.stream>>>(d_node, d_begin, d_length, d_woff, first, count, n_words,
                                                                                          view_of(T), R.packed.as<u64>(), R.word_off.as<u64>(), d_out));
}

// What is refused is found on the host, from the node lengths the tiling keeps, before the first launch.
void tiling_slices_as_reads(Engine& e, const TilingDev& T, const ReadsDev& R, u32 n, const u32* h_node, const u32* h_begin,
                            const u32* h_length, ReadsDev& out) {
  const std::string who = "[raven_hip] rvn_tiling_slices_as_reads: ";
  hipStream_t s = e.stream;
  UnitigScratch& S = e.unitig;
  if (T.reads_serial != R.serial) throw std::invalid_argument(who + "the tiling was made for another read set");
  std::vector<u64> woff(static_cast<size_t>(n) + 1, 0);
  std::vector<u32> lens(n);
  u64 total = 0;
  for (u32 i = 0; i < n; ++i) {
    if (h_node[i] >= T.n_nodes) throw std::invalid_argument(who + "node " + std::to_string(h_node[i]) + " (slice " + std::to_string(i) + ") is not in the tiling");
    lens[i] = slice_length(T.h_len[h_node[i]], h_begin[i], h_length[i]);
    total += lens[i];
    woff[i + 1] = woff[i] + (static_cast<u64>(lens[i]) + 31) / 32;
  }
  const u64 n_words = woff[n];
  if (n_words >= (1ULL << 32)) throw std::invalid_argument(who + "the slices have 2^32 packed words or more");
  u64* d_packed = out.packed.get<u64>(n_words + 2);
  if (n_words) {
    const u32* d_node = upload(S.nodes, h_node, n, s);
    const u32* d_begin = upload(S.mlen, h_begin, n, s);
    const u32* d_len = upload(S.mseg, lens.data(), n, s);
    const u64* d_woff = upload(S.woff, woff.data(), woff.size(), s);
    pack_slices_dev(e, T, R, d_node, d_begin, d_len, d_woff, 0, n, n_words, d_packed);
  }
  RVN_HIP(hipMemsetAsync(d_packed + n_words, 0, 16, s));
  RVN_HIP(rvn_stream_sync(s));  // (the host tables above are locals)
  reads_finish_device_set(e, out, woff, lens, nullptr, total);
}

// A path is a node that is never appended: its segment list is built as CreateUnitigs builds a unitig's (the members'
// prefixes one behind the other: append_segments_kernel), in a tiling of its own with one node per path, and packed by
// pack_tilings_kernel.  What is refused is found on the host, from the node lengths it keeps, before the first launch.
void tiling_paths_as_reads(Engine& e, const TilingDev& T, const ReadsDev& R, u32 n_paths, const u64* h_off, const u32* h_node,
                           const u32* h_label, ReadsDev& out) {
  const std::string who = "[raven_hip] rvn_tiling_paths_as_reads: ";
  hipStream_t s = e.stream;
  UnitigScratch& S = e.unitig;
  if (T.reads_serial != R.serial) throw std::invalid_argument(who + "the tiling was made for another read set");
  std::vector<u64> woff(static_cast<size_t>(n_paths) + 1, 0), moff(static_cast<size_t>(n_paths) + 1, 0);
  std::vector<u32> lens(n_paths);
  for (u32 p = 0; p < n_paths; ++p) {
    if (h_off[p + 1] < h_off[p]) throw std::invalid_argument(who + "offsets must not decrease (path " + std::to_string(p) + ")");
    if (h_off[p + 1] == h_off[p]) throw std::invalid_argument(who + "path " + std::to_string(p) + " is empty");
  }
  const u64 m0 = n_paths ? h_off[0] : 0;
  const u64 M = n_paths ? h_off[n_paths] - m0 : 0;
  std::vector<u32> path_of(M);
  u64 total = 0;
  for (u32 p = 0; p < n_paths; ++p) {
    u64 bases = 0;
    for (u64 i = h_off[p]; i < h_off[p + 1]; ++i) {
      if (h_node[i] >= T.n_nodes)
        throw std::invalid_argument(who + "node " + std::to_string(h_node[i]) + " (member " + std::to_string(i) + ") is not in the tiling");
      bases += path_member_keep(h_label[i], T.h_len[h_node[i]], i + 1 == h_off[p + 1]);
      path_of[i - m0] = p;
    }
    if (bases > 0xFFFFFFFFULL) throw std::invalid_argument(who + "path " + std::to_string(p) + " has 2^32 bases or more");
    lens[p] = static_cast<u32>(bases);
    total += bases;
    woff[p + 1] = woff[p] + (bases + 31) / 32;
    moff[p + 1] = h_off[p + 1] - m0;
  }
  const u64 n_words = woff[n_paths];
  u64* d_packed = out.packed.get<u64>(n_words + 2);
  if (n_words) {
    // members: what each keeps, the scans of bases and segments
    const MemberTable mt{upload(S.members, h_node + m0, M, s), upload(S.mnode, path_of.data(), M, s), S.mlen.get<u32>(M + 1),
                         S.mseg.get<u32>(M + 1), nullptr};
    const u32* d_label = upload(S.mcnt, h_label + m0, M, s);
    const u64* d_moff = upload(S.moff, moff.data(), moff.size(), s);
    const TilingView tv = view_of(T);
    RVN_KLAUNCH(kKPathTiling, path_members_kernel<<<div_up(M, 256), 256, 0, s>>>(M, mt.node, d_label, mt.unitig, d_moff, tv, mt.len, mt.seg));
    u64* d_lenscan = S.lenscan.get<u64>(M + 1);
    u64* d_segscan = S.segscan.get<u64>(M + 1);
    exclusive_scan_u32_u64(mt.len, d_lenscan, M, e.scratch.scan_tmp, s);
    exclusive_scan_u32_u64(mt.seg, d_segscan, M, e.scratch.scan_tmp, s);
    const u64 segs = read_back(e, d_segscan + M, 8);
    // the paths' own tiling: node p = path p
    Segment* d_seg = S.pseg.get<Segment>(segs + 1);
    u32* d_cum = S.pcum.get<u32>(segs + 1);
    u64* d_seg_off = S.pseg_off.get<u64>(static_cast<size_t>(n_paths) + 2);
    u32* d_len = S.plen.get<u32>(static_cast<size_t>(n_paths) + 1);
    const u32* d_lens = upload(S.ulen, lens.data(), n_paths, s);
    RVN_KLAUNCH(kKPathTiling, append_segments_kernel<<<div_up(M, 256), 256, 0, s>>>(M, mt, d_moff, d_lenscan, d_segscan, tv, 0, d_seg, d_cum));
    RVN_KLAUNCH(kKPathTiling, append_nodes_kernel<<<div_up(static_cast<u64>(n_paths) + 1, 256), 256, 0, s>>>(n_paths, 0, d_moff, d_segscan, 0, d_lens, d_seg_off, d_len));
    std::vector<u32> iota(n_paths);
    for (u32 p = 0; p < n_paths; ++p) iota[p] = p;
    const u32* d_nodes = upload(S.nodes, iota.data(), n_paths, s);
    const u64* d_woff = upload(S.woff, woff.data(), woff.size(), s);
    RVN_KLAUNCH(kKPathTiling, pack_tilings_kernel<<<div_up(n_words, 256), 256, 0, s>>>(d_nodes, d_woff, n_paths, n_words, TilingView{d_seg_off, d_seg, d_cum, d_len},
                                                             R.packed.as<u64>(), R.word_off.as<u64>(), d_packed));
  }
  RVN_HIP(hipMemsetAsync(d_packed + n_words, 0, 16, s));
  RVN_HIP(rvn_stream_sync(s));  // (the host tables above are locals)
  reads_finish_device_set(e, out, woff, lens, nullptr, total);
}

}  // namespace rvn
