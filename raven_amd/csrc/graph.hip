// graph.hip — the assembly graph as an edge table on the device (engine.h: GraphDev; rules: graph_rules.h).
//   construct    raven::ConstructAssemblyGraph (RavenLib/src/construct.cc:561-648): node ids = a prefix sum over the valid
//                piles, OverlapFinalize on every overlap (one thread each), the survivors compacted in order, two edges
//                per survivor in closed form.
//   out-lists    one CSR by tail with two orders of a node's out-edges: by edge id (the reference's outedges vectors:
//                Edge::Edge appends, RemoveEdges keeps the relative order) and by (head, edge id), in which the last of
//                a run of equal heads is what `candidate[head] = jt` ends up with.  Both are stable radix sorts of the
//                edge ids; empty slots sort behind everything.  The second is made by the first transitive marking.
//   transitive   RemoveTransitiveEdges' marking (assemble.cc:36-56): one wave per node v; the (jt, kt) pairs of 64
//                out-edges jt at a time are flattened over the lanes through a prefix sum of the heads' out-degrees kept
//                in LDS, so neither a long out-list of v nor one of a head serialises on a lane.  The candidate of
//                head(kt) is a binary search in v's (head, id) order — no list is assumed to fit anywhere.  Marks are
//                byte stores of 1.  The reference's marked_edges set is later ITERATED, so the order in which it first
//                receives each id matters: every mark also takes part in a 64-bit atomicMin of (v, position of jt), and a
//                second sweep, among the marks of that (v, jt) only, in one of (position of kt, own-or-pair); the marked
//                ids sorted by the two keys are the insertion sequence.
//   long edges   RemoveLongEdges' marking loop (assemble.cc:708-721): one wave per node of out-degree >= 2, the
//                smallest weight among the OTHER out-edges of each edge from the node's smallest, its multiplicity and
//                the smallest of the rest.
// Every loop is bounded by the CSR offsets; no wave waits on another.
#include <cstring>
#include <vector>

#include "abi.h"
#include "graph_rules.h"
#include "wave.h"

namespace rvn {

namespace {

constexpr u32 kGraphMaxBlocks = 1u << 20;

int bits_for(u64 x) {
  int b = 0;
  while (b < 64 && (x >> b) != 0) ++b;
  return b;
}

__global__ void valid_flags_kernel(const u8* __restrict__ invalid, u32 n, u8* __restrict__ valid) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) valid[i] = invalid[i] ? 0 : 1;
}
__global__ void node_ids_kernel(const u8* __restrict__ invalid, const u32* __restrict__ slot, const u16* __restrict__ median, u32 n,
                                i32* __restrict__ seq_to_node, u32* __restrict__ node_pile, u16* __restrict__ node_cov) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (invalid[i]) {
    seq_to_node[i] = -1;
    return;
  }
  const u32 node = 2u * slot[i];
  seq_to_node[i] = static_cast<i32>(node);
  node_pile[node] = node_pile[node + 1] = i;
  node_cov[node] = node_cov[node + 1] = median[i];
}
// OverlapFinalize in place; an overlap that finalizes on an invalid pile is reported (the smallest index), not kept
__global__ void finalize_kernel(Overlap* __restrict__ ovl, u64 m, const PileRegion* __restrict__ reg, u8* __restrict__ keep,
                                unsigned long long* first_bad) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  Overlap o = ovl[i];
  const PileRegion L = reg[o.lhs_id], R = reg[o.rhs_id];
  bool k = overlap_finalize(o, L, R);
  if (k && (L.invalid || R.invalid)) {
    atomicMin(first_bad, static_cast<unsigned long long>(i));
    k = false;
  }
  ovl[i] = o;
  keep[i] = k ? 1 : 0;
}
__global__ void edge_source_kernel(const u8* __restrict__ keep, const u32* __restrict__ slot, u64 m, u64* __restrict__ edge_overlap) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < m && keep[i]) edge_overlap[slot[i]] = i;
}
__global__ void edges_kernel(const Overlap* __restrict__ fin, u64 mf, const PileRegion* __restrict__ reg,
                             const i32* __restrict__ seq_to_node, u32* __restrict__ tail, u32* __restrict__ head,
                             u32* __restrict__ length) {
  const u64 j = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= mf) return;
  const Overlap f = fin[j];
  const PileRegion L = reg[f.lhs_id], R = reg[f.rhs_id];
  const EdgeRecord r = edge_record(f, static_cast<u32>(seq_to_node[f.lhs_id]), static_cast<u32>(seq_to_node[f.rhs_id]),
                                   L.end - L.begin, R.end - R.begin);
  tail[2 * j] = r.tail;
  head[2 * j] = r.head;
  length[2 * j] = r.length;
  tail[2 * j + 1] = r.head ^ 1u;
  head[2 * j + 1] = r.tail ^ 1u;
  length[2 * j + 1] = r.length_pair;
}

// out-degrees and the by-tail sort key of every slot (an empty slot: tail n_nodes, behind every node)
__global__ void csr_keys_kernel(const u32* __restrict__ tail, u64 n_edges, u32 n_nodes, u32* __restrict__ deg,
                                u32* __restrict__ k32, u32* __restrict__ v32) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  const u32 t = tail[i];
  const bool live = t != kNoEdge;
  if (live) atomicAdd(deg + t, 1u);
  k32[i] = live ? t : n_nodes;
  v32[i] = static_cast<u32>(i);
}
// the (tail, head) sort key of every slot
__global__ void head_keys_kernel(const u32* __restrict__ tail, const u32* __restrict__ head, u64 n_edges, u32 n_nodes,
                                 u64* __restrict__ k64, u64* __restrict__ v64) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  const u32 t = tail[i];
  k64[i] = t != kNoEdge ? (static_cast<u64>(t) << 32 | head[i]) : static_cast<u64>(n_nodes) << 32;
  v64[i] = i;
}
__global__ void out_order_kernel(const u32* __restrict__ v32, u64 n_live, u32* __restrict__ out_edge) {
  const u64 p = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p < n_live) out_edge[p] = v32[p];
}
__global__ void head_order_kernel(const u64* __restrict__ k64, const u64* __restrict__ v64, u64 n_live, u32* __restrict__ hs_head,
                                  u32* __restrict__ hs_edge) {
  const u64 p = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= n_live) return;
  hs_head[p] = static_cast<u32>(k64[p]);
  hs_edge[p] = static_cast<u32>(v64[p]);
}

struct GraphView {
  const u32* off;
  const u32* out_edge;
  const u32* hs_head;
  const u32* hs_edge;
  const u32* head;
  const u32* length;
  u32 n_nodes;
};

// candidate[y] after `for jt in out(v): candidate[head(jt)] = jt`: the largest edge id among v's out-edges into y
__device__ __forceinline__ u32 last_edge_into(const GraphView& G, u32 b, u32 e, u32 y) {
  u32 lo = b, hi = e;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (G.hs_head[mid] <= y) lo = mid + 1;
    else hi = mid;
  }
  if (lo == b || G.hs_head[lo - 1] != y) return kNoEdge;
  return G.hs_edge[lo - 1];
}

// sweep 0: the marks and key1 = min (v << 32 | position of jt in out(v)); sweep 1: key2 = min (position of kt in
// out(head(jt))) << 1 | (0 own, 1 as the pair) among the marks made from the (v, jt) of key1
__global__ __launch_bounds__(64) void transitive_kernel(GraphView G, int sweep, u8* mark, unsigned long long* key1,
                                                        unsigned long long* key2) {
  __shared__ u64 s_excl[64];
  __shared__ u32 s_xb[64], s_len[64];
  const u32 lane = threadIdx.x;
  for (u32 v = blockIdx.x; v < G.n_nodes; v += gridDim.x) {
    const u32 b = G.off[v], e = G.off[v + 1];
    for (u32 j0 = b; j0 < e; j0 += 64) {
      const u32 left = e - j0;  // (the loop ends on `left`: j0 + 64 may wrap beside 2^32 edges)
      const bool has = lane < left;
      u32 dx = 0, xb = 0, lj = 0;
      if (has) {
        const u32 jt = G.out_edge[j0 + lane];
        const u32 x = G.head[jt];
        xb = G.off[x];
        dx = G.off[x + 1] - xb;
        lj = G.length[jt];
      }
      const u64 incl = wave_inclusive_sum(static_cast<u64>(dx));
      const u64 total = __shfl(incl, 63, 64);
      s_excl[lane] = incl - dx;
      s_xb[lane] = xb;
      s_len[lane] = lj;
      __syncthreads();
      for (u64 t = lane; t < total; t += 64) {
        u32 l = 0;  // the last lane whose pairs start at or before t
#pragma unroll
        for (u32 step = 32; step > 0; step >>= 1)
          if (s_excl[l + step] <= t) l += step;
        const u32 kpos = static_cast<u32>(t - s_excl[l]);
        const u32 kt = G.out_edge[s_xb[l] + kpos];
        const u32 c = last_edge_into(G, b, e, G.head[kt]);
        if (c == kNoEdge || !is_transitive(s_len[l], G.length[kt], G.length[c])) continue;
        const unsigned long long mine = static_cast<unsigned long long>(v) << 32 | (j0 - b + l);
        if (sweep == 0) {
          mark[c] = 1;
          mark[c ^ 1u] = 1;
          atomicMin(key1 + c, mine);
          atomicMin(key1 + (c ^ 1u), mine);
        } else {
          const unsigned long long k2 = static_cast<unsigned long long>(kpos) << 1;
          if (key1[c] == mine) atomicMin(key2 + c, k2);
          if (key1[c ^ 1u] == mine) atomicMin(key2 + (c ^ 1u), k2 | 1ULL);
        }
      }
      __syncthreads();
      if (left <= 64) break;
    }
  }
}

__global__ void marked_ids_kernel(const u8* __restrict__ mark, const u32* __restrict__ slot, const unsigned long long* __restrict__ key2,
                                  u64 n_edges, u64* __restrict__ k, u64* __restrict__ v) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_edges || !mark[i]) return;
  k[slot[i]] = key2[i];
  v[slot[i]] = i;
}
__global__ void gather_key1_kernel(const unsigned long long* __restrict__ key1, const u64* __restrict__ v, u64 n, u64* __restrict__ k) {
  const u64 p = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p < n) k[p] = key1[v[p]];
}
__global__ void order_kernel(const u64* __restrict__ v, u64 n, u32* __restrict__ order, u8* __restrict__ odd) {
  const u64 p = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= n) return;
  order[p] = static_cast<u32>(v[p]);
  odd[p] = static_cast<u8>(v[p] & 1u);
}
__global__ void transitive_pairs_kernel(const u32* __restrict__ order, const u8* __restrict__ odd, const u32* __restrict__ slot, u64 n,
                                        const u32* __restrict__ tail, const u32* __restrict__ head, u32* __restrict__ pairs) {
  const u64 p = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= n || !odd[p]) return;
  const u32 id = order[p];
  pairs[2ULL * slot[p]] = tail[id] & ~1u;
  pairs[2ULL * slot[p] + 1] = head[id] & ~1u;
}

__global__ __launch_bounds__(64) void long_edges_kernel(const u32* __restrict__ off, const u32* __restrict__ out_edge, u32 n_nodes,
                                                        const double* __restrict__ weight, u8* flags) {
  const u32 lane = threadIdx.x;
  const double inf = __builtin_huge_val();
  for (u32 v = blockIdx.x; v < n_nodes; v += gridDim.x) {
    const u32 b = off[v], e = off[v + 1];
    if (e - b < 2) continue;
    double m1 = inf;
    for (u32 p = b + lane; p < e; p += 64) {
      const double w = weight[out_edge[p]];
      m1 = w < m1 ? w : m1;
      if (e - p <= 64) break;
    }
    m1 = wave_min(m1);
    u32 at_min = 0;
    double m2 = inf;  // the smallest weight that is not m1
    for (u32 p = b + lane; p < e; p += 64) {
      const double w = weight[out_edge[p]];
      if (w == m1) ++at_min;
      else m2 = w < m2 ? w : m2;
      if (e - p <= 64) break;
    }
    at_min = wave_sum(at_min);
    m2 = wave_min(m2);
    for (u32 p = b + lane; p < e; p += 64) {
      const u32 kt = out_edge[p];
      const double w = weight[kt];
      // the smallest among the OTHER out-edges: m1, unless kt is the only edge that weighs m1
      const double min_other = (w == m1 && at_min < 2) ? m2 : m1;
      if (is_long_edge(min_other, w)) {
        flags[kt] = 1;
        flags[kt ^ 1u] = 1;
      }
      if (e - p <= 64) break;
    }
  }
}

u32 node_blocks(u32 n_nodes) { return n_nodes < kGraphMaxBlocks ? n_nodes : kGraphMaxBlocks; }

// off / out_edge of g from its tail table
void build_out_lists(Engine& e, GraphDev& g) {
  hipStream_t s = e.stream;
  GraphScratch& S = e.graph;
  const u64 E = g.n_edges;
  const u32 n = g.n_nodes;
  u32* d_off = g.off.get<u32>(static_cast<size_t>(n) + 2);
  g.n_live = 0;
  g.head_order = false;
  if (E == 0) {
    RVN_HIP(hipMemsetAsync(d_off, 0, (static_cast<size_t>(n) + 1) * 4, s));
    RVN_HIP(rvn_stream_sync(s));
    return;
  }
  u32* d_deg = S.deg.get<u32>(static_cast<size_t>(n) + 2);
  RVN_HIP(hipMemsetAsync(d_deg, 0, (static_cast<size_t>(n) + 1) * 4, s));
  u32* k32[2] = {S.k32[0].get<u32>(E), S.k32[1].get<u32>(E)};
  u32* v32[2] = {S.v32[0].get<u32>(E), S.v32[1].get<u32>(E)};
  csr_keys_kernel<<<div_up(E, 256), 256, 0, s>>>(g.tail.as<u32>(), E, n, d_deg, k32[0], v32[0]);
  RVN_LAUNCH_CHECK();
  exclusive_scan_u32_u32(d_deg, d_off, n, e.scratch.scan_tmp, s);
  g.n_live = read_back(e, d_off + n, 4);
  const int a = radix_sort_pairs_u32_u32(k32[0], k32[1], v32[0], v32[1], E, bits_for(n), e.scratch.sort_tmp, e.scratch.scan_tmp, s);
  if (g.n_live) {
    out_order_kernel<<<div_up(g.n_live, 256), 256, 0, s>>>(v32[a], g.n_live, g.out_edge.get<u32>(g.n_live));
    RVN_LAUNCH_CHECK();
  }
  RVN_HIP(rvn_stream_sync(s));
}

// hs_head / hs_edge of g: only the transitive marking looks an out-edge up by its head, so the order is made by the
// first call that needs it (the long-edge marking of every layout round does not pay for the 64-bit sort)
void build_head_order(Engine& e, GraphDev& g) {
  if (g.head_order || g.n_live == 0) return;
  hipStream_t s = e.stream;
  GraphScratch& S = e.graph;
  const u64 E = g.n_edges;
  u64* k64[2] = {S.k64[0].get<u64>(E), S.k64[1].get<u64>(E)};
  u64* v64[2] = {S.v64[0].get<u64>(E), S.v64[1].get<u64>(E)};
  head_keys_kernel<<<div_up(E, 256), 256, 0, s>>>(g.tail.as<u32>(), g.head.as<u32>(), E, g.n_nodes, k64[0], v64[0]);
  RVN_LAUNCH_CHECK();
  const int c = radix_sort_pairs_u64_u64(k64[0], k64[1], v64[0], v64[1], E, 32 + bits_for(g.n_nodes), e.scratch.sort_tmp,
                                         e.scratch.scan_tmp, s);
  head_order_kernel<<<div_up(g.n_live, 256), 256, 0, s>>>(k64[c], v64[c], g.n_live, g.hs_head.get<u32>(g.n_live),
                                                          g.hs_edge.get<u32>(g.n_live));
  RVN_LAUNCH_CHECK();
  RVN_HIP(rvn_stream_sync(s));
  g.head_order = true;
}

GraphView view_of(const GraphDev& g) {
  return GraphView{g.off.as<u32>(), g.out_edge.as<u32>(), g.hs_head.as<u32>(), g.hs_edge.as<u32>(), g.head.as<u32>(),
                   g.length.as<u32>(), g.n_nodes};
}

}  // namespace

void graph_construct(Engine& e, const Overlap* h_ovl, u64 m, u32 n_piles, const u32* h_begin, const u32* h_end,
                     const u16* h_median, const u8* h_invalid, GraphDev& g) {
  hipStream_t s = e.stream;
  GraphScratch& S = e.graph;
  g.constructed = true;
  g.marked = false;
  g.n_piles = n_piles;
  g.n_nodes = 0;
  g.n_edges = 0;
  u64 mf = 0;
  if (n_piles) {
    // nodes: a prefix sum over the valid piles
    const u8* d_invalid = upload(S.invalid, h_invalid, n_piles, s);
    const u16* d_median = upload(S.median, h_median, n_piles, s);
    u8* d_valid = S.keep.get<u8>(static_cast<size_t>(n_piles) + 16);
    valid_flags_kernel<<<div_up(n_piles, 256), 256, 0, s>>>(d_invalid, n_piles, d_valid);
    RVN_LAUNCH_CHECK();
    const KeptSlots vs = kept_slots(e, d_valid, n_piles, S.slot);
    g.n_nodes = static_cast<u32>(2 * vs.kept);
    i32* d_s2n = g.seq_to_node.get<i32>(n_piles);
    node_ids_kernel<<<div_up(n_piles, 256), 256, 0, s>>>(d_invalid, vs.slot, d_median, n_piles, d_s2n,
                                                         g.node_pile.get<u32>(static_cast<size_t>(g.n_nodes) + 2),
                                                         g.node_cov.get<u16>(static_cast<size_t>(g.n_nodes) + 2));
    RVN_LAUNCH_CHECK();
    if (m) {
      // edges: OverlapFinalize, the survivors in order, two edges each
      upload(S.ovl, h_ovl, m, s);
      const PileRegion* d_reg = upload_pile_regions(e, S.reg, h_begin, h_end, h_invalid, n_piles);
      u8* d_keep = S.keep.get<u8>(m + 16);
      unsigned long long* d_bad = S.err.get<unsigned long long>(2);
      RVN_HIP(hipMemsetAsync(d_bad, 0xFF, 8, s));
      finalize_kernel<<<div_up(m, 256), 256, 0, s>>>(S.ovl.as<Overlap>(), m, d_reg, d_keep, d_bad);
      RVN_LAUNCH_CHECK();
      const u64 bad = read_back(e, d_bad, 8);
      if (bad != ~0ULL)
        throw std::invalid_argument("[raven_hip] rvn_construct_assembly_graph: overlap " + std::to_string(bad) +
                                    " makes an edge (type 3 or 4) but names an invalid pile");
      mf = compact_overlap_list(e, S.ovl, m, d_keep, S.slot, S.spare);
      if (2 * mf >= 0xFFFFFFFFULL) throw std::invalid_argument("[raven_hip] rvn_construct_assembly_graph: 2^32 edges or more");
      if (mf) {
        // (compact_overlap_list leaves its exclusive scan of the keep flags in S.slot — "slot stays valid for the caller",
        // engine.h — which is where every survivor went: the index of its edge pair)
        edge_source_kernel<<<div_up(m, 256), 256, 0, s>>>(d_keep, S.slot.as<u32>(), m, g.edge_overlap.get<u64>(mf));
        RVN_LAUNCH_CHECK();
        Overlap* d_fin = g.finalized.get<Overlap>(mf);
        RVN_HIP(hipMemcpyAsync(d_fin, S.ovl.ptr, mf * sizeof(Overlap), hipMemcpyDeviceToDevice, s));
        edges_kernel<<<div_up(mf, 256), 256, 0, s>>>(d_fin, mf, d_reg, d_s2n, g.tail.get<u32>(2 * mf), g.head.get<u32>(2 * mf),
                                                     g.length.get<u32>(2 * mf));
        RVN_LAUNCH_CHECK();
      }
    }
  }
  g.n_edges = 2 * mf;
  build_out_lists(e, g);
}

void graph_from_edges(Engine& e, u32 n_nodes, u64 n_edges, const u32* h_tail, const u32* h_head, const u32* h_length, GraphDev& g) {
  hipStream_t s = e.stream;
  g.constructed = false;
  g.marked = false;
  g.n_piles = 0;
  g.n_nodes = n_nodes;
  g.n_edges = n_edges;
  upload(g.tail, h_tail, n_edges, s);
  upload(g.head, h_head, n_edges, s);
  upload(g.length, h_length, n_edges, s);
  build_out_lists(e, g);
}

u64 graph_mark_transitive(Engine& e, GraphDev& g) {
  hipStream_t s = e.stream;
  GraphScratch& S = e.graph;
  g.order.clear();
  g.pairs.clear();
  g.marked = false;  // (set when the sequence is complete: a call that fails leaves no half result to fetch)
  const u64 E = g.n_edges;
  if (E == 0 || g.n_live == 0) {
    g.marked = true;
    return 0;
  }
  build_head_order(e, g);
  u8* d_mark = S.mark.get<u8>(E + 16);
  unsigned long long* d_key1 = S.key1.get<unsigned long long>(E);
  unsigned long long* d_key2 = S.key2.get<unsigned long long>(E);
  RVN_HIP(hipMemsetAsync(d_mark, 0, E, s));
  RVN_HIP(hipMemsetAsync(d_key1, 0xFF, E * 8, s));
  RVN_HIP(hipMemsetAsync(d_key2, 0xFF, E * 8, s));
  const GraphView G = view_of(g);
  for (int sweep = 0; sweep < 2; ++sweep) {
    transitive_kernel<<<node_blocks(g.n_nodes), 64, 0, s>>>(G, sweep, d_mark, d_key1, d_key2);
    RVN_LAUNCH_CHECK();
  }
  const KeptSlots ks = kept_slots(e, d_mark, E, S.slot);
  const u64 M = ks.kept;
  if (M == 0) {
    g.marked = true;
    return 0;
  }
  // the insertion sequence: by (key1, key2) — two stable sorts, the minor key first
  u64* k[2] = {S.k64[0].get<u64>(M), S.k64[1].get<u64>(M)};
  u64* v[2] = {S.v64[0].get<u64>(M), S.v64[1].get<u64>(M)};
  marked_ids_kernel<<<div_up(E, 256), 256, 0, s>>>(d_mark, ks.slot, d_key2, E, k[0], v[0]);
  RVN_LAUNCH_CHECK();
  const int a = radix_sort_pairs_u64_u64(k[0], k[1], v[0], v[1], M, 64, e.scratch.sort_tmp, e.scratch.scan_tmp, s);
  gather_key1_kernel<<<div_up(M, 256), 256, 0, s>>>(d_key1, v[a], M, k[a]);
  RVN_LAUNCH_CHECK();
  const int c = a ^ radix_sort_pairs_u64_u64(k[a], k[a ^ 1], v[a], v[a ^ 1], M, 64, e.scratch.sort_tmp, e.scratch.scan_tmp, s);
  u32* d_order = S.ids.get<u32>(M);
  u8* d_odd = S.flags.get<u8>(M + 16);
  order_kernel<<<div_up(M, 256), 256, 0, s>>>(v[c], M, d_order, d_odd);
  RVN_LAUNCH_CHECK();
  const KeptSlots os = kept_slots(e, d_odd, M, S.slot);
  g.order.resize(M);
  g.pairs.resize(2 * os.kept);
  if (os.kept) {
    u32* d_pairs = S.k32[0].get<u32>(2 * os.kept);
    transitive_pairs_kernel<<<div_up(M, 256), 256, 0, s>>>(d_order, d_odd, os.slot, M, g.tail.as<u32>(), g.head.as<u32>(), d_pairs);
    RVN_LAUNCH_CHECK();
    RVN_HIP(hipMemcpyAsync(g.pairs.data(), d_pairs, g.pairs.size() * 4, hipMemcpyDeviceToHost, s));
  }
  RVN_HIP(hipMemcpyAsync(g.order.data(), d_order, M * 4, hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));
  g.marked = true;
  return M;
}

u64 graph_mark_long_edges(Engine& e, const GraphDev& g, const double* h_weight, u8* h_marked) {
  hipStream_t s = e.stream;
  GraphScratch& S = e.graph;
  const u64 E = g.n_edges;
  if (E == 0) return 0;
  if (g.n_live == 0) {
    if (h_marked) std::memset(h_marked, 0, E);
    return 0;
  }
  const double* d_w = upload(S.weight, h_weight, E, s);
  u8* d_flags = S.flags.get<u8>(E + 16);
  RVN_HIP(hipMemsetAsync(d_flags, 0, E, s));
  long_edges_kernel<<<node_blocks(g.n_nodes), 64, 0, s>>>(g.off.as<u32>(), g.out_edge.as<u32>(), g.n_nodes, d_w, d_flags);
  RVN_LAUNCH_CHECK();
  const KeptSlots ks = kept_slots(e, d_flags, E, S.slot);
  if (h_marked) RVN_HIP(hipMemcpyAsync(h_marked, d_flags, E, hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));
  return ks.kept;
}

}  // namespace rvn
