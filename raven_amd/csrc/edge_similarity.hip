// edge_similarity.hip — printEdgeSimilarity of the CSV emitters (RavenLib/src/graph_repr.cc:247-258 in PrintCsv, :358-369 in
// getCsv) for every slot of an edge table, from the tilings: lhs = tail.InflateData(length), rhs = head.InflateData(0,
// lhs.size()), their exact global edit distance (edlibAlign, default configuration), 1 - distance / lhs.size().  The rules
// are unitig_rules.h's (edge_lhs_length, edge_rhs_length, segment_slice, slice_word); nothing about an edge passes through
// the host but the three result arrays.
//   plan      one lane per edge slot reads tail / head / length where they lie: the two lengths, and which route the edge takes
//   direct    both nodes are one segment each (every edge before unitigs exist): the two slices are spans of the reads
//             themselves, no base is copied.  ED(a, b) = ED(rc a, rc b), so a tail on strand 1 is stated as the stored span
//             of its read and the pair's strand flag says whether the head lies on the tail's strand.
//   packed    the other edges: their slices are packed (pack_slices_dev, one lane per word) into a scratch read set, a
//             chunk at a time — a chunk is the edges whose first word lies in one stretch of `budget` words of the scan over
//             the slices' word counts, so a graph whose overlaps sum to gigabytes never needs them all at once
//   distance  edit_distance_dev without thresholds; what the wave ring's doubling leaves goes to the workgroup ring, then to
//             the full sweep (wide_after)
#include <vector>

#include "abi.h"
#include "unitig_rules.h"

namespace rvn {

namespace {

struct SimPair {  // edit_distance.hip's pair record
  u32 a_idx, a_begin, a_len, b_idx, b_begin, b_len, strand, pad;
};
constexpr u32 kNoDistance = 0xFFFFFFFFu;

struct SimTiling {
  const u64* seg_off;
  const Segment* seg;
  const u32* len;
};

// per edge slot: the slices' lengths, the distance where no sweep is needed (an empty slot, two empty slices), and the route
__global__ void edge_plan_kernel(u64 n_edges, const u32* __restrict__ tail, const u32* __restrict__ head, const u32* __restrict__ length,
                                 SimTiling t, u32* __restrict__ lhs, u32* __restrict__ rhs, u32* __restrict__ dist, u8* __restrict__ direct,
                                 u8* __restrict__ mat) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  const u32 u = tail[i];
  u32 l = 0, r = 0, d = kNoDistance;
  u8 is_direct = 0, is_mat = 0;
  if (u != kNoEdge) {
    const u32 v = head[i];
    l = edge_lhs_length(t.len[u], length[i]);
    r = edge_rhs_length(l, t.len[v]);
    d = 0;
    if (l != 0) {  // (l == 0: both slices are empty, the distance is 0)
      const bool single = t.seg_off[u + 1] - t.seg_off[u] == 1 && t.seg_off[v + 1] - t.seg_off[v] == 1;
      is_direct = single ? 1 : 0;
      is_mat = single ? 0 : 1;
    }
  }
  lhs[i] = l;
  rhs[i] = r;
  dist[i] = d;
  direct[i] = is_direct;
  mat[i] = is_mat;
}

// the two lists: a direct edge's pair of read spans at its slot of the direct list, a packed edge's two slices at its slot
// of the slice list
__global__ void edge_emit_kernel(u64 n_edges, const u32* __restrict__ tail, const u32* __restrict__ head, const u32* __restrict__ length,
                                 SimTiling t, const u32* __restrict__ lhs, const u32* __restrict__ rhs, const u8* __restrict__ direct,
                                 const u8* __restrict__ mat, const u32* __restrict__ dslot, const u32* __restrict__ mslot,
                                 SimPair* __restrict__ pairs, u32* __restrict__ dids, u32* __restrict__ mids, u32* __restrict__ snode,
                                 u32* __restrict__ sbegin, u32* __restrict__ slen, u32* __restrict__ swords) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  if (direct[i]) {
    const u32 u = tail[i], v = head[i];
    const Segment a = segment_slice(t.seg[t.seg_off[u]], length[i], lhs[i]);
    const Segment b = segment_slice(t.seg[t.seg_off[v]], 0, rhs[i]);
    const u32 at = dslot[i];
    // the pattern is the stored span of the tail's read whatever its strand; the text is reverse-complemented (flag 0)
    // exactly when the head lies on the other strand
    pairs[at] = SimPair{a.read, a.begin, a.length, b.read, b.begin, b.length, a.strand == b.strand ? 1u : 0u, 0u};
    dids[at] = static_cast<u32>(i);
  } else if (mat[i]) {
    const u32 at = mslot[i];
    mids[at] = static_cast<u32>(i);
    snode[2 * at] = tail[i];
    sbegin[2 * at] = length[i];
    slen[2 * at] = lhs[i];
    swords[2 * at] = lhs[i] / 32u + (lhs[i] % 32u ? 1u : 0u);
    snode[2 * at + 1] = head[i];
    sbegin[2 * at + 1] = 0;
    slen[2 * at + 1] = rhs[i];
    swords[2 * at + 1] = rhs[i] / 32u + (rhs[i] % 32u ? 1u : 0u);
  }
}

// chunk c = the packed edges j whose first word woff[2 j] lies in [c budget, (c + 1) budget): bounds[c] = its first edge,
// wbase[c] = that edge's first word (c = n_chunks: the end of the list)
__global__ void chunk_bounds_kernel(u32 n_chunks, u64 budget, const u64* __restrict__ woff, u32 n_mat, u32* __restrict__ bounds,
                                    u64* __restrict__ wbase) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > n_chunks) return;
  u32 lo = 0, hi = n_mat;  // the first j with woff[2 j] >= c budget
  if (c == n_chunks) lo = n_mat;
  const u64 want = static_cast<u64>(c) * budget;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (woff[2ULL * mid] < want) lo = mid + 1;
    else hi = mid;
  }
  bounds[c] = lo;
  wbase[c] = woff[2ULL * lo];
}

// the chunk as a read set of its own: read 2 k = lhs of its k-th edge, read 2 k + 1 = rhs; pairs of whole reads, same strand
__global__ void chunk_pairs_kernel(u32 first, u32 count, const u32* __restrict__ mids, const u32* __restrict__ lhs, const u32* __restrict__ rhs,
                                   const u64* __restrict__ woff, u64* __restrict__ word_off, SimPair* __restrict__ pairs) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > count) return;
  const u64 base = woff[2ULL * first];
  const u64 j = static_cast<u64>(first) + k;
  word_off[2ULL * k] = woff[2 * j] - base;
  if (k == count) return;
  word_off[2ULL * k + 1] = woff[2 * j + 1] - base;
  const u32 id = mids[j];
  pairs[k] = SimPair{2 * k, 0u, lhs[id], 2 * k + 1, 0u, rhs[id], 1u, 0u};
}

__global__ void scatter_distances_kernel(u32 count, const u32* __restrict__ ids, const u32* __restrict__ from, u32* __restrict__ dist) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < count) dist[ids[k]] = from[k];
}

// words of packed slices one chunk may hold: the option, or a quarter of the largest block the arena (the driver, where no
// arena runs) can still give — the edit-distance stage's own scratch and the full sweep's boundary rows need the rest
u64 chunk_budget_words(const Engine& e) {
  if (e.opt.edge_slices_budget_kb > 0) return static_cast<u64>(e.opt.edge_slices_budget_kb) * 128;
  size_t room = 0;
  if (devpool::active()) {
    room = devpool::free_largest();
  } else {
    size_t free_b = 0, total_b = 0;
    RVN_HIP(hipMemGetInfo(&free_b, &total_b));
    room = free_b;
  }
  return std::max<u64>(room / 4 / 8, 1ULL << 17);  // (never below 1 MB: a chunk is at least one edge anyway)
}

}  // namespace

void graph_edge_similarity(Engine& e, const GraphDev& g, const TilingDev& T, const ReadsDev& R, u32* h_lhs, u32* h_rhs, u32* h_distance) {
  const std::string who = "[raven_hip] rvn_graph_edge_similarity: ";
  if (T.n_nodes != g.n_nodes)
    throw std::invalid_argument(who + "the tiling has " + std::to_string(T.n_nodes) + " nodes, the graph " + std::to_string(g.n_nodes));
  if (T.reads_serial != R.serial) throw std::invalid_argument(who + "the tiling was made for another read set");
  const u64 E = g.n_edges;
  if (E == 0) return;
  hipStream_t s = e.stream;
  EdgeSimScratch& S = e.edge_sim;
  const u32 *d_tail = g.tail.as<u32>(), *d_head = g.head.as<u32>(), *d_length = g.length.as<u32>();
  const SimTiling tv{T.seg_off.as<u64>(), T.seg.as<Segment>(), T.len.as<u32>()};

  // the plan: lengths, routes, the slots of the two lists
  u32* d_lhs = S.lhs.get<u32>(E + 1);
  u32* d_rhs = S.rhs.get<u32>(E + 1);
  u32* d_dist = S.dist.get<u32>(E + 1);
  u8* d_direct = S.direct.get<u8>(E + 16);
  u8* d_mat = S.mat.get<u8>(E + 16);
  RVN_KLAUNCH(kKEdgePairs, edge_plan_kernel<<<div_up(E, 256), 256, 0, s>>>(E, d_tail, d_head, d_length, tv, d_lhs, d_rhs, d_dist, d_direct, d_mat));
  const KeptSlots ds = kept_slots(e, d_direct, E, S.dslot);
  const KeptSlots ms = kept_slots(e, d_mat, E, S.mslot);
  const u32 D = static_cast<u32>(ds.kept), M = static_cast<u32>(ms.kept);
  SimPair* d_pairs = S.pairs.get<SimPair>(static_cast<size_t>(D) + 1);
  u32* d_dids = S.dids.get<u32>(static_cast<size_t>(D) + 1);
  u32* d_mids = S.mids.get<u32>(static_cast<size_t>(M) + 1);
  const size_t n_slices = 2 * static_cast<size_t>(M);
  u32* d_snode = S.snode.get<u32>(n_slices + 1);
  u32* d_sbegin = S.sbegin.get<u32>(n_slices + 1);
  u32* d_slen = S.slen.get<u32>(n_slices + 1);
  u32* d_swords = S.swords.get<u32>(n_slices + 1);
  if (D || M)
    RVN_KLAUNCH(kKEdgePairs, edge_emit_kernel<<<div_up(E, 256), 256, 0, s>>>(E, d_tail, d_head, d_length, tv, d_lhs, d_rhs, d_direct, d_mat, ds.slot,
                                                                             ms.slot, d_pairs, d_dids, d_mids, d_snode, d_sbegin, d_slen, d_swords));

  // the direct route: spans of the reads themselves
  if (D) {
    u32* d_ddist = S.ddist.get<u32>(static_cast<size_t>(D) + 1);
    edit_distance_dev(e, R, reinterpret_cast<const u32*>(d_pairs), D, d_ddist, nullptr, false, true);
    scatter_distances_kernel<<<div_up(D, 256), 256, 0, s>>>(D, d_dids, d_ddist, d_dist);
    RVN_LAUNCH_CHECK();
  }

  // the packed route, a chunk of the slices at a time
  if (M) {
    u64* d_woff = S.woff.get<u64>(n_slices + 2);
    exclusive_scan_u32_u64(d_swords, d_woff, n_slices, e.scratch.scan_tmp, s);
    const u64 total_words = read_back(e, d_woff + n_slices, 8);
    const u64 budget = chunk_budget_words(e);
    const u64 chunks64 = (total_words + budget - 1) / budget;
    if (chunks64 >= 0xFFFFFFFFULL) throw std::invalid_argument(who + "the slice budget cuts the edges into 2^32 chunks or more");
    const u32 n_chunks = static_cast<u32>(chunks64);
    u32* d_bounds = S.bounds.get<u32>(static_cast<size_t>(n_chunks) + 2);
    u64* d_wbase = S.wbase.get<u64>(static_cast<size_t>(n_chunks) + 2);
    RVN_KLAUNCH(kKEdgePairs, chunk_bounds_kernel<<<div_up(static_cast<u64>(n_chunks) + 1, 256), 256, 0, s>>>(n_chunks, budget, d_woff, M, d_bounds, d_wbase));
    std::vector<u32> bounds(static_cast<size_t>(n_chunks) + 1);
    std::vector<u64> wbase(static_cast<size_t>(n_chunks) + 1);
    RVN_HIP(hipMemcpyAsync(bounds.data(), d_bounds, bounds.size() * 4, hipMemcpyDeviceToHost, s));
    RVN_HIP(hipMemcpyAsync(wbase.data(), d_wbase, wbase.size() * 8, hipMemcpyDeviceToHost, s));
    RVN_HIP(rvn_stream_sync(s));
    for (u32 c = 0; c < n_chunks; ++c) {
      const u32 first = bounds[c], count = bounds[c + 1] - bounds[c];
      if (count == 0) continue;  // (an edge longer than the budget spans several stretches: it is the chunk of its first)
      const u64 words = wbase[c + 1] - wbase[c];
      u64* d_packed = S.slices.packed.get<u64>(words + 2);
      u64* d_word_off = S.slices.word_off.get<u64>(2 * static_cast<size_t>(count) + 2);
      SimPair* d_cpairs = S.cpairs.get<SimPair>(static_cast<size_t>(count) + 1);
      u32* d_cdist = S.cdist.get<u32>(static_cast<size_t>(count) + 1);
      RVN_KLAUNCH(kKEdgePairs, chunk_pairs_kernel<<<div_up(static_cast<u64>(count) + 1, 256), 256, 0, s>>>(first, count, d_mids, d_lhs, d_rhs, d_woff,
                                                                                                         d_word_off, d_cpairs));
      pack_slices_dev(e, T, R, d_snode, d_sbegin, d_slen, d_woff, 2ULL * first, 2ULL * count, words, d_packed);
      RVN_HIP(hipMemsetAsync(d_packed + words, 0, 16, s));
      edit_distance_dev(e, S.slices, reinterpret_cast<const u32*>(d_cpairs), count, d_cdist, nullptr, false, true);
      scatter_distances_kernel<<<div_up(count, 256), 256, 0, s>>>(count, d_mids + first, d_cdist, d_dist);
      RVN_LAUNCH_CHECK();
    }
  }

  if (h_lhs) RVN_HIP(hipMemcpyAsync(h_lhs, d_lhs, E * 4, hipMemcpyDeviceToHost, s));
  if (h_rhs) RVN_HIP(hipMemcpyAsync(h_rhs, d_rhs, E * 4, hipMemcpyDeviceToHost, s));
  if (h_distance) RVN_HIP(hipMemcpyAsync(h_distance, d_dist, E * 4, hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));
}

}  // namespace rvn
