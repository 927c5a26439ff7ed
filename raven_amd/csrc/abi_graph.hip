// abi_graph.hip — C ABI (include/raven_hip.h): the assembly graph on the device (graph.hip): rvn_construct_assembly_graph,
// rvn_graph_from_edges, the marking of transitive and long edges, and what a graph handle gives back; node sequences as
// tilings, rvn_graph_create_unitigs and unitig sequences as read sets (unitigs.hip); node paths as read sets and
// RemoveBubbles' similarity verdict on pairs of them (unitigs.hip, edit_distance.hip); slices of nodes as read sets and the
// CSV emitters' edge similarity (unitigs.hip, edge_similarity.hip).
#include <cmath>
#include <cstring>

#include "abi.h"
#include "graph_rules.h"

using namespace rvn;

struct rvn_graph {
  GraphDev g;
  int device = 0;
};
struct rvn_tiling {
  TilingDev t;
  int device = 0;
};
struct rvn_unitigs {
  UnitigTables u;
};

namespace {

constexpr u32 kMaxGraphNodes = 1u << 31;  // node ids are int32 in sequence_to_node

template <typename T>
void fetch(T* dst, const DevBuf& src, u64 count) {
  if (dst && count) RVN_HIP(hipMemcpy(dst, src.ptr, count * sizeof(T), hipMemcpyDeviceToHost));
}
template <typename T>
void give(T* dst, const std::vector<T>& src) {
  if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(T));
}

int nodes_as_reads(Engine& e, const rvn_tiling* t, const rvn_reads* reads, const std::vector<u32>& nodes, rvn_reads** out) {
  std::unique_ptr<rvn_reads> rr(new rvn_reads());
  tiling_as_reads(e, t->t, reads->r, nodes.data(), static_cast<u32>(nodes.size()), rr->r);
  *out = rr.release();
  return RVN_OK;
}

}  // namespace

extern "C" {

int rvn_construct_assembly_graph(rvn_engine* h, const rvn_overlap* overlaps, uint64_t n_overlaps, uint32_t n_piles,
                                 const uint32_t* pile_begin, const uint32_t* pile_end, const uint16_t* median,
                                 const uint8_t* invalid, rvn_graph** out) {
  const bool args_ok = h && out && (n_overlaps == 0 || overlaps) && (n_piles == 0 || (pile_begin && pile_end && median && invalid));
  return guarded(h, args_ok, "[raven_hip] rvn_construct_assembly_graph: NULL argument", [&](Engine& e) -> int {
    const char* who = "[raven_hip] rvn_construct_assembly_graph: ";
    *out = nullptr;
    if (n_piles >= kMaxGraphNodes / 2) return fail(RVN_EINVAL, std::string(who) + "2^30 piles or more");
    for (u32 i = 0; i < n_piles; ++i)
      if (pile_end[i] < pile_begin[i])
        return fail(RVN_EINVAL, std::string(who) + "pile " + std::to_string(i) + " ends before it begins");
    for (u64 x = 0; x < n_overlaps; ++x)
      if (overlaps[x].lhs_id >= n_piles || overlaps[x].rhs_id >= n_piles)
        return fail(RVN_EINVAL, std::string(who) + "overlap " + std::to_string(x) + " names an unknown pile");
    for (u64 x = 0; x < n_overlaps; ++x)
      if (overlaps[x].strand > 1)  // (head = node + 1 - strand)
        return fail(RVN_EINVAL, std::string(who) + "overlap " + std::to_string(x) + " has a strand other than 0 or 1");
    std::unique_ptr<rvn_graph> G(new rvn_graph());
    G->device = e.device;
    graph_construct(e, reinterpret_cast<const Overlap*>(overlaps), n_overlaps, n_piles, pile_begin, pile_end, median, invalid, G->g);
    *out = G.release();
    return RVN_OK;
  });
}

int rvn_graph_from_edges(rvn_engine* h, uint32_t n_nodes, uint64_t n_edges, const uint32_t* tail, const uint32_t* head,
                         const uint32_t* length, rvn_graph** out) {
  const bool args_ok = h && out && (n_edges == 0 || (tail && head && length));
  return guarded(h, args_ok, "[raven_hip] rvn_graph_from_edges: NULL argument", [&](Engine& e) -> int {
    const char* who = "[raven_hip] rvn_graph_from_edges: ";
    *out = nullptr;
    if (n_nodes > kMaxGraphNodes) return fail(RVN_EINVAL, std::string(who) + "more than 2^31 nodes");
    if (n_edges & 1) return fail(RVN_EINVAL, std::string(who) + "an odd number of edge slots (edges come in pairs: id and id ^ 1)");
    if (n_edges >= 0xFFFFFFFFULL) return fail(RVN_EINVAL, std::string(who) + "2^32 edge slots or more");
    for (u64 i = 0; i < n_edges; ++i) {
      if (tail[i] == kNoEdge) {
        if (tail[i ^ 1] != kNoEdge)
          return fail(RVN_EINVAL, std::string(who) + "edge " + std::to_string(i ^ 1) + " has an empty pair slot");
        continue;
      }
      if (tail[i] >= n_nodes || head[i] >= n_nodes)
        return fail(RVN_EINVAL, std::string(who) + "edge " + std::to_string(i) + " names an unknown node");
    }
    std::unique_ptr<rvn_graph> G(new rvn_graph());
    G->device = e.device;
    graph_from_edges(e, n_nodes, n_edges, tail, head, length, G->g);
    *out = G.release();
    return RVN_OK;
  });
}

int rvn_graph_info(const rvn_graph* g, uint32_t* n_nodes, uint64_t* n_edges, uint64_t* n_live_edges) {
  return guarded([&]() -> int {
    if (!g) return fail(RVN_EINVAL, "[raven_hip] NULL graph");
    if (n_nodes) *n_nodes = g->g.n_nodes;
    if (n_edges) *n_edges = g->g.n_edges;
    if (n_live_edges) *n_live_edges = g->g.n_live;
    return RVN_OK;
  });
}

int rvn_graph_fetch(const rvn_graph* g, int32_t* sequence_to_node, uint32_t* node_pile, uint16_t* node_coverage,
                    uint32_t* edge_tail, uint32_t* edge_head, uint32_t* edge_length, uint64_t* edge_overlap,
                    rvn_overlap* finalized) {
  return guarded([&]() -> int {
    if (!g) return fail(RVN_EINVAL, "[raven_hip] NULL graph");
    const GraphDev& x = g->g;
    if (!x.constructed && (sequence_to_node || node_pile || node_coverage || edge_overlap || finalized))
      return fail(RVN_EINVAL, "[raven_hip] rvn_graph_fetch: a graph made from edges has no piles, coverage or overlaps");
    RVN_HIP(hipSetDevice(g->device));
    fetch(sequence_to_node, x.seq_to_node, x.n_piles);
    fetch(node_pile, x.node_pile, x.n_nodes);
    fetch(node_coverage, x.node_cov, x.n_nodes);
    fetch(edge_tail, x.tail, x.n_edges);
    fetch(edge_head, x.head, x.n_edges);
    fetch(edge_length, x.length, x.n_edges);
    fetch(edge_overlap, x.edge_overlap, x.n_edges / 2);
    fetch(reinterpret_cast<Overlap*>(finalized), x.finalized, x.n_edges / 2);
    return RVN_OK;
  });
}

int rvn_graph_mark_transitive(rvn_engine* h, rvn_graph* g, uint64_t* n_marked) {
  return guarded(h, h && g, "[raven_hip] rvn_graph_mark_transitive: NULL argument", [&](Engine& e) -> int {
    if (g->device != e.device) return fail(RVN_EINVAL, "[raven_hip] rvn_graph_mark_transitive: the graph lives on another device");
    const u64 m = graph_mark_transitive(e, g->g);
    if (n_marked) *n_marked = m;
    return RVN_OK;
  });
}

int rvn_graph_fetch_transitive(const rvn_graph* g, uint32_t* marked_in_insertion_order, uint32_t* transitive_pairs, uint64_t* n_pairs) {
  return guarded([&]() -> int {
    if (!g) return fail(RVN_EINVAL, "[raven_hip] NULL graph");
    const GraphDev& x = g->g;
    if (!x.marked)
      return fail(RVN_EINVAL, "[raven_hip] rvn_graph_fetch_transitive: no completed rvn_graph_mark_transitive on this graph");
    if (marked_in_insertion_order && !x.order.empty()) std::memcpy(marked_in_insertion_order, x.order.data(), x.order.size() * 4);
    if (transitive_pairs && !x.pairs.empty()) std::memcpy(transitive_pairs, x.pairs.data(), x.pairs.size() * 4);
    if (n_pairs) *n_pairs = x.pairs.size() / 2;
    return RVN_OK;
  });
}

int rvn_graph_mark_long_edges(rvn_engine* h, const rvn_graph* g, const double* weight, uint8_t* marked, uint64_t* n_marked) {
  const bool args_ok = h && g && (g->g.n_edges == 0 || weight);
  return guarded(h, args_ok, "[raven_hip] rvn_graph_mark_long_edges: NULL argument", [&](Engine& e) -> int {
    if (g->device != e.device) return fail(RVN_EINVAL, "[raven_hip] rvn_graph_mark_long_edges: the graph lives on another device");
    for (u64 i = 0; i < g->g.n_edges; ++i)
      if (std::isnan(weight[i]))
        return fail(RVN_EINVAL, "[raven_hip] rvn_graph_mark_long_edges: the weight of edge " + std::to_string(i) + " is not a number");
    const u64 m = graph_mark_long_edges(e, g->g, weight, marked);
    if (n_marked) *n_marked = m;
    return RVN_OK;
  });
}

void rvn_graph_destroy(rvn_graph* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  delete g;
}

int rvn_tiling_from_piles(rvn_engine* h, const rvn_reads* reads, uint32_t n_nodes, const uint32_t* node_pile, uint32_t n_piles,
                          const uint32_t* pile_begin, const uint32_t* pile_end, rvn_tiling** out) {
  const bool args_ok = h && reads && out && (n_nodes == 0 || (node_pile && pile_begin && pile_end));
  return guarded(h, args_ok, "[raven_hip] rvn_tiling_from_piles: NULL argument", [&](Engine& e) -> int {
    *out = nullptr;
    if (n_nodes > kMaxGraphNodes) return fail(RVN_EINVAL, "[raven_hip] rvn_tiling_from_piles: more than 2^31 nodes");
    std::unique_ptr<rvn_tiling> t(new rvn_tiling());
    t->device = e.device;
    tiling_from_piles(e, reads->r, n_nodes, node_pile, n_piles, pile_begin, pile_end, t->t);
    *out = t.release();
    return RVN_OK;
  });
}

int rvn_tiling_from_segments(rvn_engine* h, const rvn_reads* reads, uint32_t n_nodes, const uint64_t* segment_offsets,
                             const uint32_t* segment_read, const uint32_t* segment_begin, const uint32_t* segment_length,
                             const uint8_t* segment_strand, rvn_tiling** out) {
  const bool have = segment_offsets && (segment_offsets[n_nodes] == 0 || (segment_read && segment_begin && segment_length && segment_strand));
  const bool args_ok = h && reads && out && segment_offsets && have;
  return guarded(h, args_ok, "[raven_hip] rvn_tiling_from_segments: NULL argument", [&](Engine& e) -> int {
    *out = nullptr;
    if (n_nodes > kMaxGraphNodes) return fail(RVN_EINVAL, "[raven_hip] rvn_tiling_from_segments: more than 2^31 nodes");
    std::unique_ptr<rvn_tiling> t(new rvn_tiling());
    t->device = e.device;
    tiling_from_segments(e, reads->r, n_nodes, segment_offsets, segment_read, segment_begin, segment_length, segment_strand, t->t);
    *out = t.release();
    return RVN_OK;
  });
}

int rvn_tiling_info(const rvn_tiling* t, uint32_t* n_nodes, uint64_t* n_segments) {
  return guarded([&]() -> int {
    if (!t) return fail(RVN_EINVAL, "[raven_hip] NULL tiling");
    if (n_nodes) *n_nodes = t->t.n_nodes;
    if (n_segments) *n_segments = t->t.n_segs;
    return RVN_OK;
  });
}

int rvn_tiling_fetch(const rvn_tiling* t, uint64_t* segment_offsets, uint32_t* segment_read, uint32_t* segment_begin,
                     uint32_t* segment_length, uint8_t* segment_strand, uint32_t* node_length) {
  return guarded([&]() -> int {
    if (!t) return fail(RVN_EINVAL, "[raven_hip] NULL tiling");
    RVN_HIP(hipSetDevice(t->device));
    tiling_fetch(t->t, segment_offsets, segment_read, segment_begin, segment_length, segment_strand, node_length);
    return RVN_OK;
  });
}

void rvn_tiling_destroy(rvn_tiling* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  delete t;
}

int rvn_graph_create_unitigs(rvn_engine* h, const rvn_graph* g, rvn_tiling* t, const uint32_t* count, const uint16_t* coverage,
                             uint32_t epsilon, uint32_t min_unitig_size, rvn_unitigs** out) {
  const bool args_ok = h && g && t && out && (g->g.n_nodes == 0 || (count && coverage));
  return guarded(h, args_ok, "[raven_hip] rvn_graph_create_unitigs: NULL argument", [&](Engine& e) -> int {
    *out = nullptr;
    if (g->device != e.device || t->device != e.device)
      return fail(RVN_EINVAL, "[raven_hip] rvn_graph_create_unitigs: the graph or the tiling lives on another device");
    std::unique_ptr<rvn_unitigs> u(new rvn_unitigs());
    graph_create_unitigs(e, g->g, t->t, count, coverage, epsilon, min_unitig_size, u->u);
    *out = u.release();
    return RVN_OK;
  });
}

int rvn_unitigs_info(const rvn_unitigs* u, uint32_t* first_node, uint32_t* n_new_nodes, uint64_t* n_members, uint64_t* first_edge,
                     uint64_t* n_new_edges) {
  return guarded([&]() -> int {
    if (!u) return fail(RVN_EINVAL, "[raven_hip] NULL unitigs");
    if (first_node) *first_node = u->u.first_node;
    if (n_new_nodes) *n_new_nodes = static_cast<u32>(u->u.begin.size());
    if (n_members) *n_members = u->u.members.size();
    if (first_edge) *first_edge = u->u.first_edge;
    if (n_new_edges) *n_new_edges = u->u.edge_tail.size();
    return RVN_OK;
  });
}

int rvn_unitigs_fetch(const rvn_unitigs* u, uint32_t* begin, uint32_t* end, uint8_t* is_circular, uint32_t* count, uint32_t* length,
                      uint16_t* coverage, uint8_t* is_unitig, uint64_t* member_offsets, uint32_t* members, uint8_t* marked,
                      uint32_t* edge_tail, uint32_t* edge_head, uint32_t* edge_length) {
  return guarded([&]() -> int {
    if (!u) return fail(RVN_EINVAL, "[raven_hip] NULL unitigs");
    const UnitigTables& x = u->u;
    give(begin, x.begin), give(end, x.end), give(is_circular, x.is_circular), give(count, x.count), give(length, x.length);
    give(coverage, x.coverage), give(is_unitig, x.is_unitig), give(member_offsets, x.member_off), give(members, x.members);
    give(marked, x.marked), give(edge_tail, x.edge_tail), give(edge_head, x.edge_head), give(edge_length, x.edge_length);
    return RVN_OK;
  });
}

void rvn_unitigs_destroy(rvn_unitigs* u) { delete u; }

int rvn_unitigs_as_reads(rvn_engine* h, const rvn_unitigs* u, const rvn_tiling* t, const rvn_reads* reads, int selection,
                         rvn_reads** out) {
  return guarded(h, h && u && t && reads && out, "[raven_hip] rvn_unitigs_as_reads: NULL argument", [&](Engine& e) -> int {
    *out = nullptr;
    if (selection != RVN_UNITIGS_SELECTED && selection != RVN_UNITIGS_ALL)
      return fail(RVN_EINVAL, "[raven_hip] rvn_unitigs_as_reads: selection is neither RVN_UNITIGS_SELECTED nor RVN_UNITIGS_ALL");
    if (t->device != e.device) return fail(RVN_EINVAL, "[raven_hip] rvn_unitigs_as_reads: the tiling lives on another device");
    std::vector<u32> nodes;
    for (u32 j = 0; j < u->u.begin.size(); ++j)
      if (selection == RVN_UNITIGS_ALL || (!(j & 1u) && u->u.is_unitig[j])) nodes.push_back(u->u.first_node + j);
    return nodes_as_reads(e, t, reads, nodes, out);
  });
}

int rvn_tiling_as_reads(rvn_engine* h, const rvn_tiling* t, const rvn_reads* reads, const uint32_t* nodes, uint32_t n, rvn_reads** out) {
  return guarded(h, h && t && reads && out && (n == 0 || nodes), "[raven_hip] rvn_tiling_as_reads: NULL argument", [&](Engine& e) -> int {
    *out = nullptr;
    if (t->device != e.device) return fail(RVN_EINVAL, "[raven_hip] rvn_tiling_as_reads: the tiling lives on another device");
    return nodes_as_reads(e, t, reads, std::vector<u32>(nodes, nodes + n), out);
  });
}

int rvn_tiling_paths_as_reads(rvn_engine* h, const rvn_tiling* t, const rvn_reads* reads, uint32_t n_paths, const uint64_t* path_offsets,
                              const uint32_t* path_node, const uint32_t* path_label, rvn_reads** out) {
  const bool args_ok = h && t && reads && out && (n_paths == 0 || (path_offsets && path_node && path_label));
  return guarded(h, args_ok, "[raven_hip] rvn_tiling_paths_as_reads: NULL argument", [&](Engine& e) -> int {
    *out = nullptr;
    if (t->device != e.device) return fail(RVN_EINVAL, "[raven_hip] rvn_tiling_paths_as_reads: the tiling lives on another device");
    std::unique_ptr<rvn_reads> rr(new rvn_reads());
    tiling_paths_as_reads(e, t->t, reads->r, n_paths, path_offsets, path_node, path_label, rr->r);
    *out = rr.release();
    return RVN_OK;
  });
}

int rvn_path_similarity_batch(rvn_engine* h, const rvn_reads* paths, const rvn_path_pair* pairs, uint32_t n_pairs, double min_ratio,
                              uint8_t* similar, uint32_t* distance) {
  const bool args_ok = h && paths && (n_pairs == 0 || (pairs && similar));
  return guarded(h, args_ok, "[raven_hip] rvn_path_similarity_batch: NULL argument", [&](Engine& e) -> int {
    static_assert(sizeof(rvn_path_pair) == 8, "a pair is two read indices");
    path_similarity_batch(e, paths->r, reinterpret_cast<const u32*>(pairs), n_pairs, min_ratio, similar, distance);
    return RVN_OK;
  });
}

int rvn_tiling_slices_as_reads(rvn_engine* h, const rvn_tiling* t, const rvn_reads* reads, uint32_t n, const uint32_t* node,
                               const uint32_t* begin, const uint32_t* length, rvn_reads** out) {
  const bool args_ok = h && t && reads && out && (n == 0 || (node && begin && length));
  return guarded(h, args_ok, "[raven_hip] rvn_tiling_slices_as_reads: NULL argument", [&](Engine& e) -> int {
    *out = nullptr;
    if (t->device != e.device) return fail(RVN_EINVAL, "[raven_hip] rvn_tiling_slices_as_reads: the tiling lives on another device");
    std::unique_ptr<rvn_reads> rr(new rvn_reads());
    tiling_slices_as_reads(e, t->t, reads->r, n, node, begin, length, rr->r);
    *out = rr.release();
    return RVN_OK;
  });
}

int rvn_graph_edge_similarity(rvn_engine* h, const rvn_graph* g, const rvn_tiling* t, const rvn_reads* reads, uint32_t* lhs_length,
                              uint32_t* rhs_length, uint32_t* distance, double* score) {
  return guarded(h, h && g && t && reads, "[raven_hip] rvn_graph_edge_similarity: NULL argument", [&](Engine& e) -> int {
    if (g->device != e.device || t->device != e.device)
      return fail(RVN_EINVAL, "[raven_hip] rvn_graph_edge_similarity: the graph or the tiling lives on another device");
    const u64 E = g->g.n_edges;
    // the score needs both numbers, whichever of them the caller wants
    std::vector<u32> own_lhs, own_dist;
    u32* lhs = lhs_length;
    u32* dist = distance;
    if (score && !lhs) own_lhs.resize(E), lhs = own_lhs.data();
    if (score && !dist) own_dist.resize(E), dist = own_dist.data();
    graph_edge_similarity(e, g->g, t->t, reads->r, lhs, rhs_length, dist);
    if (score)  // graph_repr.cc:254, in double on the host (this unit is built without fast-math); an empty slot has no score
      for (u64 i = 0; i < E; ++i) score[i] = dist[i] == 0xFFFFFFFFu ? std::nan("") : 1 - dist[i] / static_cast<double>(lhs[i]);
    return RVN_OK;
  });
}

}  // extern "C"
