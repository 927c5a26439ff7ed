// abi_graph.hip — C ABI (include/raven_hip.h): the assembly graph on the device (graph.hip): rvn_construct_assembly_graph,
// rvn_graph_from_edges, the marking of transitive and long edges, and what a graph handle gives back.
#include <cmath>
#include <cstring>

#include "abi.h"
#include "graph_rules.h"

using namespace rvn;

struct rvn_graph {
  GraphDev g;
  int device = 0;
};

namespace {

constexpr u32 kMaxGraphNodes = 1u << 31;  // node ids are int32 in sequence_to_node

template <typename T>
void fetch(T* dst, const DevBuf& src, u64 count) {
  if (dst && count) RVN_HIP(hipMemcpy(dst, src.ptr, count * sizeof(T), hipMemcpyDeviceToHost));
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

}  // extern "C"
