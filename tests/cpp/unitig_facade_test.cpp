// TEST INFRASTRUCTURE: raven::CreateUnitigs (include/raven_hip/unitigs.hpp) beside the same routine restated on the host in
// this program, over the same graph doubles (unitig_doubles.hpp) on the same seeded graph: chains of every kind between
// junctions and dead ends, cycles, seeded `transitive` sets — first with epsilon = 42, then, as GetUnitigs does, with
// epsilon = 0 on the graph the first call left.  Compared after each call: the return value, every node (id, name,
// sequence, count, coverage, is_unitig, is_circular, pair, in- and out-lists, `transitive` in ITERATION order, the
// original_node_sequence_names) and every edge.  Exits 3 on a difference.  usage: unitig_facade_test [seed]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "unitig_doubles.hpp"
#include "raven_hip/unitigs.hpp"

namespace {

using unitig_doubles::Edge;
using unitig_doubles::Graph;
using unitig_doubles::Node;
using unitig_doubles::Pile;
using unitig_doubles::Sequence;
using Piles = std::vector<std::unique_ptr<Pile>>;

constexpr std::uint32_t kMinUnitigSize = 3000;

// One unitig over first -> ... -> last: the labels of the edges on the way, then the whole of `last` unless the walk is a
// round trip; through the factory like every node.
std::unique_ptr<Node> HostUnitig(Graph& graph, Node* first, Node* last) {
  std::string data;
  std::uint32_t count = 0;
  Node* at = first;
  do {
    data += at->outedges.front()->Label();
    count += at->count;
    at = at->outedges.front()->head;
  } while (at != last);
  if (first != last) {
    data += last->sequence.InflateData();
    count += last->count;
  }
  const bool is_unitig = count > 5 && data.size() > kMinUnitigSize;
  const std::uint32_t id = graph.node_factory.NextIndex();
  auto u = graph.node_factory.MakeUnique(Sequence((is_unitig ? "Utg" : "Ctg") + std::to_string(id & ~1u), data));
  u->count = count;
  u->is_unitig = is_unitig;
  u->is_circular = first == last;
  return u;
}

std::uint32_t HostCreateUnitigs(Graph& graph, std::uint32_t epsilon) {
  std::unordered_set<std::uint32_t> marked;
  std::vector<std::unique_ptr<Node>> made;
  std::vector<std::unique_ptr<Edge>> links;
  std::vector<std::uint32_t> moved_to(graph.nodes.size(), 0);
  std::vector<char> seen(graph.nodes.size(), 0);
  auto link = [&](Node* t, Node* h, std::uint32_t len) {
    links.emplace_back(graph.edge_factory.MakeUnique(t, h, len));
    return links.back().get();
  };
  for (const auto& slot : graph.nodes) {
    Node* start = slot.get();
    if (!start || seen[start->id] || start->is_junction()) continue;
    std::uint32_t walked = 1;
    bool circular = false;
    Node* first = start;
    while (!first->is_junction()) {
      seen[first->id] = seen[first->pair->id] = 1;
      if (first->inedges.empty() || first->inedges.front()->tail->is_junction()) break;
      first = first->inedges.front()->tail;
      ++walked;
      if (first == start) {
        circular = true;
        break;
      }
    }
    Node* last = start;
    while (!last->is_junction()) {
      seen[last->id] = seen[last->pair->id] = 1;
      if (last->outedges.empty() || last->outedges.front()->head->is_junction()) break;
      last = last->outedges.front()->head;
      ++walked;
      if (last == start) {
        circular = true;
        break;
      }
    }
    if (!circular && (first == last || walked < 2 * epsilon + 2)) continue;
    if (first != last)
      for (std::uint32_t i = 0; i < epsilon; ++i) {
        first = first->outedges.front()->head;
        last = last->inedges.front()->tail;
      }
    made.emplace_back(HostUnitig(graph, first, last));
    Node* unitig = made.back().get();
    made.emplace_back(HostUnitig(graph, last->pair, first->pair));
    Node* rc = made.back().get();
    unitig->coverage = rc->coverage = static_cast<std::uint16_t>((first->coverage + last->coverage) / 2);
    unitig->pair = rc;
    rc->pair = unitig;
    std::vector<Edge*> taken;  // the edges this unitig replaces
    if (first != last) {
      if (first->indegree()) {
        Edge* in = first->inedges.front();
        taken.push_back(in);
        Edge* a = link(in->tail, unitig, in->length);
        Edge* b = link(rc, in->pair->head,
                       in->pair->length + static_cast<std::uint32_t>(rc->sequence.data.size()) - static_cast<std::uint32_t>(first->pair->sequence.data.size()));
        a->pair = b;
        b->pair = a;
      }
      if (last->outdegree()) {
        Edge* out = last->outedges.front();
        taken.push_back(out);
        Edge* a = link(unitig, out->head,
                       out->length + static_cast<std::uint32_t>(unitig->sequence.data.size()) - static_cast<std::uint32_t>(last->sequence.data.size()));
        Edge* b = link(out->pair->tail, rc, out->pair->length);
        a->pair = b;
        b->pair = a;
      }
    }
    Node* at = first;
    do {
      taken.push_back(at->outedges.front());
      moved_to[at->id & ~1u] = unitig->id;
      const auto& src = graph.nodes[at->id & ~1u]->transitive;
      unitig->transitive.insert(src.begin(), src.end());
      at = at->outedges.front()->head;
    } while (at != last);
    for (Edge* e : taken) {
      marked.insert(e->id);
      marked.insert(e->pair->id);
      for (Node* x : {e->head, e->tail}) {
        unitig->original_node_sequence_names.insert(x->sequence.name);
        rc->original_node_sequence_names.insert(x->pair->sequence.name);
      }
    }
  }
  const std::uint32_t n_made = static_cast<std::uint32_t>(made.size());
  for (auto& n : made) graph.nodes.emplace_back(std::move(n));
  for (auto& e : links) graph.edges.emplace_back(std::move(e));
  RemoveEdges(graph, marked, true);
  for (const auto& it : graph.nodes) {
    if (!it) continue;
    std::unordered_set<std::uint32_t> valid;
    for (auto jt : it->transitive) valid.emplace(moved_to[jt] == 0 ? jt : moved_to[jt]);
    it->transitive.swap(valid);
  }
  return n_made / 2;
}

struct Input {
  std::vector<std::string> reads;
  Piles piles;
  struct Join {
    std::uint32_t tail, head, length, length_pair;
  };
  std::vector<Join> joins;
  std::vector<std::pair<std::uint32_t, std::uint32_t>> transitive;  // (node, id) insertions
  std::vector<std::uint32_t> count;
};

void Build(const Input& in, Graph& graph) {
  for (std::size_t i = 0; i < in.piles.size(); ++i) {
    const Pile& p = *in.piles[i];
    if (p.is_invalid()) continue;
    Sequence s("read" + std::to_string(i), in.reads[i].substr(p.begin(), p.length()));
    graph.nodes.emplace_back(graph.node_factory.MakeUnique(s));
    s.ReverseAndComplement();
    graph.nodes.emplace_back(graph.node_factory.MakeUnique(s));
    Node* f = graph.nodes[graph.nodes.size() - 2].get();
    Node* r = graph.nodes.back().get();
    f->pair = r;
    r->pair = f;
    f->coverage = r->coverage = p.median();
    f->count = r->count = in.count[f->id / 2];
  }
  for (const auto& j : in.joins) {
    graph.edges.emplace_back(graph.edge_factory.MakeUnique(graph.nodes[j.tail].get(), graph.nodes[j.head].get(), j.length));
    graph.edges.emplace_back(graph.edge_factory.MakeUnique(graph.nodes[j.head]->pair, graph.nodes[j.tail]->pair, j.length_pair));
    Edge* a = graph.edges[graph.edges.size() - 2].get();
    Edge* b = graph.edges.back().get();
    a->pair = b;
    b->pair = a;
  }
  for (const auto& t : in.transitive) graph.nodes[t.first]->transitive.insert(t.second);
}

template <typename T>
std::vector<std::uint32_t> Ids(const std::vector<T*>& v) {
  std::vector<std::uint32_t> r;
  for (auto* x : v) r.push_back(x->id);
  return r;
}

bool Same(const Graph& a, const Graph& b, const char* when) {
  auto fail = [&](const char* what, std::size_t i) {
    std::fprintf(stderr, "%s: %s differs at %zu\n", when, what, i);
    return false;
  };
  if (a.nodes.size() != b.nodes.size() || a.edges.size() != b.edges.size()) return fail("sizes", 0);
  for (std::size_t i = 0; i < a.nodes.size(); ++i) {
    const Node* x = a.nodes[i].get();
    const Node* y = b.nodes[i].get();
    if (!x != !y) return fail("node presence", i);
    if (!x) continue;
    if (x->id != y->id || x->sequence.name != y->sequence.name || x->sequence.data != y->sequence.data) return fail("node sequence", i);
    if (x->count != y->count || x->coverage != y->coverage || x->is_unitig != y->is_unitig || x->is_circular != y->is_circular || x->pair->id != y->pair->id)
      return fail("node fields", i);
    if (Ids(x->inedges) != Ids(y->inedges) || Ids(x->outedges) != Ids(y->outedges)) return fail("edge lists", i);
    if (std::vector<std::uint32_t>(x->transitive.begin(), x->transitive.end()) != std::vector<std::uint32_t>(y->transitive.begin(), y->transitive.end()))
      return fail("transitive iteration order", i);
    std::vector<std::string> nx(x->original_node_sequence_names.begin(), x->original_node_sequence_names.end());
    std::vector<std::string> ny(y->original_node_sequence_names.begin(), y->original_node_sequence_names.end());
    std::sort(nx.begin(), nx.end());
    std::sort(ny.begin(), ny.end());
    if (nx != ny) return fail("sequence names", i);
  }
  for (std::size_t i = 0; i < a.edges.size(); ++i) {
    const Edge* x = a.edges[i].get();
    const Edge* y = b.edges[i].get();
    if (!x != !y) return fail("edge presence", i);
    if (!x) continue;
    if (x->id != y->id || x->tail->id != y->tail->id || x->head->id != y->head->id || x->length != y->length || x->pair->id != y->pair->id)
      return fail("edge", i);
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? static_cast<unsigned>(std::atoi(argv[1])) : 1;
  std::mt19937 rng(seed);
  auto pick = [&](std::uint32_t lo, std::uint32_t hi) { return lo + static_cast<std::uint32_t>(rng() % (hi - lo + 1)); };

  // reads and piles; every seventh pile invalid
  Input in;
  const std::uint32_t n_reads = 420;
  for (std::uint32_t i = 0; i < n_reads; ++i) {
    std::string s(pick(150, 300), 'A');
    for (auto& c : s) c = "ACGT"[rng() % 4];
    in.reads.push_back(s);
    in.piles.emplace_back(new Pile());
    Pile& p = *in.piles.back();
    p.id_ = i;
    p.begin_ = pick(0, 20);
    p.end_ = static_cast<std::uint32_t>(s.size()) - pick(0, 20);
    p.median_ = static_cast<std::uint16_t>(pick(1, 60000));
    p.invalid_ = i % 7 == 3;
  }
  std::vector<std::uint32_t> lengths;  // per node pair
  for (const auto& p : in.piles)
    if (!p->is_invalid()) lengths.push_back(p->length());
  const std::uint32_t n_pairs = static_cast<std::uint32_t>(lengths.size());
  for (std::uint32_t i = 0; i < n_pairs; ++i) in.count.push_back(pick(1, 4));
  std::vector<std::uint32_t> order(n_pairs);
  for (std::uint32_t i = 0; i < n_pairs; ++i) order[i] = i;
  std::shuffle(order.begin(), order.end(), rng);
  auto join = [&](std::uint32_t t, std::uint32_t h) {
    in.joins.push_back({t, h, pick(0, lengths[t / 2]), pick(0, lengths[h / 2])});
  };
  // chains of 130 and 100 node pairs (more than 2 * 42 + 2), short ones, cycles, a junction behind every third chain
  std::uint32_t at = 0, k = 0;
  for (std::uint32_t len : {130u, 100u, 1u, 2u, 3u, 7u, 12u, 5u, 1u, 9u, 30u, 4u, 2u, 6u}) {
    std::vector<std::uint32_t> ids;
    for (std::uint32_t i = 0; i < len; ++i) ids.push_back(2 * order[at++] + (rng() % 2));
    const bool circular = k % 4 == 3;
    for (std::uint32_t i = 0; i + 1 < len; ++i) join(ids[i], ids[i + 1]);
    if (circular) join(ids.back(), ids.front());
    if (!circular && k % 3 == 0) {
      const std::uint32_t j = 2 * order[at++];
      join(ids.back(), j);
      join(j, 2 * order[at++]);
      join(j, 2 * order[at++] + 1);
    }
    ++k;
  }
  for (std::uint32_t i = 0; i < 600; ++i) in.transitive.push_back({pick(0, 2 * n_pairs - 1), 2 * pick(0, n_pairs - 1)});

  Graph host, dev;
  Build(in, host);
  Build(in, dev);
  if (!Same(host, dev, "before")) return 3;

  rvn_engine* engine = nullptr;
  if (rvn_engine_create(&engine, 15, 5, 500, 4, 100, 10000, 0) != RVN_OK) {
    std::fprintf(stderr, "%s\n", rvn_last_error());
    return 2;
  }
  std::vector<std::uint8_t> codes;
  std::vector<std::uint64_t> offsets(1, 0);
  for (const auto& s : in.reads) {
    for (char c : s) codes.push_back(c == 'A' ? 0 : (c == 'C' ? 1 : (c == 'G' ? 2 : 3)));
    offsets.push_back(codes.size());
  }
  rvn_reads* reads = nullptr;
  if (rvn_reads_upload_codes(engine, codes.data(), offsets.data(), nullptr, n_reads, &reads) != RVN_OK) return 2;
  int rc = 0;
  {
    raven::Tilings tilings;
    raven::MakeTilings(engine, reads, in.piles, &tilings);
    for (std::uint32_t epsilon : {42u, 0u}) {
      const std::uint32_t want = HostCreateUnitigs(host, epsilon);
      const std::uint32_t got = raven::CreateUnitigs(engine, dev, reads, tilings, epsilon, kMinUnitigSize);
      std::printf("epsilon %u: %u unitigs (host %u), %zu nodes, %zu edges\n", epsilon, got, want, dev.nodes.size(), dev.edges.size());
      if (got != want || want == 0 || !Same(host, dev, epsilon ? "after epsilon 42" : "after epsilon 0")) {
        rc = 3;
        break;
      }
    }
    // a graph whose factory has run ahead is refused
    if (rc == 0) {
      dev.node_factory.MakeUnique(Sequence("x", "ACGT"));
      try {
        raven::CreateUnitigs(engine, dev, reads, tilings, 0);
        rc = 3;
      } catch (const std::invalid_argument&) {
      }
    }
  }
  rvn_reads_destroy(reads);
  rvn_engine_destroy(engine);
  if (rc == 0) std::printf("OK\n");
  return rc;
}
