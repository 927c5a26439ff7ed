// TEST INFRASTRUCTURE: raven::ConstructAssemblyGraph, RemoveTransitiveEdges and MarkLongEdges
// (include/raven_hip/assembly_graph.hpp) on seeded piles / overlaps / sequences, in ConstructGraph -> Assemble order,
// against the same three steps restated on the host in this program over the same graph doubles (graph_doubles.hpp).
// Compared after every step: node and edge ids, pairs, coverage, sequences, lengths, every node's in- and out-lists, every
// node's `transitive` set in ITERATION order, the finalized overlaps, the return value of RemoveTransitiveEdges and the
// long-edge set.  Exits 3 on a difference.  usage: assembly_graph_test [seed] [reads]
#include <cstdio>
#include <cstdlib>
#include <random>

#include "biosoup/overlap.hpp"
#include "graph_doubles.hpp"
#include "raven_hip/assembly_graph.hpp"

namespace {

using graph_doubles::Edge;
using graph_doubles::Graph;
using graph_doubles::Node;
using graph_doubles::Pile;
using graph_doubles::Sequence;
using Piles = std::vector<std::unique_ptr<Pile>>;
using Sequences = std::vector<std::unique_ptr<Sequence>>;
using Overlaps = std::vector<std::vector<biosoup::Overlap>>;

// The overlap's type against the two valid regions (what GetOverlapType decides): 0 when the parts that stick out beside
// the overlap are more than an eighth of either side, 1 / 2 when the lhs / rhs lies inside the other read, 3 when the lhs
// runs into the rhs, 4 when the rhs runs into the lhs.  All in 32-bit unsigned arithmetic.
std::uint32_t TypeOf(const biosoup::Overlap& o, const Piles& piles) {
  const std::uint32_t l_len = piles[o.lhs_id]->length(), r_len = piles[o.rhs_id]->length();
  const std::uint32_t l_at = piles[o.lhs_id]->begin(), r_at = piles[o.rhs_id]->begin();
  const std::uint32_t lb = o.lhs_begin - l_at, le = o.lhs_end - l_at;
  std::uint32_t rb = o.rhs_begin - r_at, re = o.rhs_end - r_at;
  if (!o.strand) {
    const std::uint32_t t = rb;
    rb = r_len - re;
    re = r_len - t;
  }
  const std::uint32_t l_after = l_len - le, r_after = r_len - re;
  const std::uint32_t loose = std::min(lb, rb) + std::min(l_after, r_after);
  const std::uint32_t l_span = le - lb, r_span = re - rb;
  if (l_span < (l_span + loose) * 0.875 || r_span < (r_span + loose) * 0.875) return 0;
  if (lb <= rb && l_after <= r_after) return 1;
  if (rb <= lb && r_after <= l_after) return 2;
  return lb > rb ? 3 : 4;
}

// The host graph the facade's is compared with, built the way the reference builds it: the type of EVERY overlap goes
// into its score; an overlap of type 3 or 4 is moved into the coordinates of the valid regions (rhs mirrored between
// opposite strands) and becomes two edges.
void HostConstruct(Graph& graph, const Piles& piles, Overlaps& overlaps, const Sequences& sequences) {
  std::vector<std::int64_t> first_node(piles.size(), -1);
  for (std::size_t i = 0; i < piles.size(); ++i) {
    const Pile& p = *piles[i];
    if (p.is_invalid()) continue;
    first_node[i] = static_cast<std::int64_t>(graph.nodes.size());
    Sequence s(sequences[i]->name, sequences[i]->InflateData(p.begin(), p.length()));
    graph.nodes.emplace_back(graph.node_factory.MakeUnique(s));
    s.ReverseAndComplement();
    graph.nodes.emplace_back(graph.node_factory.MakeUnique(s));
    Node* fwd = graph.nodes[graph.nodes.size() - 2].get();
    Node* rev = graph.nodes.back().get();
    fwd->coverage = rev->coverage = p.median();
    fwd->pair = rev;
    rev->pair = fwd;
  }
  for (biosoup::Overlap& o : overlaps.back()) {
    o.score = TypeOf(o, piles);
    if (o.score < 3) continue;
    const Pile &L = *piles[o.lhs_id], &R = *piles[o.rhs_id];
    const std::uint32_t lb = o.lhs_begin - L.begin(), le = o.lhs_end - L.begin();
    std::uint32_t rb = o.rhs_begin - R.begin(), re = o.rhs_end - R.begin();
    if (!o.strand) {
      const std::uint32_t t = rb;
      rb = R.length() - re;
      re = R.length() - t;
    }
    o.lhs_begin = lb;
    o.lhs_end = le;
    o.rhs_begin = rb;
    o.rhs_end = re;
    Node* from = graph.nodes[static_cast<std::size_t>(first_node[o.lhs_id])].get();
    Node* to = graph.nodes[static_cast<std::size_t>(first_node[o.rhs_id]) + (o.strand ? 0 : 1)].get();
    std::uint32_t span = lb - rb, twin_span = (R.length() - re) - (L.length() - le);
    if (o.score == 4) {
      std::swap(from, to);
      span = 0u - span;
      twin_span = 0u - twin_span;
    }
    graph.edges.emplace_back(graph.edge_factory.MakeUnique(from, to, span));
    graph.edges.emplace_back(graph.edge_factory.MakeUnique(to->pair, from->pair, twin_span));
    Edge* a = graph.edges[graph.edges.size() - 2].get();
    Edge* b = graph.edges.back().get();
    a->pair = b;
    b->pair = a;
  }
}

bool InBand(double x, double y) {
  const double tolerance = 0.12;
  return x >= y * (1 - tolerance) && x <= y * (1 + tolerance);
}

// RemoveTransitiveEdges on the host graph.  The marked ids live in a std::unordered_set, as in the reference, because
// its ITERATION order decides the order in which the nodes' `transitive` sets are filled.
std::uint32_t HostRemoveTransitiveEdges(Graph& graph) {
  std::vector<Edge*> direct(graph.nodes.size(), nullptr);  // per node v: the last out-edge of v into each node
  std::unordered_set<std::uint32_t> marked;
  for (std::size_t v = 0; v < graph.nodes.size(); ++v) {
    if (!graph.nodes[v]) continue;
    const std::vector<Edge*>& out = graph.nodes[v]->outedges;
    for (Edge* e : out) direct[e->head->id] = e;
    for (Edge* first : out)
      for (Edge* second : first->head->outedges) {
        Edge* shortcut = direct[second->head->id];
        if (!shortcut) continue;
        const std::uint32_t walk = first->length + second->length;
        if (InBand(walk, shortcut->length) || InBand(shortcut->length, walk)) {
          marked.insert(shortcut->id);
          marked.insert(shortcut->pair->id);
        }
      }
    for (Edge* e : out) direct[e->head->id] = nullptr;
  }
  for (std::uint32_t id : marked) {
    if (id % 2 == 0) continue;
    const std::uint32_t a = graph.edges[id]->tail->id & ~1u, b = graph.edges[id]->head->id & ~1u;
    graph.nodes[a]->transitive.insert(b);
    graph.nodes[b]->transitive.insert(a);
  }
  RemoveEdges(graph, marked);
  return static_cast<std::uint32_t>(marked.size() / 2);
}

// The marking loop of RemoveLongEdges: an out-edge that weighs more than twice some other out-edge of its node
std::unordered_set<std::uint32_t> HostMarkLongEdges(const Graph& graph) {
  std::unordered_set<std::uint32_t> marked;
  for (const auto& node : graph.nodes) {
    if (!node || node->outdegree() < 2) continue;
    const std::vector<Edge*>& out = node->outedges;
    for (std::size_t k = 0; k < out.size(); ++k)
      for (std::size_t j = 0; j < out.size(); ++j)
        if (j != k && out[j]->weight * 2.0 < out[k]->weight) {
          marked.insert(out[k]->id);
          marked.insert(out[k]->pair->id);
        }
  }
  return marked;
}

std::uint64_t Differences(const Graph& a, const Graph& b) {
  std::uint64_t d = 0;
  if (a.nodes.size() != b.nodes.size() || a.edges.size() != b.edges.size()) return 1;
  auto ids = [](const std::vector<Edge*>& l) {
    std::vector<std::uint32_t> v;
    for (auto e : l) v.push_back(e->id);
    return v;
  };
  for (std::size_t i = 0; i < a.nodes.size(); ++i) {
    const auto &x = a.nodes[i], &y = b.nodes[i];
    if (!x || !y) {
      d += (!x) != (!y);
      continue;
    }
    d += x->id != y->id || x->pair->id != y->pair->id || x->coverage != y->coverage || x->sequence.data != y->sequence.data ||
         x->sequence.name != y->sequence.name || ids(x->outedges) != ids(y->outedges) || ids(x->inedges) != ids(y->inedges);
    d += std::vector<std::uint32_t>(x->transitive.begin(), x->transitive.end()) !=
         std::vector<std::uint32_t>(y->transitive.begin(), y->transitive.end());  // the iteration order
  }
  for (std::size_t i = 0; i < a.edges.size(); ++i) {
    const auto &x = a.edges[i], &y = b.edges[i];
    if (!x || !y) {
      d += (!x) != (!y);
      continue;
    }
    d += x->id != y->id || x->pair->id != y->pair->id || x->tail->id != y->tail->id || x->head->id != y->head->id ||
         x->length != y->length || x->weight != y->weight;
  }
  return d;
}

struct Input {
  Piles piles;
  Sequences sequences;
  Overlaps overlaps;
};

// reads every ~700 bases of a line, 8 kb each, every fifth stored reverse-complemented, valid regions trimmed by up to
// 240 bases, every ninth pile invalid; each read against the next six, every other overlap listed from the far side
Input MakeInput(std::uint32_t seed, std::uint32_t n) {
  std::mt19937 rng(seed);
  auto pick = [&](std::uint32_t m) { return static_cast<std::uint32_t>(rng() % m); };
  Input in;
  std::vector<std::uint32_t> pos(n), len(n), rev(n);
  for (std::uint32_t i = 0; i < n; ++i) {
    pos[i] = 700 * i + pick(200);
    len[i] = 8000 + pick(900);
    rev[i] = i % 5 == 3;
    std::string s(len[i], 'A');
    for (auto& c : s) c = "ACGT"[pick(4)];
    in.sequences.emplace_back(new Sequence("read" + std::to_string(i), s));
    in.piles.emplace_back(new Pile());
    Pile& p = *in.piles.back();
    p.id_ = i;
    p.begin_ = 16 * pick(16);
    p.end_ = len[i] - 16 * pick(16);
    p.median_ = static_cast<std::uint16_t>(10 + pick(40));
    p.invalid_ = i % 9 == 4;
  }
  in.overlaps.resize(n + 1);
  for (std::uint32_t i = 0; i < n; ++i) {
    for (std::uint32_t d = 1; d <= 6 && i + d < n; ++d) {
      const std::uint32_t j = i + d;
      if (in.piles[i]->is_invalid() || in.piles[j]->is_invalid()) continue;
      const std::uint32_t b = pos[j], e = std::min(pos[i] + len[i], pos[j] + len[j]);
      if (e <= b + 500) continue;
      auto span = [&](std::uint32_t r, std::uint32_t& sb, std::uint32_t& se) {
        sb = b - pos[r];
        se = e - pos[r];
        if (rev[r]) {
          const std::uint32_t t = sb;
          sb = len[r] - se;
          se = len[r] - t;
        }
        sb = std::max(sb, in.piles[r]->begin());
        se = std::min(se, in.piles[r]->end());
      };
      std::uint32_t ib, ie, jb, je;
      span(i, ib, ie);
      span(j, jb, je);
      const bool strand = rev[i] == rev[j];
      if ((i + d) % 2) in.overlaps.back().emplace_back(i, ib, ie, j, jb, je, 0, strand);
      else in.overlaps.back().emplace_back(j, jb, je, i, ib, ie, 0, strand);
    }
  }
  return in;
}

}  // namespace

int main(int argc, char** argv) {
  const std::uint32_t seed = argc > 1 ? static_cast<std::uint32_t>(std::atoi(argv[1])) : 5;
  const std::uint32_t n = argc > 2 ? static_cast<std::uint32_t>(std::atoi(argv[2])) : 600;
  rvn_engine* engine = nullptr;
  if (rvn_engine_create(&engine, 15, 5, 500, 4, 100, 10000, 0) != RVN_OK) {
    std::printf("%s\n", rvn_last_error());
    return 1;
  }
  int rc = 0;
  try {
    Input dev_in = MakeInput(seed, n), host_in = MakeInput(seed, n);
    Graph dev, host;
    raven::ConstructAssemblyGraph(engine, dev, dev_in.piles, dev_in.overlaps, dev_in.sequences);
    HostConstruct(host, host_in.piles, host_in.overlaps, host_in.sequences);
    std::uint64_t ovl_diff = 0, type4 = 0;
    for (std::size_t i = 0; i < host_in.overlaps.back().size(); ++i) {
      const auto &x = dev_in.overlaps.back()[i], &y = host_in.overlaps.back()[i];
      // (the reference leaves the type in the score of EVERY overlap; the facade finalizes only the overlaps that make an
      // edge and leaves the others untouched — their scores are the one field left out of the comparison)
      const bool makes_edge = y.score >= 3;
      ovl_diff += x.lhs_begin != y.lhs_begin || x.lhs_end != y.lhs_end || x.rhs_begin != y.rhs_begin || x.rhs_end != y.rhs_end ||
                  (makes_edge && x.score != y.score) || (!makes_edge && x.score != 0);
      type4 += y.score == 4;
    }
    std::uint64_t diff = Differences(dev, host) + ovl_diff;
    std::printf("construct nodes %zu edges %zu type4 %llu differences %llu\n", host.nodes.size(), host.edges.size(),
                static_cast<unsigned long long>(type4), static_cast<unsigned long long>(diff));
    if (diff || host.edges.empty() || !type4) rc = 3;

    const std::uint32_t removed_dev = raven::RemoveTransitiveEdges(engine, dev);
    const std::uint32_t removed_host = HostRemoveTransitiveEdges(host);
    diff = Differences(dev, host);
    std::uint64_t live = 0, with_transitive = 0;
    for (const auto& e : host.edges) live += e != nullptr;
    for (const auto& v : host.nodes) with_transitive += !v->transitive.empty();
    std::printf("transitive removed %u %u live %llu nodes_with_transitive %llu differences %llu\n", removed_dev, removed_host,
                static_cast<unsigned long long>(live), static_cast<unsigned long long>(with_transitive),
                static_cast<unsigned long long>(diff));
    if (diff || removed_dev != removed_host || !removed_host || !live || !with_transitive) rc = 3;

    for (std::size_t i = 0; i < host.edges.size(); i += 2) {  // weights as a layout would leave them: an edge and its pair alike
      if (!host.edges[i]) continue;
      const double w = 0.5 + static_cast<double>((i * 2654435761u) % 1000) / 400.0;
      for (Graph* g : {&dev, &host}) g->edges[i]->weight = g->edges[i + 1]->weight = w;
    }
    const auto long_dev = raven::MarkLongEdges(engine, dev);
    const auto long_host = HostMarkLongEdges(host);
    std::uint64_t long_diff = long_dev.size() != long_host.size();
    for (auto i : long_host) long_diff += !long_dev.count(i);
    RemoveEdges(dev, long_dev);
    RemoveEdges(host, long_host);
    diff = Differences(dev, host) + long_diff;
    std::printf("long marked %zu %zu differences %llu\n", long_dev.size(), long_host.size(), static_cast<unsigned long long>(diff));
    if (diff || long_host.empty()) rc = 3;

    // out-edges out of ascending edge id: refused, not computed differently
    bool thrown = false;
    for (auto& v : dev.nodes) {
      if (!v || v->outedges.size() < 2) continue;
      std::swap(v->outedges[0], v->outedges[1]);
      try {
        raven::RemoveTransitiveEdges(engine, dev);
      } catch (const std::invalid_argument&) {
        thrown = true;
      }
      std::swap(v->outedges[0], v->outedges[1]);
      break;
    }
    std::printf("order_check_throws %d\n", thrown ? 1 : 0);
    if (!thrown) rc = 3;
  } catch (const std::exception& ex) {
    std::printf("error: %s\n", ex.what());
    rc = 1;
  }
  rvn_engine_destroy(engine);
  return rc;
}
