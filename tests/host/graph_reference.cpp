// The CPU statement that the device assembly graph (raven_amd/csrc/graph.hip) and the host build of graph_rules.h are
// compared with.  It says, in this project's own words and single-threaded, what three pieces of raven compute: the edge
// loop of ConstructAssemblyGraph (RavenLib/src/construct.cc:589-641), the marking of RemoveTransitiveEdges
// (assemble.cc:23-65) and the marking loop of RemoveLongEdges (assemble.cc:708-721) — over node and edge objects with
// per-node out-lists, a per-node table of direct edges and an insertion-ordered record of the marked set, with the
// oracle's GetOverlapType (oracle/raven_oracle.cpp, compiled into this program) deciding which overlaps make edges.
// tests/test_graph_rules.py pins it by marks derived by hand.
//
//   graph_reference construct IN OUT    IN  = u32 n_piles, u64 n_overlaps, overlaps (8 x u32), u32 begin[n], u32 end[n] (bases),
//                                             u16 median[n], u8 invalid[n]
//                                       OUT = u32 n_nodes, u64 n_edges, i32 sequence_to_node[n_piles], u32 node_pile[n_nodes],
//                                             u16 node_coverage[n_nodes], u32 tail[E], u32 head[E], u32 length[E],
//                                             u64 edge_overlap[E / 2], finalized overlaps [E / 2], then MARKS of that graph
//   graph_reference graph IN OUT        IN  = u32 n_nodes, u64 n_edges, u32 tail[E] (0xFFFFFFFF: graph.edges[i] == nullptr),
//                                             u32 head[E], u32 length[E], u8 has_weights, f64 weight[E] if so
//                                       OUT = MARKS, then if has_weights u8 long[E], u64 n_long (marked ids)
//   graph_reference comparable IN OUT   IN  = u64 n, n x (u32 len_j, u32 len_k, u32 len_c);  OUT = u8 verdict[n]: triangle i
//                                             a -> b -> c, a -> c of these lengths, is a -> c marked
//   MARKS = u64 n_marked, u32 ids[n_marked] in the order marked_edges first receives them, u64 n_pairs, u32 pairs[2 x n_pairs]:
//           (tail & ~1, head & ~1) of the odd ids in that order.
// Binary little-endian files; exit 3 for an overlap that finalizes on an invalid pile (the reference would index nodes[-1]).
#include <chrono>
#include <fstream>
#include <iostream>
#include <unordered_set>

#include "raven_oracle.cpp"

namespace {

using orc::Overlap;

// The graph as objects, the way the reference keeps it: every node owns the list of the edges that leave it, in the
// order in which they were made.
struct Link;
struct Vertex {
  std::uint32_t id = 0;
  std::uint16_t coverage = 0;
  Vertex* twin = nullptr;          // the other strand
  std::vector<Link*> outedges;     // appended by Link's constructor
  std::vector<Link*> inedges;
};
struct Link {
  Link(std::uint32_t id_, Vertex* from_, Vertex* to_, std::uint32_t span_) : id(id_), from(from_), to(to_), span(span_) {
    from->outedges.push_back(this);
    to->inedges.push_back(this);
  }
  std::uint32_t id;
  Vertex* from;
  Vertex* to;
  Link* twin = nullptr;
  std::uint32_t span;  // Edge::length
  double weight = 0;
};
struct Graph {
  std::vector<std::unique_ptr<Vertex>> nodes;
  std::vector<std::unique_ptr<Link>> edges;  // null: an empty slot
  void AddStrands(std::uint16_t coverage) {
    const std::uint32_t first = static_cast<std::uint32_t>(nodes.size());
    for (std::uint32_t k = 0; k < 2; ++k) {
      nodes.emplace_back(new Vertex());
      nodes.back()->id = first + k;
      nodes.back()->coverage = coverage;
    }
    nodes[first]->twin = nodes[first + 1].get();
    nodes[first + 1]->twin = nodes[first].get();
  }
  // an edge and the edge of the opposite strands, ids next to each other
  void AddLinkPair(std::uint32_t from, std::uint32_t to, std::uint32_t span, std::uint32_t twin_span) {
    const std::uint32_t id = static_cast<std::uint32_t>(edges.size());
    edges.emplace_back(new Link(id, nodes[from].get(), nodes[to].get(), span));
    edges.emplace_back(new Link(id + 1, nodes[to]->twin, nodes[from]->twin, twin_span));
    edges[id]->twin = edges[id + 1].get();
    edges[id + 1]->twin = edges[id].get();
  }
};

// What OverlapFinalize does to an overlap: its type goes into `score`; an overlap that joins two reads end to end (type 3
// or 4) is re-expressed relative to the two valid regions, the rhs span mirrored when the strands differ.  True when it
// makes an edge.
bool FinalizeOverlap(Overlap& o, const std::vector<orc::PileView>& piles) {
  const std::uint32_t type = orc::GetOverlapType(o, piles);
  o.score = type;
  if (type != 3 && type != 4) return false;
  const orc::PileView& lhs = piles[o.lhs_id];
  const orc::PileView& rhs = piles[o.rhs_id];
  const std::uint32_t lb = o.lhs_begin - lhs.begin, le = o.lhs_end - lhs.begin;
  std::uint32_t rb = o.rhs_begin - rhs.begin, re = o.rhs_end - rhs.begin;
  if (o.strand == 0) {
    const std::uint32_t valid = rhs.end - rhs.begin, old_rb = rb;
    rb = valid - re;
    re = valid - old_rb;
  }
  o.lhs_begin = lb;
  o.lhs_end = le;
  o.rhs_begin = rb;
  o.rhs_end = re;
  return true;
}

struct Marks {
  std::vector<std::uint32_t> order;  // the marked ids, each at its first insertion
  std::vector<std::uint32_t> pairs;
};

// x lies within 12 % of y; the two factors are double operations on the double 0.12
bool InBand(double x, double y) {
  const double tolerance = 0.12;
  const double low = 1 - tolerance, high = 1 + tolerance;
  return x >= y * low && x <= y * high;
}

// The marking of RemoveTransitiveEdges: node by node in id order, `direct[y]` = the last out-edge of the node into y (a
// later out-edge overwrites an earlier one), every walk of two edges held against the direct edge to where it ends.
// The set of marked ids is kept as a membership table plus the sequence of first insertions.
Marks MarkTransitiveEdges(const Graph& graph) {
  constexpr std::int64_t kNone = -1;
  std::vector<std::int64_t> direct(graph.nodes.size(), kNone);
  std::vector<char> is_marked(graph.edges.size(), 0);
  Marks m;
  auto insert = [&](std::uint32_t id) {
    if (is_marked[id]) return;
    is_marked[id] = 1;
    m.order.push_back(id);
  };
  for (std::size_t v = 0; v < graph.nodes.size(); ++v) {
    if (!graph.nodes[v]) continue;
    const std::vector<Link*>& out = graph.nodes[v]->outedges;
    for (std::size_t j = 0; j < out.size(); ++j) direct[out[j]->to->id] = out[j]->id;
    for (std::size_t j = 0; j < out.size(); ++j) {
      const std::vector<Link*>& next = out[j]->to->outedges;
      for (std::size_t k = 0; k < next.size(); ++k) {
        const std::int64_t c = direct[next[k]->to->id];
        if (c == kNone) continue;
        const Link& shortcut = *graph.edges[static_cast<std::size_t>(c)];
        const std::uint32_t walk = out[j]->span + next[k]->span;  // wraps in 32 bits, as the reference's sum does
        const double a = walk, b = shortcut.span;
        if (InBand(a, b) || InBand(b, a)) {
          insert(shortcut.id);
          insert(shortcut.twin->id);
        }
      }
    }
    for (std::size_t j = 0; j < out.size(); ++j) direct[out[j]->to->id] = kNone;
  }
  for (std::uint32_t id : m.order) {
    if (id % 2 == 0) continue;
    m.pairs.push_back(graph.edges[id]->from->id & ~1u);
    m.pairs.push_back(graph.edges[id]->to->id & ~1u);
  }
  return m;
}

// The marking loop of RemoveLongEdges: at a node with at least two out-edges, an out-edge is long when some OTHER
// out-edge of the node weighs less than half of it; a long edge takes its twin with it.
std::vector<std::uint8_t> MarkLongEdges(const Graph& graph, std::uint64_t* n_marked) {
  std::vector<std::uint8_t> flags(graph.edges.size(), 0);
  for (const auto& node : graph.nodes) {
    if (!node) continue;
    const std::vector<Link*>& out = node->outedges;
    if (out.size() < 2) continue;
    for (std::size_t k = 0; k < out.size(); ++k) {
      bool is_long = false;
      for (std::size_t j = 0; j < out.size() && !is_long; ++j) is_long = j != k && out[j]->weight * 2.0 < out[k]->weight;
      if (is_long) flags[out[k]->id] = flags[out[k]->twin->id] = 1;
    }
  }
  *n_marked = 0;
  for (std::uint8_t f : flags) *n_marked += f;
  return flags;
}

template <typename T>
void Get(std::ifstream& in, T* p, std::size_t n) {
  in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input");
}
template <typename T>
void Put(std::ofstream& out, const T* p, std::size_t n) {
  out.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
}
void PutMarks(std::ofstream& out, const Marks& m) {
  const std::uint64_t n = m.order.size(), np = m.pairs.size() / 2;
  Put(out, &n, 1);
  Put(out, m.order.data(), m.order.size());
  Put(out, &np, 1);
  Put(out, m.pairs.data(), m.pairs.size());
}

// graph.edges from flat arrays; the twin of slot i is slot i ^ 1
void AddEdges(Graph& graph, const std::vector<std::uint32_t>& tail, const std::vector<std::uint32_t>& head,
              const std::vector<std::uint32_t>& length) {
  for (std::size_t i = 0; i < tail.size(); ++i) {
    const bool empty = tail[i] == 0xFFFFFFFFu;
    graph.edges.emplace_back(empty ? nullptr
                                   : new Link(static_cast<std::uint32_t>(i), graph.nodes[tail[i]].get(), graph.nodes[head[i]].get(), length[i]));
  }
  for (std::size_t i = 0; i < graph.edges.size(); ++i)
    if (graph.edges[i]) graph.edges[i]->twin = graph.edges[i ^ 1].get();
}

int Construct(std::ifstream& in, std::ofstream& out) {
  std::uint32_t n = 0;
  std::uint64_t m = 0;
  Get(in, &n, 1);
  Get(in, &m, 1);
  std::vector<Overlap> overlaps(m);
  Get(in, overlaps.data(), m);
  std::vector<std::uint32_t> begin(n), end(n);
  std::vector<std::uint16_t> median(n);
  std::vector<std::uint8_t> invalid(n);
  Get(in, begin.data(), n);
  Get(in, end.data(), n);
  Get(in, median.data(), n);
  Get(in, invalid.data(), n);
  std::vector<orc::PileView> piles(n);
  for (std::uint32_t i = 0; i < n; ++i) piles[i] = orc::PileView{begin[i], end[i], invalid[i] != 0};

  const auto t0 = std::chrono::steady_clock::now();
  Graph graph;
  // nodes: two per valid pile, in pile order
  std::vector<std::int32_t> sequence_to_node(n, -1);
  std::vector<std::uint32_t> node_pile;
  for (std::uint32_t i = 0; i < n; ++i) {
    if (piles[i].invalid) continue;
    sequence_to_node[i] = static_cast<std::int32_t>(graph.nodes.size());
    graph.AddStrands(median[i]);
    node_pile.insert(node_pile.end(), 2, i);
  }
  // edges: two per overlap that survives OverlapFinalize, in list order
  std::vector<std::uint64_t> edge_overlap;
  std::vector<Overlap> finalized;
  for (std::uint64_t x = 0; x < m; ++x) {
    Overlap& o = overlaps[x];
    if (!FinalizeOverlap(o, piles)) continue;
    if (sequence_to_node[o.lhs_id] < 0 || sequence_to_node[o.rhs_id] < 0) return 3;
    const std::uint32_t lhs_len = piles[o.lhs_id].end - piles[o.lhs_id].begin, rhs_len = piles[o.rhs_id].end - piles[o.rhs_id].begin;
    // lhs runs into rhs (on the rhs's other strand when the overlap is between opposite strands) ...
    std::uint32_t from = static_cast<std::uint32_t>(sequence_to_node[o.lhs_id]);
    std::uint32_t to = static_cast<std::uint32_t>(sequence_to_node[o.rhs_id]) + (o.strand ? 0u : 1u);
    std::uint32_t span = o.lhs_begin - o.rhs_begin;
    std::uint32_t twin_span = (rhs_len - o.rhs_end) - (lhs_len - o.lhs_end);
    if (o.score == 4) {  // ... or the other way round: the same pair of edges seen from the rhs, both spans negated mod 2^32
      std::swap(from, to);
      span = 0u - span;
      twin_span = 0u - twin_span;
    }
    graph.AddLinkPair(from, to, span, twin_span);
    edge_overlap.push_back(x);
    finalized.push_back(o);
  }
  const auto t1 = std::chrono::steady_clock::now();
  const Marks marks = MarkTransitiveEdges(graph);
  const auto t2 = std::chrono::steady_clock::now();
  std::cerr << "graph_reference: construct " << std::chrono::duration<double>(t1 - t0).count() << " s, transitive "
            << std::chrono::duration<double>(t2 - t1).count() << " s" << std::endl;

  const std::uint32_t n_nodes = static_cast<std::uint32_t>(graph.nodes.size());
  const std::uint64_t n_edges = graph.edges.size();
  std::vector<std::uint16_t> coverage(n_nodes);
  for (std::uint32_t i = 0; i < n_nodes; ++i) coverage[i] = graph.nodes[i]->coverage;
  std::vector<std::uint32_t> tail(n_edges), head(n_edges), length(n_edges);
  for (std::uint64_t i = 0; i < n_edges; ++i) {
    tail[i] = graph.edges[i]->from->id;
    head[i] = graph.edges[i]->to->id;
    length[i] = graph.edges[i]->span;
  }
  Put(out, &n_nodes, 1);
  Put(out, &n_edges, 1);
  Put(out, sequence_to_node.data(), n);
  Put(out, node_pile.data(), n_nodes);
  Put(out, coverage.data(), n_nodes);
  Put(out, tail.data(), n_edges);
  Put(out, head.data(), n_edges);
  Put(out, length.data(), n_edges);
  Put(out, edge_overlap.data(), edge_overlap.size());
  Put(out, finalized.data(), finalized.size());
  PutMarks(out, marks);
  return 0;
}

int FromEdges(std::ifstream& in, std::ofstream& out) {
  std::uint32_t n_nodes = 0;
  std::uint64_t n_edges = 0;
  Get(in, &n_nodes, 1);
  Get(in, &n_edges, 1);
  std::vector<std::uint32_t> tail(n_edges), head(n_edges), length(n_edges);
  Get(in, tail.data(), n_edges);
  Get(in, head.data(), n_edges);
  Get(in, length.data(), n_edges);
  std::uint8_t has_weights = 0;
  Get(in, &has_weights, 1);
  std::vector<double> weight(has_weights ? n_edges : 0);
  Get(in, weight.data(), weight.size());
  Graph graph;
  for (std::uint32_t i = 0; i < n_nodes; i += 2) graph.AddStrands(0);
  AddEdges(graph, tail, head, length);
  const auto t0 = std::chrono::steady_clock::now();
  const Marks marks = MarkTransitiveEdges(graph);
  std::cerr << "graph_reference: transitive " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
            << " s" << std::endl;
  PutMarks(out, marks);
  if (has_weights) {
    for (std::uint64_t i = 0; i < n_edges; ++i)
      if (graph.edges[i]) graph.edges[i]->weight = weight[i];
    std::uint64_t n_long = 0;
    const auto flags = MarkLongEdges(graph, &n_long);
    Put(out, flags.data(), flags.size());
    Put(out, &n_long, 1);
  }
  return 0;
}

int Comparable(std::ifstream& in, std::ofstream& out) {
  std::uint64_t n = 0;
  Get(in, &n, 1);
  std::vector<std::uint32_t> t(3 * n);
  Get(in, t.data(), t.size());
  // triangle i on nodes 6i .. 6i + 5: a = 6i, b = 6i + 2, c = 6i + 4; edges 6i: a -> b, 6i + 2: b -> c, 6i + 4: a -> c.  The
  // pairs run c' -> b' -> a' and c' -> a' with lengths 1, 1 and 1000, which are never comparable.
  std::vector<std::uint32_t> tail, head, length;
  Graph graph;
  for (std::uint64_t i = 0; i < n; ++i) {
    const std::uint32_t a = static_cast<std::uint32_t>(6 * i), b = a + 2, c = a + 4;
    for (int k = 0; k < 3; ++k) graph.AddStrands(0);
    const std::uint32_t e[6][3] = {{a, b, t[3 * i]},     {b + 1, a + 1, 1}, {b, c, t[3 * i + 1]},
                                   {c + 1, b + 1, 1},    {a, c, t[3 * i + 2]}, {c + 1, a + 1, 1000}};
    for (const auto& x : e) {
      tail.push_back(x[0]);
      head.push_back(x[1]);
      length.push_back(x[2]);
    }
  }
  AddEdges(graph, tail, head, length);
  const Marks marks = MarkTransitiveEdges(graph);
  std::vector<std::uint8_t> verdict(n, 0);
  for (auto id : marks.order) {
    if (id % 6 == 4) verdict[id / 6] = 1;
    else if (id % 6 != 5) return 4;  // only a -> c and its pair can be marked
  }
  Put(out, verdict.data(), verdict.size());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::ifstream in(argv[2], std::ios::binary);
  std::ofstream out(argv[3], std::ios::binary);
  int rc = 2;
  if (mode == "construct") rc = Construct(in, out);
  else if (mode == "graph") rc = FromEdges(in, out);
  else if (mode == "comparable") rc = Comparable(in, out);
  if (rc) return rc;
  return out ? 0 : 1;
}
