// The CPU statement that the device unitigs (raven_amd/csrc/unitigs.hip) and the host build of unitig_rules.h are
// compared with.  It says, in this project's own words and single-threaded, what raven::CreateUnitigs
// (RavenLib/src/common.cc:32-225), the unitig constructor (graph.cc:27-57), the RemoveEdges call behind it and GetUnitigs'
// selection (common.cc:234-240) compute — over node and edge objects with std::string sequences, per-node in- and
// out-lists and insertion-ordered records of what the loop makes.  tests/test_unitig_rules.py pins it by results derived
// by hand.
//
//   unitig_reference unitigs IN OUT
//     IN  = u32 n_nodes, u64 n_edges, u32 tail[E] (0xFFFFFFFF: graph.edges[i] == nullptr), u32 head[E], u32 length[E],
//           u8 present[n_nodes] (0: graph.nodes[i] == nullptr), u32 count[n_nodes], u16 coverage[n_nodes],
//           u8 is_unitig[n_nodes], u64 seq_off[n_nodes + 1], u8 bases[seq_off[n_nodes]] (codes 0 .. 3),
//           u32 epsilon, u32 min_unitig_size
//     OUT = u32 n_new, u64 n_members, u64 n_new_edges, then per new node u32 begin[], u32 end[], u8 is_circular[],
//           u32 count[], u32 length[], u16 coverage[], u8 is_unitig[]; u64 member_off[n_new + 1], u32 members[];
//           u8 marked[E]; u32 new_tail[], u32 new_head[], u32 new_length[]; u64 new_seq_off[n_new + 1], u8 new_bases[];
//           u8 alive[n_nodes + n_new] (after RemoveEdges(marked, true)); u32 n_selected, u32 selected[] (GetUnitigs' nodes)
// Binary little-endian files; the loop's own time goes to stderr (tools/time_unitigs.py); exit 4 for a chain edge that is longer than its tail's sequence.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

using u8 = std::uint8_t;
using u16 = std::uint16_t;
using u32 = std::uint32_t;
using u64 = std::uint64_t;

struct Link;
struct Vertex {
  u32 id = 0;
  std::string bases;
  u32 count = 1;
  u16 coverage = 0;
  bool is_unitig = false, is_circular = false;
  Vertex* twin = nullptr;
  std::vector<Link*> inedges, outedges;  // appended by Link's constructor
  bool Branches() const { return outedges.size() > 1 || inedges.size() > 1; }
};
struct Link {
  Link(u32 id_, Vertex* from_, Vertex* to_, u32 span_) : id(id_), from(from_), to(to_), span(span_) {
    from->outedges.push_back(this);
    to->inedges.push_back(this);
  }
  u32 id;
  Vertex* from;
  Vertex* to;
  Link* twin = nullptr;
  u32 span;  // Edge::length
  std::string Label() const {
    if (span > from->bases.size()) throw static_cast<int>(4);
    return from->bases.substr(0, span);
  }
};
struct Graph {
  std::vector<std::unique_ptr<Vertex>> nodes;  // null: removed
  std::vector<std::unique_ptr<Link>> edges;    // null: an empty slot
};

// A unitig over the walk first -> ... -> last along the only out-edges: the labels of the edges walked, then the whole of
// `last` unless the walk came back to where it started; the members' counts added up the same way.
std::unique_ptr<Vertex> MakeUnitig(u32 id, Vertex* first, Vertex* last, u32 min_unitig_size, std::vector<u32>* walked) {
  std::unique_ptr<Vertex> u(new Vertex());
  u->id = id;
  u->count = 0;
  u->is_circular = first == last;
  Vertex* at = first;
  do {
    u->bases += at->outedges.front()->Label();
    u->count += at->count;
    walked->push_back(at->id);
    at = at->outedges.front()->to;
  } while (at != last);
  if (first != last) {
    u->bases += last->bases;
    u->count += last->count;
    walked->push_back(last->id);
  }
  u->is_unitig = u->count > 5 && u->bases.size() > min_unitig_size;
  return u;
}

struct Made {
  std::vector<std::unique_ptr<Vertex>> nodes;
  std::vector<std::unique_ptr<Link>> edges;
  std::vector<u32> begin, end;
  std::vector<std::vector<u32>> members;
  std::vector<char> marked;
};

void Connect(Made& m, u32& next_edge, Vertex* from, Vertex* to, u32 span, Vertex* from_twin, Vertex* to_twin, u32 twin_span) {
  m.edges.emplace_back(new Link(next_edge++, from, to, span));
  m.edges.emplace_back(new Link(next_edge++, from_twin, to_twin, twin_span));
  Link* a = m.edges[m.edges.size() - 2].get();
  Link* b = m.edges.back().get();
  a->twin = b;
  b->twin = a;
}

Made MakeUnitigs(Graph& graph, u32 epsilon, u32 min_unitig_size) {
  Made m;
  m.marked.assign(graph.edges.size(), 0);
  std::vector<char> seen(graph.nodes.size(), 0);
  u32 next_node = static_cast<u32>(graph.nodes.size());
  u32 next_edge = static_cast<u32>(graph.edges.size());
  auto mark = [&](Link* e) { m.marked[e->id] = m.marked[e->twin->id] = 1; };
  for (const auto& slot : graph.nodes) {
    Vertex* start = slot.get();
    if (!start || seen[start->id] || start->Branches()) continue;
    u32 walked = 1;
    bool circular = false;
    // as far back as the chain goes: up to a node without an in-edge, or to one whose predecessor branches
    Vertex* first = start;
    while (!first->Branches()) {
      seen[first->id] = seen[first->twin->id] = 1;
      if (first->inedges.empty() || first->inedges.front()->from->Branches()) break;
      first = first->inedges.front()->from;
      ++walked;
      if (first == start) {
        circular = true;
        break;
      }
    }
    // and as far forward
    Vertex* last = start;
    while (!last->Branches()) {
      seen[last->id] = seen[last->twin->id] = 1;
      if (last->outedges.empty() || last->outedges.front()->to->Branches()) break;
      last = last->outedges.front()->to;
      ++walked;
      if (last == start) {
        circular = true;
        break;
      }
    }
    if (!circular && first == last) continue;
    if (!circular && walked < 2 * epsilon + 2) continue;
    if (first != last) {  // keep away from the junctions at both ends
      for (u32 i = 0; i < epsilon; ++i) first = first->outedges.front()->to;
      for (u32 i = 0; i < epsilon; ++i) last = last->inedges.front()->from;
    }
    const u16 coverage = static_cast<u16>((first->coverage + last->coverage) / 2);
    std::vector<u32> fwd, rev;
    std::unique_ptr<Vertex> made = MakeUnitig(next_node++, first, last, min_unitig_size, &fwd);
    std::unique_ptr<Vertex> made_rc = MakeUnitig(next_node++, last->twin, first->twin, min_unitig_size, &rev);
    Vertex* unitig = made.get();
    Vertex* unitig_rc = made_rc.get();
    unitig->coverage = unitig_rc->coverage = coverage;
    unitig->twin = unitig_rc;
    unitig_rc->twin = unitig;
    m.nodes.push_back(std::move(made));
    m.nodes.push_back(std::move(made_rc));
    m.begin.push_back(first->id);
    m.end.push_back(last->id);
    m.begin.push_back(last->twin->id);
    m.end.push_back(first->twin->id);
    m.members.push_back(fwd);
    m.members.push_back(rev);
    if (first != last) {  // the unitig takes over the chain's connections
      if (!first->inedges.empty()) {
        Link* in = first->inedges.front();
        mark(in);
        Connect(m, next_edge, in->from, unitig, in->span, unitig_rc, in->twin->to,
                in->twin->span + static_cast<u32>(unitig_rc->bases.size()) - static_cast<u32>(first->twin->bases.size()));
      }
      if (!last->outedges.empty()) {
        Link* out = last->outedges.front();
        mark(out);
        Connect(m, next_edge, unitig, out->to, out->span + static_cast<u32>(unitig->bases.size()) - static_cast<u32>(last->bases.size()),
                out->twin->from, unitig_rc, out->twin->span);
      }
    }
    Vertex* at = first;
    do {
      mark(at->outedges.front());
      at = at->outedges.front()->to;
    } while (at != last);
  }
  return m;
}

// RemoveEdges(graph, marked, true): the marked edges leave their nodes' lists; a node they touched that is left without
// any edge goes too
void RemoveMarked(Graph& graph, const std::vector<char>& marked) {
  auto drop = [](std::vector<Link*>& list, Link* e) {
    std::vector<Link*> kept;
    for (Link* x : list)
      if (x != e) kept.push_back(x);
    list.swap(kept);
  };
  std::unordered_set<u32> touched;
  for (u32 i = 0; i < marked.size(); ++i) {
    if (!marked[i]) continue;
    Link* e = graph.edges[i].get();
    touched.insert(e->from->id);
    touched.insert(e->to->id);
    drop(e->from->outedges, e);
    drop(e->to->inedges, e);
  }
  for (u32 v : touched)
    if (graph.nodes[v]->outedges.empty() && graph.nodes[v]->inedges.empty()) graph.nodes[v].reset();
  for (u32 i = 0; i < marked.size(); ++i)
    if (marked[i]) graph.edges[i].reset();
}

template <typename T>
void Get(std::ifstream& in, T* p, std::size_t n) {
  in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input");
}
template <typename T>
std::vector<T> GetVec(std::ifstream& in, std::size_t n) {
  std::vector<T> v(n);
  if (n) Get(in, v.data(), n);
  return v;
}
template <typename T>
void Put(std::ofstream& out, const std::vector<T>& v) {
  out.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}
template <typename T>
void Put1(std::ofstream& out, T v) {
  out.write(reinterpret_cast<const char*>(&v), sizeof(T));
}

int Unitigs(std::ifstream& in, std::ofstream& out) {
  u32 n = 0;
  u64 E = 0;
  Get(in, &n, 1);
  Get(in, &E, 1);
  const auto tail = GetVec<u32>(in, E), head = GetVec<u32>(in, E), length = GetVec<u32>(in, E);
  const auto present = GetVec<u8>(in, n);
  const auto count = GetVec<u32>(in, n);
  const auto coverage = GetVec<u16>(in, n);
  const auto is_unitig = GetVec<u8>(in, n);
  const auto seq_off = GetVec<u64>(in, static_cast<std::size_t>(n) + 1);
  const auto bases = GetVec<u8>(in, seq_off[n]);
  u32 epsilon = 0, min_unitig_size = 0;
  Get(in, &epsilon, 1);
  Get(in, &min_unitig_size, 1);

  Graph graph;
  graph.nodes.resize(n);
  for (u32 i = 0; i < n; ++i) {
    if (!present[i]) continue;
    graph.nodes[i].reset(new Vertex());
    Vertex& v = *graph.nodes[i];
    v.id = i;
    v.bases.assign(reinterpret_cast<const char*>(bases.data()) + seq_off[i], seq_off[i + 1] - seq_off[i]);
    v.count = count[i];
    v.coverage = coverage[i];
    v.is_unitig = is_unitig[i] != 0;
  }
  for (u32 i = 0; i < n; ++i)
    if (graph.nodes[i] && (i ^ 1u) < n) graph.nodes[i]->twin = graph.nodes[i ^ 1u].get();
  graph.edges.resize(E);
  for (u64 i = 0; i < E; ++i)
    if (tail[i] != 0xFFFFFFFFu) graph.edges[i].reset(new Link(static_cast<u32>(i), graph.nodes[tail[i]].get(), graph.nodes[head[i]].get(), length[i]));
  for (u64 i = 0; i < E; ++i)
    if (graph.edges[i]) graph.edges[i]->twin = graph.edges[i ^ 1].get();

  Made m;
  const auto t0 = std::chrono::steady_clock::now();
  try {
    m = MakeUnitigs(graph, epsilon, min_unitig_size);
  } catch (int code) {
    return code;
  }
  std::fprintf(stderr, "unitigs %.6f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  const u32 n_new = static_cast<u32>(m.nodes.size());
  std::vector<u8> circ, is_u, marked(m.marked.begin(), m.marked.end());
  std::vector<u32> cnt, len, members, nt, nh, nl;
  std::vector<u16> cov;
  std::vector<u64> member_off(1, 0), new_off(1, 0);
  std::vector<u8> new_bases;
  for (u32 j = 0; j < n_new; ++j) {
    const Vertex& v = *m.nodes[j];
    circ.push_back(v.is_circular);
    is_u.push_back(v.is_unitig);
    cnt.push_back(v.count);
    len.push_back(static_cast<u32>(v.bases.size()));
    cov.push_back(v.coverage);
    members.insert(members.end(), m.members[j].begin(), m.members[j].end());
    member_off.push_back(members.size());
    new_bases.insert(new_bases.end(), v.bases.begin(), v.bases.end());
    new_off.push_back(new_bases.size());
  }
  for (const auto& e : m.edges) {
    nt.push_back(e->from->id);
    nh.push_back(e->to->id);
    nl.push_back(e->span);
  }
  Put1<u32>(out, n_new);
  Put1<u64>(out, members.size());
  Put1<u64>(out, m.edges.size());
  Put(out, m.begin), Put(out, m.end), Put(out, circ), Put(out, cnt), Put(out, len), Put(out, cov), Put(out, is_u);
  Put(out, member_off), Put(out, members), Put(out, marked), Put(out, nt), Put(out, nh), Put(out, nl), Put(out, new_off), Put(out, new_bases);

  for (auto& v : m.nodes) graph.nodes.push_back(std::move(v));
  for (auto& e : m.edges) graph.edges.push_back(std::move(e));
  RemoveMarked(graph, m.marked);
  std::vector<u8> alive;
  std::vector<u32> selected;
  for (const auto& v : graph.nodes) {
    alive.push_back(v ? 1 : 0);
    if (v && !(v->id & 1u) && v->is_unitig) selected.push_back(v->id);
  }
  Put(out, alive);
  Put1<u32>(out, static_cast<u32>(selected.size()));
  Put(out, selected);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 || std::string(argv[1]) != "unitigs") return 2;
  std::ifstream in(argv[2], std::ios::binary);
  std::ofstream out(argv[3], std::ios::binary);
  const int rc = Unitigs(in, out);
  if (rc) return rc;
  return out ? 0 : 1;
}
