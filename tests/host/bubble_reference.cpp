// The CPU statement that the device side of RemoveBubbles (rvn_tiling_paths_as_reads, rvn_path_similarity_batch and the
// facade include/raven_hip/bubbles.hpp) is compared with.  It says, in this project's own words and single-threaded, what
// raven::RemoveBubbles (RavenLib/src/assemble.cc:199-355) computes with its helpers — the search from every node with two
// out-edges or more, the checks on the two paths it finds, FindRemovableEdges (:128-197), the similarity test on the path
// strings, and RemoveEdges(marked, true) (common.cc:5-30) — over node and edge objects with std::string sequences.  The
// edit distance is Myers' bit-vector algorithm in 64-row blocks over whole columns (no band, no threshold).
// tests/test_bubble_rules.py pins it by results derived by hand.
//
//   bubble_reference bubbles IN OUT
//     IN  = u32 n_nodes, u64 n_edges, u32 tail[E] (0xFFFFFFFF: graph.edges[i] == nullptr), u32 head[E], u32 length[E],
//           u8 present[n_nodes] (0: graph.nodes[i] == nullptr), u32 count[n_nodes], u64 seq_off[n_nodes + 1],
//           u8 bases[seq_off[n_nodes]] (codes 0 .. 3)
//     OUT = u32 popped, u32 n_junctions (nodes the loop searched from), u8 node_alive[n_nodes], u8 edge_alive[E],
//           u32 n_tests, then per similarity test in the order they were made: u32 n_lhs, u32 lhs[], u32 lhs_label[],
//           u32 n_rhs, u32 rhs[], u32 rhs_label[] (the label of a step as the edge states it, unclamped; 0 for the last
//           node), u64 l, u64 r (the strings' lengths), u32 distance (0xFFFFFFFF: rejected by length, not aligned),
//           u8 similar
//   bubble_reference distance IN OUT
//     IN  = u32 n_pairs, then per pair u64 l, u64 r, u8 a[l], u8 b[r];  OUT = u32 distance[n_pairs]
// Binary little-endian files; the loop's own time goes to stderr (tools/time_bubbles.py).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

using u8 = std::uint8_t;
using u32 = std::uint32_t;
using u64 = std::uint64_t;

// ---- global unit-cost edit distance: Myers' bit-vector recurrence, the pattern cut into blocks of 64 rows ----
struct Block {
  u64 plus = ~0ULL, minus = 0;  // vertical deltas +1 / -1 of the block's rows in the current column
};
// one column step of one block: `carry` is the horizontal delta that enters at its top row, the result the one that leaves
// at its bottom row
int Step(Block& b, u64 match, int carry) {
  const u64 diag = match | b.minus;
  if (carry < 0) match |= 1ULL;
  const u64 run = (((match & b.plus) + b.plus) ^ b.plus) | match;
  u64 hplus = b.minus | ~(run | b.plus);
  u64 hminus = b.plus & run;
  const int out = (hplus >> 63) ? 1 : ((hminus >> 63) ? -1 : 0);
  hplus <<= 1;
  hminus <<= 1;
  if (carry < 0) hminus |= 1ULL;
  else if (carry > 0) hplus |= 1ULL;
  b.plus = hminus | ~(diag | hplus);
  b.minus = hplus & diag;
  return out;
}
u32 Distance(const std::string& a, const std::string& b) {
  const u64 n = a.size(), m = b.size();
  if (n == 0) return static_cast<u32>(m);
  const u64 blocks = (n + 63) / 64;
  std::vector<u64> match(blocks * 4, 0);  // rows of the pattern that hold each of the four codes
  for (u64 i = 0; i < n; ++i) match[(i / 64) * 4 + (a[i] & 3)] |= 1ULL << (i % 64);
  std::vector<Block> col(blocks);
  long long bottom = static_cast<long long>(64 * blocks);  // the score under the last block's last row
  for (u64 j = 0; j < m; ++j) {
    int carry = 1;  // the first row of the matrix grows by one per column
    for (u64 k = 0; k < blocks; ++k) carry = Step(col[k], match[k * 4 + (b[j] & 3)], carry);
    bottom += carry;
  }
  // rows behind the pattern's end match nothing: take their vertical deltas off again
  const u64 used = n - 64 * (blocks - 1);
  const u64 pad = used >= 64 ? 0ULL : ~((1ULL << used) - 1ULL);
  bottom -= __builtin_popcountll(col[blocks - 1].plus & pad);
  bottom += __builtin_popcountll(col[blocks - 1].minus & pad);
  return static_cast<u32>(bottom);
}

// ---- the graph ----
struct Link;
struct Vertex {
  u32 id = 0;
  std::string bases;
  u32 count = 1;
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
  // the first `span` bases of the tail; a span beyond the tail's end gives the whole tail (InflateData clamps)
  std::string Label() const { return from->bases.substr(0, std::min<u64>(span, from->bases.size())); }
};
struct Graph {
  std::vector<std::unique_ptr<Vertex>> nodes;  // null: removed
  std::vector<std::unique_ptr<Link>> edges;    // null: an empty slot
};
using Path = std::vector<Vertex*>;
using Marks = std::unordered_set<u32>;

struct Test {
  std::vector<u32> lhs, rhs, lhs_label, rhs_label;
  u64 l = 0, r = 0;
  u32 distance = 0xFFFFFFFFu;
  u8 similar = 0;
};

// the first out-edge of `from`, in list order, that leads to `to`
Link* StepEdge(Vertex* from, Vertex* to) {
  for (Link* e : from->outedges)
    if (e->to == to) return e;
  return nullptr;
}
void MarkSteps(const Path& p, std::size_t first, std::size_t last, Marks* m) {  // the steps p[i] -> p[i + 1], first <= i < last
  for (std::size_t i = first; i < last; ++i) {
    Link* e = StepEdge(p[i], p[i + 1]);
    m->insert(e->id);
    m->insert(e->twin->id);
  }
}

// Which steps of a path may go: the whole of it when no inner node has a second in-edge or a second out-edge; otherwise
// the stretch that hangs on the rest of the graph at one end only — in front of the first inner node with several
// in-edges, behind the last inner node with several out-edges, or between the two when the out-branch comes first.
// Nothing when one of those two nodes branches both ways.
Marks Removable(const Path& p) {
  Marks m;
  if (p.empty()) return m;
  long long join = -1, fork = -1;
  for (std::size_t i = 1; i + 1 < p.size(); ++i)
    if (p[i]->inedges.size() > 1) {
      join = static_cast<long long>(i);
      break;
    }
  for (std::size_t i = 1; i + 1 < p.size(); ++i)
    if (p[i]->outedges.size() > 1) fork = static_cast<long long>(i);
  if (join == -1 && fork == -1) {
    MarkSteps(p, 0, p.size() - 1, &m);
    return m;
  }
  if (join != -1 && p[join]->outedges.size() > 1) return m;
  if (fork != -1 && p[fork]->inedges.size() > 1) return m;
  if (join == -1) MarkSteps(p, static_cast<std::size_t>(fork), p.size() - 1, &m);
  else if (fork == -1) MarkSteps(p, 0, static_cast<std::size_t>(join), &m);
  else if (fork < join) MarkSteps(p, static_cast<std::size_t>(fork), static_cast<std::size_t>(join), &m);
  return m;
}

bool Plain(const Path& p) {  // no inner node branches
  if (p.empty()) return false;
  for (std::size_t i = 1; i + 1 < p.size(); ++i)
    if (p[i]->Branches()) return false;
  return true;
}

std::string Spell(const Path& p, std::vector<u32>* ids, std::vector<u32>* labels) {
  std::string s;
  for (std::size_t i = 0; i + 1 < p.size(); ++i) {
    Link* e = StepEdge(p[i], p[i + 1]);
    ids->push_back(p[i]->id);
    labels->push_back(e ? e->span : 0);
    if (e) s += e->Label();
  }
  ids->push_back(p.back()->id);
  labels->push_back(0);
  s += p.back()->bases;
  return s;
}

Marks Pop(const Path& lhs, const Path& rhs, std::vector<Test>* tests) {
  if (lhs.empty() || rhs.empty()) return Marks();
  // the two paths share their two ends and nothing else, and hold no node together with its twin
  std::unordered_set<Vertex*> both(lhs.begin(), lhs.end());
  both.insert(rhs.begin(), rhs.end());
  if (lhs.size() + rhs.size() - 2 != both.size()) return Marks();
  for (Vertex* v : lhs)
    if (both.count(v->twin)) return Marks();
  if (!Plain(lhs) || !Plain(rhs)) {
    if (Removable(lhs).empty() && Removable(rhs).empty()) return Marks();
    Test t;
    const std::string l = Spell(lhs, &t.lhs, &t.lhs_label), r = Spell(rhs, &t.rhs, &t.rhs_label);
    t.l = l.size();
    t.r = r.size();
    const bool by_length = std::min(l.size(), r.size()) < std::max(l.size(), r.size()) * 0.8;
    if (!by_length) {
      t.distance = Distance(l, r);
      const double score = 1 - t.distance / static_cast<double>(std::max(l.size(), r.size()));
      t.similar = score < 0.8 ? 0 : 1;
    }
    tests->push_back(t);
    if (!t.similar) return Marks();
  }
  u32 lhs_count = 0, rhs_count = 0;
  for (Vertex* v : lhs) lhs_count += v->count;
  for (Vertex* v : rhs) rhs_count += v->count;
  Marks m = Removable(lhs_count > rhs_count ? rhs : lhs);
  if (m.empty()) m = Removable(lhs_count > rhs_count ? lhs : rhs);
  return m;
}

// RemoveEdges(graph, marked, true): the marked edges leave their nodes' lists (the others keep their order); a node they
// touched that is left without any edge goes too
void RemoveMarked(Graph& graph, const Marks& marked) {
  auto drop = [](std::vector<Link*>& list, Link* e) { list.erase(std::remove(list.begin(), list.end(), e), list.end()); };
  std::unordered_set<u32> touched;
  for (u32 i : marked) {
    Link* e = graph.edges[i].get();
    touched.insert(e->from->id);
    touched.insert(e->to->id);
    drop(e->from->outedges, e);
    drop(e->to->inedges, e);
  }
  for (u32 v : touched)
    if (graph.nodes[v]->outedges.empty() && graph.nodes[v]->inedges.empty()) graph.nodes[v].reset();
  for (u32 i : marked) graph.edges[i].reset();
}

constexpr u32 kReach = 500000;

u32 PopBubbles(Graph& graph, std::vector<Test>* tests, u32* n_junctions) {
  std::vector<u32> far(graph.nodes.size(), 0);
  std::vector<Vertex*> from(graph.nodes.size(), nullptr);
  auto walk_back = [&](Vertex* begin, Vertex* end) {
    Path p;
    for (; end != begin; end = from[end->id]) p.push_back(end);
    p.push_back(begin);
    std::reverse(p.begin(), p.end());
    return p;
  };
  u32 popped = 0;
  for (const auto& slot : graph.nodes) {
    Vertex* begin = slot.get();
    if (!begin || begin->outedges.size() < 2) continue;
    ++*n_junctions;
    // breadth first from `begin`, up to kReach bases away (uint32 sums), until an edge leads to a node reached before
    Vertex* meet = nullptr;
    Vertex* via = nullptr;
    std::deque<Vertex*> todo{begin};
    std::vector<Vertex*> seen{begin};
    while (!todo.empty() && !meet) {
      Vertex* at = todo.front();
      todo.pop_front();
      for (Link* e : at->outedges) {
        if (e->to == begin) continue;
        if (static_cast<u32>(far[at->id] + e->span) > kReach) continue;
        far[e->to->id] = far[at->id] + e->span;
        seen.push_back(e->to);
        todo.push_back(e->to);
        if (from[e->to->id]) {
          meet = e->to;
          via = at;
          break;
        }
        from[e->to->id] = at;
      }
    }
    Marks marked;
    if (meet) {
      const Path lhs = walk_back(begin, meet);
      Path rhs = walk_back(begin, via);
      rhs.push_back(meet);
      marked = Pop(lhs, rhs, tests);
    }
    for (Vertex* v : seen) {
      far[v->id] = 0;
      from[v->id] = nullptr;
    }
    RemoveMarked(graph, marked);
    popped += marked.empty() ? 0 : 1;
  }
  return popped;
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

int Bubbles(std::ifstream& in, std::ofstream& out) {
  u32 n = 0;
  u64 E = 0;
  Get(in, &n, 1);
  Get(in, &E, 1);
  const auto tail = GetVec<u32>(in, E), head = GetVec<u32>(in, E), length = GetVec<u32>(in, E);
  const auto present = GetVec<u8>(in, n);
  const auto count = GetVec<u32>(in, n);
  const auto seq_off = GetVec<u64>(in, static_cast<std::size_t>(n) + 1);
  const auto bases = GetVec<u8>(in, seq_off[n]);
  Graph graph;
  graph.nodes.resize(n);
  for (u32 i = 0; i < n; ++i) {
    if (!present[i]) continue;
    graph.nodes[i].reset(new Vertex());
    Vertex& v = *graph.nodes[i];
    v.id = i;
    v.bases.assign(reinterpret_cast<const char*>(bases.data()) + seq_off[i], seq_off[i + 1] - seq_off[i]);
    v.count = count[i];
  }
  for (u32 i = 0; i < n; ++i)
    if (graph.nodes[i] && (i ^ 1u) < n) graph.nodes[i]->twin = graph.nodes[i ^ 1u].get();
  graph.edges.resize(E);
  for (u64 i = 0; i < E; ++i)
    if (tail[i] != 0xFFFFFFFFu) graph.edges[i].reset(new Link(static_cast<u32>(i), graph.nodes[tail[i]].get(), graph.nodes[head[i]].get(), length[i]));
  for (u64 i = 0; i < E; ++i)
    if (graph.edges[i]) graph.edges[i]->twin = graph.edges[i ^ 1].get();

  std::vector<Test> tests;
  u32 n_junctions = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const u32 popped = PopBubbles(graph, &tests, &n_junctions);
  std::fprintf(stderr, "bubbles %.6f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  std::vector<u8> node_alive, edge_alive;
  for (const auto& v : graph.nodes) node_alive.push_back(v ? 1 : 0);
  for (const auto& e : graph.edges) edge_alive.push_back(e ? 1 : 0);
  Put1<u32>(out, popped);
  Put1<u32>(out, n_junctions);
  Put(out, node_alive), Put(out, edge_alive);
  Put1<u32>(out, static_cast<u32>(tests.size()));
  for (const Test& t : tests) {
    Put1<u32>(out, static_cast<u32>(t.lhs.size())), Put(out, t.lhs), Put(out, t.lhs_label);
    Put1<u32>(out, static_cast<u32>(t.rhs.size())), Put(out, t.rhs), Put(out, t.rhs_label);
    Put1<u64>(out, t.l), Put1<u64>(out, t.r), Put1<u32>(out, t.distance), Put1<u8>(out, t.similar);
  }
  return 0;
}

int Distances(std::ifstream& in, std::ofstream& out) {
  u32 n = 0;
  Get(in, &n, 1);
  std::vector<u32> d;
  for (u32 i = 0; i < n; ++i) {
    u64 l = 0, r = 0;
    Get(in, &l, 1);
    Get(in, &r, 1);
    const auto a = GetVec<u8>(in, l), b = GetVec<u8>(in, r);
    d.push_back(Distance(std::string(a.begin(), a.end()), std::string(b.begin(), b.end())));
  }
  Put(out, d);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::ifstream in(argv[2], std::ios::binary);
  std::ofstream out(argv[3], std::ios::binary);
  int rc = 2;
  if (mode == "bubbles") rc = Bubbles(in, out);
  else if (mode == "distance") rc = Distances(in, out);
  if (rc) return rc;
  return out ? 0 : 1;
}
