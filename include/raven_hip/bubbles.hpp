// raven_hip/bubbles.hpp — raven::RemoveBubbles (RavenLib/src/assemble.cc:199-355) with the similarity test of complex
// bubbles decided on the MI355X (rvn_tiling_paths_as_reads, rvn_path_similarity_batch).  Header-only; see INTEGRATION.md
// 3.1h and DESIGN.md 3.14.
//
// What stays on the host, exactly as there: the search from every node with two out-edges or more, the checks on the two
// paths it finds, FindRemovableEdges, the choice of the side that goes, and RemoveEdges(graph, marked, true) (the caller's,
// found through the graph type's namespace).  What the reference does with std::strings — path_sequence of both paths and
// edlibAlign on them — is a verdict here, looked up under the two paths as (node id, label length) sequences: node
// sequences never change, so that key determines both strings.  Before the loop a read-only pass over the graph as it
// stands runs the same search and the same checks from every junction, collects the keys that would need a verdict and
// asks for all of them in ONE batch; the loop takes its verdicts from that table, and asks on the spot for a key an
// earlier pop has made new (a miss).  The result is the reference's whatever the hit rate.
//
// The facade never reads a node's sequence: the node type needs none.  GraphT needs nodes, edges (vectors of
// std::unique_ptr, entries may be null); per node id, pair, count, inedges, outedges; per edge id, pair, tail, head,
// length.  The tiling holds the sequence of node i under i (raven_hip/unitigs.hpp: MakeTilings, CreateUnitigs).
#ifndef RAVEN_HIP_BUBBLES_HPP_
#define RAVEN_HIP_BUBBLES_HPP_

#include <algorithm>
#include <chrono>
#include <deque>
#include <map>
#include <type_traits>

#include "raven_hip/assembly_graph.hpp"

namespace raven {

struct BubbleStats {
  std::uint64_t n_junctions = 0;  // nodes the loop searched from
  std::uint64_t n_checked = 0;    // similarity tests the loop needed
  std::uint64_t n_predicted = 0;  // distinct keys of the batch in front of the loop
  std::uint64_t n_misses = 0;     // tests whose key was not in that batch: asked for on the spot
  double predict_seconds = 0;     // the read-only pass and its batch
  double loop_seconds = 0;        // the loop, the misses included
  double miss_seconds = 0;        // the calls for the misses alone
};

namespace bubble_detail {

constexpr std::uint32_t kReach = 500000;
constexpr double kMinRatio = 0.8;

// a path as the verdict sees it: per node its id and the bases its step contributes (0 for the last node, which is whole)
using PathKey = std::vector<std::pair<std::uint32_t, std::uint32_t>>;
using BubbleKey = std::pair<PathKey, PathKey>;

template <typename NodeT>
auto StepEdge(NodeT* from, NodeT* to) -> typename std::decay<decltype(from->outedges.front())>::type {  // the first out-edge to `to`
  for (auto e : from->outedges)
    if (e->head == to) return e;
  return nullptr;
}

template <typename NodeT>
bool Branches(const NodeT* v) {
  return v->outedges.size() > 1 || v->inedges.size() > 1;
}

template <typename NodeT>
void MarkSteps(const std::vector<NodeT*>& p, std::size_t first, std::size_t last, std::unordered_set<std::uint32_t>* m) {
  for (std::size_t i = first; i < last; ++i) {
    auto e = StepEdge(p[i], p[i + 1]);
    m->emplace(e->id);
    m->emplace(e->pair->id);
  }
}

// FindRemovableEdges (assemble.cc:128-197): the whole path when no inner node has several in- or out-edges, else the
// stretch in front of the first inner node with several in-edges, behind the last with several out-edges, or between the
// two; nothing when one of the two branches both ways
template <typename NodeT>
std::unordered_set<std::uint32_t> Removable(const std::vector<NodeT*>& p) {
  std::unordered_set<std::uint32_t> m;
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

template <typename NodeT>
bool Plain(const std::vector<NodeT*>& p) {
  if (p.empty()) return false;
  for (std::size_t i = 1; i + 1 < p.size(); ++i)
    if (Branches(p[i])) return false;
  return true;
}

// the search of the loop body (assemble.cc:306-348) from `begin`; its two arrays are left as they were found (all zero)
template <typename NodeT>
struct Search {
  std::vector<std::uint32_t> far;
  std::vector<NodeT*> from;
  explicit Search(std::size_t n) : far(n, 0), from(n, nullptr) {}

  bool Run(NodeT* begin, std::vector<NodeT*>* lhs, std::vector<NodeT*>* rhs) {
    NodeT* meet = nullptr;
    NodeT* via = nullptr;
    std::deque<NodeT*> todo{begin};
    std::vector<NodeT*> seen{begin};
    while (!todo.empty() && !meet) {
      NodeT* at = todo.front();
      todo.pop_front();
      for (auto e : at->outedges) {
        if (e->head == begin) continue;
        if (static_cast<std::uint32_t>(far[at->id] + e->length) > kReach) continue;
        far[e->head->id] = far[at->id] + e->length;
        seen.emplace_back(e->head);
        todo.emplace_back(e->head);
        if (from[e->head->id]) {
          meet = e->head;
          via = at;
          break;
        }
        from[e->head->id] = at;
      }
    }
    lhs->clear();
    rhs->clear();
    if (meet) {
      Walk(begin, meet, lhs);
      Walk(begin, via, rhs);
      rhs->emplace_back(meet);
    }
    for (NodeT* v : seen) {
      far[v->id] = 0;
      from[v->id] = nullptr;
    }
    return meet != nullptr;
  }
  void Walk(NodeT* begin, NodeT* end, std::vector<NodeT*>* p) const {
    for (; end != begin; end = from[end->id]) p->emplace_back(end);
    p->emplace_back(begin);
    std::reverse(p->begin(), p->end());
  }
};

enum class Kind { kNothing, kPlain, kNeedsVerdict };

// the checks of bubble_pop in front of the similarity test (assemble.cc:241-262)
template <typename NodeT>
Kind Classify(const std::vector<NodeT*>& lhs, const std::vector<NodeT*>& rhs) {
  if (lhs.empty() || rhs.empty()) return Kind::kNothing;
  std::unordered_set<const NodeT*> both(lhs.begin(), lhs.end());
  both.insert(rhs.begin(), rhs.end());
  if (lhs.size() + rhs.size() - 2 != both.size()) return Kind::kNothing;
  for (const NodeT* v : lhs)
    if (both.count(v->pair) != 0) return Kind::kNothing;
  if (Plain(lhs) && Plain(rhs)) return Kind::kPlain;
  if (Removable(lhs).empty() && Removable(rhs).empty()) return Kind::kNothing;
  return Kind::kNeedsVerdict;
}

template <typename NodeT>
PathKey KeyOf(const std::vector<NodeT*>& p, const std::vector<std::uint32_t>& node_length) {
  PathKey k;
  for (std::size_t i = 0; i + 1 < p.size(); ++i) {
    auto e = StepEdge(p[i], p[i + 1]);
    k.emplace_back(p[i]->id, std::min(e->length, node_length[p[i]->id]));
  }
  k.emplace_back(p.back()->id, 0u);
  return k;
}

struct Paths {
  rvn_reads* r = nullptr;
  Paths() = default;
  Paths(const Paths&) = delete;
  Paths& operator=(const Paths&) = delete;
  ~Paths() { rvn_reads_destroy(r); }
};

// the verdicts of a batch of keys: two paths per key, one pair per key, one call each
inline std::vector<std::uint8_t> Ask(rvn_engine* engine, const rvn_tiling* tiling, const rvn_reads* reads, const std::vector<const BubbleKey*>& keys) {
  std::vector<std::uint64_t> off(1, 0);
  std::vector<std::uint32_t> node, label;
  std::vector<rvn_path_pair> pairs;
  for (const BubbleKey* k : keys) {
    for (const PathKey* p : {&k->first, &k->second}) {
      for (const auto& step : *p) {
        node.push_back(step.first);
        label.push_back(step.second);
      }
      off.push_back(node.size());
    }
    const std::uint32_t at = static_cast<std::uint32_t>(pairs.size()) * 2;
    pairs.push_back(rvn_path_pair{at, at + 1});
  }
  std::vector<std::uint8_t> similar(keys.size(), 0);
  if (keys.empty()) return similar;
  Paths paths;
  graph_detail::Check(rvn_tiling_paths_as_reads(engine, tiling, reads, static_cast<std::uint32_t>(off.size() - 1), off.data(), node.data(),
                                                label.data(), &paths.r));
  graph_detail::Check(rvn_path_similarity_batch(engine, paths.r, pairs.data(), static_cast<std::uint32_t>(pairs.size()), kMinRatio,
                                                similar.data(), nullptr));
  return similar;
}

}  // namespace bubble_detail

// Returns the number of bubbles popped.  Throws std::invalid_argument for what the two device calls refuse (a tiling that
// does not hold the graph's nodes, a read set other than the tiling's).
template <typename GraphT>
std::uint32_t RemoveBubbles(GraphT& graph, rvn_engine* engine, const rvn_tiling* tiling, const rvn_reads* reads, BubbleStats* stats = nullptr) {
  using namespace bubble_detail;
  using NodeT = typename std::remove_reference<decltype(*graph.nodes[0])>::type;
  using Path = std::vector<NodeT*>;
  BubbleStats st;
  std::uint32_t n_tiled = 0;
  graph_detail::Check(rvn_tiling_info(tiling, &n_tiled, nullptr));
  if (n_tiled < graph.nodes.size()) throw std::invalid_argument("[raven_hip] RemoveBubbles: the tiling has fewer nodes than the graph");
  std::vector<std::uint32_t> node_length(n_tiled);
  graph_detail::Check(rvn_tiling_fetch(tiling, nullptr, nullptr, nullptr, nullptr, nullptr, node_length.data()));

  Search<NodeT> search(graph.nodes.size());
  Path lhs, rhs;
  std::map<BubbleKey, std::uint8_t> verdict;
  using Clock = std::chrono::steady_clock;
  auto since = [](Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); };
  const Clock::time_point t_start = Clock::now();

  // the graph as it stands: every key the loop would need if no pop changed a neighbourhood
  for (const auto& it : graph.nodes) {
    if (it == nullptr || it->outedges.size() < 2) continue;
    if (search.Run(it.get(), &lhs, &rhs) && Classify(lhs, rhs) == Kind::kNeedsVerdict)
      verdict.emplace(BubbleKey(KeyOf(lhs, node_length), KeyOf(rhs, node_length)), std::uint8_t(0));
  }
  {
    std::vector<const BubbleKey*> keys;
    for (const auto& kv : verdict) keys.push_back(&kv.first);
    const std::vector<std::uint8_t> similar = Ask(engine, tiling, reads, keys);
    std::size_t i = 0;
    for (auto& kv : verdict) kv.second = similar[i++];
  }
  st.n_predicted = verdict.size();
  st.predict_seconds = since(t_start);

  const Clock::time_point t_loop = Clock::now();
  std::uint32_t popped = 0;
  for (const auto& it : graph.nodes) {
    if (it == nullptr || it->outedges.size() < 2) continue;
    ++st.n_junctions;
    std::unordered_set<std::uint32_t> marked;
    if (search.Run(it.get(), &lhs, &rhs)) {
      Kind kind = Classify(lhs, rhs);
      if (kind == Kind::kNeedsVerdict) {
        ++st.n_checked;
        BubbleKey key(KeyOf(lhs, node_length), KeyOf(rhs, node_length));
        auto hit = verdict.find(key);
        if (hit == verdict.end()) {
          ++st.n_misses;
          const Clock::time_point t_miss = Clock::now();
          const std::uint8_t similar = Ask(engine, tiling, reads, {&key})[0];
          st.miss_seconds += since(t_miss);
          hit = verdict.emplace(std::move(key), similar).first;
        }
        if (!hit->second) kind = Kind::kNothing;
      }
      if (kind != Kind::kNothing) {
        std::uint32_t lhs_count = 0, rhs_count = 0;
        for (const NodeT* v : lhs) lhs_count += v->count;
        for (const NodeT* v : rhs) rhs_count += v->count;
        marked = Removable(lhs_count > rhs_count ? rhs : lhs);
        if (marked.empty()) marked = Removable(lhs_count > rhs_count ? lhs : rhs);
      }
    }
    RemoveEdges(graph, marked, true);
    popped += marked.empty() ? 0 : 1;
  }
  st.loop_seconds = since(t_loop);
  if (stats) *stats = st;
  return popped;
}

}  // namespace raven

#endif  // RAVEN_HIP_BUBBLES_HPP_
