// TEST INFRASTRUCTURE: the force-directed layout of raven's RemoveLongEdges restated from its behaviour — a recursive
// quadtree filled by insertion, recursive centres of mass and forces, the iteration — as the yardstick of
// rvn_layout_force_directed (tests/host/layout_reference.cpp, tests/cpp/layout_facade_test.cpp).  It shares no code with
// raven_amd/csrc/layout.h.  Compile without floating-point contraction.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <vector>

namespace layout_restated {

struct Vec {
  double x = 0, y = 0;
};

class Quad {
 public:
  Quad(Vec middle, double half) : middle_(middle), half_(half) {}

  // false: the point lies outside the closed square middle +- half
  bool Insert(const Vec& p) {
    if (p.x < middle_.x - half_ || p.x > middle_.x + half_ || p.y < middle_.y - half_ || p.y > middle_.y + half_) return false;
    count_ += 1;
    if (count_ == 1) {
      weight_centre_ = p;
      return true;
    }
    if (quadrants_.empty()) {
      if (weight_centre_.x == p.x && weight_centre_.y == p.y) return true;  // a duplicate only adds to the count
      const double q = half_ / 2;
      const double sx[4] = {+q, -q, -q, +q}, sy[4] = {+q, +q, -q, -q};
      for (int i = 0; i < 4; ++i) quadrants_.emplace_back(Vec{middle_.x + sx[i], middle_.y + sy[i]}, q);
      HandDown(weight_centre_);
    }
    HandDown(p);
    return true;
  }

  void ComputeCentres() {
    if (quadrants_.empty()) return;
    Vec c;
    for (Quad& q : quadrants_) {
      q.ComputeCentres();
      c.x += q.weight_centre_.x * q.count_;
      c.y += q.weight_centre_.y * q.count_;
    }
    c.x /= count_;
    c.y /= count_;
    weight_centre_ = c;
  }

  Vec Repulsion(const Vec& p, double k) const {
    const Vec d{p.x - weight_centre_.x, p.y - weight_centre_.y};
    const double dist = std::sqrt(d.x * d.x + d.y * d.y);
    if (half_ * 2 / dist < 1) {
      const double f = count_ * (k * k) / (dist * dist);
      return Vec{d.x * f, d.y * f};
    }
    Vec total;
    for (const Quad& q : quadrants_) {
      const Vec r = q.Repulsion(p, k);
      total.x += r.x;
      total.y += r.y;
    }
    return total;
  }

 private:
  void HandDown(const Vec& p) {
    for (Quad& q : quadrants_)
      if (q.Insert(p)) return;
  }

  Vec middle_;
  double half_;
  Vec weight_centre_;
  std::uint32_t count_ = 0;
  std::vector<Quad> quadrants_;
};

// One component: points [first, first + n) of `pos`, neighbours as indices into `pos`.  after(i) is called with the
// number of iterations done (1 .. n_iterations).
inline void LayOut(std::vector<Vec>& pos, std::uint32_t first, std::uint32_t n, const std::uint64_t* adj_off,
                   const std::uint32_t* adj, std::uint32_t n_iterations, const std::function<void(std::uint32_t)>& after = {}) {
  const double k = std::sqrt(1. / static_cast<double>(n));
  double t = 0.1;
  const double dt = t / static_cast<double>(n_iterations + 1);
  std::vector<Vec> move(n);
  for (std::uint32_t it = 0; it < n_iterations; ++it) {
    double x_lo = 0, x_hi = 0, y_lo = 0, y_hi = 0;
    for (std::uint32_t i = first; i < first + n; ++i) {
      x_lo = std::min(x_lo, pos[i].x);
      x_hi = std::max(x_hi, pos[i].x);
      y_lo = std::min(y_lo, pos[i].y);
      y_hi = std::max(y_hi, pos[i].y);
    }
    const double w = (x_hi - x_lo) / 2, h = (y_hi - y_lo) / 2;
    Quad tree(Vec{x_lo + w, y_lo + h}, std::max(w, h) + 0.01);
    for (std::uint32_t i = first; i < first + n; ++i) tree.Insert(pos[i]);
    tree.ComputeCentres();
    for (std::uint32_t i = first; i < first + n; ++i) {
      Vec f = tree.Repulsion(pos[i], k);
      for (std::uint64_t a = adj_off[i]; a < adj_off[i + 1]; ++a) {
        const Vec d{pos[i].x - pos[adj[a]].x, pos[i].y - pos[adj[a]].y};
        double dist = std::sqrt(d.x * d.x + d.y * d.y);
        if (dist < 0.01) dist = 0.01;
        const double g = -1. * dist / k;
        f.x += d.x * g;
        f.y += d.y * g;
      }
      double len = std::sqrt(f.x * f.x + f.y * f.y);
      if (len < 0.01) len = 0.1;
      const double g = t / len;
      move[i - first] = Vec{f.x * g, f.y * g};
    }
    for (std::uint32_t i = first; i < first + n; ++i) {
      pos[i].x += move[i - first].x;
      pos[i].y += move[i - first].y;
    }
    t -= dt;
    if (after) after(it + 1);
  }
}

}  // namespace layout_restated
