// layout.h — the arithmetic of raven's force-directed layout (RavenLib/src/assemble.cc:357-627: the Barnes-Hut quadtree
// of :441-506 and the iteration of :547-613) as __host__ __device__ functions: the kernels of layout.hip, the host path
// of its exceptional iterations and the host test program (tests/host/layout_host.cpp) all compute with these.
//
// Everything is IEEE double + - * / and sqrt, each rounded once: the file is compiled with contraction off (no product
// may fuse into a sum), and every sum is written in the association the reference's recursion has.  A cell is
// (nucleus, width): the closed square nucleus +- width.  Its children, in slot order, are the quadrants (+,+), (-,+),
// (-,-), (+,-) with nucleus +- width / 2 and width / 2; a point goes to the FIRST child that contains it.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RVN_LAYOUT_HD __host__ __device__
#else
#define RVN_LAYOUT_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace rvn {
namespace layout {

constexpr int kKeyLevels = 32;  // a path key holds 2 bits per level: cells down to depth 32
constexpr int kDeviceStack = kKeyLevels + 1;
// host trees (insertion-built, exceptional iterations) subdivide until two distinct doubles part: at most ~1080 levels
constexpr int kHostStack = 1200;

struct Point {
  double x, y;
};
RVN_LAYOUT_HD inline Point add(Point a, Point b) { return Point{a.x + b.x, a.y + b.y}; }
RVN_LAYOUT_HD inline Point sub(Point a, Point b) { return Point{a.x - b.x, a.y - b.y}; }
RVN_LAYOUT_HD inline Point scale(Point a, double c) { return Point{a.x * c, a.y * c}; }
RVN_LAYOUT_HD inline double norm(Point a) { return sqrt(a.x * a.x + a.y * a.y); }
RVN_LAYOUT_HD inline bool same(Point a, Point b) { return a.x == b.x && a.y == b.y; }

struct Cell {
  Point nucleus;
  double width;
};
// Quadtree::Add's rejection test (assemble.cc:446-449), negated: the bounds are inclusive
RVN_LAYOUT_HD inline bool cell_contains(const Cell& c, Point p) {
  return !(c.nucleus.x - c.width > p.x || p.x > c.nucleus.x + c.width || c.nucleus.y - c.width > p.y ||
           p.y > c.nucleus.y + c.width);
}
RVN_LAYOUT_HD inline Cell cell_child(const Cell& c, int slot) {  // assemble.cc:457-461
  const double w = c.width / 2;
  const bool right = slot == 0 || slot == 3, up = slot < 2;
  return Cell{Point{right ? c.nucleus.x + w : c.nucleus.x - w, up ? c.nucleus.y + w : c.nucleus.y - w}, w};
}
// the child a point of the cell is handed to, -1 if rounding of nucleus +- width / 2 left it outside all four
RVN_LAYOUT_HD inline int cell_route(const Cell& c, Point p) {
  for (int s = 0; s < 4; ++s)
    if (cell_contains(cell_child(c, s), p)) return s;
  return -1;
}

// The bounding box of a component starts from 0 on every side (assemble.cc:548): it always holds the origin.
struct Box {
  double xmin, xmax, ymin, ymax;
};
RVN_LAYOUT_HD inline Box box_empty() { return Box{0, 0, 0, 0}; }
RVN_LAYOUT_HD inline double min_of(double a, double b) { return b < a ? b : a; }  // std::min / std::max
RVN_LAYOUT_HD inline double max_of(double a, double b) { return a < b ? b : a; }
RVN_LAYOUT_HD inline Box box_add(Box b, Point p) {
  return Box{min_of(b.xmin, p.x), max_of(b.xmax, p.x), min_of(b.ymin, p.y), max_of(b.ymax, p.y)};
}
RVN_LAYOUT_HD inline Box box_join(Box a, Box b) {
  return Box{min_of(a.xmin, b.xmin), max_of(a.xmax, b.xmax), min_of(a.ymin, b.ymin), max_of(a.ymax, b.ymax)};
}
RVN_LAYOUT_HD inline Cell box_root(Box b) {  // assemble.cc:555-557
  const double w = (b.xmax - b.xmin) / 2, h = (b.ymax - b.ymin) / 2;
  return Cell{Point{b.xmin + w, b.ymin + h}, max_of(w, h) + 0.01};
}

// The path of a point from the root: 2 bits per level, the first level in the top bits.  *gap is set when the root or
// some cell on the way has no place for the point (the key is then meaningless).
RVN_LAYOUT_HD inline uint64_t path_key(const Cell& root, Point p, bool* gap) {
  *gap = !cell_contains(root, p);
  Cell c = root;
  uint64_t key = 0;
  for (int level = 0; level < kKeyLevels && !*gap; ++level) {
    const int s = cell_route(c, p);
    if (s < 0) {
      *gap = true;
      break;
    }
    key |= static_cast<uint64_t>(s) << (62 - 2 * level);
    c = cell_child(c, s);
  }
  return key;
}
RVN_LAYOUT_HD inline int key_digit(uint64_t key, int level) { return static_cast<int>((key >> (62 - 2 * level)) & 3); }

// A cell of depth `level` holds the points [s, e) of its component's key order; its child q holds [b[q], b[q + 1]):
// the keys agree above that level, so their digits at it ascend.
RVN_LAYOUT_HD inline void split_bounds(const uint64_t* sorted_keys, uint32_t s, uint32_t e, int level, uint32_t b[5]) {
  b[0] = s;
  b[4] = e;
  for (int q = 1; q < 4; ++q) {
    uint32_t lo = b[q - 1], hi = e;  // first position whose digit is >= q
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (key_digit(sorted_keys[mid], level) < q) lo = mid + 1;
      else hi = mid;
    }
    b[q] = lo;
  }
}

// Quadtree::Force's rule (assemble.cc:488-493): a cell that is far enough acts as one body at its centre of mass
RVN_LAYOUT_HD inline bool cell_is_far(double width, double distance) { return width * 2 / distance < 1; }
RVN_LAYOUT_HD inline Point far_term(Point delta, uint32_t mass, double k, double distance) {
  return scale(delta, mass * (k * k) / (distance * distance));
}
// one neighbour's pull (assemble.cc:570-575)
RVN_LAYOUT_HD inline Point attraction(Point p, Point q, double k) {
  const Point delta = sub(p, q);
  double distance = norm(delta);
  if (distance < 0.01) distance = 0.01;
  return scale(delta, -1. * distance / k);
}
// the move of a point (assemble.cc:594-598); a displacement shorter than 0.01 is divided by 0.1, as there
RVN_LAYOUT_HD inline Point step(Point displacement, double t) {
  double length = norm(displacement);
  if (length < 0.01) length = 0.1;
  return scale(displacement, t / length);
}

// A tree as arrays: cell i has centre (cx, cy), mass, width and four child indices in slot order (-1: no such child;
// a leaf has none).  Cells that hold no point are left out of the device trees: they add an exact zero to every sum.
struct TreeView {
  double* cx;
  double* cy;
  const double* width;
  const uint32_t* mass;
  const int32_t* child;
};

// Quadtree::Centre of ONE cell whose children are done (assemble.cc:476-486): children in slot order, from (0, 0),
// divided by the cell's own mass.  A leaf keeps the point it was given.
RVN_LAYOUT_HD inline void centre_cell(const TreeView& t, int32_t cell) {
  Point c{0, 0};
  bool any = false;
  for (int s = 0; s < 4; ++s) {
    const int32_t ch = t.child[4 * static_cast<int64_t>(cell) + s];
    if (ch < 0) continue;
    any = true;
    c = add(c, scale(Point{t.cx[ch], t.cy[ch]}, t.mass[ch]));
  }
  if (!any) return;
  t.cx[cell] = c.x / t.mass[cell];
  t.cy[cell] = c.y / t.mass[cell];
}

// Quadtree::Force (assemble.cc:488-499) without recursion: one partial sum per open cell on the way down, a closed
// cell's value is added to its parent's sum — the association of the recursion, not one running total.
template <int kStack>
RVN_LAYOUT_HD inline Point tree_force(const TreeView& t, int32_t root, Point p, double k) {
  int32_t open_cell[kStack];
  int open_slot[kStack];
  Point sum[kStack];
  int sp = -1;
  int32_t cell = root;
  for (;;) {
    const Point delta = sub(p, Point{t.cx[cell], t.cy[cell]});
    const double distance = norm(delta);
    Point value{0, 0};
    bool closed = true;
    if (cell_is_far(t.width[cell], distance)) {
      value = far_term(delta, t.mass[cell], k, distance);
    } else if (sp + 1 < kStack) {
      ++sp;
      open_cell[sp] = cell;
      open_slot[sp] = 0;
      sum[sp] = Point{0, 0};
      closed = false;
    }
    for (;;) {
      if (closed) {
        if (sp < 0) return value;
        sum[sp] = add(sum[sp], value);
        closed = false;
      }
      int32_t next = -1;
      while (open_slot[sp] < 4 && next < 0) next = t.child[4 * static_cast<int64_t>(open_cell[sp]) + open_slot[sp]++];
      if (next >= 0) {
        cell = next;
        break;
      }
      value = sum[sp--];
      closed = true;
    }
  }
}

// The reference's tree as it builds it: points inserted one by one in the order given (Quadtree::Add, assemble.cc:445-474),
// all four children of a subdivided cell.  The host path of the exceptional iterations — duplicates, points no child
// accepts, trees deeper than a key — where the result depends on that order.
struct InsertionTree {
  std::vector<Cell> cell;
  std::vector<double> cx, cy, width;
  std::vector<uint32_t> mass;
  std::vector<int32_t> child;

  explicit InsertionTree(const Cell& root) { make(root); }
  int32_t make(const Cell& c) {
    cell.push_back(c);
    cx.push_back(0);
    cy.push_back(0);
    width.push_back(c.width);
    mass.push_back(0);
    child.insert(child.end(), 4, -1);
    return static_cast<int32_t>(cell.size() - 1);
  }
  bool add(int32_t i, Point p) {
    if (!cell_contains(cell[i], p)) return false;
    ++mass[i];
    if (mass[i] == 1) {
      cx[i] = p.x;
      cy[i] = p.y;
      return true;
    }
    if (child[4 * static_cast<size_t>(i)] < 0) {
      const Point first{cx[i], cy[i]};
      if (same(first, p)) return true;
      for (int s = 0; s < 4; ++s) {
        const int32_t c = make(cell_child(cell[i], s));
        child[4 * static_cast<size_t>(i) + s] = c;
      }
      for (int s = 0; s < 4; ++s)
        if (add(child[4 * static_cast<size_t>(i) + s], first)) break;
    }
    for (int s = 0; s < 4; ++s)
      if (add(child[4 * static_cast<size_t>(i) + s], p)) break;
    return true;
  }
  TreeView view() { return TreeView{cx.data(), cy.data(), width.data(), mass.data(), child.data()}; }
  void centre() {
    // children are created after their parent: descending index order finishes every child before its parent
    const TreeView t = view();
    for (int32_t i = static_cast<int32_t>(cell.size()) - 1; i >= 0; --i) centre_cell(t, i);
  }
};

// the repulsive force on each point of one component from the insertion-built tree over them, in the order given
inline void host_repulsion(const Point* p, uint32_t n, double k, Point* out) {
  Box b = box_empty();
  for (uint32_t i = 0; i < n; ++i) b = box_add(b, p[i]);
  InsertionTree tree(box_root(b));
  for (uint32_t i = 0; i < n; ++i) tree.add(0, p[i]);
  tree.centre();
  const TreeView t = tree.view();
  for (uint32_t i = 0; i < n; ++i) out[i] = tree_force<kHostStack>(t, 0, p[i], k);
}

}  // namespace layout
}  // namespace rvn
