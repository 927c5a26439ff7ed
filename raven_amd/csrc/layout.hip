// layout.hip — the force-directed layout of raven's RemoveLongEdges (RavenLib/src/assemble.cc:357-627) on the device,
// bit for bit: all components of a call together, a segment of the point array each.  One iteration:
//   bounding box and root cell per component -> 64-bit path key per point (the child layout.h's routing picks, 32 levels)
//   -> points ordered by (component, key) -> cells level by level from the sorted keys (a cell is subdivided when it
//   holds two points or more; only its non-empty quadrants become cells) -> centres of mass bottom-up, children in slot
//   order -> per point: repulsion by a depth-first walk that keeps one partial sum per open level (the association of
//   the reference's recursion), then the attraction terms in the order given, then the step -> points += displacements.
// The reference builds its tree by insertion; the tree does not depend on the insertion order unless two points of a
// component share a full key (duplicates, or closer than the 32nd subdivision) or rounding leaves a point outside all
// four children.  Such a component is flagged for that iteration and its repulsive forces come from the host's
// insertion-built tree (layout.h: host_repulsion); the rest of the iteration stays here.  No atomics on doubles: cell
// indices are handed out with an integer counter (their numbering does not enter any sum).
#include <vector>

#include "common.h"
#include "engine.h"
#include "layout.h"

#pragma clang fp contract(off)

namespace rvn {

using namespace layout;

namespace {

constexpr int kT = 256;
constexpr int kLevelSlots = kKeyLevels + 2;  // cells per depth 0 .. 32, one spare
constexpr u32 kOverflowSlot = kLevelSlots;   // meta[]: level counts, then the overflow mark, then one flag per component
constexpr u32 kFlagSlot = kLevelSlots + 1;

struct Cells {
  double* cx;
  double* cy;
  double* width;
  u32* mass;
  u32* start;  // first point of the cell in key order (it holds [start, start + mass))
  i32* child;
  u32 cap;
  __host__ __device__ TreeView view() const { return TreeView{cx, cy, width, mass, child}; }
};

__global__ __launch_bounds__(kT) void layout_bbox_kernel(const Point* __restrict__ xy, const u32* __restrict__ off,
                                                         Cell* __restrict__ root) {
  __shared__ Box sb[kT];
  const u32 c = blockIdx.x;
  Box b = box_empty();
  for (u32 i = off[c] + threadIdx.x; i < off[c + 1]; i += kT) b = box_add(b, xy[i]);
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) sb[threadIdx.x] = box_join(sb[threadIdx.x], sb[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) root[c] = box_root(sb[0]);
}

__global__ __launch_bounds__(kT) void layout_key_kernel(const Point* __restrict__ xy, const u32* __restrict__ comp,
                                                        const Cell* __restrict__ root, u32 n, u64* __restrict__ key_of,
                                                        u64* __restrict__ key0, u64* __restrict__ val0, u32* __restrict__ meta) {
  const u32 i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const u32 c = comp[i];
  bool gap;
  const u64 key = path_key(root[c], xy[i], &gap);
  key_of[i] = key;
  key0[i] = key;
  val0[i] = i;
  if (gap) atomicOr(&meta[kFlagSlot + c], 1u);
}

__global__ __launch_bounds__(kT) void layout_comp_key_kernel(const u64* __restrict__ val, const u32* __restrict__ comp, u32 n,
                                                             u32* __restrict__ ckey) {
  const u32 j = blockIdx.x * kT + threadIdx.x;
  if (j < n) ckey[j] = comp[val[j]];
}

// the order of the points and their keys in it; two neighbours of a component with one key flag it
__global__ __launch_bounds__(kT) void layout_order_kernel(const u64* __restrict__ val, const u64* __restrict__ key_of,
                                                          const u32* __restrict__ comp, const u32* __restrict__ off, u32 n,
                                                          u32* __restrict__ order, u64* __restrict__ skey, u32* __restrict__ meta) {
  const u32 j = blockIdx.x * kT + threadIdx.x;
  if (j >= n) return;
  const u32 i = static_cast<u32>(val[j]);
  const u64 key = key_of[i];
  order[j] = i;
  skey[j] = key;
  const u32 c = comp[i];
  if (j > off[c] && key_of[static_cast<u32>(val[j - 1])] == key) atomicOr(&meta[kFlagSlot + c], 1u);
}

__device__ inline void cell_init(const Cells& cl, u32 cell, u32 start, u32 mass, double width, const Point* xy, const u32* order) {
  cl.start[cell] = start;
  cl.mass[cell] = mass;
  cl.width[cell] = width;
  const Point p = xy[order[start]];  // a leaf's centre is its point; a subdivided cell's is set by the centre pass
  cl.cx[cell] = p.x;
  cl.cy[cell] = p.y;
  for (int s = 0; s < 4; ++s) cl.child[4 * static_cast<u64>(cell) + s] = -1;
}

__global__ __launch_bounds__(kT) void layout_roots_kernel(Cells cl, const Cell* __restrict__ root, const u32* __restrict__ off,
                                                          const Point* __restrict__ xy, const u32* __restrict__ order, u32 n_comp,
                                                          u32* __restrict__ meta) {
  const u32 c = blockIdx.x * kT + threadIdx.x;
  if (c >= n_comp) return;
  cell_init(cl, c, off[c], off[c + 1] - off[c], root[c].width, xy, order);
  if (c == 0) meta[0] = n_comp;
}

// one thread per cell of depth `level`: its non-empty quadrants become cells of depth level + 1
__global__ __launch_bounds__(kT) void layout_split_kernel(Cells cl, const u64* __restrict__ skey, const Point* __restrict__ xy,
                                                          const u32* __restrict__ order, u32* __restrict__ meta, int level) {
  const u32 i = blockIdx.x * kT + threadIdx.x;
  const u32 cnt = meta[level];
  if (i >= cnt || meta[kOverflowSlot]) return;
  u32 base = 0;
  for (int l = 0; l < level; ++l) base += meta[l];
  const u32 cell = base + i;
  const u32 s = cl.start[cell], m = cl.mass[cell];
  if (m < 2) return;
  u32 b[5];
  split_bounds(skey, s, s + m, level, b);
  u32 nc = 0;
  for (int q = 0; q < 4; ++q) nc += b[q + 1] > b[q];
  const u64 first = static_cast<u64>(base) + cnt + atomicAdd(&meta[level + 1], nc);
  if (first + nc > cl.cap) {  // more cells than the arrays hold: the whole iteration goes to the host
    atomicOr(&meta[kOverflowSlot], 1u);
    return;
  }
  const double w = cl.width[cell] / 2;
  u32 next = static_cast<u32>(first);
  for (int q = 0; q < 4; ++q) {
    if (b[q + 1] == b[q]) continue;
    cell_init(cl, next, b[q], b[q + 1] - b[q], w, xy, order);
    cl.child[4 * static_cast<u64>(cell) + q] = static_cast<i32>(next);
    ++next;
  }
}

__global__ __launch_bounds__(kT) void layout_centre_kernel(Cells cl, u32 base, u32 cnt) {
  const u32 i = blockIdx.x * kT + threadIdx.x;
  if (i < cnt) centre_cell(cl.view(), static_cast<i32>(base + i));
}

// one lane per point, in key order (neighbouring lanes walk neighbouring paths)
__global__ __launch_bounds__(kT) void layout_force_kernel(Cells cl, const Point* __restrict__ xy, const u32* __restrict__ order,
                                                          const u32* __restrict__ comp, const double* __restrict__ k_of,
                                                          const u32* __restrict__ meta, const Point* __restrict__ host_rep,
                                                          const u64* __restrict__ adj_off, const u32* __restrict__ adj, double t,
                                                          u32 n, Point* __restrict__ disp) {
  const u32 j = blockIdx.x * kT + threadIdx.x;
  if (j >= n) return;
  const u32 i = order[j];
  const u32 c = comp[i];
  const Point p = xy[i];
  const double k = k_of[c];
  Point d = meta[kFlagSlot + c] ? host_rep[i] : tree_force<kDeviceStack>(cl.view(), static_cast<i32>(c), p, k);
  for (u64 a = adj_off[i]; a < adj_off[i + 1]; ++a) d = add(d, attraction(p, xy[adj[a]], k));
  disp[i] = step(d, t);
}

__global__ __launch_bounds__(kT) void layout_update_kernel(Point* __restrict__ xy, const Point* __restrict__ disp, u32 n) {
  const u32 i = blockIdx.x * kT + threadIdx.x;
  if (i < n) xy[i] = add(xy[i], disp[i]);
}

int bits_for(u32 n_values) {
  int b = 1;
  while (b < 32 && (1ULL << b) < n_values) ++b;
  return b;
}

}  // namespace

void layout_force_directed(Engine& e, u32 C, const u32* h_off, const double* h_xy, const u64* h_adj_off, const u32* h_adj,
                           u32 n_iterations, double* h_xy_out, LayoutStats& st) {
  st = LayoutStats();
  const u32 n = h_off[C];
  if (n == 0) return;
  if (n_iterations == 0) {
    std::copy(h_xy, h_xy + 2 * static_cast<size_t>(n), h_xy_out);
    return;
  }
  hipStream_t s = e.stream;
  const u64 n_adj = h_adj_off[n];
  const u32 cap = 6 * n + 1024 + C;
  const u32 n_meta = kFlagSlot + C;

  DevBuf b_xy, b_disp, b_rep, b_comp, b_off, b_k, b_root, b_meta, b_adj_off, b_adj, b_key_of, b_key0, b_key1, b_val0, b_val1,
      b_ck0, b_ck1, b_skey, b_order, b_cx, b_cy, b_w, b_mass, b_start, b_child, sort_tmp, scan_tmp;
  Point* d_xy = b_xy.get<Point>(n);
  Point* d_disp = b_disp.get<Point>(n);
  Point* d_rep = b_rep.get<Point>(n);
  u32* d_comp = b_comp.get<u32>(n);
  u32* d_off = b_off.get<u32>(static_cast<size_t>(C) + 1);
  double* d_k = b_k.get<double>(C);
  Cell* d_root = b_root.get<Cell>(C);
  u32* d_meta = b_meta.get<u32>(n_meta);
  u64* d_adj_off = b_adj_off.get<u64>(static_cast<size_t>(n) + 1);
  u32* d_adj = b_adj.get<u32>(n_adj + 1);
  u64* d_key_of = b_key_of.get<u64>(n);
  u64* d_key[2] = {b_key0.get<u64>(n), b_key1.get<u64>(n)};
  u64* d_val[2] = {b_val0.get<u64>(n), b_val1.get<u64>(n)};
  u32* d_ck[2] = {b_ck0.get<u32>(n), b_ck1.get<u32>(n)};
  u64* d_skey = b_skey.get<u64>(n);
  u32* d_order = b_order.get<u32>(n);
  Cells cl{b_cx.get<double>(cap), b_cy.get<double>(cap), b_w.get<double>(cap), b_mass.get<u32>(cap), b_start.get<u32>(cap),
           b_child.get<i32>(4 * static_cast<size_t>(cap)), cap};

  std::vector<u32> h_comp(n);
  std::vector<double> h_k(C);
  for (u32 c = 0; c < C; ++c) {
    for (u32 i = h_off[c]; i < h_off[c + 1]; ++i) h_comp[i] = c;
    h_k[c] = sqrt(1. / static_cast<double>(h_off[c + 1] - h_off[c]));
  }
  RVN_HIP(hipMemcpyAsync(d_xy, h_xy, static_cast<size_t>(n) * sizeof(Point), hipMemcpyHostToDevice, s));
  RVN_HIP(hipMemcpyAsync(d_comp, h_comp.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, s));
  RVN_HIP(hipMemcpyAsync(d_off, h_off, (static_cast<size_t>(C) + 1) * 4, hipMemcpyHostToDevice, s));
  RVN_HIP(hipMemcpyAsync(d_k, h_k.data(), static_cast<size_t>(C) * 8, hipMemcpyHostToDevice, s));
  RVN_HIP(hipMemcpyAsync(d_adj_off, h_adj_off, (static_cast<size_t>(n) + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_adj) RVN_HIP(hipMemcpyAsync(d_adj, h_adj, n_adj * 4, hipMemcpyHostToDevice, s));
  RVN_HIP(rvn_stream_sync(s));  // (the host arrays above may be pageable and go out of scope)

  const u32 gn = div_up(n, kT), gc = div_up(C, kT);
  const int comp_bits = bits_for(C);
  std::vector<u32> h_meta(n_meta);
  std::vector<Point> h_pos, h_rep;
  double t = 0.1;
  const double dt = t / static_cast<double>(n_iterations + 1);
  for (u32 it = 0; it < n_iterations; ++it) {
    RVN_HIP(hipMemsetAsync(d_meta, 0, static_cast<size_t>(n_meta) * 4, s));
    RVN_KLAUNCH(kKLayoutTree, layout_bbox_kernel<<<C, kT, 0, s>>>(d_xy, d_off, d_root));
    RVN_KLAUNCH(kKLayoutTree, layout_key_kernel<<<gn, kT, 0, s>>>(d_xy, d_comp, d_root, n, d_key_of, d_key[0], d_val[0], d_meta));
    int cur = radix_sort_pairs_u64_u64(d_key[0], d_key[1], d_val[0], d_val[1], n, 64, sort_tmp, scan_tmp, s, kKRsUpsweep,
                                       kKRsDownsweep, false);
    if (C > 1) {  // stable: the key order survives inside each component
      RVN_KLAUNCH(kKLayoutTree, layout_comp_key_kernel<<<gn, kT, 0, s>>>(d_val[cur], d_comp, n, d_ck[0]));
      const int r = radix_sort_pairs_u32_u64(d_ck[0], d_ck[1], d_val[cur], d_val[cur ^ 1], n, comp_bits, sort_tmp, scan_tmp, s,
                                             kKRsUpsweep, kKRsDownsweep, false);
      cur ^= r;
    }
    RVN_KLAUNCH(kKLayoutTree,
                layout_order_kernel<<<gn, kT, 0, s>>>(d_val[cur], d_key_of, d_comp, d_off, n, d_order, d_skey, d_meta));
    RVN_KLAUNCH(kKLayoutTree, layout_roots_kernel<<<gc, kT, 0, s>>>(cl, d_root, d_off, d_xy, d_order, C, d_meta));
    // a level has at most one cell per point
    for (int level = 0; level < kKeyLevels; ++level)
      RVN_KLAUNCH(kKLayoutTree, layout_split_kernel<<<gn, kT, 0, s>>>(cl, d_skey, d_xy, d_order, d_meta, level));
    RVN_HIP(hipMemcpyAsync(h_meta.data(), d_meta, static_cast<size_t>(n_meta) * 4, hipMemcpyDeviceToHost, s));
    RVN_HIP(rvn_stream_sync(s));

    const bool overflow = h_meta[kOverflowSlot] != 0;
    bool any_flag = overflow;
    for (u32 c = 0; c < C; ++c) {
      if (overflow) h_meta[kFlagSlot + c] = 1;
      any_flag = any_flag || h_meta[kFlagSlot + c];
    }
    if (!overflow) {
      int depth = 0;
      while (depth + 1 <= kKeyLevels && h_meta[depth + 1]) ++depth;
      st.max_depth = std::max<u32>(st.max_depth, depth);
      std::vector<u32> base(depth + 2, 0);
      for (int l = 0; l <= depth; ++l) base[l + 1] = base[l] + h_meta[l];
      for (int l = depth - 1; l >= 0; --l)
        RVN_KLAUNCH(kKLayoutTree, layout_centre_kernel<<<div_up(h_meta[l], kT), kT, 0, s>>>(cl, base[l], h_meta[l]));
    }
    if (any_flag) {
      h_pos.resize(n);
      h_rep.resize(n);
      RVN_HIP(hipMemcpyAsync(h_pos.data(), d_xy, static_cast<size_t>(n) * sizeof(Point), hipMemcpyDeviceToHost, s));
      RVN_HIP(rvn_stream_sync(s));
      for (u32 c = 0; c < C; ++c) {
        if (!h_meta[kFlagSlot + c]) continue;
        ++st.host_tree_iterations;
        const u32 b = h_off[c], m = h_off[c + 1] - b;
        host_repulsion(h_pos.data() + b, m, h_k[c], h_rep.data() + b);
        RVN_HIP(hipMemcpyAsync(d_rep + b, h_rep.data() + b, static_cast<size_t>(m) * sizeof(Point), hipMemcpyHostToDevice, s));
      }
      if (overflow)
        RVN_HIP(hipMemcpyAsync(d_meta + kFlagSlot, h_meta.data() + kFlagSlot, static_cast<size_t>(C) * 4, hipMemcpyHostToDevice, s));
      RVN_HIP(rvn_stream_sync(s));
    }
    RVN_KLAUNCH(kKLayoutForce, layout_force_kernel<<<gn, kT, 0, s>>>(cl, d_xy, d_order, d_comp, d_k, d_meta, d_rep, d_adj_off,
                                                                     d_adj, t, n, d_disp));
    RVN_KLAUNCH(kKLayoutForce, layout_update_kernel<<<gn, kT, 0, s>>>(d_xy, d_disp, n));
    t -= dt;
  }
  RVN_HIP(hipMemcpyAsync(h_xy_out, d_xy, static_cast<size_t>(n) * sizeof(Point), hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));
}

}  // namespace rvn
