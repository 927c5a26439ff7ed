// repeats.hip — raven::ResolveRepeatInducedOverlaps (RavenLib/src/construct.cc:493-559) on the device: the loop that
// removes the overlaps of overlaps.back() that only a repeat explains, until an iteration removes none.  Per iteration:
//   components   ConnectedComponents (overlap_utils.cc:135-178): the overlaps of type > 2 are edges; union-find with
//                atomic hooking (the larger root onto the smaller) and one flattening pass.  A component counts when it
//                holds a valid pile; which BFS reached which pile does not matter, only the membership does.
//   median       the size / 2-th smallest Pile::median() of each component (nth_element): (component, median) keys
//                through the radix sort, the middle of each segment.
//   regions      Pile::FindRepetitiveRegions(median) of every member (repeats.h): one wave per pile with its coverage
//                in LDS (the first sweep of FindSlopes(1.42) on lanes, the slope pairs' plateau scans as ballots), lane 0
//                alone for piles longer than the LDS copy.  Regions go to 32 slots per pile; a pile with more is redone
//                with exactly as many as it counted.
//   update       UpdateRepetitiveRegions of both piles of every overlap: one thread per overlap, an atomic OR of bit 0.
//   check        CheckRepetitiveRegions of either pile: keep flags, then an order-preserving compaction.
// The host reads back the number of survivors per iteration; regions are rebuilt from nothing every iteration (the
// reference clears those of every member, and members only ever leave), is_repetitive accumulates.
#include <algorithm>
#include <cstring>
#include <vector>

#include "abi.h"
#include "overlap_rules.h"
#include "repeats.h"
#include "wave.h"

namespace rvn {

namespace {

constexpr int kRepCells = 4096;  // cells a wave keeps in LDS; longer piles take lane 0's serial path
constexpr u32 kRepSlot = 32;     // regions per pile on the first try

__device__ __forceinline__ u32 uf_load(const u32* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u32 uf_root(const u32* parent, u32 x) {
  for (u32 y = uf_load(parent + x); y != x; y = uf_load(parent + x)) x = y;
  return x;
}

__global__ void uf_init_kernel(u32* __restrict__ parent, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = i;
}
// the edges of ConnectedComponents: GetOverlapType(o, piles) > 2 joins lhs and rhs
__global__ void uf_hook_kernel(const Overlap* __restrict__ ovl, u64 m, const PileRegion* __restrict__ reg, u32* parent) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Overlap o = ovl[i];
  if (overlap_type(o, reg[o.lhs_id], reg[o.rhs_id]) <= 2) return;
  u32 a = o.lhs_id, b = o.rhs_id;
  for (;;) {
    a = uf_root(parent, a);
    b = uf_root(parent, b);
    if (a == b) return;
    const u32 hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
  }
}
__global__ void uf_flatten_kernel(const u32* __restrict__ parent, u32 n, u32* __restrict__ comp) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 x = i;
  while (parent[x] != x) x = parent[x];
  comp[i] = x;
}
__global__ void mark_valid_kernel(const u32* __restrict__ comp, const PileRegion* __restrict__ reg, u32 n, u8* __restrict__ has_valid) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !reg[i].invalid) has_valid[comp[i]] = 1;
}
// member flags, the (component, median) keys of the members (others sort last under root n), components counted
__global__ void member_keys_kernel(const u32* __restrict__ comp, const u8* __restrict__ has_valid, const u16* __restrict__ median,
                                   u32 n, u8* __restrict__ member, u64* __restrict__ keys, u64* __restrict__ vals,
                                   u32* __restrict__ n_comp) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 c = comp[i];
  const bool in = has_valid[c] != 0;
  member[i] = in ? 1 : 0;
  keys[i] = (static_cast<u64>(in ? c : n) << 16) | median[i];
  vals[i] = i;
  if (in && c == i) atomicAdd(n_comp, 1u);
}
__global__ void segments_kernel(const u64* __restrict__ keys, u32 n, u32* __restrict__ seg_b, u32* __restrict__ seg_e) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const u32 c = static_cast<u32>(keys[k] >> 16);
  if (c == n) return;
  if (k == 0 || static_cast<u32>(keys[k - 1] >> 16) != c) seg_b[c] = k;
  if (k + 1 == n || static_cast<u32>(keys[k + 1] >> 16) != c) seg_e[c] = k + 1;
}
// nth_element(size / 2) of the component's medians = the middle key of its sorted segment
__global__ void component_median_kernel(const u64* __restrict__ keys, const u32* __restrict__ comp, const u8* __restrict__ member,
                                        const u32* __restrict__ seg_b, const u32* __restrict__ seg_e, u32 n,
                                        u16* __restrict__ cmed) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !member[i]) return;
  const u32 c = comp[i], b = seg_b[c], e = seg_e[c];
  cmed[i] = static_cast<u16>(keys[b + (e - b) / 2] & 0xFFFFu);
}

struct RepeatJob {
  const u16* cov;
  const u64* cov_off;  // n + 1
  const u8* kmers;
  const u64* kmer_off;  // n + 1
  const u32* begin;     // Pile::begin_ / end_ (cells)
  const u32* end;
  const u16* cmed;  // the component's median
  const u8* member;
  SlopeRegion* slopes;  // pile p at 3 * cov_off[p] + 4 * p: the list (2 * len) and the first sweep's ups (len + 2)
  u16* tmp;             // pile p at cov_off[p]
  u32* out;             // first try: kRepSlot pairs per pile; retry area behind (pair offsets from kRepSlot * n)
  u32* out_retry;
  u32* count;  // regions after MergeRegions
  u64* src;    // pair offset of them
  u32* need;   // regions counted by a pile that did not fit
  u8* isrep;
  u32* ovf;       // [0] piles that did not fit, [1] slope scratch exceeded (internal error)
  u32* ovf_list;  // the piles that did not fit
  u32 n;
};

// One wave per member pile (list == nullptr: item = pile, kRepSlot slots at pile * kRepSlot; else the retry list with
// its slots and capacities).
__global__ __launch_bounds__(64) void repeat_regions_kernel(RepeatJob J, const u32* __restrict__ list,
                                                            const u64* __restrict__ slot, const u32* __restrict__ caps) {
  __shared__ u16 S[kRepCells + 128];  // cell i at [64 + i], zeros around the pile
  __shared__ u32 sh[2];
  const u32 item = blockIdx.x;
  const u32 p = list ? list[item] : item;
  const int lane = static_cast<int>(threadIdx.x);
  if (!J.member[p]) {
    if (lane == 0) J.count[p] = 0;
    return;
  }
  const u64 off = J.cov_off[p];
  const u32 len = static_cast<u32>(J.cov_off[p + 1] - off);
  const u64 koff = J.kmer_off[p];
  const u32 nk = static_cast<u32>(J.kmer_off[p + 1] - koff);
  const u32 b = J.begin[p], e = J.end[p];
  const u16 median = J.cmed[p];
  SlopeRegion* dst = J.slopes + 3 * off + 4 * static_cast<u64>(p);
  u16* tmp = J.tmp + off;
  const u64 so = slot ? slot[item] : static_cast<u64>(p) * kRepSlot;
  const u32 cap = caps ? caps[item] : kRepSlot;
  const u64 first_try = static_cast<u64>(J.n) * kRepSlot;
  u32* out = so < first_try ? J.out + 2 * so : J.out_retry + 2 * (so - first_try);
  u32 raw = 0, c = 0;
  bool sovf = false;
  if (len > static_cast<u32>(kRepCells)) {
    if (lane == 0) c = find_repetitive_regions(J.cov + off, len, J.kmers + koff, nk, b, e, median, dst, tmp, out, cap, &raw, &sovf);
  } else {
    for (u32 i = lane; i < len + 128; i += 64) {
      const int cell = static_cast<int>(i) - 64;
      S[i] = (cell >= 0 && cell < static_cast<int>(len)) ? J.cov[off + cell] : static_cast<u16>(0);
    }
    u32 n = 0;
    if (lane == 0) repeat_kmer_groups(J.kmers + koff, nk, out, cap, n);
    __syncthreads();
    const u16* D = S + 64;
    // first sweep of FindSlopes(1.42) (slopes.h find_slopes): the highest coverage within 52 cells on the left (right)
    // above coverage * q; zeros outside the pile stand for the missing cells
    const int w = 847 >> 4;
    auto flags_of = [&](int i, bool& down, bool& up) {
      const u16 d = static_cast<u16>(slope_clamp(static_cast<double>(D[i]) * kRepeatQ));
      u16 lmax = 0, rmax = 0;
      for (int x = 1; x <= w; ++x) {
        lmax = D[i - x] > lmax ? D[i - x] : lmax;
        rmax = D[i + x] > rmax ? D[i + x] : rmax;
      }
      down = lmax > d;
      up = rmax > d;
    };
    const u32 cap_s = 2 * len;
    SlopeRegion* ups = dst + cap_s + 2;  // room for len + 2
    u32 nd = 0, nde = 0, nu = 0, nue = 0;
    bool carry_d = false, carry_u = false, overflow = false;
    for (u32 c0 = 0; c0 < len; c0 += 64) {
      const int i = static_cast<int>(c0) + lane;
      bool fd = false, fu = false;
      if (i < static_cast<int>(len)) flags_of(i, fd, fu);
      bool nd_next = false, nu_next = false;
      if (c0 + 64 < len) flags_of(static_cast<int>(c0) + 64, nd_next, nu_next);
      const unsigned long long bd = __ballot(fd), bu = __ballot(fu);
      const unsigned long long sd = bd & ~((bd << 1) | (carry_d ? 1ULL : 0ULL)), su = bu & ~((bu << 1) | (carry_u ? 1ULL : 0ULL));
      const unsigned long long ed = bd & ~((bd >> 1) | (nd_next ? 1ULL << 63 : 0ULL)), eu = bu & ~((bu >> 1) | (nu_next ? 1ULL << 63 : 0ULL));
      const unsigned long long below = (1ULL << lane) - 1ULL;
      if ((sd >> lane) & 1ULL) {
        const u32 k = nd + static_cast<u32>(__popcll(sd & below));
        if (k < cap_s) dst[k].first = static_cast<u32>(i) << 1;
        else overflow = true;
      }
      if ((ed >> lane) & 1ULL) {
        const u32 k = nde + static_cast<u32>(__popcll(ed & below));
        if (k < cap_s) dst[k].second = static_cast<u32>(i);
      }
      if ((su >> lane) & 1ULL) {
        const u32 k = nu + static_cast<u32>(__popcll(su & below));
        if (k < len + 2) ups[k].first = static_cast<u32>(i) << 1 | 1u;
        else overflow = true;
      }
      if ((eu >> lane) & 1ULL) {
        const u32 k = nue + static_cast<u32>(__popcll(eu & below));
        if (k < len + 2) ups[k].second = static_cast<u32>(i);
      }
      nd += static_cast<u32>(__popcll(sd));
      nde += static_cast<u32>(__popcll(ed));
      nu += static_cast<u32>(__popcll(su));
      nue += static_cast<u32>(__popcll(eu));
      carry_d = (bd >> 63) & 1ULL;
      carry_u = (bu >> 63) & 1ULL;
    }
    sovf = __ballot(overflow) != 0 || nd + nu > cap_s;
    __threadfence_block();
    __syncthreads();
    if (!sovf)
      for (u32 k = lane; k < nu; k += 64) dst[nd + k] = ups[k];
    __threadfence_block();
    __syncthreads();
    if (lane == 0) {
      const u32 ns = sovf ? 0 : find_slopes_rest(D, kRepeatQ, dst, cap_s, nd + nu, tmp, &sovf);
      sh[0] = sovf ? 0 : ns;
      sh[1] = n;
    }
    __threadfence_block();
    __syncthreads();
    const u32 ns = sh[0];
    n = sh[1];
    // the slope pairs (pile.cc:289-309): every lane walks the same pairs; the cells between two slopes are counted
    // 64 at a time with ballots
    const u16 min_value = repeat_threshold(median);
    for (u32 i = 0; i + 1 < ns; ++i) {
      const SlopeRegion si = dst[i];
      if (!(si.first & 1u)) continue;
      for (u32 j = i + 1; j < ns; ++j) {
        const SlopeRegion sj = dst[j];
        if (sj.first & 1u) continue;
        if (!repeat_span_short(si, sj, b, e)) continue;
        const u16 peak = repeat_peak(D, si, sj);
        const u32 lo = si.second + 1, hi = sj.first >> 1;
        u32 num_valid = 0;
        bool found = false;
        for (u32 x0 = lo; x0 < hi; x0 += 64) {
          const u32 x = x0 + lane;
          const u16 v = x < hi ? D[x] : static_cast<u16>(0);
          num_valid += static_cast<u32>(__popcll(__ballot(x < hi && v > min_value)));
          found = found || __ballot(x < hi && v > peak) != 0;
        }
        if (repeat_accept(found, num_valid, si, sj)) {
          u32 n0 = n;
          if (lane == 0) repeat_pair_region(si, sj, out, cap, n0);
          ++n;
        }
      }
    }
    raw = n;
    if (lane == 0 && !sovf && raw <= cap) c = repeat_merge_and_clip(out, raw, b, e);
  }
  if (lane == 0) {
    if (sovf) {
      atomicAdd(J.ovf + 1, 1u);
      c = 0;
    } else if (raw > cap) {
      J.need[p] = raw;
      J.ovf_list[atomicAdd(J.ovf, 1u)] = p;
      c = 0;
    }
    J.count[p] = c;
    J.src[p] = so;
    if (raw) J.isrep[p] = 1;
  }
}

__global__ void regions_gather_kernel(const u32* __restrict__ out, const u32* __restrict__ out_retry, const u32* __restrict__ count,
                                      const u64* __restrict__ src, const u32* __restrict__ roff, u32 n, u32* __restrict__ reg) {
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const u32 c = count[p];
  if (c == 0) return;
  const u64 so = src[p], first_try = static_cast<u64>(n) * kRepSlot;
  const u32* s = so < first_try ? out + 2 * so : out_retry + 2 * (so - first_try);
  u32* d = reg + 2ULL * roff[p];
  for (u32 i = 0; i < 2 * c; ++i) d[i] = s[i];
}

// UpdateRepetitiveRegions on both piles (pile.cc:319-342; lhs == rhs: the lhs coordinates both times, one pass suffices)
__global__ void repeat_update_kernel(const Overlap* __restrict__ ovl, u64 m, const u32* __restrict__ roff, u32* reg,
                                     const u32* __restrict__ begin, const u32* __restrict__ end) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Overlap o = ovl[i];
  for (int side = 0; side < 2; ++side) {
    if (side == 1 && o.rhs_id == o.lhs_id) break;
    const u32 p = side ? o.rhs_id : o.lhs_id;
    const u32 ob = side ? o.rhs_begin : o.lhs_begin, oe = side ? o.rhs_end : o.lhs_end;
    for (u32 k = roff[p]; k < roff[p + 1]; ++k)
      if (repeat_update_hits(reg[2 * k], reg[2 * k + 1], ob, oe, begin[p], end[p])) atomicOr(reg + 2 * k, 1u);
  }
}
// CheckRepetitiveRegions of lhs, then of rhs (pile.cc:344-369): keep[i] = 0 when either fires
__global__ void repeat_check_kernel(const Overlap* __restrict__ ovl, u64 m, const u32* __restrict__ roff, const u32* __restrict__ reg,
                                    const u32* __restrict__ begin, const u32* __restrict__ end, u8* __restrict__ keep) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const Overlap o = ovl[i];
  bool hit = false;
  for (int side = 0; side < 2 && !hit; ++side) {
    const u32 p = side ? o.rhs_id : o.lhs_id;
    const bool lhs = p == o.lhs_id;  // the reference picks the lhs coordinates whenever the pile is o.lhs_id
    const u32 ob = lhs ? o.lhs_begin : o.rhs_begin, oe = lhs ? o.lhs_end : o.rhs_end;
    for (u32 k = roff[p]; k < roff[p + 1] && !hit; ++k) hit = repeat_check_hits(reg[2 * k], reg[2 * k + 1], ob, oe, begin[p], end[p]);
  }
  keep[i] = hit ? 0 : 1;
}

int key_bits_for(u32 n) {
  int b = 0;
  while (b < 32 && (static_cast<u64>(n) >> b) != 0) ++b;
  return 16 + b;
}

}  // namespace

void resolve_repeat_induced_overlaps(Engine& e, const Overlap* h_ovl, u64 m, u32 n, const u16* h_cov, const u64* h_cov_off,
                                     const u8* h_kmers, const u64* h_kmer_off, const u32* h_begin, const u32* h_end,
                                     const u16* h_median, const u8* h_invalid, RepeatResult& res) {
  hipStream_t s = e.stream;
  res = RepeatResult();
  res.iterations = 1;
  res.roff.assign(static_cast<size_t>(n) + 1, 0);
  res.isrep.assign(n, 0);
  if (n == 0) return;
  struct Bufs {
    DevBuf ovl, ovl2, reg, begin, end, cov, cov_off, kmers, kmer_off, median, parent, comp, has_valid, member, keys0, keys1,
        vals0, vals1, seg_b, seg_e, cmed, slopes, tmp, out, out_retry, count, src, need, ovf, ovf_list, isrep, retry, retry_slots, roff,
        regions, keep, slot, sort_tmp, scan_tmp;
  } B;
  const u64 cells = h_cov_off[n], kcells = h_kmer_off[n];
  std::vector<u32> h_bc(n), h_ec(n);
  for (u32 i = 0; i < n; ++i) {
    h_bc[i] = h_begin[i] >> 4;  // Pile::begin_ / end_
    h_ec[i] = h_end[i] >> 4;
  }
  Overlap* d_ovl = upload(B.ovl, h_ovl, m, s);
  const PileRegion* d_reg = upload_pile_regions(e, B.reg, h_begin, h_end, h_invalid, n);
  const u32* d_begin = upload(B.begin, h_bc.data(), n, s);
  const u32* d_end = upload(B.end, h_ec.data(), n, s);
  RepeatJob J{};
  J.n = n;
  J.cov = upload(B.cov, h_cov, cells, s);
  J.cov_off = upload(B.cov_off, h_cov_off, static_cast<size_t>(n) + 1, s);
  J.kmers = upload(B.kmers, h_kmers, kcells, s);
  J.kmer_off = upload(B.kmer_off, h_kmer_off, static_cast<size_t>(n) + 1, s);
  const u16* d_median = upload(B.median, h_median, n, s);
  u32* d_parent = B.parent.get<u32>(n);
  u32* d_comp = B.comp.get<u32>(n);
  u8* d_has_valid = B.has_valid.get<u8>(n);
  u8* d_member = B.member.get<u8>(n);
  u64* k0 = B.keys0.get<u64>(n);
  u64* k1 = B.keys1.get<u64>(n);
  u64* v0 = B.vals0.get<u64>(n);
  u64* v1 = B.vals1.get<u64>(n);
  u32* d_seg_b = B.seg_b.get<u32>(n);
  u32* d_seg_e = B.seg_e.get<u32>(n);
  u16* d_cmed = B.cmed.get<u16>(n);
  J.begin = d_begin;
  J.end = d_end;
  J.cmed = d_cmed;
  J.member = d_member;
  J.slopes = B.slopes.get<SlopeRegion>(3 * cells + 4 * static_cast<u64>(n));
  J.tmp = B.tmp.get<u16>(cells + 1);
  J.out = B.out.get<u32>(2 * static_cast<u64>(n) * kRepSlot);
  J.out_retry = B.out_retry.get<u32>(2);
  J.count = B.count.get<u32>(static_cast<size_t>(n) + 1);
  J.src = B.src.get<u64>(n);
  J.need = B.need.get<u32>(n);
  J.isrep = B.isrep.get<u8>(n);
  J.ovf = B.ovf.get<u32>(4);
  J.ovf_list = B.ovf_list.get<u32>(n);
  u32* d_roff = B.roff.get<u32>(static_cast<size_t>(n) + 1);
  RVN_HIP(hipMemsetAsync(J.isrep, 0, n, s));
  std::vector<u32> h_list, h_need(n), h_caps;
  std::vector<u64> h_slots;
  for (;;) {
    // ConnectedComponents
    uf_init_kernel<<<div_up(n, 256), 256, 0, s>>>(d_parent, n);
    if (m) uf_hook_kernel<<<div_up(m, 256), 256, 0, s>>>(d_ovl, m, d_reg, d_parent);
    uf_flatten_kernel<<<div_up(n, 256), 256, 0, s>>>(d_parent, n, d_comp);
    RVN_HIP(hipMemsetAsync(d_has_valid, 0, n, s));
    RVN_HIP(hipMemsetAsync(J.ovf, 0, 16, s));
    mark_valid_kernel<<<div_up(n, 256), 256, 0, s>>>(d_comp, d_reg, n, d_has_valid);
    member_keys_kernel<<<div_up(n, 256), 256, 0, s>>>(d_comp, d_has_valid, d_median, n, d_member, k0, v0, J.ovf + 2);
    RVN_LAUNCH_CHECK();
    // the median of each component
    const int which = radix_sort_pairs_u64_u64(k0, k1, v0, v1, n, key_bits_for(n), B.sort_tmp, B.scan_tmp, s);
    const u64* keys = which ? k1 : k0;
    segments_kernel<<<div_up(n, 256), 256, 0, s>>>(keys, n, d_seg_b, d_seg_e);
    component_median_kernel<<<div_up(n, 256), 256, 0, s>>>(keys, d_comp, d_member, d_seg_b, d_seg_e, n, d_cmed);
    RVN_LAUNCH_CHECK();
    // FindRepetitiveRegions of every member
    repeat_regions_kernel<<<n, 64, 0, s>>>(J, nullptr, nullptr, nullptr);
    RVN_LAUNCH_CHECK();
    RVN_HIP(hipMemcpyAsync(e.h_pin, J.ovf, 16, hipMemcpyDeviceToHost, s));
    RVN_HIP(rvn_stream_sync(s));
    u32 ovf[4];
    std::memcpy(ovf, e.h_pin, 16);
    if (res.iterations == 1) res.components = ovf[2];
    if (ovf[0]) {  // piles with more than kRepSlot regions: again, with exactly the room they counted
      const u32 nr = ovf[0];
      h_list.resize(nr);
      RVN_HIP(hipMemcpy(h_list.data(), J.ovf_list, nr * 4ULL, hipMemcpyDeviceToHost));
      RVN_HIP(hipMemcpy(h_need.data(), J.need, n * 4ULL, hipMemcpyDeviceToHost));
      h_slots.resize(nr);
      h_caps.resize(nr);
      u64 at = static_cast<u64>(n) * kRepSlot;
      for (u32 k = 0; k < nr; ++k) {
        h_slots[k] = at;
        h_caps[k] = h_need[h_list[k]];
        at += h_caps[k];
      }
      J.out_retry = B.out_retry.get<u32>(2 * (at - static_cast<u64>(n) * kRepSlot) + 2);
      u32* d_list = B.retry.get<u32>(2ULL * nr);  // list | caps
      u32* d_caps = d_list + nr;
      u64* d_slots = B.retry_slots.get<u64>(nr);
      RVN_HIP(hipMemcpyAsync(d_list, h_list.data(), nr * 4ULL, hipMemcpyHostToDevice, s));
      RVN_HIP(hipMemcpyAsync(d_caps, h_caps.data(), nr * 4ULL, hipMemcpyHostToDevice, s));
      RVN_HIP(hipMemcpyAsync(d_slots, h_slots.data(), nr * 8ULL, hipMemcpyHostToDevice, s));
      RVN_HIP(hipMemsetAsync(J.ovf, 0, 8, s));
      repeat_regions_kernel<<<nr, 64, 0, s>>>(J, d_list, d_slots, d_caps);
      RVN_LAUNCH_CHECK();
      RVN_HIP(hipMemcpyAsync(e.h_pin, J.ovf, 8, hipMemcpyDeviceToHost, s));
      RVN_HIP(rvn_stream_sync(s));
      std::memcpy(ovf, e.h_pin, 8);
      if (ovf[0]) throw HipError("[raven_hip] FindRepetitiveRegions: a pile counted more regions on its retry (internal error)");
    }
    if (ovf[1]) throw HipError("[raven_hip] FindRepetitiveRegions: a pile produced more than two slope regions per cell (internal error)");
    exclusive_scan_u32_u32(J.count, d_roff, n, B.scan_tmp, s);
    const u32 total = static_cast<u32>(read_back(e, d_roff + n, 4));
    u32* d_regions = B.regions.get<u32>(2ULL * total + 2);
    regions_gather_kernel<<<div_up(n, 256), 256, 0, s>>>(J.out, J.out_retry, J.count, J.src, d_roff, n, d_regions);
    RVN_LAUNCH_CHECK();
    if (m == 0) {
      res.reg.assign(2ULL * total, 0);
      if (total) RVN_HIP(hipMemcpyAsync(res.reg.data(), d_regions, 8ULL * total, hipMemcpyDeviceToHost, s));
      break;
    }
    // UpdateRepetitiveRegions, CheckRepetitiveRegions, the survivors in order
    repeat_update_kernel<<<div_up(m, 256), 256, 0, s>>>(d_ovl, m, d_roff, d_regions, d_begin, d_end);
    u8* d_keep = B.keep.get<u8>(m + 1);
    repeat_check_kernel<<<div_up(m, 256), 256, 0, s>>>(d_ovl, m, d_roff, d_regions, d_begin, d_end, d_keep);
    RVN_LAUNCH_CHECK();
    const KeptSlots ks = kept_slots(e, d_keep, m, B.slot);
    const u64 kept = ks.kept;
    if (kept == m) {  // nothing removed: the regions of this iteration are the piles' final state
      res.reg.assign(2ULL * total, 0);
      if (total) RVN_HIP(hipMemcpyAsync(res.reg.data(), d_regions, 8ULL * total, hipMemcpyDeviceToHost, s));
      break;
    }
    compact_overlaps(e, d_ovl, d_keep, ks.slot, m, B.ovl2.get<Overlap>(kept + 1));
    B.ovl.swap(B.ovl2);
    d_ovl = B.ovl.as<Overlap>();
    res.removed += m - kept;
    m = kept;
    ++res.iterations;
  }
  res.ovl.resize(m);
  if (m) RVN_HIP(hipMemcpyAsync(res.ovl.data(), d_ovl, m * sizeof(Overlap), hipMemcpyDeviceToHost, s));
  RVN_HIP(hipMemcpyAsync(res.roff.data(), d_roff, (static_cast<size_t>(n) + 1) * 4, hipMemcpyDeviceToHost, s));
  RVN_HIP(hipMemcpyAsync(res.isrep.data(), J.isrep, n, hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));
}

}  // namespace rvn

// ---- C ABI (include/raven_hip.h) -----------------------------------------------------------------------------------
using namespace rvn;

struct rvn_repeats {
  RepeatResult res;
};

int rvn_resolve_repeat_induced_overlaps(rvn_engine* h, const rvn_overlap* overlaps, uint64_t n_overlaps, uint32_t n_piles,
                                        const uint16_t* coverage, const uint64_t* coverage_offsets, const uint8_t* kmers,
                                        const uint64_t* kmers_offsets, const uint32_t* pile_begin, const uint32_t* pile_end,
                                        const uint16_t* median, const uint8_t* invalid, rvn_repeats** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !out || (n_overlaps && !overlaps) || !coverage_offsets || !kmers_offsets ||
        (n_piles && (!pile_begin || !pile_end || !median || !invalid)) ||
        (coverage_offsets[n_piles] && !coverage) || (kmers_offsets[n_piles] && !kmers))
      return fail(RVN_EINVAL, "[raven_hip] rvn_resolve_repeat_induced_overlaps: NULL argument");
    *out = nullptr;
    const char* csr = csr_offsets_error(coverage_offsets, n_piles, kMaxPileCells);
    if (!csr) csr = csr_offsets_error(kmers_offsets, n_piles, kMaxPileCells);
    if (csr) return fail(RVN_EINVAL, std::string("[raven_hip] rvn_resolve_repeat_induced_overlaps: ") + csr);
    for (u64 x = 0; x < n_overlaps; ++x)
      if (overlaps[x].lhs_id >= n_piles || overlaps[x].rhs_id >= n_piles)
        return fail(RVN_EINVAL, "[raven_hip] rvn_resolve_repeat_induced_overlaps: overlap of an unknown pile");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    std::unique_ptr<rvn_repeats> r(new rvn_repeats());
    resolve_repeat_induced_overlaps(e, reinterpret_cast<const Overlap*>(overlaps), n_overlaps, n_piles, coverage,
                                    coverage_offsets, kmers, kmers_offsets, pile_begin, pile_end, median, invalid, r->res);
    *out = r.release();
    return RVN_OK;
  });
}

uint64_t rvn_repeats_num_overlaps(const rvn_repeats* r) { return r ? r->res.ovl.size() : 0; }
uint64_t rvn_repeats_num_regions(const rvn_repeats* r) { return r ? r->res.reg.size() / 2 : 0; }

int rvn_repeats_fetch(const rvn_repeats* r, rvn_overlap* overlaps, uint32_t* regions, uint32_t* region_offsets,
                      uint8_t* is_repetitive, rvn_repeats_stats* stats) {
  if (!r) return fail(RVN_EINVAL, "[raven_hip] NULL repeats result");
  const RepeatResult& x = r->res;
  if (overlaps && !x.ovl.empty()) std::memcpy(overlaps, x.ovl.data(), x.ovl.size() * sizeof(Overlap));
  if (regions && !x.reg.empty()) std::memcpy(regions, x.reg.data(), x.reg.size() * 4);
  if (region_offsets) std::memcpy(region_offsets, x.roff.data(), x.roff.size() * 4);
  if (is_repetitive && !x.isrep.empty()) std::memcpy(is_repetitive, x.isrep.data(), x.isrep.size());
  if (stats) *stats = rvn_repeats_stats{x.iterations, x.components, x.removed};
  return RVN_OK;
}

void rvn_repeats_destroy(rvn_repeats* r) { delete r; }
