// segsort.h — segmented sort of 64-bit keys (with a 64-bit payload beside each when PAY): many segments of very different
// sizes, each sorted on its own, stably, by the full key.  The segments are binned by size on the device (sizeclass.h), a
// class is one launch: a workgroup per segment whose LDS is sized for the class, a wave per segment through global memory
// beyond the table.  The chain stage of Map uses it twice (chain.hip: a read's matches by group, an interval's by positions).
// Kernels live in this header's unnamed namespace: include it from ONE translation unit.
#pragma once

#include <cstring>

#include "engine.h"
#include "sizeclass.h"
#include "wave.h"

namespace rvn {

namespace {

// ---- wave-level segmented LSD radix sort ---------------------------------------------------------
// Sorts keys k0[b, b+n) (payload p0 when PAY) stably by the full 64-bit key; result always ends in k0/p0.  For the segments
// that do not fit a workgroup's LDS (HiFi: 10 000 - 100 000 matches of one read).  hist: 2 x 256 counters of the wave.
// Round 6: a pass is ONE sweep over the segment — the counts of the next digit are taken while the current one is
// scattered (and those of byte 0 while the varying bits are found), where rounds 1-5 read the keys a second time per pass —
// and a sweep takes four batches of 64 at a time, all their loads issued before the first rank is computed (a wave's
// passes are chains of dependent global loads: the stage ran at 4 % of the HBM rate, bound by their latency).
template <bool PAY>
__device__ void wave_sort_segment(u64* __restrict__ k0, u64* __restrict__ k1, u64* __restrict__ p0,
                                  u64* __restrict__ p1, u64 b, u64 n, u32* hist) {
  const int lane = lane_id();
  const unsigned long long lt = lanemask_lt();
  u32* h_cur = hist;         // counts / running offsets of the digit being scattered
  u32* h_nxt = hist + 256;   // counts of the next digit
  for (int i = lane; i < 256; i += 64) h_nxt[i] = 0;
  __builtin_amdgcn_wave_barrier();
  u64 o = 0, a = ~0ULL;
  for (u64 i = lane; i < n; i += 64) {
    const u64 key = k0[b + i];
    o |= key;
    a &= key;
    atomicAdd(&h_nxt[key & 0xFF], 1u);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    o |= __shfl_xor(o, off, 64);
    a &= __shfl_xor(a, off, 64);
  }
  const u64 varying = o ^ a;
  int cur = 0;
  bool have_counts = true;  // h_nxt holds the counts of byte 0
  int counted_shift = 0;
  for (int shift = 0; shift < 64; shift += 8) {
    if (((varying >> shift) & 0xFF) == 0) continue;
    const u64* kin = cur ? k1 : k0;
    const u64* pin = cur ? p1 : p0;
    u64* kout = cur ? k0 : k1;
    u64* pout = cur ? p0 : p1;
    __builtin_amdgcn_wave_barrier();
    if (have_counts && counted_shift == shift) {
      u32* t = h_cur;
      h_cur = h_nxt;
      h_nxt = t;
    } else {  // (the first varying byte is not byte 0: one counting sweep)
      for (int i = lane; i < 256; i += 64) h_cur[i] = 0;
      __builtin_amdgcn_wave_barrier();
      for (u64 i = lane; i < n; i += 64) atomicAdd(&h_cur[(kin[b + i] >> shift) & 0xFF], 1u);
    }
    int nshift = shift + 8;
    while (nshift < 64 && ((varying >> nshift) & 0xFF) == 0) nshift += 8;
    have_counts = nshift < 64;
    counted_shift = nshift;
    __builtin_amdgcn_wave_barrier();
    {
      const u32 h0 = h_cur[4 * lane], h1 = h_cur[4 * lane + 1], h2 = h_cur[4 * lane + 2], h3 = h_cur[4 * lane + 3];
      const u32 s = h0 + h1 + h2 + h3;
      const u32 ex = wave_inclusive_sum(s) - s;
      __builtin_amdgcn_wave_barrier();
      h_cur[4 * lane] = ex;
      h_cur[4 * lane + 1] = ex + h0;
      h_cur[4 * lane + 2] = ex + h0 + h1;
      h_cur[4 * lane + 3] = ex + h0 + h1 + h2;
      for (int i = lane; i < 256; i += 64) h_nxt[i] = 0;
    }
    __builtin_amdgcn_wave_barrier();
    for (u64 base = 0; base < n; base += 256) {
      u64 key[4], pay[4];
      bool valid[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const u64 i = base + 64 * x + lane;
        valid[x] = i < n;
        key[x] = 0;
        pay[x] = 0;
        if (valid[x]) {
          key[x] = kin[b + i];
          if (PAY) pay[x] = pin[b + i];
        }
      }
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        if (base + 64 * x >= n) break;  // (uniform)
        const unsigned d = static_cast<unsigned>((key[x] >> shift) & 0xFF);
        const unsigned long long peers = match_digit8(d, valid[x]);
        u32 before = 0;
        if (valid[x]) before = h_cur[d];
        __builtin_amdgcn_wave_barrier();
        const u32 rank = before + __popcll(peers & lt);
        if (valid[x] && (peers & lt) == 0) h_cur[d] = before + __popcll(peers);
        __builtin_amdgcn_wave_barrier();
        if (valid[x]) {
          kout[b + rank] = key[x];
          if (PAY) pout[b + rank] = pay[x];
          if (have_counts) atomicAdd(&h_nxt[(key[x] >> nshift) & 0xFF], 1u);
        }
      }
    }
    __threadfence_block();  // this wave's stores must be visible to its other lanes' loads next pass
    cur ^= 1;
  }
  if (cur) {
    for (u64 i = lane; i < n; i += 64) {
      k0[b + i] = k1[b + i];
      if (PAY) p0[b + i] = p1[b + i];
    }
    __threadfence_block();
  }
}

// ---- block-level segmented sort in LDS ----------------------------------------------------------------
// One workgroup of NT threads per segment of <= cap keys (payloads beside them when PAY): all LSD passes ping-pong between
// two LDS buffers, HBM sees one coalesced read and one coalesced write (the global-memory version moved ~20x the data,
// profiles/r01_g_final_pmc_*).  smem: seg_sort_lds_bytes(cap).
template <int NT, bool PAY>
constexpr size_t seg_sort_lds_bytes(u32 cap) {
  return static_cast<size_t>(cap) * 8 * (PAY ? 4 : 2) + (NT / 64) * 256 * 2 + 32 + (NT / 64) * 16;
}
template <int NT, bool PAY>
__device__ void block_sort_lds(u64* __restrict__ keys, u64* __restrict__ pays, u64 b, u32 n, u32 cap, unsigned char* smem) {
  constexpr int NW = NT / 64;
  static_assert(NT == 64 || NT == 256, "one wave or four");
  u64* s_k = reinterpret_cast<u64*>(smem);                         // [2][cap]
  u64* s_p = s_k + 2 * static_cast<size_t>(cap);                   // [2][cap] when PAY
  u16* wave_cnt = reinterpret_cast<u16*>(s_p + (PAY ? 2 * static_cast<size_t>(cap) : 0));  // [NW][256]
  u32* s4 = reinterpret_cast<u32*>(wave_cnt + NW * 256);           // 8 words
  u64* s_or = reinterpret_cast<u64*>(s4 + 8);                      // [NW]
  u64* s_and = s_or + NW;                                          // [NW]
  const int lane = lane_id();
  const int w = threadIdx.x >> 6;
  u64 o = 0, a = ~0ULL;
  for (u32 i = threadIdx.x; i < n; i += NT) {
    const u64 k = keys[b + i];
    s_k[i] = k;
    if (PAY) s_p[i] = pays[b + i];
    o |= k;
    a &= k;
  }
#pragma unroll
  for (int x = 32; x > 0; x >>= 1) {
    o |= __shfl_xor(o, x, 64);
    a &= __shfl_xor(a, x, 64);
  }
  if (lane == 0) {
    s_or[w] = o;
    s_and[w] = a;
  }
  __syncthreads();
  u64 all_or = 0, all_and = ~0ULL;
#pragma unroll
  for (int x = 0; x < NW; ++x) {
    all_or |= s_or[x];
    all_and &= s_and[x];
  }
  const u64 varying = all_or ^ all_and;
  // wave w owns the contiguous share [q0, q1) of the segment (stable: rank order == index order)
  const u32 per = (n + NW - 1) / NW;
  const u32 q0 = min(n, w * per), q1 = min(n, q0 + per);
  const unsigned long long lt = lanemask_lt();
  u32 cur = 0;
  for (int shift = 0; shift < 64; shift += 8) {
    if (((varying >> shift) & 0xFF) == 0) continue;
    const u64* kin = s_k + static_cast<size_t>(cur) * cap;
    u64* kout = s_k + static_cast<size_t>(cur ^ 1) * cap;
    const u64* pin = s_p + static_cast<size_t>(cur) * cap;
    u64* pout = s_p + static_cast<size_t>(cur ^ 1) * cap;
    for (int i = threadIdx.x; i < NW * 256; i += NT) wave_cnt[i] = 0;
    __syncthreads();
    // pass 1: per-wave digit counts (ranks are recomputed in pass 2 with the same ballot order)
    u16* my_cnt = wave_cnt + w * 256;
    for (u32 base = q0; base < q1; base += 64) {
      const u32 i = base + lane;
      const bool valid = i < q1;
      const unsigned d = valid ? static_cast<unsigned>((kin[i] >> shift) & 0xFF) : 0;
      const unsigned long long peers = match_digit8(d, valid);
      if (valid && (peers & lt) == 0) my_cnt[d] += static_cast<u16>(__popcll(peers));
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (NT == 256) {
      const int t = threadIdx.x;
      u32 c[NW], tot = 0;
#pragma unroll
      for (int x = 0; x < NW; ++x) {
        c[x] = wave_cnt[x * 256 + t];
        tot += c[x];
      }
      u32 total;
      u32 run = block_exclusive_sum_256<u32>(tot, s4, &total);
#pragma unroll
      for (int x = 0; x < NW; ++x) {
        wave_cnt[x * 256 + t] = static_cast<u16>(run);
        run += c[x];
      }
    } else {  // one wave: lane l owns the digits 4 l .. 4 l + 3
      const u32 h0 = wave_cnt[4 * lane], h1 = wave_cnt[4 * lane + 1], h2 = wave_cnt[4 * lane + 2], h3 = wave_cnt[4 * lane + 3];
      const u32 sum = h0 + h1 + h2 + h3;
      const u32 ex = wave_inclusive_sum(sum) - sum;
      __builtin_amdgcn_wave_barrier();
      wave_cnt[4 * lane] = static_cast<u16>(ex);
      wave_cnt[4 * lane + 1] = static_cast<u16>(ex + h0);
      wave_cnt[4 * lane + 2] = static_cast<u16>(ex + h0 + h1);
      wave_cnt[4 * lane + 3] = static_cast<u16>(ex + h0 + h1 + h2);
    }
    __syncthreads();
    // pass 2: scatter in index order
    for (u32 base = q0; base < q1; base += 64) {
      const u32 i = base + lane;
      const bool valid = i < q1;
      u64 k = 0, pv = 0;
      if (valid) {
        k = kin[i];
        if (PAY) pv = pin[i];
      }
      const unsigned d = static_cast<unsigned>((k >> shift) & 0xFF);
      const unsigned long long peers = match_digit8(d, valid);
      u32 before = 0;
      if (valid) before = my_cnt[d];
      __builtin_amdgcn_wave_barrier();
      if (valid && (peers & lt) == 0) my_cnt[d] = static_cast<u16>(before + __popcll(peers));
      __builtin_amdgcn_wave_barrier();
      if (valid) {
        const u32 dst = before + __popcll(peers & lt);
        kout[dst] = k;
        if (PAY) pout[dst] = pv;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  const u64* kfin = s_k + static_cast<size_t>(cur) * cap;
  const u64* pfin = s_p + static_cast<size_t>(cur) * cap;
  for (u32 i = threadIdx.x; i < n; i += NT) {
    keys[b + i] = kfin[i];
    if (PAY) pays[b + i] = pfin[i];
  }
}

// ---- the segments by size class, one launch per class -------------------------------------------------------------------
// Segment t is [seg_begin[t], seg_end[t]) of the key array (segments back to back: offsets off and off + 1).
// lists[c * n_seg ...] <- the segments of class c (sizeclass.h: size_class; the order within a list is irrelevant, every
// segment is sorted in place), cnt[c] <- how many
__global__ __launch_bounds__(256) void size_class_list_kernel(const u64* __restrict__ seg_begin, const u64* __restrict__ seg_end,
                                                             u32 n_seg, u64 min_n, SizeClassTable table,
                                                             u32* __restrict__ lists, u32* __restrict__ cnt) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  int cls = -1;
  if (t < n_seg) cls = size_class(seg_end[t] - seg_begin[t], table, min_n);
  const int lane = lane_id();
  for (int c = 0; c <= table.n_classes; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (!m) continue;
    u32 base = 0;
    if (lane == 0) base = atomicAdd(cnt + c, static_cast<u32>(__popcll(m)));
    base = __shfl(base, 0, 64);
    if (cls == c) lists[static_cast<size_t>(c) * n_seg + base + __popcll(m & ((1ULL << lane) - 1ULL))] = t;
  }
}
// one workgroup per segment of a class, the segment in LDS sized for the class
template <int NT, bool PAY>
__global__ __launch_bounds__(NT) void seg_sort_lds_kernel(u64* __restrict__ keys, u64* __restrict__ pays,
                                                         const u64* __restrict__ seg_begin, const u64* __restrict__ seg_end,
                                                         const u32* __restrict__ list, u32 n_list, u32 cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seg_smem[];
  if (blockIdx.x >= n_list) return;
  const u32 t = list[blockIdx.x];
  const u64 b = seg_begin[t];
  block_sort_lds<NT, PAY>(keys, PAY ? pays : nullptr, b, static_cast<u32>(seg_end[t] - b), cap, seg_smem);
}
// ... and of the segments beyond the largest class: a wave each, through global memory
template <bool PAY>
__global__ __launch_bounds__(256) void seg_sort_wave_kernel(u64* k0, u64* k1, u64* p0, u64* p1, const u64* __restrict__ seg_begin,
                                                           const u64* __restrict__ seg_end, const u32* __restrict__ list,
                                                           u32 n_list) {
  __shared__ u32 hist[4][512];
  const u32 q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_list) return;
  const u32 t = list[q];
  const u64 b = seg_begin[t], e = seg_end[t];
  wave_sort_segment<PAY>(k0, k1, PAY ? p0 : nullptr, PAY ? p1 : nullptr, b, e - b, hist[threadIdx.x >> 6]);
}

// The LDS kernel of 256 threads is launched with more than 64 KB from the 4 096-entry class (PAY) / the 8 192-entry class
// (keys only) on: the opt-in for classes up to largest_cap, on the current device.
template <bool PAY>
void seg_sort_allow_lds(u32 largest_cap) {
  RVN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(seg_sort_lds_kernel<256, PAY>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(seg_sort_lds_bytes<256, PAY>(largest_cap))));
}

// What a sort leaves for its caller: the segments by class (device lists in e.map.chain_big, valid until its next use)
struct SegClasses {
  const u32* lists = nullptr;
  u32 n_seg = 0;
  u32 count[kMaxSizeClasses + 1] = {};
  const u32* list(int c) const { return lists + static_cast<size_t>(c) * n_seg; }
};

// Sorts every segment of at least min_n keys in k0 (payloads in p0 when PAY; k1 / p1: the other side of the ping-pong,
// touched only beyond the table) on e.stream, launches attributed to `site`: one classification, one read-back of the
// counts, then the class beyond the table first and the classes downwards — the largest run longest.
template <bool PAY>
SegClasses seg_sort(Engine& e, KernelSite site, const SizeClassTable& table, u64 min_n, const u64* seg_begin,
                    const u64* seg_end, u32 n_seg, u64* k0, u64* k1, u64* p0, u64* p1) {
  hipStream_t s = e.stream;
  const int nc = table.n_classes;
  u32* lists = e.map.chain_big.get<u32>(static_cast<size_t>(n_seg) * (nc + 1) + 16);
  u32* d_cnt = lists + static_cast<size_t>(n_seg) * (nc + 1);
  RVN_HIP(hipMemsetAsync(d_cnt, 0, (nc + 1) * 4, s));
  size_class_list_kernel<<<div_up(n_seg, 256), 256, 0, s>>>(seg_begin, seg_end, n_seg, min_n, table, lists, d_cnt);
  RVN_LAUNCH_CHECK();
  read_back(e, d_cnt, (nc + 1) * 4);
  SegClasses cls;
  cls.lists = lists;
  cls.n_seg = n_seg;
  std::memcpy(cls.count, e.h_pin, (nc + 1) * 4);
  if (cls.count[nc])
    RVN_KLAUNCH(site, seg_sort_wave_kernel<PAY><<<div_up(cls.count[nc], 4), 256, 0, s>>>(k0, k1, p0, p1, seg_begin, seg_end,
                                                                                       cls.list(nc), cls.count[nc]));
  for (int c = nc - 1; c >= 0; --c) {
    if (!cls.count[c]) continue;
    const u32 cap = table.cap[c];
    if (cap <= 512)
      RVN_KLAUNCH(site, seg_sort_lds_kernel<64, PAY><<<cls.count[c], 64, seg_sort_lds_bytes<64, PAY>(cap), s>>>(
                            k0, p0, seg_begin, seg_end, cls.list(c), cls.count[c], cap));
    else
      RVN_KLAUNCH(site, seg_sort_lds_kernel<256, PAY><<<cls.count[c], 256, seg_sort_lds_bytes<256, PAY>(cap), s>>>(
                            k0, p0, seg_begin, seg_end, cls.list(c), cls.count[c], cap));
  }
  return cls;
}

}  // namespace

}  // namespace rvn
