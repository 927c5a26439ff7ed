// sizeclass.h — the size-class tables of Map's chain stage, each written ONCE, and the rule that puts a segment into its
// class: the class-list kernel (segsort.h), the host ladders that launch one kernel per class (segsort.h, chain.hip) and
// the host test program (tests/host/size_class_host.cpp, which holds tests/chain_util.py's restatement to these) all go
// by this file.  Plain C++: the host compiler alone can read it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RVN_SIZECLASS_HD __host__ __device__
#else
#define RVN_SIZECLASS_HD
#endif

namespace rvn {

constexpr int kMaxSizeClasses = 8;
// caps ascend; class c holds the segments of cap[c - 1] < n <= cap[c] entries, class n_classes those beyond the last cap
struct SizeClassTable {
  int n_classes;
  uint32_t cap[kMaxSizeClasses];
};

// Group sort of a read's matches (round 6; rounds 1-5: one workgroup of 256 threads with LDS for 2048 pairs per read
// whatever its size — 67 KB, two workgroups per CU — and a wave through global memory beyond that).  A read's segment of
// <= cap (key, payload) pairs is sorted by one workgroup whose LDS is sized for the class: the typical read of an ONT
// pass (1 000 - 3 000 matches per launch) gets a workgroup that fits four to eight times per CU.
constexpr SizeClassTable kSegClassTable = {5, {256, 512, 1024, 2048, 4096}};
constexpr uint64_t kSegClassMin = 2;  // a segment of fewer entries is sorted as it stands

// Intervals of the chain stage.  Small ones (chain <= n <= kChainSmallCap) take one LANE each (chain_small_kernel); every
// larger one is handled by ONE wave = one workgroup whose dynamic LDS is sized for the class (tails, tail indices,
// predecessors of the whole interval), so the number of resident waves per CU follows the interval size (3 KB for <= 256
// matches ... 99 KB for <= 8192) and no wave waits for a sibling's longer interval.  Intervals beyond kChainBigCap run the
// same code on global scratch (class n_classes).  The position sort goes by the same classes.
// (finer classes in the range where the intervals of a polishing round's read-to-contig maps fall, 300 - 700 matches: a
// wave's LDS is ~12 B per match of its class, and the stage is a serial LIS per wave — occupancy is its throughput)
constexpr uint32_t kChainSmallCap = 32;
constexpr uint32_t kChainBigCap = 8192;
constexpr SizeClassTable kChainClassTable = {8, {128, 256, 512, 768, 1024, 2048, 4096, kChainBigCap}};
// smallest interval that gets a class: beyond the one-lane kernel's and long enough to hold a chain at all
RVN_SIZECLASS_HD inline uint64_t chain_class_min(uint32_t chain) { return chain > kChainSmallCap ? chain : kChainSmallCap + 1; }

// class of a segment of n entries: -1 below min_n (no class: nothing is launched for it), else the first class whose cap
// holds it, else table.n_classes
RVN_SIZECLASS_HD inline int size_class(uint64_t n, const SizeClassTable& table, uint64_t min_n) {
  if (n < min_n) return -1;
  int cls = table.n_classes;
  for (int c = kMaxSizeClasses - 1; c >= 0; --c)
    if (c < table.n_classes && n <= table.cap[c]) cls = c;
  return cls;
}

}  // namespace rvn
