// poa4_esc.h — the windows the first attempt hands on, inside the same launch (round 6).  Included by poa4.hip behind the
// kernel's LDS union (Poa4LdsAll); device-only by nature: the emulator has no queue and runs the first attempt alone.
#pragma once
#include "poa4_ops.h"
namespace rvn {
namespace {
// 3 of 200 000 windows of a C4 round (244 before rows of 9..15 in-edges stayed here) need the 64-column band.  As a launch of
// their own behind this one they cost one window's latency whatever their number — 30-38 ms per round, and the reason a batch
// of a few thousand windows did not start here at all.  Now a wave whose window fails with a band hit puts its index into a queue
// in HBM (agent-scope atomics: the waves sit on eight XCDs whose L2s do not see each other's lines) and goes on with the rest of
// its group; every wave looks at the queue between two groups and runs what it finds — one window on the whole wave, poa2's window
// function with its 64-column band, the wave's four scratch slots as that function's one — and again before it leaves.  A window
// pushed after a wave looked is taken by any wave that comes by later, at the latest by the pusher itself: no wave waits for
// another.  What the 64 columns cannot do either comes back with bit 28 set in its status (the host goes on with 128 columns).
constexpr u32 kEscEmpty = 0xFFFFFFFFu;

// wave-uniform; every lane takes part (lane 0 adds one, the others nothing: see poa4_persistent on why not `if (lane == 0)`)
__host__ __device__ inline bool poa4_esc_push(const Poa4Args& A, u32 wi) {
#if defined(__HIP_DEVICE_COMPILE__)
  u32 k = __hip_atomic_fetch_add(A.esc, sv::lane() == 0 ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  k = static_cast<u32>(sv::rfl(static_cast<int>(k)));
  if (k >= A.esc_cap) return false;
  if (sv::lane() == 0) __hip_atomic_store(A.esc + 4 + k, wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
#else
  (void)A;
  (void)wi;
  return false;
#endif
}
// the next window of the queue (wave-uniform), kEscEmpty: none right now
__host__ __device__ inline u32 poa4_esc_pop(const Poa4Args& A) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (;;) {
    u32 p = static_cast<u32>(sv::rfl(static_cast<int>(poa4_esc_load(A.esc))));
    p = p < A.esc_cap ? p : A.esc_cap;
    const u32 t = static_cast<u32>(sv::rfl(static_cast<int>(poa4_esc_load(A.esc + 1))));
    if (t >= p) return kEscEmpty;
    // (all 64 lanes try the same exchange: one of them gets it, or a lane of another wave did)
    u32 expected = t;
    const bool won = __hip_atomic_compare_exchange_strong(A.esc + 1, &expected, t + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!sv::any(won)) continue;
    for (;;) {  // (the pusher stores the index right behind its ticket)
      const u32 e = static_cast<u32>(sv::rfl(static_cast<int>(poa4_esc_load(A.esc + 4 + t))));
      if (e != kEscEmpty) return e;
      __builtin_amdgcn_s_sleep(8);
    }
  }
#else
  (void)A;
  return kEscEmpty;
#endif
}
// NOT inlined, and not handed the batch description either: as part of the persistent kernel's one function the 64-column code
// changed the register allocation of the NW and of the traceback (the walk's descriptor pointer went to scratch memory again:
// tests/test_poa4_isa.py), and a reference to the kernel's arguments passed to a real call moves ALL of them to the stack.  The
// callee reads the arguments where the launch left them — the kernel-argument segment, scalar loads — and gets five registers.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __attribute__((noinline)) void poa4_esc_window_far(p2::Poa2Lds<1>* Sp, u32 ka_lo, u32 ka_hi, u32 pw_, u32 wi_) {
  P4_ASSUME_LDS(Sp);
  typedef const __attribute__((address_space(4))) Poa4Args* ArgsPtr;
  // (the address of the kernel-argument segment comes from the kernel: the intrinsic is null in a function that is not one)
  const unsigned long long ka = (static_cast<unsigned long long>(static_cast<u32>(sv::rfl(static_cast<int>(ka_hi)))) << 32) |
                                static_cast<u32>(sv::rfl(static_cast<int>(ka_lo)));
  const Poa4Args A = *(ArgsPtr)ka;  // (the kernel's first parameter)
  const u32 pw = static_cast<u32>(sv::rfl(static_cast<int>(pw_))), wi = static_cast<u32>(sv::rfl(static_cast<int>(wi_)));
  const PoaWindow win = A.windows[wi];
  Poa2Slot g = poa2_carve(A.scratch + static_cast<size_t>(pw) * P4::G * A.slot_bytes, A.nmax, A.lmax, 64);
  u32 st = p2::poa2_window<1>(win, A.layers, A.src, g, A.nmax, A.lmax, A.m, A.n_, A.gp, A.trim, *Sp, A.out + win.out_off, A.out_len + wi,
                              A.phase_cycles, 0u);
  if ((st & 0xFFu) != 1u) st |= kPoaTried64;
  if (A.esc_wide && ((st & 0xFFu) == kPoaBandHit || (st & 0xFFu) == 7u)) {
    // the 128-column band right behind it (one window per C4 step: as a launch of its own, 29 ms); its LDS is the same 10 KB
    Poa2Slot g2 = poa2_carve(A.scratch + static_cast<size_t>(pw) * P4::G * A.slot_bytes, A.nmax, A.lmax, 128);
    sv::sync();
    if (sv::lane() == 0) atomicAdd(A.esc + 2, 1u);
    st = p2::poa2_window<2>(win, A.layers, A.src, g2, A.nmax, A.lmax, A.m, A.n_, A.gp, A.trim, *reinterpret_cast<p2::Poa2Lds<2>*>(Sp), A.out + win.out_off,
                            A.out_len + wi, A.phase_cycles, 0u);
    if ((st & 0xFFu) != 1u) st |= kPoaTried64 | kPoaTried128;
  }
  if (sv::lane() == 0) A.status[wi] = st;
  sv::sync();
}
#endif
__host__ __device__ __forceinline__ void poa4_esc_window(Poa4LdsAll& S, u32 pw, u32 wi) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned long long ka = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  poa4_esc_window_far(&S.u.w64, static_cast<u32>(ka), static_cast<u32>(ka >> 32), pw, wi);
#else
  (void)S;
  (void)pw;
  (void)wi;
#endif
}
}  // namespace
}  // namespace rvn
