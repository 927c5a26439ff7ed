// poa4_ops.h — the small instruction-level helpers of the window kernel (poa4.hip): one CDNA4 instruction each, plain C++
// under the host wavefront emulator.  With simt.h and poa4_esc.h the only place where the two meanings of the source part.
#pragma once
#include "poa4_layout.h"
namespace rvn {
namespace {
__host__ __device__ __forceinline__ u32 funnel_shr(u32 hi, u32 lo, u32 sh) {  // v_alignbit_b32; sh in [0, 31]
  return static_cast<u32>(((static_cast<unsigned long long>(hi) << 32) | lo) >> sh);
}
__host__ __device__ __forceinline__ i32 sext16(u32 x) { return static_cast<i32>(static_cast<i16>(x & 0xFFFFu)); }
__host__ __device__ __forceinline__ i32 imax(i32 a, i32 b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ i32 imin(i32 a, i32 b) { return a < b ? a : b; }
// a + (p & 0xFFFF) / a + (p >> 16): v_add_u32 with an SDWA source select, so two 16-bit fields share a register
template <bool HI>
__host__ __device__ __forceinline__ u32 add_half(u32 a, u32 p) {
#if defined(__HIP_DEVICE_COMPILE__)
  u32 d;
  if constexpr (HI)
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(d) : "v"(a), "v"(p));
  else
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(d) : "v"(a), "v"(p));
  return d;
#else
  return a + (HI ? p >> 16 : p & 0xFFFFu);
#endif
}
// int16 half of w * 256 + tag: v_mad_i32_i16 reads the half through op_sel, the cells stay packed as the LDS read delivers
// them.  A key is score << 8 | tag (round 6; rounds 4-5: << 4): the score is bytes 1..2 of the key, so the two cells of a step
// go back into one packed word with ONE v_perm_b32 (keys_to_pair) instead of two shifts and a pack.
template <bool HI, int TAG>
__host__ __device__ __forceinline__ i32 cell_key(u32 w) {
#if defined(__HIP_DEVICE_COMPILE__)
  i32 d;
  if constexpr (HI) asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(d) : "v"(w), "s"(256), "n"(TAG));
  else asm("v_mad_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(w), "s"(256), "n"(TAG));
  return d;
#else
  return static_cast<i32>(static_cast<i16>((HI ? w >> 16 : w) & 0xFFFFu)) * 256 + TAG;
#endif
}
// (k0 >> 8) & 0xFFFF | (k1 >> 8) << 16
__host__ __device__ __forceinline__ u32 keys_to_pair(i32 k0, i32 k1) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(static_cast<u32>(k1), static_cast<u32>(k0), 0x06050201u);
#else
  return ((static_cast<u32>(k0) >> 8) & 0xFFFFu) | ((static_cast<u32>(k1) >> 8) << 16);
#endif
}
__host__ __device__ __forceinline__ i32 imax3(i32 a, i32 b, i32 c) {
  const i32 m = a > b ? a : b;
  return m > c ? m : c;
}
// byte B of acc replaced by the low byte of v (v_perm_b32; the other bytes of v are ignored)
template <int B>
__host__ __device__ __forceinline__ u32 put_byte(u32 acc, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr u32 sel = B == 0 ? 0x0C0C0C04u : (B == 1 ? 0x0C0C0400u : (B == 2 ? 0x0C040100u : 0x04020100u));
  return __builtin_amdgcn_perm(v, acc, sel);
#else
  const u32 keep = B == 0 ? 0u : (B == 1 ? 0xFFu : (B == 2 ? 0xFFFFu : 0xFFFFFFu));
  return (acc & keep) | ((v & 0xFFu) << (8 * B));
#endif
}
__host__ __device__ __forceinline__ u32 pack16(i32 lo, i32 hi) {  // (lo & 0xFFFF) | hi << 16
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(static_cast<u32>(hi), static_cast<u32>(lo), 0x05040100u);
#else
  return (static_cast<u32>(lo) & 0xFFFFu) | (static_cast<u32>(hi) << 16);
#endif
}
__host__ __device__ __forceinline__ u32 clamp_pair(u32 w) {  // both int16 halves clamped from below to kNegInf16
#if defined(__HIP_DEVICE_COMPILE__)
  typedef short pk16 __attribute__((ext_vector_type(2)));
  const pk16 lim = {static_cast<short>(kNegInf16), static_cast<short>(kNegInf16)};
  return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(pk16, w), lim));
#else
  const i32 a = sext16(w), b = sext16(w >> 16);
  return pack16(a < kNegInf16 ? kNegInf16 : a, b < kNegInf16 ? kNegInf16 : b);
#endif
}
// LDS of the wave as bytes from the start of its Poa4Lds (on the GPU the struct is the kernel's only __shared__ object)
__host__ __device__ __forceinline__ u32 lds_ld32(const Poa4Lds& S, u32 off) {
  return *reinterpret_cast<const u32*>(reinterpret_cast<const unsigned char*>(&S) + off);
}
__host__ __device__ __forceinline__ void lds_st32(Poa4Lds& S, u32 off, u32 v) {
  *reinterpret_cast<u32*>(reinterpret_cast<unsigned char*>(&S) + off) = v;
}
__host__ __device__ __forceinline__ i32 lds_ld16(const Poa4Lds& S, u32 off) {
  return *reinterpret_cast<const i16*>(reinterpret_cast<const unsigned char*>(&S) + off);
}
// LDS traffic of one wave is executed in order on the GPU; the emulator's fibres need a rendezvous between a lane's LDS
// write and another lane's read of it
__host__ __device__ __forceinline__ void lds_order() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_wave_barrier();
#else
  sv::sync();
#endif
}
#if defined(__HIP_DEVICE_COMPILE__)
#define P4_MARK(x) asm volatile("; P4MARK " x)
#define P4_ASSUME_GLOBAL(p) \
  __builtin_assume(!__builtin_amdgcn_is_shared((const void*)(p))); \
  __builtin_assume(!__builtin_amdgcn_is_private((const void*)(p)))
#define P4_ASSUME_LDS(p) __builtin_assume(__builtin_amdgcn_is_shared((const void*)(p)))
#define P4_NO_UNROLL _Pragma("unroll 1")  // in front of a loop of a rare path that must not cost the common path a register
#else
#define P4_NO_UNROLL
#define P4_MARK(x)
#define P4_ASSUME_GLOBAL(p)
#define P4_ASSUME_LDS(p)
#endif

// The lane's slot pointer, made opaque to the optimiser: field addresses derived from it are computed where they are used
// instead of being hoisted out of a loop and kept (or spilled: a reload is a memory load the loop then waits for) there.
__host__ __device__ __forceinline__ unsigned char* opaque(unsigned char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(p));
#endif
  return p;
}
// ---- fences for the compiler: empty asm statements, no instruction of their own; nothing under the emulator -----------
// A value in a vector register made opaque where it stands: it is computed HERE, from what it is made of here — not kept
// since before a loop, and not sunk to its use (which would keep what it is made of alive until then).
__host__ __device__ __forceinline__ u32 pin_v(u32 x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  return x;
}
// The same, and the words x, y, z of d are wanted here too: all of an LDS read, not where a branch first asks for a part.
__host__ __device__ __forceinline__ u32 pin_v(u32 x, const uint4& d) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x) : "v"(d.x), "v"(d.y), "v"(d.z));
#endif
  return x;
}
// A wave-uniform distance in scalar registers made opaque: the address it is added to is formed where it is used, not
// kept as a pointer of its own (poa4_traceback: such pointers lived in scratch memory across the walk).
template <class T>
__host__ __device__ __forceinline__ T pin_s(T x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(x));
#endif
  return x;
}
// The words of loads in flight, ORed together by the caller, are waited for HERE, by every lane: left to a branch behind
// it, the compiler has to wait again where the next loads overwrite their registers.  (An empty asm statement is no use of
// a register for the compiler's wait counting; an instruction — the OR — is.)
__host__ __device__ __forceinline__ void await_v(u32 seen) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(seen));
#endif
}
// The registers an outstanding store took its data and address from stay untouched until here: the compiler guards a
// register such a store reads against being overwritten by waiting for the store — right behind it, had it been free to
// reuse them.
__host__ __device__ __forceinline__ void hold_v(u32 a, u32 b, const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : : "v"(a), "v"(b), "v"(p));
#endif
}
// RVN_POA4_RING_FILL, host emulator of the debug build only (tests/test_poa4_emulation.py): the rings of the NW start as
// scores of cells far off the diagonal (1), as huge ones (2), as scores around those of a band's edge in a window's first
// rows (3) instead of -inf — what a read beside a predecessor's band then finds is adversarial, and every window that still
// comes back polished must equal the oracle: exactness rests on the traceback's band checks, not on what the ring holds.
template <class K>
__host__ __device__ __forceinline__ void ring_fill_knob(Poa4Lds& S, int gl, int q, u32 len) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(RVN_DEBUG_KNOBS)
  if (const char* f = knob("RVN_POA4_RING_FILL")) {
    const int mode = std::atoi(f);
    for (int idx = gl; idx < K::kRing * kRowW4; idx += 16) {
      u32 h = (static_cast<u32>(idx) * 2654435761u) ^ (static_cast<u32>(q) * 40503u) ^ (len * 97u);
      h ^= h >> 13;
      const i32 base = mode == 3 ? 10 : -100, span = mode == 3 ? 50 : 800;
      const i32 lo = mode == 2 ? 28000 : base - static_cast<i32>(h % span), hi = mode == 2 ? 28000 : base - static_cast<i32>((h >> 12) % span);
      if (mode >= 1 && mode <= 3) lds_st32(S, poa4_ring_byte(q, static_cast<u32>(idx)), pack16(lo, hi));
    }
  }
#endif
}
// minimum / maximum over the 16 lanes of a window
__host__ __device__ inline u32 group_min_u(u32 v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    const u32 o = static_cast<u32>(sv::bperm(static_cast<int>(v), sv::lane() ^ off));
    v = o < v ? o : v;
  }
  return v;
}
__host__ __device__ inline i32 group_max_i(i32 v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    const i32 o = sv::bperm(v, sv::lane() ^ off);
    v = o > v ? o : v;
  }
  return v;
}

__host__ __device__ __forceinline__ u32 mulhi_u32(u32 a, u32 b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return static_cast<u32>((static_cast<unsigned long long>(a) * b) >> 32);
#endif
}
// n / d for n * d < 2^32 through m = magic_of(d): floor(2^32 / d) + 1, 0 standing for d == 1
__host__ __device__ __forceinline__ u32 magic_of(u32 d) { return d <= 1 ? 0u : static_cast<u32>(0x100000000ULL / d) + 1u; }
__host__ __device__ __forceinline__ u32 div_magic(u32 n, u32 m) { return m ? mulhi_u32(n, m) : n; }
// atomics on a window's own data (workgroup scope: one wave owns it); the emulator's fibres run one at a time
__host__ __device__ __forceinline__ void atomic_add_i32(i32* p, i32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  *p += v;
#endif
}
__host__ __device__ __forceinline__ void atomic_inc_u16(u16* base, u32 idx) {  // base 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_add(reinterpret_cast<u32*>(base) + (idx >> 1), (idx & 1u) ? 0x10000u : 1u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  base[idx] += 1;
#endif
}

__host__ __device__ __forceinline__ void atomic_max_u32(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(p, v);
#else
  if (v > *p) *p = v;
#endif
}
__host__ __device__ __forceinline__ void atomic_add_u32(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, v);
#else
  *p += v;
#endif
}
// a word of the escalation queue (poa4_esc.h): agent scope, the waves that share it sit on different XCDs
__host__ __device__ __forceinline__ u32 poa4_esc_load(const u32* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
}  // namespace
}  // namespace rvn
