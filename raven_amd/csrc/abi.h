// abi.h — the error and guard layer of the C ABI (include/raven_hip.h): included by every translation unit that exports
// extern "C" symbols.  An entry point reports through fail() and runs its body under guarded().
#pragma once

#include <mutex>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/raven_hip.h"
#include "engine.h"

namespace rvn {

// the calling thread's rvn_last_error() (engine.hip)
void set_last_error(const std::string& msg);
const std::string& last_error();

inline int fail(int code, const std::string& msg) {
  set_last_error(msg);
  return code;
}

template <typename F>
int guarded(F f) {
  try {
    return f();
  } catch (const HipError& ex) {
    return fail(RVN_EHIP, ex.what());
  } catch (const std::bad_alloc&) {
    return fail(RVN_ENOMEM, "[raven_hip] out of host memory");
  } catch (const std::invalid_argument& ex) {
    return fail(RVN_EINVAL, ex.what());
  } catch (const std::exception& ex) {
    return fail(RVN_EHIP, ex.what());
  }
}

// same, holding the engine's lock for the whole call (nullptr: the lambda reports the NULL handle itself).  A stage
// that runs out of DEVICE memory is run once more after every scratch buffer of the engine (the other phase's included)
// and every parked block went back to the driver: the entry points are functions of their arguments, a stage that
// failed half-way leaves nothing behind but scratch.
template <typename F>
int guarded(Engine* e, F f) {
  if (!e) return guarded(f);
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  try {
    return f();
  } catch (const DeviceOutOfMemory& ex) {
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    if (knob("RVN_DEBUG_MEM")) std::fprintf(stderr, "[raven_hip] %s: all scratch back to the driver, stage repeated\n", ex.what());
    e->oom_mask |= 1u << (e->stage_kind & 31);  // next time this kind of stage starts from released scratch
    try {
      engine_release_scratch(*e);
    } catch (const std::exception& ex2) {
      return fail(RVN_EHIP, ex2.what());
    }
  } catch (const HipError& ex) {
    return fail(RVN_EHIP, ex.what());
  } catch (const std::bad_alloc&) {
    return fail(RVN_ENOMEM, "[raven_hip] out of host memory");
  } catch (const std::invalid_argument& ex) {
    return fail(RVN_EINVAL, ex.what());
  } catch (const std::exception& ex) {
    return fail(RVN_EHIP, ex.what());
  }
  return guarded(f);
}

// The opening many entry points share, done once: `args_ok` is their NULL-argument check (h included; RVN_EINVAL with
// `what` when it fails), then the engine's device is made current and its kernel timers are taken; f(Engine&) is the rest.
template <typename F>
int guarded(rvn_engine* h, bool args_ok, const char* what, F f) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!args_ok) return fail(RVN_EINVAL, what);
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    UseTimers ut(e);
    return f(e);
  });
}

// The one copy of an entry point that exists for host pointers and for device pointers (rvn_*_dev): a blocking hipMemcpy
// to or from the host, a copy ordered on the engine's stream between device buffers (the caller synchronises the stream).
inline void put(Engine& e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (kind == hipMemcpyDeviceToDevice) RVN_HIP(hipMemcpyAsync(dst, src, bytes, kind, e.stream));
  else RVN_HIP(hipMemcpy(dst, src, bytes, kind));
}

// The argument check of the span records of rvn_edit_distance_batch (and of whoever else takes them): nullptr, or what is
// wrong with them.  Every index a kernel forms from a record stays inside the read set when this passes.
inline const char* ed_pairs_error(const ReadsDev& rd, const rvn_ed_pair* pairs, u32 n_pairs) {
  for (u32 i = 0; i < n_pairs; ++i) {
    const rvn_ed_pair& p = pairs[i];
    if (p.lhs_read >= rd.n || p.rhs_read >= rd.n || static_cast<u64>(p.lhs_begin) + p.lhs_len > rd.h_len[p.lhs_read] ||
        static_cast<u64>(p.rhs_begin) + p.rhs_len > rd.h_len[p.rhs_read])
      return "span outside its read";
  }
  return nullptr;
}

// The argument check of a CSR offsets array off[n + 1] whose lists must stay below max_len entries: nullptr, or what is
// wrong with it (the entry point puts its name in front).
constexpr u64 kMaxPileCells = 1ULL << 27;  // a pile's coverage / k-mer cells
constexpr u64 kNoCsrLimit = ~0ULL;
template <typename T>
const char* csr_offsets_error(const T* off, u32 n, u64 max_len) {
  if (off[0] != 0) return "offsets must start at 0";
  for (u32 i = 0; i < n; ++i) {
    if (off[i + 1] < off[i]) return "offsets must not decrease";
    if (off[i + 1] - off[i] >= max_len) return "a pile of 2^27 cells or more";
  }
  return nullptr;
}

}  // namespace rvn
