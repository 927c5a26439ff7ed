// devpool.hip — the device arena behind the grow-only buffers (common.h: devpool).
#include <mutex>

#include "common.h"
#include "freelist.h"

namespace rvn {
namespace devpool {
namespace {
struct Arena {
  char* base = nullptr;
  FreeList list;  // freelist.h: offsets of the blocks in use and of the holes
};
constexpr int kMaxDevices = 16;
constexpr size_t kGrain = 64 << 10;
std::mutex g_mu;
Arena g_arena[kMaxDevices];
Arena* mine() {
  int d = 0;
  (void)hipGetDevice(&d);
  return (d >= 0 && d < kMaxDevices) ? &g_arena[d] : nullptr;
}
size_t offset_of(const Arena& a, const void* p) { return static_cast<size_t>(static_cast<const char*>(p) - a.base); }
bool inside(const Arena& a, const void* p) {
  return a.base && static_cast<const char*>(p) >= a.base && static_cast<const char*>(p) < a.base + a.list.size;
}
}  // namespace
bool active() {
  std::lock_guard<std::mutex> lk(g_mu);
  const Arena* a = mine();
  return a && a->base;
}
bool start(size_t bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  Arena* a = mine();
  if (!a || a->base) return a && a->base;
  bytes = bytes / kGrain * kGrain;
  if (bytes < (1ULL << 30)) return false;
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  a->base = static_cast<char*>(p);
  a->list.reset(bytes, kGrain);
  return true;
}
void* alloc(size_t bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  Arena* a = mine();
  if (!a || !a->base) return nullptr;
  size_t off = 0;
  return a->list.alloc(bytes, &off) ? a->base + off : nullptr;
}
// The arena a pointer lies in, whatever device is current (one virtual address space for all devices of the process): a
// buffer carved from device i's arena may be released while device j is current — a worker's error path, a handle
// destroyed from the main thread — and must go back to ITS arena, not be mistaken for a driver allocation.
namespace {
int owner_of(const void* p) {
  for (int d = 0; d < kMaxDevices; ++d)
    if (inside(g_arena[d], p)) return d;
  return -1;
}
}  // namespace
bool give_back(void* p) {
  int owner = -1;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    owner = owner_of(p);
    if (owner < 0 || !g_arena[owner].list.owns(offset_of(g_arena[owner], p))) return false;
  }
  // what hipFree does implicitly: nobody still reads the block when the next owner writes (the owning device's queues)
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (cur != owner) (void)hipSetDevice(owner);
  (void)hipDeviceSynchronize();
  if (cur != owner) (void)hipSetDevice(cur);
  std::lock_guard<std::mutex> lk(g_mu);
  Arena& a = g_arena[owner];
  return inside(a, p) && a.list.release(offset_of(a, p));
}
size_t free_total() {
  std::lock_guard<std::mutex> lk(g_mu);
  const Arena* a = mine();
  return a && a->base ? a->list.free_total() : 0;
}
size_t free_largest() {
  std::lock_guard<std::mutex> lk(g_mu);
  const Arena* a = mine();
  return a && a->base ? a->list.free_largest() : 0;
}
size_t size() {
  std::lock_guard<std::mutex> lk(g_mu);
  const Arena* a = mine();
  return a && a->base ? a->list.size : 0;
}
void stop() {
  std::lock_guard<std::mutex> lk(g_mu);
  Arena* a = mine();
  if (!a || !a->base || !a->list.in_use.empty()) return;
  (void)hipFree(a->base);
  a->base = nullptr;
  a->list.reset(0, kGrain);
}
}  // namespace devpool
}  // namespace rvn
