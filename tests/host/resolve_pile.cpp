// Pile::ClearChimericRegions(median) as the device runs it — raven_amd/csrc/chimeric.h, the __host__ __device__ code of
// resolve.hip's lane-0 path, compiled here for the host — on every pile that is not invalid of an input in the format of
// tests/host/resolve_reference.cpp, with the pile's own median[i] as the argument: what `resolve_reference piles` states.
// Writes the same output format, so that the CPU suite compares the shared header with the restatement without a GPU.
#include <cstdint>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "chimeric.h"

namespace {

template <typename T>
void Get(std::ifstream& in, T* p, std::size_t n) {
  in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input");
}
template <typename T>
void Put(std::ofstream& out, const T* p, std::size_t n) {
  out.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
}

}  // namespace

int main(int argc, char** argv) {
  using namespace rvn;
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  u32 n = 0, phases = 0;
  double identity = 0;
  Get(in, &n, 1);
  Get(in, &phases, 1);
  Get(in, &identity, 1);
  std::vector<u32> off(n + 1), roff(n + 1), begin(n), end(n);
  Get(in, off.data(), n + 1);
  if (off[n] != 0) return 3;  // piles only: this program takes no overlaps
  std::vector<u64> coff(n + 1);
  Get(in, coff.data(), n + 1);
  std::vector<u16> cov(coff[n]), median(n);
  Get(in, cov.data(), cov.size());
  Get(in, roff.data(), n + 1);
  std::vector<u32> reg(2 * static_cast<std::size_t>(roff[n]));
  Get(in, reg.data(), reg.size());
  Get(in, begin.data(), n);
  Get(in, end.data(), n);
  Get(in, median.data(), n);
  std::vector<u8> invalid(n), contained(n, 0), chimeric(n, 0);
  Get(in, invalid.data(), n);

  std::vector<u32> o_roff(n + 1, 0), o_reg, o_off(n + 1, 0);
  u32 cut = 0, invalidated = 0;
  for (u32 i = 0; i < n; ++i) {
    u32 left = roff[i + 1] - roff[i];
    u32* r = reg.data() + 2 * static_cast<std::size_t>(roff[i]);
    if (!invalid[i]) {
      const ChimericOutcome o = clear_chimeric_regions(cov.data() + coff[i], begin[i], end[i], r, left, median[i]);
      begin[i] = o.begin;
      end[i] = o.end;
      left = o.n_unresolved;
      chimeric[i] = o.chimeric ? 1 : 0;
      cut += o.chimeric ? 1 : 0;
      if (o.invalid) {
        invalid[i] = 1;
        ++invalidated;
      }
    }
    o_reg.insert(o_reg.end(), r, r + 2 * static_cast<std::size_t>(left));
    o_roff[i + 1] = static_cast<u32>(o_reg.size() / 2);
  }
  // (this program is run on inputs without overlaps: the lists come out empty)
  const u64 m = 0;
  const u16 global_median = 0;
  const u64 zero64[4] = {0, 0, 0, 0};
  const u32 zero32[2] = {0, 0};
  std::ofstream out(argv[2], std::ios::binary);
  Put(out, begin.data(), n);
  Put(out, end.data(), n);
  Put(out, invalid.data(), n);
  Put(out, contained.data(), n);
  Put(out, chimeric.data(), n);
  Put(out, o_roff.data(), n + 1);
  Put(out, o_reg.data(), o_reg.size());
  Put(out, &global_median, 1);
  Put(out, &m, 1);
  Put(out, o_off.data(), n + 1);
  Put(out, cov.data(), cov.size());
  Put(out, zero64, 4);
  Put(out, zero32, 2);
  Put(out, &cut, 1);
  Put(out, &invalidated, 1);
  return out ? 0 : 1;
}
