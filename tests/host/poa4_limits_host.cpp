// TEST INFRASTRUCTURE: the host build of raven_amd/csrc/poa4_limits.h — the limits of the rows-on-lanes window kernel —
// for the CPU test that holds tests/poa_cases.py's restatement to them (tests/test_poa4_limits.py).
// Output: one "name value" line per limit.
#include <cstdio>

#include "poa4_limits.h"

using rvn::P4;

int main() {
  std::printf("kRing %d\nkMaxD %d\nkEdges %d\nkEdgesMax %d\nkBand %d\nG %d\nGS %d\nkU %d\n", P4::kRing, P4::kMaxD, P4::kEdges,
              P4::kEdgesMax, P4::kBand, P4::G, P4::GS, P4::kU);
  return 0;
}
