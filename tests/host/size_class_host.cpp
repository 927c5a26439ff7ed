// TEST INFRASTRUCTURE: the host build of raven_amd/csrc/sizeclass.h — the size-class tables of Map's chain stage and
// size_class — for the CPU test that holds tests/chain_util.py's restatement to them (tests/test_size_class.py).
// Input (text, whitespace-separated): a sequence of cases, one output line per case.
//   tables        -> "seg min cap ...", "chain small_cap cap ..."  (two lines)
//   seg n         -> "class c"   the group sort's class of a read with n matches
//   chain chain n -> "class c"   the position sort's / chain_kernel's class of an interval of n matches at that `chain`
#include <cstdio>
#include <fstream>
#include <string>

#include "sizeclass.h"

using namespace rvn;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "tables") {
      std::printf("seg %llu", static_cast<unsigned long long>(kSegClassMin));
      for (int c = 0; c < kSegClassTable.n_classes; ++c) std::printf(" %u", kSegClassTable.cap[c]);
      std::printf("\nchain %u", kChainSmallCap);
      for (int c = 0; c < kChainClassTable.n_classes; ++c) std::printf(" %u", kChainClassTable.cap[c]);
      std::printf("\n");
    } else if (cmd == "seg") {
      unsigned long long n = 0;
      in >> n;
      std::printf("class %d\n", size_class(n, kSegClassTable, kSegClassMin));
    } else if (cmd == "chain") {
      unsigned chain = 0;
      unsigned long long n = 0;
      in >> chain >> n;
      std::printf("class %d\n", size_class(n, kChainClassTable, chain_class_min(chain)));
    } else {
      return 3;
    }
    if (!in) return 4;
  }
  return 0;
}
