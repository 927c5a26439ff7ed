// poa4_limits.h — the limits of the rows-on-lanes window kernel (poa4.hip): what a window may ask of the 32-column attempt
// before it goes on to poa2's wider bands.  Plain C++ (no HIP): tests/host/poa4_limits_host.cpp prints these values and
// tests/test_poa4_limits.py holds their restatement in tests/poa_cases.py to them.
#pragma once
#include <cstdint>
namespace rvn {
using u32 = std::uint32_t;  // (as common.h: the header stands alone)
using i32 = std::int32_t;
namespace {
struct P4 {
  static constexpr int G = 4, GS = 16, kBand = 32;
  static constexpr int kRing = 22;    // score rows a window keeps in LDS = longest in-edge (in ranks) + 1 (a longer one sends the
                                      // window to poa2: none in 9 220 layers of 300 C4-like windows, the longest was 17.  Rounds 4-5
                                      // kept 24; round 6 gave two rows' worth of LDS to the lanes' row descriptors (Poa4Lds::qa ..)
  static constexpr int kRowB = 64;    // bytes per ring row: the 32 cells of the row's band, addressed by the COLUMN (poa4_layout.h)
  static constexpr int kMaxD = 8;     // largest band-start difference along an in-edge (a larger one sends the window to poa2)
  static constexpr int kEdges = 8;    // in-edges a row descriptor holds (4-bit backpointers: 8 diagonal + 7 vertical codes + 0 = horizontal
                                      // or vertical through in-edge 7, see poa4.hip)
  static constexpr int kEdgesMax = 15;  // in-edges of a row this kernel follows: a row of 9..15 keeps in-edges 0..6 in its descriptor and
                                        // in-edges 7..14 in an overflow record (Poa4Slot::ovf) the step's rare path reads; a row with more
                                        // sends the window to poa2 (the graph itself keeps kPoaMaxIn = 16)
  static constexpr int kU = 8;        // steps between two service points (descriptor prefetch, backpointer store)
};
constexpr u32 kNone4 = 0xFFFFu;
constexpr i32 kNegU = -0x30000000;   // the horizontal chain's value left of a band (a key: score << 8)
constexpr u32 kInactiveS = 0x7FFFu;  // "no row": the 2 S field of a descriptor (odd — a real row's is even — and later than any step)
}  // namespace
}  // namespace rvn
