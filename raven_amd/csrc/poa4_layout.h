// poa4_layout.h — where the window kernel (poa4.hip) keeps things: the NW's LDS, the batch description, a window's
// scratch slot, and the state record a window carries from phase to phase.
#pragma once
#include "poa.h"
#include "poa2_window.h"
#include "poa4_limits.h"
namespace rvn {
namespace {
// LDS of the NW.  A ring row holds the 32 cells of its row's band as 16 words, and the word of column pair p = j / 2 is
// p mod 16 WHATEVER the row's band start (a band is 16 pairs wide: every pair of it has a word of its own).  The score rings
// of the two windows of a HALF-WAVE (lanes 0-31: q = 0, 1; lanes 32-63: q = 2, 3) are interleaved word by word — word w of
// window q's ring at pair base + (2 w + (q & 1)) * 4.  A ds_read_b32 serves a half-wave per LDS cycle over 32 banks; the bank
// of an access is 2 (p mod 16) + (q & 1), whichever ring slot it goes to: at one step the 16 lanes of a window are at 16
// consecutive column pairs (lane to lane: one row on, one pair back), so in-edge reads of any slot, the -inf words of the
// in-edges a row does not have (same addressing) and the own row's store fall into 16 different banks of the window's
// parity.  (Round 4 / early round 5 addressed a row from its band start, pads of -inf either side: the lane-to-lane bank
// step was 10 or 8 with the drift of the band along the rows, and 48 % of the kernel's LDS cycles were bank conflicts.)
// What the pads were for — a predecessor's band ending left of the column asked for, or beginning at it — now reads
// another cell of the predecessor's row instead of -inf.  That is harmless by construction: such a candidate can only
// RAISE a cell, every cell the traceback walks is checked to lie inside its row's band (a move through such a candidate
// lands outside and sends the window to the 64-column kernel, as any band miss), and a walk that never leaves the bands has
// met only true values — so its score is both an upper and a lower bound of the banded optimum and its moves are the true
// maxima's.  The ring starts every layer as -inf so that what a first column finds left of a predecessor's
// band is low, not stale.  slot = rho % kRing.
constexpr int kRowW4 = P4::kRowB / 4;
struct alignas(16) Poa4Lds {
  // The row descriptor a lane is working on, and the one it works on next (round 6): two slots per lane, [slot][lane] so that
  // the 64 lanes' reads fall into different banks whichever slot each lane is at.  The NW step reads its row's words from
  // here (one ds_read_b128 + one ds_read_b32, issued a step AHEAD) instead of keeping current / next / in-flight copies in
  // registers: finishing a row is a pointer flip.  Rounds 4-5 copied seven registers under a lane mask at every row switch,
  // and one of the wave's 64 lanes switches in 98 % of the steps — a third of the step's instructions.
  uint4 qa[2][64];  // {2 S | own row's ring bytes << 16, in-edges 0 | 1 << 16, in-edges 2 | 3 << 16, match mask}
  u32 qm[2][64];    // bits 3..6: (8 x (band start / 2 mod 16) - 8 S) mod 128 (the step's column pair as ring bytes = (this + 8 t) & 0x78);
                    // bit 8 (alone in its byte: one SDWA compare): an end node's row; bits 24..27: in-edges; bit 31: the row has no in-edge, or more than four (the step's rare path)
  uint2 qe[2][64];  // {in-edges 4 | 5 << 16, in-edges 6 | 7 << 16}
  u32 qc[2][64];    // node | band start << 16 | in-edges << 26 | marked << 30 | end node << 31 (rare paths only)
  u32 ring[2][2 * P4::kRing * kRowW4];
  u32 dump[2][32];      // where rows outside the layer's subgraph leave their cells (interleaved like the rings)
  u32 neg[40];          // -inf cells: what a descriptor's unused in-edges point at (window parity p: words p, p + 2, ..)
};
// byte offsets from the start of Poa4Lds (what a row descriptor holds)
__host__ __device__ __forceinline__ u32 poa4_ring_byte(int q, u32 w) {
  return static_cast<u32>(offsetof(Poa4Lds, ring)) + static_cast<u32>(q >> 1) * static_cast<u32>(sizeof(u32) * 2 * P4::kRing * kRowW4) +
         (2u * w + static_cast<u32>(q & 1)) * 4u;
}
__host__ __device__ __forceinline__ u32 poa4_dump_byte(int q) {
  return static_cast<u32>(offsetof(Poa4Lds, dump)) + static_cast<u32>(q >> 1) * 128u + static_cast<u32>(q & 1) * 4u;
}
__host__ __device__ __forceinline__ u32 poa4_neg_byte(int q) { return static_cast<u32>(offsetof(Poa4Lds, neg)) + static_cast<u32>(q & 1) * 4u; }
static_assert(offsetof(Poa4Lds, qa) == 0, "a lane's slot pointer is a byte offset into qa");
static_assert(offsetof(Poa4Lds, ring) % 128 == 0 && offsetof(Poa4Lds, dump) % 128 == 0 && (sizeof(u32) * 2 * P4::kRing * kRowW4) % 128 == 0,
              "a row's ring bytes leave bits 3..6 to the column pair");
// (the phases of the kernel share the wave's LDS as a union: the NW the score rings, the graph update room for 896 order
// slots, the set-up + descriptor pass the layer's bytes, the traceback its staged rows)
static_assert(sizeof(Poa4Lds) <= 10240, "sixteen waves per CU need <= 10 KB of LDS each");
static_assert(P4::kRowB == 2 * P4::kBand, "ring row = the 32 cells of a band");

struct Poa4Args {
  const PoaWindow* windows;
  u32 n_windows;
  const PoaLayer* layers;
  PoaSrc src;
  unsigned char* scratch;
  size_t slot_bytes;
  u32 nmax, lmax;
  int m, n_, gp, trim;
  u8* out;
  u32* out_len;
  u32* status;
  unsigned long long* phase_cycles;
  const u32* sched;
  u32* next;
  u32* esc;      // queue of the windows the 32-column attempt hands on, taken up by the waves of the SAME launch between two groups
                 // (poa4_esc_*): [0] entries pushed, [1] entries taken, [2] windows that went on to 128 columns, [4 + k] window
                 // index (0xFFFFFFFF until stored); null: none
  u32 esc_cap;   // entries the queue holds (a window beyond them keeps its status for the host's escalation, as without a queue)
  u32 esc_wide;  // != 0: the wave's four slots also hold the 128-column function's one
};

// Per-window scratch: poa2's graph arrays + the row descriptors of the current layer + its backpointer stream.
struct Poa4Slot {
  Poa2Slot g;
  uint4* desc;   // 2 per row: {2 S | own << 16, node | b << 16 | np << 26 | marked << 30 | end << 31, rank distances of in-edges 0..5
                 //            (5 bits each), e0 | e1 << 16}, {e2 | e3 << 16, e4 | e5 << 16, e6 | e7 << 16, match mask}: what the
                 //            traceback needs of a row is its first 16 bytes
  u32* rb;       // per node: rank | backbone coordinate << 16 (kept by the set-up and by poa4_update_graph)
  u32* rbl;      // per node, for the CURRENT layer: rank | band start << 16 (first pass of the descriptor phase)
  u32* v7;       // per row with eight in-edges: bit c = column band start + c took the VERTICAL move through the eighth in-edge —
                 // the one move the 4-bit codes cannot tell from "horizontal" (both code 0); written by the NW for such rows only.
                 // Per row with 9..15 in-edges: bit c = column band start + c took its move through one of the in-edges 7..14
                 // (the code's low three bits then count from in-edge 7: 14 - in-edge)
  uint4* ovf;    // per row with 9..15 in-edges: the ring bytes of in-edges 7..14 (8 x 16 bits; -inf cells for those it does not have)
  uint2* bps;    // backpointer stream: [step / 8][lane of the window] 8 bytes = 8 steps x 2 columns x 4 bits
  u32* seq2g;    // the current layer: [0, 60) 2 bits per base, [64, 96) its band guide as eight segments (set-up kernel ->
                 // descriptor / graph update kernels)
};
__host__ __device__ inline u32 poa4_desc_rows(u32 nmax) { return nmax + 64; }
__host__ __device__ inline u32 poa4_steps(u32 nmax, u32 lmax) { return nmax + nmax / 16 + lmax / 2 + 96; }
__host__ __device__ inline size_t poa4_v7_bytes(u32 nmax) { return (static_cast<size_t>(poa4_desc_rows(nmax)) * 4 + 255) & ~size_t(255); }
inline size_t poa4_slot_bytes(u32 nmax, u32 lmax) {
  size_t b = poa2_slot_bytes(nmax, lmax, 0, false);
  b += static_cast<size_t>(poa4_desc_rows(nmax)) * 32;
  b += 2 * ((static_cast<size_t>(nmax) * 4 + 255) & ~size_t(255));
  b += (static_cast<size_t>(poa4_steps(nmax, lmax)) / P4::kU + 2) * 16 * 8;
  b += poa4_v7_bytes(nmax);
  b += static_cast<size_t>(poa4_desc_rows(nmax)) * 16;
  b += 512;
  return (b + 255) & ~size_t(255);
}
__host__ __device__ inline Poa4Slot poa4_carve(unsigned char* base, u32 nmax, u32 lmax) {
  Poa4Slot s;
  s.g = poa2_carve(base, nmax, lmax, 0, false);
  size_t o = 0;
  poa2_fields(nmax, lmax, 0, [&](int, size_t x) { o += (x + 255) & ~size_t(255); }, false);
  s.desc = reinterpret_cast<uint4*>(base + o);
  o += static_cast<size_t>(poa4_desc_rows(nmax)) * 32;
  s.rb = reinterpret_cast<u32*>(base + o);
  o += (static_cast<size_t>(nmax) * 4 + 255) & ~size_t(255);
  s.rbl = reinterpret_cast<u32*>(base + o);
  o += (static_cast<size_t>(nmax) * 4 + 255) & ~size_t(255);
  s.bps = reinterpret_cast<uint2*>(base + o);
  o += (static_cast<size_t>(poa4_steps(nmax, lmax)) / P4::kU + 2) * 16 * 8;
  s.v7 = reinterpret_cast<u32*>(base + o);
  o += poa4_v7_bytes(nmax);
  s.ovf = reinterpret_cast<uint4*>(base + o);  // (right behind v7: the NW's rare path derives it from that pointer)
  o += static_cast<size_t>(poa4_desc_rows(nmax)) * 16;
  s.seq2g = reinterpret_cast<u32*>(base + o);
  return s;
}

// ---- the phases of a window's layer -------------------------------------------------------------------------------------
// What a window carries from phase to phase lives in an 80-byte record beside its graph (Poa4Win); a phase function reads
// it, does its part for one window (graph side) or for the wave's four (alignment side) and lane 0 stores the new state.
enum : u32 { kIdle = 0, kRunning = 1, kLayersDone = 2, kFinal = 3, kFailed = 4, kHandedOn = 5 };  // (kHandedOn: queued for the 64-column attempt of this launch — whoever runs it writes the window's result)

struct Poa4Win {  // per window in flight (four per resident wave)
  u32 wi;        // window index
  u32 phase, status, nn, n_eff, li, flip;
  u32 act, full, len, lb, span;  // the layer of this round (act = 0: none)
  u32 r_lo, n_rows, t_end, best_rho1;
  u32 b_first;   // band start of the layer's first row
  u32 dflag;     // != 0: the descriptor pass found the layer beyond this kernel's limits
  u32 cells_full, cells_band;  // work counters: rows of the layers' subgraphs x layer length / x band width
};
static_assert(sizeof(Poa4Win) == 80, "state record");

struct Poa4Ctx {  // what a phase function needs beside the batch description
  Poa4Win* st;     // state records, four per resident wave
  u32 first;       // position of the batch's first window in scheduling order
  u32 count;       // windows of the batch
  u32 quad_delta;  // (group of four windows the wave is working on) - (the wave's own index), modulo 2^32: the wave's records
                   // and scratch slots are its own, the windows are those of the group (0 when the emulator steps the
                   // phases wave by wave in lock step)
  u32 gw;          // windows per group, 1 .. 4 (0 = 4): a batch that does not fill the machine's wave slots with groups of
                   // four is dealt out in smaller groups (round 6) — a wave's layer then has fewer graph sides in front of
                   // its NW, and the latency of a group is what a small batch costs.  The wave's other slots stay empty.
};
__host__ __device__ __forceinline__ u32 poa4_group_windows(const Poa4Ctx& C) { return C.gw ? C.gw : static_cast<u32>(P4::G); }

__host__ __device__ __forceinline__ unsigned char* poa4_slot_of(const Poa4Args& A, const Poa4Ctx&, u32 wave, int q) {
  return A.scratch + (static_cast<size_t>(wave) * P4::G + static_cast<size_t>(q)) * A.slot_bytes;
}
// the lane's window of this wave: record index, or 0xFFFFFFFF beyond the batch
__host__ __device__ __forceinline__ u32 poa4_my_record(const Poa4Ctx& C, u32 wave, int q) {
  const u32 gw = poa4_group_windows(C);
  const u32 pos = (wave + C.quad_delta) * gw + static_cast<u32>(q);  // position within the batch
  return (static_cast<u32>(q) < gw && pos < C.count) ? wave * P4::G + static_cast<u32>(q) : 0xFFFFFFFFu;
}
__host__ __device__ __forceinline__ u32 poa4_position(const Poa4Ctx& C, u32 wave, int q) {
  return C.first + (wave + C.quad_delta) * poa4_group_windows(C) + static_cast<u32>(q);
}
}  // namespace
}  // namespace rvn
