// engine.h — internal structures of the MI355X overlap engine (not part of the public C ABI).
#pragma once

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"

namespace rvn {

constexpr int kSketchTile = 1024;  // k-mer positions per sketch workgroup
constexpr int kMaxWindow = 256;    // largest supported winnowing window w

// Device-resident read set: concatenated 2-bit packed words (every read starts on a word
// boundary, one pad word at the end), per-read word offsets / lengths / ids.
inline u64 next_reads_serial() {
  static std::atomic<u64> counter{0};
  return ++counter;
}

// A struct that owns device buffers names them ONCE, in for_each_buf directly under their declarations; its release()
// hands them back through that and resets every descriptor that speaks about their contents.  The engine's
// scratch-release path and the byte count of its tests are loops over these, never a list of their own.
using BufFn = std::function<void(DevBuf&)>;
template <typename G>
void release_bufs(G& g) {
  g.for_each_buf([](DevBuf& b) { b.release(); });
}

struct ReadsDev {
  u32 n = 0;
  u64 total_bases = 0;
  u64 n_words = 0;
  DevBuf packed;    // u64[n_words + 1]
  DevBuf word_off;  // u64[n + 1]
  DevBuf len;       // u32[n]
  DevBuf id;        // u32[n]
  std::vector<u64> h_word_off;
  std::vector<u32> h_len, h_id;
  // qualities attached to the read set (rvn_reads_attach_quality): Phred+33, one byte per 2^qual_shift bases,
  // read i at qual_off[i]; used by the polishing rounds when the caller passes none
  DevBuf quals, qual_off;
  std::vector<u64> h_qual_off;
  int qual_shift = -1;  // -1: none attached
  u64 serial = next_reads_serial();  // unique per read set of the process (what a cache of derived data is keyed by)
  bool ids_are_indices = false;  // ids[i] == i and all < 2^31 (needed by the pass-1 merge and the self-join)
  // sketch tiles for the owning engine's (k, w)
  u32 n_tiles = 0;
  DevBuf tile_read;      // u32[n_tiles]  read index of the tile
  DevBuf tile_start;     // u32[n_tiles]  first k-mer position of the tile
  DevBuf read_tile_off;  // u32[n + 1]
  std::vector<u32> h_read_tile_off;
};

// Sketch of a read range: minimizers in (read, position) order.
struct Sketch {
  u32 first = 0, last = 0;
  u64 count = 0;
  DevBuf val;       // V[count]   (u32 when 2k < 32, else u64)
  DevBuf org;       // u64[count] id << 32 | pos << 1 | strand
  DevBuf read_off;  // u32[last - first + 1]
  void for_each_buf(const BufFn& f) { f(val), f(org), f(read_off); }
};

struct Index {
  u64 m = 0;  // minimizers in the index
  u64 u = 0;  // distinct keys
  int table_bits = 0;
  int shift = 0;
  DevBuf s_val[2];  // sorted values (ping-pong)
  DevBuf s_org[2];  // sorted origins
  int cur = 0;
  DevBuf u_val;    // V[u]
  DevBuf u_start;  // u32[u + 1]
  DevBuf table;    // u32[2^table_bits + 1]
  DevBuf direct;   // u64[4^k]: (count << 32) | first entry of value v's run, 0 = v is not in the index — a probe is ONE
                   // cache line instead of table -> search in u_val -> u_start (built for 2k <= 30 bits and large indexes only)
  bool direct_built = false;
  u32 occurrence = 0xFFFFFFFFu;
  bool table_built = false;      // u_val / table are built lazily (only the probe path needs them)
  bool has_query_flags = false;  // origins carry kQueryFlag
  bool all_query = false;        // every index entry is a query minimizer (index built with minhash)
  u32 first = 0, last = 0;       // read range the index was built from
  void for_each_buf(const BufFn& f) {
    f(s_val[0]), f(s_val[1]), f(s_org[0]), f(s_org[1]), f(u_val), f(u_start), f(table), f(direct);
  }
};

struct MapOut {
  u32 first = 0, last = 0;
  u64 n_query = 0;    // M_q
  u64 n_matches = 0;  // H
  u64 n_intervals = 0;
  u64 n_overlaps = 0;  // O
  DevBuf ovl;          // Overlap[n_overlaps] in (query read, emission) order
  DevBuf ovl_read_off; // u32[last - first + 1]
  DevBuf filtered;     // u8[n_query] (1 = skipped by the occurrence filter); valid when requested
  // chain anchors of every overlap (lhs_pos << 32 | rhs_pos, ascending along the chain); when requested
  bool has_anchors = false;
  DevBuf anchors;      // u64[n_matches] (sparse: regions of the emitting intervals)
  DevBuf anchor_off;   // u64[n_overlaps] index of an overlap's first anchor in `anchors`
  DevBuf anchor_cnt;   // u32[n_overlaps]
  void for_each_buf(const BufFn& f) { f(ovl), f(ovl_read_off), f(filtered), f(anchors), f(anchor_off), f(anchor_cnt); }
};

struct StageTimes {
  // accumulated device milliseconds per stage (HIP events on the engine stream)
  enum { kSketch, kSort, kIndex, kFilter, kQuery, kMatch, kSegSort, kIntervals, kChain, kCompact, kMerge, kPile,
         kTruncate, kNum };
  double ms[kNum] = {};
  u64 launches[kNum] = {};
};

struct PileState;
struct PileRegion;  // overlap_rules.h
struct ResolveState;

// Tuning a deployment may set (rvn_engine_set_option; 0 = the built-in default everywhere).  None of them changes a result.
struct EngineOptions {
  long long nw_budget_mb = 0;        // alignment-path stage: HBM for the stored band words (default: a quarter of the free memory, <= 64 GB)
  long long nw_group_walk = 0;       // alignment-path stage: 1 = every walk one lane per alignment, 2 = every walk a group of lanes per
                                     // alignment (nwtrace.h), 3 = one lane per alignment with strips of sixteen kept columns, otherwise
                                     // by the number of alignments in the launch.  Same records either way
  long long nw_stripe_lanes = 0;     // alignment-path stage: lanes of the widest ring of one sweep (1 .. 64, default 64 = a wave); a band
                                     // wider than that is swept in stripes of that many super-blocks (nwpath.h).  Same records either way
  long long ed_wide_lanes = 0;       // path similarity: lanes of the workgroup ring that sweeps thresholds beyond the wave ring (64 .. 512 in
                                     // steps of 64, default 512); 1 = no such sweep, those pairs are the full sweep's.  Same distances either way
  long long edge_slices_budget_kb = 0;  // edge similarity: HBM for the packed slices of one chunk of the edges whose nodes are tilings of several
                                     // segments (default: a quarter of the largest free block the arena, or the driver, reports).  Same values either way
  long long index_direct_min_keys = 0;  // index: distinct values from which every possible value is addressed directly (index.hip; default 8 M,
                                     // 1 = every index with 2k <= 30 bits — the tests of that path on small inputs).  Same matches either way
  long long poa_rows_min_windows = -1;  // window-consensus stage: smallest batch that starts with the rows-on-lanes kernel (poa4.hip);
                                        // a smaller one starts with the 64-column kernel (poa2.hip).  < 0: the default, kPoaRowsMinWindowsDefault = 8 192
  long long io_threads = 0;          // rvn_reads_load: inflate threads (default min(32, cores - 2))
  long long io_slab_mb = 0;          // ... page-locked slab size (default 8)
  long long io_ring = 0;             // ... slabs in flight (default 8)
  long long io_zlib = 0;             // ... != 0: zlib instead of inflate_fast.h on a single gzip member
  long long arena_mb = 0;            // device arena (common.h: devpool): its size when it starts (default: free memory - margin)
  long long arena_margin_mb = 0;     // ... memory left to the driver (default max(12 GB, 1/16 of the device))
  long long no_arena = 0;            // ... != 0: never start one
  long long release_always = 0;      // != 0: every stage entry hands the scratch back (the tests of that path)
  long long polish_join = 0;         // != 0: a polishing round maps by sorting the reads' minimizers with the targets' and streaming
                                     // the runs instead of probing the targets' index (round 6: built, bit-identical, slower — DESIGN.md 3.7)
  long long polish_sketch_cache_mb = -1;  // HBM for the reads' sketch kept between polishing rounds (< 0: an eighth of the device; 0: none)
};
const char* engine_option_names();   // comma-separated, for the error message
long long* engine_option(EngineOptions& o, const char* name);

struct Engine;

// Scratch every stage may use between two of its own launches; nothing in it outlives the call that filled it
struct SharedScratch {
  DevBuf tmp_a, tmp_b, tmp_c, tmp_d, tmp_e, tmp_f, scan_tmp, sort_tmp;
  void for_each_buf(const BufFn& f) {
    f(tmp_a), f(tmp_b), f(tmp_c), f(tmp_d), f(tmp_e), f(tmp_f), f(scan_tmp), f(sort_tmp);
  }
  void release() { release_bufs(*this); }
};

// input path (io.hip)
struct IoState {
  DevBuf text[2];  // the file's text in HBM
  std::vector<std::pair<std::unique_ptr<PinBuf>, bool>> pin;  // its page-locked slabs (buffer, handed out): host memory, kept
  void for_each_buf(const BufFn& f) { f(text[0]), f(text[1]); }
  void release() { release_bufs(*this); }
};
struct LoadStats {
  u64 n_sequences = 0, n_bases = 0;
  int has_quality = 0;
  double parse_s = 0, device_s = 0, total_s = 0;  // record scanner | copies + packing on the device (caller thread) | whole call
  u32 inflate_threads = 0, members = 0;           // the inflate pool and what it found in the archive
  int streaming = 0, restarted = 0;               // one stream front to back | a wrong member cut made the load start over
};
void reads_load(Engine& e, const std::string& path, ReadsDev& R, std::vector<std::string>& names, LoadStats& st);

// ---- stages (one translation unit each) -------------------------------------
// sketches and the index (sketch.hip, index.hip; abi_shard.hip for the sharded pass)
struct SketchState {
  Index index;
  Sketch index_sketch, query_sketch, raw_sketch;
  struct QueryReady {  // query_sketch was prepared ahead of map_batch, for exactly this range / minhash flag
    bool valid = false;
    u32 first = 0, last = 0;
    bool minhash = false;
  } query_ready;
  u64 join_query_count = 0;           // number of query minimizers flagged in the index (self-join path)
  bool shard_sketch_minhash = false;  // which sketch rvn_shard_sketch left its result in
  DevBuf foreign_val, foreign_org;    // a query-only sketch appended from its pieces (rvn_shard_sketch_range)
  DevBuf sum;  // 64-bit total of a sketch whose 32-bit offsets could wrap (sketch.hip)
  void for_each_buf(const BufFn& f) {
    index.for_each_buf(f), index_sketch.for_each_buf(f), query_sketch.for_each_buf(f), raw_sketch.for_each_buf(f);
    f(foreign_val), f(foreign_org), f(sum);
  }
  void release() {
    release_bufs(*this);
    index.m = index.u = 0;
    index.table_built = index.direct_built = false;
    index_sketch.count = query_sketch.count = raw_sketch.count = join_query_count = 0;
    query_ready = {};
  }
};
// Map (map.hip, chain.hip): the last result and the scratch of the match / chain stages
struct MapState {
  MapOut out;
  DevBuf q_start, q_cnt, m_off;
  DevBuf m_grp[2], m_pos[2];
  // room for H matches (group and position words): side [0] holds them, side [1] is the chain stage's ping-pong
  void reserve_matches(u64 H) {
    m_grp[0].reserve((H + 1) * 8), m_pos[0].reserve((H + 1) * 8);
    m_grp[1].reserve((H + 1) * 8), m_pos[1].reserve((H + 1) * 8);
  }
  DevBuf seg_off, iv_slot_begin, iv_slot_end, iv_cnt, iv_off, iv_begin, iv_end;
  DevBuf lis_min, lis_pred, lis_tail, lis_mask, ovl_slots, ovl_flags, ovl_scan, chain_big;
  DevBuf anc_slot_off, anc_slot_cnt;
  bool keep_anchors = false;  // map_batch also returns the chain anchors of every overlap
  u32 shard_join_reads = 0;   // rvn_shard_join: segments of the last join (in seg_off / m_grp[0] / m_pos[0])
  u64 shard_join_matches = 0;
  void for_each_buf(const BufFn& f) {
    out.for_each_buf(f);
    f(q_start), f(q_cnt), f(m_off), f(m_grp[0]), f(m_grp[1]), f(m_pos[0]), f(m_pos[1]);
    f(seg_off), f(iv_slot_begin), f(iv_slot_end), f(iv_cnt), f(iv_off), f(iv_begin), f(iv_end);
    f(lis_min), f(lis_pred), f(lis_tail), f(lis_mask), f(ovl_slots), f(ovl_flags), f(ovl_scan), f(chain_big);
    f(anc_slot_off), f(anc_slot_cnt);
  }
  void release() {
    release_bufs(*this);
    out.first = out.last = 0;
    out.n_query = out.n_matches = out.n_intervals = out.n_overlaps = 0;
    out.has_anchors = false;
    shard_join_reads = 0;
    shard_join_matches = 0;
  }
};
void reads_build_tiles(Engine& e, ReadsDev& r);
// 2-bit packing of one-byte codes already in HBM: read i = codes[base_off[i] ..), words at word_off[i] (sketch.hip)
void pack_codes_on_device(Engine& e, const u8* d_codes, const u64* d_base_off, const u64* d_word_off, u32 n_reads,
                          u64 n_words, u64* d_packed);
void sketch_raw(Engine& e, const ReadsDev& r, u32 first, u32 last, Sketch& out);
void sketch_minhash(Engine& e, const ReadsDev& r, const Sketch& raw, Sketch& out);
void sketch_range(Engine& e, const ReadsDev& r, u32 first, u32 last, bool minhash, Sketch& out);
void index_build(Engine& e, Sketch& sk, bool build_table = true);  // consumes sk.val/sk.org
void index_build_table(Engine& e);                               // lazy: distinct keys + direct-address table
// minhash-select on a raw sketch, marking the selected minimizers with kQueryFlag in raw.org; returns their count
u64 sketch_flag_queries(Engine& e, const ReadsDev& r, Sketch& raw);
void index_filter(Engine& e, double freq);               // sets e.sketch.index.occurrence
void index_key_histogram(Engine& e, std::vector<u64>& hist, std::vector<u32>& over);  // count-of-counts (65536 bins)
void map_batch(Engine& e, const ReadsDev& r, u32 first, u32 last, bool avoid_equal, bool avoid_symmetric,
               bool minhash, bool want_filtered, MapOut& out);
// Map() of reads whose own minimizers sit in the index as query-only entries: the polishing round's mapping (map.hip)
void map_batch_query_only(Engine& e, const ReadsDev& r, u32 first, u32 last, u64 n_query, MapOut& out);
// self-join of the index for global query ids 0..n_reads-1 -> e.map.m_grp[0] / e.map.m_pos[0] / e.map.seg_off (map.hip)
u64 join_index_matches(Engine& e, u32 n_reads, bool avoid_equal, bool avoid_symmetric, u32 q_lo = 0,
                       u32 q_hi = 0xFFFFFFFFu);  // only query reads with q_lo <= id < q_hi
// the probe branch of the match stage on a query sketch of nr reads -> the same three buffers; returns the matches (map.hip)
u64 match_probe(Engine& e, const Sketch& qs, u32 nr, bool avoid_equal, bool avoid_symmetric, u8* filt, u64* seg_off);
// chain stage of Map on matches already in e.map.m_grp[0] / e.map.m_pos[0] / e.map.seg_off (chain.hip)
void chain_matches(Engine& e, const ReadsDev& r, u32 first, u32 last, u64 H, MapOut& out);
// its kernels' opt-in to more than 64 KB of dynamic LDS on the current device: once per engine, where it is created
void chain_allow_big_lds();

struct EditDistanceState {
  DevBuf cnt, sort, todo;
  void for_each_buf(const BufFn& f) { f(cnt), f(sort), f(todo); }
  void release() { release_bufs(*this); }
};
// Batched exact edit distance (edit_distance.hip). h_pairs: n_pairs x {a_idx,a_begin,a_len,b_idx,b_begin,b_len,strand,0}
void edit_distance_batch(Engine& e, const ReadsDev& r, const u32* h_pairs, u32 n_pairs, u32* h_out, double* kernel_ms,
                         u64* cells);
// the same with pairs and distances resident in HBM (pass2.hip: identity filters)
// wide_sweep: the pairs' thresholds lie beyond the wave ring; they go straight to the ring over a workgroup's lanes and
// from there to the full sweep (path_similarity_batch alone asks for it, for that part of its pairs)
// wide_after: what the wave ring's doubling sweeps leave as overflow goes to the workgroup ring in one sweep at its capacity
// before the full sweep takes the rest (graph_edge_similarity alone asks for it: unbounded distances beyond 8 064)
void edit_distance_dev(Engine& e, const ReadsDev& r, const u32* d_pairs, u32 n_pairs, u32* d_out, const u32* d_kmax = nullptr,
                       bool wide_sweep = false, bool wide_after = false);

// window consensus (poa.hip): scratch of a batch, which kernels run (tests), and what the last batch / all batches did
struct PoaState {
  DevBuf scratch, scratch2;
  DevBuf sched, redo_w, redo_i;  // LPT order / escalation lists of a POA batch (poa_run_dev)
  int mode = 0;  // 0 banded 32 (poa4.hip) -> 64 -> 128 -> 256 (poa2.hip) -> full matrix; 1 full matrix only; 2 / 3 / 4 band 64 / 128 / 256 only (tests); 9 poa4.hip only (band 32, rows on lanes)
  u32 fallback_windows = 0;    // windows of the last batch that needed more than the 128-column band
  u32 fullmatrix_windows = 0;  // ... of which re-run by the full-matrix kernel
  u32 wide_windows = 0;        // windows of the last batch re-run with the 128-column band
  u32 narrow_windows = 0;      // windows of the 32-column first attempt (poa4.hip) re-run with the 64-column band
  unsigned long long phase_cycles[8] = {};  // subgraph, dp, traceback, add, order, consensus (last call); [6], [7]: DP cells
  // DP cells of the banded POA kernel since the last reset_stats: full-matrix equivalent (graph rows x layer length of
  // every layer alignment: what spoa computes) / inside the computed band; number of batches
  u64 cells_full = 0, cells_band = 0, calls = 0;
  void for_each_buf(const BufFn& f) { f(scratch), f(scratch2), f(sched), f(redo_w), f(redo_i); }
  void release() { release_bufs(*this); }
};
// Batched POA window consensus (poa.hip); all arrays are host pointers, see rvn_poa_consensus_batch
void poa_consensus_batch(Engine& e, const u8* h_codes, const u8* h_quals, const u64* h_layer_off, const u32* h_begins,
                         const u32* h_ends, const u32* h_has_qual, const u32* h_win_off, u32 n_windows, int m, int n,
                         int g, int trim, u8* h_out, const u64* h_out_off, u32* h_out_len, u32* h_status,
                         double* device_ms);

// poa4.hip's phase functions stepped through on the host (wavefront emulator): see rvn_poa_banded_emulate
void poa_banded_emulate(const u8* h_codes, const u8* h_quals, const u64* h_layer_off, const u32* h_begins,
                        const u32* h_ends, const u32* h_has_qual, const u32* h_win_off, u32 n_windows, int m, int n, int g,
                        int trim, u8* h_out, const u64* h_out_off, u32* h_out_len, u32* h_status, int variant);

struct PolishStats {
  u64 n_overlaps = 0, n_reads_used = 0, n_layers = 0, n_windows = 0, n_polished_windows = 0, n_failed_windows = 0;
  u64 n_dropped_layers = 0;  // reads whose alignment is beyond the path stage (band > 262 144 rows, or above the HBM budget): not used
  double poa_ms = 0;                            // device time of the POA batch
  double map_ms = 0, host_ms = 0, total_ms = 0;  // wall: index + map | host planning (jobs, window tables) | all
  double align_ms = 0;                           // device time of the alignment-path stage (forward + traceback)
  u64 n_aligned = 0, n_align_retries = 0, align_band_cells = 0, align_store_bytes = 0;
};

// alignment-path stage (nwpath.hip)
struct NwStats {
  u64 n_aligned = 0, n_retries = 0, n_unaligned = 0, n_batches = 0;
  u64 band_cells = 0, sum_distance = 0, store_bytes = 0;
  double ms = 0;
};
struct NwState {
  struct Set {
    DevBuf hs, ck;  // stored band words (horizontal-delta streams), checkpoints
  } sets[4];        // a sweep fills one while the walks of the others run
  DevBuf strip, jobs, res;
  double rate = -1.0;  // running estimate of edit distance / length of the read-to-target alignments (< 0: unknown); learned,
                       // not a description of a buffer: it survives release()
  NwStats last;        // what the last call of nw_breakpoints counted (read by the test hooks only)
  // created together on the first use (open), destroyed with the engine
  hipStream_t streams[5] = {};  // [0..3] walk streams (beside the sweeps), one per buffer set; [4] uploads of a pass planned while another one sweeps
  hipEvent_t ev[5] = {};        // [0..3] the walk of a buffer set is done, [4] sweep -> walk
  hipStream_t side[3] = {};     // sweep launches of few waves (the pilot's, the several-blocks-per-lane variants of the longest alignments) beside the main stream's
  hipEvent_t side_ev[4] = {};   // [0..2] the side stream's sweeps are done, [3] main -> side
  void for_each_buf(const BufFn& f) {
    for (Set& s : sets) f(s.hs), f(s.ck);
    f(strip), f(jobs), f(res);
  }
  void release() { release_bufs(*this); }
  void open();   // all streams and events, or none and the error
  void close();
  ~NwState() { close(); }
};
struct NwJob;
struct NwWindowRec;
// the path form's slots (nwpath.hip): the blocks the walks wrote their runs into, per job where its runs end
struct NwPathSlots {
  std::vector<std::unique_ptr<DevBuf>> blocks;
  std::vector<u64> slot_end;  // device address of the word behind the job's runs (it holds their number); 0: not walked
};
// distances (optional): per job the exact distance, ~0 for a job that was not aligned
void nw_breakpoints(Engine& e, const ReadsDev& T, const ReadsDev& R, std::vector<NwJob>& jobs, u32 w, NwWindowRec* d_recs,
                    u64 n_recs, NwStats& st, std::vector<u32>* distances = nullptr, NwPathSlots* path = nullptr);
// The alignment paths of a batch of pairs (rvn_align_path_batch): jobs as polishing builds them (rows = target span,
// columns = query span in the target's orientation; empty spans allowed), results on the device in pair order.
struct NwPaths {
  u32 n = 0, n_not_aligned = 0;
  u64 n_runs = 0, n_ops = 0;
  std::vector<u32> distances;      // exact edit distance; ~0: not aligned
  DevBuf run_off, runs, op_off;    // u64[n + 1], u32[n_runs] (count << 2 | op, alignment order), u64[n + 1]
  double device_ms = 0;
};
void nw_align_paths(Engine& e, const ReadsDev& T, const ReadsDev& Q, std::vector<NwJob>& jobs, NwPaths& out);
// runs -> one byte per op (edlib's alignment array) into d_ops[n_ops]
void nw_paths_expand(Engine& e, const NwPaths& p, u8* d_ops);
// the same code stepped on the CPU (64 emulated lanes): test hook, see rvn_test_nw_breakpoints
int nw_breakpoints_host(const u64* t_words, u32 t_len, const u64* r_words, u32 r_len, u32 t_begin, u32 n, u32 q_begin, u32 m,
                        int rc, u32 w, u32 k, int force_R, NwWindowRec* recs, u32* distance, u32* band);
// shard.hip — partition / regroup steps of the sharded pass, all pointers device pointers unless noted
struct ShardState {
  DevBuf hist, off, ptrs;  // tile histograms / offsets / pointer tables of the partition steps
  void for_each_buf(const BufFn& f) { f(hist), f(off), f(ptrs); }
  void release() { release_bufs(*this); }
};
void shard_split_minimizers(Engine& e, const u64* d_val, const u64* d_org, u64 n, u32 world, u64* d_val_out, u64* d_org_out,
                            u64* counts /* host [world] */);
void shard_split_overlaps(Engine& e, const Overlap* d_ovl, u64 n, const u32* bounds /* host [world + 1] */, u32 world, u32 self,
                          Overlap* d_out, u64* counts /* host [world + 1], [world] = overlaps that stay */);
u64 shard_count_flagged(Engine& e, const u64* d_org, u64 n);
void shard_adjacent_diff(Engine& e, const u64* d_seg, u64 n, u64* d_cnt);
void shard_regroup(Engine& e, u32 world, const u64* const* d_cnt, const u64* const* d_grp, const u64* const* d_pos,
                   const u64* n_src /* host */, u32 n_reads, u64* d_seg, u64* d_grp_out, u64* d_pos_out);
void shard_lhs_offsets(Engine& e, const Overlap* d_ovl, u64 n, u32 n_reads, u32* d_off);
// One racon polishing round (polish.hip): targets T, reads R, optional per-base Phred+33 qualities of the reads
// polish_round's consensus straight into the caller's buffer (target t at out + off[t], at most off[t + 1] - off[t] bytes;
// len[t] = its length) instead of into `polished` (which then stays empty): one pass over the 100 MB of a C4 round less
struct PolishDirectOut {
  u8* out;
  const u64* off;
  u64* len;
};
// What a polishing round keeps in the engine (polish.hip; read by abi_polish.hip and abi_reads.hip)
struct PolishState {
  // front end: best overlaps, window records, layer tables, consensus
  DevBuf best, best_t, idmap, recs, keep, win_cnt, win_off, win_fill, win_meta, first_window, keys, lays_tmp, lays, wins, out,
      len, status, ok, cons_off, stitched, quals, qual_off, misc;
  DevBuf tval, torg;  // the targets' minimizers of the round, appended to every read batch's
  // the reads' sketch of a round's mapping, kept for the next round (the reads do not change between rounds; only the
  // targets do): per read batch, for ONE read set at a time (sketch_owner = ReadsDev::serial)
  struct KeptSketch {
    u32 first = 0, last = 0;
    Sketch sk;
  };
  u64 sketch_owner = 0;
  std::vector<std::unique_ptr<KeptSketch>> sketches;
  // The two results a round leaves resident.  polish_round empties a record BEFORE the first write to its buffers and
  // fills it when they are complete: a round that fails in between leaves no record, never the last one over new bytes.
  struct LastLayers {  // the layer table in wins / lays / ok (rvn_polish_fetch_layers)
    u32 windows = 0;
    u64 layers = 0, w0 = 0;
    bool has_ok = false;
    std::vector<u64> read_off;
  } last_layers;
  struct LastConsensus {  // the stitched consensus of a round over every window: target t at stitched + off[t]
    std::vector<u64> off;  // (rvn_polish_output_as_reads: the next round's targets without the way over the host)
    bool valid = false;
  } last_cons;
  std::vector<u32> target_reads;  // reads used per target in the last round
  // best-overlap table for the NEXT round (rvn_polish_set_best; consumed by that round)
  std::vector<Overlap> given_best;
  std::vector<u32> given_best_t;
  bool given_valid = false;
  void for_each_buf(const BufFn& f) {
    f(best), f(best_t), f(idmap), f(recs), f(keep), f(win_cnt), f(win_off), f(win_fill), f(win_meta), f(first_window), f(keys);
    f(lays_tmp), f(lays), f(wins), f(out), f(len), f(status), f(ok), f(cons_off), f(stitched), f(quals), f(qual_off), f(misc);
    f(tval), f(torg);
    for (auto& c : sketches) c->sk.for_each_buf(f);
  }
  void release() {
    release_bufs(*this);
    sketches.clear();  // (derived data, recomputed when needed)
    sketch_owner = 0;
    last_layers = {};
    last_cons = {};
  }
};
void polish_map_best(Engine& e, ReadsDev& T, ReadsDev& R, u32 r_first, u32 r_last, double err_thr,
                     std::vector<Overlap>& best, std::vector<u32>& best_t, u64* n_overlaps);
void polish_round(Engine& e, ReadsDev& T, ReadsDev& R, const u8* h_quals, const u64* h_qual_off, double q_thr,
                  double err_thr, u32 w, bool trim, int m, int n, int g, std::vector<std::vector<u8>>& polished,
                  std::vector<double>& ratio, PolishStats& stats, u64 win_first = 0, u64 win_last = ~0ULL,
                  std::vector<u32>* win_count = nullptr, std::vector<u32>* win_polished = nullptr,
                  const PolishDirectOut* direct = nullptr);

// scratch of the second pass / identity filters (pass2.hip)
struct Pass2Scratch {
  DevBuf slot, pairs, dist, regions, index_of, kmers_off, ok, keep, tmp_ovl;
  void for_each_buf(const BufFn& f) {
    f(slot), f(pairs), f(dist), f(regions), f(index_of), f(kmers_off), f(ok), f(keep), f(tmp_ovl);
  }
  void release() { release_bufs(*this); }
};
// Result of the second mapping pass (pass2.hip), resident in HBM
struct Pass2State {
  u32 n = 0;
  u64 n_overlaps = 0;
  DevBuf ovl;        // Overlap[n_overlaps]: overlaps.back() of construct.cc:352,451
  DevBuf contained;  // u8[n]: piles this pass marked as contained
  DevBuf kmers;      // Pile::kmers_ cells: (len >> 4) + 1 bytes per VALID read at h_kmers_off[id] (0 bytes for invalid ones)
  std::vector<u64> h_kmers_off;
  u64 kmers_total = 0;
};
// ram::MinimizerEngine::Minimize(first, last, minhash) on a read set (engine.hip).  With prefetch_query the minhash QUERY
// sketch of the same range is derived from the same raw sketch, so map_batch over that range does not sketch again.
void engine_minimize(Engine& e, const ReadsDev& r, u32 first, u32 last, bool minhash, bool prefetch_query = false);
// minimizer values of a sketch or an index to the host as u64, whatever their width on the device (engine.hip)
void fetch_values(Engine& e, const DevBuf& val, u64 n, u64* values);
void reads_subset(Engine& e, const ReadsDev& R, const std::vector<u32>& src, ReadsDev& V);
void second_pass(Engine& e, const ReadsDev& R, const u32* h_begin, const u32* h_end, const u8* h_invalid, double freq,
                 u32 kmer_len, double identity, u64 batch_bases, Pass2State& out);
// The stages of second_pass, also driven per rank by the device group (group.hip)
struct Pass2Prep {
  std::vector<u32> valid;                       // ids of the valid reads, ascending
  u32 sv = 0;                                   // valid reads that are mapped (0: every pile valid, construct.cc:343-349)
  ReadsDev V;                                   // the valid reads (ids = original ids)
  std::vector<u64> h_v_kmers_off;               // first k-mer cell of valid read i (+ the total)
  std::vector<std::pair<u32, u32>> batches;     // index batches [first, last) of the valid reads
  PileRegion* d_regions = nullptr;              // engine scratch: pile regions by id
  u32* d_index_of = nullptr;                    // engine scratch: id -> index among the valid reads
  u64* d_v_kmers_off = nullptr;
};
void second_pass_prepare(Engine& e, const ReadsDev& R, const u32* h_begin, const u32* h_end, const u8* h_invalid,
                         u64 batch_bases, Pass2State& out, Pass2Prep& P);
u64 second_pass_batch(Engine& e, Pass2Prep& P, u32 first, u32 last, u32 q_first, u32 q_last, double freq, u32 kmer_len,
                      double identity, Pass2State& out);
// its part behind Map: AddKmers, update_and_identity, classify, compaction, append (mo = Map's output for the query reads)
u64 second_pass_merge(Engine& e, Pass2Prep& P, u32 q_first, u32 q_last, const MapOut& mo, u32 kmer_len, double identity,
                      Pass2State& out);
void second_pass_finish(Engine& e, PileRegion* d_regions, Pass2State& out);
void or_bytes(Engine& e, u8* d_dst, const u8* d_src, u64 n);  // d_dst[i] |= d_src[i]
void identity_filter_lists(Engine& e, const ReadsDev& R, Overlap* h_ovl, u32* h_off, const u32* h_begin, const u32* h_end,
                           const u8* h_invalid, double identity);
// its two halves: the device part on a flat list (ok flags + updated overlaps out) and the per-pile compaction
void identity_filter_flags(Engine& e, const ReadsDev& R, const Overlap* h_ovl, u64 O, const u32* h_begin, const u32* h_end,
                           const u8* h_invalid, double identity, u8* h_ok, Overlap* h_upd);
void identity_filter_compact(Overlap* h_ovl, u32* h_off, u32 n, const u8* ok, const Overlap* upd);
// OverlapUpdate + [identity != 0: the edit-distance score] on a list in HBM, in place: ok flags out.  regions by read id,
// index_of: id -> index in r, nullptr = the ids are the indices (both unused when identity == 0, where this is
// update_kernel alone)
void update_and_identity(Engine& e, const ReadsDev& r, Overlap* d_ovl, u64 n, const PileRegion* d_regions,
                         const u32* d_index_of, double identity, u8* d_ok);

// ---- keep flags -> survivors, in order (pass2.hip).  The flags are 0 or 1 by contract: the scan sums them. ----
// slot (u32[n + 1]) = exclusive scan of keep[0..n), slot[n] = the number kept, which is read back (one stream sync).
// n == 0: no launch, nothing kept.
struct KeptSlots {
  const u32* slot;
  u64 kept;
};
KeptSlots kept_slots(Engine& e, const u8* d_keep, u64 n, DevBuf& slot);
// compact_kernel, the one scatter launch: out[slot[i]] = in[i] where keep[i]
void compact_overlaps(Engine& e, const Overlap* d_in, const u8* d_keep, const u32* d_slot, u64 n, Overlap* d_out);
// list[0..n) becomes its survivors: kept_slots, the scatter into spare, list.swap(spare).  Returns the number kept; slot
// stays valid for the caller.  No stream sync behind the scatter: spare, which now holds the old list, is regrown only
// behind the read-back of the next call, and every caller ends its stage on a sync of its own before the buffers are
// used for anything else.
u64 compact_overlap_list(Engine& e, DevBuf& list, u64 n, const u8* d_keep, DevBuf& slot, DevBuf& spare);

// Host array -> device buffer on the stream (asynchronous: the host array outlives the copy); nothing copied at count == 0
template <typename T>
T* upload(DevBuf& b, const T* h, size_t count, hipStream_t s) {
  T* d = b.get<T>(count + 16);
  if (count) RVN_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, s));
  return d;
}
// PileRegion{begin, end, invalid ? 1 : 0} of n piles into b, positions in bases (pass2.hip); synchronises the stream
PileRegion* upload_pile_regions(Engine& e, DevBuf& b, const u32* h_begin, const u32* h_end, const u8* h_invalid, u32 n);

// ResolveContainedReads / ResolveChimericSequences on the device (resolve.hip): the piles' state and the per-pile
// overlap lists in HBM between and after the two phases
struct ResolveStats {  // == rvn_resolve_stats
  u64 dropped_by_update[2] = {0, 0};  // overlaps OverlapUpdate dropped in the marking loop of phase 1 / in phase 2
  u64 dropped_by_filter = 0;          // overlaps the identity filter loop dropped (OverlapUpdate or the score)
  u64 dropped_by_containment = 0;     // type 1 / 2 overlaps of phase 1 that marked a pile
  u32 contained[2] = {0, 0};          // piles that became contained in phase 1 / phase 2
  u32 cut = 0, invalidated = 0;       // piles ClearChimericRegions cut / made invalid
};
struct ResolveState {
  u32 n = 0;
  u32 phases_done = 0;
  DevBuf begin, end, median, invalid, contained, chimeric;  // u32 cells, u32 cells, u16, u8, u8, u8 per pile
  DevBuf pr;                                                // PileRegion[n]: begin / end in bases + invalid
  DevBuf roff, rcount, regions;  // chimeric regions: slots of pile i at roff[i] (u32[n + 1]), rcount[i] of them in use
  u32 regions_total = 0;         // slots
  DevBuf ovl, off;               // Overlap[n_overlaps], u32[n + 1]
  u64 n_overlaps = 0;
  DevBuf own_cov, own_cov_off;  // the host-array form's coverage (the resident form works on PileState::pile_data)
  u16* cov = nullptr;
  const u64* cov_off = nullptr;
  u64 cov_words = 0;
  u16 global_median = 0;
  ResolveStats stats;
};

// Pass-1 state: per-pile kept overlaps + coverage (pile.hip)
struct PileState {
  u32 n = 0;
  DevBuf pile_off;   // u64[n + 1] in u16 units
  DevBuf pile_data;  // u16[total]
  u64 pile_words = 0;
  DevBuf kept_off;   // u32[n + 1]
  DevBuf kept;       // Overlap[kept_total]
  u64 kept_total = 0;
  DevBuf new_off, new_list, tmp1, tmp2, tmp3, tmp4, tmp5, tmp6;
  // TrimAndAnnotatePiles' result per pile, kept in HBM for the stages behind it (resolve.hip)
  DevBuf ann_begin, ann_end, ann_median, ann_invalid;  // u32[n] cells, u32[n] cells, u16[n], u8[n]
  bool trimmed = false;
  std::shared_ptr<ResolveState> resolve;  // what rvn_pass1_resolve left on this pass (resolve.hip)
};
void piles_init(Engine& e, const ReadsDev& r, PileState& ps);
void piles_merge(Engine& e, const ReadsDev& r, const MapOut& mo, u32 kmax, PileState& ps);
// Pile::FindValidRegion(coverage) + FindMedian on every pile, in place in HBM (pile.hip); host output arrays of n
void piles_trim_and_median(Engine& e, PileState& ps, u32 coverage, u32* h_begin, u32* h_end, u16* h_median, u8* h_invalid);
// Pile::FindChimericRegions of every valid pile on the coverage in HBM (pile.hip): CSR of (begin, end) cell pairs.
// kernel: which of the two kernels runs — kChimericByKnob = one wave per pile unless RVN_CHIMERIC_PER_THREAD is set (a
// knob(): the product library always takes the wave kernel); the other two values are for the test hook
// (rvn_test_piles_annotate), which runs both on the same piles.
enum ChimericKernel { kChimericByKnob = -1, kChimericWave = 0, kChimericPerThread = 1 };
void piles_find_chimeric_regions(Engine& e, PileState& ps, const u8* h_invalid, std::vector<u32>& h_off,
                                 std::vector<u32>& h_regions, ChimericKernel kernel = kChimericByKnob);
// the same with the flags and the result in HBM: d_roff[n + 1], regions = (begin, end) pairs; returns the number of pairs
u32 piles_find_chimeric_regions_dev(Engine& e, PileState& ps, const u8* d_invalid, DevBuf& roff, DevBuf& regions,
                                    ChimericKernel kernel = kChimericByKnob);
// Pile::AddKmers for reads [first_read, first_read + n_reads) (pile.hip)
void pile_add_kmers_batch(Engine& e, const ReadsDev& r, const u32* h_pos, const u64* h_pos_off, u32 n_reads,
                          u32 first_read, u8* h_out, const u64* h_out_off);
// Pile::AddLayers on a single pile (ps initialised for one read); h_ovl is a host array
void pile_add_layers_single(Engine& e, PileState& ps, const u32* d_ids, const Overlap* h_ovl, u32 n);

// raven::ResolveRepeatInducedOverlaps (repeats.hip): the surviving overlaps in order, the last iteration's regions of
// every pile ((first, second) pairs, flag in bit 0 of first; CSR roff[n + 1]), is_repetitive, and the loop's counts
struct RepeatResult {
  std::vector<Overlap> ovl;
  std::vector<u32> roff, reg;
  std::vector<u8> isrep;
  u32 iterations = 0, components = 0;
  u64 removed = 0;
};
void resolve_repeat_induced_overlaps(Engine& e, const Overlap* h_ovl, u64 m, u32 n, const u16* h_cov, const u64* h_cov_off,
                                     const u8* h_kmers, const u64* h_kmer_off, const u32* h_begin, const u32* h_end,
                                     const u16* h_median, const u8* h_invalid, RepeatResult& res);

// The force-directed layout of raven's RemoveLongEdges (layout.hip; arithmetic: layout.h): every component of the call
// (points [off[c], off[c + 1])) laid out for n_iterations from the given start positions; neighbours are point indices
// in the order their terms are added.  host_tree_iterations counts the (component, iteration) pairs whose repulsive
// forces came from the host's insertion-built tree, max_depth is the deepest device tree of the call.
struct LayoutStats {
  u64 host_tree_iterations = 0;
  u32 max_depth = 0;
};
void layout_force_directed(Engine& e, u32 n_components, const u32* h_off, const double* h_xy, const u64* h_adj_off,
                           const u32* h_adj, u32 n_iterations, double* h_xy_out, LayoutStats& st);

// The assembly graph as an edge table in HBM (graph.hip): ConstructAssemblyGraph (RavenLib/src/construct.cc:561-648), the
// marking of RemoveTransitiveEdges (assemble.cc:23-56) and of RemoveLongEdges' loop (assemble.cc:708-721).  Node 2i / 2i + 1
// = the i-th valid pile and its reverse complement, edge 2j / 2j + 1 = the pair of the j-th finalized overlap; an edge's
// pair is always id ^ 1.  The tables are immutable once made; the marks of the last rvn_graph_mark_transitive come on top.
struct GraphDev {
  u32 n_piles = 0, n_nodes = 0;
  u64 n_edges = 0, n_live = 0;  // slots / slots that hold an edge (tail != kNoEdge)
  bool constructed = false;     // made from overlaps: the node tables and the edge pairs' sources exist
  DevBuf seq_to_node, node_pile, node_cov;  // i32[n_piles], u32[n_nodes], u16[n_nodes]
  DevBuf tail, head, length;                // u32[n_edges]
  DevBuf edge_overlap, finalized;           // u64[n_edges / 2] index in the caller's list, Overlap[n_edges / 2]
  DevBuf off;                // u32[n_nodes + 1]: the out-edges of node v are [off[v], off[v + 1]) of both orders below
  DevBuf out_edge;           // u32[n_live] edge ids by (tail, id): the order of the reference's outedges vectors
  DevBuf hs_head, hs_edge;   // u32[n_live] heads / edge ids by (tail, head, id): the LAST of a run of equal heads is the
                             // edge `candidate[head]` ends up with (parallel edges: the largest id wins)
  bool head_order = false;   // hs_head / hs_edge exist (made by the first transitive marking)
  bool marked = false;
  std::vector<u32> order;    // the marked ids in the order the reference's marked_edges first receives them
  std::vector<u32> pairs;    // (tail & ~1, head & ~1) of the odd ids of `order`, in that order
};
struct GraphScratch {
  DevBuf ovl, spare, reg, keep, slot, invalid, median, deg, k32[2], v32[2], k64[2], v64[2], key1, key2, mark, ids, weight, flags, err;
  void for_each_buf(const BufFn& f) {
    f(ovl), f(spare), f(reg), f(keep), f(slot), f(invalid), f(median), f(deg), f(k32[0]), f(k32[1]), f(v32[0]), f(v32[1]);
    f(k64[0]), f(k64[1]), f(v64[0]), f(v64[1]), f(key1), f(key2), f(mark), f(ids), f(weight), f(flags), f(err);
  }
  void release() { release_bufs(*this); }
};
// h_* are host arrays; pile_begin / pile_end in bases.  Throws std::invalid_argument for an overlap that finalizes on an
// invalid pile and for more than 2^32 - 2 edges.
void graph_construct(Engine& e, const Overlap* h_ovl, u64 m, u32 n_piles, const u32* h_begin, const u32* h_end,
                     const u16* h_median, const u8* h_invalid, GraphDev& g);
void graph_from_edges(Engine& e, u32 n_nodes, u64 n_edges, const u32* h_tail, const u32* h_head, const u32* h_length, GraphDev& g);
u64 graph_mark_transitive(Engine& e, GraphDev& g);  // fills g.order / g.pairs, returns order.size()
u64 graph_mark_long_edges(Engine& e, const GraphDev& g, const double* h_weight, u8* h_marked);

// Node sequences as tilings (unitigs.hip; rules: unitig_rules.h): per node a list of read segments whose concatenation is
// the node's sequence.  A tiling belongs to ONE read set (reads_serial) and only ever grows: raven::CreateUnitigs appends
// the new nodes' lists, so a later call on the grown graph finds them under their ids.
struct Segment;  // unitig_rules.h
struct TilingDev {
  u32 n_nodes = 0;
  u64 n_segs = 0;
  u64 reads_serial = 0;
  DevBuf seg_off;  // u64[n_nodes + 1]
  DevBuf seg;      // Segment[n_segs]
  DevBuf cum;      // u32[n_segs]: bases of the node in front of the segment
  DevBuf len;      // u32[n_nodes]
  std::vector<u32> h_len;
};
// What raven::CreateUnitigs (RavenLib/src/common.cc:32-225) collects before its single RemoveEdges, as flat host tables:
// new node j has id first_node + j (even j: a unitig, j + 1: its reverse-complement unitig), new edge x id first_edge + x.
struct UnitigTables {
  u32 first_node = 0;
  u64 first_edge = 0;
  std::vector<u32> begin, end, count, length;
  std::vector<u16> coverage;
  std::vector<u8> is_circular, is_unitig;
  std::vector<u64> member_off;  // [new nodes + 1]
  std::vector<u32> members;     // in walk order
  std::vector<u8> marked;       // [first_edge]: marked_edges as flags
  std::vector<u32> edge_tail, edge_head, edge_length;
};
struct UnitigScratch {
  DevBuf indeg, outdeg, in_e, out_e, succ, cls, ptr[2], dist[2], endn[2], mn[2], cyc, flag, slot, cbegin, chain_of_end, chain_len;
  DevBuf count, cov, mcount, moff, members, mnode, mlen, mseg, mcnt, lenscan, segscan, cntscan, mark, err;
  DevBuf ubegin, uend, ucount, ulen, ucov, ucirc, uis, useg, ecnt, eoff, etail, ehead, elen, nodes, woff;
  DevBuf pseg, pcum, pseg_off, plen;  // the temporary tiling of tiling_paths_as_reads: one node per path
  void for_each_buf(const BufFn& f) {
    f(pseg), f(pcum), f(pseg_off), f(plen);
    f(indeg), f(outdeg), f(in_e), f(out_e), f(succ), f(cls), f(ptr[0]), f(ptr[1]), f(dist[0]), f(dist[1]), f(endn[0]), f(endn[1]);
    f(mn[0]), f(mn[1]), f(cyc), f(flag), f(slot), f(cbegin), f(chain_of_end), f(chain_len);
    f(count), f(cov), f(mcount), f(moff), f(members), f(mnode), f(mlen), f(mseg), f(mcnt), f(lenscan), f(segscan), f(cntscan), f(mark), f(err);
    f(ubegin), f(uend), f(ucount), f(ulen), f(ucov), f(ucirc), f(uis), f(useg), f(ecnt), f(eoff), f(etail), f(ehead), f(elen), f(nodes), f(woff);
  }
  void release() { release_bufs(*this); }
};
// h_* are host arrays.  Every one of these throws std::invalid_argument for what include/raven_hip.h lists as refused.
void tiling_from_piles(Engine& e, const ReadsDev& R, u32 n_nodes, const u32* h_node_pile, u32 n_piles, const u32* h_begin,
                       const u32* h_end, TilingDev& T);
void tiling_from_segments(Engine& e, const ReadsDev& R, u32 n_nodes, const u64* h_seg_off, const u32* h_read, const u32* h_begin,
                          const u32* h_length, const u8* h_strand, TilingDev& T);
void tiling_fetch(const TilingDev& T, u64* seg_off, u32* read, u32* begin, u32* length, u8* strand, u32* node_length);
// the grown tiling and the tables; nothing of T changes when the call throws
void graph_create_unitigs(Engine& e, const GraphDev& g, TilingDev& T, const u32* h_count, const u16* h_coverage, u32 epsilon,
                          u32 min_unitig_size, UnitigTables& out);
// the sequences of the listed nodes of T as a read set over the reads R the tiling was made for (read i = node h_nodes[i])
void tiling_as_reads(Engine& e, const TilingDev& T, const ReadsDev& R, const u32* h_nodes, u32 n, ReadsDev& out);
// the sequences of node paths (CSR h_off[n_paths + 1] over h_node / h_label) as a read set: per member but the last the
// first min(label, length) bases, then the whole last node (unitig_rules.h: path_member_keep).  T is not changed
void tiling_paths_as_reads(Engine& e, const TilingDev& T, const ReadsDev& R, u32 n_paths, const u64* h_off, const u32* h_node,
                           const u32* h_label, ReadsDev& out);
// RemoveBubbles' verdict on pairs (lhs, rhs) of reads of P (edit_distance.hip): h_pairs = n x 2 read indices; h_distance
// may be nullptr
void path_similarity_batch(Engine& e, const ReadsDev& P, const u32* h_pairs, u32 n_pairs, double min_ratio, u8* h_similar,
                           u32* h_distance);
// InflateData(begin[i], length[i]) of node node[i] as read i of a read set (unitig_rules.h: slice_length, slice_word)
void tiling_slices_as_reads(Engine& e, const TilingDev& T, const ReadsDev& R, u32 n, const u32* h_node, const u32* h_begin,
                            const u32* h_length, ReadsDev& out);
// its packing with everything in HBM: slices [first, first + count) of the lists, d_woff[s] = first word of slice s in a
// numbering that starts anywhere; the words of the range go to d_out[0 ..) (one lane per word, site slice_pack)
void pack_slices_dev(Engine& e, const TilingDev& T, const ReadsDev& R, const u32* d_node, const u32* d_begin, const u32* d_length,
                     const u64* d_woff, u64 first, u64 count, u64 n_words, u64* d_out);
// The edge similarity of the CSV emitters (RavenLib/src/graph_repr.cc:247-254) for every slot of an edge table
// (edge_similarity.hip): the two slices' lengths and their exact edit distance; empty slot: 0, 0, 0xFFFFFFFF.  Host arrays
// of n_edges entries, each may be nullptr.
struct EdgeSimScratch {
  DevBuf lhs, rhs, dist, direct, mat, dslot, mslot, dids, mids, pairs, ddist, snode, sbegin, slen, swords, woff, bounds, wbase;
  DevBuf cpairs, cdist;
  ReadsDev slices;  // the scratch read set of one chunk: packed words and word offsets only
  void for_each_buf(const BufFn& f) {
    f(lhs), f(rhs), f(dist), f(direct), f(mat), f(dslot), f(mslot), f(dids), f(mids), f(pairs), f(ddist), f(snode), f(sbegin), f(slen);
    f(swords), f(woff), f(bounds), f(wbase), f(cpairs), f(cdist), f(slices.packed), f(slices.word_off);
  }
  void release() { release_bufs(*this); }
};
void graph_edge_similarity(Engine& e, const GraphDev& g, const TilingDev& T, const ReadsDev& R, u32* h_lhs, u32* h_rhs, u32* h_distance);
// what every device-made read set shares once its packed words lie in r.packed (abi_reads.hip): the tables, the ids, the tiles
void reads_finish_device_set(Engine& e, ReadsDev& r, const std::vector<u64>& woff, const std::vector<u32>& lens, const uint32_t* ids,
                             u64 total_bases);

// ---- the engine: parameters, stream, and one state group per stage, each released by its owner's release() ----
struct Engine {
  EngineOptions opt;
  // Every C-ABI entry point that touches the engine's state (scratch buffers, stream, last Map result) holds this
  // lock for its whole duration: ram::MinimizerEngine::Map is const and called concurrently from Raven's pool workers
  // (RavenLib/src/construct.cc:60-64, :373-381), so the boundary has to be safe under concurrent callers.
  std::recursive_mutex mu;
  u32 k, w, bandwidth, chain, matches, gap;
  int device = 0;
  bool val64 = false;  // true when minimizer values need 64 bits
  hipStream_t stream = nullptr;
  SketchState sketch;
  MapState map;
  ShardState shard;
  EditDistanceState ed;
  Pass2Scratch p2;
  PoaState poa;
  NwState nw;
  PolishState polish;
  IoState io;
  GraphScratch graph;
  UnitigScratch unitig;
  EdgeSimScratch edge_sim;
  SharedScratch scratch;
  // every group that owns device buffers (what engine_release_scratch releases)
  template <typename F>
  void for_each_group(F&& f) {
    f(sketch), f(map), f(shard), f(ed), f(p2), f(poa), f(nw), f(polish), f(io), f(graph), f(unitig), f(edge_sim), f(scratch);
  }
  int stage_kind = 0;   // the stage entry point running (engine_release_scratch_if_tight)
  u32 oom_mask = 0;     // kinds of stages that ran out of device memory once: they start from released scratch
  StageTimes times;
  KernelTimers ktimers;
  // counters for algorithmic bytes
  u64 c_index_bases = 0, c_index_min = 0, c_index_keys = 0, c_query_bases = 0, c_query_min = 0, c_matches = 0,
      c_overlaps = 0;
  u64 c_intervals = 0;
  bool timing = true;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  u64* h_pin = nullptr;  // pinned host scratch for small device->host size read-backs
  PinBuf pin_big;        // pinned staging for bulk read-backs up to 256 MB (polishing: chain anchors)
  HostBuf host_big;      // ... and the unpinned one for larger ones
  PinBuf pin_out;        // pinned consensus buffer of the POA chunk in flight
  u64 polish_chunk_windows = 16384;  // windows per POA chunk of a polishing round (0 = everything in one batch)
  PileState* pile_pool = nullptr;  // buffers of the last destroyed pass, adopted by the next one (rvn_pass1 below)
  std::shared_ptr<int> life = std::make_shared<int>(0);  // lets handles notice that their engine is gone
};

// The per-site kernel timers of the engine count the launches of the entry point that holds one of these
struct UseTimers {
  explicit UseTimers(Engine& e) {
    e.ktimers.stream = e.stream;
    // Fold the event pairs of the previous entry point into the per-site sums now (the stream is idle between entry
    // points): the events are reused instead of growing the pool by two hipEventCreate per launch, which cost more
    // than the launches themselves on a slow host (0.5 s per pass at C4).
    if (e.ktimers.enabled && !e.ktimers.recs.empty()) {
      (void)rvn_stream_sync(e.stream);
      e.ktimers.resolve();
    }
    g_kernel_timers = &e.ktimers;
  }
  ~UseTimers() { g_kernel_timers = nullptr; }
};

// Hands every scratch / intermediate buffer of the engine back to the allocator: every group's release(), then the pile
// pool.  Buffers only ever grow, so a stage with a very different footprint (HiFi first pass -> polishing)
// can otherwise find the HBM full of the previous stage's scratch.  Only valid between stages: nothing of the
// released state may be needed afterwards (every stage entry point rebuilds what it uses).
void engine_release_scratch(Engine& e);
// ... when less than a quarter of the device memory is free (called at stage entry points)
void engine_release_scratch_if_tight(Engine& e, int stage_kind);  // kind: 0 pass 1, 1 pass 2, 2 polishing round, 3 polishing map

// Reads one 4- or 8-byte value from the device through pinned memory (stream-ordered, then synchronises).
inline u64 read_back(Engine& e, const void* dptr, size_t bytes) {
  e.h_pin[0] = 0;
  RVN_HIP(hipMemcpyAsync(e.h_pin, dptr, bytes, hipMemcpyDeviceToHost, e.stream));
  RVN_HIP(rvn_stream_sync(e.stream));
  return e.h_pin[0];
}

// Stage timing helper: records HIP events on the engine stream around a stage.
struct StageTimer {
  Engine& e;
  int stage;
  StageTimer(Engine& eng, int st) : e(eng), stage(st) {
    if (e.timing) RVN_HIP(hipEventRecord(e.ev0, e.stream));
  }
  void stop() {
    if (!e.timing) return;
    RVN_HIP(hipEventRecord(e.ev1, e.stream));
    RVN_HIP(hipEventSynchronize(e.ev1));
    float ms = 0;
    RVN_HIP(hipEventElapsedTime(&ms, e.ev0, e.ev1));
    e.times.ms[stage] += ms;
    e.times.launches[stage] += 1;
  }
};

}  // namespace rvn

// Handles of the C ABI (include/raven_hip.h) that several translation units look into
struct rvn_engine {
  rvn::Engine e;
};
struct rvn_reads {
  rvn::ReadsDev r;
  std::vector<std::string> names;  // rvn_reads_load: the sequences' names
};
// The pile buffers (coverage, kept lists, merge scratch: a dozen allocations) are recycled through the engine:
// destroying a pass hands them back, the next pass adopts them, so steady-state passes do not touch the allocator.
struct rvn_pass1 {
  rvn::Engine* e = nullptr;
  std::unique_ptr<rvn::PileState> state;
  rvn::PileState& ps;
  std::weak_ptr<int> engine_life;  // a handle may outlive its engine (e.g. interpreter teardown order)
  std::unique_ptr<rvn::ReadsDev> meta;  // sharded pass: lengths / ids of ALL reads (piles need no bases)
  explicit rvn_pass1(rvn::Engine& eng)
      : e(&eng), state(eng.pile_pool ? eng.pile_pool : new rvn::PileState()), ps(*state), engine_life(eng.life) {
    eng.pile_pool = nullptr;
  }
  ~rvn_pass1() {
    ps.resolve.reset();  // the resolved state is the pass's, not the pool's (a result handle may still share it)
    if (!engine_life.expired() && !e->pile_pool) e->pile_pool = state.release();
  }
};
struct rvn_pass2 {
  rvn::Engine* e = nullptr;
  rvn::Pass2State st;
  std::weak_ptr<int> engine_life;
};
