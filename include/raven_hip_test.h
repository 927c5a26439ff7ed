/* raven_hip_test.h — TEST INFRASTRUCTURE, not part of the product: the host-side hooks of libraven_hip_test.so.
 *
 * libraven_hip_test.so = the objects of libraven_hip.so with engine / poa / poa4 / nwpath compiled again under
 * -DRVN_TEST_HOOKS, plus the host wavefront emulator (simt_emu.hip).  It exports everything raven_hip.h declares and,
 * in addition, the entry points below, which step the __host__ __device__ building blocks of the kernels on the CPU
 * so that the CPU suite (pytest -m "not gpu") can compare them with the oracle without a GPU.  Nothing on the product
 * path calls them and libraven_hip.so does not export them (tests/test_abi.py checks both). */
#ifndef RAVEN_HIP_TEST_H_
#define RAVEN_HIP_TEST_H_

#include "raven_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rows-on-lanes banded kernel (poa4.hip) stepped through on the HOST by a 64-fibre
 * wavefront emulator — the same phase functions, no GPU and no engine needed.  Arguments as rvn_poa_consensus_batch +
 * variant (ignored: one kernel); first attempt only (status 8: the window needs a wider band).  The CPU suite
 * compares it with the oracle (tests/test_poa4_emulation.py); nothing on the product path calls it. */
int rvn_poa_banded_emulate(const uint8_t* codes, const uint8_t* quals, const uint64_t* layer_offsets,
                           const uint32_t* begins, const uint32_t* ends, const uint32_t* has_qual,
                           const uint32_t* window_offsets, uint32_t n_windows, int match, int mismatch, int gap,
                           int trim, uint8_t* consensus, const uint64_t* consensus_offsets, uint32_t* consensus_len,
                           uint32_t* status, int variant);

/* host-side test hooks for the __host__ __device__ building blocks (no GPU needed) */
uint64_t rvn_test_hash(uint64_t key, uint32_t k, int use32);
int rvn_test_canonical(const uint64_t* words, uint32_t pos, uint32_t k, int use32, uint64_t* value, uint32_t* strand);
int rvn_test_low_complexity(const uint8_t* codes, uint32_t k);
/* the alignment-path stage of a polishing round (nwpath.h) stepped on the CPU: the forward sweep's lane code driven
 * for 64 emulated lanes + the traceback, i.e. exactly what the kernels execute.  Rows = target span
 * [t_begin, t_begin + n) of a packed target, columns = span [q_begin, q_begin + m) of the read in the target's
 * orientation (rc: the read is reverse-complemented).  k = first band threshold (doubled until exact), force_r = 0
 * or the blocks per lane (1 / 2 / 4 / 8).  recs: one 32-byte record per window of w target bases touched by the span
 * {first_t, first_q, last_t, last_q, u16 grid[8]}; distance = exact edit distance; band = {k, lanes, R} used.
 * Bits 8-15 of rc: 0 = the walk of one lane per alignment (whole strips), 1 = the same with strips of sixteen kept columns (what
 * the kernel runs where the strips live in LDS); 4 / 16 / 64 = the group walk with that many lanes per alignment
 * (nwtrace.h: NwGroupWalk, its phases stepped lane by lane) — band then has a fourth entry, the batches the walk took.
 * Bits 16-23 of rc: 0 = one ring, else the striped sweep with stripes of that many lanes (1 .. 64; R = force_r, 0 = 1)
 * whatever the band — band then has five entries {k, lanes one ring would need, R, batches of a group walk, stripes};
 * a band wider than 8 such rings is refused (-3).  Bit 24 of rc: the production stage on the GPU instead (nwpath.hip
 * nw_breakpoints as a polishing round runs it, in an engine of its own on device 0; bits 16-23 = engine option
 * nw_stripe_lanes, 0 = default; k / force_r / bits 8-15 unused): band then has five entries {k, stripe lanes (0: one
 * ring), R, stripes, microseconds of the stage} of the job's final plan; -3 if the stage did not align it.
 * Returns 0, 1 if the walk did not end at cost 0, < 0 on invalid arguments. */
int rvn_test_nw_breakpoints(const uint64_t* t_words, uint32_t t_len, const uint64_t* r_words, uint32_t r_len,
                            uint32_t t_begin, uint32_t n, uint32_t q_begin, uint32_t m, int rc, uint32_t w, uint32_t k,
                            int force_r, uint32_t* recs, uint32_t* distance, uint32_t* band);
/* Pile::FindChimericRegions (slopes.h, the __host__ __device__ code the kernel runs) on one coverage array: out = (begin,
 * end) cell pairs; returns their number, -5 if a capacity was exceeded */
int64_t rvn_test_find_chimeric_regions(const uint16_t* data, uint32_t size, uint32_t* out, uint64_t cap_pairs);
/* TrimAndAnnotatePiles (pile.hip) ON THE DEVICE for a crafted coverage CSR: the hook makes an engine of its own (device 0),
 * lays out n piles of offsets[i + 1] - offsets[i] cells each (below 2^28) as a pass does, copies data[offsets[0] ..
 * offsets[n]) into them and calls what rvn_pass1_trim_and_annotate and rvn_pass1_find_chimeric_regions call — it launches
 * no kernel itself.  coverage: the threshold of Pile::FindValidRegion (<= 65535).  chimeric_mode: 0 = one wave per pile
 * (what ships), 1 = one thread per pile (otherwise behind RVN_CHIMERIC_PER_THREAD).  skip_trim != 0: the trim does not run
 * (begin / end / median / invalid are not written and may be NULL) and FindChimericRegions sees the data as given.
 * invalid_in (nullable, n flags): the piles FindChimericRegions skips; NULL = the trim's own flags, or none when the trim
 * was skipped.  Outputs: data_after (nullable) = the cells after the trim, laid out as data; begin / end (cells), median,
 * invalid = per pile, as rvn_pass1_trim_and_annotate; region_offsets[n + 1] and *regions = CSR of (begin, end) cell pairs,
 * *regions malloc'ed (rvn_free).  n == 0 or no cells at all: RVN_OK, region_offsets all 0.  RVN_EINVAL for a NULL
 * argument, another chimeric_mode, descending offsets. */
int rvn_test_piles_annotate(const uint16_t* data, const uint64_t* offsets, uint32_t n, uint32_t coverage, int chimeric_mode,
                            const uint8_t* invalid_in, int skip_trim, uint16_t* data_after, uint32_t* begin, uint32_t* end,
                            uint16_t* median, uint8_t* invalid, uint32_t* region_offsets, uint32_t** regions);
/* OverlapUpdate + GetOverlapType (overlap_rules.h, the __host__ __device__ code the kernels run) on a list: ok[i] =
 * OverlapUpdate result (the overlap is updated in place when ok), type[i] = GetOverlapType of the updated overlap */
int rvn_test_overlap_update_and_type(rvn_overlap* overlaps, uint64_t n, const uint32_t* pile_begin, const uint32_t* pile_end,
                                     const uint8_t* pile_invalid, uint32_t n_piles, uint8_t* ok, uint32_t* type);
/* The host half of rvn_reads_load (io_text.h: gzip member cut, inflate pool, FASTA / FASTQ record scanner) without a
 * device: fastq 0 / 1; threads 0 = default; force_streaming: one inflate thread front to back; slab_bytes 0 = default.
 * Outputs malloc'ed (free with rvn_free): all bases back to back, all qualities (FASTQ), lengths[n_records], names
 * separated by '\n'; info[8] = {gzip, streaming, members found, pool threads, 1 if a wrong cut made it start over,
 * microseconds of the inflate + scan loop, of which inside the scanner, 1 if the single stream went through
 * inflate_fast.h}. */
int rvn_test_parse_file(const char* path, int fastq, uint32_t threads, int force_streaming, uint64_t slab_bytes,
                        uint8_t** bases, uint8_t** quals, uint32_t** lengths, uint32_t* n_records, char** names,
                        uint32_t* info);
/* inflate_fast.h (the single-stream deflate decoder of the input path) on ONE gzip member: dst gets the text, out[4] =
 * {bytes produced, bytes of the member consumed incl. its trailer, CRC-32 and ISIZE found in the trailer}; chunk > 0:
 * through a drained buffer of that many bytes (as the input path runs it).  RVN_EINVAL + message for an invalid stream. */
int rvn_test_inflate_fast(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap, uint64_t chunk, uint64_t* out);
/* freelist.h — the offset bookkeeping of the device arena behind the engine's grow-only buffers — driven by a list of
 * operations: ops[i] > 0 allocates that many bytes (out[i] = offset, -1 if no hole holds it), ops[i] <= 0 gives back the
 * block allocated by operation -ops[i] (out[i] = 1, or 0 if it was not in use); state[3] = {bytes free, largest hole,
 * blocks in use} afterwards. */
int rvn_test_freelist(uint64_t size, uint64_t grain, const int64_t* ops, uint32_t n_ops, int64_t* out, uint64_t* state);
/* The lane-per-pair edit-distance kernel (edit_distance.hip: ed_lane_kernel<W>) stepped on the CPU: its per-pair body is
 * one __host__ __device__ function without a cross-lane operation, called here pair by pair.  packed / word_off: a packed
 * read set as rvn_reads_upload takes it (one pad word behind the last read); pairs: n x {a_idx, a_begin, a_len, b_idx,
 * b_begin, b_len, strand, 0}, strand 0 = the b span is reverse-complemented; kmax (nullable): per-pair threshold of the
 * bounded mode; W = 3, 5 or 7 slots of the window.  out[p] = the RAW value the kernel stores: the exact distance when it
 * is <= min(threshold of the window, kmax), else one of
 *   0xFFFFFFFE  the distance is above the pair's kmax (bounded mode; its value is not needed),
 *   0xFFFFFFFF  beyond the window of W = 3 or 5 slots (the widest window may still decide the pair),
 *   0xFFFFFFFD  beyond the widest window, W = 7 (the pair goes to the wave-per-pair kernel).
 * Returns 0, RVN_EINVAL for a NULL argument or another W. */
int rvn_test_ed_lane(const uint64_t* packed, const uint64_t* word_off, const uint32_t* pairs, uint32_t n,
                     const uint32_t* kmax, int W, uint32_t* out);
/* edit_distance_dev (edit_distance.hip: the function behind rvn_edit_distance_batch, the identity filters of both passes
 * and rvn_path_similarity_batch) ON THE DEVICE with pairs and thresholds taken from the host, so that a test chooses the
 * route and the threshold a product door would derive.  h / reads: an engine and an uploaded read set of THIS library.
 * pairs: n_pairs x {a_idx, a_begin, a_len, b_idx, b_begin, b_len, strand, 0}, the records of rvn_edit_distance_batch
 * (strand 0 = the b span is reverse-complemented).  kmax (nullable): per-pair thresholds as the identity filter passes
 * them; NULL = unbounded.  wide_sweep: 0 = the usual route (lane windows, wave ring, striped sweep), 1 = the workgroup
 * ring of engine option ed_wide_lanes, then the striped sweep (ed_wide_lanes = 1: the usual route after all).  The hook
 * uploads, makes ONE call of edit_distance_dev(e, r, pairs, n_pairs, out, kmax, wide_sweep != 0) and copies the values
 * back AS STORED: the exact distance, or 0xFFFFFFFE where it is above the pair's kmax — except that a pair the striped
 * sweep decided comes back exact even above its kmax (rvn_path_similarity_batch documents the exception).  It launches
 * no kernel itself.  RVN_EINVAL with a message, before anything is launched: a NULL h / reads / pairs / out, a
 * wide_sweep other than 0 / 1, and every span rvn_edit_distance_batch refuses (read index out of range, begin + len
 * beyond the read; the same check, abi.h).  n_pairs == 0: RVN_OK, nothing runs. */
int rvn_test_edit_distance_dev(rvn_engine* h, const rvn_reads* reads, const uint32_t* pairs, uint32_t n_pairs,
                               const uint32_t* kmax, int wide_sweep, uint32_t* out);
/* The probe branch of Map's match stage (map.hip: index_build_table, match_count_kernel, the scan, match_emit_kernel, the
 * gather of the segment offsets — the one function map_batch_impl calls) ON THE DEVICE with the query sketch taken from
 * the host instead of from reads.  h: an engine of THIS library whose index is built (rvn_shard_index_build or
 * rvn_engine_minimize; occurrence and the option index_direct_min_keys as set on it).  q_values (below 4^k) / q_origins
 * (id << 32 | pos << 1 | strand): the n_query minimizers of n_reads query reads in (read, position) order, read i's at
 * [q_read_off[i], q_read_off[i + 1]), q_read_off[0] = 0, q_read_off[n_reads] = n_query.  Outputs, as they are BEFORE the
 * chain stage sorts them: *group / *positions = the matches in ram's emission order (query minimizer, then run order),
 * malloc'ed (rvn_free); seg_off[n_reads + 1] = per-read offsets into them; filtered[n_query] = 1 where the occurrence
 * filter skipped the minimizer; *n_matches.  No query minimizers or an empty index: RVN_OK and no matches (Map returns
 * before the stage).  RVN_EINVAL for a NULL argument, offsets that do not ascend from 0 to n_query, a value of more than 2k
 * bits.  It launches no kernel itself. */
int rvn_test_match_probe(rvn_engine* h, const uint64_t* q_values, const uint64_t* q_origins, uint64_t n_query,
                         const uint32_t* q_read_off, uint32_t n_reads, int avoid_equal, int avoid_symmetric,
                         uint64_t** group, uint64_t** positions, uint64_t* seg_off, uint8_t* filtered,
                         uint64_t* n_matches);
/* The device-wide stable LSD radix sort (radix_sort.hip) on n host pairs, in place: variant 0 = radix_sort_pairs_u32_u64
 * (the index of k <= 15), 1 = _u64_u64 (k >= 16), 2 = _u32_u32; keys and values travel as 64-bit words whatever the variant
 * (RVN_EINVAL if one does not fit).  key_bits (0 .. 32 or 64): the sort orders by the 8-bit digits that hold bits [0, key_bits), i.e. by
 * the low ceil(key_bits / 8) bytes, and leaves the order by the bytes above alone (callers' keys have no bits there);
 * skip_constant_digits as the function's argument of that name (the index sorts with 0).  The hook makes an engine of its
 * own (device 0) for the stream and the scratch, copies, and calls the one function — it launches no kernel itself. */
int rvn_test_radix_sort_pairs(int variant, uint64_t* keys, uint64_t* values, uint64_t n, int key_bits,
                              int skip_constant_digits);
/* The device-wide exclusive prefix sum (scan.hip) of n host values: variant 0 = exclusive_scan_u32_u64, 1 = _u32_u32,
 * 2 = _u8_u32 (RVN_EINVAL if a value does not fit the input type); out[n + 1], out[n] = the total.  in_offset_items /
 * out_offset_items (<= 64): the device arrays start that many ELEMENTS behind a 256-byte boundary, so that an offset that is
 * no multiple of 16 bytes takes the kernels' element-wise path instead of their 16-byte accesses.  Engine of its own
 * (device 0), one call, no kernel launched from here. */
int rvn_test_exclusive_scan(int variant, const uint64_t* in, uint64_t n, uint32_t in_offset_items,
                            uint32_t out_offset_items, uint64_t* out);
/* compact_overlap_list (pass2.hip), the overlap phase's keep flags -> survivors in order, on n host overlaps: applied
 * with keep1[n] (flags 0 or 1), then, when keep2 is not NULL, again with keep2[kept1] on the same three buffers, so that
 * list and spare change places in both directions.  out[n] takes the survivors, *n_out their number, slot[n + 1] the scan
 * the last application left: slot[0 .. m] for its m flags, slot[m] = their sum (an application to an empty list scans
 * nothing: slot[0] = 0).  Engine of its own (device 0), no kernel launched from here. */
int rvn_test_compact_overlap_list(const rvn_overlap* in, uint64_t n, const uint8_t* keep1, const uint8_t* keep2,
                                  rvn_overlap* out, uint64_t* n_out, uint32_t* slot);
/* The scratch an engine holds: the sum of the capacities of every device buffer that rvn_engine_release_scratch hands back
 * (every buffer the engine's state groups name for release; the read sets and pass handles are not the engine's).  0 right
 * after a release.  It only reads the handle, so h may also be an engine made by libraven_hip.so of the same build. */
int rvn_test_engine_scratch_bytes(rvn_engine* h, uint64_t* bytes);
/* best_overlap_kernel (polish.hip: racon's choice of one overlap per read) ON THE DEVICE on a list given by the host, one
 * launch as a polishing round makes it for a mapped batch of n reads that starts at read `first`.  overlaps[n_overlaps]:
 * the batch's overlaps, read i's at [read_off[i], read_off[i + 1]) (read_off[n + 1], ascending, read_off[n] <= n_overlaps).
 * err_thr: a read is unused when 1 - min(span) / max(span) > err_thr, in doubles.  id_to_target[n_ids]: target index of a
 * target id (0xFFFFFFFF = none); an rhs_id >= n_ids leaves the read unused.  best / best_target: n_rows rows the caller
 * fills; the kernel writes the rows [first, first + n) (first + n <= n_rows) and the others come back as they went in.
 * n == 0: no launch.  Engine of its own (device 0).  RVN_EINVAL for a NULL argument or offsets / rows out of range. */
int rvn_test_best_overlap(const rvn_overlap* overlaps, uint64_t n_overlaps, const uint32_t* read_off, uint32_t first,
                          uint32_t n, double err_thr, const uint32_t* id_to_target, uint32_t n_ids, rvn_overlap* best,
                          uint32_t* best_target, uint32_t n_rows);
/* The second mapping pass (pass2.hip) ON THE DEVICE with Map's output of every batch taken from the host: runs
 * second_pass_prepare, then for every batch the part of second_pass_batch that follows Map (second_pass_merge: AddKmers of
 * the filtered positions, OverlapUpdate, the identity filter, type and containment flags, survivors appended), then
 * second_pass_finish — the functions the product calls; no kernel is launched from the hook.  h / reads: an engine and an
 * uploaded read set of THIS library (ids[i] == i); pile_begin / pile_end (bases, begin <= end <= length) / pile_invalid
 * as rvn_find_overlaps_and_repetitive_regions.  A batch: the query reads [q_first, q_last) counted among the VALID reads
 * (ascending id), their sketch as the kernel sees it — q_origins[n_query] (id << 32 | pos << 1 | strand; pos <= length -
 * kmer_len), q_read_off[q_last - q_first + 1] ascending from 0 to n_query, filtered[n_query] flags (0 / 1) — and Map's
 * overlaps in (query read, emission) order (ids < n).  No pile invalid, or every pile: as the product, nothing runs.
 * *out: a result for rvn_pass2_num_overlaps / _kmer_cells / _fetch / _destroy.  RVN_EINVAL for a NULL argument, ids or
 * positions out of range, offsets that do not ascend, kmer_len outside [1, 32], identity outside [0, 1]. */
typedef struct rvn_test_pass2_batch {
  uint32_t q_first, q_last;
  const uint64_t* q_origins;
  const uint32_t* q_read_off;
  const uint8_t* filtered;
  uint64_t n_query;
  const rvn_overlap* overlaps;
  uint64_t n_overlaps;
} rvn_test_pass2_batch;
int rvn_test_second_pass(rvn_engine* h, const rvn_reads* reads, const uint32_t* pile_begin, const uint32_t* pile_end,
                         const uint8_t* pile_invalid, double identity, uint32_t kmer_len,
                         const rvn_test_pass2_batch* batches, uint32_t n_batches, rvn_pass2** out);
/* rvn_align_path_batch (the same function: arguments, errors and the result handle, for rvn_paths_info / _fetch /
 * _fetch_ops / _destroy of THIS library) that also reports what the stage decided and counted.  plans[5 * n_pairs]: per
 * pair the job's final plan {k, kcap, R, G, S} (threshold of its last attempt, the largest its variant holds, blocks per
 * lane, lanes per alignment, stripe lanes or 0; all 0 for a pair that was never planned: an empty span).  stats[6]:
 * {n_aligned, n_retries, n_unaligned, n_batches, band_cells, store_bytes} of the call's NwStats.  With RVN_NW_RATE set in
 * the environment (this library reads it at every call) the thresholds come from that rate at any batch size. */
int rvn_test_align_path_batch(rvn_engine* h, const rvn_reads* queries, const rvn_reads* targets, const rvn_align_pair* pairs,
                              uint32_t n_pairs, rvn_paths** out, uint32_t* plans, uint64_t* stats);
void rvn_test_std_sort_lendesc(uint64_t* data, uint64_t n);
void rvn_test_heap_sort_lendesc(uint64_t* data, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* RAVEN_HIP_TEST_H_ */
