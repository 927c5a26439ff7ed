/* raven_hip.h — C ABI of the MI355X-native overlap-and-polish engine for Raven (libraven_hip.so).
 *
 * Drop-in boundary: the entry points below are what a binding for Raven's overlap and
 * polishing hot path would bind instead of the un-vendored ram::MinimizerEngine, edlib and racon::Polisher;
 * each cites the reference interface it replaces (paths relative to the lbcb-sci/raven tree).  Plain
 * pointers and sizes only.  Groups: engine / reads; Minimize / Filter / Map; FindOverlapsAndCreatePiles;
 * Pile::AddLayers / AddKmers; edit distance; POA window consensus; polishing round (whole, or a window range
 * for sharding); stage-level entry points of the sharded pass (host and device-pointer variants);
 * introspection and test hooks.
 *
 * Conventions
 *   - every function returning int returns RVN_OK (0) or a negative RVN_E* code; rvn_last_error()
 *     gives the thread-local message.  The C++ facade (include/ram/minimizer_engine.hpp) rethrows
 *     RVN_EINVAL as std::invalid_argument, matching ram/biosoup behaviour.
 *   - reads are handed over in biosoup::NucleicAcid layout: 2 bits per base, 32 bases per uint64_t,
 *     base i at bits (2i mod 64) of word i/32, A=0 C=1 G=2 T=3; every read starts on a word boundary
 *     (i.e. the concatenation of each read's `deflated_data`); `word_offsets` has n+1 entries.
 *   - rvn_overlap == biosoup::Overlap without the alignment string (8 x uint32_t).
 *   - the library fails loudly (RVN_ENODEVICE) when no HIP device is present; there is no CPU path.
 */
#ifndef RAVEN_HIP_H_
#define RAVEN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVN_OK 0
#define RVN_EINVAL (-1)    /* invalid argument (ram: std::invalid_argument) */
#define RVN_ENODEVICE (-2) /* no usable HIP device */
#define RVN_EHIP (-3)      /* HIP runtime / kernel failure */
#define RVN_ENOMEM (-4)

typedef struct rvn_engine rvn_engine; /* one per (device, k, w): replaces ram::MinimizerEngine */
typedef struct rvn_reads rvn_reads;   /* device-resident packed read set */
typedef struct rvn_pass1 rvn_pass1;   /* result of FindOverlapsAndCreatePiles, resident in HBM */

typedef struct rvn_overlap {
  uint32_t lhs_id, lhs_begin, lhs_end;
  uint32_t rhs_id, rhs_begin, rhs_end;
  uint32_t score;
  uint32_t strand;
} rvn_overlap;

const char* rvn_last_error(void);
int rvn_device_count(void);

/* ram::MinimizerEngine{thread_pool, k, w[, bandwidth=500, chain=4, matches=100, gap=10000]}
 * (RavenLib/src/construct.cc:661-662, RavenLib/src/assemble.cc:753).  k is clamped to [1,31] as in ram. */
int rvn_engine_create(rvn_engine** out, uint32_t k, uint32_t w, uint32_t bandwidth, uint32_t chain,
                      uint32_t matches, uint32_t gap, int device);
void rvn_engine_destroy(rvn_engine* e);

/* Copies the packed reads to HBM once; they stay resident for any number of calls
 * (the reference keeps std::vector<std::unique_ptr<biosoup::NucleicAcid>> in RAM, RavenExe/src/main.cc:258-299). */
int rvn_reads_upload(rvn_engine* e, const uint64_t* packed, uint64_t n_words, const uint64_t* word_offsets,
                     const uint32_t* lengths, const uint32_t* ids, uint32_t n_reads, rvn_reads** out);
/* Same from one-byte base codes (0..3; read i = codes[offsets[i] .. offsets[i+1])): the 2-bit packing happens on the
 * device.  This is how the consensus of one polishing round becomes the target set of the next
 * (RavenLib/src/polish.cc:50-71 rebuilds biosoup::NucleicAcid objects from the polished strings). */
int rvn_reads_upload_codes(rvn_engine* e, const uint8_t* codes, const uint64_t* offsets, const uint32_t* ids,
                           uint32_t n_reads, rvn_reads** out);

/* The consensus of the engine's last complete rvn_polish_round (every window: not a _range call over a part) as a read
 * set, straight from HBM.  Replaces, for rounds after the first, the upload of the targets raven::Polish hands the next
 * racon::Polisher (RavenLib/src/polish.cc:43-74: the polished sequences of round r are round r + 1's targets); the result
 * equals rvn_reads_upload_codes of the sequences the round returned, bit for bit.  RVN_EINVAL when no such consensus is
 * resident (no round yet, a partial round, or the engine released its scratch since). */
int rvn_polish_output_as_reads(rvn_engine* engine, rvn_reads** out);
void rvn_reads_destroy(rvn_reads* r);
/* The input path: raven::CreateParser(path) + Parse(-1) (RavenLib/src/io.cc:7-41, RavenExe/src/main.cc:258-299) straight
 * into HBM.  Format by extension exactly as io.cc (.fasta / .fa / .fastq / .fq, optionally .gz; anything else is
 * RVN_EINVAL with the reference's message).  A gzip file is cut into its members (BGZF blocks, concatenated members) and a
 * pool of host threads inflates them straight into page-locked slabs of the text (a single-member archive is one deflate
 * stream: one thread, front to back); the caller's thread finds the records with one memchr pass per slab, copies the
 * slab to HBM as it is, and the device cuts the records out and 2-bit packs them (biosoup's coder table: IUPAC folded,
 * any other character is RVN_EINVAL "not a nucleotide").  A damaged or truncated archive is RVN_EINVAL.  Read ids = 0 .. n-1 in file order.  FASTQ: biosoup's block qualities (integer mean of
 * every 64-base block) are computed on the device and attached to the read set (as rvn_reads_attach_quality with
 * block_shift 6 would).  rvn_reads_name: first word of the header of sequence i. */
typedef struct rvn_load_stats {
  uint64_t n_sequences, n_bases;
  int has_quality;
  double parse_s, device_s, total_s; /* record scanner | copies + packing on the device (caller thread) | whole call */
  uint32_t inflate_threads, members; /* the inflate pool (host threads) and the gzip members / file pieces it worked on */
  int32_t streaming, restarted; /* 1: one deflate stream, inflated front to back by one thread | 1: a member cut was wrong */
} rvn_load_stats;
int rvn_reads_load(rvn_engine* e, const char* path, rvn_reads** out, rvn_load_stats* stats);
const char* rvn_reads_name(const rvn_reads* r, uint32_t i);
int rvn_reads_info(const rvn_reads* r, uint32_t* n_reads, uint64_t* n_words, uint64_t* n_bases, uint64_t* n_quality_bytes,
                   int* quality_shift);
/* read-back of a device-resident read set (tests, callers that need the packed words on the host) */
int rvn_reads_fetch(const rvn_reads* r, uint64_t* packed, uint64_t* word_offsets, uint32_t* lengths, uint8_t* quals,
                    uint64_t* quality_offsets);
/* Base qualities of an uploaded read set, kept in HBM beside the bases for every later polishing round
 * (biosoup::NucleicAcid::block_quality; raven::Polish computes its threshold from them, polish.cc:26-41).
 * quals: Phred+33 bytes, one per 2^block_shift bases of a read (block_shift 0: per base; 6: biosoup's block qualities
 * = the mean of 64 bases + 33, which is all racon ever sees of them), read i at offsets[i] (offsets[n_reads+1]).
 * rvn_polish_round uses them when called with read_quals == NULL.  quals == NULL detaches. */
int rvn_reads_attach_quality(rvn_engine* e, rvn_reads* r, const uint8_t* quals, const uint64_t* offsets, int block_shift);

/* ram::MinimizerEngine::Minimize(first, last, minhash) — builds the index (construct.cc:42-43, :363). */
int rvn_engine_minimize(rvn_engine* e, const rvn_reads* r, uint32_t first, uint32_t last, int minhash);
/* ram::MinimizerEngine::Filter(frequency) (construct.cc:44, :372); RVN_EINVAL unless 0 <= f <= 1. */
int rvn_engine_filter(rvn_engine* e, double frequency);
uint32_t rvn_engine_occurrence(const rvn_engine* e);

/* Batched ram::MinimizerEngine::Map(sequence, avoid_equal, avoid_symmetric, minhash[, filtered])
 * for reads [first, last) (construct.cc:59-64 / :377-381).  Results stay on the device until fetched;
 * overlaps come back in (read, Map-output) order with per-read offsets (last-first+1 entries). */
int rvn_engine_map_batch(rvn_engine* e, const rvn_reads* r, uint32_t first, uint32_t last, int avoid_equal,
                         int avoid_symmetric, int minhash, int want_filtered, uint64_t* n_overlaps);
int rvn_engine_map_fetch(rvn_engine* e, rvn_overlap* overlaps, uint32_t* read_offsets);
/* positions of query minimizers skipped by the occurrence filter (`filtered` argument of Map),
 * per read: offsets (last-first+1) into `positions`.  Pass positions == NULL to query the total. */
int rvn_engine_map_fetch_filtered(rvn_engine* e, uint32_t* positions, uint32_t* read_offsets, uint64_t* total);
/* Map + fetch as ONE critical section: ram::MinimizerEngine::Map is const and Raven calls it concurrently from its
 * pool workers (construct.cc:60-64, :373-381), so a caller that cannot hold its own lock across
 * rvn_engine_map_batch / rvn_engine_map_fetch uses this.  Every entry point of this library takes the engine's lock,
 * so concurrent calls on one engine are safe; this one additionally returns the results of ITS map (not a later
 * caller's).  Outputs are malloc'ed by the library (overlaps of all reads concatenated, read_offsets[last-first+1];
 * with want_filtered also the `filtered` positions and their offsets) and released with rvn_free. */
int rvn_engine_map_collect(rvn_engine* e, const rvn_reads* r, uint32_t first, uint32_t last, int avoid_equal,
                           int avoid_symmetric, int minhash, int want_filtered, rvn_overlap** overlaps,
                           uint32_t** read_offsets, uint32_t** filtered, uint32_t** filtered_offsets);
void rvn_free(void* p);
/* Hands the engine's scratch and intermediate buffers (index, sketches, last Map result, stage scratch) back to the
 * allocator.  They only ever grow, so that steady-state calls never touch the allocator; the stage entry points
 * (first pass, second pass, polishing round) call this themselves when less than a third of the HBM is free.
 * Result handles (rvn_reads, rvn_pass1, rvn_pass2) are not affected; rvn_engine_map_fetch results are. */
int rvn_engine_release_scratch(rvn_engine* e);

/* raven::FindOverlapsAndCreatePiles (RavenLib/src/construct.cc:14-121; decl construct.h:22-29):
 * index batches of `index_batch_bases` (reference: 1<<32), query flushes of `flush_bases` (reference:
 * 1<<30), merge, Pile::AddLayers (pile.cc:33-62) and the top-kMax truncation, all on the device.
 * Requires ids[i] == i (the reference's own invariant, construct.cc:25,74-75). */
int rvn_find_overlaps_and_create_piles(rvn_engine* e, const rvn_reads* r, double freq, uint32_t k_max_overlaps,
                                       int use_minhash, uint64_t index_batch_bases, uint64_t flush_bases,
                                       rvn_pass1** out);
uint64_t rvn_pass1_pile_words(const rvn_pass1* p);   /* sum over reads of (len >> 4) */
uint64_t rvn_pass1_num_overlaps(const rvn_pass1* p); /* sum of per-pile list sizes */
/* pile coverage: uint16 data of all piles concatenated + offsets[n+1] (Pile::data_, pile.h:133) */
int rvn_pass1_fetch_piles(const rvn_pass1* p, uint16_t* data, uint64_t* offsets);
/* overlaps[i] of construct.cc:666, concatenated + offsets[n+1] */
/* raven::TrimAndAnnotatePiles' first two steps on the coverage arrays where they are, in HBM
 * (RavenLib/src/construct.cc:131-139): Pile::FindValidRegion(coverage) + UpdateValidRegion + FindMedian
 * (pile.cc:122-174) for every pile.  begin / end in cells (Pile::begin_ / end_, i.e. bases >> 4), invalid = the
 * pile's is_invalid flag (the caller clears overlaps[i] for those, construct.cc:134-135); the coverage of valid piles
 * is zeroed outside the region exactly as UpdateValidRegion does (visible through rvn_pass1_fetch_piles).
 * The result also stays with the pass, for rvn_pass1_resolve.  FindChimericRegions: rvn_pass1_find_chimeric_regions. */
int rvn_pass1_trim_and_annotate(rvn_pass1* p, uint32_t coverage, uint32_t* begin, uint32_t* end, uint16_t* median,
                                uint8_t* invalid);
/* The third step of raven::TrimAndAnnotatePiles (construct.cc:139): Pile::FindChimericRegions (pile.cc:176-187) =
 * FindSlopes(1.82) (pile.cc:403-600: coverage drops / rises against the sliding maxima within 52 cells, evaluated in
 * double as the reference does), down-slope / up-slope pairing and MergeRegions (pile.cc:373-400), for every pile that
 * rvn_pass1_trim_and_annotate left valid (`invalid` = its output), on the coverage arrays in HBM.  Output: the piles'
 * chimeric_regions_ as (begin, end) cell pairs, pile i at region_offsets[i] .. region_offsets[i+1] (pairs; n + 1 entries,
 * caller's array); *regions is malloc'ed by the library (2 uint32 per pair), release with rvn_free.
 * Pile::is_maybe_chimeric() == (region_offsets[i+1] > region_offsets[i]). */
int rvn_pass1_find_chimeric_regions(rvn_pass1* p, const uint8_t* invalid, uint32_t* region_offsets, uint32_t** regions);
int rvn_pass1_fetch_overlaps(const rvn_pass1* p, rvn_overlap* overlaps, uint32_t* offsets);
void rvn_pass1_destroy(rvn_pass1* p);

/* raven::FindOverlapsAndRepetetiveRegions (RavenLib/src/construct.cc:316-491; decl construct.h:49-54), the second
 * all-vs-all pass on the VALID reads: valid reads first by id, index batches of `batch_bases` (reference: 1 << 30)
 * without minhash, Map(read, true, true, false, &filtered) + Pile::AddKmers(filtered, kmer_len) (pile.cc:64-120),
 * the identity filter when identity != 0 (construct.cc:385-424: OverlapUpdate, edlibAlign of the two spans, drop below
 * the threshold), then the merge of construct.cc:430-455 — OverlapUpdate, GetOverlapType (overlap_utils.cc:14-113),
 * containment flags, consecutive overlaps of the same pair keep the longer — the contained piles turned invalid and
 * the final OverlapUpdate sweep (construct.cc:466-480), all on the device.
 *   r               ALL reads, ids[i] == i
 *   pile_begin/end  Pile::begin() / Pile::end() of every pile in BASES (begin_ << 4), pile_invalid = Pile::is_invalid()
 * Result (rvn_pass2_fetch): the overlaps the reference leaves in the extra slot overlaps.back(), contained[n] = piles
 * this pass marked with set_is_contained() (the caller also sets them invalid, construct.cc:466-470), and the k-mer
 * cells Pile::kmers_ of the valid reads: (len >> 4) + 1 bytes (0/1) per valid read at kmers_offsets[id], nothing for
 * invalid reads (kmers_offsets has n + 1 entries; rvn_pass2_kmer_cells = their total). */
typedef struct rvn_pass2 rvn_pass2;
int rvn_find_overlaps_and_repetitive_regions(rvn_engine* e, const rvn_reads* r, const uint32_t* pile_begin,
                                             const uint32_t* pile_end, const uint8_t* pile_invalid, double freq,
                                             uint32_t kmer_len, double identity, uint64_t batch_bases, rvn_pass2** out);
uint64_t rvn_pass2_num_overlaps(const rvn_pass2* p);
uint64_t rvn_pass2_kmer_cells(const rvn_pass2* p);
int rvn_pass2_fetch(const rvn_pass2* p, rvn_overlap* overlaps, uint8_t* contained, uint8_t* kmers, uint64_t* kmers_offsets);
void rvn_pass2_destroy(rvn_pass2* p);

/* raven::ResolveRepeatInducedOverlaps (RavenLib/src/construct.cc:493-559, called at :690), on the device: until an
 * iteration removes nothing, ConnectedComponents (overlap_utils.cc:135-178: overlaps of GetOverlapType > 2 are edges,
 * components that hold a valid pile), the nth_element median of each component's Pile::median(),
 * Pile::FindRepetitiveRegions(median) of every member (pile.cc:230-317: k-mer groups, FindSlopes(1.42) pairs,
 * MergeRegions, clip to the valid region), UpdateRepetitiveRegions of both piles of every overlap and the removal of the
 * overlaps CheckRepetitiveRegions flags on either pile (pile.cc:319-369), survivors in order.
 *   overlaps, n_overlaps   overlaps.back() as rvn_pass2_fetch gives it (coordinates in bases); not modified
 *   coverage               Pile::data_ of every pile (uint16 per cell of 16 bases), pile i at coverage_offsets[i] ..
 *                          coverage_offsets[i+1] (n_piles + 1 entries), as rvn_pass1_fetch_piles gives it after the
 *                          host's ClearChimericRegions
 *   kmers                  Pile::kmers_ (0/1 per cell; none: kmers_ empty), offsets as rvn_pass2_fetch gives them
 *   pile_begin/end         Pile::begin() / Pile::end() in BASES (begin_ << 4), median = Pile::median(),
 *                          invalid = Pile::is_invalid(); the piles hold no repetitive regions yet
 * Result (rvn_repeats_fetch): the surviving overlaps (rvn_repeats_num_overlaps of them, in order), the piles'
 * repetitive_regions_ after the last iteration as (first, second) uint32 pairs — first = cell << 1 | flag bit set by
 * UpdateRepetitiveRegions, second = cell — pile i at region_offsets[i] .. region_offsets[i+1] (pairs; n_piles + 1
 * entries; rvn_repeats_num_regions pairs in all), is_repetitive[n_piles] = set_is_repetitive() happened, and stats. */
typedef struct rvn_repeats rvn_repeats;
typedef struct rvn_repeats_stats {
  uint32_t iterations; /* passes of the loop (the last one removes nothing) */
  uint32_t components; /* components with a valid pile, in the first iteration */
  uint64_t removed;    /* overlaps removed in all */
} rvn_repeats_stats;
int rvn_resolve_repeat_induced_overlaps(rvn_engine* e, const rvn_overlap* overlaps, uint64_t n_overlaps, uint32_t n_piles,
                                        const uint16_t* coverage, const uint64_t* coverage_offsets, const uint8_t* kmers,
                                        const uint64_t* kmers_offsets, const uint32_t* pile_begin, const uint32_t* pile_end,
                                        const uint16_t* median, const uint8_t* invalid, rvn_repeats** out);
uint64_t rvn_repeats_num_overlaps(const rvn_repeats* r);
uint64_t rvn_repeats_num_regions(const rvn_repeats* r);
/* every output may be NULL */
int rvn_repeats_fetch(const rvn_repeats* r, rvn_overlap* overlaps, uint32_t* regions, uint32_t* region_offsets,
                      uint8_t* is_repetitive, rvn_repeats_stats* stats);
void rvn_repeats_destroy(rvn_repeats* r);

/* The tail of stage -5 of raven::ConstructGraph on the device, in two phases (`phases`: bit 0 | bit 1):
 *   1  raven::ResolveContainedReads (RavenLib/src/construct.cc:154-248): the identity filter loop when identity != 0
 *      (:162-217), then for every overlap in list order OverlapUpdate and GetOverlapType (:221-237) — type 1 with an rhs
 *      pile that is not is_maybe_chimeric() marks pile i contained, type 2 with pile i not is_maybe_chimeric() marks the
 *      rhs pile, both drop the overlap, everything else is kept with its updated coordinates — and every contained pile
 *      made invalid with its list emptied (:238-244);
 *   2  raven::ResolveChimericSequences (construct.cc:250-314): the nth_element median of the non-zero Pile::median() of
 *      all piles (:259-267), Pile::ClearChimericRegions(median) with UpdateValidRegion on every pile that is not invalid
 *      (:270-282; pile.cc:189-228, :144-157), OverlapUpdate of every remaining overlap and the containment marks of
 *      types 1 and 2 (:287-308), the lists cleared (:310).  When no pile has a non-zero median the reference reads an
 *      empty vector; a valid pile always has one, so there is no valid pile either and the state is returned unchanged
 *      (lists included).
 * A result (rvn_resolved_fetch, every output may be NULL): begin / end (cells, Pile::begin_ / end_), invalid, contained,
 * chimeric (set_is_chimeric() happened) per pile; the piles' remaining chimeric_regions_ as (first, second) cell pairs,
 * pile i at region_offsets[i] .. region_offsets[i+1] (pairs; n + 1 entries; rvn_resolved_num_regions pairs in all);
 * the global median of phase 2 (0: it did not run or changed nothing); the lists (rvn_resolved_num_overlaps entries)
 * and offsets[n + 1] as they stand after the last phase that ran (empty after phase 2); the coverage of the host-array
 * form (rvn_resolved_coverage_words cells; the resident form leaves it on the pass); stats. */
typedef struct rvn_resolved rvn_resolved;
typedef struct rvn_resolve_stats {
  uint64_t dropped_by_update[2];   /* overlaps OverlapUpdate dropped in the marking loop of phase 1 / in phase 2 */
  uint64_t dropped_by_filter;      /* overlaps the identity filter loop dropped (OverlapUpdate or the score) */
  uint64_t dropped_by_containment; /* type 1 / 2 overlaps of phase 1 that marked a pile */
  uint32_t contained[2];           /* piles that became contained in phase 1 / phase 2 */
  uint32_t cut;                    /* piles whose valid region ClearChimericRegions changed (set_is_chimeric) */
  uint32_t invalidated;            /* piles UpdateValidRegion made invalid in ClearChimericRegions */
} rvn_resolve_stats;
/* ... on a first pass whose lists and coverage are in HBM (replaces construct.cc:671-674 for a caller that keeps its
 * piles on the device).  Runs raven::TrimAndAnnotatePiles (construct.cc:123-152, FindValidRegion(coverage)) first when
 * the pass has not been trimmed yet, and FindChimericRegions with its result left in HBM.  A phase runs once per pass:
 * phases = 1 and later phases = 2 give what phases = 3 gives.  The lists of a result of phase 1 are read from the pass:
 * fetch them before phase 2 runs on it.  r: the reads of the pass, needed when identity != 0 (else it may be NULL).
 * Afterwards the coverage of the pass (rvn_pass1_fetch_piles) is what the reference's piles hold; the lists
 * rvn_pass1_fetch_overlaps gives are still the first pass's. */
int rvn_pass1_resolve(rvn_pass1* p, const rvn_reads* r, uint32_t coverage, double identity, uint32_t phases,
                      rvn_resolved** out);
/* ... on the caller's arrays (replaces construct.cc:154-248 and :250-314 behind their signatures): overlaps / offsets
 * as rvn_pass1_fetch_overlaps gives them (every entry of list i has lhs_id == i, construct.cc:74-75), coverage /
 * coverage_offsets as rvn_pass1_fetch_piles, regions / region_offsets as rvn_pass1_find_chimeric_regions, begin / end
 * (cells) / median / invalid as rvn_pass1_trim_and_annotate.  Nothing is modified.  RVN_EINVAL when an entry of list i
 * has another lhs_id, an id is out of range, or a region or valid region leaves its pile. */
int rvn_resolve_contained_and_chimeric(rvn_engine* e, const rvn_reads* r, const rvn_overlap* overlaps,
                                       const uint32_t* offsets, uint32_t n_piles, const uint16_t* coverage,
                                       const uint64_t* coverage_offsets, const uint32_t* regions,
                                       const uint32_t* region_offsets, const uint32_t* begin, const uint32_t* end,
                                       const uint16_t* median, const uint8_t* invalid, double identity, uint32_t phases,
                                       rvn_resolved** out);
uint64_t rvn_resolved_num_overlaps(const rvn_resolved* r);
uint64_t rvn_resolved_num_regions(const rvn_resolved* r);
uint64_t rvn_resolved_coverage_words(const rvn_resolved* r);
int rvn_resolved_fetch(const rvn_resolved* r, uint32_t* begin, uint32_t* end, uint8_t* invalid, uint8_t* contained,
                       uint8_t* chimeric, uint32_t* regions, uint32_t* region_offsets, uint16_t* median,
                       rvn_overlap* overlaps, uint32_t* offsets, uint16_t* coverage, rvn_resolve_stats* stats);
void rvn_resolved_destroy(rvn_resolved* r);

/* The identity filter loop of raven::ResolveContainedReads (RavenLib/src/construct.cc:162-217) on the per-pile overlap
 * lists overlaps[i] (concatenated, offsets[n+1], both updated in place): every overlap goes through OverlapUpdate
 * (overlap_utils.cc:14-80; dropped when it fails), its two spans through the batched exact edit distance (rhs
 * reverse-complemented on the opposite strand), and is kept with its updated coordinates when
 * 1 - distance / max(length) >= identity.  The containment marking that follows in the reference is host graph logic. */
int rvn_filter_overlaps_by_identity(rvn_engine* e, const rvn_reads* r, rvn_overlap* overlaps, uint32_t* offsets,
                                    const uint32_t* pile_begin, const uint32_t* pile_end, const uint8_t* pile_invalid,
                                    double identity);

/* raven::Pile::AddLayers on one pile (RavenLib/src/pile.cc:33-62): `data` (cells = len >> 4) is updated
 * in place with the coverage of `n` overlaps touching pile `id`. */
int rvn_pile_add_layers(rvn_engine* e, uint16_t* data, uint32_t cells, uint32_t id, const rvn_overlap* overlaps,
                        uint64_t n);

/* raven::Pile::AddKmers (RavenLib/src/pile.cc:64-120; call site construct.cc:382) for reads
 * [first_read, first_read + n_reads): `positions` are the `filtered` outputs of Map (rvn_engine_map_fetch_filtered)
 * concatenated with position_offsets[n_reads+1]; `kmers` holds, per read, Pile::kmers_ as (len >> 4) + 1 bytes
 * (0/1) at kmers_offsets[i]; cells of k-mers that pass the low-complexity filter are set to 1. */
int rvn_pile_add_kmers_batch(rvn_engine* e, const rvn_reads* r, uint32_t first_read, uint32_t n_reads,
                             const uint32_t* positions, const uint64_t* position_offsets, uint8_t* kmers,
                             const uint64_t* kmers_offsets);

/* Batched edlibAlign(lhs, rhs, edlibDefaultAlignConfig()).editDistance (global / NW, unit costs) between
 * spans of uploaded reads: RavenLib/src/construct.cc:176-199 (identity filter of ResolveContainedReads) and
 * :393-416 (second pass).  lhs/rhs_read are read INDICES in `r`; strand == 0 reverse-complements the rhs span
 * first (construct.cc:184-188).  distances[i] is the exact edit distance (any size; no threshold). */
typedef struct rvn_ed_pair {
  uint32_t lhs_read, lhs_begin, lhs_len;
  uint32_t rhs_read, rhs_begin, rhs_len;
  uint32_t strand;
  uint32_t reserved;
} rvn_ed_pair;
int rvn_edit_distance_batch(rvn_engine* e, const rvn_reads* r, const rvn_ed_pair* pairs, uint32_t n_pairs,
                            uint32_t* distances, double* device_ms, uint64_t* cells);

/* Batched global alignment PATHS of read spans: what racon gets from edlibAlign(query, target, EDLIB_MODE_NW,
 * EDLIB_TASK_PATH) in Overlap::find_breaking_points, behind racon::Polisher::Initialize / Polish of
 * RavenLib/src/polish.cc:43-51 — the alignment-path stage of rvn_polish_round, with the path itself as the result.
 * Pair i aligns a span of read `query_read` of `queries` with a span of read `target_read` of `targets` (the two sets may
 * be one handle); begins are counted in the reads as stored, and strand == 0 reverse-complements the query span first.
 * The path is an optimal one (its cost is the exact edit distance).  Where several are optimal the walk, which goes from
 * the end of the alignment to its start, prefers the diagonal ('=' or 'X'), then a query base only ('I'), then a target
 * base only ('D').  edlib documents NO tie rule for the paths it returns — any optimal path is "the" edlib path —, so the
 * distance, not the op string, is what agrees with edlib on every input.
 * Result (a handle; its arrays stay on the device until they are fetched):
 *   distances[n_pairs]     the exact edit distance; 0xFFFFFFFF: not aligned (below)
 *   run_offsets[n_pairs+1] the runs of pair i are runs[run_offsets[i] .. run_offsets[i + 1])
 *   runs[n_runs]           count << 2 | op, op = EDLIB_EDOP_* (0 '=', 1 'I', 2 'D', 3 'X'), in alignment order from the
 *                          start; adjacent runs of a pair have different ops.  'I' consumes a query base, 'D' a target
 *                          base: counts of ops {0, 3, 1} add up to query_len, of {0, 3, 2} to target_len, and the ops
 *                          other than '=' to distances[i].  An empty query gives one 'D' run, an empty target one 'I'
 *                          run, both empty no run.
 *   ops (rvn_paths_fetch_ops)  the same paths as edlib's alignment array, one byte per op, expanded on the device;
 *                          pair i at ops[op_offsets[i] .. op_offsets[i + 1]), n_ops bytes in all
 * A pair whose band is beyond the stage's limits (the ones that make a polishing round count n_dropped_layers: a band of
 * more than eight rings of eight 64-row blocks per lane, or one whose stored columns exceed the engine option
 * nw_budget_mb) gets distance 0xFFFFFFFF and no runs and is counted in n_not_aligned; that is not an error of the call.
 * A read index outside its set or a span outside its read: RVN_EINVAL.
 * The alignment of (lhs, reverse complement of rhs) of a Raven overlap: pass rhs as the QUERY with strand = 0, lhs as the
 * target, and swap 'I' and 'D' in the result. */
typedef struct rvn_align_pair {
  uint32_t query_read, query_begin, query_len;    /* span of read `query_read` of `queries`, as stored */
  uint32_t target_read, target_begin, target_len; /* span of read `target_read` of `targets` */
  uint32_t strand;   /* 0: the query span is reverse-complemented before it is aligned; 1: as stored */
  uint32_t reserved;
} rvn_align_pair;
typedef struct rvn_paths rvn_paths;
int rvn_align_path_batch(rvn_engine* e, const rvn_reads* queries, const rvn_reads* targets, const rvn_align_pair* pairs,
                         uint32_t n_pairs, rvn_paths** out);
int rvn_paths_info(const rvn_paths* p, uint32_t* n_pairs, uint64_t* n_runs, uint64_t* n_ops, uint32_t* n_not_aligned);
int rvn_paths_fetch(const rvn_paths* p, uint32_t* distances, uint64_t* run_offsets, uint32_t* runs);
int rvn_paths_fetch_ops(const rvn_paths* p, uint64_t* op_offsets, uint8_t* ops);
void rvn_paths_destroy(rvn_paths* p);

/* Batched racon Window::GenerateConsensus (the POA consensus behind racon::Polisher::Polish,
 * RavenLib/src/polish.cc:43-51; scores = AlignCfg of polish.hpp:13-17): for every window, layer 0 is the
 * backbone, the others are the read pieces aligned to it.
 *   codes            base codes 0..3 of all layers of all windows, concatenated
 *   quals            Phred+33 characters parallel to codes, or NULL; has_qual[layer] selects per layer
 *                    (racon gives a backbone without quality a dummy '!' string, i.e. weight 0)
 *   layer_offsets    [n_layers+1] into codes;  begins/ends [n_layers]: first/last covered backbone position
 *   window_offsets   [n_windows+1] into the layer tables
 *   consensus        output codes, window w at consensus_offsets[w] (capacity = next offset - this one)
 *   status           0: fewer than 3 sequences, backbone returned (racon: unpolished)   1: polished
 *                    2: window exceeds the device limits (nodes / layer length / in-degree), backbone returned
 * Results agree with the CPU path within edit-distance tolerance (ties between equal-score paths may resolve
 * differently). */
int rvn_poa_consensus_batch(rvn_engine* e, const uint8_t* codes, const uint8_t* quals, const uint64_t* layer_offsets,
                            const uint32_t* begins, const uint32_t* ends, const uint32_t* has_qual,
                            const uint32_t* window_offsets, uint32_t n_windows, int match, int mismatch, int gap,
                            int trim, uint8_t* consensus, const uint64_t* consensus_offsets, uint32_t* consensus_len,
                            uint32_t* status, double* device_ms);

/* One polishing round == racon::Polisher::Polish(targets, sequences, drop_unpolished = false) as raven::Polish calls
 * it (RavenLib/src/polish.cc:43-51: e = 0.3, w = 500, trim = true; `q` = the average read quality computed at
 * polish.cc:26-41; match/mismatch/gap = AlignCfg).  `e` must have been created with k = 15, w = 5 (racon's own
 * minimizer engine).  targets / reads are uploaded read sets; read_quals = per-base Phred+33 of every read
 * concatenated in read order (qual_offsets[n_reads+1]) or NULL.  Output: polished base codes of target t at
 * out_offsets[t] (capacity out_offsets[t+1]-out_offsets[t]; 2 x length + 1024 is ample), out_len[t], and the
 * polished-window ratio racon writes into the XC:f: tag (polish.cc:57-59 tests it for > 0).
 * Window breakpoints come from the exact global alignment path of every read's best overlap, as in racon
 * (DESIGN.md §3.7); read_quals == NULL uses the qualities attached with rvn_reads_attach_quality, if any. */
typedef struct rvn_polish_stats {
  uint64_t n_overlaps, n_reads_used, n_layers, n_windows, n_polished_windows, n_failed_windows;
  double poa_ms;                    /* device time of the window-consensus batch */
  double map_ms, host_ms, total_ms; /* wall: index + map + best overlap | host planning (jobs, window tables) | whole call */
  uint64_t n_dropped_layers;        /* reads left out because their alignment is beyond the path stage (band > 262 144 rows, or
                                       its stored band alone above the stage's HBM budget, engine option nw_budget_mb) */
  double align_ms;                  /* device time of the alignment-path stage (banded NW forward + traceback) */
  uint64_t n_aligned, n_align_retries; /* read-to-target alignments done | attempts repeated with a doubled band */
  uint64_t align_band_cells;        /* DP cells inside the computed bands (all attempts) */
  uint64_t align_store_bytes;       /* largest band store of one batch (16 + 4 bytes per 64 cells) */
} rvn_polish_stats;
int rvn_polish_round(rvn_engine* e, rvn_reads* targets, rvn_reads* reads, const uint8_t* read_quals,
                     const uint64_t* qual_offsets, double q, double err, uint32_t w, int trim, int match, int mismatch,
                     int gap, uint8_t* out_codes, const uint64_t* out_offsets, uint32_t* out_len, double* ratio,
                     rvn_polish_stats* stats);

/* ---- stage-level entry points of the SHARDED single-genome pass (one engine per GPU) ------------
 * FindOverlapsAndCreatePiles (construct.cc:14-121) split where the data has to move between GPUs.  Reads are
 * range-partitioned by pile (rank g owns a contiguous id range and uploads only those reads, ids = global read
 * indices), minimizer values are partitioned by hash class.  Host side: raven_amd/sharded.py.
 *   1. rvn_shard_sketch           own reads -> (value, origin) with the minhash-selected entries flagged (bit 63 of
 *                                 origin) == the per-read part of ram Minimize + the query sketch of Map
 *      -- all-to-all #1: every minimizer to the owner of its hash class --
 *   2. rvn_shard_index_build      owner: stable sort by value == its hash class of ram's index, same relative order
 *   3. rvn_shard_key_counts       per-key counts -> all-reduce of the count histogram -> exact global Filter
 *      rvn_engine_set_occurrence
 *   4. rvn_shard_join             owner: index probes of Map for every query entry of its hash class; matches
 *                                 segmented by the query read's GLOBAL id
 *      -- all-to-all #2: every match to the owner of its query read (the candidate-pair exchange) --
 *   5. rvn_shard_chain            read owner: sort / bands / LIS / emission of Map -> rvn_engine_map_fetch
 *      -- all-to-all #3: every overlap also to the owner of its rhs read --
 *   6. rvn_shard_piles            pile owner: merge (construct.cc:72-77), AddLayers, top-kMax truncation
 * The result for the reads a rank owns is bit-identical to the single-GPU pass (tests/test_gpu_sharded.py). */
int rvn_shard_sketch(rvn_engine* e, const rvn_reads* own_reads, int index_minhash, uint64_t* count);
/* The same for the reads [first, last) of `own` (indices into the handle).  foreign != 0: these reads belong to an EARLIER
 * index batch of a pass with several (construct.cc:32-37: an index batch is 2^32 bases; every read up to the batch's end is
 * mapped against it, :59-64): only their minhash-selected minimizers come back, flagged query-only (bit 62 of the origin
 * word beside the query flag, bit 63) — the index shard sorts them in beside its members, the self-join matches them
 * against the members and never counts them towards a key's occurrence.  Fetch with rvn_shard_sketch_fetch[_dev] before
 * the next call. */
int rvn_shard_sketch_range(rvn_engine* e, const rvn_reads* own, uint32_t first, uint32_t last, int index_minhash, int foreign,
                           uint64_t* count);
int rvn_shard_sketch_fetch(rvn_engine* e, uint64_t* values, uint64_t* origins);
int rvn_shard_index_build(rvn_engine* e, const uint64_t* values, const uint64_t* origins, uint64_t n, int all_query);
int rvn_shard_key_counts(rvn_engine* e, uint32_t* counts /* n_keys of rvn_engine_index_size */);
int rvn_engine_set_occurrence(rvn_engine* e, uint32_t occurrence);
int rvn_shard_join(rvn_engine* e, uint32_t n_reads_total, int avoid_equal, int avoid_symmetric, uint64_t* n_matches);
/* same, restricted to the query reads [query_first, query_last) of one flush window (construct.cc:56-70): a pass with
 * several flush windows joins, chains and merges window by window, exactly as the reference flushes */
int rvn_shard_join_range(rvn_engine* e, uint32_t n_reads_total, int avoid_equal, int avoid_symmetric,
                         uint32_t query_first, uint32_t query_last, uint64_t* n_matches);
int rvn_shard_join_fetch(rvn_engine* e, uint64_t* group, uint64_t* positions, uint64_t* seg_off /* n_reads_total+1 */);
int rvn_shard_chain(rvn_engine* e, const rvn_reads* own_reads, const uint64_t* group, const uint64_t* positions,
                    const uint64_t* seg_off /* own n + 1 */, uint64_t* n_overlaps);
/* overlaps: Map outputs in (query read, emission) order over ALL reads' id space; only piles of reads whose
 * overlaps are complete in the list (the caller's own range) are meaningful in the returned handle */
int rvn_shard_piles(rvn_engine* e, const uint32_t* lengths, uint32_t n_reads_total, const rvn_overlap* overlaps,
                    uint64_t n, uint32_t kmax, rvn_pass1** out);

/* piles kept across the flush windows of a pass: create once, merge the Map outputs of every window (each merge =
 * the serial merge + AddLayers + top-kMax truncation of one flush, construct.cc:72-110); rvn_shard_piles = both.
 * Precondition of every merge entry: the list is grouped by ascending lhs_id, every id is < n_reads_total and every
 * overlap has lhs_id < rhs_id (Map with avoid_equal and avoid_symmetric) — a pile's list is built as kept ++ reversed
 * incoming ++ own, which is the reference's order only then.  The host entries (rvn_shard_piles, rvn_shard_piles_merge)
 * check all three and return RVN_EINVAL, leaving the pass as it was; the _dev entries (rvn_shard_piles_merge_dev,
 * rvn_shard_piles_merge_parts_dev, rvn_shard_piles_dev) do NOT look at the list: there the caller guarantees them, and
 * a list that breaks them gives an undefined result. */
int rvn_shard_piles_create(rvn_engine* e, const uint32_t* lengths, uint32_t n_reads_total, rvn_pass1** out);
int rvn_shard_piles_merge(rvn_pass1* p, const rvn_overlap* overlaps, uint64_t n, uint32_t kmax);
int rvn_shard_piles_merge_dev(rvn_pass1* p, const rvn_overlap* d_overlaps, const uint32_t* d_overlap_read_off, uint64_t n,
                              uint32_t kmax);

/* Device-pointer variants of the same stages: every d_* argument is a pointer into HBM owned by the caller (the
 * torch CUDA tensors the exchanges run on), so nothing crosses PCIe between the stages.  Calls are synchronous with
 * respect to the engine's stream; the caller synchronises its own stream before passing buffers in. */
int rvn_shard_sketch_fetch_dev(rvn_engine* e, uint64_t* d_values, uint64_t* d_origins);
int rvn_shard_index_build_dev(rvn_engine* e, const uint64_t* d_values, const uint64_t* d_origins, uint64_t n,
                              int all_query, uint64_t n_flagged /* origins with bit 63 set */);
/* count-of-counts of this shard's keys: hist[65536] (host; bin 65535 = number of keys with count >= 65535, whose
 * counts go to over[0..*n_over)) */
int rvn_shard_key_histogram(rvn_engine* e, uint64_t* hist, uint32_t* over, uint32_t over_cap, uint32_t* n_over);
int rvn_shard_join_fetch_dev(rvn_engine* e, uint64_t* d_group, uint64_t* d_positions, uint64_t* d_seg_off);
int rvn_shard_chain_dev(rvn_engine* e, const rvn_reads* own_reads, const uint64_t* d_group, const uint64_t* d_positions,
                        const uint64_t* d_seg_off, uint64_t n_matches, uint64_t* n_overlaps);
int rvn_engine_map_fetch_dev(rvn_engine* e, rvn_overlap* d_overlaps, uint32_t* d_read_offsets);
/* Partition / regroup steps between the stages (device pointers; `counts`, `bounds`, `n_per_source` and the pointer tables
 * themselves are host memory).  They replace what a host would do with sort / bincount / gather:
 *   split_minimizers  stable partition of (value, origin) by owner rank = hash class of the value (the order inside a
 *                     rank's part is the input order = ram's (read, position) order); counts[world]
 *   count_flagged     number of origins with bit 63 set (the minhash-selected query entries) in a received buffer
 *   adjacent_diff     per-read match counts out of the per-read offsets of rvn_shard_join_fetch_dev
 *   regroup           matches received from every index owner -> per-read segments, sources in rank order
 *   split_overlaps    stable partition of Map's overlaps by the owner of their rhs read (bounds[world + 1] = read ranges);
 *                     counts[world + 1], the last bucket = overlaps whose rhs read is `self`'s (they stay and are not copied
 *                     to d_out's first buckets)
 *   merge_parts       rvn_shard_piles_merge_dev on the concatenation of `n_parts` lists (received parts in rank order, own
 *                     overlaps last), per-read offsets computed on the device */
int rvn_shard_split_minimizers_dev(rvn_engine* e, const uint64_t* d_values, const uint64_t* d_origins, uint64_t n,
                                   uint32_t world, uint64_t* d_values_out, uint64_t* d_origins_out, uint64_t* counts);
int rvn_shard_count_flagged_dev(rvn_engine* e, const uint64_t* d_origins, uint64_t n, uint64_t* count);
int rvn_shard_adjacent_diff_dev(rvn_engine* e, const uint64_t* d_seg_off, uint64_t n, uint64_t* d_counts);
int rvn_shard_regroup_dev(rvn_engine* e, uint32_t world, const uint64_t* const* d_counts, const uint64_t* const* d_group,
                          const uint64_t* const* d_positions, const uint64_t* n_per_source, uint32_t n_reads,
                          uint64_t* d_seg_off, uint64_t* d_group_out, uint64_t* d_positions_out);
int rvn_shard_split_overlaps_dev(rvn_engine* e, const rvn_overlap* d_overlaps, uint64_t n, const uint32_t* bounds,
                                 uint32_t world, uint32_t self, rvn_overlap* d_out, uint64_t* counts);
int rvn_shard_piles_merge_parts_dev(rvn_pass1* p, uint32_t n_parts, const rvn_overlap* const* d_parts,
                                    const uint64_t* n_per_part, uint32_t kmax);
int rvn_shard_piles_dev(rvn_engine* e, const uint32_t* lengths /* host */, uint32_t n_reads_total,
                        const rvn_overlap* d_overlaps, const uint32_t* d_overlap_read_off /* n_reads_total + 1 */,
                        uint64_t n, uint32_t kmax, rvn_pass1** out);

/* The two halves of the first step of a round, for the sharded round: reads are mapped independently of
 * each other, so rank g maps the slice [read_first, read_last) of the reads and the ranks all-gather the table.
 *   rvn_polish_map_best  index the targets, map the slice, best overlap per read (racon Polisher::Initialize: longest
 *                        overlap after the error filter); best[i] / best_target[i] describe read read_first + i,
 *                        best_target = index into `targets` or 0xFFFFFFFF when the read is not used.
 *   rvn_polish_set_best  hands the complete table (n_reads = size of the read set) to the NEXT rvn_polish_round[_range]
 *                        call on this engine, which then skips its own mapping; the table is consumed by that call. */
int rvn_polish_map_best(rvn_engine* e, rvn_reads* targets, rvn_reads* reads, uint32_t read_first, uint32_t read_last,
                        double err, rvn_overlap* best, uint32_t* best_target, uint64_t* n_overlaps);
int rvn_polish_set_best(rvn_engine* e, const rvn_overlap* best, const uint32_t* best_target, uint32_t n_reads);

/* Same round restricted to the windows [window_first, window_last) of the global numbering (windows of target 0,
 * then of target 1, ...; ceil(len / w) per target): what one GPU does when a round is sharded by windows
 * (windows are independent).  out_codes receives, per target, the consensus of ITS windows inside the
 * range only (possibly empty), n_windows / n_polished the per-target window counts inside the range; concatenating the
 * per-target pieces of consecutive ranges reproduces rvn_polish_round exactly (raven_amd/sharded.py). */
int rvn_polish_round_range(rvn_engine* e, rvn_reads* targets, rvn_reads* reads, const uint8_t* read_quals,
                           const uint64_t* qual_offsets, double q, double err, uint32_t w, int trim, int match,
                           int mismatch, int gap, uint64_t window_first, uint64_t window_last, uint8_t* out_codes,
                           const uint64_t* out_offsets, uint32_t* out_len, double* ratio, uint32_t* n_windows,
                           uint32_t* n_polished, rvn_polish_stats* stats);

/* ---- N GPUs behind ONE host process (the engine with a device list; 8(e): reads by pile, minimizers by hash
 * class, three exchanges per flush window) --------------------------------------------------------------------------------
 * raven::ConstructGraph / raven::Polish own one ram::MinimizerEngine / one racon::Polisher (RavenLib/src/construct.cc:661-669,
 * polish.cc:43-51), so "all visible GPUs" lives behind one handle: a group = one engine + one worker thread per listed
 * device (a device may be listed more than once: virtual ranks).  The stages are the rvn_shard_* entry points above; the
 * exchanges are pairwise hipMemcpyPeerAsync pulls between the engines' buffers (xGMI between devices) bracketed by
 * in-process barriers — the all-to-all a torch.distributed job performs with RCCL (raven_amd/sharded.py), without leaving
 * the process.  Results are bit-identical to the single-engine calls.
 *   rvn_group_find_overlaps_and_create_piles   = rvn_find_overlaps_and_create_piles over all devices: bounds[n_devices + 1]
 *       receives the read ranges, out[r] a pass handle whose piles / overlap lists are complete for the reads
 *       [bounds[r], bounds[r+1]) (fetch them with rvn_pass1_fetch_* — arrays are indexed by GLOBAL read id — and release
 *       with rvn_pass1_destroy).  A read set beyond 2^32 bases is indexed in several batches as construct.cc:32-37 does
 *       (rvn_group_find_overlaps_and_create_piles_batched takes the batch size: tests force several batches with it).
 *   rvn_group_polish_round                     = rvn_polish_round over all devices (reads mapped by slice, windows by range,
 *       pieces concatenated in rank order); host arrays in, consensus out as in rvn_polish_round. */
typedef struct rvn_group rvn_group;
int rvn_group_create(rvn_group** out, uint32_t k, uint32_t w, uint32_t bandwidth, uint32_t chain, uint32_t matches,
                     uint32_t gap, const int* devices, uint32_t n_devices);
void rvn_group_destroy(rvn_group* g);
uint32_t rvn_group_size(const rvn_group* g);
rvn_engine* rvn_group_engine(rvn_group* g, uint32_t rank);
int rvn_group_find_overlaps_and_create_piles(rvn_group* g, const uint64_t* packed, const uint64_t* word_offsets,
                                             const uint32_t* lengths, uint32_t n_reads, double freq, uint32_t kmax,
                                             int use_minhash, uint64_t flush_bases, uint32_t* bounds, rvn_pass1** out);
int rvn_group_find_overlaps_and_create_piles_batched(rvn_group* g, const uint64_t* packed, const uint64_t* word_offsets,
                                                     const uint32_t* lengths, uint32_t n_reads, double freq, uint32_t kmax,
                                                     int use_minhash, uint64_t index_batch_bases, uint64_t flush_bases,
                                                     uint32_t* bounds, rvn_pass1** out);
int rvn_group_polish_round(rvn_group* g, const uint64_t* t_packed, const uint64_t* t_word_offsets, const uint32_t* t_lengths,
                           uint32_t n_targets, const uint64_t* r_packed, const uint64_t* r_word_offsets,
                           const uint32_t* r_lengths, uint32_t n_reads, double q, double err, uint32_t w, int trim, int match,
                           int mismatch, int gap, uint8_t* out_codes, const uint64_t* out_offsets, uint32_t* out_len,
                           double* ratio);
/* The same round with base qualities (the FASTQ variant of raven::Polish: racon's mean-quality filter against `q`,
 * polish.cc:26-41, and quality-weighted edges in the window graphs): r_quals = Phred+33 bytes, one per
 * 2^qual_block_shift bases of a read (6 = biosoup's block_quality), read i at r_qual_offsets[i] — exactly what
 * rvn_reads_attach_quality takes; every rank attaches them to its copy of the read set.  r_quals == NULL is
 * rvn_group_polish_round. */
int rvn_group_polish_round_q(rvn_group* g, const uint64_t* t_packed, const uint64_t* t_word_offsets, const uint32_t* t_lengths,
                             uint32_t n_targets, const uint64_t* r_packed, const uint64_t* r_word_offsets,
                             const uint32_t* r_lengths, uint32_t n_reads, const uint8_t* r_quals, const uint64_t* r_qual_offsets,
                             int qual_block_shift, double q, double err, uint32_t w, int trim, int match, int mismatch, int gap,
                             uint8_t* out_codes, const uint64_t* out_offsets, uint32_t* out_len, double* ratio);
/* Which ranks reach each other's memory directly: direct[i * n + j] = 1 when rank i pulls from rank j without staging (the
 * same device, or hipDeviceCanAccessPeer + hipDeviceEnablePeerAccess succeeded: xGMI on an MI355X node); 0 = the copy goes
 * through host memory (still correct, PCIe speed).  direct may be NULL.  Returns 1 when every pair is direct, 0 when
 * some pair is not, RVN_EINVAL for a NULL group. */
int rvn_group_peer_access(const rvn_group* g, uint8_t* direct);

/* The rest of the overlap phase of raven::ConstructGraph (construct.cc:650-707) over the group; host arrays in, the reads
 * as rvn_group_find_overlaps_and_create_piles takes them (read i = id i).
 *   rvn_group_find_overlaps_and_repetitive_regions  = rvn_find_overlaps_and_repetitive_regions over all devices: ONE result
 *       handle, owned by rank 0's engine, byte-identical to the single engine's on the same input (fetch and release it
 *       with rvn_pass2_*).  The valid reads are split into contiguous ranges balanced by length x index batches mapped
 *       against; every rank builds the index of each batch that ends after the start of its range (the whole batch:
 *       replicated, not divided) and maps the valid reads of its range (Map, AddKmers, identity filter, classification); rank 0
 *       gathers the survivors in batch-major, rank-minor order, the k-mer cells of every range and the containment flags
 *       OR'd over the ranks, then runs the de-duplication, invalidation and final OverlapUpdate sweep once.
 *   rvn_group_filter_overlaps_by_identity           = rvn_filter_overlaps_by_identity over all devices: piles split
 *       into contiguous ranges balanced by the span lengths of their overlaps, lists updated in place exactly as the
 *       single-engine call does. */
int rvn_group_find_overlaps_and_repetitive_regions(rvn_group* g, const uint64_t* packed, const uint64_t* word_offsets,
                                                   const uint32_t* lengths, uint32_t n_reads, const uint32_t* pile_begin,
                                                   const uint32_t* pile_end, const uint8_t* pile_invalid, double freq,
                                                   uint32_t kmer_len, double identity, uint64_t batch_bases, rvn_pass2** out);
int rvn_group_filter_overlaps_by_identity(rvn_group* g, const uint64_t* packed, const uint64_t* word_offsets,
                                          const uint32_t* lengths, uint32_t n_reads, rvn_overlap* overlaps, uint32_t* offsets,
                                          const uint32_t* pile_begin, const uint32_t* pile_end, const uint8_t* pile_invalid,
                                          double identity);

/* raven::OverlapUpdate (RavenLib/src/overlap_utils.cc:14-85) followed by raven::GetOverlapType (:87-121) on a list of
 * overlaps, on the HOST (the library's __host__ build of the rules its kernels run: raven_amd/csrc/overlap_rules.h) — for
 * a caller that holds overlaps and pile regions in host arrays between two device stages, as ResolveContainedReads does
 * (construct.cc:218-254).  pile_begin / pile_end in bases, pile_invalid != 0 = Pile::is_invalid().  ok[i] = OverlapUpdate's
 * result (the overlap is updated in place when 1); type[i] = GetOverlapType of the updated overlap (0 internal, 1 lhs
 * contained, 2 rhs contained, 3 / 4 dovetails), 0xFFFFFFFF when ok[i] == 0. */
int rvn_overlap_update_and_type(rvn_overlap* overlaps, uint64_t n, const uint32_t* pile_begin, const uint32_t* pile_end,
                                const uint8_t* pile_invalid, uint32_t n_piles, uint8_t* ok, uint32_t* type);

/* The force-directed layout of raven's RemoveLongEdges (RavenLib/src/assemble.cc:357-627: a Barnes-Hut quadtree and one
 * force per point, n_iterations times) for every component of the call at once, bit for bit what the reference's loop
 * computes from the same start positions.  Points [component_offsets[c], component_offsets[c + 1]) are
 * component c; xy_in holds their start positions (x, y per point: the reference draws them from its generator, the
 * facade include/raven_hip/layout.hpp does the same); adj[adj_offsets[i] .. adj_offsets[i + 1]) are the neighbours of
 * point i as point indices, in the order their attraction terms are added (the reference: in-edges, out-edges,
 * transitive).  Per component k = sqrt(1 / size), t = 0.1, dt = t / (n_iterations + 1), t -= dt after every iteration.
 * xy_out receives the positions after the last iteration (n_iterations == 0: xy_in).  Components of any size are taken:
 * the reference's size >= 6 and junction rules are the caller's.
 * stats (may be NULL): host_tree_iterations = (component, iteration) pairs whose repulsive forces were computed on the
 * host from an insertion-built tree, because two points shared a 32-level path or a point fell between the children of
 * a cell (the only cases in which the reference's tree depends on its insertion order); max_depth = the deepest tree
 * built on the device.
 * RVN_EINVAL: offsets that do not ascend from 0, an empty component, a neighbour outside its point's component, a
 * coordinate that is NaN or infinite, more than 2^28 points. */
typedef struct {
  uint64_t host_tree_iterations;
  uint32_t max_depth;
  uint32_t reserved;
} rvn_layout_stats;
int rvn_layout_force_directed(rvn_engine* e, uint32_t n_components, const uint32_t* component_offsets, const double* xy_in,
                              const uint64_t* adj_offsets, const uint32_t* adj, uint32_t n_iterations, double* xy_out,
                              rvn_layout_stats* stats);

/* The assembly graph on the device (facade: include/raven_hip/assembly_graph.hpp): raven's
 * ConstructAssemblyGraph (RavenLib/src/construct.cc:561-648) as an edge table in HBM, and the marking halves of
 * RemoveTransitiveEdges (assemble.cc:23-56) and of RemoveLongEdges' loop (assemble.cc:708-721) on it.  RemoveEdges, tips,
 * bubbles stay the caller's (unitigs: the next block).  A graph is immutable once made.
 * Node 2i / 2i + 1 = the i-th valid pile and its reverse complement; edge 2j / 2j + 1 = the pair made of the j-th overlap
 * that OverlapFinalize keeps; the pair of an edge is always id ^ 1.
 *
 * rvn_construct_assembly_graph: overlaps = overlaps.back() as rvn_resolve_repeat_induced_overlaps leaves it, pile_begin /
 * pile_end in bases, median = Pile::median(), invalid 0/1.  Per kept overlap: tail = node(lhs), head = node(rhs) + 1 -
 * strand, length = lhs_begin - rhs_begin, the pair's length = (len(rhs) - rhs_end) - (len(lhs) - lhs_end) on the finalized
 * coordinates in uint32 arithmetic; score 4 swaps head and tail and negates both lengths.
 * rvn_graph_from_edges: the same handle from an existing graph (graph.edges flattened): tail == 0xFFFFFFFF marks an empty
 * slot (graph.edges[i] == nullptr).
 * rvn_graph_fetch: every output may be NULL.  sequence_to_node[n_piles] (-1: invalid pile), node_pile / node_coverage
 * [n_nodes], edge_tail / edge_head / edge_length [n_edges], edge_overlap [n_edges / 2] (index of the pair's overlap in the
 * caller's list), finalized [n_edges / 2] (the overlaps after OverlapFinalize).  A graph made from edges has only the three
 * edge arrays.
 * rvn_graph_mark_transitive: for every node v, every out-edge jt and every out-edge kt of head(jt) (out-edges in
 * ascending edge id), c = the out-edge of v into head(kt) with the largest id; when c exists and length(jt) + length(kt)
 * (wrapping in 32 bits) is within 12 % of length(c) either way, c and c ^ 1 are marked.  n_marked = marked ids.
 * rvn_graph_fetch_transitive: the marked ids in the order in which the reference's marked_edges set first receives them
 * (nodes ascending, jt, kt, c before its pair) - emplacing them in this order reproduces that set's iteration order - and
 * (tail & ~1, head & ~1) of the odd ids among them in the same order (2 x n_pairs values): what assemble.cc:58-65 feeds
 * the nodes' `transitive` sets.
 * rvn_graph_mark_long_edges: one weight per edge slot; marked[n_edges] (may be NULL) = 1 for an edge kt, and its pair,
 * of a node with two or more out-edges when another out-edge jt of that node has weight(jt) * 2 < weight(kt).
 * RVN_EINVAL: an id >= n_piles / n_nodes, pile_end < pile_begin, an overlap of type 3 or 4 on an invalid pile (the
 * reference would index nodes[-1]), an odd n_edges, an edge whose pair slot is empty, a strand other than 0 or 1, a NaN weight, 2^32
 * edges or more.
 * Empty inputs give empty tables. */
typedef struct rvn_graph rvn_graph;
int rvn_construct_assembly_graph(rvn_engine* e, const rvn_overlap* overlaps, uint64_t n_overlaps, uint32_t n_piles,
                                 const uint32_t* pile_begin, const uint32_t* pile_end, const uint16_t* median,
                                 const uint8_t* invalid, rvn_graph** out);
int rvn_graph_from_edges(rvn_engine* e, uint32_t n_nodes, uint64_t n_edges, const uint32_t* tail, const uint32_t* head,
                         const uint32_t* length, rvn_graph** out);
int rvn_graph_info(const rvn_graph* g, uint32_t* n_nodes, uint64_t* n_edges, uint64_t* n_live_edges);
int rvn_graph_fetch(const rvn_graph* g, int32_t* sequence_to_node, uint32_t* node_pile, uint16_t* node_coverage,
                    uint32_t* edge_tail, uint32_t* edge_head, uint32_t* edge_length, uint64_t* edge_overlap,
                    rvn_overlap* finalized);
int rvn_graph_mark_transitive(rvn_engine* e, rvn_graph* g, uint64_t* n_marked);
int rvn_graph_fetch_transitive(const rvn_graph* g, uint32_t* marked_in_insertion_order, uint32_t* transitive_pairs,
                               uint64_t* n_pairs);
int rvn_graph_mark_long_edges(rvn_engine* e, const rvn_graph* g, const double* weight, uint8_t* marked, uint64_t* n_marked);
void rvn_graph_destroy(rvn_graph* g);

/* Unitigs on the device (facade: include/raven_hip/unitigs.hpp): raven::CreateUnitigs
 * (RavenLib/src/common.cc:32-225, with the unitig constructor graph.cc:27-57) on the edge table as it stands after the
 * host's surgery, and GetUnitigs' selection (common.cc:227-252) as a device read set.  The chains are found by list
 * ranking, the sequences are a 2-bit gather out of the reads: no base of a unitig passes through the host.
 *
 * A TILING holds, per node, a list of segments (read, first base, length, strand) whose concatenation is the node's
 * sequence; strand 1 = the reverse complement of that stretch of the read.  `read` is the index of the read in the read
 * set the tiling was made for.
 * rvn_tiling_from_piles: node u = one segment (node_pile[u], pile_begin, pile_end - pile_begin, u & 1), with node_pile as
 * rvn_graph_fetch reports it and pile i = read i.
 * rvn_tiling_from_segments: the lists as the caller states them (CSR: segment_offsets[n_nodes + 1]).
 * rvn_tiling_fetch: every output may be NULL; node_length[n_nodes] = the nodes' lengths in bases.
 *
 * rvn_graph_create_unitigs: count / coverage per node of the graph (Node::count, Node::coverage), epsilon as the
 * reference's (42 in front of the layout, 0 in SalvagePlasmids and GetUnitigs), min_unitig_size = the reference's global
 * (9999).  The graph stays as it is; the result holds what the reference's loop collects before its single RemoveEdges:
 *   new nodes     id first_node + j (first_node = the graph's n_nodes), j in the order of the reference's factory calls:
 *                 nodes walked in ascending id, a chain and its paired chain created together when the first node of either
 *                 is met; even j = the unitig (the orientation that holds that node), j + 1 = its reverse-complement unitig.
 *                 Per new node: begin / end (after the epsilon trim), is_circular, count (summed in uint32), length in
 *                 bases, coverage ((coverage(begin) + coverage(end)) / 2 of the unitig, for both), is_unitig (count > 5 and
 *                 length > min_unitig_size), and the members in walk order (CSR member_offsets[n_new_nodes + 1]): begin ..
 *                 end of a linear chain, from the creating node on round a circular one.  A non-circular chain of fewer than
 *                 2 epsilon + 2 nodes (or of one node) makes nothing and consumes no id.
 *   marked        [n_edges] marked_edges as flags: the chain edges from begin to end, the in-edge of begin and the out-edge
 *                 of end where they exist, and the pairs of all of them.
 *   new edges     id first_edge + x (first_edge = the graph's n_edges), in factory order; per unitig with begin != end: the
 *                 in-edge's replacement, its pair, the out-edge's replacement, its pair; lengths as common.cc:136-159 in
 *                 uint32 arithmetic.
 *   sequences     per member but the last the first length(out-edge) bases of the member, then the whole of `end`; a
 *                 circular chain closes on its creating node and appends nothing.  The reverse-complement unitig is built
 *                 from the pair edges in the same way.  The new nodes' segment lists are APPENDED to the tiling: a later
 *                 call on the grown graph (rvn_graph_from_edges with n_nodes + n_new_nodes) finds them under their ids.
 * rvn_unitigs_fetch: every output may be NULL.
 * rvn_unitigs_as_reads: the new nodes' sequences as a read set like any other (ids 0 .. n - 1): RVN_UNITIGS_SELECTED = the
 * new nodes GetUnitigs would return (even id and is_unitig, in node order), RVN_UNITIGS_ALL = every new node.  Equal to
 * rvn_reads_upload_codes of the same sequences word for word.
 * rvn_tiling_as_reads: the same for any list of nodes of a tiling (nodes of earlier calls that a later one left standing).
 * RVN_EINVAL: a segment that names an unknown read, runs past its read or has a strand other than 0 or 1, offsets that
 * decrease, a node of 2^32 bases or more, a node that names an unknown pile; in rvn_graph_create_unitigs (the message names
 * the offending id) a chain edge longer than its tail's sequence, an edge table that is not pair-symmetric (tail[e ^ 1] !=
 * head[e] ^ 1 or head[e ^ 1] != tail[e] ^ 1), a unitig of 2^32 bases or more, a tiling with fewer (or more) nodes than the
 * graph, epsilon above 2^30, more than 2^31 nodes or 2^32 edge slots with the new ones; in the *_as_reads calls a node that
 * is not in the tiling, a read set other than the tiling's, an unknown selection.  A refused call leaves the tiling as it was.
 * Empty graphs give empty tables. */
typedef struct rvn_tiling rvn_tiling;
typedef struct rvn_unitigs rvn_unitigs;
enum { RVN_UNITIGS_SELECTED = 0, RVN_UNITIGS_ALL = 1 };
int rvn_tiling_from_piles(rvn_engine* e, const rvn_reads* reads, uint32_t n_nodes, const uint32_t* node_pile, uint32_t n_piles,
                          const uint32_t* pile_begin, const uint32_t* pile_end, rvn_tiling** out);
int rvn_tiling_from_segments(rvn_engine* e, const rvn_reads* reads, uint32_t n_nodes, const uint64_t* segment_offsets,
                             const uint32_t* segment_read, const uint32_t* segment_begin, const uint32_t* segment_length,
                             const uint8_t* segment_strand, rvn_tiling** out);
int rvn_tiling_info(const rvn_tiling* t, uint32_t* n_nodes, uint64_t* n_segments);
int rvn_tiling_fetch(const rvn_tiling* t, uint64_t* segment_offsets, uint32_t* segment_read, uint32_t* segment_begin,
                     uint32_t* segment_length, uint8_t* segment_strand, uint32_t* node_length);
void rvn_tiling_destroy(rvn_tiling* t);
int rvn_graph_create_unitigs(rvn_engine* e, const rvn_graph* g, rvn_tiling* t, const uint32_t* count, const uint16_t* coverage,
                             uint32_t epsilon, uint32_t min_unitig_size, rvn_unitigs** out);
int rvn_unitigs_info(const rvn_unitigs* u, uint32_t* first_node, uint32_t* n_new_nodes, uint64_t* n_members, uint64_t* first_edge,
                     uint64_t* n_new_edges);
int rvn_unitigs_fetch(const rvn_unitigs* u, uint32_t* begin, uint32_t* end, uint8_t* is_circular, uint32_t* count, uint32_t* length,
                      uint16_t* coverage, uint8_t* is_unitig, uint64_t* member_offsets, uint32_t* members, uint8_t* marked,
                      uint32_t* edge_tail, uint32_t* edge_head, uint32_t* edge_length);
void rvn_unitigs_destroy(rvn_unitigs* u);
int rvn_unitigs_as_reads(rvn_engine* e, const rvn_unitigs* u, const rvn_tiling* t, const rvn_reads* reads, int selection,
                         rvn_reads** out);
int rvn_tiling_as_reads(rvn_engine* e, const rvn_tiling* t, const rvn_reads* reads, const uint32_t* nodes, uint32_t n,
                        rvn_reads** out);

/* The similarity test of raven's RemoveBubbles (RavenLib/src/assemble.cc:225-281) without a base on the
 * host: the sequences of node PATHS as a device read set, and the reference's verdict on pairs of them.
 *
 * rvn_tiling_paths_as_reads: path p has the members path_node[path_offsets[p] .. path_offsets[p + 1]).  Its sequence is,
 * for every member but the last, the first min(path_label[i], length(node)) bases of the node (Edge::Label() as
 * biosoup::NucleicAcid::InflateData(0, length) returns it: a length beyond the sequence gives the whole sequence, so an
 * edge length that has wrapped in 32 bits is NOT refused here; label 0 contributes nothing), then the whole last node,
 * whose label is ignored.  The result is a read set like any other (ids 0 .. n_paths - 1), equal to
 * rvn_reads_upload_codes of the same strings word for word.  The paths' tilings are temporary: the tiling is not changed.
 * RVN_EINVAL (the message names the offender): a node that is not in the tiling, a read set other than the tiling's, an
 * empty path, offsets that decrease, a path of 2^32 bases or more.  n_paths == 0 gives an empty read set.
 *
 * rvn_path_similarity_batch: `paths` is such a read set (or any other), a pair names two of its reads.  With l, r the
 * two lengths and mx = max(l, r), similar[i] = 1 exactly when the reference goes on to pop the bubble:
 *   !(min(l, r) < mx * min_ratio)      (the product formed in double, assemble.cc:267)  and
 *   !(1 - d / (double)mx < min_ratio)  with d the exact global unit-cost edit distance (edlibAlign, default configuration).
 * The second rule is decided by a bounded sweep per pair at kmax = the largest x that still passes it (one sweep where the
 * wave ring of the edit-distance stage holds kmax); pairs the length rule rejects are never swept.  distance (may be NULL): the exact distance where it is <= kmax, 0xFFFFFFFE where it is
 * above, 0xFFFFFFFF for a pair rejected by the length rule.  min_ratio is the reference's 0.8.  A threshold beyond the
 * wave ring (8 064: paths of 40 kb and more at 0.8) is swept by a ring over the lanes of one workgroup (engine option
 * ed_wide_lanes; up to 65 408; one sweep, at kmax or at the ring's capacity), what lies beyond that by the full sweep:
 * exact at any size.
 * RVN_EINVAL: a pair that names an unknown read, a path of length 0 (the reference's arithmetic on it is 0 / 0), a
 * min_ratio that is not a number.  Every pair is checked first: a refused call has written nothing. */
typedef struct rvn_path_pair {
  uint32_t lhs_path, rhs_path;
} rvn_path_pair;
int rvn_tiling_paths_as_reads(rvn_engine* e, const rvn_tiling* t, const rvn_reads* reads, uint32_t n_paths,
                              const uint64_t* path_offsets, const uint32_t* path_node, const uint32_t* path_label, rvn_reads** out);
int rvn_path_similarity_batch(rvn_engine* e, const rvn_reads* paths, const rvn_path_pair* pairs, uint32_t n_pairs, double min_ratio,
                              uint8_t* similar, uint32_t* distance);

/* printEdgeSimilarity of the CSV emitters (RavenLib/src/graph_repr.cc:247-258 in PrintCsv, :358-369 in getCsv; DESIGN.md
 * 3.15; facade: include/raven_hip/graph_repr.hpp) without a base on the host: slices of node sequences as a device read
 * set, and the reference's score for every edge of an edge table.
 *
 * rvn_tiling_slices_as_reads: read i of the result is biosoup::NucleicAcid::InflateData(begin[i], length[i]) of node[i]:
 * bases [begin, begin + min(length, length(node) - begin)), nothing when begin >= length(node) (a read of length 0).  A
 * read set like any other (ids 0 .. n - 1), equal to rvn_reads_upload_codes of the same strings word for word.
 * RVN_EINVAL, found before the first launch: a node that is not in the tiling, a read set other than the tiling's, slices
 * of 2^32 packed words or more in total.  A refused call leaves the tiling as it was.  n == 0 gives an empty read set.
 *
 * rvn_graph_edge_similarity: per edge slot e with L = the edge's length as stored,
 *   lhs_length[e] = length(tail) > L ? length(tail) - L : 0     (tail.InflateData(L); a wrapped L gives 0, it is not refused)
 *   rhs_length[e] = min(lhs_length[e], length(head))            (head.InflateData(0, lhs.size()))
 *   distance[e]   = the exact global unit-cost edit distance of the two slices (edlibAlign, default configuration; no
 *                   threshold, any size; the other slice's length when one is empty)
 *   score[e]      = 1 - distance / (double)lhs_length, formed in double on the host as graph_repr.cc:254 writes it: NaN for
 *                   a live edge whose lhs is empty (0 / 0.)
 * An empty slot (tail 0xFFFFFFFF) gets 0, 0, 0xFFFFFFFF and NaN.  Every output has n_edges entries and may be NULL.
 * An edge whose two nodes are one segment each is swept as two spans of the reads themselves; the others' slices are
 * packed into scratch of the engine, a chunk at a time (engine option edge_slices_budget_kb).  A distance beyond the wave
 * ring (8 064) is swept by the workgroup ring (engine option ed_wide_lanes; up to 65 408), what lies beyond by the full sweep.
 * RVN_EINVAL: a tiling whose node count is not the graph's, a read set other than the tiling's.  An empty graph writes
 * nothing. */
int rvn_tiling_slices_as_reads(rvn_engine* e, const rvn_tiling* t, const rvn_reads* reads, uint32_t n, const uint32_t* node,
                               const uint32_t* begin, const uint32_t* length, rvn_reads** out);
int rvn_graph_edge_similarity(rvn_engine* e, const rvn_graph* g, const rvn_tiling* t, const rvn_reads* reads,
                              uint32_t* lhs_length, uint32_t* rhs_length, uint32_t* distance, double* score);

/* Tuning a deployment may set; -1 restores the built-in default of any option (so does 0, except for poa_rows_min_windows).
 * No option changes an overlap list, a pile or a layer table; poa_rows_min_windows chooses which window-consensus kernel
 * makes the first attempt, and the two agree on 19 998 of 20 000 C4-like windows, not on every one: a
 * consensus is reproducible for a fixed value of that option, not across values.  The product library reads
 * NO environment variable that alters what a call computes or how it is scheduled (the only ones it reads at all:
 * RVN_EDLIB_DEVICE of the edlibAlign drop-in, RVN_DEVICES of include/raven_hip/multi_gpu.hpp — which device); debugging
 * switches exist only in libraven_hip_test.so (built with -DRVN_DEBUG_KNOBS).  Options:
 *   nw_budget_mb       alignment-path stage: HBM for the stored band words (default: a quarter of the free memory, <= 64 GB)
 *   nw_group_walk      alignment-path stage: which walk a launch takes — 1 a lane per alignment, 2 a group of sixteen lanes per
 *                      alignment, 3 a lane per alignment with half-size strips, otherwise (default) the group for launches of at
 *                      most 8 192 alignments and the half-size strips beyond 65 536; same records either way
 *   nw_stripe_lanes    alignment-path stage: the widest ring of one sweep, in lanes (1 .. 64; default 64, a whole wave).  A band
 *                      wider than that ring is swept in stripes of that many lanes (at most 8 rings: 262 144 rows by default);
 *                      smaller values force striping on small inputs; same records either way
 *   ed_wide_lanes      rvn_path_similarity_batch, rvn_graph_edge_similarity: lanes of the workgroup ring that sweeps thresholds beyond the wave ring (64 .. 512
 *                      in steps of 64; default 512 = thresholds up to 65 408); 1 = no such sweep, those pairs take the usual
 *                      route to the full sweep; smaller rings reach their limit on small inputs; same verdicts and distances
 *                      either way.  Any other value is refused
 *   edge_slices_budget_kb  rvn_graph_edge_similarity: HBM, in KB, for the packed slices of one chunk of the edges whose nodes have
 *                      several segments (default: a quarter of the largest free block the arena, or the driver, reports;
 *                      a chunk always holds one edge at least); same values either way
 *   index_direct_min_keys  index: distinct values from which all 4^k possible values are addressed directly (an 8-GB table at
 *                      k = 15, one cache line per probe; default 8 388 608; 1 = every index with k <= 15); same matches either way
 *   poa_rows_min_windows  window-consensus stage: smallest batch that starts with the rows-on-lanes kernel (default 8 192;
 *                      0 means every batch, -1 the default)
 *   io_threads, io_slab_mb, io_ring, io_zlib   rvn_reads_load: inflate threads, page-locked slab size, slabs in flight,
 *                      != 0: zlib instead of this library's own inflate on a single gzip member
 *   arena_mb, arena_margin_mb, no_arena, release_always   the device arena behind the scratch buffers
 *   polish_sketch_cache_mb  polishing rounds: HBM for the reads' sketch kept from one round to the next (the reads do not change
 *                      between rounds; default an eighth of the device, 0 = recompute every round)
 *   polish_join        != 0: a round maps by sorting the reads' minimizers with the targets' and streaming the runs instead of
 *                      probing the targets' index — same overlaps, slower at the metric's size
 * previous (may be NULL) receives the value the option had (its default's value when it was at the default).  RVN_EINVAL:
 * unknown name, a value below -1, io_ring == 1 (a ring needs two slabs), an ed_wide_lanes that is neither 1 nor a multiple of
 * 64 from 64 to 512. */
int rvn_engine_set_option(rvn_engine* e, const char* name, int64_t value, int64_t* previous);

/* Kept for source compatibility: a round no longer has a host cutting stage to overlap with the POA, all windows
 * of a call are one device batch.  Stores the value, returns the previous one; results never depended on it. */
uint64_t rvn_polish_set_chunk_windows(rvn_engine* e, uint64_t windows);

/* The window layers of the last rvn_polish_round / _range call, as racon would have added them (steps 1-4 of its
 * round: mapping, best overlap, alignment path, breakpoints, layer rules — all integer work, compared bit-exactly with
 * the CPU restatement by the tests): 7 uint32 per layer {global window, read index, first base in the oriented read,
 * bases, begin, end, reverse-complemented}, windows in order, layers in racon's order, layers dropped by the
 * mean-quality filter left out.  out == NULL or cap too small: only *n is set. */
int rvn_polish_fetch_layers(rvn_engine* e, uint32_t* out, uint64_t cap, uint64_t* n);

/* reads used per target (their best overlap passed the error filter) in the last rvn_polish_round call: the RC:i:
 * tag racon writes next to XC:f: */
int rvn_polish_target_reads(const rvn_engine* e, uint32_t* counts, uint32_t n_targets);

/* shader-clock cycles summed over all windows of the last rvn_poa_consensus_batch call, per phase:
 * {subgraph, NW matrix, traceback, AddAlignment, order rebuild, consensus} */
void rvn_poa_phase_cycles(const rvn_engine* e, uint64_t out[6]);

/* DP work of the banded window kernel since the last rvn_engine_reset_stats: {cells of the full-matrix equivalent =
 * graph rows x layer length over every layer alignment (what spoa's NW computes; windows repeated with a wider band
 * count again), cells inside the computed bands, POA batches}.  bench.py prices the kernel's roofline with it. */
void rvn_poa_work(const rvn_engine* e, uint64_t out[3]);

/* Which window kernel rvn_poa_consensus_batch / rvn_polish_round use: 0 (default) = the rows-on-lanes kernel with a
 * 32-column band (poa4.hip); windows whose alignment touches the band edge, or whose graph is beyond that kernel's
 * limits, are repeated by the one-row-per-iteration kernel (poa2.hip) with 64, then 128 and 256 columns, and what is
 * left (or beyond a limit) by the full-matrix kernel; 1 = full-matrix kernel only; 2 / 3 / 4 = 64- / 128- / 256-column
 * band only (flagged windows come back with status 8); 9 = poa4.hip only.  Returns the previous mode. */
int rvn_poa_set_mode(rvn_engine* e, int mode);
/* mode 0: windows of the last batch repeated with the 128-column band (wide) / that needed more than that (fallback:
 * 256 columns or the full matrix) */
uint32_t rvn_poa_fallback_windows(const rvn_engine* e);
uint32_t rvn_poa_wide_windows(const rvn_engine* e);
/* mode 0: windows of the last batch that the 32-column first attempt (poa4.hip) handed on to the 64-column kernel */
uint32_t rvn_poa_narrow_windows(const rvn_engine* e);

/* ---- introspection used by the parity tests and bench.py ------------------------------------- */
/* sketch of reads [first,last) == ram Minimize(sequence, minhash) per read; values widened to u64 */
int rvn_engine_sketch(rvn_engine* e, const rvn_reads* r, uint32_t first, uint32_t last, int minhash,
                      uint64_t* count);
int rvn_engine_sketch_fetch(rvn_engine* e, uint64_t* values, uint64_t* origins, uint32_t* read_offsets);
/* sorted index content: (value, origin) pairs in index order; count = minimizers in the index */
int rvn_engine_index_size(const rvn_engine* e, uint64_t* n_minimizers, uint64_t* n_keys);
int rvn_engine_index_fetch(rvn_engine* e, uint64_t* values, uint64_t* origins);
/* counters since the last reset: {index_bases, index_minimizers, index_keys, query_bases,
 * query_minimizers, matches, overlaps(Map outputs), intervals} */
int rvn_engine_counters(const rvn_engine* e, uint64_t out[8]);
/* accumulated device milliseconds per stage (HIP events on the engine's stream) and launch counts */
int rvn_engine_num_stages(void);
const char* rvn_engine_stage_name(int stage);
int rvn_engine_stage_ms(const rvn_engine* e, double* ms, uint64_t* launches, int n);
void rvn_engine_reset_stats(rvn_engine* e);
void rvn_engine_set_timing(rvn_engine* e, int enabled);
/* per-kernel-site device time: HIP events recorded on the engine's stream around every launch of the
 * site (no host synchronisation while recording); rvn_engine_kernel_ms synchronises and accumulates. */
void rvn_engine_set_kernel_timing(rvn_engine* e, int enabled);
int rvn_engine_num_kernel_sites(void);
const char* rvn_engine_kernel_site_name(int site);
int rvn_engine_kernel_ms(rvn_engine* e, double* ms, uint64_t* launches, int n);

/* The host-side test hooks (rvn_test_*, rvn_poa_banded_emulate) are NOT part of this library: include/raven_hip_test.h,
 * libraven_hip_test.so. */

#ifdef __cplusplus
}
#endif
#endif /* RAVEN_HIP_H_ */
