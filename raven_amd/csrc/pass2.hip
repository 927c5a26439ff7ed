// pass2.hip — the second mapping pass and the identity filters of the overlap phase on the device:
//   raven::FindOverlapsAndRepetetiveRegions   RavenLib/src/construct.cc:316-491  (second_pass)
//   identity filter of ResolveContainedReads   RavenLib/src/construct.cc:162-217  (identity_filter_lists)
// with the per-overlap rules of RavenLib/src/overlap_utils.cc (overlap_rules.h) and Pile::AddKmers (pile.cc:64-120).
//
// Second pass, per index batch of 2^30 bases of VALID reads (valid first, by id — construct.cc:324-359):
//   Minimize(batch) without minhash, Filter(freq), Map(read, true, true, false, &filtered) of every valid read up to the
//   batch end (one device pass), AddKmers of the filtered positions into the k-mer cells kept in HBM, [identity != 0:
//   OverlapUpdate -> batched exact edit distance of the two spans -> drop below the threshold], then the merge of
//   construct.cc:430-455 in Map-output order: OverlapUpdate, GetOverlapType, containment flags, survivors (type 3 / 4)
//   appended to the result list.  After the last batch: consecutive overlaps of the same read pair keep the longer one
//   (the first of equal length), contained piles become invalid, the list is re-checked with OverlapUpdate.
// Every step is a flat kernel over all overlaps of a batch; order-dependent steps (the de-duplication of consecutive
// pairs) work on the compacted list, whose order is the reference's serial order.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "engine.h"
#include "kmer.h"
#include "lowcomplexity.h"
#include "overlap_rules.h"
#include "wave.h"
#ifdef RVN_TEST_HOOKS
#include "../../include/raven_hip_test.h"
#include "abi.h"
#endif

namespace rvn {

namespace {

constexpr u32 kPSS2 = 4;

// one thread per output word: words of read i of the subset come from read src[i] of the full set
__global__ void gather_reads_kernel(const u64* __restrict__ in_packed, const u64* __restrict__ in_word_off,
                                    const u32* __restrict__ src, const u64* __restrict__ out_word_off, u32 n, u64 n_words,
                                    u64* __restrict__ out_packed) {
  const u64 wi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (wi >= n_words) return;
  u32 lo = 0, hi = n;
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (out_word_off[mid] <= wi) lo = mid;
    else hi = mid;
  }
  out_packed[wi] = in_packed[in_word_off[src[lo]] + (wi - out_word_off[lo])];
}

// Pile::AddKmers on the `filtered` flags of a Map batch: one thread per query minimizer
__global__ void add_kmers_flags_kernel(const u64* __restrict__ packed, const u64* __restrict__ word_off,
                                       const u8* __restrict__ filtered, const u64* __restrict__ org,
                                       const u32* __restrict__ read_off, u32 n_reads, u64 n_query, u32 k,
                                       const u64* __restrict__ kmers_off, u8* __restrict__ kmers) {
  const u64 q = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (q >= n_query || !filtered[q]) return;
  u32 lo = 0, hi = n_reads;  // read of this minimizer: last r with read_off[r] <= q
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (read_off[mid] <= q) lo = mid;
    else hi = mid;
  }
  const u32 p = static_cast<u32>(org[q]) >> 1;
  const u64* w = packed + word_off[lo];
  const u64 mask = k >= 32 ? ~0ULL : ((1ULL << (2 * k)) - 1);
  const u32 bit = 2 * p;
  const u64 x = extract_bits(w[bit >> 6], w[(bit >> 6) + 1], bit & 63, mask);
  u8 codes[32];
  for (u32 i = 0; i < k; ++i) codes[i] = static_cast<u8>((x >> (2 * i)) & 3);
  if (lc_kmer_passes(codes, k)) kmers[kmers_off[lo] + (p >> kPSS2)] = 1;
}

// OverlapUpdate of every overlap, in place: updated coordinates + ok flag
__global__ void update_kernel(Overlap* __restrict__ ovl, u64 n, const PileRegion* __restrict__ regions,
                              u8* __restrict__ ok) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Overlap o = ovl[i];
  const bool good = overlap_update(o, regions[o.lhs_id], regions[o.rhs_id]);
  ovl[i] = o;
  ok[i] = good ? 1 : 0;
}

struct EdPairRec {
  u32 a_idx, a_begin, a_len, b_idx, b_begin, b_len, strand, pad;
};

// edlibAlign(lhs span, rhs span [reverse-complemented on the opposite strand]) pairs of the overlaps that survived the update
// (the reference's keep rule on a distance: identity_keeps, overlap_rules.h).
// Also the largest distance that still passes the filter (kmax): the edit-distance stage then needs ONE sweep at that
// threshold per pair — "exact distance if <= kmax, else above" decides the overlap exactly as the unbounded distance would.
__global__ void ed_pairs_kernel(const Overlap* __restrict__ ovl, const u8* __restrict__ ok, const u32* __restrict__ slot,
                                u64 n, const u32* __restrict__ index_of, double identity, EdPairRec* __restrict__ pairs,
                                u32* __restrict__ kmax) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n || !ok[i]) return;
  const Overlap o = ovl[i];
  const u32 a = o.lhs_end - o.lhs_begin, b = o.rhs_end - o.rhs_begin;
  const u32 ai = index_of ? index_of[o.lhs_id] : o.lhs_id, bi = index_of ? index_of[o.rhs_id] : o.rhs_id;
  pairs[slot[i]] = EdPairRec{ai, o.lhs_begin, a, bi, o.rhs_begin, b, o.strand ? 1u : 0u, 0u};
  const u32 maxlen = a > b ? a : b;
  kmax[slot[i]] = identity_kmax(maxlen, identity);
}

// score = 1 - distance / max(length) in double; overlaps below the identity threshold lose their ok flag
__global__ void identity_keep_kernel(const Overlap* __restrict__ ovl, u8* __restrict__ ok, const u32* __restrict__ slot,
                                     u64 n, const u32* __restrict__ dist, double identity) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n || !ok[i]) return;
  const Overlap o = ovl[i];
  const u32 a = o.lhs_end - o.lhs_begin, b = o.rhs_end - o.rhs_begin;
  // dist is exact up to the pair's kmax and 0xFFFFFFFE above it: the rule gives the same answer either way
  const double score = 1. - static_cast<double>(dist[slot[i]]) / static_cast<double>(a > b ? a : b);
  if (score < identity) ok[i] = 0;
}

// the merge of construct.cc:430-455 without its order-dependent part: OverlapUpdate (a no-op on an already updated
// overlap), type, containment flags; keep[i] = goes to the result list (type 3 / 4)
__global__ void classify_kernel(Overlap* __restrict__ ovl, const u8* __restrict__ ok, u64 n,
                                const PileRegion* __restrict__ regions, u8* __restrict__ contained,
                                u8* __restrict__ keep) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u8 k = 0;
  if (ok[i]) {
    Overlap o = ovl[i];
    const PileRegion L = regions[o.lhs_id], R = regions[o.rhs_id];
    if (overlap_update(o, L, R)) {
      const u32 type = overlap_type(o, L, R);
      if (type == 1) contained[o.lhs_id] = 1;
      else if (type == 2) contained[o.rhs_id] = 1;
      else if (type >= 3) {
        ovl[i] = o;
        k = 1;
      }
    }
  }
  keep[i] = k;
}

__global__ void compact_kernel(const Overlap* __restrict__ in, const u8* __restrict__ keep, const u32* __restrict__ slot,
                               u64 n, Overlap* __restrict__ out) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n && keep[i]) out[slot[i]] = in[i];
}

// consecutive overlaps of the same (lhs, rhs) pair: the survivor is the first one of maximal length
// (construct.cc:444-453: replaced only when strictly longer).  One thread per run head.
__global__ void dedup_kernel(const Overlap* __restrict__ ovl, u64 n, u8* __restrict__ keep) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Overlap o = ovl[i];
  if (i > 0 && ovl[i - 1].lhs_id == o.lhs_id && ovl[i - 1].rhs_id == o.rhs_id) return;  // not a run head
  u64 best = i;
  u32 best_len = overlap_length(o);
  keep[i] = 0;
  for (u64 j = i + 1; j < n && ovl[j].lhs_id == o.lhs_id && ovl[j].rhs_id == o.rhs_id; ++j) {
    keep[j] = 0;
    const u32 l = overlap_length(ovl[j]);
    if (best_len < l) {
      best_len = l;
      best = j;
    }
  }
  keep[best] = 1;
}

__global__ void merge_invalid_kernel(PileRegion* __restrict__ regions, const u8* __restrict__ contained, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && contained[i]) regions[i].invalid = 1;
}

}  // namespace

KeptSlots kept_slots(Engine& e, const u8* d_keep, u64 n, DevBuf& slot) {
  if (n == 0) return {nullptr, 0};
  u32* d_slot = slot.get<u32>(n + 2);
  exclusive_scan_u8_u32(d_keep, d_slot, n, e.scratch.scan_tmp, e.stream);
  return {d_slot, read_back(e, d_slot + n, 4)};
}

void compact_overlaps(Engine& e, const Overlap* d_in, const u8* d_keep, const u32* d_slot, u64 n, Overlap* d_out) {
  if (n == 0) return;
  compact_kernel<<<div_up(n, 256), 256, 0, e.stream>>>(d_in, d_keep, d_slot, n, d_out);
  RVN_LAUNCH_CHECK();
}

u64 compact_overlap_list(Engine& e, DevBuf& list, u64 n, const u8* d_keep, DevBuf& slot, DevBuf& spare) {
  if (n == 0) return 0;
  const KeptSlots ks = kept_slots(e, d_keep, n, slot);
  compact_overlaps(e, list.as<Overlap>(), d_keep, ks.slot, n, spare.get<Overlap>(ks.kept + 1));
  list.swap(spare);
  return ks.kept;
}

// OverlapUpdate + [identity] on a device list; ok flags out.  regions indexed by read id, index_of: id -> index in r
// (nullptr: the ids are the indices).
void update_and_identity(Engine& e, const ReadsDev& r, Overlap* d_ovl, u64 n, const PileRegion* d_regions,
                         const u32* d_index_of, double identity, u8* d_ok) {
  if (n == 0) return;
  hipStream_t s = e.stream;
  update_kernel<<<div_up(n, 256), 256, 0, s>>>(d_ovl, n, d_regions, d_ok);
  RVN_LAUNCH_CHECK();
  if (identity == 0) return;
  const KeptSlots ks = kept_slots(e, d_ok, n, e.p2.slot);
  const u32* d_slot = ks.slot;
  const u64 np = ks.kept;
  if (np == 0) return;
  if (np >= 0xFFFFFFFFULL) throw std::invalid_argument("[raven_hip] identity filter: too many pairs in one batch");
  EdPairRec* d_pairs = e.p2.pairs.get<EdPairRec>(np + 1);
  u32* d_dist = e.p2.dist.get<u32>(2 * (np + 1));
  u32* d_kmax = d_dist + np + 1;
  ed_pairs_kernel<<<div_up(n, 256), 256, 0, s>>>(d_ovl, d_ok, d_slot, n, d_index_of, identity, d_pairs, d_kmax);
  RVN_LAUNCH_CHECK();
  edit_distance_dev(e, r, reinterpret_cast<const u32*>(d_pairs), static_cast<u32>(np), d_dist, d_kmax);
  identity_keep_kernel<<<div_up(n, 256), 256, 0, s>>>(d_ovl, d_ok, d_slot, n, d_dist, identity);
  RVN_LAUNCH_CHECK();
}

PileRegion* upload_pile_regions(Engine& e, DevBuf& b, const u32* h_begin, const u32* h_end, const u8* h_invalid, u32 n) {
  std::vector<PileRegion> reg(n);
  for (u32 i = 0; i < n; ++i) reg[i] = PileRegion{h_begin[i], h_end[i], h_invalid[i] ? 1u : 0u};
  PileRegion* d = upload(b, reg.data(), n, e.stream);
  RVN_HIP(rvn_stream_sync(e.stream));  // reg is gone on return
  return d;
}

// Device copy of the reads `src` (indices into R, increasing) as a read set of its own: ids = the original indices
void reads_subset(Engine& e, const ReadsDev& R, const std::vector<u32>& src, ReadsDev& V) {
  hipStream_t s = e.stream;
  const u32 n = static_cast<u32>(src.size());
  V.n = n;
  V.h_word_off.assign(static_cast<size_t>(n) + 1, 0);
  V.h_len.resize(n);
  V.h_id.resize(n);
  V.total_bases = 0;
  for (u32 i = 0; i < n; ++i) {
    V.h_len[i] = R.h_len[src[i]];
    V.h_id[i] = R.h_id[src[i]];
    V.total_bases += V.h_len[i];
    V.h_word_off[i + 1] = V.h_word_off[i] + (R.h_word_off[src[i] + 1] - R.h_word_off[src[i]]);
  }
  V.ids_are_indices = false;
  V.n_words = V.h_word_off[n];
  u64* d_packed = V.packed.get<u64>(V.n_words + 2);
  u64* d_wo = V.word_off.get<u64>(static_cast<size_t>(n) + 1);
  u32* d_len = V.len.get<u32>(static_cast<size_t>(n) + 1);
  u32* d_id = V.id.get<u32>(static_cast<size_t>(n) + 1);
  u32* d_src = e.p2.slot.get<u32>(static_cast<size_t>(n) + 2);
  RVN_HIP(hipMemcpyAsync(d_wo, V.h_word_off.data(), (static_cast<size_t>(n) + 1) * 8, hipMemcpyHostToDevice, s));
  if (n) {
    RVN_HIP(hipMemcpyAsync(d_len, V.h_len.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, s));
    RVN_HIP(hipMemcpyAsync(d_id, V.h_id.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, s));
    RVN_HIP(hipMemcpyAsync(d_src, src.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, s));
    if (V.n_words) {
      gather_reads_kernel<<<div_up(V.n_words, 256), 256, 0, s>>>(R.packed.as<u64>(), R.word_off.as<u64>(), d_src, d_wo, n,
                                                                 V.n_words, d_packed);
      RVN_LAUNCH_CHECK();
    }
  }
  RVN_HIP(hipMemsetAsync(d_packed + V.n_words, 0, 16, s));
  RVN_HIP(rvn_stream_sync(s));
  reads_build_tiles(e, V);
}

namespace {
// dst[i] |= src[i] (the containment flags of several ranks' second passes)
__global__ void or_bytes_kernel(u8* __restrict__ dst, const u8* __restrict__ src, u64 n) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) dst[i] |= src[i];
}
}  // namespace

void or_bytes(Engine& e, u8* d_dst, const u8* d_src, u64 n) {
  if (n == 0) return;
  or_bytes_kernel<<<div_up(n, 256), 256, 0, e.stream>>>(d_dst, d_src, n);
  RVN_LAUNCH_CHECK();
  RVN_HIP(rvn_stream_sync(e.stream));
}

// Stages of raven::FindOverlapsAndRepetetiveRegions (construct.cc:316-491) shared by the single engine (second_pass) and
// the device group (group.hip): prepare (valid reads, k-mer cell offsets, index batches), one index batch with the
// Map of a range of query reads, finish (de-duplication, invalidation, final OverlapUpdate sweep).
// R = all reads with ids[i] == i.
void second_pass_prepare(Engine& e, const ReadsDev& R, const u32* h_begin, const u32* h_end, const u8* h_invalid,
                         u64 batch_bases, Pass2State& out, Pass2Prep& P) {
  hipStream_t s = e.stream;
  const u32 n = R.n;
  out.n = n;
  out.n_overlaps = 0;
  P.batches.clear();
  P.d_regions = upload_pile_regions(e, e.p2.regions, h_begin, h_end, h_invalid, n);
  u8* d_contained = out.contained.get<u8>(static_cast<size_t>(n) + 16);
  RVN_HIP(hipMemsetAsync(d_contained, 0, static_cast<size_t>(n) + 16, s));
  // valid reads first, by id (construct.cc:324-349); index_of: id -> position among the valid reads
  P.valid.clear();
  std::vector<u32> index_of(n, 0xFFFFFFFFu);
  out.h_kmers_off.assign(static_cast<size_t>(n) + 1, 0);
  for (u32 i = 0; i < n; ++i) {
    if (!h_invalid[i]) {
      index_of[i] = static_cast<u32>(P.valid.size());
      P.valid.push_back(i);
      out.h_kmers_off[i + 1] = out.h_kmers_off[i] + (static_cast<u64>(R.h_len[i]) >> kPSS2) + 1;
    } else {
      out.h_kmers_off[i + 1] = out.h_kmers_off[i];
    }
  }
  out.kmers_total = out.h_kmers_off[n];
  u8* d_kmers = out.kmers.get<u8>(out.kmers_total + 16);
  RVN_HIP(hipMemsetAsync(d_kmers, 0, out.kmers_total + 16, s));
  const u32 nv = static_cast<u32>(P.valid.size());
  P.h_v_kmers_off.assign(static_cast<size_t>(nv) + 1, out.kmers_total);
  for (u32 i = 0; i < nv; ++i) P.h_v_kmers_off[i] = out.h_kmers_off[P.valid[i]];
  // construct.cc:343-349: `s` is the position of the FIRST INVALID pile after the valid-first sort and stays 0 when no
  // pile is invalid at all — the reference then maps nothing and overlaps.back() stays empty.  Reproduced on purpose
  // (results identical to the reference's on the same input); real read sets always have contained, hence invalid, piles.
  P.sv = nv == n ? 0u : nv;
  if (P.sv == 0) {
    if (nv == n && n > 0)  // (say so: an empty second pass otherwise looks like "no overlaps found")
      std::fprintf(stderr, "[raven_hip] second pass: every pile is valid, so nothing is mapped — the reference's behaviour "
                           "(construct.cc:343-349), reproduced on purpose\n");
    RVN_HIP(rvn_stream_sync(s));
    return;
  }
  const u32 sv = P.sv;
  reads_subset(e, R, P.valid, P.V);
  P.d_index_of = upload(e.p2.index_of, index_of.data(), n, s);
  P.d_v_kmers_off = upload(e.p2.kmers_off, P.h_v_kmers_off.data(), static_cast<size_t>(sv) + 1, s);
  RVN_HIP(rvn_stream_sync(s));
  // index batches of batch_bases valid bases: [first, last) of the valid reads
  u64 bytes = 0;
  for (u32 i = 0, j = 0; i < sv; ++i) {
    bytes += P.V.h_len[i];
    if (i != sv - 1 && bytes < batch_bases) continue;
    bytes = 0;
    P.batches.emplace_back(j, i + 1);
    j = i + 1;
  }
}

// What follows the Map of the query reads [q_first, q_last) in an index batch: `mo` is Map's output for them (overlaps in
// (query read, emission) order, `filtered` flags of the query sketch, which is e.sketch.query_sketch).  AddKmers of the
// filtered positions, OverlapUpdate, the identity filter, type, containment flags, survivors appended to out.ovl.
// Returns the number appended.
u64 second_pass_merge(Engine& e, Pass2Prep& P, u32 q_first, u32 q_last, const MapOut& mo, u32 kmer_len, double identity,
                      Pass2State& out) {
  hipStream_t s = e.stream;
  const ReadsDev& V = P.V;
  // Pile::AddKmers(filtered, kmer_len, sequence) of every mapped read (construct.cc:382)
  if (mo.n_query) {
    RVN_KLAUNCH(kKAddKmers, add_kmers_flags_kernel<<<div_up(mo.n_query, 256), 256, 0, s>>>(
                                V.packed.as<u64>(), V.word_off.as<u64>() + q_first, mo.filtered.as<u8>(),
                                e.sketch.query_sketch.org.as<u64>(), e.sketch.query_sketch.read_off.as<u32>(), q_last - q_first, mo.n_query,
                                kmer_len, P.d_v_kmers_off + q_first, out.kmers.as<u8>()));
  }
  const u64 O = mo.n_overlaps;
  if (O == 0) return 0;
  const u64 acc_n = out.n_overlaps;
  Overlap* d_ovl = mo.ovl.as<Overlap>();
  u8* d_ok = e.p2.ok.get<u8>(O + 16);
  u8* d_keep = e.p2.keep.get<u8>(O + 16);
  update_and_identity(e, V, d_ovl, O, P.d_regions, P.d_index_of, identity, d_ok);
  classify_kernel<<<div_up(O, 256), 256, 0, s>>>(d_ovl, d_ok, O, P.d_regions, out.contained.as<u8>(), d_keep);
  RVN_LAUNCH_CHECK();
  const KeptSlots ks = kept_slots(e, d_keep, O, e.p2.slot);
  const u64 m = ks.kept;
  if (m == 0) return 0;
  // append to the result list
  out.ovl.grow_keeping(acc_n * sizeof(Overlap), (acc_n + m + 1) * sizeof(Overlap), s);
  compact_overlaps(e, d_ovl, d_keep, ks.slot, O, out.ovl.as<Overlap>() + acc_n);
  out.n_overlaps = acc_n + m;
  return m;
}

// Index batch [first, last) of the valid reads; the query reads [q_first, q_last) (inside [0, last)) are mapped against it
// (the reference maps all of [0, last): construct.cc:362-383), their k-mer cells filled, their overlaps updated,
// identity-filtered, classified and appended to out.ovl.  Returns the number appended.
u64 second_pass_batch(Engine& e, Pass2Prep& P, u32 first, u32 last, u32 q_first, u32 q_last, double freq, u32 kmer_len,
                      double identity, Pass2State& out) {
  if (q_first >= q_last) return 0;
  const ReadsDev& V = P.V;
  engine_minimize(e, V, first, last, false);
  index_filter(e, freq);
  MapOut& mo = e.map.out;
  map_batch(e, V, q_first, q_last, true, true, false, true, mo);
  e.c_intervals += mo.n_intervals;
  return second_pass_merge(e, P, q_first, q_last, mo, kmer_len, identity, out);
}

// After the last batch, on the list in the reference's merge order: consecutive overlaps of the same pair keep the longer
// one (construct.cc:444-453), contained piles become invalid (:466-470) in d_regions, the list is re-checked (:472-480).
void second_pass_finish(Engine& e, PileRegion* d_regions, Pass2State& out) {
  hipStream_t s = e.stream;
  u64 acc_n = out.n_overlaps;
  if (acc_n) {
    u8* d_keep = e.p2.keep.get<u8>(acc_n + 16);
    RVN_HIP(hipMemsetAsync(d_keep, 1, acc_n, s));
    dedup_kernel<<<div_up(acc_n, 256), 256, 0, s>>>(out.ovl.as<Overlap>(), acc_n, d_keep);
    RVN_LAUNCH_CHECK();
    acc_n = compact_overlap_list(e, out.ovl, acc_n, d_keep, e.p2.slot, e.p2.tmp_ovl);
  }
  if (out.n) {
    merge_invalid_kernel<<<div_up(out.n, 256), 256, 0, s>>>(d_regions, out.contained.as<u8>(), out.n);
    RVN_LAUNCH_CHECK();
  }
  if (acc_n) {
    u8* d_ok = e.p2.ok.get<u8>(acc_n + 16);
    update_kernel<<<div_up(acc_n, 256), 256, 0, s>>>(out.ovl.as<Overlap>(), acc_n, d_regions, d_ok);
    RVN_LAUNCH_CHECK();
    acc_n = compact_overlap_list(e, out.ovl, acc_n, d_ok, e.p2.slot, e.p2.tmp_ovl);
  }
  RVN_HIP(rvn_stream_sync(s));
  out.n_overlaps = acc_n;
}

// raven::FindOverlapsAndRepetetiveRegions (construct.cc:316-491); R = all reads with ids[i] == i
void second_pass(Engine& e, const ReadsDev& R, const u32* h_begin, const u32* h_end, const u8* h_invalid, double freq,
                 u32 kmer_len, double identity, u64 batch_bases, Pass2State& out) {
  Pass2Prep P;
  second_pass_prepare(e, R, h_begin, h_end, h_invalid, batch_bases, out, P);
  if (P.sv == 0) return;
  for (const auto& b : P.batches) second_pass_batch(e, P, b.first, b.second, 0, b.second, freq, kmer_len, identity, out);
  second_pass_finish(e, P.d_regions, out);
}

// The identity filter loop of ResolveContainedReads (construct.cc:162-217) on a flat list of O overlaps (host):
// OverlapUpdate + edlib score of the two spans; ok[x] = survives, upd[x] = the overlap with its updated coordinates.
void identity_filter_flags(Engine& e, const ReadsDev& R, const Overlap* h_ovl, u64 O, const u32* h_begin, const u32* h_end,
                           const u8* h_invalid, double identity, u8* h_ok, Overlap* h_upd) {
  hipStream_t s = e.stream;
  if (O == 0) return;
  PileRegion* d_regions = upload_pile_regions(e, e.p2.regions, h_begin, h_end, h_invalid, R.n);
  Overlap* d_ovl = upload(e.p2.tmp_ovl, h_ovl, O, s);
  u8* d_ok = e.p2.ok.get<u8>(O + 16);
  update_and_identity(e, R, d_ovl, O, d_regions, nullptr, identity, d_ok);  // ids are indices
  RVN_HIP(hipMemcpyAsync(h_ok, d_ok, O, hipMemcpyDeviceToHost, s));
  RVN_HIP(hipMemcpyAsync(h_upd, d_ovl, O * sizeof(Overlap), hipMemcpyDeviceToHost, s));
  RVN_HIP(rvn_stream_sync(s));
}

// per-pile compaction of the survivors (construct.cc:208-210): lists h_off[n + 1] of h_ovl, in place
void identity_filter_compact(Overlap* h_ovl, u32* h_off, u32 n, const u8* ok, const Overlap* upd) {
  u64 k = 0;
  u32 prev_end = h_off[0];
  for (u32 i = 0; i < n; ++i) {
    const u32 b = prev_end, en = h_off[i + 1];
    prev_end = en;
    h_off[i] = static_cast<u32>(k);
    for (u32 x = b; x < en; ++x)
      if (ok[x]) h_ovl[k++] = upd[x];
  }
  h_off[n] = static_cast<u32>(k);
}

// The identity filter loop of ResolveContainedReads (construct.cc:162-217) on per-pile overlap lists (CSR, host, in
// place): OverlapUpdate, edlib score of the two spans, survivors keep their updated coordinates and their order.
void identity_filter_lists(Engine& e, const ReadsDev& R, Overlap* h_ovl, u32* h_off, const u32* h_begin, const u32* h_end,
                           const u8* h_invalid, double identity) {
  const u32 n = R.n;
  const u64 O = h_off[n];
  if (O == 0) return;
  std::vector<u8> ok(O);
  std::vector<Overlap> upd(O);
  identity_filter_flags(e, R, h_ovl, O, h_begin, h_end, h_invalid, identity, ok.data(), upd.data());
  identity_filter_compact(h_ovl, h_off, n, ok.data(), upd.data());
}

#ifdef RVN_TEST_HOOKS
// rvn_test_second_pass (include/raven_hip_test.h): second_pass with the Map output of every batch taken from the host.
// Every argument that a kernel would index with is checked here, for all batches, before the first launch; no kernel is
// launched from here.  It leaves e.sketch.query_sketch and e.map.out fabricated (counts and offsets of the last batch, no
// minimizer values, no matches): the engine must not Map afterwards without a fresh engine_minimize / map_batch.
static void test_second_pass(Engine& e, const ReadsDev& R, const u32* h_begin, const u32* h_end, const u8* h_invalid,
                             double identity, u32 kmer_len, const rvn_test_pass2_batch* batches, u32 n_batches,
                             Pass2State& out) {
  auto bad = [](const char* what) { throw std::invalid_argument(std::string("[raven_hip] rvn_test_second_pass: ") + what); };
  if (kmer_len == 0 || kmer_len > 32) bad("kmer_len must be in [1, 32]");
  if (!(0 <= identity && identity <= 1)) bad("identity must be in [0, 1]");
  std::vector<u32> valid;  // as second_pass_prepare orders them: the valid reads by id
  for (u32 i = 0; i < R.n; ++i) {
    if (R.h_id[i] != i) bad("requires ids[i] == i");
    if (h_begin[i] > h_end[i] || h_end[i] > R.h_len[i]) bad("a valid region outside its read");
    if (!h_invalid[i]) valid.push_back(i);
  }
  // (as second_pass: with every pile valid or every pile invalid nothing is mapped and no batch is looked at)
  const u32 sv = valid.size() == R.n ? 0u : static_cast<u32>(valid.size());
  for (u32 b = 0; sv && b < n_batches; ++b) {
    const rvn_test_pass2_batch& B = batches[b];
    if (B.q_first > B.q_last || B.q_last > sv) bad("query reads outside the valid reads");
    const u32 nr = B.q_last - B.q_first;
    const u64 nq = B.n_query, O = B.n_overlaps;
    if (nq >= (1ULL << 32) || O >= (1ULL << 32)) bad(">= 2^32 entries in a batch");
    if (!B.q_read_off || (nq && (!B.q_origins || !B.filtered)) || (O && !B.overlaps)) bad("NULL array in a batch");
    if (B.q_read_off[0] != 0 || B.q_read_off[nr] != nq) bad("offsets must run from 0 to n_query");
    if (nr == 0 && O) bad("overlaps in a batch without query reads");
    for (u32 r = 0; r < nr; ++r) {
      if (B.q_read_off[r + 1] < B.q_read_off[r] || B.q_read_off[r + 1] > nq) bad("offsets must ascend to n_query");
      const u32 len = R.h_len[valid[B.q_first + r]];
      for (u64 q = B.q_read_off[r]; q < B.q_read_off[r + 1]; ++q) {
        if (B.filtered[q] > 1) bad("filtered flags are 0 or 1");
        if (len < kmer_len || (static_cast<u32>(B.q_origins[q]) >> 1) > len - kmer_len) bad("a k-mer beyond its read");
      }
    }
    for (u64 x = 0; x < O; ++x)
      if (B.overlaps[x].lhs_id >= R.n || B.overlaps[x].rhs_id >= R.n) bad("overlap id out of range");
  }
  Pass2Prep P;
  second_pass_prepare(e, R, h_begin, h_end, h_invalid, 1ULL << 30, out, P);
  if (P.sv == 0) return;
  hipStream_t s = e.stream;
  for (u32 b = 0; b < n_batches; ++b) {
    const rvn_test_pass2_batch& B = batches[b];
    const u32 nr = B.q_last - B.q_first;
    const u64 nq = B.n_query, O = B.n_overlaps;
    if (nr == 0) continue;  // (no query reads, hence no overlaps: checked above)
    Sketch& qs = e.sketch.query_sketch;
    e.sketch.query_ready = {};
    qs.first = B.q_first;
    qs.last = B.q_last;
    qs.count = nq;
    MapOut& mo = e.map.out;
    mo.first = B.q_first;
    mo.last = B.q_last;
    mo.n_query = nq;
    mo.n_matches = mo.n_intervals = 0;
    mo.n_overlaps = O;
    mo.has_anchors = false;
    upload(qs.org, B.q_origins, nq, s);
    upload(qs.read_off, B.q_read_off, static_cast<size_t>(nr) + 1, s);
    upload(mo.filtered, B.filtered, nq, s);
    upload(mo.ovl, reinterpret_cast<const Overlap*>(B.overlaps), O, s);
    RVN_HIP(rvn_stream_sync(s));
    second_pass_merge(e, P, B.q_first, B.q_last, mo, kmer_len, identity, out);
  }
  second_pass_finish(e, P.d_regions, out);
}
#endif  // RVN_TEST_HOOKS

}  // namespace rvn

#ifdef RVN_TEST_HOOKS
extern "C" int rvn_test_second_pass(rvn_engine* h, const rvn_reads* rr, const uint32_t* pile_begin, const uint32_t* pile_end,
                                    const uint8_t* pile_invalid, double identity, uint32_t kmer_len,
                                    const rvn_test_pass2_batch* batches, uint32_t n_batches, rvn_pass2** out) {
  using namespace rvn;
  const bool ok = h && rr && out && !(rr->r.n && (!pile_begin || !pile_end || !pile_invalid)) && !(n_batches && !batches);
  return guarded(h, ok, "[raven_hip] rvn_test_second_pass: NULL argument", [&](Engine& e) -> int {
    std::unique_ptr<rvn_pass2> p(new rvn_pass2());
    p->e = &e;
    p->engine_life = e.life;
    test_second_pass(e, rr->r, pile_begin, pile_end, pile_invalid, identity, kmer_len, batches, n_batches, p->st);
    *out = p.release();
    return RVN_OK;
  });
}
#endif  // RVN_TEST_HOOKS
