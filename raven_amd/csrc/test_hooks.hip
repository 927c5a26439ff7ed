// test_hooks.hip — host test hooks of include/raven_hip_test.h that need no file-local code of a stage: compiled only
// into libraven_hip_test.so (TEST INFRASTRUCTURE).
#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/raven_hip_test.h"
#include "abi.h"
#include "freelist.h"
#include "inflate_fast.h"
#include "introsort.h"
#include "io_text.h"
#include "kmer.h"
#include "lowcomplexity.h"
#include "nwpath.h"
#include "slopes.h"

using namespace rvn;

namespace {

// The device-wide primitives (radix_sort.hip, scan.hip) on host arrays, in an engine of its own (device 0) for the stream
// and the scratch; f(Engine&) does the copies and the one call.
template <typename F>
int with_own_engine(F f) {
  rvn_engine* h = nullptr;
  int r = rvn_engine_create(&h, 15, 5, 500, 4, 100, 10000, 0);
  if (r != RVN_OK) return r;
  r = guarded(&h->e, [&]() -> int { return f(h->e); });
  rvn_engine_destroy(h);
  return r;
}

template <typename K, typename V, typename Sort>
int radix_sort_pairs_host(Engine& e, uint64_t* keys, uint64_t* values, u64 n, int key_bits, bool skip, Sort sort) {
  std::vector<K> hk(n);
  std::vector<V> hv(n);
  for (u64 i = 0; i < n; ++i) {
    hk[i] = static_cast<K>(keys[i]);
    hv[i] = static_cast<V>(values[i]);
    if (hk[i] != keys[i] || hv[i] != values[i]) return fail(RVN_EINVAL, "[raven_hip] rvn_test_radix_sort_pairs: value too wide for the variant");
  }
  DevBuf bk[2], bv[2];
  K* k0 = bk[0].get<K>(n + 1);
  K* k1 = bk[1].get<K>(n + 1);
  V* v0 = bv[0].get<V>(n + 1);
  V* v1 = bv[1].get<V>(n + 1);
  if (n) {
    RVN_HIP(hipMemcpy(k0, hk.data(), n * sizeof(K), hipMemcpyHostToDevice));
    RVN_HIP(hipMemcpy(v0, hv.data(), n * sizeof(V), hipMemcpyHostToDevice));
  }
  const int cur = sort(k0, k1, v0, v1, n, key_bits, e.scratch.sort_tmp, e.scratch.scan_tmp, e.stream, kKRsUpsweep, kKRsDownsweep, skip);
  RVN_HIP(rvn_stream_sync(e.stream));
  if (n) {
    RVN_HIP(hipMemcpy(hk.data(), cur ? k1 : k0, n * sizeof(K), hipMemcpyDeviceToHost));
    RVN_HIP(hipMemcpy(hv.data(), cur ? v1 : v0, n * sizeof(V), hipMemcpyDeviceToHost));
  }
  for (u64 i = 0; i < n; ++i) {
    keys[i] = hk[i];
    values[i] = hv[i];
  }
  return RVN_OK;
}

template <typename In, typename Out, typename Scan>
int exclusive_scan_host(Engine& e, const uint64_t* in, uint64_t* out, u64 n, u32 in_off, u32 out_off, Scan scan) {
  std::vector<In> hi(n);
  for (u64 i = 0; i < n; ++i) {
    hi[i] = static_cast<In>(in[i]);
    if (hi[i] != in[i]) return fail(RVN_EINVAL, "[raven_hip] rvn_test_exclusive_scan: value too wide for the variant");
  }
  DevBuf bi, bo;  // (hipMalloc aligns to at least 256 bytes: the element offsets alone decide the 16-byte alignment)
  In* d_in = bi.get<In>(n + in_off + 1) + in_off;
  Out* d_out = bo.get<Out>(n + out_off + 2) + out_off;
  if (n) RVN_HIP(hipMemcpy(d_in, hi.data(), n * sizeof(In), hipMemcpyHostToDevice));
  scan(d_in, d_out, n, e.scratch.scan_tmp, e.stream);
  RVN_HIP(rvn_stream_sync(e.stream));
  std::vector<Out> ho(n + 1);
  RVN_HIP(hipMemcpy(ho.data(), d_out, (n + 1) * sizeof(Out), hipMemcpyDeviceToHost));
  for (u64 i = 0; i <= n; ++i) out[i] = ho[i];
  return RVN_OK;
}

// rvn_test_match_probe (include/raven_hip_test.h): match_probe (map.hip) on a query sketch given by the host.  Every
// argument that a kernel would index with is checked here; no kernel is launched from here.
int test_match_probe(Engine& e, const u64* q_values, const u64* q_origins, u64 nq, const u32* q_read_off, u32 nr,
                     bool avoid_equal, bool avoid_symmetric, u64** grp, u64** pos, u64* seg_off, u8* filtered, u64* n_matches) {
  *grp = *pos = nullptr;
  *n_matches = 0;
  std::memset(seg_off, 0, (static_cast<size_t>(nr) + 1) * 8);
  if (nq) std::memset(filtered, 0, nq);
  if (nq >= (1ULL << 32)) throw std::invalid_argument("[raven_hip] rvn_test_match_probe: >= 2^32 query minimizers");
  if (q_read_off[0] != 0 || q_read_off[nr] != nq) throw std::invalid_argument("[raven_hip] rvn_test_match_probe: offsets must run from 0 to n_query");
  for (u32 i = 0; i < nr; ++i)
    if (q_read_off[i + 1] < q_read_off[i]) throw std::invalid_argument("[raven_hip] rvn_test_match_probe: offsets must ascend");
  const u64 limit = 1ULL << (2 * e.k);  // (k <= 31)
  for (u64 i = 0; i < nq; ++i)
    if (q_values[i] >= limit) throw std::invalid_argument("[raven_hip] rvn_test_match_probe: value of more than 2k bits");
  auto empty = [](u64** p) {
    *p = static_cast<u64*>(std::malloc(8));
    if (!*p) throw std::bad_alloc();
  };
  if (nq == 0 || e.sketch.index.m == 0) {  // (map_batch returns before the match stage)
    empty(grp);
    empty(pos);
    return RVN_OK;
  }
  Sketch& qs = e.sketch.query_sketch;
  e.sketch.query_ready = {};
  qs.first = 0;
  qs.last = nr;
  qs.count = nq;
  if (e.val64) {
    RVN_HIP(hipMemcpy(qs.val.get<u64>(nq + 1), q_values, nq * 8, hipMemcpyHostToDevice));
  } else {
    std::vector<u32> v32(nq);
    for (u64 i = 0; i < nq; ++i) v32[i] = static_cast<u32>(q_values[i]);
    RVN_HIP(hipMemcpy(qs.val.get<u32>(nq + 1), v32.data(), nq * 4, hipMemcpyHostToDevice));
  }
  RVN_HIP(hipMemcpy(qs.org.get<u64>(nq + 1), q_origins, nq * 8, hipMemcpyHostToDevice));
  RVN_HIP(hipMemcpy(qs.read_off.get<u32>(static_cast<size_t>(nr) + 1), q_read_off, (static_cast<size_t>(nr) + 1) * 4, hipMemcpyHostToDevice));
  u8* d_filt = e.map.out.filtered.get<u8>(nq + 1);
  u64* d_seg = e.map.seg_off.get<u64>(static_cast<size_t>(nr) + 2);
  const u64 H = match_probe(e, qs, nr, avoid_equal, avoid_symmetric, d_filt, d_seg);
  RVN_HIP(hipMemcpy(filtered, d_filt, nq, hipMemcpyDeviceToHost));
  *grp = static_cast<u64*>(std::malloc((H + 1) * 8));
  *pos = static_cast<u64*>(std::malloc((H + 1) * 8));
  if (!*grp || !*pos) throw std::bad_alloc();
  if (H) {
    RVN_HIP(hipMemcpy(*grp, e.map.m_grp[0].ptr, H * 8, hipMemcpyDeviceToHost));
    RVN_HIP(hipMemcpy(*pos, e.map.m_pos[0].ptr, H * 8, hipMemcpyDeviceToHost));
    RVN_HIP(hipMemcpy(seg_off, d_seg, (static_cast<size_t>(nr) + 1) * 8, hipMemcpyDeviceToHost));
  }
  *n_matches = H;
  return RVN_OK;
}

}  // namespace

extern "C" {

int rvn_test_match_probe(rvn_engine* h, const uint64_t* q_values, const uint64_t* q_origins, uint64_t n_query,
                         const uint32_t* q_read_off, uint32_t n_reads, int avoid_equal, int avoid_symmetric,
                         uint64_t** group, uint64_t** positions, uint64_t* seg_off, uint8_t* filtered, uint64_t* n_matches) {
  const bool ok = h && q_read_off && group && positions && seg_off && n_matches && !(n_query && (!q_values || !q_origins || !filtered));
  return guarded(h, ok, "[raven_hip] rvn_test_match_probe: NULL argument", [&](Engine& e) -> int {
    try {
      return test_match_probe(e, q_values, q_origins, n_query, q_read_off, n_reads, avoid_equal != 0, avoid_symmetric != 0, group,
                              positions, seg_off, filtered, n_matches);
    } catch (...) {
      std::free(*group);
      std::free(*positions);
      *group = *positions = nullptr;
      throw;
    }
  });
}

int64_t rvn_test_find_chimeric_regions(const uint16_t* data, uint32_t size, uint32_t* out, uint64_t cap_pairs) {
  if (!data || !out || size == 0) return RVN_EINVAL;
  std::vector<SlopeRegion> slopes(2 * static_cast<size_t>(size) + 2);  // same bounds as the device path (pile.hip)
  std::vector<u16> tmp(size + 1);
  bool overflow = false;
  const u32 n = find_chimeric_regions(data, static_cast<int>(size), slopes.data(), 2 * size, tmp.data(), out,
                                      static_cast<u32>(std::min<uint64_t>(cap_pairs, size)), &overflow);
  return overflow ? -5 : static_cast<int64_t>(n);
}

int rvn_test_overlap_update_and_type(rvn_overlap* overlaps, uint64_t n, const uint32_t* pile_begin, const uint32_t* pile_end,
                                     const uint8_t* pile_invalid, uint32_t n_piles, uint8_t* ok, uint32_t* type) {
  return rvn_overlap_update_and_type(overlaps, n, pile_begin, pile_end, pile_invalid, n_piles, ok, type);
}

int rvn_poa_banded_emulate(const uint8_t* codes, const uint8_t* quals, const uint64_t* layer_offsets, const uint32_t* begins,
                           const uint32_t* ends, const uint32_t* has_qual, const uint32_t* window_offsets,
                           uint32_t n_windows, int match, int mismatch, int gap, int trim, uint8_t* consensus,
                           const uint64_t* consensus_offsets, uint32_t* consensus_len, uint32_t* status, int variant) {
  return guarded([&]() -> int {
    if (n_windows && (!codes || !layer_offsets || !begins || !ends || !window_offsets || !consensus || !consensus_offsets ||
                      !consensus_len || !status))
      return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    for (uint32_t w = 0; w < n_windows; ++w)
      if (window_offsets[w + 1] <= window_offsets[w])
        return fail(RVN_EINVAL, "[raven_hip] rvn_poa_banded_emulate: window without a backbone");
    poa_banded_emulate(codes, quals, layer_offsets, begins, ends, has_qual, window_offsets, n_windows, match, mismatch, gap,
                       trim, consensus, consensus_offsets, consensus_len, status, variant);
    return RVN_OK;
  });
}

uint64_t rvn_test_hash(uint64_t key, uint32_t k, int use32) {
  const u64 mask = (1ULL << (2 * k)) - 1;
  if (use32) return hash32(static_cast<u32>(key), static_cast<u32>(mask));
  return hash64(key, mask);
}

int rvn_test_canonical(const uint64_t* words, uint32_t pos, uint32_t k, int use32, uint64_t* value,
                       uint32_t* strand) {
  const u64 mask = (1ULL << (2 * k)) - 1;
  const u32 bit = 2 * pos;
  const u64 x = extract_bits(words[bit >> 6], words[(bit >> 6) + 1], bit & 63, mask);
  unsigned st = 0;
  bool ok;
  if (use32) {
    u32 v = 0;
    ok = canonical_hash<u32>(x, k, mask, &v, &st);
    *value = v;
  } else {
    u64 v = 0;
    ok = canonical_hash<u64>(x, k, mask, &v, &st);
    *value = v;
  }
  *strand = st;
  return ok ? 1 : 0;
}

// The host half of rvn_reads_load (io_text.h: member cut + inflate pool + record scanner) without a device: the kept
// text is assembled in host memory exactly as the H2D copies would lay it out in HBM, then cut into the records' fields.
// Outputs are malloc'ed (rvn_free): bases and qualities back to back, lengths, names separated by '\n';
// info[8] = {gzip, streaming, members, threads, restarted, loop microseconds, scan microseconds, fast single-stream decoder}.
int rvn_test_parse_file(const char* path, int fastq, uint32_t threads, int force_streaming, uint64_t slab_bytes,
                        uint8_t** bases, uint8_t** quals, uint32_t** lengths, uint32_t* n_records, char** names,
                        uint32_t* info) {
  return guarded([&]() -> int {
    if (!path || !bases || !quals || !lengths || !n_records || !names) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    for (int attempt = 0; attempt < 2; ++attempt) {
      try {
        io::SourceOptions opt;
        opt.threads = threads;
        opt.force_streaming = force_streaming != 0 || attempt == 1;
        if (slab_bytes) opt.slab_bytes = slab_bytes;
        io::TextSource src(path, opt);
        io::RecordScanner sc(fastq != 0);
        std::vector<u8> text;
        std::vector<io::TextRecord> recs;
        std::vector<std::string> nm;
        u8* slab = nullptr;
        u64 n = 0;
        bool first = true;
        const bool timing_only = knob("RVN_TEST_IO_TIMING_ONLY") != nullptr;  // records then come back empty
        const auto t_loop = std::chrono::steady_clock::now();
        double scan_s = 0;
        while (src.next(&slab, &n)) {
          const u8* run = nullptr;
          u64 run_len = 0, run_base = 0;
          const auto t_scan = std::chrono::steady_clock::now();
          sc.scan(slab, n, &run, &run_len, &run_base, recs, nm);
          scan_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_scan).count();
          if (!timing_only) {
            if (text.size() < run_base + run_len) text.resize(run_base + run_len);
            if (run_len) std::memcpy(text.data() + run_base, run, run_len);
          }
          if (!first) src.release();
          first = false;
        }
        const double loop_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop).count();
        u8 extra = 0;
        const u64 at = sc.text_end();
        if (sc.finish(recs, nm, &extra)) {
          text.resize(std::max<u64>(text.size(), at + 1));
          text[at] = extra;
        }
        u64 total = 0, nb = 0;
        for (const io::TextRecord& r : recs) total += r.len;
        for (const std::string& x : nm) nb += x.size() + 1;
        u8* b = static_cast<u8*>(std::malloc(total + 1));
        u8* q = static_cast<u8*>(std::malloc(total + 1));
        uint32_t* l = static_cast<uint32_t*>(std::malloc((recs.size() + 1) * 4));
        char* names_out = static_cast<char*>(std::malloc(nb + 1));
        if (!b || !q || !l || !names_out) return fail(RVN_ENOMEM, "[raven_hip] out of memory");
        u64 o = 0, no = 0;
        if (timing_only) recs.clear();
        for (size_t i = 0; i < recs.size(); ++i) {
          std::memcpy(b + o, text.data() + recs[i].seq_off, recs[i].len);
          if (fastq) std::memcpy(q + o, text.data() + recs[i].qual_off, recs[i].len);
          l[i] = static_cast<uint32_t>(recs[i].len);
          o += recs[i].len;
          std::memcpy(names_out + no, nm[i].data(), nm[i].size());
          no += nm[i].size();
          names_out[no++] = '\n';
        }
        names_out[no] = 0;
        *bases = b;
        *quals = q;
        *lengths = l;
        *n_records = static_cast<uint32_t>(recs.size());
        *names = names_out;
        if (info) {
          info[0] = src.gzip();
          info[1] = src.streaming();
          info[2] = src.members();
          info[3] = src.threads();
          info[4] = static_cast<uint32_t>(attempt);
          info[5] = static_cast<uint32_t>(loop_s * 1e6);  // inflate + scan + assembling the kept text, microseconds
          info[6] = static_cast<uint32_t>(scan_s * 1e6);  // of which inside RecordScanner::scan
          info[7] = src.fast_stream() ? 1 : 0;            // the single stream went through inflate_fast.h
        }
        return RVN_OK;
      } catch (const io::SpeculationFailed&) {
        if (attempt == 1) return fail(RVN_EINVAL, "[bioparser] error: corrupt or truncated file");
      } catch (const std::invalid_argument&) {  // (as reads_load: only the zlib attempt reports an error)
        if (attempt == 1) throw;
      }
    }
    return RVN_OK;
  });
}

// inflate_fast.h on ONE gzip member (header and trailer handled here): dst gets the text, out[4] = {bytes produced, bytes
// of the member consumed incl. the trailer, CRC-32 found in the trailer, ISIZE found}; chunk > 0: the output is produced
// through a buffer of that many bytes that is drained whenever it fills (the way the input path uses the decoder).
// Returns 0, RVN_EINVAL with the decoder's message for an invalid stream.
int rvn_test_inflate_fast(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap, uint64_t chunk, uint64_t* out) {
  return guarded([&]() -> int {
    if (!src || !dst || !out) return fail(RVN_EINVAL, "[raven_hip] NULL argument");
    const u64 hdr = io::gz_header_len(src, n, nullptr);
    if (!hdr) return fail(RVN_EINVAL, "not a gzip member");
    io::FastInflate dec;
    dec.reset(src + hdr, src + n);
    u64 produced = 0;
    if (chunk == 0) {
      u8* o = dst;
      const io::FastInflate::Status st = dec.run(dst, &o, dst + cap);
      produced = static_cast<u64>(o - dst);
      if (st == io::FastInflate::kOutputFull) return fail(RVN_EINVAL, "output buffer too small");
      if (st == io::FastInflate::kError) return fail(RVN_EINVAL, dec.error());
    } else {
      const u64 hist = 32768;
      std::vector<u8> buf(hist + chunk + io::FastInflate::kOutMargin);
      u8* base = buf.data();
      u8* o = base;  // (no history yet)
      const u8* valid_from = base;
      for (;;) {
        const io::FastInflate::Status st = dec.run(valid_from, &o, base + buf.size());
        const u8* from = valid_from == base && produced == 0 ? base : base + hist;
        // drain what is new: everything behind the history area (or the whole buffer the first time round)
        const u64 fresh = static_cast<u64>(o - from);
        if (produced + fresh > cap) return fail(RVN_EINVAL, "output buffer too small");
        std::memcpy(dst + produced, from, fresh);
        produced += fresh;
        if (st == io::FastInflate::kError) return fail(RVN_EINVAL, dec.error());
        if (st == io::FastInflate::kStreamEnd) break;
        // keep the last 32 KB in front
        const u64 have = static_cast<u64>(o - base);
        const u64 keep = std::min<u64>(hist, have);
        std::memmove(base + hist - keep, o - keep, keep);
        valid_from = base + hist - keep;
        o = base + hist;
      }
    }
    const u8* p = dec.input_position();
    if (p + 8 > src + n) return fail(RVN_EINVAL, "unexpected end of file");
    out[0] = produced;
    out[1] = static_cast<u64>(p + 8 - src);
    out[2] = p[0] | (static_cast<u64>(p[1]) << 8) | (static_cast<u64>(p[2]) << 16) | (static_cast<u64>(p[3]) << 24);
    out[3] = p[4] | (static_cast<u64>(p[5]) << 8) | (static_cast<u64>(p[6]) << 16) | (static_cast<u64>(p[7]) << 24);
    return RVN_OK;
  });
}

// freelist.h (the bookkeeping of the device arena) driven by a list of operations: ops[i] > 0 = allocate that many bytes
// (out[i] = offset, or -1 if no hole holds it), ops[i] <= 0 = give back the block allocated by operation -ops[i] (out[i] = 1,
// 0 if that was no block in use).  state[3] = {bytes free, largest hole, blocks in use} at the end.
int rvn_test_freelist(uint64_t size, uint64_t grain, const int64_t* ops, uint32_t n_ops, int64_t* out, uint64_t* state) {
  if (!ops || !out || !state) return RVN_EINVAL;
  rvn::FreeList fl;
  fl.reset(size, grain);
  std::vector<char> given_back(n_ops, 0);  // (a block is named by the operation that made it: its offset may have a new owner)
  for (uint32_t i = 0; i < n_ops; ++i) {
    if (ops[i] > 0) {
      size_t off = 0;
      out[i] = fl.alloc(static_cast<size_t>(ops[i]), &off) ? static_cast<int64_t>(off) : -1;
    } else {
      const uint64_t j = static_cast<uint64_t>(-ops[i]);
      const bool ok = j < i && ops[j] > 0 && out[j] >= 0 && !given_back[j] && fl.release(static_cast<size_t>(out[j]));
      if (ok) given_back[j] = 1;
      out[i] = ok ? 1 : 0;
    }
  }
  state[0] = fl.free_total();
  state[1] = fl.free_largest();
  state[2] = fl.in_use.size();
  return RVN_OK;
}

// Bit 24 of rc: the PRODUCTION stage on the device (nw_breakpoints, as a polishing round runs it: planning, variants,
// stripes, retries, walks) on this one job, in an engine of its own (device 0); bits 16-23 = nw_stripe_lanes (0: default),
// k and force_r unused.  band[5] = {k, stripe lanes (0: one ring), R, stripes, microseconds of the stage}; -3: not aligned.
static int nw_breakpoints_device(const uint64_t* t_words, uint32_t t_len, const uint64_t* r_words, uint32_t r_len,
                                 uint32_t t_begin, uint32_t n, uint32_t q_begin, uint32_t m, int rc, uint32_t w, uint32_t,
                                 int, uint32_t* recs, uint32_t* distance, uint32_t* band) {
  rvn_engine* h = nullptr;
  int r = rvn_engine_create(&h, 15, 5, 500, 4, 100, 10000, 0);
  if (r != RVN_OK) return r;
  rvn_reads *T = nullptr, *Rd = nullptr;
  const u64 tw = (static_cast<u64>(t_len) + 31) / 32, rw = (static_cast<u64>(r_len) + 31) / 32;
  const u64 toff[2] = {0, tw}, roff[2] = {0, rw};
  const u32 tid = 0;
  r = rvn_reads_upload(h, t_words, tw, toff, &t_len, &tid, 1, &T);
  if (r == RVN_OK) r = rvn_reads_upload(h, r_words, rw, roff, &r_len, &tid, 1, &Rd);
  if (r == RVN_OK) {
    const u32 lanes = static_cast<u32>(rc >> 16) & 0xFFu;
    if (lanes) h->e.opt.nw_stripe_lanes = lanes;
    r = guarded(&h->e, [&]() -> int {
      std::vector<NwJob> jobs(1);
      NwJob& J = jobs[0];
      J = NwJob{};
      J.t_word = 0;
      J.r_word = 0;
      J.t_begin = t_begin;
      J.n = n;
      J.q_begin = q_begin;
      J.m = m;
      J.r_len = r_len;
      J.rc = rc & 1;
      J.n_windows = (t_begin + n - 1) / w - t_begin / w + 1;
      J.bp_off = 0;
      DevBuf d_recs;
      NwWindowRec* dr = d_recs.get<NwWindowRec>(J.n_windows + 1);
      NwStats st;
      std::vector<u32> dist;
      nw_breakpoints(h->e, T->r, Rd->r, jobs, w, dr, J.n_windows, st, &dist);
      RVN_HIP(hipMemcpy(recs, dr, static_cast<size_t>(J.n_windows) * sizeof(NwWindowRec), hipMemcpyDeviceToHost));
      *distance = dist[0];
      if (band) {
        band[0] = jobs[0].k;
        band[1] = jobs[0].S;
        band[2] = jobs[0].R;
        band[3] = static_cast<u32>(nw_geo_job(jobs[0]).n_stripes);
        band[4] = static_cast<u32>(st.ms * 1000.0);
      }
      return dist[0] == ~0u ? -3 : RVN_OK;
    });
  }
  if (Rd) rvn_reads_destroy(Rd);
  if (T) rvn_reads_destroy(T);
  rvn_engine_destroy(h);
  return r;
}

// TrimAndAnnotatePiles on a crafted coverage CSR, on the device, through the functions the C ABI calls (pile.hip:
// piles_init, piles_trim_and_median, piles_find_chimeric_regions) in an engine of its own (device 0).  No kernel is
// launched from here.
int rvn_test_piles_annotate(const uint16_t* data, const uint64_t* offsets, uint32_t n, uint32_t coverage, int chimeric_mode,
                            const uint8_t* invalid_in, int skip_trim, uint16_t* data_after, uint32_t* begin, uint32_t* end,
                            uint16_t* median, uint8_t* invalid, uint32_t* region_offsets, uint32_t** regions) {
  if (!offsets || !region_offsets || !regions || (chimeric_mode != 0 && chimeric_mode != 1) || coverage > 65535)
    return fail(RVN_EINVAL, "[raven_hip] rvn_test_piles_annotate: bad argument");
  *regions = nullptr;
  const u64 total = offsets[n] - offsets[0];
  if ((total && !data) || (!skip_trim && n && (!begin || !end || !median || !invalid)))
    return fail(RVN_EINVAL, "[raven_hip] rvn_test_piles_annotate: NULL argument");
  for (u32 i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] >= (1u << 28))
      return fail(RVN_EINVAL, "[raven_hip] rvn_test_piles_annotate: offsets must ascend, piles below 2^28 cells");
  std::memset(region_offsets, 0, (static_cast<size_t>(n) + 1) * 4);
  auto empty = [&]() -> int {
    *regions = static_cast<uint32_t*>(std::malloc(4));
    return *regions ? RVN_OK : fail(RVN_ENOMEM, "[raven_hip] out of host memory");
  };
  if (n == 0) return empty();
  rvn_engine* h = nullptr;
  int r = rvn_engine_create(&h, 15, 5, 500, 4, 100, 10000, 0);
  if (r != RVN_OK) return r;
  r = guarded(&h->e, [&]() -> int {
    Engine& e = h->e;
    ReadsDev rd;  // lengths only: a pile is (length >> 4) cells (as rvn_pile_add_layers lays out its one pile)
    rd.n = n;
    rd.h_len.resize(n);
    for (u32 i = 0; i < n; ++i) rd.h_len[i] = static_cast<u32>(offsets[i + 1] - offsets[i]) << 4;
    PileState ps;
    piles_init(e, rd, ps);
    if (total) RVN_HIP(hipMemcpy(ps.pile_data.ptr, data + offsets[0], total * 2, hipMemcpyHostToDevice));
    std::vector<u8> inv(n, 0);
    if (!skip_trim) {
      piles_trim_and_median(e, ps, coverage, begin, end, median, invalid);
      inv.assign(invalid, invalid + n);
    }
    if (invalid_in) inv.assign(invalid_in, invalid_in + n);
    if (data_after && total) RVN_HIP(hipMemcpy(data_after, ps.pile_data.ptr, total * 2, hipMemcpyDeviceToHost));
    std::vector<u32> off, reg;
    piles_find_chimeric_regions(e, ps, inv.data(), off, reg, chimeric_mode ? kChimericPerThread : kChimericWave);
    std::memcpy(region_offsets, off.data(), off.size() * 4);
    auto* out = static_cast<uint32_t*>(std::malloc((reg.size() + 1) * 4));
    if (!out) return fail(RVN_ENOMEM, "[raven_hip] out of host memory");
    if (!reg.empty()) std::memcpy(out, reg.data(), reg.size() * 4);
    *regions = out;
    return RVN_OK;
  });
  rvn_engine_destroy(h);
  return r;
}

int rvn_test_nw_breakpoints(const uint64_t* t_words, uint32_t t_len, const uint64_t* r_words, uint32_t r_len,
                            uint32_t t_begin, uint32_t n, uint32_t q_begin, uint32_t m, int rc, uint32_t w, uint32_t k,
                            int force_r, uint32_t* recs, uint32_t* distance, uint32_t* band) {
  if (!t_words || !r_words || !recs || !distance || w == 0) return RVN_EINVAL;
  if (static_cast<u64>(t_begin) + n > t_len || static_cast<u64>(q_begin) + m > r_len) return RVN_EINVAL;
  static_assert(sizeof(NwWindowRec) == 32, "record layout");
  if ((rc >> 24) & 1) return nw_breakpoints_device(t_words, t_len, r_words, r_len, t_begin, n, q_begin, m, rc, w, k, force_r,
                                                   recs, distance, band);
  return nw_breakpoints_host(t_words, t_len, r_words, r_len, t_begin, n, q_begin, m, rc, w, k, force_r,
                             reinterpret_cast<NwWindowRec*>(recs), distance, band);
}

int rvn_test_radix_sort_pairs(int variant, uint64_t* keys, uint64_t* values, uint64_t n, int key_bits, int skip_constant_digits) {
  const int width = variant == 1 ? 64 : 32;
  if (variant < 0 || variant > 2 || (n && (!keys || !values)) || key_bits < 0 || key_bits > width || n >= (1ULL << 32))
    return fail(RVN_EINVAL, "[raven_hip] rvn_test_radix_sort_pairs: bad argument");
  return with_own_engine([&](Engine& e) -> int {
    const bool skip = skip_constant_digits != 0;
    if (variant == 0) return radix_sort_pairs_host<u32, u64>(e, keys, values, n, key_bits, skip, radix_sort_pairs_u32_u64);
    if (variant == 1) return radix_sort_pairs_host<u64, u64>(e, keys, values, n, key_bits, skip, radix_sort_pairs_u64_u64);
    return radix_sort_pairs_host<u32, u32>(e, keys, values, n, key_bits, skip, radix_sort_pairs_u32_u32);
  });
}

int rvn_test_compact_overlap_list(const rvn_overlap* in, uint64_t n, const uint8_t* keep1, const uint8_t* keep2,
                                  rvn_overlap* out, uint64_t* n_out, uint32_t* slot) {
  if ((n && (!in || !keep1 || !out)) || !n_out || !slot || n >= (1ULL << 32))
    return fail(RVN_EINVAL, "[raven_hip] rvn_test_compact_overlap_list: bad argument");
  return with_own_engine([&](Engine& e) -> int {
    DevBuf list, spare, slots, keep;
    upload(list, reinterpret_cast<const Overlap*>(in), n, e.stream);
    u64 m = n, kept = compact_overlap_list(e, list, m, upload(keep, keep1, m, e.stream), slots, spare);
    if (keep2) {
      m = kept;
      kept = compact_overlap_list(e, list, m, upload(keep, keep2, m, e.stream), slots, spare);
    }
    RVN_HIP(rvn_stream_sync(e.stream));
    slot[0] = 0;
    if (m) RVN_HIP(hipMemcpy(slot, slots.ptr, (m + 1) * 4, hipMemcpyDeviceToHost));
    if (kept) RVN_HIP(hipMemcpy(out, list.ptr, kept * sizeof(Overlap), hipMemcpyDeviceToHost));
    *n_out = kept;
    return RVN_OK;
  });
}

int rvn_test_exclusive_scan(int variant, const uint64_t* in, uint64_t n, uint32_t in_offset_items, uint32_t out_offset_items,
                            uint64_t* out) {
  if (variant < 0 || variant > 2 || (n && !in) || !out || n >= (1ULL << 32) || in_offset_items > 64 || out_offset_items > 64)
    return fail(RVN_EINVAL, "[raven_hip] rvn_test_exclusive_scan: bad argument");
  return with_own_engine([&](Engine& e) -> int {
    if (variant == 0) return exclusive_scan_host<u32, u64>(e, in, out, n, in_offset_items, out_offset_items, exclusive_scan_u32_u64);
    if (variant == 1) return exclusive_scan_host<u32, u32>(e, in, out, n, in_offset_items, out_offset_items, exclusive_scan_u32_u32);
    return exclusive_scan_host<u8, u32>(e, in, out, n, in_offset_items, out_offset_items, exclusive_scan_u8_u32);
  });
}

int rvn_test_engine_scratch_bytes(rvn_engine* h, uint64_t* bytes) {
  if (!h || !bytes) return fail(RVN_EINVAL, "[raven_hip] rvn_test_engine_scratch_bytes: NULL argument");
  std::lock_guard<std::recursive_mutex> lk(h->e.mu);
  *bytes = 0;
  h->e.for_each_group([&](auto& group) { group.for_each_buf([&](DevBuf& b) { *bytes += b.cap; }); });
  return RVN_OK;
}

// rvn_test_edit_distance_dev (include/raven_hip_test.h): the records and thresholds go up, ONE call of edit_distance_dev, the
// stored values come back.  The buffers are the ones path_similarity_batch hands to the same function.  No kernel is
// launched from here; every record is checked (abi.h: ed_pairs_error, as rvn_edit_distance_batch) before anything runs.
int rvn_test_edit_distance_dev(rvn_engine* h, const rvn_reads* reads, const uint32_t* pairs, uint32_t n_pairs, const uint32_t* kmax,
                               int wide_sweep, uint32_t* out) {
  return guarded(h, h && reads && pairs && out, "[raven_hip] rvn_test_edit_distance_dev: NULL argument", [&](Engine& e) -> int {
    static_assert(sizeof(rvn_ed_pair) == 32, "pair layout");
    if (wide_sweep != 0 && wide_sweep != 1) return fail(RVN_EINVAL, "[raven_hip] rvn_test_edit_distance_dev: wide_sweep is 0 or 1");
    if (const char* what = ed_pairs_error(reads->r, reinterpret_cast<const rvn_ed_pair*>(pairs), n_pairs))
      return fail(RVN_EINVAL, std::string("[raven_hip] rvn_test_edit_distance_dev: ") + what);
    if (n_pairs == 0) return RVN_OK;
    hipStream_t s = e.stream;
    const u32* d_pairs = upload(e.scratch.tmp_a, pairs, 8 * static_cast<size_t>(n_pairs), s);
    const u32* d_kmax = kmax ? upload(e.scratch.tmp_c, kmax, n_pairs, s) : nullptr;
    u32* d_out = e.scratch.tmp_b.get<u32>(static_cast<size_t>(n_pairs) + 1);
    edit_distance_dev(e, reads->r, d_pairs, n_pairs, d_out, d_kmax, wide_sweep == 1);
    RVN_HIP(hipMemcpyAsync(out, d_out, static_cast<size_t>(n_pairs) * 4, hipMemcpyDeviceToHost, s));
    RVN_HIP(rvn_stream_sync(s));
    return RVN_OK;
  });
}

int rvn_test_low_complexity(const uint8_t* codes, uint32_t k) { return lc_kmer_passes(codes, k) ? 1 : 0; }

void rvn_test_std_sort_lendesc(uint64_t* data, uint64_t n) { std_sort(data, data + n, LenDesc()); }
void rvn_test_heap_sort_lendesc(uint64_t* data, uint64_t n) { intro::heap_sort(data, data + n, LenDesc()); }

}  // extern "C"
