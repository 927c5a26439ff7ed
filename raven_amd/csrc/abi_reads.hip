// abi_reads.hip — C ABI (include/raven_hip.h): read sets (rvn_reads_*).
#include <cstring>
#include <memory>

#include "abi.h"

using namespace rvn;

// the tables of a read set whose packed words the device made (r.packed holds them, pad words included)
void rvn::reads_finish_device_set(Engine& e, ReadsDev& r, const std::vector<u64>& woff, const std::vector<u32>& lens, const uint32_t* ids,
                                  u64 total_bases) {
  const u32 n = static_cast<u32>(lens.size());
  r.n = n;
  r.h_word_off = woff;
  r.h_len = lens;
  r.h_id.resize(n);
  r.ids_are_indices = true;
  r.total_bases = total_bases;
  for (u32 i = 0; i < n; ++i) {
    r.h_id[i] = ids ? ids[i] : i;
    if (r.h_id[i] != i || i >= kMaxReadId) r.ids_are_indices = false;
    if (r.h_id[i] >= kMaxReadId) throw std::invalid_argument("[raven_hip] read ids must be below 2^30");  // (bit 62 of an origin word is kForeignFlag: ADVICE r05)
  }
  r.n_words = woff[n];
  u64* d_wo = r.word_off.get<u64>(static_cast<size_t>(n) + 1);
  RVN_HIP(hipMemcpy(d_wo, r.h_word_off.data(), (static_cast<size_t>(n) + 1) * 8, hipMemcpyHostToDevice));
  u32* d_len = r.len.get<u32>(static_cast<size_t>(n) + 1);
  u32* d_id = r.id.get<u32>(static_cast<size_t>(n) + 1);
  if (n) {
    RVN_HIP(hipMemcpy(d_len, r.h_len.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
    RVN_HIP(hipMemcpy(d_id, r.h_id.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
  }
  reads_build_tiles(e, r);
}

extern "C" {

int rvn_reads_upload(rvn_engine* h, const uint64_t* packed, uint64_t n_words, const uint64_t* word_offsets,
                     const uint32_t* lengths, const uint32_t* ids, uint32_t n, rvn_reads** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !out || (n && (!packed || !word_offsets || !lengths)))
      return fail(RVN_EINVAL, "[raven_hip] rvn_reads_upload: NULL argument");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    std::unique_ptr<rvn_reads> rr(new rvn_reads());
    ReadsDev& r = rr->r;
    r.n = n;
    r.h_word_off.assign(word_offsets, word_offsets + n + 1);
    r.h_len.assign(lengths, lengths + n);
    r.h_id.resize(n);
    r.ids_are_indices = true;
    for (u32 i = 0; i < n; ++i) {
      r.h_id[i] = ids ? ids[i] : i;
      if (r.h_id[i] != i || i >= kMaxReadId) r.ids_are_indices = false;
      // (bits 63 / 62 of a minimizer's origin word are the query / query-only flags: 30 bits of read id are left)
      if (r.h_id[i] >= kMaxReadId) return fail(RVN_EINVAL, "[raven_hip] read ids must be below 2^30");
    }
    r.total_bases = 0;
    for (u32 i = 0; i < n; ++i) {
      r.total_bases += lengths[i];
      const u64 need = (static_cast<u64>(lengths[i]) + 31) / 32;
      if (word_offsets[i + 1] < word_offsets[i] || word_offsets[i + 1] - word_offsets[i] < need ||
          word_offsets[i + 1] > n_words)
        return fail(RVN_EINVAL, "[raven_hip] rvn_reads_upload: word_offsets inconsistent with lengths");
    }
    r.n_words = n_words;
    u64* d_packed = r.packed.get<u64>(n_words + 2);
    if (n_words) RVN_HIP(hipMemcpy(d_packed, packed, n_words * 8, hipMemcpyHostToDevice));
    RVN_HIP(hipMemset(d_packed + n_words, 0, 16));  // pad words: kernels may read one word past a read
    u64* d_wo = r.word_off.get<u64>(static_cast<size_t>(n) + 1);
    RVN_HIP(hipMemcpy(d_wo, r.h_word_off.data(), (static_cast<size_t>(n) + 1) * 8, hipMemcpyHostToDevice));
    u32* d_len = r.len.get<u32>(static_cast<size_t>(n) + 1);
    u32* d_id = r.id.get<u32>(static_cast<size_t>(n) + 1);
    if (n) {
      RVN_HIP(hipMemcpy(d_len, r.h_len.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
      RVN_HIP(hipMemcpy(d_id, r.h_id.data(), static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
    }
    reads_build_tiles(e, r);
    *out = rr.release();
    return RVN_OK;
  });
}

void rvn_reads_destroy(rvn_reads* r) { delete r; }

namespace {
// a read set from one-byte codes that are already in HBM (d_codes + boff[i] .. + boff[i + 1]: read i), packed there
int reads_from_device_codes(Engine& e, const u8* d_codes, const std::vector<u64>& boff, const uint32_t* ids, uint32_t n, rvn_reads** out) {
  std::vector<u64> woff(static_cast<size_t>(n) + 1, 0);
  std::vector<u32> lens(n);
  for (u32 i = 0; i < n; ++i) {
    if (boff[i + 1] < boff[i] || boff[i + 1] - boff[i] > 0xFFFFFFFFULL)
      return fail(RVN_EINVAL, "[raven_hip] rvn_reads_upload_codes: bad offsets");
    lens[i] = static_cast<u32>(boff[i + 1] - boff[i]);
    woff[i + 1] = woff[i] + (static_cast<u64>(lens[i]) + 31) / 32;
  }
  const u64 n_words = woff[n], n_codes = n ? boff[n] - boff[0] : 0;
  u64* d_boff = e.scratch.tmp_b.get<u64>(static_cast<size_t>(n) + 1);
  u64* d_woff = e.scratch.tmp_c.get<u64>(static_cast<size_t>(n) + 1);
  RVN_HIP(hipMemcpy(d_boff, boff.data(), boff.size() * 8, hipMemcpyHostToDevice));
  RVN_HIP(hipMemcpy(d_woff, woff.data(), woff.size() * 8, hipMemcpyHostToDevice));
  std::unique_ptr<rvn_reads> rr(new rvn_reads());
  ReadsDev& r = rr->r;
  u64* d_packed = r.packed.get<u64>(n_words + 2);
  pack_codes_on_device(e, d_codes, d_boff, d_woff, n, n_words, d_packed);
  RVN_HIP(hipMemsetAsync(d_packed + n_words, 0, 16, e.stream));
  RVN_HIP(rvn_stream_sync(e.stream));
  reads_finish_device_set(e, r, woff, lens, ids, n_codes);
  *out = rr.release();
  return RVN_OK;
}
}  // namespace

int rvn_reads_upload_codes(rvn_engine* h, const uint8_t* codes, const uint64_t* offsets, const uint32_t* ids, uint32_t n,
                           rvn_reads** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !out || (n && (!codes || !offsets))) return fail(RVN_EINVAL, "[raven_hip] rvn_reads_upload_codes: NULL argument");
    Engine& e = h->e;
    RVN_HIP(hipSetDevice(e.device));
    for (u32 i = 0; i < n; ++i)
      if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0xFFFFFFFFULL)
        return fail(RVN_EINVAL, "[raven_hip] rvn_reads_upload_codes: bad offsets");
    const u64 n_codes = n ? offsets[n] - offsets[0] : 0;
    // bases to HBM as bytes, packed there (one thread per word)
    u8* d_codes = e.scratch.tmp_a.get<u8>(n_codes + 16);
    if (n_codes) RVN_HIP(hipMemcpy(d_codes, codes + (n ? offsets[0] : 0), n_codes, hipMemcpyHostToDevice));
    std::vector<u64> boff(static_cast<size_t>(n) + 1, 0);
    for (u32 i = 0; i <= n && n; ++i) boff[i] = offsets[i] - offsets[0];
    return reads_from_device_codes(e, d_codes, boff, ids, n, out);
  });
}

// The consensus of the engine's last COMPLETE polishing round as a read set, straight from HBM: what raven::Polish hands the
// next round's racon::Polisher as targets (RavenLib/src/polish.cc:43-74: the polished sequences of round r are the targets of
// round r + 1).  The host has them too (rvn_polish_round returned them); this spares their way back — at C4 100 MB through
// the host's page cache and PCIe per round, ~40 ms with the GPU idle (profiles/r06_gaps.txt).  Bit-identical to
// rvn_reads_upload_codes of the sequences the round returned (tests/test_gpu_polish.py).
int rvn_polish_output_as_reads(rvn_engine* h, rvn_reads** out) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !out) return fail(RVN_EINVAL, "[raven_hip] rvn_polish_output_as_reads: NULL argument");
    Engine& e = h->e;
    if (!e.polish.last_cons.valid) return fail(RVN_EINVAL, "[raven_hip] rvn_polish_output_as_reads: no complete polishing round's consensus is resident");
    RVN_HIP(hipSetDevice(e.device));
    const u32 n = static_cast<u32>(e.polish.last_cons.off.size() - 1);
    return reads_from_device_codes(e, e.polish.stitched.ptr ? reinterpret_cast<const u8*>(e.polish.stitched.ptr) : nullptr, e.polish.last_cons.off, nullptr, n, out);
  });
}

int rvn_reads_load(rvn_engine* h, const char* path, rvn_reads** out, rvn_load_stats* stats) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !path || !out) return fail(RVN_EINVAL, "[raven_hip] rvn_reads_load: NULL argument");
    *out = nullptr;
    RVN_HIP(hipSetDevice(h->e.device));
    std::unique_ptr<rvn_reads> rr(new rvn_reads());
    LoadStats st;
    reads_load(h->e, path, rr->r, rr->names, st);
    if (stats) {
      stats->n_sequences = st.n_sequences;
      stats->n_bases = st.n_bases;
      stats->has_quality = st.has_quality;
      stats->parse_s = st.parse_s;
      stats->device_s = st.device_s;
      stats->total_s = st.total_s;
      stats->inflate_threads = st.inflate_threads;
      stats->members = st.members;
      stats->streaming = st.streaming;
      stats->restarted = st.restarted;
    }
    *out = rr.release();
    return RVN_OK;
  });
}

const char* rvn_reads_name(const rvn_reads* r, uint32_t i) {
  return (r && i < r->names.size()) ? r->names[i].c_str() : "";
}

int rvn_reads_info(const rvn_reads* r, uint32_t* n_reads, uint64_t* n_words, uint64_t* n_bases, uint64_t* n_quality_bytes,
                   int* quality_shift) {
  if (!r) return fail(RVN_EINVAL, "[raven_hip] NULL read set");
  if (n_reads) *n_reads = r->r.n;
  if (n_words) *n_words = r->r.n_words;
  if (n_bases) *n_bases = r->r.total_bases;
  if (n_quality_bytes) *n_quality_bytes = r->r.qual_shift >= 0 && !r->r.h_qual_off.empty() ? r->r.h_qual_off.back() : 0;
  if (quality_shift) *quality_shift = r->r.qual_shift;
  return RVN_OK;
}

int rvn_reads_fetch(const rvn_reads* r, uint64_t* packed, uint64_t* word_offsets, uint32_t* lengths, uint8_t* quals,
                    uint64_t* quality_offsets) {
  return guarded([&]() -> int {
    if (!r) return fail(RVN_EINVAL, "[raven_hip] NULL read set");
    const ReadsDev& rd = r->r;
    if (packed && rd.n_words) RVN_HIP(hipMemcpy(packed, rd.packed.ptr, rd.n_words * 8, hipMemcpyDeviceToHost));
    if (word_offsets) std::memcpy(word_offsets, rd.h_word_off.data(), rd.h_word_off.size() * 8);
    if (lengths && rd.n) std::memcpy(lengths, rd.h_len.data(), static_cast<size_t>(rd.n) * 4);
    if (rd.qual_shift >= 0 && !rd.h_qual_off.empty()) {
      if (quals && rd.h_qual_off.back()) RVN_HIP(hipMemcpy(quals, rd.quals.ptr, rd.h_qual_off.back(), hipMemcpyDeviceToHost));
      if (quality_offsets) std::memcpy(quality_offsets, rd.h_qual_off.data(), rd.h_qual_off.size() * 8);
    }
    return RVN_OK;
  });
}

int rvn_reads_attach_quality(rvn_engine* h, rvn_reads* rr, const uint8_t* quals, const uint64_t* offsets, int block_shift) {
  return guarded(h ? &h->e : nullptr, [&]() -> int {
    if (!h || !rr) return fail(RVN_EINVAL, "[raven_hip] rvn_reads_attach_quality: NULL argument");
    ReadsDev& r = rr->r;
    if (!quals) {  // detach
      r.qual_shift = -1;
      return RVN_OK;
    }
    if (!offsets || (block_shift != 0 && block_shift != 6))
      return fail(RVN_EINVAL, "[raven_hip] rvn_reads_attach_quality: offsets missing or block_shift not 0 / 6");
    for (u32 i = 0; i < r.n; ++i) {
      const u64 need = (static_cast<u64>(r.h_len[i]) + (1u << block_shift) - 1) >> block_shift;
      if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] < need)
        return fail(RVN_EINVAL, "[raven_hip] rvn_reads_attach_quality: offsets inconsistent with the read lengths");
    }
    RVN_HIP(hipSetDevice(h->e.device));
    const u64 total = offsets[r.n];
    u8* dq = r.quals.get<u8>(total + 16);
    u64* dqo = r.qual_off.get<u64>(static_cast<size_t>(r.n) + 1);
    if (total) RVN_HIP(hipMemcpy(dq, quals, total, hipMemcpyHostToDevice));
    RVN_HIP(hipMemcpy(dqo, offsets, (static_cast<size_t>(r.n) + 1) * 8, hipMemcpyHostToDevice));
    r.h_qual_off.assign(offsets, offsets + r.n + 1);
    r.qual_shift = block_shift;
    return RVN_OK;
  });
}

}  // extern "C"
