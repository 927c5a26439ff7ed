"""ctypes binding of libraven_hip.so (the C ABI in include/raven_hip.h).

This is the product path: it fails loudly when the HIP extension is missing or
no GPU is present — there is no CPU fallback (the CPU oracle lives in oracle/
and is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVN_LIB_PATH") or os.path.join(_HERE, "lib", "libraven_hip.so")  # override: A/B builds
TEST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libraven_hip_test.so")  # test hooks + host emulator, never the product

OVERLAP_DTYPE = np.dtype([
    ("lhs_id", "<u4"), ("lhs_begin", "<u4"), ("lhs_end", "<u4"),
    ("rhs_id", "<u4"), ("rhs_begin", "<u4"), ("rhs_end", "<u4"),
    ("score", "<u4"), ("strand", "<u4")])

ED_PAIR_DTYPE = np.dtype([
    ("lhs_read", "<u4"), ("lhs_begin", "<u4"), ("lhs_len", "<u4"),
    ("rhs_read", "<u4"), ("rhs_begin", "<u4"), ("rhs_len", "<u4"),
    ("strand", "<u4"), ("reserved", "<u4")])

ALIGN_PAIR_DTYPE = np.dtype([
    ("query_read", "<u4"), ("query_begin", "<u4"), ("query_len", "<u4"),
    ("target_read", "<u4"), ("target_begin", "<u4"), ("target_len", "<u4"),
    ("strand", "<u4"), ("reserved", "<u4")])

RVN_OK, RVN_EINVAL, RVN_ENODEVICE, RVN_EHIP, RVN_ENOMEM = 0, -1, -2, -3, -4

# The C ABI as ctypes sees it: name -> (restype, argtypes), one entry per symbol of include/raven_hip.h (tests/test_abi.py
# compares the keys with the header).  Handles and arrays are void pointers; _declare() applies the table to a loaded library.
_vp, _u32, _u64, _i32, _i64, _dbl, _cstr = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_int64, C.c_double, C.c_char_p
_pp, _pu32, _pu64, _pdbl = C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
_SIGNATURES = {
    "rvn_last_error": (_cstr, []),
    "rvn_device_count": (_i32, []),
    "rvn_engine_create": (_i32, [_pp, _u32, _u32, _u32, _u32, _u32, _u32, _i32]),
    "rvn_engine_destroy": (None, [_vp]),
    "rvn_reads_upload": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _u32, _pp]),
    "rvn_reads_upload_codes": (_i32, [_vp, _vp, _vp, _vp, _u32, _pp]),
    "rvn_polish_output_as_reads": (_i32, [_vp, _pp]),
    "rvn_reads_destroy": (None, [_vp]),
    "rvn_reads_load": (_i32, [_vp, _cstr, _pp, _vp]),
    "rvn_reads_name": (_cstr, [_vp, _u32]),
    "rvn_reads_info": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_reads_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_reads_attach_quality": (_i32, [_vp, _vp, _vp, _vp, _i32]),
    "rvn_engine_minimize": (_i32, [_vp, _vp, _u32, _u32, _i32]),
    "rvn_engine_filter": (_i32, [_vp, _dbl]),
    "rvn_engine_occurrence": (_u32, [_vp]),
    "rvn_engine_map_batch": (_i32, [_vp, _vp, _u32, _u32, _i32, _i32, _i32, _i32, _pu64]),
    "rvn_engine_map_fetch": (_i32, [_vp, _vp, _vp]),
    "rvn_engine_map_fetch_filtered": (_i32, [_vp, _vp, _vp, _pu64]),
    "rvn_engine_map_collect": (_i32, [_vp, _vp, _u32, _u32, _i32, _i32, _i32, _i32, _pp, _pp, _pp, _pp]),
    "rvn_free": (None, [_vp]),
    "rvn_engine_release_scratch": (_i32, [_vp]),
    "rvn_find_overlaps_and_create_piles": (_i32, [_vp, _vp, _dbl, _u32, _i32, _u64, _u64, _pp]),
    "rvn_pass1_pile_words": (_u64, [_vp]),
    "rvn_pass1_num_overlaps": (_u64, [_vp]),
    "rvn_pass1_fetch_piles": (_i32, [_vp, _vp, _vp]),
    "rvn_pass1_trim_and_annotate": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "rvn_pass1_find_chimeric_regions": (_i32, [_vp, _vp, _vp, _pp]),
    "rvn_pass1_fetch_overlaps": (_i32, [_vp, _vp, _vp]),
    "rvn_pass1_destroy": (None, [_vp]),
    "rvn_find_overlaps_and_repetitive_regions": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _u32, _dbl, _u64, _pp]),
    "rvn_pass2_num_overlaps": (_u64, [_vp]),
    "rvn_pass2_kmer_cells": (_u64, [_vp]),
    "rvn_pass2_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "rvn_pass2_destroy": (None, [_vp]),
    "rvn_resolve_repeat_induced_overlaps": (_i32, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pp]),
    "rvn_repeats_num_overlaps": (_u64, [_vp]),
    "rvn_repeats_num_regions": (_u64, [_vp]),
    "rvn_repeats_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_repeats_destroy": (None, [_vp]),
    "rvn_pass1_resolve": (_i32, [_vp, _vp, _u32, _dbl, _u32, _pp]),
    "rvn_resolve_contained_and_chimeric": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _dbl, _u32, _pp]),
    "rvn_resolved_num_overlaps": (_u64, [_vp]),
    "rvn_resolved_num_regions": (_u64, [_vp]),
    "rvn_resolved_coverage_words": (_u64, [_vp]),
    "rvn_resolved_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_resolved_destroy": (None, [_vp]),
    "rvn_filter_overlaps_by_identity": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _dbl]),
    "rvn_pile_add_layers": (_i32, [_vp, _vp, _u32, _u32, _vp, _u64]),
    "rvn_pile_add_kmers_batch": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "rvn_edit_distance_batch": (_i32, [_vp, _vp, _vp, _u32, _vp, _pdbl, _pu64]),
    "rvn_align_path_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _pp]),
    "rvn_paths_info": (_i32, [_vp, _pu32, _pu64, _pu64, _pu32]),
    "rvn_paths_fetch": (_i32, [_vp, _vp, _vp, _vp]),
    "rvn_paths_fetch_ops": (_i32, [_vp, _vp, _vp]),
    "rvn_paths_destroy": (None, [_vp]),
    "rvn_poa_consensus_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp,
                                       _vp, _vp, _vp, _pdbl]),
    "rvn_polish_round": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                _vp, _vp]),
    "rvn_shard_sketch": (_i32, [_vp, _vp, _i32, _pu64]),
    "rvn_shard_sketch_range": (_i32, [_vp, _vp, _u32, _u32, _i32, _i32, _vp]),
    "rvn_shard_sketch_fetch": (_i32, [_vp, _vp, _vp]),
    "rvn_shard_index_build": (_i32, [_vp, _vp, _vp, _u64, _i32]),
    "rvn_shard_key_counts": (_i32, [_vp, _vp]),
    "rvn_engine_set_occurrence": (_i32, [_vp, _u32]),
    "rvn_shard_join": (_i32, [_vp, _u32, _i32, _i32, _pu64]),
    "rvn_shard_join_range": (_i32, [_vp, _u32, _i32, _i32, _u32, _u32, _pu64]),
    "rvn_shard_join_fetch": (_i32, [_vp, _vp, _vp, _vp]),
    "rvn_shard_chain": (_i32, [_vp, _vp, _vp, _vp, _vp, _pu64]),
    "rvn_shard_piles": (_i32, [_vp, _vp, _u32, _vp, _u64, _u32, _pp]),
    "rvn_shard_piles_create": (_i32, [_vp, _vp, _u32, _pp]),
    "rvn_shard_piles_merge": (_i32, [_vp, _vp, _u64, _u32]),
    "rvn_shard_piles_merge_dev": (_i32, [_vp, _vp, _vp, _u64, _u32]),
    "rvn_shard_sketch_fetch_dev": (_i32, [_vp, _vp, _vp]),
    "rvn_shard_index_build_dev": (_i32, [_vp, _vp, _vp, _u64, _i32, _u64]),
    "rvn_shard_key_histogram": (_i32, [_vp, _vp, _vp, _u32, _pu32]),
    "rvn_shard_join_fetch_dev": (_i32, [_vp, _vp, _vp, _vp]),
    "rvn_shard_chain_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _pu64]),
    "rvn_engine_map_fetch_dev": (_i32, [_vp, _vp, _vp]),
    "rvn_shard_split_minimizers_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp]),
    "rvn_shard_count_flagged_dev": (_i32, [_vp, _vp, _u64, _vp]),
    "rvn_shard_adjacent_diff_dev": (_i32, [_vp, _vp, _u64, _vp]),
    "rvn_shard_regroup_dev": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "rvn_shard_split_overlaps_dev": (_i32, [_vp, _vp, _u64, _vp, _u32, _u32, _vp, _vp]),
    "rvn_shard_piles_merge_parts_dev": (_i32, [_vp, _u32, _vp, _vp, _u32]),
    "rvn_shard_piles_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _u64, _u32, _pp]),
    "rvn_polish_map_best": (_i32, [_vp, _vp, _vp, _u32, _u32, _dbl, _vp, _vp, _vp]),
    "rvn_polish_set_best": (_i32, [_vp, _vp, _vp, _u32]),
    "rvn_polish_round_range": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _u32, _i32, _i32, _i32, _i32, _u64, _u64,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_group_create": (_i32, [_pp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _u32]),
    "rvn_group_destroy": (None, [_vp]),
    "rvn_group_size": (_u32, [_vp]),
    "rvn_group_engine": (_vp, [_vp, _u32]),
    "rvn_group_find_overlaps_and_create_piles": (_i32, [_vp, _vp, _vp, _vp, _u32, _dbl, _u32, _i32, _u64, _vp, _pp]),
    "rvn_group_find_overlaps_and_create_piles_batched": (_i32, [_vp, _vp, _vp, _vp, _u32, _dbl, _u32, _i32, _u64,
                                                                _u64, _vp, _pp]),
    "rvn_group_polish_round": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _dbl, _dbl, _u32, _i32, _i32,
                                      _i32, _i32, _vp, _vp, _vp, _vp]),
    "rvn_group_polish_round_q": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _i32, _dbl, _dbl,
                                        _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "rvn_group_peer_access": (_i32, [_vp, _vp]),
    "rvn_group_find_overlaps_and_repetitive_regions": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _dbl, _u32,
                                                              _dbl, _u64, _pp]),
    "rvn_group_filter_overlaps_by_identity": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _dbl]),
    "rvn_overlap_update_and_type": (_i32, [_vp, _u64, _vp, _vp, _vp, _u32, _vp, _vp]),
    "rvn_layout_force_directed": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _vp]),
    "rvn_construct_assembly_graph": (_i32, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _pp]),
    "rvn_graph_from_edges": (_i32, [_vp, _u32, _u64, _vp, _vp, _vp, _pp]),
    "rvn_graph_info": (_i32, [_vp, _pu32, _pu64, _pu64]),
    "rvn_graph_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_graph_mark_transitive": (_i32, [_vp, _vp, _pu64]),
    "rvn_graph_fetch_transitive": (_i32, [_vp, _vp, _vp, _pu64]),
    "rvn_graph_mark_long_edges": (_i32, [_vp, _vp, _vp, _vp, _pu64]),
    "rvn_graph_destroy": (None, [_vp]),
    "rvn_tiling_from_piles": (_i32, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _pp]),
    "rvn_tiling_from_segments": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _pp]),
    "rvn_tiling_info": (_i32, [_vp, _pu32, _pu64]),
    "rvn_tiling_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_tiling_destroy": (None, [_vp]),
    "rvn_graph_create_unitigs": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _pp]),
    "rvn_unitigs_info": (_i32, [_vp, _pu32, _pu32, _pu64, _pu64, _pu64]),
    "rvn_unitigs_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_unitigs_destroy": (None, [_vp]),
    "rvn_unitigs_as_reads": (_i32, [_vp, _vp, _vp, _vp, _i32, _pp]),
    "rvn_tiling_as_reads": (_i32, [_vp, _vp, _vp, _vp, _u32, _pp]),
    "rvn_tiling_paths_as_reads": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _pp]),
    "rvn_path_similarity_batch": (_i32, [_vp, _vp, _vp, _u32, _dbl, _vp, _vp]),
    "rvn_tiling_slices_as_reads": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _pp]),
    "rvn_graph_edge_similarity": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rvn_engine_set_option": (_i32, [_vp, _cstr, _i64, _vp]),
    "rvn_polish_set_chunk_windows": (_u64, [_vp, _u64]),
    "rvn_polish_fetch_layers": (_i32, [_vp, _vp, _u64, _pu64]),
    "rvn_polish_target_reads": (_i32, [_vp, _vp, _u32]),
    "rvn_poa_phase_cycles": (None, [_vp, _vp]),
    "rvn_poa_work": (None, [_vp, _vp]),
    "rvn_poa_set_mode": (_i32, [_vp, _i32]),
    "rvn_poa_fallback_windows": (_u32, [_vp]),
    "rvn_poa_wide_windows": (_u32, [_vp]),
    "rvn_poa_narrow_windows": (_u32, [_vp]),
    "rvn_engine_sketch": (_i32, [_vp, _vp, _u32, _u32, _i32, _pu64]),
    "rvn_engine_sketch_fetch": (_i32, [_vp, _vp, _vp, _vp]),
    "rvn_engine_index_size": (_i32, [_vp, _pu64, _pu64]),
    "rvn_engine_index_fetch": (_i32, [_vp, _vp, _vp]),
    "rvn_engine_counters": (_i32, [_vp, _vp]),
    "rvn_engine_num_stages": (_i32, []),
    "rvn_engine_stage_name": (_cstr, [_i32]),
    "rvn_engine_stage_ms": (_i32, [_vp, _vp, _vp, _i32]),
    "rvn_engine_reset_stats": (None, [_vp]),
    "rvn_engine_set_timing": (None, [_vp, _i32]),
    "rvn_engine_set_kernel_timing": (None, [_vp, _i32]),
    "rvn_engine_num_kernel_sites": (_i32, []),
    "rvn_engine_kernel_site_name": (_cstr, [_i32]),
    "rvn_engine_kernel_ms": (_i32, [_vp, _vp, _vp, _i32]),
}
SYMBOLS = list(_SIGNATURES)

# TEST INFRASTRUCTURE: what include/raven_hip_test.h declares on top (libraven_hip_test.so only)
_TEST_SIGNATURES = {
    "rvn_poa_banded_emulate": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                      _vp, _i32]),
    "rvn_test_hash": (_u64, [_u64, _u32, _i32]),
    "rvn_test_canonical": (_i32, [_vp, _u32, _u32, _i32, _pu64, _pu32]),
    "rvn_test_low_complexity": (_i32, [_vp, _u32]),
    "rvn_test_nw_breakpoints": (_i32, [_vp, _u32, _vp, _u32, _u32, _u32, _u32, _u32, _i32, _u32, _u32, _i32, _vp,
                                       _vp, _vp]),
    "rvn_test_find_chimeric_regions": (_i64, [_vp, _u32, _vp, _u64]),
    "rvn_test_piles_annotate": (_i32, [_vp, _vp, _u32, _u32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _pp]),
    "rvn_test_overlap_update_and_type": (_i32, [_vp, _u64, _vp, _vp, _vp, _u32, _vp, _vp]),
    "rvn_test_parse_file": (_i32, [_cstr, _i32, _u32, _i32, _u64, _pp, _pp, _pp, _pu32, _pp, _vp]),
    "rvn_test_inflate_fast": (_i32, [_vp, _u64, _vp, _u64, _u64, _vp]),
    "rvn_test_freelist": (_i32, [_u64, _u64, _vp, _u32, _vp, _vp]),
    "rvn_test_ed_lane": (_i32, [_vp, _vp, _vp, _u32, _vp, _i32, _vp]),
    "rvn_test_edit_distance_dev": (_i32, [_vp, _vp, _vp, _u32, _vp, _i32, _vp]),
    "rvn_test_match_probe": (_i32, [_vp, _vp, _vp, _u64, _vp, _u32, _i32, _i32, _pp, _pp, _vp, _vp, _pu64]),
    "rvn_test_radix_sort_pairs": (_i32, [_i32, _vp, _vp, _u64, _i32, _i32]),
    "rvn_test_exclusive_scan": (_i32, [_i32, _vp, _u64, _u32, _u32, _vp]),
    "rvn_test_compact_overlap_list": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "rvn_test_engine_scratch_bytes": (_i32, [_vp, _pu64]),
    "rvn_test_best_overlap": (_i32, [_vp, _u64, _vp, _u32, _u32, _dbl, _vp, _u32, _vp, _vp, _u32]),
    "rvn_test_second_pass": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _u32, _vp, _u32, _vp]),
    "rvn_test_align_path_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _pp, _vp, _vp]),
    "rvn_test_std_sort_lendesc": (None, [_vp, _u64]),
    "rvn_test_heap_sort_lendesc": (None, [_vp, _u64]),
}
TEST_SYMBOLS = list(_TEST_SIGNATURES)


class RavenHipError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libraven_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RavenHipError(
            "libraven_hip.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or raven_amd/csrc/build.sh" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    _declare(L)
    _lib = L
    return L


_test_lib = None


def test_lib():
    """TEST INFRASTRUCTURE: libraven_hip_test.so = the product's objects + the rvn_test_* hooks and the host wavefront
    emulator (include/raven_hip_test.h).  Only tests/ and tools/ call this; the product binding above never does."""
    global _test_lib
    if _test_lib is not None:
        return _test_lib
    if not os.path.exists(TEST_LIB_PATH):
        raise RavenHipError("libraven_hip_test.so not built (%s): run raven_amd/csrc/build.sh" % TEST_LIB_PATH)
    L = C.CDLL(TEST_LIB_PATH)
    _declare(L)
    _declare(L, _TEST_SIGNATURES)
    _test_lib = L
    return L


def _declare(L, signatures=_SIGNATURES):
    for name, (restype, argtypes) in signatures.items():
        f = getattr(L, name)
        f.restype = restype
        f.argtypes = argtypes


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check(rc):
    if rc != RVN_OK:
        msg = lib().rvn_last_error().decode(errors="replace")
        if rc == RVN_EINVAL:
            raise ValueError(msg)
        raise RavenHipError("rc=%d: %s" % (rc, msg))


def device_count() -> int:
    return int(lib().rvn_device_count())


class CodeSet:
    """Just enough of a ReadSet for a Reads handle made from one-byte codes (Engine.upload_codes)."""

    def __init__(self, lengths):
        self.lengths = np.asarray(lengths, dtype=np.uint32)
        self.n = int(self.lengths.shape[0])
        self.ids = np.arange(self.n, dtype=np.uint32)

    @property
    def total_bases(self):
        return int(self.lengths.astype(np.int64).sum())


class Reads:
    def __init__(self, engine: "Engine", rs, codes=None, handle=None):
        self.rs = rs
        self.engine = engine
        h = C.c_void_p()
        if handle is not None:  # a read set the library made on the device (Engine.polish_output_as_reads)
            self._h = handle
            return
        if codes is not None:  # one-byte codes, packed on the device
            off = np.zeros(rs.n + 1, dtype=np.uint64)
            np.cumsum(rs.lengths.astype(np.uint64), out=off[1:])
            flat = np.ascontiguousarray(codes, dtype=np.uint8)
            assert flat.shape[0] == int(off[-1])
            _check(lib().rvn_reads_upload_codes(engine._h, _p(flat), _p(off), None, rs.n, C.byref(h)))
            self._h = h
            return
        packed = np.ascontiguousarray(rs.packed, dtype=np.uint64)
        n_words = int(rs.word_offsets[-1])
        _check(lib().rvn_reads_upload(engine._h, _p(packed), n_words,
                                      _p(np.ascontiguousarray(rs.word_offsets, dtype=np.uint64)),
                                      _p(np.ascontiguousarray(rs.lengths, dtype=np.uint32)),
                                      _p(np.ascontiguousarray(rs.ids, dtype=np.uint32)), rs.n, C.byref(h)))
        self._h = h

    @property
    def n(self):
        return self.rs.n

    def fetch(self):
        """Device-resident read set back on the host: (packed words, word offsets, lengths, quality bytes or None,
        quality offsets or None, quality shift)."""
        n, nw, nb, nq, sh = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        _check(lib().rvn_reads_info(self._h, C.byref(n), C.byref(nw), C.byref(nb), C.byref(nq), C.byref(sh)))
        packed = np.zeros(nw.value, dtype=np.uint64)
        woff = np.zeros(n.value + 1, dtype=np.uint64)
        lens = np.zeros(n.value, dtype=np.uint32)
        q = np.zeros(nq.value, dtype=np.uint8) if sh.value >= 0 else None
        qoff = np.zeros(n.value + 1, dtype=np.uint64) if sh.value >= 0 else None
        _check(lib().rvn_reads_fetch(self._h, _p(packed), _p(woff), _p(lens), _p(q), _p(qoff)))
        return packed, woff, lens, q, qoff, sh.value

    def attach_quality(self, quals, block_shift=0):
        """Keep the reads' qualities in HBM for the polishing rounds: `quals` = list of per-read uint8 arrays of
        Phred+33 bytes, one per 2^block_shift bases (0: per base; 6: biosoup block qualities + 33)."""
        if isinstance(quals, tuple):  # (flat uint8 array, uint64 offsets[n + 1]) as they are
            flat = np.ascontiguousarray(quals[0], dtype=np.uint8)
            off = np.ascontiguousarray(quals[1], dtype=np.uint64)
        else:
            lens = np.array([len(q) for q in quals], dtype=np.uint64)
            off = np.zeros(self.rs.n + 1, dtype=np.uint64)
            np.cumsum(lens, out=off[1:])
            flat = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.uint8) for q in quals])
                                        if len(quals) else np.zeros(0, np.uint8))
        _check(lib().rvn_reads_attach_quality(self.engine._h, self._h, _p(flat), _p(off), int(block_shift)))

    def close(self):
        if getattr(self, "_h", None):
            lib().rvn_reads_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass


def _fetch_resolved(h, n):
    """rvn_resolved_fetch of everything, then rvn_resolved_destroy: the dict Pass1.resolve and
    Engine.resolve_contained_and_chimeric return."""
    L = lib()
    try:
        begin, end = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        invalid, contained, chimeric = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        reg = np.zeros((int(L.rvn_resolved_num_regions(h)), 2), dtype=np.uint32)
        roff = np.zeros(n + 1, dtype=np.uint32)
        median = np.zeros(1, dtype=np.uint16)
        ovl = np.zeros(int(L.rvn_resolved_num_overlaps(h)), dtype=OVERLAP_DTYPE)
        off = np.zeros(n + 1, dtype=np.uint32)
        words = int(L.rvn_resolved_coverage_words(h))
        cov = np.zeros(words, dtype=np.uint16)
        stats = np.zeros(6, dtype=np.uint64)  # rvn_resolve_stats: 4 x u64, 4 x u32
        _check(L.rvn_resolved_fetch(h, _p(begin), _p(end), _p(invalid), _p(contained), _p(chimeric), _p(reg), _p(roff),
                                    _p(median), _p(ovl), _p(off), _p(cov), _p(stats)))
    finally:
        L.rvn_resolved_destroy(h)
    s32 = stats[4:].view(np.uint32)
    return dict(begin=begin, end=end, invalid=invalid, contained=contained, chimeric=chimeric, regions=reg,
                region_offsets=roff, median=int(median[0]), overlaps=ovl, offsets=off, coverage=cov,
                stats=dict(dropped_by_update=(int(stats[0]), int(stats[1])), dropped_by_filter=int(stats[2]),
                           dropped_by_containment=int(stats[3]), contained=(int(s32[0]), int(s32[1])), cut=int(s32[2]),
                           invalidated=int(s32[3])))


class Pass1:
    def __init__(self, h, n):
        self._h = h
        self.n = n

    def resolve(self, reads=None, identity=0.0, coverage=4, phases=3):
        """raven::ResolveContainedReads (phases & 1) and raven::ResolveChimericSequences (phases & 2) on the lists and the
        coverage of this pass in HBM (rvn_pass1_resolve); TrimAndAnnotatePiles(coverage) first when it has not run yet.
        Returns dict(begin, end (cells), invalid, contained, chimeric, regions ((k, 2) cells), region_offsets[n + 1],
        median (the global one of phase 2), overlaps, offsets[n + 1] (after the last phase that ran), coverage (empty:
        it stays on the pass, see piles()), stats)."""
        L = lib()
        h = C.c_void_p()
        _check(L.rvn_pass1_resolve(self._h, reads._h if reads is not None else None, int(coverage), float(identity),
                                   int(phases), C.byref(h)))
        return _fetch_resolved(h, self.n)

    def piles(self):
        L = lib()
        words = int(L.rvn_pass1_pile_words(self._h))
        data = np.zeros(words, dtype=np.uint16)
        off = np.zeros(self.n + 1, dtype=np.uint64)
        _check(L.rvn_pass1_fetch_piles(self._h, _p(data), _p(off)))
        return data, off

    def merge(self, overlaps, kmax=32):
        """Sharded pass: one flush (merge + AddLayers + truncation) of overlaps in (query read, emission) order."""
        overlaps = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        _check(lib().rvn_shard_piles_merge(self._h, _p(overlaps), overlaps.shape[0], kmax))

    def merge_parts_dev(self, parts, kmax=32):
        """rvn_shard_piles_merge_parts_dev: parts = [(device pointer, number of overlaps), ...] in ascending lhs order."""
        n = len(parts)
        ptrs = (C.c_void_p * max(n, 1))(*[int(a) for a, _ in parts])
        cnts = (C.c_uint64 * max(n, 1))(*[int(c) for _, c in parts])
        L = lib()
        _check(L.rvn_shard_piles_merge_parts_dev(self._h, n, ptrs, cnts, kmax))

    def merge_dev(self, d_overlaps, d_read_off, n, kmax=32):
        _check(lib().rvn_shard_piles_merge_dev(self._h, d_overlaps, d_read_off, int(n), kmax))

    def trim_and_annotate(self, coverage=4):
        """Pile::FindValidRegion(coverage) + FindMedian for every pile, in place in HBM: (begin, end, median, invalid)."""
        L = lib()
        b = np.zeros(self.n, dtype=np.uint32)
        e = np.zeros(self.n, dtype=np.uint32)
        m = np.zeros(self.n, dtype=np.uint16)
        inv = np.zeros(self.n, dtype=np.uint8)
        _check(L.rvn_pass1_trim_and_annotate(self._h, int(coverage), _p(b), _p(e), _p(m), _p(inv)))
        return b, e, m, inv.astype(bool)

    def find_chimeric_regions(self, invalid):
        """Pile::FindChimericRegions of every valid pile (after trim_and_annotate): list of (k, 2) uint32 arrays of
        (begin, end) cells, one per pile."""
        inv = np.ascontiguousarray(invalid, dtype=np.uint8)
        off = np.zeros(self.n + 1, dtype=np.uint32)
        ptr = C.c_void_p()
        _check(lib().rvn_pass1_find_chimeric_regions(self._h, _p(inv), _p(off), C.byref(ptr)))
        total = int(off[-1])
        try:
            flat = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(max(2 * total, 1),))[:2 * total].copy()
        finally:
            lib().rvn_free(ptr)
        flat = flat.reshape(-1, 2)
        return [flat[int(off[i]):int(off[i + 1])] for i in range(self.n)]

    def overlaps(self):
        L = lib()
        n = int(L.rvn_pass1_num_overlaps(self._h))
        ovl = np.zeros(n, dtype=OVERLAP_DTYPE)
        off = np.zeros(self.n + 1, dtype=np.uint32)
        _check(L.rvn_pass1_fetch_overlaps(self._h, _p(ovl), _p(off)))
        return ovl, off

    def close(self):
        if getattr(self, "_h", None):
            lib().rvn_pass1_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass


def _pack_poa_windows(windows):
    """Flat arrays of a window batch as rvn_poa_consensus_batch / rvn_poa_banded_emulate take them."""
    codes, quals, loff, begins, ends, hasq, woff, ooff = [], [], [0], [], [], [], [0], [0]
    any_q = False
    for wdw in windows:
        layers = wdw["layers"]
        k = len(layers)
        blen = len(layers[0])
        b = wdw.get("begins") or [0] * k
        e_ = wdw.get("ends") or [max(blen - 1, 0)] * k
        q = wdw.get("quals")
        for i, lay in enumerate(layers):
            lay = np.asarray(lay, dtype=np.uint8)
            codes.append(lay)
            loff.append(loff[-1] + lay.shape[0])
            begins.append(int(b[i]))
            ends.append(int(e_[i]))
            if q is not None and q[i] is not None:
                quals.append(np.asarray(q[i], dtype=np.uint8))
                hasq.append(1)
                any_q = True
            else:
                quals.append(np.full(lay.shape[0], 33, dtype=np.uint8))
                hasq.append(0)
        woff.append(woff[-1] + k)
        ooff.append(ooff[-1] + 4 * blen + 256)
    nw = len(windows)
    return dict(codes=np.concatenate(codes) if codes else np.zeros(0, np.uint8),
                quals=np.concatenate(quals) if any_q else None, loff=np.asarray(loff, dtype=np.uint64),
                begins=np.asarray(begins, dtype=np.uint32), ends=np.asarray(ends, dtype=np.uint32),
                hasq=np.asarray(hasq, dtype=np.uint32), woff=np.asarray(woff, dtype=np.uint32), nw=nw,
                out=np.zeros(ooff[-1] + 16, dtype=np.uint8), ooff=np.asarray(ooff, dtype=np.uint64),
                out_len=np.zeros(nw, dtype=np.uint32), status=np.zeros(nw, dtype=np.uint32))


def _unpack_poa_consensus(a):
    ooff = a["ooff"]
    return [a["out"][int(ooff[i]): int(ooff[i]) + int(a["out_len"][i])].copy() for i in range(a["nw"])]


def poa_banded_emulate(windows, m=3, n=-5, g=-4, trim=True, variant=4):
    """TEST INFRASTRUCTURE: poa4.hip's phase functions stepped through on the HOST by the wavefront emulator (no GPU,
    no engine).  First attempt of the escalation chain only: status 8 = the window needs a wider band (or is beyond
    the kernel's limits).  Returns (list of consensus code arrays, status array)."""
    a = _pack_poa_windows(windows)
    T = test_lib()
    rc = T.rvn_poa_banded_emulate(
        _p(a["codes"]), _p(a["quals"]), _p(a["loff"]), _p(a["begins"]), _p(a["ends"]), _p(a["hasq"]), _p(a["woff"]),
        a["nw"], m, n, g, int(trim), _p(a["out"]), _p(a["ooff"]), _p(a["out_len"]), _p(a["status"]), int(variant))
    if rc != RVN_OK:
        raise (ValueError if rc == RVN_EINVAL else RavenHipError)(T.rvn_last_error().decode(errors="replace"))
    return _unpack_poa_consensus(a), a["status"]


class Engine:
    """Mirror of ram::MinimizerEngine over the C ABI (defaults as in ram)."""

    def __init__(self, k=15, w=5, bandwidth=500, chain=4, matches=100, gap=10000, device=0):
        self.k, self.w = min(max(k, 1), 31), w
        h = C.c_void_p()
        _check(lib().rvn_engine_create(C.byref(h), k, w, bandwidth, chain, matches, gap, device))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().rvn_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def upload(self, rs) -> Reads:
        return Reads(self, rs)

    def load(self, path) -> Reads:
        """raven::CreateParser(path) + Parse(-1) straight into HBM (rvn_reads_load): gzip members inflated by a pool of
        host threads, records found by one memchr pass, text cut into packed reads on the device.  The returned handle's .rs holds lengths / ids / names and .load_stats."""
        h = C.c_void_p()
        st = np.zeros(8, dtype=np.uint64)
        _check(lib().rvn_reads_load(self._h, str(path).encode(), C.byref(h), _p(st)))
        n = C.c_uint32(0)
        lib().rvn_reads_info(h, C.byref(n), None, None, None, None)
        lengths = np.zeros(n.value, dtype=np.uint32)
        lib().rvn_reads_fetch(h, None, None, _p(lengths), None, None)
        rs = CodeSet(lengths)
        rs.names = [lib().rvn_reads_name(h, i).decode() for i in range(n.value)]
        r = Reads.__new__(Reads)
        r.rs, r.engine, r._h = rs, self, h
        r.load_stats = {"n_sequences": int(st[0]), "n_bases": int(st[1]), "has_quality": int(st[2] & 0xFFFFFFFF),
                        "parse_s": float(st[3:4].view(np.float64)[0]), "device_s": float(st[4:5].view(np.float64)[0]),
                        "total_s": float(st[5:6].view(np.float64)[0]), "inflate_threads": int(st[6] & 0xFFFFFFFF),
                        "members": int(st[6] >> 32), "streaming": int(st[7] & 0xFFFFFFFF), "restarted": int(st[7] >> 32)}
        return r

    def upload_codes(self, code_arrays) -> Reads:
        """Read set from one-byte code arrays (values 0..3), packed on the device (rvn_reads_upload_codes): how the
        consensus of one polishing round becomes the target set of the next."""
        lens = [int(len(c)) for c in code_arrays]
        flat = np.concatenate([np.asarray(c, dtype=np.uint8) for c in code_arrays]) if lens else np.zeros(0, np.uint8)
        return Reads(self, CodeSet(lens), codes=flat)

    def polish_output_as_reads(self, lengths) -> Reads:
        """The consensus of this engine's last complete polish_round as the next round's target set, straight from HBM
        (rvn_polish_output_as_reads): the same read set upload_codes(<what the round returned>) gives, without the 100 MB
        of a C4 round going through host memory and PCIe again.  lengths = the lengths of the sequences the round returned."""
        h = C.c_void_p()
        _check(lib().rvn_polish_output_as_reads(self._h, C.byref(h)))
        return Reads(self, CodeSet([int(x) for x in lengths]), handle=h)

    # -- ram::MinimizerEngine interface -----------------------------------------------------
    def minimize(self, reads: Reads, first=0, last=None, minhash=False):
        last = reads.n if last is None else last
        _check(lib().rvn_engine_minimize(self._h, reads._h, first, last, int(minhash)))

    def filter(self, f):
        _check(lib().rvn_engine_filter(self._h, float(f)))

    @property
    def occurrence(self):
        return int(lib().rvn_engine_occurrence(self._h))

    def map_batch(self, reads: Reads, first=0, last=None, avoid_equal=True, avoid_symmetric=True, minhash=False,
                  want_filtered=False):
        last = reads.n if last is None else last
        n = C.c_uint64(0)
        _check(lib().rvn_engine_map_batch(self._h, reads._h, first, last, int(avoid_equal), int(avoid_symmetric),
                                          int(minhash), int(want_filtered), C.byref(n)))
        ovl = np.zeros(n.value, dtype=OVERLAP_DTYPE)
        off = np.zeros(last - first + 1, dtype=np.uint32)
        _check(lib().rvn_engine_map_fetch(self._h, _p(ovl), _p(off)))
        res = dict(overlaps=ovl, read_offsets=off)
        if want_filtered:
            tot = C.c_uint64(0)
            _check(lib().rvn_engine_map_fetch_filtered(self._h, None, None, C.byref(tot)))
            pos = np.zeros(tot.value, dtype=np.uint32)
            foff = np.zeros(last - first + 1, dtype=np.uint32)
            _check(lib().rvn_engine_map_fetch_filtered(self._h, _p(pos), _p(foff), C.byref(tot)))
            res["filtered"] = pos
            res["filtered_offsets"] = foff
        return res

    # -- raven::FindOverlapsAndCreatePiles ---------------------------------------------------
    def find_overlaps_and_create_piles(self, reads: Reads, freq=0.001, kmax=32, use_minhash=False,
                                       index_batch_bases=1 << 32, flush_bases=1 << 30) -> Pass1:
        h = C.c_void_p()
        _check(lib().rvn_find_overlaps_and_create_piles(self._h, reads._h, float(freq), kmax, int(use_minhash),
                                                        index_batch_bases, flush_bases, C.byref(h)))
        return Pass1(h, reads.n)

    # -- stage-level entry points of the sharded pass (raven_amd/sharded.py) ------------------------
    def shard_sketch(self, own_reads: Reads, index_minhash=False):
        n = C.c_uint64(0)
        _check(lib().rvn_shard_sketch(self._h, own_reads._h, int(index_minhash), C.byref(n)))
        values = np.zeros(n.value, dtype=np.uint64)
        origins = np.zeros(n.value, dtype=np.uint64)
        _check(lib().rvn_shard_sketch_fetch(self._h, _p(values), _p(origins)))
        return values, origins

    def shard_sketch_range_count(self, own_reads: Reads, first, last, index_minhash=False, foreign=False) -> int:
        """rvn_shard_sketch_range: reads [first, last) of the handle; foreign = reads of an earlier index batch (their
        minhash-selected minimizers as query-only entries).  Fetch with shard_sketch_fetch / shard_sketch_fetch_dev."""
        n = C.c_uint64(0)
        _check(lib().rvn_shard_sketch_range(self._h, own_reads._h, int(first), int(last), int(index_minhash), int(foreign),
                                            C.byref(n)))
        return int(n.value)

    def shard_sketch_fetch(self, n):
        values = np.zeros(n, dtype=np.uint64)
        origins = np.zeros(n, dtype=np.uint64)
        if n:
            _check(lib().rvn_shard_sketch_fetch(self._h, _p(values), _p(origins)))
        return values, origins

    def shard_index_build(self, values, origins, all_query=False):
        values = np.ascontiguousarray(values, dtype=np.uint64)
        origins = np.ascontiguousarray(origins, dtype=np.uint64)
        _check(lib().rvn_shard_index_build(self._h, _p(values), _p(origins), values.shape[0], int(all_query)))

    def shard_key_counts(self):
        m, u = C.c_uint64(0), C.c_uint64(0)
        _check(lib().rvn_engine_index_size(self._h, C.byref(m), C.byref(u)))
        counts = np.zeros(u.value, dtype=np.uint32)
        _check(lib().rvn_shard_key_counts(self._h, _p(counts)))
        return counts

    def set_occurrence(self, occurrence):
        _check(lib().rvn_engine_set_occurrence(self._h, int(occurrence)))

    def shard_join(self, n_reads_total, avoid_equal=True, avoid_symmetric=True, query_first=0, query_last=None):
        h = C.c_uint64(0)
        query_last = n_reads_total if query_last is None else query_last
        _check(lib().rvn_shard_join_range(self._h, n_reads_total, int(avoid_equal), int(avoid_symmetric), query_first,
                                          query_last, C.byref(h)))
        grp = np.zeros(h.value, dtype=np.uint64)
        pos = np.zeros(h.value, dtype=np.uint64)
        seg = np.zeros(n_reads_total + 1, dtype=np.uint64)
        _check(lib().rvn_shard_join_fetch(self._h, _p(grp), _p(pos), _p(seg)))
        return grp, pos, seg

    def shard_chain(self, own_reads: Reads, grp, pos, seg_off):
        grp = np.ascontiguousarray(grp, dtype=np.uint64)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
        assert seg_off.shape[0] == own_reads.n + 1
        n = C.c_uint64(0)
        _check(lib().rvn_shard_chain(self._h, own_reads._h, _p(grp), _p(pos), _p(seg_off), C.byref(n)))
        ovl = np.zeros(n.value, dtype=OVERLAP_DTYPE)
        off = np.zeros(own_reads.n + 1, dtype=np.uint32)
        _check(lib().rvn_engine_map_fetch(self._h, _p(ovl), _p(off)))
        return ovl, off

    def shard_piles_create(self, lengths) -> Pass1:
        """Empty piles of ALL reads; Pass1.merge / merge_dev add the Map outputs of one flush window each."""
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        h = C.c_void_p()
        _check(lib().rvn_shard_piles_create(self._h, _p(lengths), lengths.shape[0], C.byref(h)))
        return Pass1(h, lengths.shape[0])

    def shard_piles(self, lengths, overlaps, kmax=32) -> Pass1:
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        overlaps = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        h = C.c_void_p()
        _check(lib().rvn_shard_piles(self._h, _p(lengths), lengths.shape[0], _p(overlaps), overlaps.shape[0], kmax,
                                     C.byref(h)))
        return Pass1(h, lengths.shape[0])

    # device-pointer variants (pointers are integers, e.g. torch.Tensor.data_ptr() of CUDA tensors)
    def shard_sketch_count(self, own_reads: Reads, index_minhash=False) -> int:
        n = C.c_uint64(0)
        _check(lib().rvn_shard_sketch(self._h, own_reads._h, int(index_minhash), C.byref(n)))
        return int(n.value)

    def shard_sketch_fetch_dev(self, d_values, d_origins):
        _check(lib().rvn_shard_sketch_fetch_dev(self._h, d_values, d_origins))

    def shard_index_build_dev(self, d_values, d_origins, n, all_query, n_flagged):
        _check(lib().rvn_shard_index_build_dev(self._h, d_values, d_origins, int(n), int(all_query), int(n_flagged)))

    def shard_key_histogram(self):
        hist = np.zeros(65536, dtype=np.uint64)
        over = np.zeros(1 << 20, dtype=np.uint32)
        n = C.c_uint32(0)
        _check(lib().rvn_shard_key_histogram(self._h, _p(hist), _p(over), over.shape[0], C.byref(n)))
        return hist.astype(np.int64), over[:n.value].astype(np.int64)

    def shard_join_count(self, n_reads_total, avoid_equal=True, avoid_symmetric=True, query_first=0, query_last=None) -> int:
        h = C.c_uint64(0)
        query_last = n_reads_total if query_last is None else query_last
        _check(lib().rvn_shard_join_range(self._h, n_reads_total, int(avoid_equal), int(avoid_symmetric), query_first,
                                          query_last, C.byref(h)))
        return int(h.value)

    # partition / regroup steps of the sharded pass on device pointers (shard.hip)
    def shard_split_minimizers_dev(self, d_val, d_org, n, world, d_val_out, d_org_out):
        counts = (C.c_uint64 * world)()
        L = lib()
        _check(L.rvn_shard_split_minimizers_dev(self._h, d_val, d_org, int(n), world, d_val_out, d_org_out, counts))
        return [int(x) for x in counts]

    def shard_count_flagged_dev(self, d_org, n) -> int:
        c = C.c_uint64(0)
        L = lib()
        _check(L.rvn_shard_count_flagged_dev(self._h, d_org, int(n), C.byref(c)))
        return int(c.value)

    def shard_adjacent_diff_dev(self, d_seg, n, d_cnt):
        L = lib()
        _check(L.rvn_shard_adjacent_diff_dev(self._h, d_seg, int(n), d_cnt))

    def shard_regroup_dev(self, d_cnt, d_grp, d_pos, n_src, n_reads, d_seg, d_grp_out, d_pos_out):
        world = len(d_cnt)
        arr = lambda xs: (C.c_void_p * world)(*[int(x) for x in xs])
        ns = (C.c_uint64 * world)(*[int(x) for x in n_src])
        L = lib()
        _check(L.rvn_shard_regroup_dev(self._h, world, arr(d_cnt), arr(d_grp), arr(d_pos), ns, int(n_reads), d_seg,
                                       d_grp_out, d_pos_out))

    def shard_split_overlaps_dev(self, d_ovl, n, bounds, world, self_rank, d_out):
        b = np.ascontiguousarray(bounds, dtype=np.uint32)
        counts = (C.c_uint64 * (world + 1))()
        L = lib()
        _check(L.rvn_shard_split_overlaps_dev(self._h, d_ovl, int(n), _p(b), world, self_rank, d_out, counts))
        return [int(x) for x in counts]

    def shard_join_fetch_dev(self, d_grp, d_pos, d_seg):
        _check(lib().rvn_shard_join_fetch_dev(self._h, d_grp, d_pos, d_seg))

    def shard_chain_dev(self, own_reads: Reads, d_grp, d_pos, d_seg, n_matches) -> int:
        n = C.c_uint64(0)
        _check(lib().rvn_shard_chain_dev(self._h, own_reads._h, d_grp, d_pos, d_seg, int(n_matches), C.byref(n)))
        return int(n.value)

    def map_fetch_dev(self, d_overlaps, d_read_off):
        _check(lib().rvn_engine_map_fetch_dev(self._h, d_overlaps, d_read_off))

    def shard_piles_dev(self, lengths, d_overlaps, d_read_off, n, kmax=32) -> Pass1:
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        h = C.c_void_p()
        _check(lib().rvn_shard_piles_dev(self._h, _p(lengths), lengths.shape[0], d_overlaps, d_read_off, int(n), kmax,
                                         C.byref(h)))
        return Pass1(h, lengths.shape[0])

    def pile_add_layers(self, data: np.ndarray, pile_id: int, overlaps: np.ndarray):
        assert data.dtype == np.uint16 and overlaps.dtype == OVERLAP_DTYPE
        overlaps = np.ascontiguousarray(overlaps)
        _check(lib().rvn_pile_add_layers(self._h, _p(data), data.shape[0], pile_id, _p(overlaps),
                                         overlaps.shape[0]))

    # -- racon::Polisher::Polish, one round ------------------------------------------------------------
    def polish_round_range(self, targets: Reads, reads: Reads, window_first, window_last, quals=None, q=0.0, err=0.3,
                           w=500, trim=True, m=3, n=-5, g=-4):
        """One round restricted to global windows [window_first, window_last): returns (per-target partial consensus,
        per-target window counts in range, per-target polished counts, stats)."""
        nt = targets.n
        ooff = np.zeros(nt + 1, dtype=np.uint64)
        np.cumsum(2 * targets.rs.lengths.astype(np.uint64) + 1024, out=ooff[1:])
        out = np.zeros(int(ooff[-1]) + 1, dtype=np.uint8)
        out_len = np.zeros(nt, dtype=np.uint32)
        nw = np.zeros(nt, dtype=np.uint32)
        npol = np.zeros(nt, dtype=np.uint32)
        stats = np.zeros(16, dtype=np.uint64)
        qa = qo = None
        if quals is not None:
            qo = np.zeros(len(quals) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in quals], out=qo[1:])
            qa = np.concatenate([np.asarray(x, dtype=np.uint8) for x in quals])
        L = lib()
        _check(L.rvn_polish_round_range(self._h, targets._h, reads._h, _p(qa), _p(qo), float(q), float(err), w,
                                        int(trim), m, n, g, int(window_first), int(window_last), _p(out), _p(ooff),
                                        _p(out_len), None, _p(nw), _p(npol), _p(stats)))
        cons = [out[int(ooff[i]): int(ooff[i]) + int(out_len[i])].copy() for i in range(nt)]
        st = {"n_windows": int(stats[3]), "n_layers": int(stats[2])}
        for i, k2 in enumerate(("poa_ms", "map_ms", "host_ms", "total_ms")):
            st[k2] = float(stats[6 + i: 7 + i].view(np.float64)[0])
        st["align_ms"] = float(stats[11:12].view(np.float64)[0])
        return cons, nw, npol, st

    def polish_map_best(self, targets: Reads, reads: Reads, read_first=0, read_last=None, err=0.3):
        """First step of a round for the reads [read_first, read_last): (best overlaps [n, 8] uint32 rows of rvn_overlap,
        best target index per read uint32 with 0xFFFFFFFF = unused, number of overlaps found)."""
        read_last = reads.n if read_last is None else int(read_last)
        n = read_last - int(read_first)
        best = np.zeros((max(n, 1), 8), dtype=np.uint32)
        bt = np.zeros(max(n, 1), dtype=np.uint32)
        n_ovl = C.c_uint64(0)
        L = lib()
        _check(L.rvn_polish_map_best(self._h, targets._h, reads._h, int(read_first), read_last, float(err), _p(best),
                                     _p(bt), C.byref(n_ovl)))
        return best[:n], bt[:n], int(n_ovl.value)

    def polish_set_best(self, best, best_target):
        """Hands the complete best-overlap table to the next polish_round / polish_round_range call (which then skips
        its own mapping)."""
        best = np.ascontiguousarray(best, dtype=np.uint32).reshape(-1, 8)
        bt = np.ascontiguousarray(best_target, dtype=np.uint32)
        assert best.shape[0] == bt.shape[0]
        L = lib()
        _check(L.rvn_polish_set_best(self._h, _p(best), _p(bt), int(bt.shape[0])))

    # -- second mapping pass and identity filter (construct.cc:316-491, :162-217) ------------------------------------
    def find_overlaps_and_repetitive_regions(self, reads: Reads, pile_begin, pile_end, pile_invalid, freq=0.001,
                                             kmer_len=None, identity=0.0, batch_bases=1 << 30):
        """raven::FindOverlapsAndRepetetiveRegions on the device.  pile_begin / pile_end in bases (Pile::begin() /
        end()), pile_invalid 0/1.  Returns dict(overlaps, contained[n], kmers (list of per-read uint8 cell arrays, empty
        for invalid reads))."""
        n = reads.n
        b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
        en = np.ascontiguousarray(pile_end, dtype=np.uint32)
        inv = np.ascontiguousarray(pile_invalid, dtype=np.uint8)
        assert b.shape[0] == n and en.shape[0] == n and inv.shape[0] == n
        h = C.c_void_p()
        L = lib()
        _check(L.rvn_find_overlaps_and_repetitive_regions(self._h, reads._h, _p(b), _p(en), _p(inv), float(freq),
                                                          int(self.k if kmer_len is None else kmer_len), float(identity),
                                                          int(batch_bases), C.byref(h)))
        try:
            no, nk = int(L.rvn_pass2_num_overlaps(h)), int(L.rvn_pass2_kmer_cells(h))
            ovl = np.zeros(no, dtype=OVERLAP_DTYPE)
            contained = np.zeros(n, dtype=np.uint8)
            kmers = np.zeros(nk, dtype=np.uint8)
            koff = np.zeros(n + 1, dtype=np.uint64)
            _check(L.rvn_pass2_fetch(h, _p(ovl), _p(contained), _p(kmers), _p(koff)))
        finally:
            L.rvn_pass2_destroy(h)
        return dict(overlaps=ovl, contained=contained, kmers=[kmers[int(koff[i]):int(koff[i + 1])] for i in range(n)])

    def resolve_repeat_induced_overlaps(self, overlaps, coverage, coverage_offsets, kmers, kmers_offsets, pile_begin,
                                        pile_end, median, invalid):
        """raven::ResolveRepeatInducedOverlaps on the device (rvn_resolve_repeat_induced_overlaps): overlaps.back(), the
        piles' coverage / k-mer cells as flat arrays + offsets[n + 1], begin / end in bases, median, invalid 0/1.
        Returns dict(overlaps (survivors, in order), regions ((k, 2) uint32: cell << 1 | flag, cell), region_offsets[n + 1]
        (pairs), is_repetitive[n], iterations, components, removed)."""
        o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        cov = np.ascontiguousarray(coverage, dtype=np.uint16)
        coff = np.ascontiguousarray(coverage_offsets, dtype=np.uint64)
        km = np.ascontiguousarray(kmers, dtype=np.uint8)
        koff = np.ascontiguousarray(kmers_offsets, dtype=np.uint64)
        b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
        en = np.ascontiguousarray(pile_end, dtype=np.uint32)
        med = np.ascontiguousarray(median, dtype=np.uint16)
        inv = np.ascontiguousarray(invalid, dtype=np.uint8)
        n = b.shape[0]
        assert en.shape[0] == n and med.shape[0] == n and inv.shape[0] == n and coff.shape[0] == n + 1 == koff.shape[0]
        h = C.c_void_p()
        L = lib()
        _check(L.rvn_resolve_repeat_induced_overlaps(self._h, _p(o), o.shape[0], n, _p(cov), _p(coff), _p(km), _p(koff),
                                                     _p(b), _p(en), _p(med), _p(inv), C.byref(h)))
        try:
            ovl = np.zeros(int(L.rvn_repeats_num_overlaps(h)), dtype=OVERLAP_DTYPE)
            reg = np.zeros((int(L.rvn_repeats_num_regions(h)), 2), dtype=np.uint32)
            roff = np.zeros(n + 1, dtype=np.uint32)
            isrep = np.zeros(n, dtype=np.uint8)
            stats = np.zeros(2, dtype=np.uint64)  # rvn_repeats_stats: {u32 iterations, u32 components}, u64 removed
            _check(L.rvn_repeats_fetch(h, _p(ovl), _p(reg), _p(roff), _p(isrep), _p(stats)))
        finally:
            L.rvn_repeats_destroy(h)
        return dict(overlaps=ovl, regions=reg, region_offsets=roff, is_repetitive=isrep,
                    iterations=int(stats[0]) & 0xFFFFFFFF, components=int(stats[0]) >> 32, removed=int(stats[1]))

    def resolve_contained_and_chimeric(self, overlaps, offsets, coverage, coverage_offsets, regions, region_offsets, begin,
                                       end, median, invalid, reads=None, identity=0.0, phases=3):
        """The stage of Pass1.resolve on host arrays (rvn_resolve_contained_and_chimeric): lists + offsets[n + 1] as
        Pass1.overlaps() gives them, coverage + offsets as Pass1.piles(), regions ((k, 2) cells) + region_offsets[n + 1],
        begin / end in cells, median, invalid 0/1.  Returns the same dict, with the coverage."""
        o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        cov = np.ascontiguousarray(coverage, dtype=np.uint16)
        coff = np.ascontiguousarray(coverage_offsets, dtype=np.uint64)
        reg = np.ascontiguousarray(regions, dtype=np.uint32).reshape(-1)
        roff = np.ascontiguousarray(region_offsets, dtype=np.uint32)
        b = np.ascontiguousarray(begin, dtype=np.uint32)
        en = np.ascontiguousarray(end, dtype=np.uint32)
        med = np.ascontiguousarray(median, dtype=np.uint16)
        inv = np.ascontiguousarray(invalid, dtype=np.uint8)
        n = b.shape[0]
        assert en.shape[0] == n and med.shape[0] == n and inv.shape[0] == n
        assert off.shape[0] == n + 1 == coff.shape[0] == roff.shape[0]
        assert o.shape[0] == int(off[-1]) and cov.shape[0] == int(coff[-1]) and reg.shape[0] == 2 * int(roff[-1])
        h = C.c_void_p()
        L = lib()
        _check(L.rvn_resolve_contained_and_chimeric(self._h, reads._h if reads is not None else None, _p(o), _p(off), n,
                                                    _p(cov), _p(coff), _p(reg), _p(roff), _p(b), _p(en), _p(med), _p(inv),
                                                    float(identity), int(phases), C.byref(h)))
        return _fetch_resolved(h, n)

    def filter_overlaps_by_identity(self, reads: Reads, overlaps, offsets, pile_begin, pile_end, pile_invalid, identity):
        """Identity filter loop of ResolveContainedReads on per-pile lists: returns (overlaps, offsets) filtered."""
        o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE).copy()
        off = np.ascontiguousarray(offsets, dtype=np.uint32).copy()
        _check(lib().rvn_filter_overlaps_by_identity(self._h, reads._h, _p(o), _p(off),
                                                     _p(np.ascontiguousarray(pile_begin, dtype=np.uint32)),
                                                     _p(np.ascontiguousarray(pile_end, dtype=np.uint32)),
                                                     _p(np.ascontiguousarray(pile_invalid, dtype=np.uint8)), float(identity)))
        return o[:int(off[-1])], off

    def layout_force_directed(self, component_offsets, xy, adj_offsets, adj, n_iterations=100):
        """raven's force-directed layout of every component at once (rvn_layout_force_directed): xy float64[n, 2] start
        positions, adj the neighbours of each point as point indices (CSR, in the order their terms are added).
        Returns (float64[n, 2] positions after the last iteration, {"host_tree_iterations", "max_depth"})."""
        off = np.ascontiguousarray(component_offsets, dtype=np.uint32)
        pos = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        aoff = np.ascontiguousarray(adj_offsets, dtype=np.uint64)
        a = np.ascontiguousarray(adj, dtype=np.uint32)
        if off.shape[0] < 1 or pos.shape[0] != int(off[-1]) or aoff.shape[0] != pos.shape[0] + 1 or (
                aoff.shape[0] and a.shape[0] < int(aoff[-1])):
            raise ValueError("layout_force_directed: array sizes do not fit the offsets")
        out = np.zeros_like(pos)
        st = np.zeros(2, dtype=np.uint64)  # rvn_layout_stats: uint64, uint32, uint32
        _check(lib().rvn_layout_force_directed(self._h, off.shape[0] - 1, _p(off), _p(pos), _p(aoff), _p(a), int(n_iterations),
                                               _p(out), _p(st)))
        return out, {"host_tree_iterations": int(st[0]), "max_depth": int(st[1] & 0xFFFFFFFF)}

    def construct_assembly_graph(self, overlaps, pile_begin, pile_end, median, invalid):
        """raven::ConstructAssemblyGraph as an edge table on the device (rvn_construct_assembly_graph): overlaps.back(),
        begin / end in bases, median, invalid 0/1.  Returns a Graph."""
        o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
        b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
        en = np.ascontiguousarray(pile_end, dtype=np.uint32)
        med = np.ascontiguousarray(median, dtype=np.uint16)
        inv = np.ascontiguousarray(invalid, dtype=np.uint8)
        n = b.shape[0]
        assert en.shape[0] == n and med.shape[0] == n and inv.shape[0] == n
        h = C.c_void_p()
        _check(lib().rvn_construct_assembly_graph(self._h, _p(o), o.shape[0], n, _p(b), _p(en), _p(med), _p(inv), C.byref(h)))
        return Graph(self, h, n)

    def graph_from_edges(self, n_nodes, tail, head, length):
        """A Graph from flattened graph.edges (rvn_graph_from_edges): tail 0xFFFFFFFF = an empty slot."""
        t = np.ascontiguousarray(tail, dtype=np.uint32)
        hd = np.ascontiguousarray(head, dtype=np.uint32)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        assert hd.shape[0] == t.shape[0] == ln.shape[0]
        h = C.c_void_p()
        _check(lib().rvn_graph_from_edges(self._h, int(n_nodes), t.shape[0], _p(t), _p(hd), _p(ln), C.byref(h)))
        return Graph(self, h, None)

    def tiling_from_piles(self, reads: Reads, node_pile, pile_begin, pile_end):
        """Node sequences as read segments (rvn_tiling_from_piles): node u = pile node_pile[u]'s valid region, reverse
        complemented for odd u; node_pile as Graph.fetch() reports it, begin / end in bases.  Returns a Tiling."""
        npile = np.ascontiguousarray(node_pile, dtype=np.uint32)
        b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
        en = np.ascontiguousarray(pile_end, dtype=np.uint32)
        assert b.shape[0] == en.shape[0]
        h = C.c_void_p()
        _check(lib().rvn_tiling_from_piles(self._h, reads._h, npile.shape[0], _p(npile), b.shape[0], _p(b), _p(en), C.byref(h)))
        return Tiling(self, reads, h)

    def tiling_from_segments(self, reads: Reads, offsets, read, begin, length, strand):
        """A Tiling from caller-stated segment lists (rvn_tiling_from_segments): CSR offsets[n_nodes + 1] over (read index,
        first base, length, strand) arrays."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        r = np.ascontiguousarray(read, dtype=np.uint32)
        b = np.ascontiguousarray(begin, dtype=np.uint32)
        ln = np.ascontiguousarray(length, dtype=np.uint32)
        st = np.ascontiguousarray(strand, dtype=np.uint8)
        assert r.shape[0] == b.shape[0] == ln.shape[0] == st.shape[0] and off.shape[0] >= 1
        h = C.c_void_p()
        _check(lib().rvn_tiling_from_segments(self._h, reads._h, off.shape[0] - 1, _p(off), _p(r), _p(b), _p(ln), _p(st), C.byref(h)))
        return Tiling(self, reads, h)

    def release_scratch(self):
        _check(lib().rvn_engine_release_scratch(self._h))

    def poa_cells(self):
        """DP work of the banded POA kernel since the last reset_stats (rvn_poa_work)."""
        out = np.zeros(3, dtype=np.uint64)
        lib().rvn_poa_work(self._h, _p(out))
        return {"cells_full": int(out[0]), "cells_banded": int(out[1]), "calls": int(out[2])}

    def polish_layers(self):
        """Layer table of the last polishing round: uint32[n, 7] rows {window, read, first base in the oriented read,
        bases, begin, end, rc} in racon's order (rvn_polish_fetch_layers)."""
        n = C.c_uint64(0)
        _check(lib().rvn_polish_fetch_layers(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 7), dtype=np.uint32)
        _check(lib().rvn_polish_fetch_layers(self._h, _p(out), n.value, C.byref(n)))
        return out

    def polish_round(self, targets: Reads, reads: Reads, quals=None, q=0.0, err=0.3, w=500, trim=True, m=3, n=-5, g=-4):
        """quals: list of uint8 Phred+33 arrays (one per read) or None.  Returns (list of polished code arrays,
        ratio array, stats dict).  The engine must have k=15, w=5 (racon's mapping parameters)."""
        nt = targets.n
        ooff = np.zeros(nt + 1, dtype=np.uint64)
        np.cumsum(2 * targets.rs.lengths.astype(np.uint64) + 1024, out=ooff[1:])
        out = np.empty(int(ooff[-1]) + 1, dtype=np.uint8)  # (the library writes every byte it reports)
        out_len = np.zeros(nt, dtype=np.uint32)
        ratio = np.zeros(nt, dtype=np.float64)
        stats = np.zeros(16, dtype=np.uint64)
        qa = qo = None
        if quals is not None:
            qo = np.zeros(len(quals) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in quals], out=qo[1:])
            qa = np.concatenate([np.asarray(x, dtype=np.uint8) for x in quals])
        _check(lib().rvn_polish_round(self._h, targets._h, reads._h, _p(qa), _p(qo), float(q), float(err), w, int(trim),
                                      m, n, g, _p(out), _p(ooff), _p(out_len), _p(ratio), _p(stats)))
        # (views of this call's own buffer — never written again —, not copies: 100 MB at C4)
        cons = [out[int(ooff[i]): int(ooff[i]) + int(out_len[i])] for i in range(nt)]
        keys = ("n_overlaps", "n_reads_used", "n_layers", "n_windows", "n_polished_windows", "n_failed_windows")
        st = {k2: int(v) for k2, v in zip(keys, stats[:6])}
        for i, k2 in enumerate(("poa_ms", "map_ms", "host_ms", "total_ms")):
            st[k2] = float(stats[6 + i: 7 + i].view(np.float64)[0])
        st["n_dropped_layers"] = int(stats[10])
        st["align_ms"] = float(stats[11:12].view(np.float64)[0])
        st["n_aligned"], st["n_align_retries"] = int(stats[12]), int(stats[13])
        st["align_band_cells"], st["align_store_bytes"] = int(stats[14]), int(stats[15])
        return cons, ratio, st

    # -- raven::Pile::AddKmers, batched ---------------------------------------------------------------
    def pile_add_kmers_batch(self, reads: Reads, first, positions_per_read):
        """positions_per_read: list of uint32 arrays (the `filtered` output of Map per read, starting at read
        `first`).  Returns a list of uint8 arrays, Pile::kmers_ of each read ((len >> 4) + 1 entries)."""
        n = len(positions_per_read)
        poff = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in positions_per_read], out=poff[1:])
        pos = (np.concatenate([np.asarray(x, dtype=np.uint32) for x in positions_per_read])
               if n and poff[-1] else np.zeros(1, np.uint32))
        sizes = [(int(reads.rs.lengths[first + i]) >> 4) + 1 for i in range(n)]
        koff = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(sizes, out=koff[1:])
        out = np.zeros(int(koff[-1]) + 1, dtype=np.uint8)
        _check(lib().rvn_pile_add_kmers_batch(self._h, reads._h, first, n, _p(pos), _p(poff), _p(out), _p(koff)))
        return [out[int(koff[i]): int(koff[i + 1])].copy() for i in range(n)]

    # -- edlibAlign(default config).editDistance, batched -----------------------------------------
    def edit_distance_batch(self, reads: Reads, pairs: np.ndarray):
        """pairs: array of ED_PAIR_DTYPE; returns (uint32 distances, device ms, DP cells)."""
        pairs = np.ascontiguousarray(pairs, dtype=ED_PAIR_DTYPE)
        out = np.zeros(pairs.shape[0], dtype=np.uint32)
        ms, cells = C.c_double(0), C.c_uint64(0)
        _check(lib().rvn_edit_distance_batch(self._h, reads._h, _p(pairs), pairs.shape[0], _p(out), C.byref(ms),
                                             C.byref(cells)))
        return out, ms.value, cells.value

    # -- RemoveBubbles' similarity test on pairs of path sequences -----------------------------------
    def path_similarity(self, paths: Reads, pairs, min_ratio=0.8):
        """rvn_path_similarity_batch.  pairs: n x 2 read indices of `paths` (Tiling.paths_as_reads).  Returns (uint8 similar,
        uint32 distance: exact where it passes the rule, PATH_DISTANCE_ABOVE above it, PATH_REJECTED_BY_LENGTH where the
        length rule rejected the pair)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        similar = np.zeros(pairs.shape[0], np.uint8)
        distance = np.zeros(pairs.shape[0], np.uint32)
        _check(lib().rvn_path_similarity_batch(self._h, paths._h, _p(pairs), pairs.shape[0], float(min_ratio), _p(similar),
                                               _p(distance)))
        return similar, distance

    # -- edlibAlign(NW, TASK_PATH), batched ---------------------------------------------------------
    def align_paths(self, queries: Reads, targets: Reads, pairs: np.ndarray, ops=False):
        """rvn_align_path_batch.  pairs: array of ALIGN_PAIR_DTYPE.  Returns (uint32 distances — 0xFFFFFFFF: not aligned —,
        uint64 run_offsets[n + 1], uint32 runs: count << 2 | op in alignment order, number of pairs not aligned); with
        ops=True instead of the runs (uint64 op_offsets[n + 1], uint8 ops: edlib's alignment bytes, expanded on the device)."""
        pairs = np.ascontiguousarray(pairs, dtype=ALIGN_PAIR_DTYPE)
        h = C.c_void_p()
        L = lib()
        _check(L.rvn_align_path_batch(self._h, queries._h, targets._h, _p(pairs), pairs.shape[0], C.byref(h)))
        try:
            n, n_runs, n_ops, n_bad = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
            _check(L.rvn_paths_info(h, C.byref(n), C.byref(n_runs), C.byref(n_ops), C.byref(n_bad)))
            dist = np.zeros(n.value, dtype=np.uint32)
            if ops:
                off = np.zeros(n.value + 1, dtype=np.uint64)
                out = np.zeros(n_ops.value, dtype=np.uint8)
                _check(L.rvn_paths_fetch(h, _p(dist), None, None))
                _check(L.rvn_paths_fetch_ops(h, _p(off), _p(out) if n_ops.value else None))
            else:
                off = np.zeros(n.value + 1, dtype=np.uint64)
                out = np.zeros(n_runs.value, dtype=np.uint32)
                _check(L.rvn_paths_fetch(h, _p(dist), _p(off), _p(out) if n_runs.value else None))
            return dist, off, out, int(n_bad.value)
        finally:
            L.rvn_paths_destroy(h)

    # -- racon Window::GenerateConsensus, batched --------------------------------------------------
    def poa_consensus_batch(self, windows, m=3, n=-5, g=-4, trim=True):
        """windows: list of dicts {layers: [uint8 code arrays, layer 0 = backbone], begins, ends, quals (list of
        uint8 Phred+33 arrays or None entries) or None}.  Returns (list of consensus code arrays, status array, ms)."""
        a = _pack_poa_windows(windows)
        ms = C.c_double(0)
        _check(lib().rvn_poa_consensus_batch(
            self._h, _p(a["codes"]), _p(a["quals"]), _p(a["loff"]), _p(a["begins"]), _p(a["ends"]), _p(a["hasq"]),
            _p(a["woff"]), a["nw"], m, n, g, int(trim), _p(a["out"]), _p(a["ooff"]), _p(a["out_len"]), _p(a["status"]),
            C.byref(ms)))
        return _unpack_poa_consensus(a), a["status"], ms.value

    def poa_phase_cycles(self):
        c = np.zeros(6, dtype=np.uint64)
        lib().rvn_poa_phase_cycles(self._h, _p(c))
        return dict(zip(("subgraph", "dp", "traceback", "add_alignment", "order", "consensus"), (int(x) for x in c)))

    def polish_set_chunk_windows(self, windows):
        """Windows per POA chunk of a polishing round (0 = one batch); returns the previous value."""
        return int(lib().rvn_polish_set_chunk_windows(self._h, int(windows)))

    def set_option(self, name, value):
        """rvn_engine_set_option: a tuning option (include/raven_hip.h lists them; -1 = built-in default, and so is 0 for
        every option but poa_rows_min_windows, whose 0 means "every batch" and selects another first kernel: consensus is
        reproducible per value of that option, not across values); returns the previous value.  Unknown names raise."""
        prev = C.c_int64(0)
        L = lib()
        _check(L.rvn_engine_set_option(self._h, name.encode(), int(value), C.byref(prev)))
        return int(prev.value)

    def poa_set_mode(self, mode):
        """0 band 32 (rows on lanes, poa4.hip) -> 64 -> 128 -> 256 -> full matrix (default), 1 full matrix only,
        2 / 3 / 4 band 64 / 128 / 256 only, 9 poa4.hip only."""
        return int(lib().rvn_poa_set_mode(self._h, int(mode)))

    def poa_fallback_windows(self):
        return int(lib().rvn_poa_fallback_windows(self._h))

    def poa_wide_windows(self):
        return int(lib().rvn_poa_wide_windows(self._h))

    def poa_narrow_windows(self):
        return int(lib().rvn_poa_narrow_windows(self._h))

    # -- introspection ---------------------------------------------------------------------
    def sketch(self, reads: Reads, first=0, last=None, minhash=False):
        last = reads.n if last is None else last
        cnt = C.c_uint64(0)
        _check(lib().rvn_engine_sketch(self._h, reads._h, first, last, int(minhash), C.byref(cnt)))
        v = np.zeros(cnt.value, dtype=np.uint64)
        o = np.zeros(cnt.value, dtype=np.uint64)
        off = np.zeros(last - first + 1, dtype=np.uint32)
        _check(lib().rvn_engine_sketch_fetch(self._h, _p(v), _p(o), _p(off)))
        return v, o, off

    def index_content(self):
        m, u = C.c_uint64(0), C.c_uint64(0)
        _check(lib().rvn_engine_index_size(self._h, C.byref(m), C.byref(u)))
        v = np.zeros(m.value, dtype=np.uint64)
        o = np.zeros(m.value, dtype=np.uint64)
        _check(lib().rvn_engine_index_fetch(self._h, _p(v), _p(o)))
        return v, o, int(u.value)

    def counters(self):
        c = np.zeros(8, dtype=np.uint64)
        _check(lib().rvn_engine_counters(self._h, _p(c)))
        return dict(zip(("index_bases", "index_minimizers", "index_keys", "query_bases", "query_minimizers",
                         "matches", "overlaps", "intervals"), (int(x) for x in c)))

    def stage_ms(self):
        L = lib()
        n = L.rvn_engine_num_stages()
        ms = np.zeros(n, dtype=np.float64)
        la = np.zeros(n, dtype=np.uint64)
        _check(L.rvn_engine_stage_ms(self._h, _p(ms), _p(la), n))
        return {L.rvn_engine_stage_name(i).decode(): (float(ms[i]), int(la[i])) for i in range(n)}

    def set_kernel_timing(self, enabled: bool):
        lib().rvn_engine_set_kernel_timing(self._h, int(enabled))

    def kernel_ms(self):
        """{site: (total device ms, launches)} since the last reset_stats()."""
        L = lib()
        n = L.rvn_engine_num_kernel_sites()
        ms = np.zeros(n, dtype=np.float64)
        la = np.zeros(n, dtype=np.uint64)
        _check(L.rvn_engine_kernel_ms(self._h, _p(ms), _p(la), n))
        return {L.rvn_engine_kernel_site_name(i).decode(): (float(ms[i]), int(la[i])) for i in range(n)}

    def reset_stats(self):
        lib().rvn_engine_reset_stats(self._h)

    def set_timing(self, enabled: bool):
        lib().rvn_engine_set_timing(self._h, int(enabled))


class Graph:
    """An assembly graph's edge table in HBM (rvn_graph): Engine.construct_assembly_graph / Engine.graph_from_edges."""

    def __init__(self, engine, handle, n_piles):
        self._e, self._h, self.n_piles = engine, handle, n_piles
        nn, ne, nl = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(lib().rvn_graph_info(self._h, C.byref(nn), C.byref(ne), C.byref(nl)))
        self.n_nodes, self.n_edges, self.n_live_edges = nn.value, ne.value, nl.value

    def fetch(self):
        """dict(tail, head, length) of every edge slot; for a constructed graph also sequence_to_node, node_pile,
        node_coverage, edge_overlap (per edge pair) and finalized (the overlaps after OverlapFinalize, per edge pair)."""
        E = self.n_edges
        r = dict(tail=np.zeros(E, np.uint32), head=np.zeros(E, np.uint32), length=np.zeros(E, np.uint32))
        if self.n_piles is not None:
            r.update(sequence_to_node=np.zeros(self.n_piles, np.int32), node_pile=np.zeros(self.n_nodes, np.uint32),
                     node_coverage=np.zeros(self.n_nodes, np.uint16), edge_overlap=np.zeros(E // 2, np.uint64),
                     finalized=np.zeros(E // 2, OVERLAP_DTYPE))
        _check(lib().rvn_graph_fetch(self._h, _p(r.get("sequence_to_node")), _p(r.get("node_pile")), _p(r.get("node_coverage")),
                                     _p(r["tail"]), _p(r["head"]), _p(r["length"]), _p(r.get("edge_overlap")),
                                     _p(r.get("finalized"))))
        return r

    def mark_transitive(self):
        """RemoveTransitiveEdges' marking (rvn_graph_mark_transitive): (marked ids in the reference's insertion order,
        (k, 2) uint32 transitive pairs of the odd ids in that order)."""
        n = C.c_uint64()
        _check(lib().rvn_graph_mark_transitive(self._e._h, self._h, C.byref(n)))
        order = np.zeros(n.value, np.uint32)
        pairs = np.zeros((n.value, 2), np.uint32)
        npairs = C.c_uint64()
        _check(lib().rvn_graph_fetch_transitive(self._h, _p(order), _p(pairs), C.byref(npairs)))
        return order, pairs[:npairs.value].copy()

    def mark_long_edges(self, weight):
        """RemoveLongEdges' marking loop (rvn_graph_mark_long_edges): (flags uint8[n_edges], number of marked ids)."""
        w = np.ascontiguousarray(weight, dtype=np.float64)
        assert w.shape[0] == self.n_edges
        flags = np.zeros(self.n_edges, np.uint8)
        n = C.c_uint64()
        _check(lib().rvn_graph_mark_long_edges(self._e._h, self._h, _p(w), _p(flags), C.byref(n)))
        return flags, n.value

    def edge_similarity(self, tiling):
        """printEdgeSimilarity of the CSV emitters for every edge slot (rvn_graph_edge_similarity): dict(lhs_length,
        rhs_length, distance uint32 — EDGE_SLOT_EMPTY for an empty slot —, score float64 = 1 - distance / lhs_length, NaN
        where lhs_length is 0 or the slot is empty)."""
        E = self.n_edges
        r = dict(lhs_length=np.zeros(E, np.uint32), rhs_length=np.zeros(E, np.uint32), distance=np.zeros(E, np.uint32),
                 score=np.zeros(E, np.float64))
        _check(lib().rvn_graph_edge_similarity(self._e._h, self._h, tiling._h, tiling.reads._h, _p(r["lhs_length"]),
                                               _p(r["rhs_length"]), _p(r["distance"]), _p(r["score"])))
        return r

    def create_unitigs(self, tiling, count, coverage, epsilon=0, min_unitig_size=9999):
        """raven::CreateUnitigs on the edge table (rvn_graph_create_unitigs): count / coverage per node.  The tiling grows
        by the new nodes; returns a Unitigs."""
        c = np.ascontiguousarray(count, dtype=np.uint32)
        cov = np.ascontiguousarray(coverage, dtype=np.uint16)
        assert c.shape[0] == self.n_nodes and cov.shape[0] == self.n_nodes
        h = C.c_void_p()
        _check(lib().rvn_graph_create_unitigs(self._e._h, self._h, tiling._h, _p(c), _p(cov), int(epsilon), int(min_unitig_size),
                                              C.byref(h)))
        return Unitigs(self._e, tiling, h)

    def close(self):
        if self._h is not None:
            lib().rvn_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tiling:
    """Node sequences as lists of read segments in HBM (rvn_tiling): Engine.tiling_from_piles / tiling_from_segments.
    Graph.create_unitigs appends the new nodes' lists."""

    def __init__(self, engine, reads, handle):
        self._e, self.reads, self._h = engine, reads, handle

    @property
    def n_nodes(self):
        n, m = C.c_uint32(), C.c_uint64()
        _check(lib().rvn_tiling_info(self._h, C.byref(n), C.byref(m)))
        return n.value

    def fetch(self):
        """dict(offsets uint64[n_nodes + 1], read, begin, length uint32[segments], strand uint8[segments], node_length)."""
        n, m = C.c_uint32(), C.c_uint64()
        _check(lib().rvn_tiling_info(self._h, C.byref(n), C.byref(m)))
        r = dict(offsets=np.zeros(n.value + 1, np.uint64), read=np.zeros(m.value, np.uint32), begin=np.zeros(m.value, np.uint32),
                 length=np.zeros(m.value, np.uint32), strand=np.zeros(m.value, np.uint8), node_length=np.zeros(n.value, np.uint32))
        _check(lib().rvn_tiling_fetch(self._h, _p(r["offsets"]), _p(r["read"]), _p(r["begin"]), _p(r["length"]), _p(r["strand"]),
                                      _p(r["node_length"])))
        return r

    def as_reads(self, nodes) -> Reads:
        """The sequences of the listed nodes as a read set (rvn_tiling_as_reads)."""
        ids = np.ascontiguousarray(nodes, dtype=np.uint32)
        h = C.c_void_p()
        _check(lib().rvn_tiling_as_reads(self._e._h, self._h, self.reads._h, _p(ids), ids.shape[0], C.byref(h)))
        return _device_reads(self._e, h)

    def slices_as_reads(self, nodes, begins, lengths) -> Reads:
        """InflateData(begins[i], lengths[i]) of nodes[i] as read i of a read set (rvn_tiling_slices_as_reads)."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        bg = np.ascontiguousarray(begins, dtype=np.uint32)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        if not (nd.shape[0] == bg.shape[0] == ln.shape[0]):
            raise ValueError("slices_as_reads: the three arrays differ in size")
        h = C.c_void_p()
        _check(lib().rvn_tiling_slices_as_reads(self._e._h, self._h, self.reads._h, nd.shape[0], _p(nd), _p(bg), _p(ln), C.byref(h)))
        return _device_reads(self._e, h)

    def paths_as_reads(self, offsets, nodes, labels) -> Reads:
        """The sequences of node paths as a read set (rvn_tiling_paths_as_reads): path p = nodes[offsets[p] .. offsets[p + 1]),
        every member but the last cut to its first min(label, length) bases."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        lb = np.ascontiguousarray(labels, dtype=np.uint32)
        if off.shape[0] < 1 or nd.shape[0] != lb.shape[0] or (off.shape[0] > 1 and int(off.max()) > nd.shape[0]):
            raise ValueError("paths_as_reads: array sizes do not fit the offsets")
        h = C.c_void_p()
        _check(lib().rvn_tiling_paths_as_reads(self._e._h, self._h, self.reads._h, off.shape[0] - 1, _p(off), _p(nd), _p(lb), C.byref(h)))
        return _device_reads(self._e, h)

    def close(self):
        if self._h is not None:
            lib().rvn_tiling_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _device_reads(engine, handle) -> Reads:
    """A Reads over a read set the library made: its lengths come from the handle."""
    n = C.c_uint32()
    _check(lib().rvn_reads_info(handle, C.byref(n), None, None, None, None))
    lens = np.zeros(n.value, np.uint32)
    _check(lib().rvn_reads_fetch(handle, None, None, _p(lens), None, None))
    return Reads(engine, CodeSet(lens), handle=handle)


UNITIGS_SELECTED, UNITIGS_ALL = 0, 1
PATH_DISTANCE_ABOVE, PATH_REJECTED_BY_LENGTH = 0xFFFFFFFE, 0xFFFFFFFF  # Engine.path_similarity's distance codes
EDGE_SLOT_EMPTY = 0xFFFFFFFF  # Graph.edge_similarity's distance of an empty edge slot


class Unitigs:
    """What raven::CreateUnitigs collects before its RemoveEdges, as flat tables (rvn_unitigs): Graph.create_unitigs."""

    def __init__(self, engine, tiling, handle):
        self._e, self.tiling, self._h = engine, tiling, handle
        fn, nn, nm, fe, ne = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().rvn_unitigs_info(self._h, C.byref(fn), C.byref(nn), C.byref(nm), C.byref(fe), C.byref(ne)))
        self.first_node, self.n_new_nodes, self.n_members = fn.value, nn.value, nm.value
        self.first_edge, self.n_new_edges = fe.value, ne.value

    def fetch(self):
        """dict(begin, end, is_circular, count, length, coverage, is_unitig per new node; member_offsets, members; marked
        per edge slot of the graph; edge_tail, edge_head, edge_length per new edge)."""
        U, E = self.n_new_nodes, self.n_new_edges
        r = dict(begin=np.zeros(U, np.uint32), end=np.zeros(U, np.uint32), is_circular=np.zeros(U, np.uint8),
                 count=np.zeros(U, np.uint32), length=np.zeros(U, np.uint32), coverage=np.zeros(U, np.uint16),
                 is_unitig=np.zeros(U, np.uint8), member_offsets=np.zeros(U + 1, np.uint64),
                 members=np.zeros(self.n_members, np.uint32), marked=np.zeros(self.first_edge, np.uint8),
                 edge_tail=np.zeros(E, np.uint32), edge_head=np.zeros(E, np.uint32), edge_length=np.zeros(E, np.uint32))
        _check(lib().rvn_unitigs_fetch(self._h, *[_p(r[k]) for k in (
            "begin", "end", "is_circular", "count", "length", "coverage", "is_unitig", "member_offsets", "members", "marked",
            "edge_tail", "edge_head", "edge_length")]))
        return r

    def as_reads(self, selection=UNITIGS_SELECTED) -> Reads:
        """The new nodes' sequences as a read set (rvn_unitigs_as_reads): GetUnitigs' choice, or UNITIGS_ALL."""
        h = C.c_void_p()
        _check(lib().rvn_unitigs_as_reads(self._e._h, self._h, self.tiling._h, self.tiling.reads._h, int(selection), C.byref(h)))
        return _device_reads(self._e, h)

    def close(self):
        if self._h is not None:
            lib().rvn_unitigs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group:
    """Several engines behind one handle (rvn_group_*): one per listed device, a device may repeat (virtual ranks).
    The calls take host read sets (anything with packed / word_offsets / lengths, read i = id i) and return what the
    single-engine calls of Engine return on the same input."""

    def __init__(self, devices, k=15, w=5, bandwidth=500, chain=4, matches=100, gap=10000):
        self.k, self.w = min(max(k, 1), 31), w
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        _check(lib().rvn_group_create(C.byref(h), k, w, bandwidth, chain, matches, gap, _p(dev), int(dev.shape[0])))
        self._h = h

    @property
    def size(self):
        return int(lib().rvn_group_size(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().rvn_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_scratch(self):
        """rvn_engine_release_scratch on every rank's engine."""
        for r in range(self.size):
            _check(lib().rvn_engine_release_scratch(lib().rvn_group_engine(self._h, r)))

    @staticmethod
    def _reads(rs):
        return (np.ascontiguousarray(rs.packed, dtype=np.uint64), np.ascontiguousarray(rs.word_offsets, dtype=np.uint64),
                np.ascontiguousarray(rs.lengths, dtype=np.uint32))

    def find_overlaps_and_repetitive_regions(self, rs, pile_begin, pile_end, pile_invalid, freq=0.001, kmer_len=None,
                                             identity=0.0, batch_bases=1 << 30):
        """rvn_group_find_overlaps_and_repetitive_regions: the same dict as Engine.find_overlaps_and_repetitive_regions."""
        n = int(rs.n)
        pk, wo, ln = self._reads(rs)
        b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
        en = np.ascontiguousarray(pile_end, dtype=np.uint32)
        inv = np.ascontiguousarray(pile_invalid, dtype=np.uint8)
        assert b.shape[0] == n and en.shape[0] == n and inv.shape[0] == n
        h = C.c_void_p()
        L = lib()
        _check(L.rvn_group_find_overlaps_and_repetitive_regions(
            self._h, _p(pk), _p(wo), _p(ln), n, _p(b), _p(en), _p(inv), float(freq),
            int(self.k if kmer_len is None else kmer_len), float(identity), int(batch_bases), C.byref(h)))
        try:
            no, nk = int(L.rvn_pass2_num_overlaps(h)), int(L.rvn_pass2_kmer_cells(h))
            ovl = np.zeros(no, dtype=OVERLAP_DTYPE)
            contained = np.zeros(n, dtype=np.uint8)
            kmers = np.zeros(nk, dtype=np.uint8)
            koff = np.zeros(n + 1, dtype=np.uint64)
            _check(L.rvn_pass2_fetch(h, _p(ovl), _p(contained), _p(kmers), _p(koff)))
        finally:
            L.rvn_pass2_destroy(h)
        return dict(overlaps=ovl, contained=contained, kmers=[kmers[int(koff[i]):int(koff[i + 1])] for i in range(n)])

    def filter_overlaps_by_identity(self, rs, overlaps, offsets, pile_begin, pile_end, pile_invalid, identity):
        """rvn_group_filter_overlaps_by_identity: (overlaps, offsets) as Engine.filter_overlaps_by_identity returns them."""
        pk, wo, ln = self._reads(rs)
        o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE).copy()
        off = np.ascontiguousarray(offsets, dtype=np.uint32).copy()
        _check(lib().rvn_group_filter_overlaps_by_identity(
            self._h, _p(pk), _p(wo), _p(ln), int(rs.n), _p(o), _p(off), _p(np.ascontiguousarray(pile_begin, dtype=np.uint32)),
            _p(np.ascontiguousarray(pile_end, dtype=np.uint32)), _p(np.ascontiguousarray(pile_invalid, dtype=np.uint8)),
            float(identity)))
        return o[:int(off[-1])], off


def test_find_chimeric_regions(data):
    """slopes.h on the host: Pile::FindChimericRegions of one coverage array -> (k, 2) uint32 (begin, end) cells."""
    d = np.ascontiguousarray(data, dtype=np.uint16)
    out = np.zeros(max(2, d.shape[0]), dtype=np.uint32)
    n = test_lib().rvn_test_find_chimeric_regions(_p(d), d.shape[0], _p(out), out.shape[0] // 2)
    if n < 0:
        raise ValueError("rvn_test_find_chimeric_regions: %d" % n)
    return out[:2 * n].reshape(-1, 2).copy()


def test_piles_annotate(data, offsets, coverage=4, per_thread=False, invalid=None, skip_trim=False):
    """TrimAndAnnotatePiles on the DEVICE for a crafted coverage CSR (rvn_test_piles_annotate: the functions behind
    Pass1.trim_and_annotate / find_chimeric_regions in an engine of its own).  per_thread: the one-thread-per-pile
    chimeric kernel instead of the wave kernel; invalid: the piles FindChimericRegions skips (None: the trim's flags);
    skip_trim: FindChimericRegions on the data as given.  Returns dict(data (after the trim), begin, end, median, invalid
    (all None when the trim was skipped), region_offsets[n + 1], regions: one (k, 2) uint32 array per pile)."""
    d = np.ascontiguousarray(data, dtype=np.uint16)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = off.shape[0] - 1
    assert n >= 0 and int(off[-1]) - int(off[0]) <= d.shape[0] - int(off[0])
    inv_in = None if invalid is None else np.ascontiguousarray(invalid, dtype=np.uint8)
    assert inv_in is None or inv_in.shape[0] == n
    after = np.zeros(int(off[-1]) - int(off[0]), dtype=np.uint16)
    b, e = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    m, inv = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint8)
    roff = np.zeros(n + 1, dtype=np.uint32)
    ptr = C.c_void_p()
    T = test_lib()
    rc = T.rvn_test_piles_annotate(_p(d), _p(off), n, int(coverage), int(per_thread), _p(inv_in), int(skip_trim), _p(after),
                                   _p(b), _p(e), _p(m), _p(inv), _p(roff), C.byref(ptr))
    if rc != RVN_OK:
        msg = T.rvn_last_error().decode(errors="replace")
        if rc == RVN_EINVAL:
            raise ValueError(msg)
        raise RavenHipError("rc=%d: %s" % (rc, msg))
    total = int(roff[-1])
    try:
        flat = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(max(2 * total, 1),))[:2 * total].copy()
    finally:
        T.rvn_free(ptr)
    flat = flat.reshape(-1, 2)
    regions = [flat[int(roff[i]):int(roff[i + 1])] for i in range(n)]
    if skip_trim:
        return dict(data=after, begin=None, end=None, median=None, invalid=None, region_offsets=roff, regions=regions)
    return dict(data=after, begin=b, end=e, median=m, invalid=inv.astype(bool), region_offsets=roff, regions=regions)


def _test_check(rc):
    if rc != RVN_OK:
        msg = test_lib().rvn_last_error().decode(errors="replace")
        if rc == RVN_EINVAL:
            raise ValueError(msg)
        raise RavenHipError("rc=%d: %s" % (rc, msg))


SORT_VARIANTS = {"u32_u64": 0, "u64_u64": 1, "u32_u32": 2}
SCAN_VARIANTS = {"u32_u64": 0, "u32_u32": 1, "u8_u32": 2}


def test_radix_sort_pairs(variant, keys, values, key_bits, skip_constant_digits=True):
    """The device-wide radix sort (radix_sort.hip) on host pairs (rvn_test_radix_sort_pairs): variant = a key of
    SORT_VARIANTS.  Returns (sorted keys, values carried along) as uint64."""
    k = np.array(keys, dtype=np.uint64)
    v = np.array(values, dtype=np.uint64)
    assert k.shape == v.shape and k.ndim == 1
    _test_check(test_lib().rvn_test_radix_sort_pairs(SORT_VARIANTS[variant], _p(k), _p(v), k.shape[0], int(key_bits),
                                                     int(skip_constant_digits)))
    return k, v


def test_exclusive_scan(variant, values, in_offset=0, out_offset=0):
    """The device-wide exclusive prefix sum (scan.hip) of host values (rvn_test_exclusive_scan): variant = a key of
    SCAN_VARIANTS; in_offset / out_offset = elements by which the device arrays are shifted off their 16-byte alignment.
    Returns uint64[n + 1] (the last entry = the total)."""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    out = np.zeros(a.shape[0] + 1, dtype=np.uint64)
    _test_check(test_lib().rvn_test_exclusive_scan(SCAN_VARIANTS[variant], _p(a), a.shape[0], int(in_offset), int(out_offset),
                                                   _p(out)))
    return out


def test_compact_overlap_list(overlaps, keep1, keep2=None):
    """compact_overlap_list (pass2.hip) on host overlaps (rvn_test_compact_overlap_list): keep1[n], then keep2 on the
    survivors when given.  Returns (survivors, the scan of the last application: uint32[its flags + 1])."""
    o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
    k1 = np.ascontiguousarray(keep1, dtype=np.uint8)
    assert k1.shape == o.shape and o.ndim == 1
    m = o.shape[0]
    k2 = None
    if keep2 is not None:
        k2 = np.ascontiguousarray(keep2, dtype=np.uint8)
        m = int(k1.sum())
        assert k2.shape == (m,)
    out = np.zeros(o.shape[0], dtype=OVERLAP_DTYPE)
    slot = np.zeros(o.shape[0] + 1, dtype=np.uint32)
    n_out = C.c_uint64(0)
    _test_check(test_lib().rvn_test_compact_overlap_list(_p(o), o.shape[0], _p(k1), _p(k2), _p(out),
                                                         C.byref(n_out), _p(slot)))
    return out[:n_out.value], slot[:m + 1]


def test_engine_scratch_bytes(engine) -> int:
    """Bytes of device scratch the engine holds, i.e. what release_scratch() would hand back
    (rvn_test_engine_scratch_bytes)."""
    n = C.c_uint64(0)
    _test_check(test_lib().rvn_test_engine_scratch_bytes(engine._h, C.byref(n)))
    return int(n.value)


def test_best_overlap(overlaps, read_off, first, err_thr, id_to_target, best, best_target):
    """best_overlap_kernel (polish.hip) on a host overlap list (rvn_test_best_overlap): read i of the batch has the
    overlaps [read_off[i], read_off[i + 1]) and writes row first + i of best / best_target, which the caller has filled.
    Returns (best, best_target) after the one launch; the arguments are left as they are."""
    o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE)
    off = np.ascontiguousarray(read_off, dtype=np.uint32)
    idm = np.ascontiguousarray(id_to_target, dtype=np.uint32)
    b = np.ascontiguousarray(best, dtype=OVERLAP_DTYPE).copy()
    bt = np.ascontiguousarray(best_target, dtype=np.uint32).copy()
    assert off.ndim == 1 and off.shape[0] >= 1 and b.shape == bt.shape and b.ndim == 1
    _test_check(test_lib().rvn_test_best_overlap(_p(o), o.shape[0], _p(off), int(first), off.shape[0] - 1, float(err_thr),
                                                 _p(idm), idm.shape[0], _p(b), _p(bt), bt.shape[0]))
    return b, bt


class _Pass2Batch(C.Structure):  # rvn_test_pass2_batch (include/raven_hip_test.h)
    _fields_ = [("q_first", C.c_uint32), ("q_last", C.c_uint32), ("q_origins", C.c_void_p), ("q_read_off", C.c_void_p),
                ("filtered", C.c_void_p), ("n_query", C.c_uint64), ("overlaps", C.c_void_p), ("n_overlaps", C.c_uint64)]


class HookEngine:
    """TEST INFRASTRUCTURE: an engine made by libraven_hip_test.so (a handle belongs to the library that made it), with
    what rvn_test_match_probe needs around it: an index from a crafted stream, the occurrence, the probe itself."""

    def __init__(self, k, direct_index=False):
        T = test_lib()
        h = C.c_void_p()
        _test_check(T.rvn_engine_create(C.byref(h), k, 5, 500, 4, 100, 10000, 0))
        self._h, self.k = h, k
        if direct_index:  # every index with 2k <= 30 bits gets the direct-address table
            _test_check(T.rvn_engine_set_option(h, b"index_direct_min_keys", 1, None))

    def close(self):
        if getattr(self, "_h", None):
            test_lib().rvn_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def index_build(self, values, origins):
        values = np.ascontiguousarray(values, dtype=np.uint64)
        origins = np.ascontiguousarray(origins, dtype=np.uint64)
        _test_check(test_lib().rvn_shard_index_build(self._h, _p(values), _p(origins), values.shape[0], 0))

    def set_occurrence(self, occurrence):
        _test_check(test_lib().rvn_engine_set_occurrence(self._h, int(occurrence)))

    def count_launches(self, on=True):
        """Start counting kernel launches per site from zero (on) / stop."""
        T = test_lib()
        T.rvn_engine_set_kernel_timing(self._h, int(on))
        if on:
            T.rvn_engine_reset_stats(self._h)

    def launches(self):
        """{site: launches} since count_launches()."""
        T = test_lib()
        n = T.rvn_engine_num_kernel_sites()
        ms, la = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint64)
        _test_check(T.rvn_engine_kernel_ms(self._h, _p(ms), _p(la), n))
        return {T.rvn_engine_kernel_site_name(i).decode(): int(la[i]) for i in range(n)}

    def upload(self, rs):
        """A read set of this engine's library (rvn_reads_upload): the handle, to be given back with reads_destroy()."""
        h = C.c_void_p()
        packed = np.ascontiguousarray(rs.packed, dtype=np.uint64)
        _test_check(test_lib().rvn_reads_upload(self._h, _p(packed), int(rs.word_offsets[-1]),
                                                _p(np.ascontiguousarray(rs.word_offsets, dtype=np.uint64)),
                                                _p(np.ascontiguousarray(rs.lengths, dtype=np.uint32)),
                                                _p(np.ascontiguousarray(rs.ids, dtype=np.uint32)), rs.n, C.byref(h)))
        return h

    def reads_destroy(self, h):
        test_lib().rvn_reads_destroy(h)

    def upload_codes(self, code_arrays):
        """A read set of this engine's library from one-byte codes (rvn_reads_upload_codes): the handle, as upload()."""
        lens = np.array([len(a) for a in code_arrays], dtype=np.uint64)
        off = np.zeros(len(code_arrays) + 1, dtype=np.uint64)
        np.cumsum(lens, out=off[1:])
        flat = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(a, np.uint8) for a in code_arrays]))
        h = C.c_void_p()
        _test_check(test_lib().rvn_reads_upload_codes(self._h, _p(flat), _p(off), None, len(code_arrays), C.byref(h)))
        return h

    def set_option(self, name, value):
        """rvn_engine_set_option (Engine.set_option); returns the previous value."""
        prev = C.c_int64(0)
        _test_check(test_lib().rvn_engine_set_option(self._h, name.encode(), int(value), C.byref(prev)))
        return int(prev.value)

    def align_paths(self, queries, targets, pairs, ops=False, guard=0):
        """rvn_test_align_path_batch on read handles of this engine: Engine.align_paths' (distances, offsets, runs or ops,
        pairs not aligned) + plans uint32[n, 5] = every job's final (k, kcap, R, G, S) + the call's counters as a dict.
        guard > 0: the fetch buffers are that many elements longer, pre-set to a pattern, and come back whole (the caller
        checks that nothing was written behind the last element)."""
        pairs = np.ascontiguousarray(pairs, dtype=ALIGN_PAIR_DTYPE)
        T = test_lib()
        h = C.c_void_p()
        plans = np.zeros((max(pairs.shape[0], 1), 5), dtype=np.uint32)
        stats = np.zeros(6, dtype=np.uint64)
        _test_check(T.rvn_test_align_path_batch(self._h, queries, targets, _p(pairs), pairs.shape[0], C.byref(h), _p(plans),
                                                _p(stats)))
        try:
            n, n_runs, n_ops, n_bad = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
            _test_check(T.rvn_paths_info(h, C.byref(n), C.byref(n_runs), C.byref(n_ops), C.byref(n_bad)))
            dist = np.zeros(n.value, dtype=np.uint32)
            off = np.full(n.value + 1 + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            if ops:
                out = np.full(n_ops.value + guard, 0xA5, dtype=np.uint8)
                _test_check(T.rvn_paths_fetch(h, _p(dist), None, None))
                _test_check(T.rvn_paths_fetch_ops(h, _p(off), _p(out) if n_ops.value else None))
            else:
                out = np.full(n_runs.value + guard, 0xA5A5A5A5, dtype=np.uint32)
                _test_check(T.rvn_paths_fetch(h, _p(dist), _p(off), _p(out) if n_runs.value else None))
        finally:
            T.rvn_paths_destroy(h)
        names = ("n_aligned", "n_retries", "n_unaligned", "n_batches", "band_cells", "store_bytes")
        return dist, off, out, int(n_bad.value), plans[:pairs.shape[0]], dict(zip(names, (int(x) for x in stats)))

    def edit_distance_dev(self, reads_handle, pairs, kmax=None, wide_sweep=False):
        """rvn_test_edit_distance_dev: one call of edit_distance_dev (edit_distance.hip) on a read handle of this engine.
        pairs: ED_PAIR_DTYPE; kmax: uint32 per pair or None (unbounded); wide_sweep: the workgroup ring's route (an int
        other than 0 / 1 is passed on as it is, for the refusal).  Returns the uint32 values as stored: the exact distance
        or ED_ABOVE."""
        pairs = np.ascontiguousarray(pairs, dtype=ED_PAIR_DTYPE)
        km = None if kmax is None else np.ascontiguousarray(kmax, dtype=np.uint32)
        assert km is None or km.shape == pairs.shape
        out = np.zeros(max(pairs.shape[0], 1), dtype=np.uint32)
        _test_check(test_lib().rvn_test_edit_distance_dev(self._h, reads_handle, _p(pairs), pairs.shape[0], _p(km),
                                                          int(wide_sweep), _p(out)))
        return out[:pairs.shape[0]]

    def second_pass(self, reads_handle, n, pile_begin, pile_end, pile_invalid, identity, kmer_len, batches):
        """rvn_test_second_pass: the second pass with Map's output of every batch given by the host.  batches = list of
        (q_first, q_last, origins uint64, read_off uint32[q_last - q_first + 1], filtered uint8, overlaps).  Returns
        dict(overlaps, contained, kmers, kmers_offsets) as rvn_pass2_fetch fills them."""
        T = test_lib()
        keep, arr = [], (_Pass2Batch * max(len(batches), 1))()
        for i, (qf, ql, org, off, flt, ovl) in enumerate(batches):
            org = np.ascontiguousarray(org, dtype=np.uint64)
            off = np.ascontiguousarray(off, dtype=np.uint32)
            flt = np.ascontiguousarray(flt, dtype=np.uint8)
            ovl = np.ascontiguousarray(ovl, dtype=OVERLAP_DTYPE)
            assert off.shape[0] == ql - qf + 1 and flt.shape == org.shape
            keep.append((org, off, flt, ovl))
            arr[i] = _Pass2Batch(qf, ql, _p(org) if org.shape[0] else None, _p(off), _p(flt) if flt.shape[0] else None,
                                 org.shape[0], _p(ovl) if ovl.shape[0] else None, ovl.shape[0])
        b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
        en = np.ascontiguousarray(pile_end, dtype=np.uint32)
        inv = np.ascontiguousarray(pile_invalid, dtype=np.uint8)
        assert b.shape[0] == n and en.shape[0] == n and inv.shape[0] == n
        h = C.c_void_p()
        _test_check(T.rvn_test_second_pass(self._h, reads_handle, _p(b), _p(en), _p(inv), float(identity), int(kmer_len),
                                           C.cast(arr, C.c_void_p), len(batches), C.byref(h)))
        try:
            no, nk = int(T.rvn_pass2_num_overlaps(h)), int(T.rvn_pass2_kmer_cells(h))
            ovl = np.zeros(no, dtype=OVERLAP_DTYPE)
            contained = np.zeros(n, dtype=np.uint8)
            kmers = np.zeros(nk, dtype=np.uint8)
            koff = np.zeros(n + 1, dtype=np.uint64)
            _test_check(T.rvn_pass2_fetch(h, _p(ovl), _p(contained), _p(kmers), _p(koff)))
        finally:
            T.rvn_pass2_destroy(h)
        return dict(overlaps=ovl, contained=contained, kmers=kmers, kmers_offsets=koff)

    def match_probe(self, q_values, q_origins, q_read_off, avoid_equal, avoid_symmetric):
        """rvn_test_match_probe: (group words, position words, seg_off[n_reads + 1], filtered[n_query])."""
        qv = np.ascontiguousarray(q_values, dtype=np.uint64)
        qo = np.ascontiguousarray(q_origins, dtype=np.uint64)
        off = np.ascontiguousarray(q_read_off, dtype=np.uint32)
        nr = off.shape[0] - 1
        assert nr >= 0 and qv.shape == qo.shape
        seg = np.zeros(nr + 1, dtype=np.uint64)
        filt = np.zeros(max(qv.shape[0], 1), dtype=np.uint8)
        pg, pp, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        T = test_lib()
        _test_check(T.rvn_test_match_probe(self._h, _p(qv), _p(qo), qv.shape[0], _p(off), nr, int(avoid_equal),
                                           int(avoid_symmetric), C.byref(pg), C.byref(pp), _p(seg), _p(filt), C.byref(n)))
        try:
            grp, pos = (np.ctypeslib.as_array(C.cast(x, C.POINTER(C.c_uint64)), shape=(max(n.value, 1),))[:n.value].copy()
                        for x in (pg, pp))
        finally:
            T.rvn_free(pg)
            T.rvn_free(pp)
        return grp, pos, seg, filt[:qv.shape[0]]


def overlap_update_and_type(overlaps, pile_begin, pile_end, pile_invalid):
    """rvn_overlap_update_and_type: raven::OverlapUpdate + GetOverlapType on host arrays (overlap_utils.cc:14-121):
    (updated overlaps, ok, type)."""
    o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE).copy()
    b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
    ok = np.zeros(o.shape[0], dtype=np.uint8)
    ty = np.zeros(o.shape[0], dtype=np.uint32)
    _check(lib().rvn_overlap_update_and_type(_p(o), o.shape[0], _p(b), _p(np.ascontiguousarray(pile_end, dtype=np.uint32)),
                                             _p(np.ascontiguousarray(pile_invalid, dtype=np.uint8)), b.shape[0], _p(ok), _p(ty)))
    return o, ok, ty


def test_overlap_update_and_type(overlaps, pile_begin, pile_end, pile_invalid):
    """overlap_rules.h on the host (the __host__ __device__ code of the kernels): (updated overlaps, ok, type)."""
    o = np.ascontiguousarray(overlaps, dtype=OVERLAP_DTYPE).copy()
    b = np.ascontiguousarray(pile_begin, dtype=np.uint32)
    ok = np.zeros(o.shape[0], dtype=np.uint8)
    ty = np.zeros(o.shape[0], dtype=np.uint32)
    rc = test_lib().rvn_test_overlap_update_and_type(_p(o), o.shape[0], _p(b), _p(np.ascontiguousarray(pile_end, dtype=np.uint32)),
                                                _p(np.ascontiguousarray(pile_invalid, dtype=np.uint8)), b.shape[0], _p(ok),
                                                _p(ty))
    if rc != 0:
        raise ValueError("rvn_test_overlap_update_and_type")
    return o, ok, ty


def test_parse_file(path, fastq, threads=0, force_streaming=False, slab_bytes=0):
    """TEST INFRASTRUCTURE: the host half of rvn_reads_load (member cut, inflate pool, record scanner) without a device.
    Returns (names, list of base strings, list of quality strings or None, info dict)."""
    T = test_lib()
    b, q, l, nm = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n = C.c_uint32(0)
    info = np.zeros(8, dtype=np.uint32)
    rc = T.rvn_test_parse_file(os.fsencode(path), int(fastq), threads, int(force_streaming), slab_bytes, C.byref(b),
                               C.byref(q), C.byref(l), C.byref(n), C.byref(nm), _p(info))
    if rc != RVN_OK:
        raise (ValueError if rc == RVN_EINVAL else RavenHipError)(T.rvn_last_error().decode(errors="replace"))
    try:
        lens = np.ctypeslib.as_array(C.cast(l, C.POINTER(C.c_uint32)), shape=(max(n.value, 1),))[:n.value].copy()
        total = int(lens.sum())
        bases = C.string_at(b, total)
        quals = C.string_at(q, total) if fastq else None
        names = C.string_at(nm).decode().split("\n")[:-1] if n.value else []
    finally:
        for x in (b, q, l, nm):
            T.rvn_free(x)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seqs = [bases[off[i]:off[i + 1]] for i in range(n.value)]
    qs = [quals[off[i]:off[i + 1]] for i in range(n.value)] if fastq else None
    return names, seqs, qs, dict(gzip=int(info[0]), streaming=int(info[1]), members=int(info[2]), threads=int(info[3]),
                                 restarted=int(info[4]), loop_s=info[5] / 1e6, scan_s=info[6] / 1e6, fast=int(info[7]))


ED_ABOVE, ED_OVERFLOW, ED_OVERFLOW_WIDE = 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFD  # raw codes of the lane kernel


def test_ed_lane(packed, word_offsets, pairs, W, kmax=None):
    """TEST INFRASTRUCTURE: the per-pair body of ed_lane_kernel<W> (edit_distance.hip) on the host, no GPU needed.  pairs:
    ED_PAIR_DTYPE; kmax: uint32 per pair or None; returns the raw uint32 the kernel stores per pair: the exact distance,
    ED_ABOVE (above kmax), ED_OVERFLOW (beyond a window of 3 / 5 slots) or ED_OVERFLOW_WIDE (beyond the widest, 7)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    wo = np.ascontiguousarray(word_offsets, dtype=np.uint64)
    pairs = np.ascontiguousarray(pairs, dtype=ED_PAIR_DTYPE)
    km = None if kmax is None else np.ascontiguousarray(kmax, dtype=np.uint32)
    assert km is None or km.shape[0] == pairs.shape[0]
    out = np.zeros(pairs.shape[0], dtype=np.uint32)
    rc = test_lib().rvn_test_ed_lane(_p(packed), _p(wo), _p(pairs), pairs.shape[0], None if km is None else _p(km), int(W),
                                     _p(out))
    if rc != 0:
        raise ValueError("rvn_test_ed_lane: %d" % rc)
    return out


NW_REC_DTYPE = np.dtype([("first_t", "<u4"), ("first_q", "<u4"), ("last_t", "<u4"), ("last_q", "<u4"),
                         ("grid", "<u2", (8,))])


def test_nw_breakpoints(t_words, t_len, r_words, r_len, t_begin, n, q_begin, m, rc, w, k=64, force_r=0, group_lanes=0,
                       stripe_lanes=0, device=False):
    """nwpath.h stepped on the CPU (no GPU needed): the forward sweep's lane code for 64 emulated lanes + the
    traceback (group_lanes = 4 / 16 / 64: the walk by a group of lanes per alignment, nwtrace.h).  stripe_lanes > 0: the
    striped sweep, stripes of that many lanes (R = force_r, default 1; a band wider than 8 such rings is refused).  Returns
    (records per window, exact distance, band, status) with band = (k, lanes, R), (k, lanes, R, batches of the group
    walk) with group_lanes, and always the five entries (k, lanes, R, batches or 0, stripes) with stripe_lanes.
    device=True: the production stage on the GPU instead (an engine of its own; stripe_lanes = engine option
    nw_stripe_lanes, k / force_r / group_lanes unused); band is then a dict {k, stripe_lanes (0: one ring), R, stripes,
    stage_ms} of the job's final plan."""
    t_words = np.ascontiguousarray(t_words, dtype=np.uint64)
    r_words = np.ascontiguousarray(r_words, dtype=np.uint64)
    n_win = (t_begin + n - 1) // w - t_begin // w + 1
    recs = np.zeros(n_win, dtype=NW_REC_DTYPE)
    dist = np.zeros(1, dtype=np.uint32)
    band = np.zeros(5 if (stripe_lanes or device) else (4 if group_lanes else 3), dtype=np.uint32)
    flags = (1 if rc else 0) | (int(stripe_lanes) << 16) | (1 << 24 if device else int(group_lanes) << 8)
    rc_ = test_lib().rvn_test_nw_breakpoints(_p(t_words), t_len, _p(r_words), r_len, t_begin, n, q_begin, m, flags, w, k,
                                             force_r, _p(recs), _p(dist), _p(band))
    if rc_ < 0:
        raise ValueError("rvn_test_nw_breakpoints: %d" % rc_)
    if device:
        return recs, int(dist[0]), dict(k=int(band[0]), stripe_lanes=int(band[1]), R=int(band[2]), stripes=int(band[3]),
                                        stage_ms=band[4] / 1000.0), rc_
    return recs, int(dist[0]), tuple(int(x) for x in band), rc_
