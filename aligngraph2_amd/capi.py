"""The C ABI of libpagraph_hip.so / libpagraph_host.so restated for ctypes and numpy — the ONLY place where it is.

include/pagraph_hip.h and include/pagraph_host.h are the ABI; include/pagraph_debug.h declares the exported test hooks.
This module mirrors them: one ctypes.Structure per struct Python fills or reads, one numpy dtype per record type Python
fills as arrays, the constants, and SIGNATURES = (restype, argtypes) of every function.  bind(lib) applies the table to a
loaded library; everything else in the tree imports from here.  tests/test_abi.py compiles a probe generated from this
module against the headers (sizes, offsets, constants) and parses the headers' declarations against SIGNATURES, so a header
change is followed by a change here or that test fails.

Imports ctypes and numpy only: importable without torch, without a GPU and without a built library.

Pointer parameters are c_void_p unless every caller passes the one thing a narrower type takes: c_void_p accepts
byref(...), ctypes arrays, None and the plain integers (tensor.data_ptr(), ndarray.ctypes.data) the callers pass.  c_char_p
is kept where callers pass bytes for NUL-terminated strings.  c_void_p as a restype gives None for NULL and a Python int
otherwise (handles, path and text pointers).
"""
import ctypes as C

import numpy as np

# ---- constants ------------------------------------------------------------------------------------------------------------
CONSTANTS = {
    "PAG_OK": 0, "PAG_EINVAL": -22, "PAG_ENOMEM": -12, "PAG_ENODEV": -19, "PAG_ERANGE": -34, "PAG_EFAULT": -14, "PAG_EDOM": -33,
    "PAG_NONE": 0xFFFFFFFF,
    "PAG_ALN_REV_STRAND": 1, "PAG_ALN_WALK_BACK": 2, "PAG_ALN_ELIGIBLE": 4,
    "PAG_ORIENT_NONE": -1, "PAG_ORIENT_REVERSE": 0, "PAG_ORIENT_FORWARD": 1, "PAG_ORIENT_BOTH": 2,
    "PAG_TRAVEL_RENDER_DUMPS": 1, "PAG_TRAVEL_RENDER_SEQS": 2,
    "PAG_DEBUG_WALK_GUARD": 16,
    "PAG_WALK_END": 0, "PAG_WALK_BRANCH": 1, "PAG_WALK_LIMIT": 2, "PAG_WALK_LEAP": 3, "PAG_WALK_LIMIT_MAX": 65536,
}
globals().update(CONSTANTS)

# ---- record types Python fills as arrays: C name -> dtype -------------------------------------------------------------------
DTYPES = {
    "pag_aln": np.dtype([("query", "<u4"), ("target", "<u4"), ("t_begin", "<u4"), ("t_end", "<u4"), ("q_start", "<u4"),
                         ("t_start", "<u4"), ("n_cols", "<u4"), ("n_valid", "<u4"), ("diff_off", "<u8"), ("flags", "<u4"),
                         ("reserved", "<u4")]),
    "pag_ctg": np.dtype([("len", "<u4"), ("selected", "<u4"), ("single_base", "<u4"), ("multi", "<u4"), ("map_off", "<u8")]),
    "pag_ref": np.dtype([("len", "<u4"), ("accepted", "<u4"), ("single_base", "<u4"), ("reserved", "<u4")]),
    # an ALN record as the parser leaves it, names resolved to indices
    "pag_raw_aln": np.dtype([("query", "<u4"), ("target", "<u4"), ("score", "<u8"), ("q_begin", "<u8"), ("q_end", "<u8"),
                             ("t_begin", "<u8"), ("t_end", "<u8"), ("diff_off", "<u8"), ("n_cols", "<u4"), ("n_emit", "<u4"),
                             ("n_radv", "<u4"), ("forward", "<u4")]),
    "pag_path_node": np.dtype([("code", "<u4"), ("ctg", "<u4"), ("ref", "<u4"), ("cnt", "<u2"), ("reserved", "<u2"),
                               ("step", "<i4"), ("vid", "<u4")]),
    # include/pagraph_debug.h: a TravContig as the hooks on constructed graphs take it
    "pag_debug_trav_contig": np.dtype([("nodes_off", "<u8"), ("gbits_off", "<u8"), ("gset_off", "<u8"), ("n_kmers", "<u4"),
                                       ("ctg_left", "<u4"), ("ctg_right", "<u4"), ("in_lo", "<u4"), ("in_hi", "<u4"), ("g_lo", "<u4"),
                                       ("g_hi", "<u4"), ("gmask", "<u4")]),
    # ... the jobs and results of pag_debug_walk
    "pag_debug_walk_job": np.dtype([("has_size", "<u8"), ("seq_cap", "<u8"), ("init_len", "<u8"), ("set_size", "<u8"), ("out_off", "<u8"),
                                    ("ctg", "<u4"), ("start", "<u4"), ("exact", "<u4"), ("mode", "<u4"), ("stop_pc", "<u4"), ("win_low", "<u4")]),
    "pag_debug_walk_out": np.dtype([("seq_len", "<u8"), ("seq_size", "<u8"), ("n_classify", "<u8"), ("n_probe", "<u8"), ("n_records", "<u8"),
                                    ("n_fill", "<u8"), ("n_out", "<u8"), ("n_main", "<u8"), ("max_probe", "<u8"), ("last_ctg", "<u4"),
                                    ("overflow", "<u4"), ("stopped", "<u4"), ("max_back", "<u4"), ("max_chosen", "<u4"),
                                    ("wd_below_max", "<u4"), ("wd_forced_min", "<u4"), ("poison", "<u4")]),
}
PAG_DEBUG_NULL = 0xFFFFFFFFFFFFFFFF  # (pagraph_debug.h; as a C long long it is -1, so it is not among CONSTANTS)

# ---- struct mirrors -----------------------------------------------------------------------------------------------------------
_u32, _i32, _u64, _f64, _vp = C.c_uint32, C.c_int32, C.c_uint64, C.c_double, C.c_void_p


class PagSeqs(C.Structure):
    _c_name_ = "pag_seqs"
    _fields_ = [("n_seqs", _u64), ("byte_off", _vp), ("len", _vp), ("packed", _vp), ("packed_bytes", _u64)]


class PagAlnDb(C.Structure):
    _c_name_ = "pag_aln_db"
    _fields_ = [("n_aln", _u64), ("aln", _vp), ("query_off", _vp), ("diff", _vp), ("n_diff_words", _u64)]


class PagBuildInput(C.Structure):
    _c_name_ = "pag_build_input"
    _fields_ = [("on_device", _u32), ("n_threads", _u32), ("reads", PagSeqs), ("emit_order", _vp), ("read_to_ctg", PagAlnDb),
                ("read_to_ref", PagAlnDb), ("n_ctgs", _u64), ("ctgs", _vp), ("ctg_ent_off", _vp), ("n_ctg_ent_off", _u64),
                ("ctg_ent", _vp), ("n_ctg_ent", _u64), ("n_refs", _u64), ("refs", _vp), ("eps", _u32), ("cov_filter", _u32),
                ("outer_sample", _u32), ("topk_ctg", _i32), ("topk_ref", _i32), ("reserved", _u32)]


class PagRawDb(C.Structure):
    _c_name_ = "pag_raw_db"
    _fields_ = [("n", _u64), ("rec", _vp), ("diff", _vp), ("n_diff_words", _u64)]


class PagRawInput(C.Structure):
    _c_name_ = "pag_raw_input"
    _fields_ = [("bulk_on_device", _u32), ("n_threads", _u32), ("reads", PagSeqs), ("read_to_ctg", PagRawDb),
                ("read_to_ref", PagRawDb), ("ctg_to_ref", PagRawDb), ("n_ctgs", _u64), ("ctg_len", _vp), ("ctg_selected", _vp),
                ("ctg_forward", _vp), ("n_refs", _u64), ("ref_len", _vp), ("ref_accepted", _vp), ("read_to_ctg_ratio", _f64),
                ("read_to_ref_ratio", _f64), ("eps", _u32), ("cov_filter", _u32), ("outer_sample", _u32), ("topk_ctg", _i32),
                ("topk_ref", _i32), ("reserved", _u32)]


class BuildStats(C.Structure):
    _c_name_ = "pag_build_stats"
    _fields_ = [("merge_edge", _u64 * 2), ("total_pos", _u64 * 2), ("merge_pos", _u64 * 2), ("n_tuples", _u64 * 2),
                ("n_edges", _u64 * 2), ("n_nodes", _u64), ("n_pos", _u64), ("n_uniq_edges", _u64), ("ms_extract", _f64),
                ("ms_sort", _f64), ("ms_cluster", _f64), ("ms_edges", _f64), ("ms_total", _f64), ("ms_sort_kernel", _f64),
                ("sort_records", _u64)]

    def counts(self):
        """the six numbers PositionProcessor::process prints, in its order"""
        return (self.merge_edge[0], self.total_pos[0], self.merge_pos[0], self.merge_edge[1], self.total_pos[1],
                self.merge_pos[1])


class Csr(C.Structure):
    _c_name_ = "pag_csr"
    _fields_ = [("n_nodes", _u64), ("n_pos", _u64), ("n_edges", _u64), ("node_code", _vp), ("pos_off", _vp), ("pos_ctg", _vp),
                ("pos_ref", _vp), ("pos_cnt", _vp), ("edge_off", _vp), ("edge_to", _vp), ("edge_step", _vp)]


class ShardSlice(C.Structure):
    _c_name_ = "pag_shard_slice"
    _fields_ = [("n_t", _u64), ("n_e", _u64), ("tkey", _vp), ("tval", _vp), ("tseg", _vp), ("tcnt", _vp), ("ekey", _vp),
                ("eval", _vp), ("eseg", _vp), ("stats", BuildStats)]


class Region(C.Structure):
    _c_name_ = "pag_region"
    _fields_ = [("n_ctg_iv", _u64), ("ctg_iv", _vp), ("n_ref_iv", _u64), ("ref_iv", _vp), ("ref_open", _vp)]


class SerialStats(C.Structure):
    _c_name_ = "pag_serial_stats"
    _fields_ = [("held_vertices", _u64), ("held_edges", _u64), ("tuples_in", _u64), ("edges_in", _u64), ("region_bytes", _u64),
                ("s_extract", _f64), ("s_build", _f64), ("s_select", _f64), ("s_import", _f64)]


class TravelParams(C.Structure):
    _c_name_ = "pag_travel_params"
    _fields_ = [("ref_threads", _u32), ("reserved", _u32), ("deviation", _u64), ("error_rate", _f64), ("start_split", _f64),
                ("min_len", _u64)]


class TravelStats(C.Structure):
    _c_name_ = "pag_travel_stats"
    _fields_ = [("ms_compact", _f64), ("ms_walk", _f64), ("ms_total", _f64), ("rounds", _u64), ("jobs", _u64),
                ("walk_steps", _u64), ("classify_calls", _u64), ("probes", _u64), ("records", _u64)]


class PagSucc(C.Structure):
    _c_name_ = "pag_succ"
    _fields_ = [("code", _u32), ("step", _u32), ("pos", _u64), ("grade", _u32), ("ctg_similar", _u32)]


class PagSuccQuery(C.Structure):
    _c_name_ = "pag_succ_query"
    _fields_ = [("code", _u32), ("reserved", _u32), ("pos", _u64)]


class PagFindHit(C.Structure):
    _c_name_ = "pag_find_hit"
    _fields_ = [("offset", _u32), ("code", _u32), ("first", _u64), ("n_pos", _u32), ("reserved", _u32)]


class PagFindVertex(C.Structure):
    _c_name_ = "pag_find_vertex"
    _fields_ = [("pos", _u64), ("abundance", _u32), ("reserved", _u32)]


class PagWalkFrame(C.Structure):
    _c_name_ = "pag_walk_frame"
    _fields_ = [("ctg_left", _u32), ("ctg_right", _u32), ("rev_left", _u32), ("rev_right", _u32), ("split_size", _u64), ("leap_min", _f64),
                ("hull_lo", _u32 * 2), ("hull_hi", _u32 * 2), ("excl_off", _u64), ("excl_n", _u64)]


class PagWalkQuery(C.Structure):
    _c_name_ = "pag_walk_query"
    _fields_ = [("code", _u32), ("dist", _u32), ("pos", _u64), ("has_size", _u64), ("frame", _u32), ("limit", _u32)]


class PagWalkNode(C.Structure):
    _c_name_ = "pag_walk_node"
    _fields_ = [("code", _u32), ("step", _u32), ("pos", _u64), ("abundance", _u32), ("reserved", _u32)]


# ... as numpy record types (derived: the Structures above are what tests/test_abi.py holds to the header)
FIND_HIT_DTYPE, FIND_VERTEX_DTYPE = np.dtype(PagFindHit), np.dtype(PagFindVertex)
SUCC_DTYPE, SUCC_QUERY_DTYPE = np.dtype(PagSucc), np.dtype(PagSuccQuery)
WALK_FRAME_DTYPE, WALK_QUERY_DTYPE, WALK_NODE_DTYPE = np.dtype(PagWalkFrame), np.dtype(PagWalkQuery), np.dtype(PagWalkNode)


class CnsAln(C.Structure):
    _c_name_ = "pag_cns_aln"
    _fields_ = [("str_off", _u64), ("len", _u32), ("start", _u32), ("weight", _i32), ("reserved", _u32)]


class CnsPart(C.Structure):
    _c_name_ = "pag_cns_part"
    _fields_ = [("bb_off", _u64), ("bb_len", _u32), ("n_aln", _u32), ("aln_first", _u64), ("node_cap", _u32),
                ("edge_cap", _u32), ("aux_cap", _u32), ("out_cap", _u32)]


class CnsSlice(C.Structure):
    _c_name_ = "pag_cns_slice"
    _fields_ = [("q_off", _u64), ("t_off", _u64), ("origin_start", _u64), ("slice_start", _u64), ("slice_end", _u64),
                ("out_off", _u64), ("n_cols", _u32), ("out_cap", _u32), ("slot", _u32), ("reserved", _u32)]


class CnsRow(C.Structure):
    _c_name_ = "pag_cns_row"
    _fields_ = [("str_off", _u64), ("len", _u32), ("n_ins", _u32), ("n_edge_cols", _u32), ("flag", _u32)]


class KmerCountResult(C.Structure):
    _c_name_ = "pag_kmer_count_result"
    _fields_ = [("min_abundance", _u64), ("n_solid", _u64), ("n_kmers_counted", _u64), ("ms_count", _f64), ("ms_select", _f64)]


class TraverseStats(C.Structure):
    _c_name_ = "pagh_traverse_stats"
    _fields_ = [("n_contigs", _u64), ("n_path_nodes", _u64), ("n_path_bases", _u64), ("n_chains_emitted", _u64),
                ("n_fasta_bases", _u64), ("path_checksum", _u64), ("ms_export", _f64), ("ms_traverse", _f64), ("ms_total", _f64),
                ("ms_successors", _f64), ("ms_walk", _f64), ("walk_rounds", _u64), ("walk_jobs", _u64), ("walk_steps", _u64),
                ("walk_classifications", _u64)]


class DebugTravGraph(C.Structure):
    _c_name_ = "pag_debug_trav_graph"
    _fields_ = [("n_nodes", _u64), ("n_pos", _u64), ("k", _u32), ("reserved", _u32), ("ncode", _vp), ("npos_off", _vp), ("vpos", _vp),
                ("vcnt", _vp), ("vnode", _vp), ("uold", _vp), ("newid", _vp), ("upos", _vp), ("ucnt", _vp), ("bitmap", _vp), ("rank", _vp),
                ("succ_off", _vp), ("succ", _vp), ("incomplete", _vp), ("n_succ", _u64)]


class DebugWalkContig(C.Structure):
    _c_name_ = "pag_debug_walk_contig"
    _fields_ = [("ctg_left", _u32), ("ctg_right", _u32), ("rev_left", _u32), ("rev_right", _u32), ("split_size", _u64), ("leap_min", _f64),
                ("n_ctgs", _u32), ("in_lo", _u32), ("in_hi", _u32), ("g_lo", _u32), ("g_hi", _u32), ("gmask", _u32), ("gwin_lo", _u32),
                ("gwin_hi", _u32), ("starts", _vp), ("sizes", _vp), ("gbits", _vp), ("gset", _vp), ("n_gbits", _u64)]


STRUCTS = {s._c_name_: s for s in (PagSeqs, PagAlnDb, PagBuildInput, PagRawDb, PagRawInput, BuildStats, Csr, ShardSlice, Region,
                                   SerialStats, TravelParams, TravelStats, PagSucc, PagSuccQuery, PagFindHit, PagFindVertex, PagWalkFrame, PagWalkQuery, PagWalkNode, CnsAln, CnsPart, CnsSlice, CnsRow, KmerCountResult, TraverseStats,
                                   DebugTravGraph, DebugWalkContig)}

# structs of the headers that are deliberately mirrored neither in STRUCTS nor in DTYPES: C name -> why.  (The opaque
# handles pag_graph and pag_comm have no body to mirror.)
NOT_MIRRORED = {}

# ---- signatures: name -> (restype, argtypes) ----------------------------------------------------------------------------------
_int, _i64, _cs = C.c_int, C.c_int64, C.c_char_p
_u64p, _i64p, _intp = C.POINTER(_u64), C.POINTER(_i64), C.POINTER(_int)
_stats, _slice, _region = C.POINTER(BuildStats), C.POINTER(ShardSlice), C.POINTER(Region)
# pagh_traverse; pagh_traverse_begin takes the same list without the statistics
_traverse = [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _u64, _cs, _cs, _u32, _vp]
_cns = [_int, _cs, _u64, _vp, _u64, _vp, _u64, _cs, _cs, _u64, _i32, _vp, _u64, _vp, _vp, _vp]

SIGNATURES = {
    # include/pagraph_hip.h
    "pag_create": (_vp, [_vp, _u64, _u32, _int, _intp]),
    "pag_create_from_bitmap": (_vp, [_vp, _u64, _u32, _int, _int, _intp]),
    "pag_destroy": (None, [_vp]),
    "pag_solid_count": (_u64, [_vp]),
    "pag_reset": (_int, [_vp]),
    "pag_process": (_int, [_vp, _vp, _vp]),
    "pag_prepare": (_int, [_vp, _vp, _vp]),
    "pag_shard_extract": (_int, [_vp, _vp, _u32, _u32, _u64p]),
    "pag_shard_extract_range": (_int, [_vp, _vp, _u64, _u64, _u32, _u64p]),
    "pag_shard_extract_for": (_int, [_vp, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _u64, _u64, _u64p]),
    "pag_shard_take": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "pag_shard_take_part": (_int, [_vp, _u64, _u64, _vp, _vp, _u64, _u64, _vp, _vp]),
    "pag_shard_build": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _u32, _stats]),
    "pag_shard_export": (_int, [_vp, _slice]),
    "pag_shard_take_slice": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pag_shard_import": (_int, [_vp, _slice, _u32, _stats]),
    "pag_shard_select": (_int, [_vp, _region, _slice]),
    "pag_shard_set_region": (_int, [_vp, _region]),
    "pag_shard_release_build": (_int, [_vp]),
    "pag_shard_adopt": (_int, [_vp, _u64, _u64, _stats]),
    "pag_comm_create": (_vp, [_int, _int, _cs, _int, _cs, _intp]),
    "pag_comm_destroy": (None, [_vp]),
    "pag_comm_rank": (_int, [_vp]),
    "pag_comm_world": (_int, [_vp]),
    "pag_comm_bytes_sent": (_u64, [_vp]),
    "pag_comm_abort": (None, [_vp, _cs]),
    "pag_comm_barrier": (_int, [_vp]),
    "pag_comm_all_gather": (_int, [_vp, _vp, _u64, _vp]),
    "pag_comm_gather_v": (_int, [_vp, _vp, _u64, _int, _vp, _u64, _vp, _vp]),
    "pag_comm_all_to_all_v": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "pag_shard_run": (_int, [_vp, _vp, _vp, _vp, _stats]),
    "pag_shard_run_serial": (_int, [_vp, _vp, _vp, _u32, _u32, _stats, _vp]),
    "pag_csr_sizes": (_int, [_vp, _u64p, _u64p, _u64p]),
    "pag_export_csr": (_int, [_vp, _vp]),
    "pag_travel_prepare": (_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "pag_travel_prepare_for": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "pag_travel_view_sizes": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pag_travel": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "pag_successors": (_i64, [_vp, _u32, _u64, _vp, _u64]),
    "pag_successors_batch": (_int, [_vp, _vp, _u64, _u64, _f64, _vp, _vp, _vp, _u64, _u64p, _vp]),
    "pag_successors_batch_bytes": (_u64, [_u64, _u64]),
    "pag_find_all_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _u64p, _u64p, _vp]),
    "pag_find_all_batch_bytes": (_u64, [_u64, _u64, _u64, _u64]),
    "pag_walk_straight_batch": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _f64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64p, _u64p,
                                       _vp]),
    "pag_walk_straight_batch_bytes": (_u64, [_u64, _u64, _u64, _u64, _u64]),
    "pag_travel_path": (_vp, [_vp, _u64, _u64p]),
    "pag_travel_path_oriented": (_vp, [_vp, _u64, _int, _u64p]),
    "pag_reserve_walk_arena": (_int, [_vp, _u64]),
    "pag_render_dump_lines": (_int, [_vp, _u64, _u32, _vp, _u64, _vp, _u64, _vp, _u64, _u64p, _int]),
    "pag_travel_dump_text": (_vp, [_vp, _u64, _int, _u64p]),
    "pag_render_path_sequence": (_int, [_vp, _u64, _u32, _vp, _vp, _u64, _f64, _vp, _u64, _u64p, _int]),
    "pag_travel_seq_sources": (_int, [_vp, _vp]),
    "pag_travel_seq_text": (_vp, [_vp, _u64, _int, _u64p]),
    "pag_pack_text_seqs": (_int, [_vp, _int, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _int]),
    "pag_classify_columns": (_int, [_vp, _int, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _int]),
    "pag_classify_columns_host": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _int]),
    "pag_cns_consensus": (_int, _cns),
    "pag_cns_consensus_wave": (_int, _cns),
    "pag_cns_normalize": (_int, [_int, _vp, _u64, _vp, _u64, _vp, _vp]),
    "pag_cns_rows_bytes": (_u64, [_vp]),
    "pag_cns_rows_times": (None, [_vp, _vp, _vp]),
    "pag_cns_rows_counts": (None, [_vp, _vp, _vp]),
    "pag_cns_rows_fetch": (_int, [_vp, _vp, _vp, _u64]),
    "pag_cns_rows_free": (None, [_vp]),
    "pag_cns_consensus_rows": (_int, [_int, _int, _cs, _u64, _vp, _u64, _vp, _u64, _vp, _i32, _vp, _u64, _vp, _vp, _vp]),
    "pag_kmer_count": (_int, [_vp, _int, _u32, _f64, _int, _vp, _int, _vp]),
    "pag_last_error": (_cs, []),
    "pag_device_available": (_int, []),
    "pag_device_warm": (_int, [_int]),
    # include/pagraph_host.h
    "pagh_traverse": (_int, _traverse),
    "pagh_traverse_begin": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _u64, _cs, _cs, _u32]),
    "pagh_traverse_end": (_int, [_vp, _vp]),
    "pagh_assemble_paths": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _u64, _cs, _cs, _u32, _vp]),
    "pagh_assemble_paths_text": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _u64, _cs, _cs, _u32,
                                        _vp]),
    "pagh_assemble_paths_seq": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _u64, _cs, _cs,
                                       _u32, _vp]),
    "pagh_release": (None, [_vp]),
    "pagh_last_error": (_cs, []),
    # include/pagraph_debug.h: test hooks, not API
    "pag_debug_edit_distance": (_u64, [_cs, _cs]),
    "pag_debug_mapper_d2s": (_u64, [_vp, _u64, _i64, _i64]),
    "pag_debug_mapper_s2d": (None, [_vp, _u64, _u64, _i64p, _i64p]),
    "pag_debug_mapper_extra": (_u64, [_vp, _u64]),
    "pag_debug_succ_sizes": (_int, [_vp, _vp, _vp]),
    "pag_debug_succ": (_int, [_vp, _vp, _vp]),
    "pag_debug_trav_vertices": (_int, [_vp, _vp, _vp]),
    "pag_debug_stream_sizes": (_int, [_vp, _u64p, _u64p]),
    "pag_debug_streams": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "pag_debug_slot_grow": (_int, [_vp, _vp, _u32, _vp, _vp, _u64]),
    "pag_debug_cov_filter": (_int, [_vp, _u64, _vp, _u64, _u32, _vp, _int]),
    "pag_debug_predicates": (_int, [_vp, _u64, _f64, _vp, _vp, _int]),
    "pag_debug_predicates_tab": (_int, [_vp, _u64, _f64, _vp, _vp, _int, _vp]),
    "pag_debug_owner_pick": (_int, [_vp, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _u64, _u64, _u64, _u64p, _int]),
    "pag_debug_shard_run_serial": (_int, [_vp, _vp, _vp, _u32, _u32, _stats, _vp, _int]),
    "pag_debug_zone_bands": (_int, [_vp, _u64, _vp, _u32, _vp, _vp, _int]),
    "pag_debug_trav_compact": (_int, [_u32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _region, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _int]),
    "pag_debug_view_region": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _f64, _vp, _vp, _vp, _vp, _u64]),
    "pag_debug_trav_bounds": (_int, [_vp, _vp, _u32, _vp, _vp, _u32, _int]),
    "pag_debug_ctg_nodes": (_int, [_vp, _vp, _u64, _vp, _u32, _u32, _vp, _u64, _int]),
    "pag_debug_trav_seeds": (_int, [_vp, _int, _vp, _u32, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u32, _u64, _vp, _u64, _u32, _int]),
    "pag_debug_pack_paths": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _u32, _u64, _vp, _u64, _int]),
    "pag_debug_commit": (_int, [_vp, _u64, _u32, _u32, _vp, _u64, _u64, _vp, _u32, _int]),
    "pag_debug_clear_ranges": (_int, [_vp, _u64, _vp, _u64, _int]),
    "pag_debug_concat_parts": (_int, [_vp, _vp, _u64, _vp, _u32, _vp, _vp, _u64, _u32, _int]),
    "pag_debug_gathers": (_int, [_vp, _int, _vp, _vp, _u64, _u32, _vp, _int]),
    "pag_debug_walk": (_int, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u64, _vp, _int]),
    "pag_debug_walk_geometry": (_int, [_vp, _u32]),
    "pagh_debug_classify_columns": (None, [_cs, _u64, _cs, _u64, _vp, _vp, _vp, _int]),
    "pagh_debug_pack_bases": (None, [_cs, _u64, _vp, _int]),
}


def bind(lib, rename=None):
    """Applies SIGNATURES to every listed symbol that `lib` exports and returns `lib`.  rename(name) -> the symbol that carries
    name's signature in `lib`, or None for no such symbol (the C oracle's pago_* twins of some pag_* entry points)."""
    for name, (restype, argtypes) in SIGNATURES.items():
        sym = rename(name) if rename else name
        fn = getattr(lib, sym, None) if sym else None
        if fn is not None:
            fn.restype = restype
            fn.argtypes = list(argtypes)
    return lib
