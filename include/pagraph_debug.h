/* include/pagraph_debug.h — test hooks, not API.
 *
 * The two libraries export a handful of functions for the test suite alone: internal pieces (the edit distance, the
 * position mapper, the predicates, the coverage filter, the host packers) and intermediate state (emitted streams,
 * successor records) that no entry point of pagraph_hip.h / pagraph_host.h hands out.  Nothing in the product calls them
 * and they may change with the code they look into.  They are declared here so that the translation units that define
 * them are held to one declaration by the compiler, and the Python mirror (aligngraph2_amd/capi.py) by
 * tests/test_abi.py. */
#ifndef PAGRAPH_DEBUG_H
#define PAGRAPH_DEBUG_H

#include "pagraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- libpagraph_hip.so ---- */
/* host restatements the traversal uses, against the reference's function-level golden tables */
uint64_t pag_debug_edit_distance(const char *a, const char *b);
uint64_t pag_debug_mapper_d2s(const uint32_t *len, uint64_t n, int64_t idx, int64_t pos);
void pag_debug_mapper_s2d(const uint32_t *len, uint64_t n, uint64_t single, int64_t *idx, int64_t *pos);
uint64_t pag_debug_mapper_extra(const uint32_t *len, uint64_t n);
/* the prepared view's successor records: succ_off[n_pos + 1], then n_succ records of 16 bytes; its vertices by value */
int pag_debug_succ_sizes(const pag_graph *g, uint64_t *n_pos, uint64_t *n_succ);
int pag_debug_succ(const pag_graph *g, uint32_t *succ_off, void *recs);
int pag_debug_trav_vertices(const pag_graph *g, uint32_t *code, uint64_t *pos);
/* raw emitted streams of the last pag_process (needs PAG_DEBUG_KEEP_STREAMS=1) */
int pag_debug_stream_sizes(const pag_graph *g, uint64_t *n_tuples, uint64_t *n_edges);
int pag_debug_streams(const pag_graph *g, uint32_t *tkey, uint64_t *tval, uint32_t *ekey, uint64_t *eval);
/* the coverage filter's kernel on records in host memory: ok[n_aln] */
int pag_debug_cov_filter(const pag_aln *aln, uint64_t n_aln, const pag_ref *refs, uint64_t n_refs, uint32_t cov_filter,
                         uint8_t *ok, int device);
/* checkPosition / isEdgeSimilar over rows of six u32, directly and through the successor kernels' ratio table */
int pag_debug_predicates(const uint32_t *rows, uint64_t n, double err, uint8_t *grade, uint8_t *edge_sim, int device);
int pag_debug_predicates_tab(const uint32_t *rows, uint64_t n, double err, uint8_t *grade, uint8_t *edge_sim, int device,
                             uint64_t *n_through_table);
/* the stable compaction of one owner's records (k_owner_pick.hip) on HOST arrays: the records i of (key, val)[n] with
 * (key[i] >> shift) == owner, in order — i < n1 to out[at1 ..), the others to out[at2 ..); counts[2].  out_key / out_val[cap]
 * are uploaded as they are and come back: what the kernel did not write is what the caller put there. */
int pag_debug_owner_pick(const uint32_t *key, const uint64_t *val, uint64_t n, uint64_t n1, uint32_t shift, uint32_t owner,
                         uint32_t *out_key, uint64_t *out_val, uint64_t cap, uint64_t at1, uint64_t at2, uint64_t *counts, int device);
/* pag_shard_run_serial with the owner's records taken the other way when via_partition != 0: pag_shard_extract_range (both
 * streams partitioned by owner) + pag_shard_take_part.  For the one measurement that compares the two, and the test that
 * they build the same graph. */
int pag_debug_shard_run_serial(pag_graph *g, const pag_build_input *in, const pag_region *regions, uint32_t n_ranks, uint32_t turn,
                               pag_build_stats *total, pag_serial_stats *st, int via_partition);

/* ---- libpagraph_host.so ---- */
/* one record's column classes / one sequence packed, by the production path or by the scalar loop alone */
void pagh_debug_classify_columns(const char *q, uint64_t n, const char *r, uint64_t rn, uint32_t *words, uint32_t *n_emit,
                                 uint32_t *n_radv, int scalar_only);
void pagh_debug_pack_bases(const char *sq, uint64_t n, uint8_t *out, int scalar_only);

#ifdef __cplusplus
}
#endif
#endif /* PAGRAPH_DEBUG_H */
