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
/* The grow rule of the handle's pool slots (slot_grow, pag_graph_impl.hpp) on one slot of a SCRATCH handle (pag_create; nothing
 * else of it is used), step by step.  steps[n_steps] rows of four u64 (need, want, keep, op):
 *   op 0: the slot grown to hold `need` bytes — a new array of `want` bytes whose first `keep` are the old one's, unless the slot
 *         holds `need` already;  op 1: the same while frees are deferred (the replaced array is parked, not freed)
 *   op 2: the parked arrays are released;  op 3: byte i of the slot set to (uint8_t)(i * 7 + need), all of its capacity;
 *   op 4: the slot freed
 * out[n_steps] rows of five u64, the state after the step: the step's return code (a PAG_* value, sign-extended), the slot's
 * pointer, its capacity, the number of parked arrays, and 1 when this step parked the replaced array and its first `keep` bytes
 * still read the same as the new one's.  kept[n_steps * kept_stride]: row i holds the first min(keep, kept_stride) bytes of the
 * slot as read back after a successful op 0 / 1 with keep != 0. */
int pag_debug_slot_grow(pag_graph *g, const uint64_t *steps, uint32_t n_steps, uint64_t *out, uint8_t *kept, uint64_t kept_stride);
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
/* The cut of the traversal graph, piece by piece (tests/test_gpu_view_cut.py against tests/view_rule.py).
 * k_zone_bands (k5_view.hip) on HOST arrays: per zone z of zones[2 n_z] (sorted disjoint [lo, hi) pairs of contig coordinates) the
 * lowest / highest reference coordinate among the slots of tval[T] whose contig coordinate lies in it; lo[z] all ones and hi[z] 0
 * where there is none. */
int pag_debug_zone_bands(const uint64_t *tval, uint64_t T, const uint32_t *zones, uint32_t n_z, uint32_t *lo, uint32_t *hi, int device);
/* trav_compact (k5_view.hip) on HOST arrays in the layout of a slice (pag_shard_slice): the view's vertices and nodes out of the
 * tuple slots, the edges of its nodes.  region: the interval tables of the view (its ref_open is not read), NULL: the whole graph.
 * counts[3] goes in as (nodes, vertices, edges) of the graph — what pag_process counts: exact for region == NULL, upper bounds
 * otherwise — and comes back as those of the view.  The outputs are sized by what went in: vpos / vcnt / vnode[vertices],
 * ncode[nodes], npos_off / nedge_off[nodes + 1], eto / estep[edges]; the view's part of each is written.  Device buffers of its
 * own, freed before it returns. */
int pag_debug_trav_compact(uint32_t k, const uint32_t *tkey, const uint64_t *tval, const uint32_t *tseg, const uint16_t *tcnt, uint64_t T,
                           const uint32_t *ekey, const uint64_t *eval, const uint32_t *eseg, uint64_t E, const pag_region *region,
                           uint64_t *vpos, uint16_t *vcnt, uint32_t *vnode, uint32_t *ncode, uint32_t *npos_off, uint32_t *nedge_off,
                           uint32_t *eto, uint32_t *estep, uint64_t *counts, int device);
/* trav_view_region (trav_prepare_host.hpp) for the handle's current graph under the current PAG_VIEW_HALO / PAG_VIEW_MARGIN: what
 * pag_travel_prepare_for(orient) would cut the view to.  sizes[2] = pairs in civ / riv; civ[2 cap], riv[2 cap], ropen[2 cap] are
 * filled when both fit `cap` pairs (PAG_ERANGE otherwise, sizes set). */
int pag_debug_view_region(pag_graph *g, const uint32_t *ctg_len, uint64_t n_ctgs, const int32_t *orient, const uint32_t *ref_len,
                          uint64_t n_refs, double start_split, uint32_t *civ, uint32_t *riv, uint8_t *ropen, uint64_t *sizes, uint64_t cap);

/* The kernels around the walker waves (k5_walk_aux.hip, and k_ctg_nodes of k5_view.hip), one by one, on CONSTRUCTED graphs
 * (tests/test_gpu_walk_aux.py against tests/walk_aux_rule.py).  No handle: a traversal graph is described by host arrays, as the
 * kernels read it; an array a kernel does not read may be NULL.  Every hook uploads into device buffers of its own, calls the
 * PRODUCTION launcher (trav_launch_*, trav_clear_ranges) and frees the buffers before it returns.  Output arrays are uploaded as
 * the caller filled them and copied back whole: what a kernel did not write is what the caller put there.  The hooks refuse
 * (PAG_EINVAL) what would make a kernel read or write outside these buffers or never end. */
typedef struct pag_debug_trav_graph {
    uint64_t n_nodes, n_pos;
    uint32_t k, reserved;
    const uint32_t *ncode;    /* [n_nodes] */
    const uint32_t *npos_off; /* [n_nodes + 1] */
    const uint64_t *vpos;     /* [n_pos] ctg << 32 | ref, k-mer-major */
    const uint16_t *vcnt;     /* [n_pos] */
    const uint32_t *vnode;    /* [n_pos] */
    const uint32_t *uold;     /* [n_pos] new id -> vertex */
    const uint32_t *newid;    /* [n_pos] vertex -> new id */
    const uint64_t *upos;     /* [n_pos] positions by new id */
    const uint32_t *ucnt;     /* [n_pos] abundances by new id */
    const uint64_t *bitmap;   /* [(4^k + 63) / 64] */
    const uint32_t *rank;     /* [(4^k + 63) / 64] */
    /* what the walker waves read beside newid / upos / ucnt (pag_debug_walk) */
    const uint32_t *succ_off; /* [n_pos + 1] successor records of new id u; succ_off[n_pos] = n_succ */
    const void *succ;         /* [n_succ] records of 16 bytes: tgt, pc, meta, toff (SuccRec, pag_travel.hpp) */
    const uint32_t *incomplete; /* [(n_pos + 31) / 32] bit u: the records of u are a marker (may be NULL).  Uploaded into
                                 * TravGraph::incomplete and nothing more: a walk reads the marker RECORDS, never this bitmap */
    uint64_t n_succ;
} pag_debug_trav_graph;
/* the fields of a TravContig (pag_travel.hpp) these kernels read, by value; its three pointers as word offsets into the arrays
 * `nodes`, `gbits`, `gset` given beside the records (PAG_DEBUG_NULL: a null pointer) */
#define PAG_DEBUG_NULL 0xFFFFFFFFFFFFFFFFull
typedef struct pag_debug_trav_contig {
    uint64_t nodes_off, gbits_off, gset_off;
    uint32_t n_kmers, ctg_left, ctg_right, in_lo, in_hi, g_lo, g_hi, gmask;
} pag_debug_trav_contig;
/* k_id_bounds over coords[n] -> out[n], then k_ranges over ctgs[n_ctgs]: in_lo / in_hi / g_lo / g_hi of the records come back */
int pag_debug_trav_bounds(const pag_debug_trav_graph *g, const uint32_t *coords, uint32_t n, uint32_t *out, pag_debug_trav_contig *ctgs,
                          uint32_t n_ctgs, int device);
/* k_ctg_nodes: jobs[n_jobs] rows of four u64 (byte_off, out_off, len, forward) -> out[n_out].  `packed` as pag_seqs wants it
 * (every strand on a 4-byte boundary, >= 16 readable bytes behind the last); the device copy gets the 64 bytes setup_contigs
 * adds.  The kernel reads the 32-bit word BEHIND the one a k-mer starts in whether the k-mer reaches into it or not: for the last
 * k-mer of the last strand that word may lie wholly behind the strand's bytes — inside the 16 bytes of pag_seqs' padding. */
int pag_debug_ctg_nodes(const pag_debug_trav_graph *g, const uint8_t *packed, uint64_t packed_bytes, const uint64_t *jobs, uint32_t n_jobs,
                        uint32_t max_len, uint32_t *out, uint64_t n_out, int device);
/* the seed family.  which = 0: k_seed_first over ctgs[n_ctgs] (out: n_ctgs x stride words); 1: k_seed_window over reqs[n_req]
 * rows of four u64 (ctg, left, right, pos) (out: n_req x TRAV_SEED_PARTS x stride words); 2: k_checkpoints over reqs (out: 3 words per
 * request; stride is not read).  out[out_words] may be longer than that: the rest must come back as it went in. */
int pag_debug_trav_seeds(const pag_debug_trav_graph *g, int which, const pag_debug_trav_contig *ctgs, uint32_t n_ctgs, const uint32_t *nodes,
                         uint64_t n_node_words, const uint32_t *gbits, uint64_t n_gbits, const uint32_t *gset, uint64_t n_gset,
                         const uint64_t *reqs, uint32_t n_req, uint64_t dev, uint32_t *out, uint64_t out_words, uint32_t stride, int device);
/* k_pack_paths: descs[n] rows of four u64 (first entry in seq_v / seq_s / seq_x, len, word offset in out, leap job: seq_x is
 * read) */
int pag_debug_pack_paths(const pag_debug_trav_graph *g, const uint32_t *seq_v, const uint32_t *seq_s, const uint64_t *seq_x, uint64_t n_seq,
                         const uint64_t *descs, uint32_t n, uint64_t max_len, uint32_t *out, uint64_t out_words, int device);
/* k_commit of seq_v[len] into gbits + gbits_off (bitmap over [in_lo, in_hi)) and gset[ncap] */
int pag_debug_commit(const uint32_t *seq_v, uint64_t len, uint32_t in_lo, uint32_t in_hi, uint32_t *gbits, uint64_t n_gbits, uint64_t gbits_off,
                     uint32_t *gset, uint32_t ncap, int device);
/* k_clear_ranges on buf[bytes], whose device copy starts on a 256-byte boundary: ranges[n] rows of three u64 (offset, bytes, word) */
int pag_debug_clear_ranges(uint8_t *buf, uint64_t bytes, const uint64_t *ranges, uint64_t n, int device);
/* k_concat_parts: parts[n_parts] rows of three u64 (first entry in src_v / src_s, start in out_v / out_s, n) */
int pag_debug_concat_parts(const uint32_t *src_v, const uint32_t *src_s, uint64_t n_src, const uint64_t *parts, uint32_t n_parts, uint32_t *out_v,
                           uint32_t *out_s, uint64_t n_out, uint32_t first_step, int device);
/* the gathers.  which = 0: k_gather_pc (out: u32[len]); 1: k_gather_path with max_blocks (out: pag_path_node[len]); 2:
 * k_gather_vertices over the k-mer-major ids seq_v (out: pag_path_node[len]; seq_s, max_blocks not read) */
int pag_debug_gathers(const pag_debug_trav_graph *g, int which, const uint32_t *seq_v, const uint32_t *seq_s, uint64_t len, uint32_t max_blocks,
                      void *out, int device);

/* The walker wave itself (walk_job of k5_travel.hip: graphTravel / walkStraight / classifySuccessors over the successor records) on
 * a CONSTRUCTED graph (tests/test_gpu_walk.py against tests/walk_rule.py).  The graph is g's newid / upos / ucnt / succ_off / succ
 * (all required).  ctgs[n_ctgs]: the TravContig records by value, their arrays as host pointers (starts[n_ctgs + 1], sizes[n_ctgs];
 * gbits[n_gbits] a bitmap over [g_lo, g_hi), gset[gmask + 1], both NULL or both given).  jobs[n_jobs]: one walk each.
 *
 * Buffers.  seq_v / seq_s / seq_x[n_seq] are uploaded as the caller filled them and come back whole.  Job j owns the entries
 * [out_off, out_off + seq_cap) of each, followed by PAG_DEBUG_WALK_GUARD guard entries inside the same allocation which no job may
 * touch (the caller fills them and compares them afterwards); the ranges of the jobs, guards included, must not overlap.  A
 * RESUME job finds the init_len entries of its path at the head of its seq_v / seq_s range.  seq_x is handed to a LEAP job only,
 * its range zeroed first.  The other buffers of a job are built as post_batch (walk_session_jobs.hpp) builds them, each in an
 * allocation of its own with guard words behind it that the hook itself checks (PAG_EFAULT when one was written):
 *   stamp  TRAV_PROBE_GROUPS arrays of `stride` words, stride = (in_hi - in_lo + 1) rounded up to a multiple of four; zeroed
 *   tbits  stride + 4 words, zeroed
 *   tset   set_size 64-bit entries, all ones;  pset  TRAV_PROBE_GROUPS x set_size entries, zeroed (tmask = pmask = set_size - 1)
 *   arena  TRAV_PROBE_GROUPS x seq_cap entries for vertices and as many for steps
 * The launch is trav_launch_walk — the one-shot k_walk, the same walk_job body as the persistent grid; the persistent kernel and
 * its queue are never started here.  outs[n_jobs] is TravJobOut in plain C (n_fill: bits 32.. hold the reasons of a
 * mis-speculation, as the kernel reports them).
 *
 * Refused with PAG_EINVAL before anything is launched — what would let the kernel read or write outside these buffers: a record
 * with tgt >= n_pos, or whose pc / toff / count nibble disagree with upos[tgt] >> 32 (a marker record, grade 6 or 7: 0), succ_off[tgt] and min(count of tgt, 15);
 * succ_off not starting at 0, not monotonic or not ending at n_succ; newid[start] (or start) out of range; a contig without
 * g_lo <= in_lo <= in_hi <= g_hi <= n_pos, with in_lo - g_lo no multiple of 32, a bitmap shorter than its range, starts not
 * ascending, a gset that is no power of two in size or has no empty entry; seq_cap = 0; a RESUME path that is empty, longer
 * than seq_cap, names a vertex >= n_pos or has more vertices outside [in_lo, in_hi) than set_size - 1; a set_size that is no
 * power of two or below 8; overlapping output ranges.
 * Termination needs no guard of its own: every vertex a walk or a probe appends is marked first and a marked vertex is never
 * accepted again, every append to the sequence is bounded by seq_cap and every probe by its share of the arena (both end the
 * job with overflow set), and a hash set is never searched without an empty entry — the load-factor tests end the job before
 * (n_out * 2 > tmask, (po.n + 1) * 2 > pmask, with tmask = pmask), which the limit on a RESUME path extends to its take-over. */
#define PAG_DEBUG_WALK_GUARD 16
typedef struct pag_debug_walk_contig {
    uint32_t ctg_left, ctg_right, rev_left, rev_right;
    uint64_t split_size;
    double leap_min;
    uint32_t n_ctgs, in_lo, in_hi, g_lo, g_hi, gmask, gwin_lo, gwin_hi;
    const uint64_t *starts; /* [n_ctgs + 1] */
    const uint64_t *sizes;  /* [n_ctgs] */
    const uint32_t *gbits;  /* [n_gbits] or NULL */
    const uint32_t *gset;   /* [gmask + 1] or NULL */
    uint64_t n_gbits;
} pag_debug_walk_contig;
typedef struct pag_debug_walk_job {
    uint64_t has_size, seq_cap, init_len, set_size, out_off;
    uint32_t ctg, start, exact, mode, stop_pc, win_low;
} pag_debug_walk_job;
typedef struct pag_debug_walk_out {
    uint64_t seq_len, seq_size, n_classify, n_probe, n_records, n_fill, n_out, n_main, max_probe;
    uint32_t last_ctg, overflow, stopped, max_back, max_chosen, wd_below_max, wd_forced_min, poison;
} pag_debug_walk_out;
int pag_debug_walk(const pag_debug_trav_graph *g, const pag_debug_walk_contig *ctgs, uint32_t n_ctgs, const pag_debug_walk_job *jobs,
                   uint32_t n_jobs, uint32_t *seq_v, uint32_t *seq_s, uint64_t *seq_x, uint64_t n_seq, pag_debug_walk_out *outs, int device);
/* the walker's geometry as built (make WALK_WINDOW=...): out[9] = LIST_CAP, BR_CAP, PB_CAP, PROBE_GROUPS, WIN_IDS, WIN_REC, WIN_BACK,
 * WIN_AHEAD, FILT_WORDS.  No device is touched. */
int pag_debug_walk_geometry(uint32_t *out, uint32_t n);

/* ---- libpagraph_host.so ---- */
/* one record's column classes / one sequence packed, by the production path or by the scalar loop alone */
void pagh_debug_classify_columns(const char *q, uint64_t n, const char *r, uint64_t rn, uint32_t *words, uint32_t *n_emit,
                                 uint32_t *n_radv, int scalar_only);
void pagh_debug_pack_bases(const char *sq, uint64_t n, uint8_t *out, int scalar_only);

#ifdef __cplusplus
}
#endif
#endif /* PAGRAPH_DEBUG_H */
