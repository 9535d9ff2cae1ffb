// pool_slots.hpp — the registry of the handle's device pool (pag_graph::pool, pag_graph_impl.hpp): every slot by name, grouped
// by the stage that owns it, in the order a block passes through them.  Plain C++.  This file is the ONLY place that knows the
// layout: a stage names its buffers (DevBuf(g, ps::TK0)), never numbers them, and the values themselves mean nothing outside
// this file.  Two stages that use the same name share the buffer on purpose; the sharings are listed at the entries
// (DESIGN.md 2 has the summary).
#pragma once

namespace pagdev {
namespace ps {

// ---- indexed families: "the same buffers, i-th copy".  A family's members are laid out behind its base entry; family() is
// the only arithmetic on slot ids.
// the buffers of prepare_read_db (k_prepare.hip), once per read database (read -> contig, read -> reference)
enum PrepDbBuf {
    DB_REC,                // the database's raw records (uploaded)
    DB_K0, DB_V0,          // sort pair (query, record index), and
    DB_K1, DB_V1,          //   its ping-pong partner
    DB_TMP,                // sort / scan scratch
    DB_OFF,                // per read: offset of its list (prep_offsets)
    DB_LONG,               // counter + the reads whose list is too long for the device sort (the host sorts those)
    DB_ALNT,               // pag_aln records of the listed alignments before compaction (prep_pass1 / prep_pass2)
    DB_KEEP,               // their keep flags
    DB_POS,                // scan of the keep flags
    DB_ALN,                // OUTPUT: the compacted pag_aln records (+ pass 2's coverage-only records), read by extract_stage
    DB_QOFF,               // OUTPUT: query_off per read
    DB_INL,                // pass 2, per raw record: it is in its read's list
    DB_POS2,               // pass 2: scan of the coverage-only flags
    PREP_DB_BUFS
};
constexpr int PREP_DBS = 2;
// the seven arrays of a graph in slice layout (pag_shard_slice): the tuple stream with its segment results, then the edge stream
enum GraphArr { G_TKEY, G_TVAL, G_TSEG, G_TCNT, G_EKEY, G_EVAL, G_ESEG, GRAPH_ARRS };
constexpr int GRAPH_TUPLE_ARRS = 4;                             // the first four are per tuple, the rest per edge
constexpr int GRAPH_ESZ[GRAPH_ARRS] = {4, 8, 4, 2, 4, 8, 4};  // bytes per element
constexpr int STREAM_ESZ[4] = {4, 8, 4, 8};                    // ... of a stream pair: tkey tval ekey eval

enum Id : int {
    // ---- preparation (pag_prepare, k_prepare.hip): raw alignments -> pag_build_input.  What it hands to pag_process stays
    // valid until the next pag_prepare.
    PREP_ROFF, PREP_RLEN, PREP_PACKED,     // reads: byte offsets, lengths, packed bases (uploaded unless the bulk is on the device)
    PREP_D1, PREP_D2, PREP_D3,             // difference words of read -> contig, read -> reference, contig -> reference (likewise)
    PREP_CLEN, PREP_CSEL, PREP_CFWD,       // contigs: length, selected, forward (uploaded)
    PREP_RFLEN, PREP_RACC,                 // references: length, accepted (uploaded)
    PREP_CTAB, PREP_RTAB,                  // OUTPUT: pag_ctg / pag_ref tables
    PREP_ORDER,                            // OUTPUT: emission order of the reads (prep_emit_order)
    PREP_ERR,                              // error flags of the stage's kernels
    PREP_JOBS, PREP_CFIRST, PREP_PRE,      // contig map: jobs, first chunk of each, per-chunk prefix (ctgmap_chunks)
    PREP_CNT, PREP_MULTI, PREP_ISEND,      // contig map: per-base counts then cursors, per-contig multi flag, end-of-contig marks
    PREP_RUN, PREP_SCAN, PREP_STMP,        // contig map: run lengths, their scan, scan scratch
    PREP_EOFF, PREP_ENT,                   // OUTPUT: ctg_ent_off, ctg_ent
    PREP_ENDS,                             // end slots of the selected contigs (uploaded)
    PREP_DB,                               // family PrepDbBuf x PREP_DBS
    PREP_DB_LAST = PREP_DB + PREP_DBS * PREP_DB_BUFS - 1,

    // ---- extraction inputs (extract_stage, pag_api.hip): staging of a host-resident pag_build_input; idle when the input is
    // on the device (pag_prepare's)
    IN_ROFF, IN_RLEN, IN_PACKED, IN_ORDER,  // reads and emission order
    IN_ALN1, IN_Q1, IN_D1,                  // read -> contig database: records, query_off, difference words
    IN_ALN2, IN_Q2, IN_D2,                  // read -> reference database
    IN_CTG, IN_EOFF, IN_ENT, IN_REF,        // contig table, contig map offsets and entries, reference table

    // ---- coverage filter and column index (extract_stage)
    COV_OK, COV_TMP,                        // pass 2's per-alignment verdict (launch_cov_filter) and its scratch
    CI_CC,                                  // column chunks per alignment (chunk_counts)
    CI_OFF1, CI_OFF2,                       // scan of it per database
    CI_1, CI_2,                             // the column index per database (launch_colidx)
    X_SCAN, X_TOT,                          // scan scratch and the totals the host reads back (both also K1's)

    // ---- K1 (extract_stage)
    K1_PTMP, K1_PERM,                       // the order pass 0's jobs run in: sort scratch, permutation (launch_exec_perm)
    K1_JS, K1_JT, K1_JE,                    // per job: samples, tuples, edges
    K1_TOFF, K1_EOFF,                       // scans of the last two: where each job emits
    K1_PK0, K1_PV0, K1_PK1, K1_PV1,         // sort pairs of launch_exec_perm
    SOLID_MASK,                             // per-read solid k-mer mask (launch_solid_mask; unused when every k-mer is solid)

    // ---- the extraction streams, their ping-pong partners, the sort scratch (StreamBufs, pag_api.hip).
    // TK0/TV0 (tuples) and EK0/EV0 (edges) are written by extract_stage in canonical order [pass 1] ++ [pass 2], or filled by
    // pag_shard_build with what the owner was sent; read by build_stage, keep_debug_streams, pag_shard_extract_range and, through
    // streams_at(), by pag_shard_take / pag_shard_take_part / the chunk sends of shard_comm.hip.  The partners and the sort
    // scratch are shared between build_stage (K2) and pag_shard_extract_range (the owner partition); the finished graph's
    // tkey/tval/ekey/eval point at whichever side of a pair the sort ended on.  The value partners hold 12 bytes per record: they
    // double as the segment kernels' scratch.
    TK0, TV0, TK1, TV1,
    EK0, EV0, EK1, EV1,
    SORT_TMP,

    // ---- segment scratch and results (build_stage: K3 / K4)
    T_SCR, E_SCR,                           // scratch of the segment kernels when the sort ended in the big value buffer
    T_SEG, T_CNT, E_SEG,                    // RESULTS: the finished graph's tseg, tcnt, eseg
    SEG_LONG, SEG_LCNT,                     // list of the long segments and its counter
    CTR,                                    // counters: K3 / K4 (build_stage, 128 bytes) and owner_counts (pag_shard_extract_range, 512)

    // ---- imported graph (family GraphArr): filled by pag_shard_import, or received in place by shard_comm.hip and taken over by
    // pag_shard_adopt.  Slots of its own because the imported parts may be the handle's own slice.  Kept by pag_shard_release_build.
    IMPORT,
    IMPORT_LAST = IMPORT + GRAPH_ARRS - 1,

    // ---- traversal graph (trav_prepare_graph, trav_prepare_host.hpp): built once per graph, kept in g->tg
    TG_NCODE, TG_NPOS, TG_NEDGE,            // nodes: k-mer code, offsets of their vertices and edges
    TG_VPOS, TG_VCNT, TG_VNODE,             // vertices: coordinates, counts, node
    TG_ETO, TG_ESTEP,                       // edges: target node, step
    TG_BITMAP, TG_RANK,                     // 4^k-bit node bitmap and its rank directory
    TG_CTMP,                                // scratch of trav_compact; afterwards b_heavy views it (vertices done by a wave each + emit counters)
    TG_UOLD, TG_NEWID, TG_UPOS, TG_UCNT,    // vertices in coordinate order: old id, new id of old, coordinates, counts
    TG_SOFF, TG_SUCC,                       // successor records: offsets, records
    TG_OK0, TG_OV0, TG_OK1, TG_OV1, TG_OTMP,  // sort pairs and scratch of the coordinate order and the emission stream, unless
                                              // on loan from the build (LENDABLE below)
    TG_INC, TG_INC_TMP,                     // incomplete-vertex bitmap of a regional / cut graph and its scratch (trav_mark_incomplete)
    TG_VIEW, TG_VIEW_IV,                    // the view: zone-band scratch (trav_view_region), interval tables (trav_compact reads them)

    // ---- walk session (WalkSession, walk_session_*.hpp): one pag_travel
    WALK_PACKED, WALK_NODES,                // contigs' packed bases, per-strand node tables
    WALK_STARTS, WALK_SIZES,                // PositionMapper tables
    WALK_TC,                                // TravContig per walked strand
    WALK_SEEDOUT, WALK_REQ,                 // seed searches: results, requests
    WALK_GSET, WALK_GBITS,                  // per-contig global visited structures
    WALK_GATHER, WALK_VIDS,                 // vertex / path attributes gathered for the host, the ids asked for
    WALK_CJ,                                // jobs of the node-table launch (setup_contigs)
    WALK_CKREQ, WALK_CKOUT,                 // checkpoint and id-bound queries and their answers
    WALK_FIN,                               // the epilogue's undelivered paths (ids, steps)
    WALK_SEQS,                              // PAG_TRAVEL_RENDER_SEQS: the packed contigs and references with their byte offsets (k5_seq.hip SeqSources)

    // ---- selection (pag_shard_select, k_select.hip): a selection lives here until the next one
    SEL_CIV, SEL_RIV,                       // the region's contig intervals and reference bands (uploaded)
    SEL_KEEP, SEL_POS,                      // keep flags and their scan
    SEL_CODES,                              // bitmap of the k-mers that keep a vertex
    SEL_TMP, SEL_CNT,                       // scan scratch, node counter
    SEL_OUT,                                // family GraphArr: the selected slice
    SEL_OUT_LAST = SEL_OUT + GRAPH_ARRS - 1,

    // ---- the sharded run (shard_comm.hip)
    OWN_TK, OWN_TV, OWN_EK, OWN_EV,         // owner layout: the received chunks in canonical order (pag_shard_build copies them to TK0 ..)
    SEND,                                   // family GraphArr: the selections of all destinations, one behind the other
    SEND_LAST = SEND + GRAPH_ARRS - 1,

    // ---- one owner's records out of an extraction (pag_shard_extract_for, k_owner_pick.hip): tile counters, their scans, scan scratch
    PICK_TMP,

    COUNT
};

constexpr Id family(Id base, int i) { return (Id)((int)base + i); }
constexpr Id prep_db(int db, PrepDbBuf b) { return family(PREP_DB, db * PREP_DB_BUFS + b); }  // database db's copy of a PrepDbBuf
static_assert(PREP_DB_LAST + 1 == IN_ROFF && IMPORT_LAST + 1 == TG_NCODE && SEL_OUT_LAST + 1 == OWN_TK && SEND_LAST + 1 == PICK_TMP,
              "a family's members lie between its base and the next entry");

// pag_shard_release_build hands back everything but the imported graph and the traversal's (graph and session) slots
constexpr bool released_after_import(Id s) { return s < IMPORT || s > WALK_SEQS; }

// Build buffers the traversal graph's sorts may BORROW (Lender, trav_prepare_graph): between two pag_process calls they are
// idle unless the finished graph points into them.  A loan never grows a slot; ties go to the earlier entry.
constexpr Id LENDABLE[] = {TK0, TV0, TK1, TV1, EK0, EV0, EK1, EV1, SORT_TMP, T_SCR, E_SCR};

}  // namespace ps
}  // namespace pagdev
