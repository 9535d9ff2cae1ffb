// shard_serial.hip — pag_shard_run_serial: ONE turn of a block built as N ranks that take turns on one device and one handle
// (include/pagraph_hip.h has the contract; aligngraph2_amd/rank_serial.py `run` is the Python prototype it restates).
//
//   turn 0 only:  counts[r][o] — one extraction per read range r, its records counted per owner (no partition)
//   for owner o (ascending):
//       for read range r:  extract r, o's records compacted into o's receive buffers       (pag_shard_extract_for; ps::OWN_*)
//       K2-K4 on them                                                                       (pag_shard_build)
//       pag_shard_select for the turn's region, appended to the import family               (ps::IMPORT)
//   the import family adopted as the handle's graph, the region set, the build's memory released
//
// One handle: an extraction begins with free_graph_results(), which clears the handle's POINTERS to its graph and nothing in
// the pool; no build stage touches the import family (pool_slots.hpp), so what owner o's selection left there is intact when
// owner o + 1 is extracted, built and selected.  Pool slots are reused from owner to owner; a slot of the import family grows by
// allocate-copy-free (its contents are the region so far) and keeps its size from turn to turn.
// Memory, the trade: the build's slots are released before the caller's traversal (they are what the traversal
// needs: ~70 GB at BASELINE configs[2]) and taken again in the next turn; the traversal's slots of the turn before are released
// when a turn begins (they would stand beside the build otherwise) — so a turn's peak is the prototype's, whose handles came and
// went, while the allocations of a turn are one set of build slots and one set of traversal slots, not one per owner.  The
// pinned path memory, the walk streams and the import family stay from turn to turn.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pag_graph_impl.hpp"
#include "pagraph_debug.h"
#include "serial_layout.hpp"

using namespace pagdev;

namespace {

// what the traversal of the turn before took: its slots (graph view, successor records, walk session) and the walk arena, which
// pag_travel sizes again from what is free once the build is released (as it did for the prototype's fresh handles)
void release_traversal(pag_graph *g) {
    hipStreamSynchronize(g->stream);
    g->tg_ready = false;
    for (int i = ps::TG_NCODE; i <= ps::WALK_SEQS; ++i) slot_free(g, g->pool[i]);
    g->walk_arena.release();
    g->walk_arena_used = 0;
}

// pag_shard_release_build that keeps the arrays of a device-resident input (pag_prepare's outputs live in the handle's pool;
// the next turn extracts from them again)
void release_build_keeping(pag_graph *g, const pag_build_input *in) {
    hipStreamSynchronize(g->stream);
    std::vector<const void *> keep;
    const GraphArrays held = arrays_of(*g);
    for (void *p : held.p) keep.push_back(p);
    if (in->on_device)
        for (const void *p : {(const void *)in->reads.byte_off, (const void *)in->reads.len, (const void *)in->reads.packed, (const void *)in->emit_order,
                              (const void *)in->read_to_ctg.aln, (const void *)in->read_to_ctg.query_off, (const void *)in->read_to_ctg.diff,
                              (const void *)in->read_to_ref.aln, (const void *)in->read_to_ref.query_off, (const void *)in->read_to_ref.diff,
                              (const void *)in->ctgs, (const void *)in->ctg_ent_off, (const void *)in->ctg_ent, (const void *)in->refs})
            keep.push_back(p);
    for (int i = 0; i < ps::COUNT; ++i) {
        pag_graph::Slot &sl = g->pool[i];
        if (!ps::released_after_import((ps::Id)i) || !sl.p) continue;
        const char *lo = (const char *)sl.p, *hi = lo + sl.cap;
        bool used = false;
        for (const void *p : keep) used = used || (p && (const char *)p >= lo && (const char *)p < hi);
        if (!used) slot_free(g, sl);
    }
}

bool same_count_lines(const pag_build_stats &a, const pag_build_stats &b) {
    return !std::memcmp(a.merge_edge, b.merge_edge, sizeof a.merge_edge) && !std::memcmp(a.total_pos, b.total_pos, sizeof a.total_pos) &&
           !std::memcmp(a.merge_pos, b.merge_pos, sizeof a.merge_pos) && !std::memcmp(a.n_tuples, b.n_tuples, sizeof a.n_tuples) &&
           !std::memcmp(a.n_edges, b.n_edges, sizeof a.n_edges);
}

int serial_turn(pag_graph *g, const pag_build_input *in, const pag_region *regions, uint32_t n, uint32_t turn, pag_build_stats *total,
                pag_serial_stats *st_out, bool via_partition) {
    if (!g || !in || !regions || (n != 2 && n != 4 && n != 8) || turn >= n) {
        set_error("pag_shard_run_serial: n_ranks must be 2, 4 or 8 (got %u) and the turn below it (got %u)", n, turn);
        return PAG_EINVAL;
    }
    pag_graph::SerialRun &S = g->serial;
    if (turn != 0 && (!S.valid || S.n != n)) {
        set_error("pag_shard_run_serial: turn %u of %u without a turn 0 of the same block on this handle before it", turn, n);
        return PAG_EINVAL;
    }
    PAG_HIP_TRY(hipSetDevice(g->device));
    const uint64_t n_reads = in->reads.n_seqs;
    auto range_lo = [&](uint32_t r) { return n_reads * r / n; };
    pag_serial_stats st{};
    int rc;
    const double alloc_ms0 = g->alloc_ms;
    const uint64_t alloc_calls0 = g->alloc_calls, alloc_bytes0 = g->alloc_bytes;
    const double t_turn = now_s();
    S.valid = false;  // (until this turn has passed its checks: a failed turn ends the block)
    if (turn != 0) release_traversal(g);

    // ---- turn 0: what every read range sends every owner
    double t0 = now_s();
    if (turn == 0) {
        S.n = n;
        S.counts.assign((size_t)n * n * 4, 0);
        S.total = pag_build_stats{};
        for (uint32_t r = 0; r < n; ++r)
            if ((rc = shard_count_range(g, in, range_lo(r), range_lo(r + 1), n, S.counts.data() + (size_t)r * n * 4))) return rc;
        st.s_extract += now_s() - t0;
    }

    // ---- owner after owner: its records from every range, K2-K4, the turn's part of its slice behind the region so far
    pag_build_stats tot{};
    uint64_t at_t = 0, at_e = 0;
    std::vector<uint64_t> full((size_t)4 * n);
    for (uint32_t o = 0; o < n; ++o) {
        t0 = now_s();
        const OwnerLayout L = owner_layout(S.counts.data(), n, n, o);
        DevBuf own_tk(g, ps::OWN_TK), own_tv(g, ps::OWN_TV), own_ek(g, ps::OWN_EK), own_ev(g, ps::OWN_EV);
        if ((rc = own_tk.alloc((L.n_t + 1) * 4)) || (rc = own_tv.alloc((L.n_t + 1) * 8)) || (rc = own_ek.alloc((L.n_e + 1) * 4)) ||
            (rc = own_ev.alloc((L.n_e + 1) * 8)))
            return rc;
        for (uint32_t r = 0; r < n; ++r) {
            const uint64_t *first = S.counts.data() + ((size_t)r * n + o) * 4;
            const RangeSlots at = range_slots(S.counts.data(), n, n, o, r);
            uint64_t c[4] = {0, 0, 0, 0};
            if (!via_partition) {
                if ((rc = pag_shard_extract_for(g, in, range_lo(r), range_lo(r + 1), n, o, own_tk.as<uint32_t>(), own_tv.as<uint64_t>(), L.n_t, at.t_at1,
                                                at.t_at2, own_ek.as<uint32_t>(), own_ev.as<uint64_t>(), L.n_e, at.e_at1, at.e_at2, c)))
                    return rc;
            } else {
                if ((rc = pag_shard_extract_range(g, in, range_lo(r), range_lo(r + 1), n, full.data()))) return rc;
                std::memcpy(c, full.data() + (size_t)o * 4, sizeof c);
                if (std::memcmp(c, first, sizeof c) == 0) {  // (else: reported below, nothing copied)
                    const RangeSlots from = partitioned_slots(full.data(), n, o, 0 /* full[] is this range's row */);
                    if ((rc = pag_shard_take_part(g, from.t_at1, c[0], own_tk.as<uint32_t>() + at.t_at1, own_tv.as<uint64_t>() + at.t_at1, from.e_at1, c[2],
                                                  own_ek.as<uint32_t>() + at.e_at1, own_ev.as<uint64_t>() + at.e_at1)) ||
                        (rc = pag_shard_take_part(g, from.t_at2, c[1], own_tk.as<uint32_t>() + at.t_at2, own_tv.as<uint64_t>() + at.t_at2, from.e_at2, c[3],
                                                  own_ek.as<uint32_t>() + at.e_at2, own_ev.as<uint64_t>() + at.e_at2)))
                        return rc;
                }
            }
            if (std::memcmp(c, first, sizeof c) != 0) {
                set_error("pag_shard_run_serial: read range %u is not reproducible: {%llu, %llu, %llu, %llu} records for owner %u in turn %u, "
                          "{%llu, %llu, %llu, %llu} when turn 0 counted them",
                          r, (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3], o, turn,
                          (unsigned long long)first[0], (unsigned long long)first[1], (unsigned long long)first[2], (unsigned long long)first[3]);
                return PAG_EFAULT;
            }
            st.tuples_in += c[0] + c[1];
            st.edges_in += c[2] + c[3];
        }
        const double t1 = now_s();
        pag_build_stats ost{};
        if ((rc = pag_shard_build(g, own_tk.as<uint32_t>(), own_tv.as<uint64_t>(), L.n_t, L.t1, own_ek.as<uint32_t>(), own_ev.as<uint64_t>(), L.n_e, L.e1,
                                  in->eps, &ost)))
            return rc;
        const double t2 = now_s();
        pag_shard_slice sel{};
        if ((rc = pag_shard_select(g, &regions[turn], &sel))) return rc;
        const double t3 = now_s();
        // behind the region so far (owner order = ascending k-mer ranges).  A slot that has to grow is sized for the owners to
        // come as well: k-mer ranges of equal width hold about as much each.
        const GraphArrays from = arrays_of(sel);
        for (int a = 0; a < ps::GRAPH_ARRS; ++a) {
            const bool tup = a < ps::GRAPH_TUPLE_ARRS;
            const size_t esz = (size_t)ps::GRAPH_ESZ[a], have = (size_t)(tup ? at_t : at_e) * esz, add = (size_t)(tup ? sel.n_t : sel.n_e) * esz;
            const size_t need = have + add + esz;
            const size_t guess = (have + add) / (o + 1) * n;
            DevBuf imp(g, ps::family(ps::IMPORT, a));
            if ((rc = imp.alloc_keeping(need, have, std::max(need, guess + guess / 16) + 256))) return rc;
            if (add) PAG_HIP_TRY(hipMemcpyAsync((char *)imp.p + have, from.p[a], add, hipMemcpyDeviceToDevice, g->stream));
            st.region_bytes += add;
        }
        PAG_HIP_TRY(hipStreamSynchronize(g->stream));
        at_t += sel.n_t;
        at_e += sel.n_e;
        add_stats(tot, sel.stats);
        st.s_extract += t1 - t0;
        st.s_build += t2 - t1;
        st.s_select += t3 - t2;
        st.s_import += now_s() - t3;
    }

    // ---- the count lines are sums over the owners: the same in every turn
    if (turn == 0) {
        S.total = tot;
    } else if (!same_count_lines(tot, S.total)) {
        set_error("pag_shard_run_serial: the count lines of turn %u {%llu %llu %llu | %llu %llu %llu} differ from those of turn 0 {%llu %llu %llu | %llu %llu %llu}",
                  turn, (unsigned long long)tot.merge_edge[0], (unsigned long long)tot.total_pos[0], (unsigned long long)tot.merge_pos[0],
                  (unsigned long long)tot.merge_edge[1], (unsigned long long)tot.total_pos[1], (unsigned long long)tot.merge_pos[1],
                  (unsigned long long)S.total.merge_edge[0], (unsigned long long)S.total.total_pos[0], (unsigned long long)S.total.merge_pos[0],
                  (unsigned long long)S.total.merge_edge[1], (unsigned long long)S.total.total_pos[1], (unsigned long long)S.total.merge_pos[1]);
        return PAG_EFAULT;
    }

    // ---- the region becomes the handle's graph; the build's memory goes back
    t0 = now_s();
    if ((rc = pag_shard_adopt(g, at_t, at_e, &tot))) return rc;
    if ((rc = pag_shard_set_region(g, &regions[turn]))) return rc;
    release_build_keeping(g, in);
    st.s_import += now_s() - t0;
    st.held_vertices = g->stats.n_pos;
    st.held_edges = g->stats.n_uniq_edges;
    S.valid = true;
    if (env_timing())
        fprintf(stderr,
                "[timing] pag_shard_run_serial turn %u/%u: %.3f s (extract %.3f, build %.3f, select %.3f, import + release %.3f), of which %.3f s in %llu "
                "hipMalloc of pool slots (%.1f GB)\n",
                turn, n, now_s() - t_turn, st.s_extract, st.s_build, st.s_select, st.s_import, (g->alloc_ms - alloc_ms0) / 1e3,
                (unsigned long long)(g->alloc_calls - alloc_calls0), (double)(g->alloc_bytes - alloc_bytes0) / 1e9);
    if (total) *total = tot;
    if (st_out) *st_out = st;
    return PAG_OK;
}

}  // namespace

extern "C" int pag_shard_run_serial(pag_graph *g, const pag_build_input *in, const pag_region *regions, uint32_t n_ranks, uint32_t turn,
                                    pag_build_stats *total, pag_serial_stats *st) {
    return serial_turn(g, in, regions, n_ranks, turn, total, st, false);
}

extern "C" int pag_debug_shard_run_serial(pag_graph *g, const pag_build_input *in, const pag_region *regions, uint32_t n_ranks, uint32_t turn,
                                          pag_build_stats *total, pag_serial_stats *st, int via_partition) {
    return serial_turn(g, in, regions, n_ranks, turn, total, st, via_partition != 0);
}
