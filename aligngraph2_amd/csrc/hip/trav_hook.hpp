// What the test hooks on constructed graphs share (include/pagraph_debug.h; defined at the foot of k5_walk_aux.hip,
// k5_view.hip and k5_travel.hip): the upload of a pag_debug_trav_graph into a TravGraph, in the buffers of the hook's DevCall
// (dev_call.hpp).  Nothing in the product includes this.
#pragma once
#include <vector>

#include "dev_call.hpp"
#include "pag_device.hpp"
#include "pag_travel.hpp"
#include "pagraph_debug.h"

namespace pagdev {

// the arrays of g that are given, on the device; refuses a graph whose own indices point outside it
inline int hook_upload_graph(DevCall &D, const pag_debug_trav_graph *g, TravGraph *G) {
    if (!g || g->k < 1 || g->k > 16 || g->n_pos >= 0xFFFFFFF0ull || g->n_nodes >= 0xFFFFFFF0ull) return PAG_EINVAL;
    const uint64_t nn = g->n_nodes, np = g->n_pos;
    if (g->npos_off) {
        if (g->npos_off[0] != 0 || g->npos_off[nn] != np) return PAG_EINVAL;
        for (uint64_t i = 0; i < nn; ++i)
            if (g->npos_off[i] > g->npos_off[i + 1]) return PAG_EINVAL;
    }
    for (uint64_t i = 0; i < np; ++i)
        if ((g->vnode && g->vnode[i] >= nn) || (g->uold && g->uold[i] >= np) || (g->newid && g->newid[i] >= np)) return PAG_EINVAL;
    *G = TravGraph{};
    G->n_nodes = nn;
    G->n_pos = np;
    int rc;
    if (g->ncode && (rc = D.up(g->ncode, nn, &G->ncode))) return rc;
    if (g->npos_off && (rc = D.up(g->npos_off, nn + 1, &G->npos_off))) return rc;
    if (g->vpos && (rc = D.up(g->vpos, np, &G->vpos))) return rc;
    if (g->vcnt && (rc = D.up(g->vcnt, np, &G->vcnt))) return rc;
    if (g->vnode && (rc = D.up(g->vnode, np, &G->vnode))) return rc;
    if (g->uold && (rc = D.up(g->uold, np, &G->uold))) return rc;
    if (g->newid && (rc = D.up(g->newid, np, &G->newid))) return rc;
    if (g->upos && (rc = D.up(g->upos, np, &G->upos))) return rc;
    if (g->ucnt && (rc = D.up(g->ucnt, np, &G->ucnt))) return rc;
    const uint64_t n_words = ((1ull << (2 * g->k)) + 63) / 64;
    if (g->bitmap && (rc = D.up(g->bitmap, n_words, &G->bitmap))) return rc;
    if (g->rank && (rc = D.up(g->rank, n_words, &G->rank))) return rc;
    // the walker's arrays (pag_debug_walk checks the records against the graph before it comes here)
    if (g->succ_off && (rc = D.up(g->succ_off, np + 1, &G->succ_off))) return rc;
    if (g->succ && g->n_succ) {
        SuccRec *d = nullptr;
        if ((rc = D.up((const SuccRec *)g->succ, g->n_succ, &d))) return rc;
        G->succ = d;
        G->n_succ = g->n_succ;
    }
    if (g->incomplete) {
        uint32_t *d = nullptr;
        if ((rc = D.up(g->incomplete, (np + 31) / 32, &d))) return rc;
        G->incomplete = d;
    }
    return PAG_OK;
}

}  // namespace pagdev
