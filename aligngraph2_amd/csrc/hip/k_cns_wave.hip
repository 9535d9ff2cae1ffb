// k_cns_wave.hip — pa_cns's graph stage on the device with the LANES of a wavefront on the parallel parts of a part's work
// (PA_CNS_BACKEND=wave, pag_cns_consensus_wave).  One wavefront per part as in k_cns.hip, on the same regions and layout
// (cns_graph.hpp: Arrays / Part, doubly linked in / out lists, the same caps), with the same results to the byte — and the
// same node and edge numbers, so a difference is a comparison of arrays:
//   * init_backbone: lanes over the backbone positions, nodes and edges numbered as the serial loops number them.
//   * add_aln: the alignments in their order; inside one, the columns 64 at a time.  Ballots give each column its backbone
//     position, the id of its insertion vertex (n_nodes + the insertions before it) and its `prev` (the last match or
//     insertion column before it, carried across chunks); each lane then does its own add_edge, new edge slots numbered by a
//     ballot in column order.  Exact because inside one alignment every `cur` is distinct and every `prev` is distinct (the
//     backbone positions rise, insertion vertices are new): no two lanes touch one list or one node, a list gets at most one
//     append per alignment (so its order is the serial one), and nothing is freed before mergeNodes (free_head == NONE, so
//     the slots are the serial ones).  An alignment that leaves its part's backbone (a match or deletion at position 0 or at
//     the exit vertex and beyond, which the serial code tolerates until it overruns) goes on serially from that chunk.  The
//     first failing column decides the error code, as in the serial loop.
//   * mergeNodes: its control depends on order (the BFS queue, the capture stack, the recursion into the surviving node);
//     lane 0 runs cns_graph.hpp's merge_nodes.
//   * bestPath: a node's score depends only on its out-neighbours' scores, and the serial FIFO is the levels of Kahn's
//     algorithm from the exit vertex one after another, so the levels are taken in turn with a lane per node (a count of
//     unvisited out-edges per node in the aux region).  A node keeps the FIRST best out-edge in list order; the float
//     expression is the serial one (HIPFLAGS: -ffp-contract=off).  Where the level form could part from the queue (a queue
//     the serial loop could overflow, an exit vertex with out-edges, which the serial loop would take twice) lane 0 runs the
//     serial best_path.  The walk along the best edges and the trimming are O(part length): lane 0.
#include "cns_device.hpp"

namespace pagdev {
namespace {

using namespace pagcns;

enum : uint32_t { K_NONE = 0, K_MATCH = 1, K_DEL = 2, K_INS = 3, K_EXIT = 4 };

__device__ inline uint32_t popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
__device__ inline uint32_t highest_lane(uint64_t m) { return 63u - (uint32_t)__builtin_clzll(m); }  // m != 0

// after code that lane 0 ran alone: the wave-uniform state of the graph from lane 0
__device__ inline void take_lane0(Graph &g) {
    __syncthreads();
    g.n_nodes = __shfl(g.n_nodes, 0);
    g.n_edges_hi = __shfl(g.n_edges_hi, 0);
    g.free_head = __shfl(g.free_head, 0);
    g.err = __shfl(g.err, 0);
}

// AlnGraphBoost(backbone): blen + 2 nodes, then the edges i -> i + 1 in slots 0 .. blen
__device__ void wave_init_backbone(Graph &g, const char *bb, uint32_t blen, uint32_t lane) {
    if ((uint64_t)blen + 2 > g.node_cap) {  // (the serial loops create the nodes first: the first region too small is the error)
        g.err = CNS_E_NODES;
        return;
    }
    if ((uint64_t)blen + 1 > g.edge_cap) {
        g.err = CNS_E_EDGES;
        return;
    }
    const uint32_t exit_ = blen + 1;
    for (uint32_t v = lane; v <= exit_; v += PAG_WAVE) {
        const bool inner = v != 0 && v != exit_;
        g.nb[v] = v == 0 ? (uint8_t)'^' : v == exit_ ? (uint8_t)'$' : (uint8_t)bb[v - 1];
        g.nf[v] = 1;
        g.ncov[v] = 0;
        g.nw[v] = inner ? 1 : 0;
        g.nbb[v] = inner ? v : 0;
        g.noh[v] = g.not_[v] = v != exit_ ? v : NONE;
        g.noc[v] = v != exit_ ? 1u : 0u;
        g.nih[v] = g.nit[v] = v != 0 ? v - 1 : NONE;
        g.nic[v] = v != 0 ? 1u : 0u;
    }
    for (uint32_t e = lane; e < exit_; e += PAG_WAVE) {
        g.es[e] = e;
        g.ed[e] = e + 1;
        g.ec[e] = 0;
        g.ev[e] = 0;
        g.eon[e] = g.eop[e] = g.ein[e] = g.eip[e] = NONE;
    }
    g.n_nodes = exit_ + 1;
    g.n_edges_hi = exit_;
    g.enter = 0;
    g.exit_ = exit_;
    __syncthreads();
}

// add_edge's search: every edge u -> v gains w (the in-edges of v from u are the out-edges of u to v: the shorter list is
// walked); whether there was one
__device__ bool add_weight(Graph &g, uint32_t u, uint32_t v, int w) {
    bool exists = false;
    if (g.noc[u] <= g.nic[v]) {
        for (uint32_t e = g.noh[u]; e != NONE; e = g.eon[e])
            if (g.ed[e] == v) {
                g.ec[e] += w;
                exists = true;
            }
    } else {
        for (uint32_t e = g.nih[v]; e != NONE; e = g.ein[e])
            if (g.es[e] == u) {
                g.ec[e] += w;
                exists = true;
            }
    }
    return exists;
}

// add_edge_raw's appends for the slot e the serial allocation hands out at this column, and add_edge's weight
__device__ void link_edge(Graph &g, uint32_t e, uint32_t u, uint32_t v, int w) {
    g.es[e] = u;
    g.ed[e] = v;
    g.ec[e] = w;
    g.ev[e] = 0;
    g.eon[e] = NONE;
    const uint32_t ot = g.not_[u];
    g.eop[e] = ot;
    if (ot != NONE) g.eon[ot] = e;
    else g.noh[u] = e;
    g.not_[u] = e;
    g.noc[u] += 1;
    g.ein[e] = NONE;
    const uint32_t it = g.nit[v];
    g.eip[e] = it;
    if (it != NONE) g.ein[it] = e;
    else g.nih[v] = e;
    g.nit[v] = e;
    g.nic[v] += 1;
}

// addAln (:64-113), the columns 64 at a time; column `len` is the closing edge to the exit vertex
__device__ void wave_add_aln(Graph &g, const char *q, const char *t, uint32_t len, uint32_t start, int weight, uint32_t lane) {
    if (weight <= 0) return;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t bb_pos = start, prev = g.enter;
    for (uint32_t c0 = 0; c0 <= len; c0 += PAG_WAVE) {
        const uint32_t i = c0 + lane;
        uint32_t kind = K_NONE;
        uint8_t qb = 0, tb = 0;
        if (i < len) {
            qb = (uint8_t)q[i];
            tb = (uint8_t)t[i];
            kind = qb == tb ? K_MATCH : (qb == '-' && tb != '-') ? K_DEL : (qb != '-' && tb == '-') ? K_INS : K_NONE;
        } else if (i == len) {
            kind = K_EXIT;
        }
        const bool on_bb = kind == K_MATCH || kind == K_DEL;
        const uint64_t m_pos = __ballot(on_bb);                            // columns that advance the backbone position
        const uint64_t m_ins = __ballot(kind == K_INS);                    // columns that create a vertex
        const uint64_t m_vtx = __ballot(kind == K_MATCH || kind == K_INS); // columns that become the next column's prev
        const uint32_t pos = bb_pos + popc(m_pos & below);
        const uint32_t nv = g.n_nodes + popc(m_ins & below);
        if (__ballot(on_bb && (pos == 0 || pos >= g.exit_))) {
            // off the part's backbone: the lists of two columns may coincide; the serial loop from this chunk on
            if (lane == 0) add_aln_from(g, q, t, c0, len, bb_pos, prev, weight);
            take_lane0(g);
            return;
        }
        const uint32_t cur = kind == K_INS ? nv : kind == K_EXIT ? g.exit_ : pos;
        const uint64_t m_prev = m_vtx & below;
        const uint32_t from = __shfl(cur, (int)(m_prev ? highest_lane(m_prev) : lane));
        const uint32_t pv = m_prev ? from : prev;
        // an existing edge gains the weight; a vertex created in this chunk has no out-edges yet
        bool fresh = kind == K_INS;
        if (kind == K_MATCH || kind == K_EXIT) fresh = pv >= g.n_nodes || !add_weight(g, pv, cur, weight);
        const uint64_t m_fresh = __ballot(fresh);
        const uint32_t e = g.n_edges_hi + popc(m_fresh & below);
        int fail = CNS_OK;
        if (kind == K_INS && nv >= g.node_cap) fail = CNS_E_NODES;
        else if (fresh && e >= g.edge_cap) fail = CNS_E_EDGES;
        const uint64_t m_fail = __ballot(fail != CNS_OK);
        if (m_fail) {  // the first failing column is the serial loop's error (the part's graph is given up)
            g.err = __shfl(fail, (int)__builtin_ctzll(m_fail));
            return;
        }
        if (on_bb) {
            const uint32_t bbv = g.nbb[pos];
            g.ncov[bbv] += weight;
            g.nb[bbv] = tb;
            if (kind == K_MATCH) g.nw[pos] += weight;
        } else if (kind == K_INS) {
            g.nb[nv] = qb;
            g.nf[nv] = 0;
            g.ncov[nv] = 0;
            g.nw[nv] = weight;
            g.nbb[nv] = pos;
            g.noh[nv] = g.not_[nv] = g.nih[nv] = g.nit[nv] = NONE;
            g.noc[nv] = g.nic[nv] = 0;
        }
        __syncthreads();  // the chunk's vertices exist before edges are linked to them
        if (fresh) link_edge(g, e, pv, cur, weight);
        __syncthreads();
        g.n_nodes += popc(m_ins);
        g.n_edges_hi += popc(m_fresh);
        bb_pos += popc(m_pos);
        const uint32_t last = __shfl(cur, (int)(m_vtx ? highest_lane(m_vtx) : 0));
        if (m_vtx) prev = last;
    }
}

// bestPath (:383-467) level by level, then the walk and the trimming (:293-333) on lane 0
__device__ void wave_consensus(Graph &g, int min_weight, char *out, uint32_t out_cap, uint32_t *out_len, uint32_t lane, uint32_t *s_tail) {
    const uint32_t nn = g.n_nodes;
    // the levels need a queue the serial loop cannot overflow (a node is queued once: q_cap > nn) — it then also holds the
    // counts and the levels — and an exit vertex without out-edges
    if (g.q_cap <= nn || g.noc[g.exit_] != 0) {
        if (lane == 0) best_path(g);
        take_lane0(g);
    } else {
        uint32_t *cnt = g.queue, *lvl = g.queue + nn;
        for (uint32_t e = lane; e < g.n_edges_hi; e += PAG_WAVE) g.ev[e] = 0;
        for (uint32_t v = lane; v < nn; v += PAG_WAVE) {
            g.nbest[v] = -1;
            g.nscore[v] = 0.0f;
            cnt[v] = g.noc[v];
        }
        if (lane == 0) {
            lvl[0] = g.exit_;
            *s_tail = 1;
        }
        __syncthreads();
        bool overrun = false;
        for (uint32_t lo = 0, hi = 1; lo < hi;) {
            for (uint32_t k = lo + lane; k < hi; k += PAG_WAVE) {  // a level's nodes: their out-neighbours are all scored
                const uint32_t n = lvl[k];
                float best_score = -3.402823466e+38f;  // -FLT_MAX
                int best_edge = -1;
                for (uint32_t oe = g.noh[n]; oe != NONE; oe = g.eon[oe]) {
                    const uint32_t od = g.ed[oe];
                    float new_score;
                    const float score = g.nscore[od];
                    if ((g.nf[od] & 1u) && g.nw[od] == 1) {
                        new_score = score - 10.0f;
                    } else {
                        const uint32_t bbv = g.nbb[od];
                        if (bbv >= nn) {
                            overrun = true;
                            break;
                        }
                        new_score = (float)g.ec[oe] - (float)g.ncov[bbv] * 0.5f + score;
                    }
                    if (new_score > best_score) {
                        best_score = new_score;
                        best_edge = (int)oe;
                    }
                }
                if (best_edge >= 0) {
                    g.nscore[n] = best_score;
                    g.nbest[n] = best_edge;
                }
            }
            if (__ballot(overrun)) break;  // (the serial loop meets it too: it visits the same nodes)
            for (uint32_t k = lo + lane; k < hi; k += PAG_WAVE) {  // their in-edges visited: a source with none left joins the next level
                const uint32_t n = lvl[k];
                for (uint32_t ie = g.nih[n]; ie != NONE; ie = g.ein[ie]) {
                    g.ev[ie] = 1;
                    const uint32_t s = g.es[ie];
                    if (atomicSub(&cnt[s], 1u) == 1u) lvl[atomicAdd(s_tail, 1u)] = s;
                }
            }
            __syncthreads();
            lo = hi;
            hi = *s_tail;
        }
        if (__ballot(overrun)) g.err = CNS_E_OVERRUN;
    }
    if (g.err) return;
    if (lane == 0) trim_path(g, min_weight, out, out_cap, out_len);
    take_lane0(g);
}

}  // namespace

__global__ __launch_bounds__(64) void cns_parts_wave_kernel(Arrays A, const Part *__restrict__ parts, uint32_t n_parts, const char *__restrict__ backbone,
                                                             const Aln *__restrict__ alns, const char *__restrict__ qpool, const char *__restrict__ tpool,
                                                             int min_weight, char *__restrict__ out, uint32_t *__restrict__ out_len, int32_t *__restrict__ part_err) {
    __shared__ uint32_t s_tail;
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    if (p >= n_parts) return;
    const Part P = parts[p];
    Graph g;
    bind(g, A, P);
    wave_init_backbone(g, backbone + P.bb_off, P.bb_len, lane);
    for (uint32_t a = 0; a < P.n_aln && !g.err; ++a) {
        const Aln al = alns[P.aln_first + a];
        wave_add_aln(g, qpool + al.str_off, tpool + al.str_off, al.len, al.start, al.weight, lane);
    }
    if (!g.err) {
        if (lane == 0) merge_nodes(g);
        take_lane0(g);
    }
    uint32_t len = 0;
    if (!g.err) wave_consensus(g, min_weight, out + P.out_off, P.out_cap, &len, lane, &s_tail);
    if (lane == 0) {
        out_len[p] = g.err ? 0u : len;
        part_err[p] = g.err;
    }
}

static void launch_wave(const pagcns::Arrays &A, const pagcns::Part *parts, uint32_t n, const char *backbone, const pagcns::Aln *alns, const char *qpool,
                        const char *tpool, int min_weight, char *out, uint32_t *out_len, int32_t *part_err) {
    cns_parts_wave_kernel<<<dim3(n), dim3(PAG_WAVE), 0, 0>>>(A, parts, n, backbone, alns, qpool, tpool, min_weight, out, out_len, part_err);
}

CnsLaunchFn cns_launcher_wave() { return launch_wave; }

}  // namespace pagdev

extern "C" int pag_cns_consensus_wave(int device, const char *backbone, uint64_t backbone_len, const pag_cns_part *parts, uint64_t n_parts, const pag_cns_aln *alns,
                                      uint64_t n_alns, const char *qpool, const char *tpool, uint64_t pool_bytes, int32_t min_weight, char *out, uint64_t out_bytes,
                                      uint64_t *out_off, uint32_t *out_len, int32_t *part_err) {
    return pagdev::cns_consensus_batched("pag_cns_consensus_wave", pagdev::launch_wave, device, backbone, backbone_len, parts, n_parts, alns, n_alns, qpool, tpool,
                                         pool_bytes, min_weight, out, out_bytes, out_off, out_len, part_err);
}
