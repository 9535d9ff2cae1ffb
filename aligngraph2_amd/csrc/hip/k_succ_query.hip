// k_succ_query.hip — pag_successors_batch: the successor lists of a LIST of vertices, evaluated on demand from the finished graph.
//
// PABruijnGraph::successors (PABruijnGraph.cpp:370-373 -> searchSuccessors :167-197) with the caller's deviation and error rate,
// for vertices named by (k-mer code, position), straight from the arrays pag_process / pag_shard_import leave in the handle —
// the k-mer-sorted tuple stream with its in-place segment results and the source-sorted edge stream (the layout pag_export_csr
// reads, pag_api.hip): no traversal view, no compact CSR, no records of anybody else's vertex.
//
// One wavefront per query, every wave on its own (no block barrier, no LDS).  A query is a chain of dependent loads from
// arrays of 10^8 entries, so the kernel is built to keep that chain short, with the toolbox of query_graph.hpp (steps 1 and 2
// are this kernel's own, 3 and 4 are SuccPairs, which k_walk_query.hip deals from as well):
//   1. the heads of the k-mer's tuple segment and of its edge segment, TOGETHER: lanes 0-31 search tkey, lanes 32-63 ekey, 32
//      pivots per round each (six rounds over the 4.5e8 tuples of BASELINE configs[1]; one lane's binary search is 29);
//   2. what stands at the two heads, requested together: the leader count tseg[head] and the first 64 leaders (one of them is
//      the query's position, or the graph holds no such vertex), the unique-edge count eseg[head] and the first 64 edges;
//   3. per 64 edges: target code and step one edge per lane; the targets' segment heads by groups of lanes, ALL edges at once:
//      with n edges the wave splits into groups of 64 / n lanes (a power of two), each group its own search with that many
//      pivots per round — one edge: 64 pivots, two: 32 each, ... 33 and more: one lane each, a binary search; then the
//      targets' leader counts, one load;
//   4. the candidate pairs (edge, leader of its target) flattened in edge order, then position order, and dealt to the lanes 64
//      at a time: a lane finds its pair's edge in the exclusive prefix sums of the leader counts (six shuffles), fetches that
//      lane's head and step (shuffles again), loads the leader's position and evaluates d_check_position — the f64 predicate,
//      whatever the error rate; a ballot and the count of the lower lanes give an accepted pair its place, so the list keeps
//      the reference's order (PABruijnGraph.cpp:182-195).
// The kernel runs twice: it counts, the counts are scanned into off[], it runs again and fills.  off[] and out[] are a function
// of the inputs alone (the two passes of a call: query_call.hpp).  The walker's "used" marks play no part: this is the
// reference's call on a fresh graph.
#include <algorithm>

#include "query_call.hpp"
#include "query_graph.hpp"

namespace pagdev {
namespace {

struct SuccOut {  // pag_succ
    uint32_t code, step;
    uint64_t pos;
    uint32_t grade, ctg_similar;
};
static_assert(sizeof(SuccOut) == sizeof(pag_succ), "pag_succ layout");

// FILL = false: cnt[i] = length of query i's list, status[i] = PAG_OK / PAG_EINVAL (no such vertex).  FILL = true: the records
// of query i to out[off[i] ..) (off: the scan of cnt; nothing is written at or beyond n_out)
template <bool FILL>
__global__ void __launch_bounds__(256) k_succ_query(QueryGraph G, const pag_succ_query *__restrict__ q, uint64_t n_q, uint32_t dev, double err,
                                                    uint32_t *__restrict__ cnt, int32_t *__restrict__ status, const uint64_t *__restrict__ off,
                                                    SuccOut *__restrict__ out, uint64_t n_out) {
    const uint32_t lane = lane_id(), waves = blockDim.x / 64u;
    const uint64_t n_waves = (uint64_t)gridDim.x * waves;
    for (uint64_t i = (uint64_t)blockIdx.x * waves + uniform_u32(threadIdx.x / 64u); i < n_q; i += n_waves) {
        const uint32_t code = q[i].code;
        const uint64_t pos = q[i].pos;
        uint64_t at = 0;
        if (FILL) {
            at = off[i];
            if (off[i + 1] == at) continue;  // (an empty list, a vertex the graph does not hold)
        }
        bool found = false;
        uint32_t n_rec = 0;
        // the k-mer's tuple segment (lanes 0-31 look for it) and its edge segment (lanes 32-63)
        const bool edge_half = lane >= 32u;
        const Bound hd = group_lower_bound(edge_half ? G.ekey : G.tkey, edge_half ? G.E : G.T, code, 32u, true);
        const uint64_t h = from_lane(hd.at, 0u), eh = from_lane(hd.at, 32u);
        const bool have_node = __shfl((int)hd.hit, 0) != 0, have_edges = __shfl((int)hd.hit, 32) != 0;
        if (have_node) {
            // leaders of the k-mer: the clustered positions, slots h .. h + nl - 1; its unique edges: slots eh .. eh + ne - 1
            const uint32_t nl = G.tseg[h];
            const uint32_t ne = have_edges ? G.eseg[eh] : 0u;
            const uint64_t first_pos = h + lane < G.T ? G.tval[h + lane] : 0ull;
            uint64_t ev = have_edges && eh + lane < G.E ? G.eval[eh + lane] : 0ull;
            found = __ballot(lane < nl && h + lane < G.T && first_pos == pos) != 0ull;
            for (uint32_t jb = 64u; jb < nl && !found; jb += 64u) {
                const uint64_t s = h + jb + lane;
                found = __ballot(jb + lane < nl && s < G.T && G.tval[s] == pos) != 0ull;
            }
            const uint32_t ac = (uint32_t)(pos >> 32), ar = (uint32_t)pos;
            for (uint32_t eb = 0; found && eb < ne; eb += 64u) {
                const uint32_t turn = ne - eb < 64u ? ne - eb : 64u;
                if (eb != 0u) ev = edge_turn(G, eh + eb, turn);  // (the first 64 came with the leaders)
                const SuccPairs P(G, ev, turn);
                for (uint64_t pb = 0; pb < P.n_pairs; pb += 64u) {
                    const SuccPairs::Pair p = P.pair(pb + lane);
                    int grade = G_OOPS;
                    uint32_t esim = 0;
                    if (p.live) grade = d_check_position(ac, ar, (uint32_t)(p.pos >> 32), (uint32_t)p.pos, p.step, dev, err, &esim);
                    const uint64_t taken = __ballot(grade != G_OOPS);
                    if (FILL && grade != G_OOPS) {
                        const uint64_t slot = at + n_rec + (uint32_t)__popcll(taken & lanemask_lt());
                        if (slot < n_out) {
                            SuccOut r;
                            r.code = p.code;
                            r.step = p.step;
                            r.pos = p.pos;
                            r.grade = (uint32_t)grade;
                            r.ctg_similar = esim & 1u;
                            out[slot] = r;
                        }
                    }
                    n_rec += (uint32_t)__popcll(taken);
                }
            }
        }
        if (!FILL && lane == 0u) {
            cnt[i] = n_rec;
            status[i] = found ? PAG_OK : PAG_EINVAL;
        }
    }
}

// the temporary device memory of a call that is allocated before the counts are known
struct BatchLayout {
    Carver c;
    size_t q, off, cnt, status, scan;
    explicit BatchLayout(uint64_t n_q)
        : q(c.take<pag_succ_query>(n_q)), off(c.take<uint64_t>(n_q + 1)), cnt(c.take<uint32_t>(n_q)), status(c.take<int32_t>(n_q)),
          scan(c.take<char>(scan_tmp_bytes(n_q))) {}
};

}  // namespace
}  // namespace pagdev

using namespace pagdev;

extern "C" {

uint64_t pag_successors_batch_bytes(uint64_t n_q, uint64_t n_records) {
    return n_q ? BatchLayout(n_q).c.bytes + n_records * sizeof(pag_succ) : 0;
}

int pag_successors_batch(const pag_graph *g, const pag_succ_query *q, uint64_t n_q, uint64_t deviation, double error_rate, uint64_t *off,
                         int32_t *status, pag_succ *out, uint64_t cap, uint64_t *n_total, double *ms_kernels) {
    if (n_total) *n_total = 0;
    if (ms_kernels) *ms_kernels = 0;
    if (!g || !off || !n_total || (!q && n_q) || (!out && cap)) {
        set_error("pag_successors_batch: a null handle, query list, off or total, or a null buffer with room");
        return PAG_EINVAL;
    }
    int rc = check_finished_graph(g, "pag_successors_batch", "successor of its vertices");
    if (rc) return rc;
    off[0] = 0;
    if (n_q == 0) return PAG_OK;
    QueryCall B("pag_successors_batch");
    const BatchLayout L(n_q);
    if ((rc = B.open(g, L.c.bytes))) return rc;
    const hipStream_t s = B.s;
    pag_succ_query *d_q = B.at<pag_succ_query>(L.q);
    uint64_t *d_off = B.at<uint64_t>(L.off);
    uint32_t *d_cnt = B.at<uint32_t>(L.cnt);
    int32_t *d_status = B.at<int32_t>(L.status);
    const QueryGraph G = query_graph(g);
    const uint32_t dev = (uint32_t)std::min<uint64_t>(deviation, 0xFFFFFFFFull);  // (coordinates are 32 bits: so is every difference of two)
    const dim3 grid(wave_per_item_grid(n_q));
    PAG_HIP_TRY(hipMemcpyAsync(d_q, q, n_q * sizeof(pag_succ_query), hipMemcpyHostToDevice, s));
    if ((rc = B.begin(QueryCall::COUNT))) return rc;
    k_succ_query<false><<<grid, dim3(256), 0, s>>>(G, d_q, n_q, dev, error_rate, d_cnt, d_status, nullptr, nullptr, 0);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = scan_u32_to_u64(d_cnt, d_off, n_q, d_off + n_q, B.at<char>(L.scan), s)) || (rc = B.end(QueryCall::COUNT))) return rc;
    PAG_HIP_TRY(hipMemcpyAsync(off, d_off, (n_q + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (status) PAG_HIP_TRY(hipMemcpyAsync(status, d_status, n_q * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if ((rc = B.done(QueryCall::COUNT, ms_kernels))) return rc;
    const uint64_t total = *n_total = off[n_q];
    if (total > cap) {
        set_error("pag_successors_batch: %llu records, room for %llu", (unsigned long long)total, (unsigned long long)cap);
        return PAG_ERANGE;
    }
    if (total == 0) return PAG_OK;
    SuccOut *d_out = nullptr;
    if ((rc = B.alloc(&d_out, total)) || (rc = B.begin(QueryCall::FILL))) return rc;
    k_succ_query<true><<<grid, dim3(256), 0, s>>>(G, d_q, n_q, dev, error_rate, nullptr, nullptr, d_off, d_out, total);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = B.end(QueryCall::FILL))) return rc;
    PAG_HIP_TRY(hipMemcpyAsync(out, d_out, total * sizeof(pag_succ), hipMemcpyDeviceToHost, s));
    return B.done(QueryCall::FILL, ms_kernels);
}

}  // extern "C"
