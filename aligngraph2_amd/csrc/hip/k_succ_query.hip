// k_succ_query.hip — pag_successors_batch: the successor lists of a LIST of vertices, evaluated on demand from the finished graph.
//
// PABruijnGraph::successors (PABruijnGraph.cpp:370-373 -> searchSuccessors :167-197) with the caller's deviation and error rate,
// for vertices named by (k-mer code, position), straight from the arrays pag_process / pag_shard_import leave in the handle —
// the k-mer-sorted tuple stream with its in-place segment results and the source-sorted edge stream (the layout pag_export_csr
// reads, pag_api.hip): no traversal view, no compact CSR, no records of anybody else's vertex.
//
// One wavefront per query, every wave on its own (no block barrier, no LDS).  A query is a chain of dependent loads from
// arrays of 10^8 entries, so the kernel is built to keep that chain short (group_lower_bound):
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
// of the inputs alone.  The walker's "used" marks play no part: this is the reference's call on a fresh graph.
#include <algorithm>
#include <cstring>

#include "dev_call.hpp"
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
                if (eb != 0u) ev = lane < turn && eh + eb + lane < G.E ? G.eval[eh + eb + lane] : 0ull;
                const uint32_t tcode = (uint32_t)(ev >> 32), step = (uint32_t)ev >> 1;
                // head and leader count of every edge's target (none: a k-mer without positions), edge e by the lanes e W .. e W + W - 1
                uint32_t W = 64u;
                while (64u / W < turn) W >>= 1;
                const uint32_t grp = lane / W;
                const Bound tb = group_lower_bound(G.tkey, G.T, (uint32_t)__shfl((int)tcode, (int)grp), W, grp < turn);
                const uint32_t mine = lane < turn ? lane * W : 0u;  // (first lane of the group that looked this lane's target up)
                const uint64_t th = from_lane(tb.at, mine);
                const bool t_hit = __shfl((int)tb.hit, (int)mine) != 0;
                uint32_t tn = lane < turn && t_hit ? G.tseg[th] : 0u;
                if (tn > G.T - th) tn = (uint32_t)(G.T - th);  // (never in a finished graph: a segment ends inside the stream)
                // the candidate pairs of these edges, flattened: pair x belongs to the last edge whose prefix sum is <= x
                uint64_t n_pairs;
                const uint64_t ex = wave_excl_sum64((uint64_t)tn, &n_pairs);
                for (uint64_t pb = 0; pb < n_pairs; pb += 64u) {
                    const uint64_t x = pb + lane;
                    uint32_t e = 0;
#pragma unroll
                    for (uint32_t b = 32u; b != 0u; b >>= 1) {
                        const uint64_t v = __shfl(ex, (int)(e + b));
                        if (v <= x) e += b;
                    }
                    const uint64_t e_th = __shfl(th, (int)e), e_ex = __shfl(ex, (int)e);
                    const uint32_t e_step = (uint32_t)__shfl((int)step, (int)e), e_code = (uint32_t)__shfl((int)tcode, (int)e);
                    int grade = G_OOPS;
                    uint32_t esim = 0;
                    uint64_t tp = 0;
                    if (x < n_pairs) {
                        tp = G.tval[e_th + (x - e_ex)];
                        grade = d_check_position(ac, ar, (uint32_t)(tp >> 32), (uint32_t)tp, e_step, dev, err, &esim);
                    }
                    const uint64_t taken = __ballot(grade != G_OOPS);
                    if (FILL && grade != G_OOPS) {
                        const uint64_t slot = at + n_rec + (uint32_t)__popcll(taken & lanemask_lt());
                        if (slot < n_out) {
                            SuccOut r;
                            r.code = e_code;
                            r.step = e_step;
                            r.pos = tp;
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

size_t align256(size_t x) { return (x + 255u) & ~(size_t)255u; }
// the temporary device memory of a call: what is allocated before the counts are known, and the records
struct BatchLayout {
    size_t q, off, cnt, status, scan, bytes;
    explicit BatchLayout(uint64_t n_q) {
        q = 0;
        off = q + align256(n_q * sizeof(pag_succ_query));
        cnt = off + align256((n_q + 1) * sizeof(uint64_t));
        status = cnt + align256(n_q * sizeof(uint32_t));
        scan = status + align256(n_q * sizeof(int32_t));
        bytes = scan + align256(scan_tmp_bytes(n_q));
    }
};

struct BatchScratch : DevCall {  // on the handle's stream; the events of the two timings
    char *a = nullptr;
    SuccOut *b = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    BatchScratch() : DevCall("pag_successors_batch") {}
    ~BatchScratch() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
};

// 4 waves per block; more blocks than are resident at once (6 or 7 per CU by the kernels' registers): the dispatcher keeps every CU full to the end
unsigned query_grid(uint64_t n_q) { return (unsigned)std::min<uint64_t>((n_q + 3) / 4, 256u * 32u); }

}  // namespace
}  // namespace pagdev

using namespace pagdev;

extern "C" {

uint64_t pag_successors_batch_bytes(uint64_t n_q, uint64_t n_records) {
    return n_q ? BatchLayout(n_q).bytes + n_records * sizeof(pag_succ) : 0;
}

int pag_successors_batch(const pag_graph *g, const pag_succ_query *q, uint64_t n_q, uint64_t deviation, double error_rate, uint64_t *off,
                         int32_t *status, pag_succ *out, uint64_t cap, uint64_t *n_total, double *ms_kernels) {
    if (n_total) *n_total = 0;
    if (ms_kernels) *ms_kernels = 0;
    if (!g || !off || !n_total || (!q && n_q) || (!out && cap)) return PAG_EINVAL;
    if (!g->tkey) {
        set_error("pag_successors_batch: the handle holds no finished graph (pag_process / pag_shard_import first)");
        return PAG_EINVAL;
    }
    if (g->regional) {
        set_error("pag_successors_batch: the handle holds one rank's region of a block (pag_shard_set_region): a region does not hold every successor of its vertices");
        return PAG_ERANGE;
    }
    off[0] = 0;
    if (n_q == 0) return PAG_OK;
    BatchScratch B;
    const hipStream_t s = B.s = g->stream;
    const BatchLayout L(n_q);
    int rc = B.open(g->device, false, DevCall::NO_STREAM);
    if (rc || (rc = B.alloc(&B.a, L.bytes))) return rc;
    for (hipEvent_t &ev : B.ev) PAG_HIP_TRY(hipEventCreate(&ev));
    pag_succ_query *d_q = (pag_succ_query *)(B.a + L.q);
    uint64_t *d_off = (uint64_t *)(B.a + L.off);
    uint32_t *d_cnt = (uint32_t *)(B.a + L.cnt);
    int32_t *d_status = (int32_t *)(B.a + L.status);
    QueryGraph G{g->tkey, g->tval, g->tseg, g->ekey, g->eval, g->eseg, g->n_t, g->n_e};
    const uint32_t dev = (uint32_t)std::min<uint64_t>(deviation, 0xFFFFFFFFull);  // (coordinates are 32 bits: so is every difference of two)
    PAG_HIP_TRY(hipMemcpyAsync(d_q, q, n_q * sizeof(pag_succ_query), hipMemcpyHostToDevice, s));
    PAG_HIP_TRY(hipEventRecord(B.ev[0], s));
    k_succ_query<false><<<dim3(query_grid(n_q)), dim3(256), 0, s>>>(G, d_q, n_q, dev, error_rate, d_cnt, d_status, nullptr, nullptr, 0);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = scan_u32_to_u64(d_cnt, d_off, n_q, d_off + n_q, B.a + L.scan, s))) return rc;
    PAG_HIP_TRY(hipEventRecord(B.ev[1], s));
    PAG_HIP_TRY(hipMemcpyAsync(off, d_off, (n_q + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (status) PAG_HIP_TRY(hipMemcpyAsync(status, d_status, n_q * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PAG_HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = off[n_q];
    *n_total = total;
    float ms = 0, ms2 = 0;
    PAG_HIP_TRY(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
    if (ms_kernels) *ms_kernels = ms;
    if (total > cap) {
        set_error("pag_successors_batch: %llu records, room for %llu", (unsigned long long)total, (unsigned long long)cap);
        return PAG_ERANGE;
    }
    if (total == 0) return PAG_OK;
    if ((rc = B.alloc(&B.b, total))) return rc;
    PAG_HIP_TRY(hipEventRecord(B.ev[2], s));
    k_succ_query<true><<<dim3(query_grid(n_q)), dim3(256), 0, s>>>(G, d_q, n_q, dev, error_rate, nullptr, nullptr, d_off, B.b, total);
    PAG_HIP_TRY(hipGetLastError());
    PAG_HIP_TRY(hipEventRecord(B.ev[3], s));
    PAG_HIP_TRY(hipMemcpyAsync(out, B.b, total * sizeof(pag_succ), hipMemcpyDeviceToHost, s));
    PAG_HIP_TRY(hipStreamSynchronize(s));
    PAG_HIP_TRY(hipEventElapsedTime(&ms2, B.ev[2], B.ev[3]));
    if (ms_kernels) *ms_kernels = (double)ms + (double)ms2;
    return PAG_OK;
}

}  // extern "C"
