// k_walk_query.hip — pag_walk_straight_batch: PAlgorithm::walkStraight (PAlgorithm.tcc:93-170, with classifySuccessors :35-90) for
// a LIST of start vertices, evaluated on demand from the finished graph: the arrays pag_process / pag_shard_import leave in the
// handle, as k_succ_query.hip reads them.  No traversal view, no successor records, no marks of the walker.
//
// One wavefront per query, every wave on its own (no block barrier, no LDS, nothing shared between workgroups).  A step of a walk:
//   1. the successor list of the current vertex with the toolbox of query_graph.hpp, as k_succ_query.hip: the head of the k-mer's
//      edge segment (64 pivots per round), per 64 edges the candidate pairs (SuccPairs: the heads of all targets at once by groups
//      of lanes, the pairs flattened) dealt to the lanes 64 at a time through d_check_position;
//   2. instead of a record, every lane grades, filters and classifies its pair: the caller's frame (reverse strand, the two
//      coordinate hulls), the walk's own hull, the leap test with the landing rule, the class by grade — all from registers and
//      the contig table; then, ONLY for the pairs that are still alive, the two memberships: the frame's sorted `excl` slice (a
//      binary search per surviving lane, all survivors at once, 64-bit keys compared whole) and the path so far (the lanes scan
//      it, 64 entries a turn, one survivor after the other);
//   3. a ballot per class: the running count of each class and the first record of each (kept in lane c for class c).  After
//      the list the first non-empty class decides: none — End; more than one — Branch; one — the step.
// Every step appends a vertex the path does not hold and the path has at most `limit` entries, so every walk ends; every loop
// is bounded by a segment length, the path length or the limit.
//
// The kernel runs twice, as its siblings do: it counts (path length, size of the branch's class, status), the counts are
// scanned into the two offset arrays, it runs again and fills.  While counting, a wave keeps its path in a slot of call-scope
// scratch (the membership test reads it); while filling, the path lies where it is delivered.  In the filling run a Branch
// evaluates its last list once more to write the chosen class in record order.  Offsets and outputs are a function of the
// inputs alone.
#include <algorithm>
#include <vector>

#include "query_call.hpp"
#include "query_graph.hpp"

namespace pagdev {
namespace {

struct WalkNode {  // pag_walk_node
    uint32_t code, step;
    uint64_t pos;
    uint32_t abundance, reserved;
};
static_assert(sizeof(WalkNode) == sizeof(pag_walk_node), "pag_walk_node layout");
struct AltOut {  // pag_succ
    uint32_t code, step;
    uint64_t pos;
    uint32_t grade, ctg_similar;
};
static_assert(sizeof(AltOut) == sizeof(pag_succ), "pag_succ layout");
static_assert(sizeof(pag_walk_frame) == 64 && sizeof(pag_walk_query) == 32, "pag_walk_frame / pag_walk_query layout");

enum { WS_END = PAG_WALK_END, WS_BRANCH = PAG_WALK_BRANCH, WS_LIMIT = PAG_WALK_LIMIT, WS_LEAP = PAG_WALK_LEAP };

struct WalkTables {
    const pag_walk_frame *frames;
    const pag_succ_query *excl;
    const uint64_t *starts, *sizes;  // PositionMapper's start table [n_ctgs + 1] (one entry, 0, without contigs) and the lengths
    uint32_t n_ctgs;
    uint32_t dev;
    double err;
};

// the landing rule (PAlgorithm.tcc:60-67): singleToDual on the start table, refused when the offset lies beyond size * leap_min —
// the walker's own arithmetic (classify_record, k5_travel.hip)
__device__ __forceinline__ bool landing_refused(const WalkTables &W, uint32_t pc, double leap_min) {
    uint32_t lo = 0, hi = W.n_ctgs + 1u;
    while (lo < hi) {  // upper_bound(starts, pc)
        const uint32_t mid = (lo + hi) >> 1;
        if (W.starts[mid] <= (uint64_t)pc) lo = mid + 1u;
        else hi = mid;
    }
    const uint32_t idx = lo ? lo - 1u : 0u;
    uint64_t off = (uint64_t)pc - W.starts[idx];
    const uint64_t sz = idx < W.n_ctgs ? W.sizes[idx] : 0ull;
    if (off >= 2u * sz) off -= 2u * sz;
    return (double)(int64_t)off > (double)sz * leap_min;
}

// FILL = false: n_cnt[i] = entries of query i's path, a_cnt[i] = records of its branch's class, status[i]; the path is kept in
// the wave's slot of `scratch` (stride entries, >= every limit).  FILL = true: the path to nodes[n_off[i] ..), the class to
// alts[a_off[i] ..); nothing is written at or beyond n_nodes / n_alts.
template <bool FILL>
__global__ void __launch_bounds__(256) k_walk_query(QueryGraph G, WalkTables W, const pag_walk_query *__restrict__ q, uint64_t n_q,
                                                    uint32_t *__restrict__ n_cnt, uint32_t *__restrict__ a_cnt, int32_t *__restrict__ status,
                                                    const uint64_t *__restrict__ n_off, const uint64_t *__restrict__ a_off, WalkNode *nodes,
                                                    uint64_t n_nodes, AltOut *__restrict__ alts, uint64_t n_alts, WalkNode *scratch, uint32_t stride) {
    const uint32_t lane = lane_id(), waves = blockDim.x / 64u;
    const uint64_t n_waves = (uint64_t)gridDim.x * waves, wave = (uint64_t)blockIdx.x * waves + uniform_u32(threadIdx.x / 64u);
    for (uint64_t i = wave; i < n_q; i += n_waves) {
        const uint32_t q_code = q[i].code, q_dist = q[i].dist, limit = q[i].limit;
        const uint64_t q_pos = q[i].pos, has_size = q[i].has_size;
        const pag_walk_frame *__restrict__ F = W.frames + q[i].frame;
        const uint32_t ctg_left = F->ctg_left, ctg_right = F->ctg_right, rev_left = F->rev_left, rev_right = F->rev_right;
        const uint32_t h0_lo = F->hull_lo[0], h0_hi = F->hull_hi[0], h1_lo = F->hull_lo[1], h1_hi = F->hull_hi[1];
        const uint64_t split_size = F->split_size, excl_n = F->excl_n;
        const double leap_min = F->leap_min;
        const pag_succ_query *__restrict__ X = W.excl + F->excl_off;
        WalkNode *path = scratch + wave * stride;
        uint64_t cap = stride, a_at = 0;
        if (FILL) {
            cap = n_off[i + 1] - n_off[i];
            if (cap == 0) continue;  // (a vertex the graph does not hold)
            path = nodes + n_off[i];
            if (n_off[i] + cap > n_nodes) cap = n_off[i] < n_nodes ? n_nodes - n_off[i] : 0;
            a_at = a_off[i];
        }
        // the start: its k-mer's leaders, its slot among them (the count lies there)
        const Bound sb = group_lower_bound(G.tkey, G.T, q_code, 64u, true);
        bool found = false;
        uint64_t slot0 = 0;
        if (__ballot(sb.hit) != 0ull) {
            const uint64_t h = from_lane(sb.at, 0u);
            const uint32_t nl = G.tseg[h];
            for (uint32_t jb = 0; jb < nl && !found; jb += 64u) {
                const uint64_t s = h + jb + lane;
                const uint64_t m = __ballot(jb + lane < nl && s < G.T && G.tval[s] == q_pos);
                if (m != 0ull) {
                    found = true;
                    slot0 = h + jb + (uint32_t)__ffsll((long long)m) - 1u;
                }
            }
        }
        uint32_t len = 0, n_alt = 0;
        int st = PAG_EINVAL;
        if (found) {
            if (lane == 0u && cap > 0u) {
                WalkNode r;
                r.code = q_code, r.step = q_dist, r.pos = q_pos, r.abundance = G.tcnt[slot0], r.reserved = 0;
                path[0] = r;
            }
            len = 1;
            __threadfence_block();  // (the lanes read the path back)
            uint32_t cur_code = q_code;
            uint64_t cur_pos = q_pos, now = q_dist;
            uint32_t own_lo = 0xFFFFFFFFu, own_hi = 0u;
            const uint32_t c_start = (uint32_t)(q_pos >> 32);
            bool walking = true;
            if (c_start != 0u) {
                if (c_start < ctg_left || c_start >= ctg_right) st = WS_LEAP, walking = false;
                own_lo = own_hi = c_start;
            }
            int emit = -1;  // the class written to alts in this evaluation (the second one of a Branch's last vertex)
            while (walking) {
                const bool can_leap = has_size + now >= split_size;
                const uint32_t ac = (uint32_t)(cur_pos >> 32), ar = (uint32_t)cur_pos;
                uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;                  // records of each class so far
                uint32_t sv_code = 0, sv_step = 0;                        // lane c: the first record of class c
                uint64_t sv_pos = 0, sv_slot = 0;
                const Bound hd = group_lower_bound(G.ekey, G.E, cur_code, 64u, true);
                const uint64_t eh = from_lane(hd.at, 0u);
                const uint32_t ne = __ballot(hd.hit) != 0ull ? G.eseg[eh] : 0u;
                for (uint32_t eb = 0; eb < ne; eb += 64u) {
                    const uint32_t turn = ne - eb < 64u ? ne - eb : 64u;
                    const SuccPairs P(G, edge_turn(G, eh + eb, turn), turn);
                    for (uint64_t pb = 0; pb < P.n_pairs; pb += 64u) {
                        const SuccPairs::Pair p = P.pair(pb + lane);
                        const uint64_t tp = p.pos;
                        int grade = G_OOPS;
                        uint32_t esim = 0;
                        if (p.live) grade = d_check_position(ac, ar, (uint32_t)(tp >> 32), (uint32_t)tp, p.step, W.dev, W.err, &esim);
                        // the filters that cost nothing: the frame's reverse strand and hulls, the own hull, the leap test, the class
                        const uint32_t tc = (uint32_t)(tp >> 32);
                        const bool bound_by_hulls = tc != 0u && (esim & 1u) == 0u;
                        bool ok = grade != G_OOPS;
                        ok = ok && !(tc != 0u && tc >= rev_left && tc < rev_right);
                        ok = ok && !(bound_by_hulls && ((h0_lo <= tc && tc <= h0_hi) || (h1_lo <= tc && tc <= h1_hi) || (own_lo <= tc && tc <= own_hi)));
                        const bool leap = tc != 0u && (tc < ctg_left || tc >= ctg_right);
                        if (ok && leap) ok = can_leap && !landing_refused(W, tc, leap_min);
                        // class by grade through a nibble table: Amazing 0, Excellent 1, Good 2, Skip 3 (only once leaping is allowed)
                        const uint32_t table = can_leap ? 0xFFF0123Fu : 0xFFF012FFu;
                        const uint32_t cls = leap ? 0u : (table >> ((uint32_t)grade * 4u)) & 0xFu;
                        ok = ok && cls != 0xFu;
                        // the two memberships, for what is left: the frame's excl slice ...
                        if (ok && excl_n != 0ull) {
                            uint64_t lo = 0, hi = excl_n;
                            while (lo < hi) {
                                const uint64_t mid = (lo + hi) >> 1;
                                const uint32_t xc = X[mid].code;
                                if (xc < p.code || (xc == p.code && X[mid].pos < tp)) lo = mid + 1u;
                                else hi = mid;
                            }
                            if (lo < excl_n && X[lo].code == p.code && X[lo].pos == tp) ok = false;
                        }
                        // ... and the path so far
                        for (uint64_t left = __ballot(ok); left != 0ull; left &= left - 1ull) {
                            const uint32_t l = (uint32_t)__ffsll((long long)left) - 1u;
                            const uint32_t s_code = (uint32_t)__shfl((int)p.code, (int)l);
                            const uint64_t s_pos = from_lane(tp, l);
                            bool on_path = false;
                            for (uint32_t jb = 0; jb < len && !on_path; jb += 64u) {
                                const uint32_t j = jb + lane;
                                on_path = __ballot(j < len && j < cap && path[j].code == s_code && path[j].pos == s_pos) != 0ull;
                            }
                            if (on_path && lane == l) ok = false;
                        }
                        // per class: the first record stays in lane c, a Branch's class goes out in record order
#pragma unroll
                        for (uint32_t c = 0; c < 4u; ++c) {
                            const uint64_t m = __ballot(ok && cls == c);
                            if (m == 0ull) continue;
                            const uint32_t have = c == 0u ? c0 : c == 1u ? c1 : c == 2u ? c2 : c3;
                            if (have == 0u) {
                                const uint32_t l = (uint32_t)__ffsll((long long)m) - 1u;
                                const uint32_t f_code = (uint32_t)__shfl((int)p.code, (int)l), f_step = (uint32_t)__shfl((int)p.step, (int)l);
                                const uint64_t f_pos = from_lane(tp, l), f_slot = from_lane(p.slot, l);
                                if (lane == c) sv_code = f_code, sv_step = f_step, sv_pos = f_pos, sv_slot = f_slot;
                            }
                            if (FILL && emit == (int)c && ok && cls == c) {
                                const uint64_t o = a_at + have + (uint32_t)__popcll(m & lanemask_lt());
                                if (o < n_alts) {
                                    AltOut r;
                                    r.code = p.code, r.step = p.step, r.pos = tp, r.grade = (uint32_t)grade, r.ctg_similar = esim & 1u;
                                    alts[o] = r;
                                }
                            }
                            const uint32_t add = (uint32_t)__popcll(m);
                            if (c == 0u) c0 += add;
                            else if (c == 1u) c1 += add;
                            else if (c == 2u) c2 += add;
                            else c3 += add;
                        }
                    }
                }
                if (emit >= 0) break;  // (the Branch's class is written)
                const uint32_t c = c0 ? 0u : c1 ? 1u : c2 ? 2u : 3u;
                const uint32_t n = c0 ? c0 : c1 ? c1 : c2 ? c2 : c3;
                if (n == 0u) {
                    st = WS_END;
                    break;
                }
                if (n > 1u) {
                    st = WS_BRANCH;
                    n_alt = n;
                    if (!FILL) break;
                    emit = (int)c;
                    continue;
                }
                const uint32_t nx_code = (uint32_t)__shfl((int)sv_code, (int)c), nx_step = (uint32_t)__shfl((int)sv_step, (int)c);
                const uint64_t nx_pos = from_lane(sv_pos, c), nx_slot = from_lane(sv_slot, c);
                if (lane == 0u && len < cap) {
                    WalkNode r;
                    r.code = nx_code, r.step = nx_step, r.pos = nx_pos, r.abundance = G.tcnt[nx_slot], r.reserved = 0;
                    path[len] = r;
                }
                ++len;
                __threadfence_block();
                now += nx_step;
                const uint32_t nc = (uint32_t)(nx_pos >> 32);
                if (nc != 0u) {
                    own_lo = nc < own_lo ? nc : own_lo;
                    own_hi = nc > own_hi ? nc : own_hi;
                    if (nc < ctg_left || nc >= ctg_right) {
                        st = WS_LEAP;
                        break;
                    }
                }
                if (len >= limit) {
                    st = WS_LIMIT;
                    break;
                }
                cur_code = nx_code;
                cur_pos = nx_pos;
            }
        }
        if (!FILL && lane == 0u) {
            n_cnt[i] = len;
            a_cnt[i] = n_alt;
            status[i] = st;
        }
    }
}

// the temporary device memory of a call that is allocated before the counts are known
struct WalkLayout {
    Carver c;
    size_t q, frames, excl, n_off, a_off, n_cnt, a_cnt, status, scan;
    WalkLayout(uint64_t n_q, uint64_t n_frames, uint64_t n_excl)
        : q(c.take<pag_walk_query>(n_q)), frames(c.take<pag_walk_frame>(n_frames)), excl(c.take<pag_succ_query>(n_excl)), n_off(c.take<uint64_t>(n_q + 1)),
          a_off(c.take<uint64_t>(n_q + 1)), n_cnt(c.take<uint32_t>(n_q)), a_cnt(c.take<uint32_t>(n_q)), status(c.take<int32_t>(n_q)),
          scan(c.take<char>(scan_tmp_bytes(n_q))) {}
};
// The counting run's path slots: one per wave of the grid, `stride` entries each (the largest limit of the call).  At most
// SCRATCH_BYTES of them (but 64 waves at any limit), and never more waves than queries.
constexpr uint64_t SCRATCH_BYTES = 256ull << 20, GRID_WAVES_MAX = 256u * 32u * 4u, GRID_WAVES_MIN = 64u;
uint64_t grid_waves(uint64_t n_q, uint64_t stride) {
    const uint64_t fit = std::max<uint64_t>(GRID_WAVES_MIN, std::min<uint64_t>(GRID_WAVES_MAX, SCRATCH_BYTES / (stride * sizeof(WalkNode))));
    return (std::min<uint64_t>(n_q, fit) + 3u) / 4u * 4u;  // (whole blocks of 4 waves)
}

}  // namespace
}  // namespace pagdev

using namespace pagdev;

extern "C" {

uint64_t pag_walk_straight_batch_bytes(uint64_t n_q, uint64_t n_frames, uint64_t n_excl, uint64_t n_nodes, uint64_t n_alts) {
    if (n_q == 0) return 0;
    return WalkLayout(n_q, n_frames, n_excl).c.bytes + grid_waves(n_q, PAG_WALK_LIMIT_MAX) * PAG_WALK_LIMIT_MAX * sizeof(pag_walk_node) +
           n_nodes * sizeof(pag_walk_node) + n_alts * sizeof(pag_succ);
}

int pag_walk_straight_batch(const pag_graph *g, const pag_walk_query *q, uint64_t n_q, const pag_walk_frame *frames, uint64_t n_frames,
                            const pag_succ_query *excl, uint64_t n_excl, const uint32_t *ctg_len, uint64_t n_ctgs, uint64_t deviation,
                            double error_rate, uint64_t *node_off, pag_walk_node *nodes, uint64_t node_cap, uint64_t *alt_off, pag_succ *alts,
                            uint64_t alt_cap, int32_t *status, uint64_t *n_nodes, uint64_t *n_alts, double *ms_kernels) {
    if (n_nodes) *n_nodes = 0;
    if (n_alts) *n_alts = 0;
    if (ms_kernels) *ms_kernels = 0;
    // the arguments first, the handle after them, all on the host: nothing below touches a device before every check has passed
    if (!node_off || !alt_off || !n_nodes || !n_alts || (!q && n_q) || (!frames && n_frames) || (!excl && n_excl) || (!ctg_len && n_ctgs) ||
        (!nodes && node_cap) || (!alts && alt_cap)) {
        set_error("pag_walk_straight_batch: a null argument");
        return PAG_EINVAL;
    }
    if (n_ctgs >= 0xFFFFFFFFull) {
        set_error("pag_walk_straight_batch: %llu contigs", (unsigned long long)n_ctgs);
        return PAG_EINVAL;
    }
    uint32_t stride = 2;
    for (uint64_t i = 0; i < n_q; ++i) {
        if (q[i].frame >= n_frames) {
            set_error("pag_walk_straight_batch: query %llu names frame %u of %llu", (unsigned long long)i, q[i].frame, (unsigned long long)n_frames);
            return PAG_EINVAL;
        }
        if (q[i].limit < 2u || q[i].limit > PAG_WALK_LIMIT_MAX) {
            set_error("pag_walk_straight_batch: query %llu has limit %u (2 .. %u)", (unsigned long long)i, q[i].limit, (unsigned)PAG_WALK_LIMIT_MAX);
            return PAG_EINVAL;
        }
        stride = std::max(stride, q[i].limit);
    }
    for (uint64_t f = 0; f < n_frames; ++f) {
        const uint64_t lo = frames[f].excl_off, n = frames[f].excl_n;
        if (lo > n_excl || n > n_excl - lo) {
            set_error("pag_walk_straight_batch: frame %llu: excl[%llu .. + %llu) of %llu", (unsigned long long)f, (unsigned long long)lo, (unsigned long long)n,
                      (unsigned long long)n_excl);
            return PAG_EINVAL;
        }
        for (uint64_t j = lo + 1; j < lo + n; ++j)
            if (excl[j - 1].code > excl[j].code || (excl[j - 1].code == excl[j].code && excl[j - 1].pos >= excl[j].pos)) {
                set_error("pag_walk_straight_batch: frame %llu: excl is not strictly ascending at entry %llu", (unsigned long long)f, (unsigned long long)j);
                return PAG_EINVAL;
            }
    }
    if (!g) {
        set_error("pag_walk_straight_batch: a null handle");
        return PAG_EINVAL;
    }
    int rc = check_finished_graph(g, "pag_walk_straight_batch", "successor of its vertices");
    if (rc) return rc;
    node_off[0] = alt_off[0] = 0;
    if (n_q == 0) return PAG_OK;
    // PositionMapper's tables over ctg_len (position_mapper.hpp:18-25); without contigs a single start, 0
    std::vector<uint64_t> tables(2 * n_ctgs + 1, 0);
    uint64_t *starts = tables.data(), *sizes = starts + n_ctgs + 1;
    for (uint64_t c = 0; c < n_ctgs; ++c) sizes[c] = ctg_len[c];
    if (n_ctgs) {
        starts[0] = sizes[0];
        for (uint64_t c = 1; c < n_ctgs; ++c) starts[c] = starts[c - 1] + 3 * sizes[c - 1] + std::max(sizes[c - 1], sizes[c]);
        starts[n_ctgs] = starts[n_ctgs - 1] + 4 * sizes[n_ctgs - 1];
    }
    QueryCall B("pag_walk_straight_batch");
    const WalkLayout L(n_q, n_frames, n_excl);
    const uint64_t waves = grid_waves(n_q, stride);
    uint64_t *d_tables = nullptr;
    WalkNode *d_paths = nullptr, *d_nodes = nullptr;
    AltOut *d_alts = nullptr;
    if ((rc = B.open(g, L.c.bytes)) || (rc = B.up(tables.data(), tables.size(), &d_tables, 0)) || (rc = B.alloc(&d_paths, waves * stride))) return rc;
    const hipStream_t s = B.s;
    pag_walk_query *d_q = B.at<pag_walk_query>(L.q);
    pag_walk_frame *d_frames = B.at<pag_walk_frame>(L.frames);
    pag_succ_query *d_excl = B.at<pag_succ_query>(L.excl);
    uint64_t *d_n_off = B.at<uint64_t>(L.n_off), *d_a_off = B.at<uint64_t>(L.a_off);
    uint32_t *d_n_cnt = B.at<uint32_t>(L.n_cnt), *d_a_cnt = B.at<uint32_t>(L.a_cnt);
    int32_t *d_status = B.at<int32_t>(L.status);
    const QueryGraph G = query_graph(g);
    WalkTables W;
    W.frames = d_frames, W.excl = d_excl, W.starts = d_tables, W.sizes = d_tables + n_ctgs + 1, W.n_ctgs = (uint32_t)n_ctgs;
    W.dev = (uint32_t)std::min<uint64_t>(deviation, 0xFFFFFFFFull);  // (coordinates are 32 bits: so is every difference of two)
    W.err = error_rate;
    PAG_HIP_TRY(hipMemcpyAsync(d_q, q, n_q * sizeof(pag_walk_query), hipMemcpyHostToDevice, s));
    PAG_HIP_TRY(hipMemcpyAsync(d_frames, frames, n_frames * sizeof(pag_walk_frame), hipMemcpyHostToDevice, s));
    if (n_excl) PAG_HIP_TRY(hipMemcpyAsync(d_excl, excl, n_excl * sizeof(pag_succ_query), hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)(waves / 4u));
    if ((rc = B.begin(QueryCall::COUNT))) return rc;
    k_walk_query<false><<<grid, dim3(256), 0, s>>>(G, W, d_q, n_q, d_n_cnt, d_a_cnt, d_status, nullptr, nullptr, nullptr, 0, nullptr, 0, d_paths, stride);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = scan_u32_to_u64(d_n_cnt, d_n_off, n_q, d_n_off + n_q, B.at<char>(L.scan), s))) return rc;
    if ((rc = scan_u32_to_u64(d_a_cnt, d_a_off, n_q, d_a_off + n_q, B.at<char>(L.scan), s)) || (rc = B.end(QueryCall::COUNT))) return rc;
    PAG_HIP_TRY(hipMemcpyAsync(node_off, d_n_off, (n_q + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PAG_HIP_TRY(hipMemcpyAsync(alt_off, d_a_off, (n_q + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (status) PAG_HIP_TRY(hipMemcpyAsync(status, d_status, n_q * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if ((rc = B.done(QueryCall::COUNT, ms_kernels))) return rc;
    const uint64_t total_n = *n_nodes = node_off[n_q], total_a = *n_alts = alt_off[n_q];
    if (total_n > node_cap || total_a > alt_cap) {
        set_error("pag_walk_straight_batch: %llu path entries and %llu alternatives, room for %llu and %llu", (unsigned long long)total_n,
                  (unsigned long long)total_a, (unsigned long long)node_cap, (unsigned long long)alt_cap);
        return PAG_ERANGE;
    }
    if (total_n == 0) return PAG_OK;
    if ((rc = B.alloc(&d_nodes, total_n)) || (rc = B.alloc(&d_alts, total_a)) || (rc = B.begin(QueryCall::FILL))) return rc;
    k_walk_query<true><<<grid, dim3(256), 0, s>>>(G, W, d_q, n_q, nullptr, nullptr, nullptr, d_n_off, d_a_off, d_nodes, total_n, d_alts, total_a, d_paths,
                                                  stride);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = B.end(QueryCall::FILL))) return rc;
    PAG_HIP_TRY(hipMemcpyAsync(nodes, d_nodes, total_n * sizeof(pag_walk_node), hipMemcpyDeviceToHost, s));
    if (total_a) PAG_HIP_TRY(hipMemcpyAsync(alts, d_alts, total_a * sizeof(pag_succ), hipMemcpyDeviceToHost, s));
    return B.done(QueryCall::FILL, ms_kernels);
}

}  // extern "C"
