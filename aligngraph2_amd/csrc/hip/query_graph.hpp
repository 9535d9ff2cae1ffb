// query_graph.hpp — the device toolbox of the on-demand kernels over the FINISHED graph (k_succ_query.hip: the successor lists of a
// list of vertices; k_find.hip: the vertices along a list of sequences; k_walk_query.hip: walkStraight from a list of vertices):
// the arrays pag_process / pag_shard_import leave in the handle, the lower bound by groups of lanes that keeps a query's chain of
// dependent loads short, the heads of up to 64 keys at once, the candidate pairs of a successor list dealt to the lanes, and the
// small lane helpers.  One wavefront per item in all three; every helper here is called by ALL 64 lanes together.
#pragma once
#include "pag_graph_impl.hpp"
#include "trav_device.hpp"

namespace pagdev {

struct QueryGraph {
    const uint32_t *tkey;
    const uint64_t *tval;
    const uint32_t *tseg;
    const uint16_t *tcnt;  // the positions' counts, by tuple slot
    const uint32_t *ekey;
    const uint64_t *eval;
    const uint32_t *eseg;
    uint64_t T, E;
};
inline QueryGraph query_graph(const pag_graph *g) { return QueryGraph{g->tkey, g->tval, g->tseg, g->tcnt, g->ekey, g->eval, g->eseg, g->n_t, g->n_e}; }

// Lower bounds by groups of lanes.  The wave is cut into groups of G lanes (G a power of two, the same in every lane; group =
// lane / G); every lane of a group passes the group's sorted array a[0 .. n), its key, and whether the group searches at all.
// Returns, in every lane of the group, the first index whose element is >= key (n: none) and whether that element IS the key.
// ALL 64 lanes call it together.  A round: G pivots cut the window [lo, hi] into G + 1 parts, the lanes whose pivot is below
// the key say so (a ballot, masked to the group), the window becomes the part behind the last of them; the invariant is that
// the answer lies in [lo, hi] and a[hi] >= key (or hi = n).  The last round reads the whole window, hi included: the element
// at the answer is in some lane's hands and is compared with the key there, no load of its own.
struct Bound {
    uint64_t at;
    bool hit;
};
__device__ __forceinline__ Bound group_lower_bound(const uint32_t *__restrict__ a, uint64_t n, uint32_t key, uint32_t G, bool on) {
    const uint32_t lane = lane_id(), sub = lane & (G - 1u);
    const uint64_t gmask = (G == 64u ? ~0ull : (1ull << G) - 1ull) << (lane & ~(G - 1u));
    uint64_t lo = 0, hi = on ? n : 0;
    while (__ballot(hi - lo >= G) != 0ull) {
        const bool act = hi - lo >= G;
        const uint64_t chunk = (hi - lo + 1u + G) / (G + 1u);  // ceil((window + 1) / (G + 1))
        const uint64_t p = lo + (uint64_t)(sub + 1u) * chunk - 1u;
        const bool below = act && p < hi && a[p] < key;
        const uint32_t c = (uint32_t)__popcll(__ballot(below) & gmask);  // (a[] is sorted: the group's first c lanes)
        if (act) {
            lo += (uint64_t)c * chunk;  // (behind pivot c - 1; c = 0: where it was)
            hi = lo + chunk - 1u < hi ? lo + chunk - 1u : hi;  // (pivot c, which is not below the key — or the old end)
        }
    }
    const uint64_t x = lo + sub;  // (the window holds at most G - 1 elements below hi)
    const bool ok = on && x <= hi && x < n;
    const uint32_t v = ok ? a[x] : 0u;
    Bound r;
    r.at = lo + (uint64_t)__popcll(__ballot(ok && x < hi && v < key) & gmask);
    r.hit = (__ballot(ok && x == r.at && v == key) & gmask) != 0ull;
    return r;
}
__device__ __forceinline__ uint32_t uniform_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint32_t from_lane(uint32_t x, uint32_t l) { return (uint32_t)__shfl((int)x, (int)l); }
__device__ __forceinline__ uint64_t from_lane(uint64_t x, uint32_t l) {
    return (uint64_t)from_lane((uint32_t)x, l) | ((uint64_t)from_lane((uint32_t)(x >> 32), l) << 32);
}
// the last lane whose exclusive sum is <= x (the sums ascend with the lane): the lane that holds item x of the flattened lists,
// when x is below their total
template <typename T>
__device__ __forceinline__ uint32_t holder_of(T excl, T x) {
    uint32_t e = 0;
#pragma unroll
    for (uint32_t b = 32u; b != 0u; b >>= 1)
        if (from_lane(excl, e + b) <= x) e += b;
    return e;
}

// The heads of up to 64 keys at once: lane e < turn passes key e, and key e is looked up in keys[0 .. n) by the lanes
// e W .. e W + W - 1, W the largest power of two with turn groups in a wave — one key: 64 pivots per round, two: 32 each, ...
// 33 and more: one lane each, a binary search.  Returns, in lane e < turn, the slot the key's segment begins at, whether the key
// is there at all, and its leader count tseg[head] (0 without the key; clamped to the end of the stream, which never happens in
// a finished graph: a segment ends inside the stream); in the other lanes present = false, count = 0.
struct Heads {
    uint64_t head;
    bool present;
    uint32_t count;
};
__device__ __forceinline__ Heads group_heads(const uint32_t *__restrict__ keys, uint64_t n, const uint32_t *__restrict__ tseg, uint32_t key, uint32_t turn) {
    const uint32_t lane = lane_id();
    uint32_t W = 64u;
    while (64u / W < turn) W >>= 1;
    const uint32_t grp = lane / W;
    const Bound b = group_lower_bound(keys, n, from_lane(key, grp), W, grp < turn);
    const uint32_t mine = lane < turn ? lane * W : 0u;  // (first lane of the group that looked this lane's key up)
    Heads r;
    r.head = from_lane(b.at, mine);
    const bool hit = from_lane((uint32_t)b.hit, mine) != 0u;  // (a shuffle: by every lane, before the lanes part)
    r.present = lane < turn && hit;
    r.count = r.present ? tseg[r.head] : 0u;
    if (r.count > n - r.head) r.count = (uint32_t)(n - r.head);
    return r;
}

// The edges of one turn of a successor list, one per lane: slots first .. first + turn - 1 of the edge stream.
__device__ __forceinline__ uint64_t edge_turn(const QueryGraph &G, uint64_t first, uint32_t turn) {
    const uint32_t lane = lane_id();
    return lane < turn && first + lane < G.E ? G.eval[first + lane] : 0ull;
}

// The candidate pairs (edge, leader of its target) of one turn of up to 64 edges — the core of searchSuccessors
// (PABruijnGraph.cpp:182-195).  Made from the turn's edges (lane e < turn: edge e, edge_turn's or loaded ahead by the caller; the
// other lanes' are not looked at): target code and step one edge per lane, the targets' heads and leader counts (group_heads),
// the exclusive sums of the counts.  The pairs are flattened in edge order, then position order; the caller deals them to the
// lanes 64 at a time (x = pb + lane for pb = 0, 64, ... below n_pairs) and pair(x) is the pair with index x: it belongs to the
// last edge whose exclusive sum is <= x (six shuffles), whose head, code and step come by shuffles again; then the leader's
// position, one load.  A lane with x >= n_pairs gets live = false and nothing of it is to be used.
struct SuccPairs {
    const uint64_t *tval;
    uint32_t tcode, step;  // lane e: edge e's target k-mer and step
    uint64_t th, ex;       // lane e: the head of that k-mer's leaders; the pairs of the edges before e
    uint64_t n_pairs;
    struct Pair {
        uint32_t code, step;  // the edge's target k-mer and step
        uint64_t slot, pos;   // the leader's tuple slot and its position
        bool live;
    };
    __device__ __forceinline__ SuccPairs(const QueryGraph &G, uint64_t ev, uint32_t turn) : tval(G.tval), tcode((uint32_t)(ev >> 32)), step((uint32_t)ev >> 1) {
        const Heads t = group_heads(G.tkey, G.T, G.tseg, tcode, turn);  // (absent: a k-mer without positions)
        th = t.head;
        ex = wave_excl_sum64((uint64_t)t.count, &n_pairs);
    }
    __device__ __forceinline__ Pair pair(uint64_t x) const {
        const uint32_t e = holder_of(ex, x);
        const uint64_t e_th = from_lane(th, e), e_ex = from_lane(ex, e);
        Pair p;
        p.step = from_lane(step, e);
        p.code = from_lane(tcode, e);
        p.live = x < n_pairs;
        p.slot = p.live ? e_th + (x - e_ex) : 0ull;
        p.pos = p.live ? tval[p.slot] : 0ull;
        return p;
    }
};

}  // namespace pagdev
