// query_graph.hpp — what the on-demand kernels over the FINISHED graph share (k_succ_query.hip: the successor lists of a list of
// vertices; k_walk_query.hip: walkStraight from a list of vertices): the arrays pag_process / pag_shard_import leave in the handle,
// the lower bound by groups of lanes that keeps a query's chain of dependent loads short, and the small lane helpers.
#pragma once
#include "pag_graph_impl.hpp"
#include "trav_device.hpp"

namespace pagdev {

struct QueryGraph {
    const uint32_t *tkey;
    const uint64_t *tval;
    const uint32_t *tseg;
    const uint32_t *ekey;
    const uint64_t *eval;
    const uint32_t *eseg;
    uint64_t T, E;
};

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
__device__ __forceinline__ uint64_t from_lane(uint64_t x, uint32_t l) {  // (the lane's number is a constant)
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)x, (int)l) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(x >> 32), (int)l) << 32);
}

}  // namespace pagdev
