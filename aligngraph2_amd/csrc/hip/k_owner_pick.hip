// k_owner_pick.hip — ONE owner's records straight out of an extraction: a stable stream compaction.
//
// A serial-rank run (pag_shard_run_serial, shard_serial.hip) extracts every read range once per owner and keeps only that
// owner's records of it.  pag_shard_extract_range + pag_shard_take_part do that by partitioning BOTH streams by owner — a
// stable radix pass that moves every record (and needs the ping-pong partners and the sort scratch) — and copying one stretch
// out.  Here the streams stay where extract_stage left them (SoA: u32 key, u64 value; the first n1 records are pass 1) and the
// survivors go straight to their places in the owner's receive buffers:
//
//   k_pick_mark    a thread per record on tiles of PK_TILE: survivors of pass 1 / pass 2 per tile (wave ballots + popcounts)
//   (exclusive prefix over the tiles: two scans of n / PK_TILE counters — tile offsets from a scan, as k_view_mark /
//    k_view_write do it: this code base's measured preference over look-back, profiles/r05_sort_variants.txt)
//   k_pick_write   the ballots again from the keys, a survivor's rank = tile offset + the ballots before its wave's + the
//                  popcount below its lane; pass 1 to one destination, pass 2 to the other.
// Keys are read twice, values by survivors only; the order is the ballots' — no atomic decides a place.  The pass boundary n1
// is a per-record test: it may fall anywhere in a wave or a tile.
#include <algorithm>
#include <initializer_list>

#include "dev_call.hpp"
#include "pag_device.hpp"
#include "pagraph_debug.h"

namespace pagdev {
namespace {

constexpr uint32_t PK_T = 256, PK_R = 8, PK_TILE = PK_T * PK_R, PK_W = PK_T / 64;

__global__ __launch_bounds__(PK_T) void k_pick_mark(const uint32_t *__restrict__ key, uint64_t n, uint64_t n1, uint32_t shift, uint32_t owner,
                                                    uint32_t *__restrict__ tile_c1, uint32_t *__restrict__ tile_c2, uint64_t n_tiles) {
    __shared__ uint32_t s_c1[PK_W], s_c2[PK_W];
    const uint32_t w = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t c1 = 0, c2 = 0;  // (wave-uniform)
#pragma unroll
        for (uint32_t r = 0; r < PK_R; ++r) {
            const uint64_t i = tile * PK_TILE + (uint64_t)r * PK_T + threadIdx.x;
            const bool hit = i < n && (key[i] >> shift) == owner;
            c1 += (uint32_t)__popcll(__ballot(hit && i < n1));
            c2 += (uint32_t)__popcll(__ballot(hit && i >= n1));
        }
        if (lane_id() == 0) {
            s_c1[w] = c1;
            s_c2[w] = c2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t a = 0, b = 0;
            for (uint32_t ww = 0; ww < PK_W; ++ww) {
                a += s_c1[ww];
                b += s_c2[ww];
            }
            tile_c1[tile] = a;
            tile_c2[tile] = b;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PK_T) void k_pick_write(const uint32_t *__restrict__ key, const uint64_t *__restrict__ val, uint64_t n, uint64_t n1,
                                                     uint32_t shift, uint32_t owner, const uint64_t *__restrict__ base1,
                                                     const uint64_t *__restrict__ base2, uint64_t n_tiles, uint32_t *__restrict__ okey,
                                                     uint64_t *__restrict__ oval, uint64_t at1, uint64_t at2) {
    __shared__ uint32_t s_n1[PK_R][PK_W], s_n2[PK_R][PK_W];  // survivors of (round, wave), then their exclusive prefix in the tile
    const uint32_t w = threadIdx.x >> 6;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t kx[PK_R];
        uint64_t m1[PK_R], m2[PK_R];
#pragma unroll
        for (uint32_t r = 0; r < PK_R; ++r) {
            const uint64_t i = tile * PK_TILE + (uint64_t)r * PK_T + threadIdx.x;
            kx[r] = i < n ? key[i] : 0u;
            const bool hit = i < n && (kx[r] >> shift) == owner;
            m1[r] = __ballot(hit && i < n1);
            m2[r] = __ballot(hit && i >= n1);
            if (lane_id() == 0) {
                s_n1[r][w] = (uint32_t)__popcll(m1[r]);
                s_n2[r][w] = (uint32_t)__popcll(m2[r]);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {  // (stream order inside a tile: round, then wave, then lane)
            uint32_t a = 0, b = 0;
            for (uint32_t r = 0; r < PK_R; ++r)
                for (uint32_t ww = 0; ww < PK_W; ++ww) {
                    const uint32_t x = s_n1[r][ww], y = s_n2[r][ww];
                    s_n1[r][ww] = a;
                    s_n2[r][ww] = b;
                    a += x;
                    b += y;
                }
        }
        __syncthreads();
        const uint64_t b1 = at1 + base1[tile], b2 = at2 + base2[tile];
        const uint64_t me = 1ull << lane_id();
#pragma unroll
        for (uint32_t r = 0; r < PK_R; ++r) {
            const uint64_t i = tile * PK_TILE + (uint64_t)r * PK_T + threadIdx.x;
            if (m1[r] & me) {
                const uint64_t p = b1 + s_n1[r][w] + (uint32_t)__popcll(m1[r] & lanemask_lt());
                okey[p] = kx[r];
                oval[p] = val[i];
            } else if (m2[r] & me) {
                const uint64_t p = b2 + s_n2[r][w] + (uint32_t)__popcll(m2[r] & lanemask_lt());
                okey[p] = kx[r];
                oval[p] = val[i];
            }
        }
        __syncthreads();  // (the next tile's counts go into the same LDS)
    }
}

uint64_t pick_tiles(uint64_t n) { return (n + PK_TILE - 1) / PK_TILE; }
size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// tmp: [tile_c1 u32][tile_c2 u32][base1 u64][base2 u64][totals 2 x u64][scan scratch]
size_t owner_pick_tmp_bytes(uint64_t n) {
    const uint64_t nt = pick_tiles(n) + 1;
    return 2 * up256(nt * 4) + 2 * up256(nt * 8) + 256 + up256(scan_tmp_bytes(nt)) + 256;
}

int owner_pick(const uint32_t *key, const uint64_t *val, uint64_t n, uint64_t n1, uint32_t shift, uint32_t owner, uint32_t *okey,
               uint64_t *oval, uint64_t cap, uint64_t at1, uint64_t at2, uint64_t *counts, void *tmp, hipStream_t s) {
    counts[0] = counts[1] = 0;
    if (shift > 31 || n1 > n) {
        set_error("owner_pick: shift %u, %llu of %llu records from pass 1", shift, (unsigned long long)n1, (unsigned long long)n);
        return PAG_EINVAL;
    }
    if (n == 0) return PAG_OK;
    const uint64_t n_tiles = pick_tiles(n), nt = n_tiles + 1;
    char *q = (char *)tmp;
    uint32_t *c1 = (uint32_t *)q;
    q += up256(nt * 4);
    uint32_t *c2 = (uint32_t *)q;
    q += up256(nt * 4);
    uint64_t *b1 = (uint64_t *)q;
    q += up256(nt * 8);
    uint64_t *b2 = (uint64_t *)q;
    q += up256(nt * 8);
    uint64_t *tot = (uint64_t *)q;
    q += 256;
    const unsigned grid = (unsigned)std::min<uint64_t>(n_tiles, 256 * 16);
    k_pick_mark<<<dim3(grid), dim3(PK_T), 0, s>>>(key, n, n1, shift, owner, c1, c2, n_tiles);
    int rc;
    if ((rc = scan_u32_to_u64(c1, b1, n_tiles, tot, q, s))) return rc;
    if ((rc = scan_u32_to_u64(c2, b2, n_tiles, tot + 1, q, s))) return rc;
    uint64_t h[2] = {0, 0};
    PAG_HIP_TRY(hipMemcpyAsync(h, tot, 16, hipMemcpyDeviceToHost, s));
    PAG_HIP_TRY(hipStreamSynchronize(s));
    counts[0] = h[0];
    counts[1] = h[1];
    if (h[0] + h[1] == 0) return PAG_OK;
    // both stretches inside the destination, and not into each other
    const bool fits = at1 <= cap && h[0] <= cap - at1 && at2 <= cap && h[1] <= cap - at2;
    const bool apart = h[0] == 0 || h[1] == 0 || at1 + h[0] <= at2 || at2 + h[1] <= at1;
    if (!fits || !apart || !okey || !oval) {
        set_error("owner_pick: %llu records at %llu and %llu at %llu do not fit a destination of %llu", (unsigned long long)h[0],
                  (unsigned long long)at1, (unsigned long long)h[1], (unsigned long long)at2, (unsigned long long)cap);
        return PAG_ERANGE;
    }
    k_pick_write<<<dim3(grid), dim3(PK_T), 0, s>>>(key, val, n, n1, shift, owner, b1, b2, n_tiles, okey, oval, at1, at2);
    PAG_HIP_TRY(hipGetLastError());
    return PAG_OK;
}

}  // namespace pagdev

using namespace pagdev;

// test hook (include/pagraph_debug.h): the compaction on caller-given HOST arrays.  out_key / out_val[cap] go to the device as
// they are and come back, so what the kernel did not write is what the caller put there.
extern "C" int pag_debug_owner_pick(const uint32_t *key, const uint64_t *val, uint64_t n, uint64_t n1, uint32_t shift, uint32_t owner,
                                    uint32_t *out_key, uint64_t *out_val, uint64_t cap, uint64_t at1, uint64_t at2, uint64_t *counts,
                                    int device) {
    if (!counts || (n && (!key || !val)) || (cap && (!out_key || !out_val))) return PAG_EINVAL;
    DevCall D("pag_debug_owner_pick");
    uint32_t *d_key = nullptr, *d_ok = nullptr;
    uint64_t *d_val = nullptr, *d_ov = nullptr;
    char *d_tmp = nullptr;
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault)) || (rc = D.up(key, n, &d_key, 16)) || (rc = D.up(val, n, &d_val, 16)) || (rc = D.up((const uint32_t *)out_key, cap, &d_ok, 16)) ||
        (rc = D.up((const uint64_t *)out_val, cap, &d_ov, 16)) || (rc = D.alloc(&d_tmp, owner_pick_tmp_bytes(n))))
        return rc;
    if ((rc = owner_pick(d_key, d_val, n, n1, shift, owner, d_ok, d_ov, cap, at1, at2, counts, d_tmp, D.s)) || (rc = D.down(out_key, d_ok, cap)) ||
        (rc = D.down(out_val, d_ov, cap)))
        return rc;
    return D.finish();
}
