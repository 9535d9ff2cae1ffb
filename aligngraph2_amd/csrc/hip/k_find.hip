// k_find.hip — pag_find_all_batch: the graph's vertices along a LIST of sequences.
//
// PABruijnGraph::findAll (PABruijnGraph.cpp:339-353, through fromCode :90-96; find :334-337 is a sequence of k bases) for every
// sequence of a list, each in the strand the caller names, straight from the arrays pag_process / pag_shard_import leave in the
// handle — the solid bitmap and the k-mer-sorted tuple stream with its in-place segment results (the layout pag_export_csr
// reads): no traversal view.  A hit is a searched offset whose k-mer is in the solid set; its vertices are the clustered positions
// of that k-mer's node, slots head .. head + tseg[head] of the stream, each with its count from tcnt.
//
// One wavefront per tile of 1 024 offsets of one (sequence, strand), every wave on its own (no block barrier, no LDS); the
// tile list comes from the host (find_plan.hpp):
//   1. the k-mer codes: lane l holds the offsets 16 l .. 16 l + 15 of the tile in one 64-bit window over the packed words, as
//      K1's LaneWindow does (k1_extract.hip) — forward: the groups reversed once, a code is a shift and a mask; reverse
//      (CompressedSeq::toString(false): the complement read back to front): the window from the other end, a code is a shift,
//      a complement and a mask;
//   2. the solid test: one gather from the bitmap per offset, sixteen in flight per lane; a 16-bit mask per lane;
//   3. the hits in offset order, 64 at a time: the exclusive sums of the lanes' hit counts say which lane holds hit h (six
//      shuffles), its mask which of its offsets it is, its window (shuffles again) the code — no staging array;
//   4. their nodes: lower bounds in tkey by groups of lanes (group_heads, query_graph.hpp): with n hits in the turn
//      the wave splits into groups of 64 / n lanes, each group its own search with that many pivots per round — a single k-mer
//      (find): 64 pivots, five rounds over 10^8 slots; 33 and more: one lane each, a binary search; then tseg[head], one load;
//   5. (fill) the hits to their places, then the (hit, position) pairs of the turn flattened in hit order, then position order,
//      and dealt to the lanes 64 at a time, as k_succ_query deals candidate pairs: a node of 300 positions and 60 nodes of one
//      position cost the same per vertex.
// The kernel runs twice: it counts hits and vertices per tile, the counts are scanned into tile bases (the vertex counts as two
// 32-bit halves: a tile of a homopolymer can name one heavy node 1 024 times), it runs again and fills — the search is repeated,
// nothing but twelve bytes per TILE is kept between the passes (the two passes of a call: query_call.hpp).  hit_off[], hits[] and
// vert[] are a function of the inputs alone.
// The walker's "used" marks play no part: this is the reference's call on a fresh graph.
#include <algorithm>

#include "find_plan.hpp"
#include "query_call.hpp"
#include "query_graph.hpp"

namespace pagdev {
namespace {

struct FindHit {  // pag_find_hit
    uint32_t offset, code;
    uint64_t first;
    uint32_t n_pos, reserved;
};
struct FindVertex {  // pag_find_vertex
    uint64_t pos;
    uint32_t abundance, reserved;
};
static_assert(sizeof(FindHit) == sizeof(pag_find_hit) && sizeof(FindVertex) == sizeof(pag_find_vertex), "pag_find_hit / pag_find_vertex layout");

struct FindArgs {
    // the sequences and their tiles
    const uint8_t *packed;
    const uint64_t *byte_off;
    const uint32_t *len;
    const FindTile *tiles;
    uint64_t n_tiles;
    // the handle
    const uint32_t *solid_bits;
    int all_solid;
    uint32_t k;
    QueryGraph G;
    // count pass: per tile its hits and its vertices (low and high half)
    uint32_t *hcnt, *vlo, *vhi;
    // fill pass: the scans of the three, the buffers (vert null: hits only) and their sizes
    const uint64_t *hbase, *vlo_base, *vhi_base;
    FindHit *hits;
    uint64_t n_hits;
    FindVertex *vert;
    uint64_t n_vert;
};

// The window of a lane's sixteen offsets p0 .. p0 + 15 (K1's LaneWindow, k1_extract.hip): forward strand — the 64 bits from
// base p0 on with their 2-bit groups reversed, a code is a shift and a mask; reverse strand — the 64 bits from the base the
// LAST of the sixteen k-mers begins with in the stored strand, a code is a shift, a complement and a mask.
struct Window {
    uint64_t x = 0;
    uint32_t s0 = 0;  // forward: shift of offset 0, 2 (32 - k); reverse: twice what the window's start was clamped by (<= 0)
    __device__ __forceinline__ uint32_t code(uint32_t strand, uint32_t kmask, uint32_t j) const {
        if (strand == 0) return (uint32_t)(x >> (s0 - 2u * j)) & kmask;
        return ~(uint32_t)(x >> ((2u * (15u - j) + s0) & 63u)) & kmask;
    }
};
__device__ __forceinline__ Window lane_window(const uint32_t *__restrict__ words, uint32_t strand, uint32_t len, uint32_t k, uint32_t p0,
                                              uint32_t n_mine) {
    Window L;
    if (!n_mine) return L;  // lanes past the end of the strand must not touch memory
    if (strand == 0) {
        const uint32_t w0 = p0 >> 4;
        const uint32_t lo = words[w0], hi = words[w0 + 1];
        L.x = ((uint64_t)rev2(lo) << 32) | (uint64_t)rev2(hi);
        L.s0 = 2u * (32u - k);
    } else {
        const int64_t a0 = (int64_t)len - (int64_t)k - (int64_t)p0 - 15;
        const uint32_t a1 = a0 > 0 ? (uint32_t)a0 : 0u;
        const uint32_t w = a1 >> 4, sh = (a1 & 15u) * 2u;
        const uint64_t lo64 = (uint64_t)words[w] | ((uint64_t)words[w + 1] << 32);
        L.x = lo64 >> sh;
        if (sh) L.x |= (uint64_t)words[w + 2] << (64 - sh);
        L.s0 = (uint32_t)((a0 - (int64_t)a1) * 2);
    }
    return L;
}

// FILL = false: hcnt / vlo / vhi[t] = hits and vertices of tile t.  FILL = true: the hits of tile t to hits[hbase[t] ..), their
// vertices to vert[vbase[t] ..) (nothing is written at or beyond n_hits / n_vert)
template <bool FILL>
__global__ void __launch_bounds__(256) k_find(FindArgs A) {
    const uint32_t lane = lane_id(), waves = blockDim.x / 64u;
    const uint64_t n_waves = (uint64_t)gridDim.x * waves;
    const uint32_t k = A.k, kmask = k >= 16u ? 0xFFFFFFFFu : (1u << (2u * k)) - 1u;
    for (uint64_t t = (uint64_t)blockIdx.x * waves + uniform_u32(threadIdx.x / 64u); t < A.n_tiles; t += n_waves) {
        const FindTile tile = A.tiles[t];
        const uint32_t strand = tile.at & 1u, t0 = tile.at & ~(FIND_TILE - 1u);
        const uint32_t len = A.len[tile.seq];
        const uint32_t *__restrict__ words = (const uint32_t *)(A.packed + A.byte_off[tile.seq]);
        const uint32_t rest = len - k + 1u - t0;  // offsets from t0 on: 1 or more (find_cut)
        const uint32_t n_mine = lane * 16u >= rest ? 0u : (rest - lane * 16u > 16u ? 16u : rest - lane * 16u);
        const Window win = lane_window(words, strand, len, k, t0 + lane * 16u, n_mine);
        uint32_t mask = 0;  // bit j: offset t0 + 16 lane + j is a hit
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            bool solid = j < n_mine;
            if (solid && !A.all_solid) {
                const uint32_t c = win.code(strand, kmask, j);
                solid = (A.solid_bits[c >> 5] >> (c & 31u)) & 1u;
            }
            mask |= (solid ? 1u : 0u) << j;
        }
        uint32_t tile_hits;
        const uint32_t hits_before = wave_excl_sum((uint32_t)__popc(mask), &tile_hits);
        tile_hits = uniform_u32(tile_hits);
        uint64_t hb = 0, vb = 0;
        if (FILL) {
            if (tile_hits == 0u) continue;
            hb = A.hbase[t];
            vb = A.vlo_base[t] + (A.vhi_base[t] << 32);
        }
        uint64_t tile_verts = 0;
        for (uint32_t rb = 0; rb < tile_hits; rb += 64u) {
            const uint32_t turn = tile_hits - rb < 64u ? tile_hits - rb : 64u;
            const bool have = lane < turn;
            // hit rb + lane of the tile: whose it is, which of that lane's offsets, its code
            const uint32_t h = rb + lane;
            const uint32_t o = holder_of(hits_before, h);
            const uint32_t o_mask = from_lane(mask, o), o_nth = h - from_lane(hits_before, o);
            Window ow;
            ow.x = from_lane(win.x, o);
            ow.s0 = from_lane(win.s0, o);
            uint32_t m = have ? o_mask : 1u;
#pragma unroll
            for (uint32_t s = 0; s < 15u; ++s)
                if (have && s < o_nth) m &= m - 1u;
            const uint32_t j = (uint32_t)__ffs((int)m) - 1u;  // (a lane that has a hit: the mask has more than o_nth bits)
            const uint32_t code = have ? ow.code(strand, kmask, j & 15u) : 0u;
            // the hits' nodes (absent: a solid k-mer nothing was placed on)
            const Heads node = group_heads(A.G.tkey, A.G.T, A.G.tseg, code, turn);
            uint64_t n_pairs;
            const uint64_t ex = wave_excl_sum64((uint64_t)node.count, &n_pairs);
            if (FILL) {
                const uint64_t first = vb + tile_verts;
                if (have && hb + h < A.n_hits) {
                    FindHit r;
                    r.offset = t0 + o * 16u + j;
                    r.code = code;
                    r.first = first + ex;
                    r.n_pos = node.count;
                    r.reserved = 0u;
                    A.hits[hb + h] = r;
                }
                // the (hit, position) pairs of the turn, flattened: pair x belongs to the last hit whose exclusive sum is <= x
                for (uint64_t pb = 0; A.vert && pb < n_pairs; pb += 64u) {
                    const uint64_t x = pb + lane;
                    const uint32_t e = holder_of(ex, x);
                    const uint64_t e_head = from_lane(node.head, e), e_ex = from_lane(ex, e);
                    if (x < n_pairs && first + x < A.n_vert) {
                        const uint64_t slot = e_head + (x - e_ex);
                        FindVertex v;
                        v.pos = A.G.tval[slot];
                        v.abundance = A.G.tcnt[slot];
                        v.reserved = 0u;
                        A.vert[first + x] = v;
                    }
                }
            }
            tile_verts += n_pairs;
        }
        if (!FILL && lane == 0u) {
            A.hcnt[t] = tile_hits;
            A.vlo[t] = (uint32_t)tile_verts;
            A.vhi[t] = (uint32_t)(tile_verts >> 32);
        }
    }
}

// hit_off[i] = the hit base of sequence i's first tile (i = n_seqs: of the end of the list); tot[0 / 1] = hits, vertices
__global__ void k_find_offsets(const uint64_t *__restrict__ seq_tile, uint64_t n_seqs, uint64_t n_tiles, const uint64_t *__restrict__ hbase,
                               const uint64_t *__restrict__ vlo_base, const uint64_t *__restrict__ vhi_base, uint64_t *__restrict__ hit_off,
                               uint64_t *__restrict__ tot) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_seqs) hit_off[i] = hbase[seq_tile[i]];
    if (i == 0) {
        tot[0] = hbase[n_tiles];
        tot[1] = vlo_base[n_tiles] + (vhi_base[n_tiles] << 32);
    }
}

// the temporary device memory of a call that is allocated before the counts are known
struct FindLayout {
    Carver c;
    size_t packed, byte_off, len, seq_tile, tiles, hcnt, vlo, vhi, hbase, vlo_base, vhi_base, scan, hit_off, tot;
    FindLayout(uint64_t n_seqs, uint64_t packed_bytes, uint64_t n_tiles)
        : packed(c.take<uint8_t>(packed_bytes + 64)),  // (the padding pag_seqs promises behind the last sequence, zeroed)
          byte_off(c.take<uint64_t>(n_seqs)), len(c.take<uint32_t>(n_seqs)), seq_tile(c.take<uint64_t>(n_seqs + 1)), tiles(c.take<FindTile>(n_tiles)),
          hcnt(c.take<uint32_t>(n_tiles)), vlo(c.take<uint32_t>(n_tiles)), vhi(c.take<uint32_t>(n_tiles)), hbase(c.take<uint64_t>(n_tiles + 1)),
          vlo_base(c.take<uint64_t>(n_tiles + 1)), vhi_base(c.take<uint64_t>(n_tiles + 1)), scan(c.take<char>(scan_tmp_bytes(n_tiles))),
          hit_off(c.take<uint64_t>(n_seqs + 1)), tot(c.take<uint64_t>(2)) {}
};

}  // namespace
}  // namespace pagdev

using namespace pagdev;

extern "C" {

uint64_t pag_find_all_batch_bytes(uint64_t n_seqs, uint64_t packed_bytes, uint64_t n_hits, uint64_t n_vert) {
    if (!n_seqs) return 0;
    // (tiles: one per 1 024 offsets and a last one per sequence; sequences that share no byte of `packed` have 4 bases a byte at most)
    return FindLayout(n_seqs, packed_bytes, n_seqs + packed_bytes / (FIND_TILE / 4)).c.bytes + n_hits * sizeof(pag_find_hit) + n_vert * sizeof(pag_find_vertex);
}

int pag_find_all_batch(const pag_graph *g, const pag_seqs *seqs, const uint8_t *reverse, uint64_t *hit_off, pag_find_hit *hits, uint64_t hit_cap,
                       pag_find_vertex *vert, uint64_t vert_cap, uint64_t *n_hits, uint64_t *n_vert, double *ms_kernels) {
    if (n_hits) *n_hits = 0;
    if (n_vert) *n_vert = 0;
    if (ms_kernels) *ms_kernels = 0;
    if (!g || !seqs || !hit_off || !n_hits || !n_vert || (!hits && hit_cap) || (!vert && vert_cap)) {
        set_error("pag_find_all_batch: a null handle, sequence list, hit_off or total, or a null buffer with room");
        return PAG_EINVAL;
    }
    const uint64_t n = seqs->n_seqs;
    if (n && (!seqs->byte_off || !seqs->len || !seqs->packed)) {
        set_error("pag_find_all_batch: the sequence list lacks byte_off, len or packed");
        return PAG_EINVAL;
    }
    int rc = check_finished_graph(g, "pag_find_all_batch", "position of its k-mers");
    if (rc) return rc;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || g->device >= n_dev) {
        (void)hipGetLastError();
        set_error("pag_find_all_batch: no HIP device");
        return PAG_ENODEV;
    }
    hit_off[0] = 0;
    if (n == 0) return PAG_OK;
    if (n > 0xFFFFFFFFull) {
        set_error("pag_find_all_batch: %llu sequences, at most 2^32 - 1 in a call", (unsigned long long)n);
        return PAG_EINVAL;
    }
    FindPlan plan;
    if (!find_check(seqs->byte_off, seqs->len, n, seqs->packed_bytes, &plan)) {
        set_error("pag_find_all_batch: sequence %llu: %s", (unsigned long long)plan.bad, plan.why);
        return PAG_EINVAL;
    }
    find_cut(seqs->len, reverse, n, g->k, &plan);
    const uint64_t n_tiles = plan.tiles.size();
    if (n_tiles == 0) {  // (no sequence has k bases)
        std::fill(hit_off, hit_off + n + 1, (uint64_t)0);
        return PAG_OK;
    }
    QueryCall B("pag_find_all_batch");
    const FindLayout L(n, seqs->packed_bytes, n_tiles);
    if ((rc = B.open(g, L.c.bytes))) return rc;
    const hipStream_t s = B.s;
    uint64_t *d_seq_tile = B.at<uint64_t>(L.seq_tile), *d_hbase = B.at<uint64_t>(L.hbase), *d_vlo_base = B.at<uint64_t>(L.vlo_base),
             *d_vhi_base = B.at<uint64_t>(L.vhi_base), *d_hit_off = B.at<uint64_t>(L.hit_off), *d_tot = B.at<uint64_t>(L.tot);
    uint8_t *d_packed = B.at<uint8_t>(L.packed);
    char *d_scan = B.at<char>(L.scan);
    FindArgs A{};
    A.packed = d_packed;
    A.byte_off = B.at<uint64_t>(L.byte_off);
    A.len = B.at<uint32_t>(L.len);
    A.tiles = B.at<FindTile>(L.tiles);
    A.n_tiles = n_tiles;
    A.solid_bits = g->solid_bits;
    A.all_solid = g->all_solid;
    A.k = g->k;
    A.G = query_graph(g);
    A.hcnt = B.at<uint32_t>(L.hcnt);
    A.vlo = B.at<uint32_t>(L.vlo);
    A.vhi = B.at<uint32_t>(L.vhi);
    const dim3 grid(wave_per_item_grid(n_tiles));  // (a wave per tile)
    PAG_HIP_TRY(hipMemsetAsync(d_packed + seqs->packed_bytes, 0, 64, s));
    if (seqs->packed_bytes) PAG_HIP_TRY(hipMemcpyAsync(d_packed, seqs->packed, seqs->packed_bytes, hipMemcpyHostToDevice, s));
    PAG_HIP_TRY(hipMemcpyAsync(B.at<uint64_t>(L.byte_off), seqs->byte_off, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    PAG_HIP_TRY(hipMemcpyAsync(B.at<uint32_t>(L.len), seqs->len, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    PAG_HIP_TRY(hipMemcpyAsync(d_seq_tile, plan.seq_tile.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    PAG_HIP_TRY(hipMemcpyAsync(B.at<FindTile>(L.tiles), plan.tiles.data(), n_tiles * sizeof(FindTile), hipMemcpyHostToDevice, s));
    if ((rc = B.begin(QueryCall::COUNT))) return rc;
    k_find<false><<<grid, dim3(256), 0, s>>>(A);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = scan_u32_to_u64(A.hcnt, d_hbase, n_tiles, d_hbase + n_tiles, d_scan, s))) return rc;
    if ((rc = scan_u32_to_u64(A.vlo, d_vlo_base, n_tiles, d_vlo_base + n_tiles, d_scan, s))) return rc;
    if ((rc = scan_u32_to_u64(A.vhi, d_vhi_base, n_tiles, d_vhi_base + n_tiles, d_scan, s))) return rc;
    k_find_offsets<<<dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s>>>(d_seq_tile, n, n_tiles, d_hbase, d_vlo_base, d_vhi_base, d_hit_off, d_tot);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = B.end(QueryCall::COUNT))) return rc;
    uint64_t tot[2] = {0, 0};
    PAG_HIP_TRY(hipMemcpyAsync(hit_off, d_hit_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PAG_HIP_TRY(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, s));
    if ((rc = B.done(QueryCall::COUNT, ms_kernels))) return rc;
    *n_hits = tot[0];
    *n_vert = tot[1];
    if (tot[0] > hit_cap || (vert && tot[1] > vert_cap)) {
        set_error("pag_find_all_batch: %llu hits and %llu vertices, room for %llu and %llu", (unsigned long long)tot[0], (unsigned long long)tot[1],
                  (unsigned long long)hit_cap, (unsigned long long)vert_cap);
        return PAG_ERANGE;
    }
    if (tot[0] == 0) return PAG_OK;
    if ((rc = B.alloc(&A.hits, tot[0]))) return rc;
    if (vert && tot[1] && (rc = B.alloc(&A.vert, tot[1]))) return rc;
    A.hbase = d_hbase;
    A.vlo_base = d_vlo_base;
    A.vhi_base = d_vhi_base;
    A.n_hits = tot[0];
    A.n_vert = A.vert ? tot[1] : 0;
    if ((rc = B.begin(QueryCall::FILL))) return rc;
    k_find<true><<<grid, dim3(256), 0, s>>>(A);
    PAG_HIP_TRY(hipGetLastError());
    if ((rc = B.end(QueryCall::FILL))) return rc;
    PAG_HIP_TRY(hipMemcpyAsync(hits, A.hits, tot[0] * sizeof(pag_find_hit), hipMemcpyDeviceToHost, s));
    if (A.vert) PAG_HIP_TRY(hipMemcpyAsync(vert, A.vert, tot[1] * sizeof(pag_find_vertex), hipMemcpyDeviceToHost, s));
    return B.done(QueryCall::FILL, ms_kernels);
}

}  // extern "C"
