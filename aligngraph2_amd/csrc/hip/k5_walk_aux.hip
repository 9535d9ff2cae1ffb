// k5_walk_aux.hip — what runs around the walker waves (k5_travel.hip): id ranges of the strands, seed scans (searchPANode /
// searchPANode2, PAGraph/src/tools/graph/PAlgorithm.tcc:300-365), checkpoints of the segment jobs, the kernels that hand finished
// paths to the host (packed with their block tables, gathered into pag_path_node records), the global visited marks of a
// committed walk, the clearing of a batch of job buffers, the last round of a leaping contig put together on the device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pag_device.hpp"
#include "pag_travel.hpp"
#include "trav_device.hpp"
#include "trav_hook.hpp"

namespace pagdev {


// [first, last) new-id range of the vertices whose contig coordinate lies in [lo, hi)
__global__ void k_ranges(TravGraph G, TravContig *ctgs, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto lower = [&](uint32_t x) {
        uint64_t lo = 0, hi = G.n_pos;
        while (lo < hi) {
            uint64_t mid = (lo + hi) >> 1;
            if ((uint32_t)(G.upos[mid] >> 32) < x) lo = mid + 1;
            else hi = mid;
        }
        return (uint32_t)lo;
    };
    ctgs[i].in_lo = lower(ctgs[i].ctg_left);
    ctgs[i].in_hi = lower(ctgs[i].ctg_right);
    ctgs[i].g_lo = ctgs[i].in_lo;
    ctgs[i].g_hi = ctgs[i].in_hi;
}

// first new id whose contig coordinate is >= coords[i] (the vertices with a coordinate are ordered by it)
__global__ void k_id_bounds(TravGraph G, const uint32_t *__restrict__ coords, uint32_t n, uint32_t *__restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = coords[i];
    uint64_t lo = 0, hi = G.n_pos;
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        if ((uint32_t)(G.upos[mid] >> 32) < x) lo = mid + 1;
        else hi = mid;
    }
    out[i] = (uint32_t)lo;
}

// =================================================================================================
// seeds
// =================================================================================================
// searchPANode(onlyFirst = true) (PAlgorithm.tcc:300-327): the first contig k-mer one of whose positions
// lies on this contig strand within `dev` of the k-mer's own offset; all such positions of that k-mer.
// One wave per contig.  out[0] = count, then (vertex, node) pairs.
__global__ __launch_bounds__(64) void k_seed_first(TravGraph G, const TravContig *__restrict__ ctgs, uint32_t n_ctgs_sel,
                                                   uint64_t dev, uint32_t *__restrict__ out, uint32_t out_stride) {
    const uint32_t c = blockIdx.x;
    if (c >= n_ctgs_sel) return;
    const TravContig C = ctgs[c];
    const uint32_t lane = lane_id();
    uint32_t *o = out + (uint64_t)c * out_stride;
    uint32_t found = 0;
    for (uint32_t base = 0; base < C.n_kmers && !found; base += 64) {
        uint32_t i = base + lane;
        bool hit = false;
        uint32_t node = PAG_NONE;
        if (i < C.n_kmers) {
            node = C.nodes[i];
            if (node != PAG_NONE) {
                for (uint32_t p = G.npos_off[node]; p < G.npos_off[node + 1] && !hit; ++p) {
                    uint32_t pc = (uint32_t)(G.vpos[p] >> 32);
                    if (pc >= C.ctg_left && pc < C.ctg_right) {
                        uint64_t off = pc - C.ctg_left;
                        uint64_t d = off > i ? off - i : (uint64_t)i - off;
                        hit = d <= dev;
                    }
                }
            }
        }
        uint64_t m = __ballot(hit);
        if (m) {
            int src = __ffsll((long long)m) - 1;
            if ((int)lane == src) {
                uint32_t n = 0;
                for (uint32_t p = G.npos_off[node]; p < G.npos_off[node + 1]; ++p) {
                    uint32_t pc = (uint32_t)(G.vpos[p] >> 32);
                    if (pc >= C.ctg_left && pc < C.ctg_right) {
                        uint64_t off = pc - C.ctg_left;
                        uint64_t d = off > i ? off - i : (uint64_t)i - off;
                        if (d <= dev && 1 + 2 * n + 1 < out_stride) {
                            o[1 + 2 * n] = p;
                            o[2 + 2 * n] = i;
                            ++n;
                        }
                    }
                }
                o[0] = n;
            }
            found = 1;
        }
    }
    if (!found && lane == 0) o[0] = 0;
}

// searchPANode2 (PAlgorithm.tcc:329-365): every (contig offset in [left, right], position) pair whose
// position lies on this strand within `dev` of `pos`, in order.  Duplicates of a vertex are removed on
// the host (first occurrence wins).  TRAV_SEED_PARTS waves per request, each scanning one part of the offset range
// (the window spans 1000 x deviation offsets on either side); part p of request r writes out[(r * PARTS + p) * stride]:
// [0] = count, then vertex ids; the host concatenates the parts in order.
__global__ __launch_bounds__(64) void k_seed_window(TravGraph G, const TravContig *__restrict__ ctgs,
                                                    const TravSeedReq *__restrict__ reqs, uint32_t n_req, uint64_t dev,
                                                    uint32_t *__restrict__ out, uint32_t out_stride) {
    const uint32_t r = blockIdx.x, part = blockIdx.y;
    if (r >= n_req) return;
    const TravSeedReq R = reqs[r];
    const TravContig C = ctgs[R.ctg];
    const uint32_t lane = lane_id();
    uint32_t *o = out + ((uint64_t)r * TRAV_SEED_PARTS + part) * out_stride;
    uint32_t n_out = 0;
    const uint64_t right_all = R.right < (uint64_t)C.n_kmers ? R.right + 1 : C.n_kmers;  // exclusive
    const uint64_t span = right_all > R.left ? right_all - R.left : 0;
    const uint64_t per = ((span + TRAV_SEED_PARTS - 1) / TRAV_SEED_PARTS + 63) & ~63ull;  // offsets per part (whole wave rows)
    const uint64_t left = R.left + (uint64_t)part * per;
    const uint64_t right = left + per < right_all ? left + per : right_all;
    for (uint64_t base = left; base < right; base += 64) {
        uint64_t i = base + lane;
        uint32_t node = i < right ? C.nodes[i] : PAG_NONE;
        uint32_t p0 = 0, p1 = 0;
        if (node != PAG_NONE) {
            p0 = G.npos_off[node];
            p1 = G.npos_off[node + 1];
        }
        // lanes emit in lane order, positions in order: serialise over the lanes that have matches
        // filterPANodes (PAlgorithm.cpp:97-105): vertices of the contig's globalUniqueTable are dropped here, on the device
        // (a per-vertex predicate: applying it before the host removes duplicates gives the same list)
        auto visited = [&](uint32_t p) -> bool {
            if (!C.gbits) return false;
            const uint32_t u = G.newid[p];
            if (u >= C.g_lo && u < C.g_hi) return ((C.gbits[(u - C.g_lo) >> 5] >> ((u - C.g_lo) & 31u)) & 1u) != 0u;
            return C.gset ? hs_has(C.gset, C.gmask, u) : false;
        };
        uint32_t cnt = 0;
        for (uint32_t p = p0; p < p1; ++p) {
            uint32_t pc = (uint32_t)(G.vpos[p] >> 32);
            if (pc >= C.ctg_left && pc < C.ctg_right) {
                uint64_t off = pc - C.ctg_left;
                uint64_t d = off > R.pos ? off - R.pos : R.pos - off;
                cnt += (d <= dev && !visited(p)) ? 1u : 0u;
            }
        }
        uint32_t tot;
        uint32_t ex = wave_excl_sum(cnt, &tot);
        uint32_t w = n_out + ex;
        for (uint32_t p = p0; p < p1 && cnt; ++p) {
            uint32_t pc = (uint32_t)(G.vpos[p] >> 32);
            if (pc >= C.ctg_left && pc < C.ctg_right) {
                uint64_t off = pc - C.ctg_left;
                uint64_t d = off > R.pos ? off - R.pos : R.pos - off;
                if (d <= dev && !visited(p)) {
                    if (1 + w < out_stride) o[1 + w] = p;
                    ++w;
                }
            }
        }
        n_out += tot;
    }
    if (lane == 0) o[0] = n_out;
}

// Checkpoints of the segment-parallel walk (k5_travel_host.hip): for every request (contig, contig offset) the most
// abundant vertex that lies ON the contig strand (its k-mer is the contig's k-mer at offset i and its contig coordinate
// is within `dev` of i, like a seed of searchPANode) for i in [left, right], and that is not in the contig's global
// visited set.  Ties: the lowest offset, then position order.  One wave per request; out = (old vertex id, contig
// coordinate, abundance) or (PAG_NONE, 0, 0).  Which vertex is picked has no influence on the results of the
// traversal, only on how soon the walk that arrives from behind meets the piece started here.
// The visited test reads the bitmap alone: a vertex on the strand has its new id in [g_lo, g_hi) as k_ranges leaves them, so the
// hash set holds none of the candidates.  The tie-breaks are 20-bit fields: they wrap for a window of more than 2^20 offsets or a
// k-mer with more than 2^20 positions, and the pick among equal abundances is then another one (still a valid checkpoint).
__global__ __launch_bounds__(64) void k_checkpoints(TravGraph G, const TravContig *__restrict__ ctgs, const TravSeedReq *__restrict__ reqs,
                                                    uint32_t n_req, uint64_t dev, uint32_t *__restrict__ out) {
    const uint32_t r = blockIdx.x;
    if (r >= n_req) return;
    const TravSeedReq R = reqs[r];
    const TravContig C = ctgs[R.ctg];
    const uint32_t lane = lane_id();
    const uint64_t right = R.right < (uint64_t)C.n_kmers ? R.right + 1 : C.n_kmers;  // exclusive
    uint64_t best = 0;  // abundance << 40 | (0xFFFFF - (offset - left)) << 20 | (0xFFFFF - position rank): larger is better
    uint32_t best_v = PAG_NONE, best_pc = 0;
    for (uint64_t base = R.left; base < right; base += 64) {
        const uint64_t i = base + lane;
        const uint32_t node = i < right ? C.nodes[i] : PAG_NONE;
        if (node == PAG_NONE) continue;
        const uint32_t p0 = G.npos_off[node], p1 = G.npos_off[node + 1];
        for (uint32_t p = p0; p < p1; ++p) {
            const uint32_t pc = (uint32_t)(G.vpos[p] >> 32);
            if (pc < C.ctg_left || pc >= C.ctg_right) continue;
            const uint64_t off = pc - C.ctg_left;
            const uint64_t d = off > i ? off - i : i - off;
            if (d > dev) continue;
            const uint32_t u = G.newid[p];
            if (C.gbits && u >= C.g_lo && u < C.g_hi && ((C.gbits[(u - C.g_lo) >> 5] >> ((u - C.g_lo) & 31u)) & 1u)) continue;
            const uint64_t key = ((uint64_t)G.vcnt[p] << 40) | ((uint64_t)(0xFFFFFu - (uint32_t)((i - R.left) & 0xFFFFFu)) << 20) |
                                 (uint64_t)(0xFFFFFu - ((p - p0) & 0xFFFFFu));
            if (key > best) {
                best = key;
                best_v = p;
                best_pc = pc;
            }
        }
    }
    for (int d2 = 32; d2 >= 1; d2 >>= 1) {
        const uint64_t ob = __shfl_xor(best, d2, 64);
        const uint32_t ov = (uint32_t)__shfl_xor((int)best_v, d2, 64), op = (uint32_t)__shfl_xor((int)best_pc, d2, 64);
        if (ob > best) {
            best = ob;
            best_v = ov;
            best_pc = op;
        }
    }
    if (lane == 0) {
        out[3 * r] = best_v;
        out[3 * r + 1] = best_pc;
        out[3 * r + 2] = (uint32_t)(best >> 40);
    }
}

// The new parts of the sequences of a batch of finished jobs, packed for ONE copy to the host: per job its vertices (new
// ids), its steps and the contig coordinates of its vertices (+ the two words of the iteration log of a TRAV_MODE_LEAP
// job), each `len` words, at out + off — and behind them the job's BLOCK TABLES (walk_stitch.hpp: AGG_WORDS words per 64
// entries, + AGG_XWORDS for a leap job): a wave copies 64 consecutive entries per turn and reduces them while it holds them.
__global__ void k_pack_paths(TravGraph G, const TravPackDesc *__restrict__ descs, uint32_t n, uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.y;
    if (j >= n) return;
    const TravPackDesc D = descs[j];
    uint32_t *o = out + D.off;
    const uint32_t lane = lane_id();
    const uint64_t n_arrays = D.seq_x ? 5 : 3;
    uint32_t *agg = o + n_arrays * D.len;
    uint32_t *xagg = agg + ((D.len + 63) / 64) * 5;
    // (wave-uniform loop: every lane of a wave takes part in the reductions of its block)
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < D.len; i0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = i0 + lane;
        const bool valid = i < D.len;
        uint32_t v = 0, st = 0, c = 0, xl = 0, xh = 0;
        if (valid) {
            v = D.seq_v[i];
            st = D.seq_s[i];
            c = (uint32_t)(G.upos[v] >> 32);
            o[i] = v;
            o[D.len + i] = st;
            o[2 * D.len + i] = c;
            if (D.seq_x) {
                const uint64_t x = D.seq_x[i];
                xl = (uint32_t)x;
                xh = (uint32_t)(x >> 32);
                o[3 * D.len + i] = xl;
                o[4 * D.len + i] = xh;
            }
        }
        const uint32_t mx = wave_max_u32(valid ? c : 0u);
        const uint32_t m0 = wave_max_u32(valid && c == 0u ? v + 1u : 0u);
        const uint32_t lo = wave_min_u32(valid ? c : 0xFFFFFFFFu);
        const uint32_t lnz = wave_min_u32(valid && c != 0u ? c : 0xFFFFFFFFu);
        const uint32_t sum = wave_sum(valid ? st : 0u);
        const uint64_t blk = i0 >> 6;
        if (lane == 0) {
            uint32_t *a = agg + blk * 5;
            a[0] = mx;
            a[1] = m0;
            a[2] = lo;
            a[3] = lnz;
            a[4] = sum;
        }
        if (D.seq_x) {
            const bool bd = valid && (xh >> 31) != 0u;
            const uint32_t elow = wave_min_u32(bd ? (xh & 0x7FFFFFFFu) : 0xFFFFFFFFu);
            const uint32_t xm0 = wave_min_u32(bd ? xl : 0xFFFFFFFFu);
            if (lane == 0) {
                xagg[blk * 2] = elow;
                xagg[blk * 2 + 1] = xm0;
            }
        }
    }
}

// contig coordinates of a path (new ids) for the host-side stitch
__global__ void k_gather_pc(TravGraph G, const uint32_t *__restrict__ seq_v, uint64_t len, uint32_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = (uint32_t)(G.upos[seq_v[i]] >> 32);
}

// record a finished walk (new ids) in the contig's global visited structures
__global__ void k_commit(const uint32_t *__restrict__ seq_v, uint64_t len, uint32_t in_lo, uint32_t in_hi, uint32_t *gbits,
                         uint32_t *gset, uint32_t gmask) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t u = seq_v[i];
        if (u >= in_lo && u < in_hi) atomicOr(&gbits[(u - in_lo) >> 5], 1u << ((u - in_lo) & 31u));
        else hs_insert(gset, gmask, u);
    }
}

// vertex attributes of a path (new ids) for the host
__global__ void k_gather_path(TravGraph G, const uint32_t *__restrict__ seq_v, const uint32_t *__restrict__ seq_s, uint64_t len,
                              pag_path_node *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t v = G.uold[seq_v[i]];
        uint64_t p = G.vpos[v];
        pag_path_node o;
        o.code = G.ncode[G.vnode[v]];
        o.ctg = (uint32_t)(p >> 32);
        o.ref = (uint32_t)p;
        o.cnt = G.vcnt[v];
        o.reserved = 0;
        o.step = (int32_t)seq_s[i];
        o.vid = v;
        out[i] = o;
    }
}

__global__ void k_gather_vertices(TravGraph G, const uint32_t *__restrict__ vids, uint32_t n, pag_path_node *__restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t v = vids[i];
    uint64_t p = G.vpos[v];
    pag_path_node o;
    o.code = G.ncode[G.vnode[v]];
    o.ctg = (uint32_t)(p >> 32);
    o.ref = (uint32_t)p;
    o.cnt = G.vcnt[v];
    o.reserved = 0;
    o.step = 0;
    o.vid = v;
    out[i] = o;
}

void trav_launch_seed_first(TravGraph G, const TravContig *ctgs, uint32_t n, uint64_t dev, uint32_t *out, uint32_t stride,
                            hipStream_t s) {
    if (n) k_seed_first<<<dim3(n), dim3(64), 0, s>>>(G, ctgs, n, dev, out, stride);
}
void trav_launch_seed_window(TravGraph G, const TravContig *ctgs, const TravSeedReq *reqs, uint32_t n, uint64_t dev,
                             uint32_t *out, uint32_t stride, hipStream_t s) {
    if (n) k_seed_window<<<dim3(n, TRAV_SEED_PARTS), dim3(64), 0, s>>>(G, ctgs, reqs, n, dev, out, stride);
}
void trav_launch_checkpoints(TravGraph G, const TravContig *ctgs, const TravSeedReq *reqs, uint32_t n, uint64_t dev, uint32_t *out,
                             hipStream_t s) {
    if (n) k_checkpoints<<<dim3(n), dim3(64), 0, s>>>(G, ctgs, reqs, n, dev, out);
}
void trav_launch_id_bounds(TravGraph G, const uint32_t *coords, uint32_t n, uint32_t *out, hipStream_t s) {
    if (n) k_id_bounds<<<dim3((n + 63) / 64), dim3(64), 0, s>>>(G, coords, n, out);
}
void trav_launch_pack_paths(TravGraph G, const TravPackDesc *descs, uint32_t n, uint64_t max_len, uint32_t *out, hipStream_t s) {
    if (!n) return;
    const unsigned gx = (unsigned)std::min<uint64_t>(std::max<uint64_t>((max_len + 255) / 256, 1), 64);
    k_pack_paths<<<dim3(gx, n), dim3(256), 0, s>>>(G, descs, n, out);
}
void trav_launch_gather_pc(TravGraph G, const uint32_t *seq_v, uint64_t len, uint32_t *out, hipStream_t s) {
    if (len) k_gather_pc<<<dim3(grid_for(len)), dim3(256), 0, s>>>(G, seq_v, len, out);
}
void trav_launch_commit(const uint32_t *seq_v, uint64_t len, uint32_t in_lo, uint32_t in_hi, uint32_t *gbits, uint32_t *gset,
                        uint32_t gmask, hipStream_t s) {
    if (len) k_commit<<<dim3(grid_for(len)), dim3(256), 0, s>>>(seq_v, len, in_lo, in_hi, gbits, gset, gmask);
}
void trav_launch_ranges(TravGraph G, TravContig *ctgs, uint32_t n, hipStream_t s) {
    if (n) k_ranges<<<dim3((n + 63) / 64), dim3(64), 0, s>>>(G, ctgs, n);
}

// blockIdx.y = range; 16 bytes per lane and turn where the range allows (the job buffers are 256-byte aligned), bytes at its edges.
// The byte at address a becomes byte (a & 3) of `word`, at the edges as in the body: a range on a 4-byte boundary is filled with
// whole copies of `word` whatever its bytes are, wherever its first 16-byte line begins.
__global__ void k_clear_ranges(const TravClear *__restrict__ ranges) {
    const TravClear c = ranges[blockIdx.y];
    uint8_t *p = as_global((uint8_t *)c.p);  // (device memory: global stores, not flat ones)
    const uint64_t head = (16u - ((uintptr_t)p & 15u)) & 15u, h = head < c.bytes ? head : c.bytes;
    const uint64_t n16 = (c.bytes - h) >> 4, tail = (c.bytes - h) & 15u;
    uint4 *q = (uint4 *)(p + h);
    const uint4 w = make_uint4(c.word, c.word, c.word, c.word);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) q[i] = w;
    if (blockIdx.x == 0) {
        auto byte_at = [&](const uint8_t *a) { return (uint8_t)(c.word >> (8u * (uint32_t)((uintptr_t)a & 3u))); };
        if (threadIdx.x < h) p[threadIdx.x] = byte_at(p + threadIdx.x);
        if (threadIdx.x < tail) p[h + (n16 << 4) + threadIdx.x] = byte_at(p + h + (n16 << 4) + threadIdx.x);
    }
}
int trav_clear_ranges(const TravClear *ranges_dev, size_t n, hipStream_t s) {
    for (size_t at = 0; at < n; at += 32768) {
        const uint32_t m = (uint32_t)std::min<size_t>(32768, n - at);
        k_clear_ranges<<<dim3(32, m), dim3(256), 0, s>>>(ranges_dev + at);
    }
    PAG_HIP_TRY(hipGetLastError());
    return PAG_OK;
}
void trav_launch_gather_path(TravGraph G, const uint32_t *seq_v, const uint32_t *seq_s, uint64_t len, pag_path_node *out,
                             hipStream_t s, unsigned max_blocks) {
    const unsigned grid = max_blocks ? std::min(grid_for(len), max_blocks) : grid_for(len);
    if (len) k_gather_path<<<dim3(grid), dim3(256), 0, s>>>(G, seq_v, seq_s, len, out);
}
// blockIdx.y = the part; the blocks of a row stride over its entries
__global__ void __launch_bounds__(256) k_concat_parts(const TravConcatPart *__restrict__ parts, uint32_t *__restrict__ out_v,
                                                      uint32_t *__restrict__ out_s, uint32_t first_step) {
    const TravConcatPart P = parts[blockIdx.y];
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < P.n; x += (uint64_t)gridDim.x * blockDim.x) {
        out_v[P.start + x] = P.v[x];
        out_s[P.start + x] = (P.start + x == 0) ? first_step : P.s[x];
    }
}
void trav_launch_concat_parts(const TravConcatPart *parts, uint32_t n_parts, uint32_t *out_v, uint32_t *out_s, uint32_t first_step,
                              hipStream_t s) {
    for (uint32_t at = 0; at < n_parts; at += 32768) {
        const uint32_t n = std::min<uint32_t>(32768, n_parts - at);
        k_concat_parts<<<dim3(16, n), dim3(256), 0, s>>>(parts + at, out_v, out_s, first_step);
    }
}
void trav_launch_gather_vertices(TravGraph G, const uint32_t *vids, uint32_t n, pag_path_node *out, hipStream_t s) {
    if (n) k_gather_vertices<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(G, vids, n, out);
}

}  // namespace pagdev

using namespace pagdev;

// test hooks (include/pagraph_debug.h): the kernels above through their production launchers, on caller-given HOST arrays with
// device buffers of their own (trav_hook.hpp).  Each refuses what would let a kernel leave those buffers or never end.
namespace {
// TravContig records out of their mirrors: nodes / gbits / gset patched in from the uploaded arrays
int hook_contigs(const pag_debug_trav_contig *ctgs, uint32_t n_ctgs, uint64_t n_graph_nodes, const uint32_t *nodes, uint64_t n_node_words,
                 uint64_t n_gbits, const uint32_t *gset, uint64_t n_gset, const uint32_t *d_nodes, uint32_t *d_gbits, uint32_t *d_gset,
                 std::vector<TravContig> &tc) {
    if (n_ctgs && !ctgs) return PAG_EINVAL;
    for (uint64_t i = 0; i < n_node_words; ++i)
        if (nodes[i] != PAG_NONE && nodes[i] >= n_graph_nodes) return PAG_EINVAL;
    tc.assign(n_ctgs, TravContig{});
    for (uint32_t i = 0; i < n_ctgs; ++i) {
        const pag_debug_trav_contig &m = ctgs[i];
        TravContig &t = tc[i];
        if (m.n_kmers && (m.nodes_off > n_node_words || m.n_kmers > n_node_words - m.nodes_off)) return PAG_EINVAL;
        if (m.g_hi < m.g_lo || m.in_hi < m.in_lo) return PAG_EINVAL;
        t.nodes = d_nodes + m.nodes_off;
        t.n_kmers = m.n_kmers;
        t.ctg_left = m.ctg_left;
        t.ctg_right = m.ctg_right;
        t.in_lo = m.in_lo;
        t.in_hi = m.in_hi;
        t.g_lo = m.g_lo;
        t.g_hi = m.g_hi;
        t.gmask = m.gmask;
        if (m.gbits_off != PAG_DEBUG_NULL) {
            const uint64_t words = ((uint64_t)(m.g_hi - m.g_lo) + 31) / 32;
            if (m.gbits_off > n_gbits || words > n_gbits - m.gbits_off) return PAG_EINVAL;
            t.gbits = d_gbits + m.gbits_off;
        }
        if (m.gset_off != PAG_DEBUG_NULL) {
            const uint64_t cap = (uint64_t)m.gmask + 1;
            if ((cap & (cap - 1)) || m.gset_off > n_gset || cap > n_gset - m.gset_off) return PAG_EINVAL;
            bool free_slot = false;  // (a lookup ends at a key or at an empty slot)
            for (uint64_t x = 0; x < cap && !free_slot; ++x) free_slot = gset[m.gset_off + x] == HS_EMPTY;
            if (!free_slot) return PAG_EINVAL;
            t.gset = d_gset + m.gset_off;
        }
    }
    return PAG_OK;
}
}  // namespace

extern "C" int pag_debug_trav_bounds(const pag_debug_trav_graph *g, const uint32_t *coords, uint32_t n, uint32_t *out, pag_debug_trav_contig *ctgs,
                                     uint32_t n_ctgs, int device) {
    if (!g || (g->n_pos && !g->upos) || (n && (!coords || !out)) || (n_ctgs && !ctgs)) return PAG_EINVAL;
    DevCall D("test hook");
    TravGraph G;
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault)) || (rc = hook_upload_graph(D, g, &G))) return rc;
    uint32_t *d_coords = nullptr, *d_out = nullptr;
    TravContig *d_tc = nullptr;
    std::vector<TravContig> tc(n_ctgs, TravContig{});
    for (uint32_t i = 0; i < n_ctgs; ++i) {
        tc[i].ctg_left = ctgs[i].ctg_left;
        tc[i].ctg_right = ctgs[i].ctg_right;
        tc[i].in_lo = ctgs[i].in_lo;
        tc[i].in_hi = ctgs[i].in_hi;
        tc[i].g_lo = ctgs[i].g_lo;
        tc[i].g_hi = ctgs[i].g_hi;
    }
    if ((rc = D.up(coords, n, &d_coords)) || (rc = D.up((const uint32_t *)out, n, &d_out)) || (rc = D.up((const TravContig *)tc.data(), n_ctgs, &d_tc))) return rc;
    trav_launch_id_bounds(G, d_coords, n, d_out, D.s);
    trav_launch_ranges(G, d_tc, n_ctgs, D.s);
    if ((rc = D.down(out, d_out, n)) || (rc = D.down(tc.data(), d_tc, n_ctgs)) || (rc = D.finish())) return rc;
    for (uint32_t i = 0; i < n_ctgs; ++i) {
        ctgs[i].in_lo = tc[i].in_lo;
        ctgs[i].in_hi = tc[i].in_hi;
        ctgs[i].g_lo = tc[i].g_lo;
        ctgs[i].g_hi = tc[i].g_hi;
    }
    return PAG_OK;
}

extern "C" int pag_debug_trav_seeds(const pag_debug_trav_graph *g, int which, const pag_debug_trav_contig *ctgs, uint32_t n_ctgs, const uint32_t *nodes,
                                    uint64_t n_node_words, const uint32_t *gbits, uint64_t n_gbits, const uint32_t *gset, uint64_t n_gset,
                                    const uint64_t *reqs, uint32_t n_req, uint64_t dev, uint32_t *out, uint64_t out_words, uint32_t stride, int device) {
    if (!g || which < 0 || which > 2 || !g->npos_off || (g->n_pos && (!g->vpos || !g->newid || !g->vcnt)) || (n_node_words && !nodes) ||
        (n_gbits && !gbits) || (n_gset && !gset) || !out)
        return PAG_EINVAL;
    const uint64_t need = which == 0 ? (uint64_t)n_ctgs * stride : which == 1 ? (uint64_t)n_req * TRAV_SEED_PARTS * stride : 3ull * n_req;
    if ((which != 2 && stride < 2) || out_words < need || (which != 0 && n_req && !reqs)) return PAG_EINVAL;
    std::vector<TravSeedReq> rq(which == 0 ? 0 : n_req);
    for (size_t r = 0; r < rq.size(); ++r) {
        if (reqs[4 * r] >= n_ctgs) return PAG_EINVAL;
        rq[r].ctg = (uint32_t)reqs[4 * r];
        rq[r].pad = 0;
        rq[r].left = reqs[4 * r + 1];
        rq[r].right = reqs[4 * r + 2];
        rq[r].pos = reqs[4 * r + 3];
    }
    DevCall D("test hook");
    TravGraph G;
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault)) || (rc = hook_upload_graph(D, g, &G))) return rc;
    uint32_t *d_nodes = nullptr, *d_gbits = nullptr, *d_gset = nullptr, *d_out = nullptr;
    TravContig *d_tc = nullptr;
    TravSeedReq *d_rq = nullptr;
    if ((rc = D.up(nodes, n_node_words, &d_nodes)) || (rc = D.up(gbits, n_gbits, &d_gbits)) || (rc = D.up(gset, n_gset, &d_gset)) ||
        (rc = D.up((const uint32_t *)out, out_words, &d_out)))
        return rc;
    std::vector<TravContig> tc;
    if ((rc = hook_contigs(ctgs, n_ctgs, g->n_nodes, nodes, n_node_words, n_gbits, gset, n_gset, d_nodes, d_gbits, d_gset, tc))) return rc;
    if ((rc = D.up((const TravContig *)tc.data(), n_ctgs, &d_tc)) || (rc = D.up((const TravSeedReq *)rq.data(), rq.size(), &d_rq))) return rc;
    if (which == 0) trav_launch_seed_first(G, d_tc, n_ctgs, dev, d_out, stride, D.s);
    else if (which == 1) trav_launch_seed_window(G, d_tc, d_rq, n_req, dev, d_out, stride, D.s);
    else trav_launch_checkpoints(G, d_tc, d_rq, n_req, dev, d_out, D.s);
    if ((rc = D.down(out, d_out, out_words))) return rc;
    return D.finish();
}

extern "C" int pag_debug_pack_paths(const pag_debug_trav_graph *g, const uint32_t *seq_v, const uint32_t *seq_s, const uint64_t *seq_x, uint64_t n_seq,
                                    const uint64_t *descs, uint32_t n, uint64_t max_len, uint32_t *out, uint64_t out_words, int device) {
    if (!g || !g->upos || (n_seq && (!seq_v || !seq_s)) || (n && !descs) || !out || n > 65535u) return PAG_EINVAL;
    for (uint64_t i = 0; i < n_seq; ++i)
        if (seq_v[i] >= g->n_pos) return PAG_EINVAL;
    for (uint32_t j = 0; j < n; ++j) {
        const uint64_t from = descs[4 * j], len = descs[4 * j + 1], off = descs[4 * j + 2];
        const bool leap = descs[4 * j + 3] != 0;
        if (from > n_seq || len > n_seq - from || len > max_len || (leap && !seq_x)) return PAG_EINVAL;
        if (off > out_words || trav_pack_words(len, leap) > out_words - off) return PAG_EINVAL;
    }
    DevCall D("test hook");
    TravGraph G;
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault)) || (rc = hook_upload_graph(D, g, &G))) return rc;
    uint32_t *d_v = nullptr, *d_s = nullptr, *d_out = nullptr;
    uint64_t *d_x = nullptr;
    TravPackDesc *d_desc = nullptr;
    if ((rc = D.up(seq_v, n_seq, &d_v)) || (rc = D.up(seq_s, n_seq, &d_s)) || (rc = D.up(seq_x, seq_x ? n_seq : 0, &d_x)) ||
        (rc = D.up((const uint32_t *)out, out_words, &d_out)))
        return rc;
    std::vector<TravPackDesc> pd(n);
    for (uint32_t j = 0; j < n; ++j) {
        pd[j].seq_v = d_v + descs[4 * j];
        pd[j].seq_s = d_s + descs[4 * j];
        pd[j].len = descs[4 * j + 1];
        pd[j].off = descs[4 * j + 2];
        pd[j].seq_x = descs[4 * j + 3] ? d_x + descs[4 * j] : nullptr;
    }
    if ((rc = D.up((const TravPackDesc *)pd.data(), n, &d_desc))) return rc;
    trav_launch_pack_paths(G, d_desc, n, max_len, d_out, D.s);
    if ((rc = D.down(out, d_out, out_words))) return rc;
    return D.finish();
}

extern "C" int pag_debug_commit(const uint32_t *seq_v, uint64_t len, uint32_t in_lo, uint32_t in_hi, uint32_t *gbits, uint64_t n_gbits, uint64_t gbits_off,
                                uint32_t *gset, uint32_t ncap, int device) {
    if ((len && !seq_v) || in_hi < in_lo || !gset || !ncap || (ncap & (ncap - 1)) || (n_gbits && !gbits)) return PAG_EINVAL;
    if (gbits_off > n_gbits || ((uint64_t)(in_hi - in_lo) + 31) / 32 > n_gbits - gbits_off) return PAG_EINVAL;
    {   // an insert ends at its key or at an empty slot: more empty slots than distinct keys to come
        std::vector<uint32_t> outside;
        for (uint64_t i = 0; i < len; ++i)
            if (seq_v[i] < in_lo || seq_v[i] >= in_hi) outside.push_back(seq_v[i]);
        std::sort(outside.begin(), outside.end());
        const uint64_t distinct = (uint64_t)(std::unique(outside.begin(), outside.end()) - outside.begin());
        uint64_t empty = 0;
        for (uint32_t x = 0; x < ncap; ++x) empty += gset[x] == HS_EMPTY;
        if (empty <= distinct) return PAG_EINVAL;
    }
    DevCall D("test hook");
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault))) return rc;
    uint32_t *d_v = nullptr, *d_bits = nullptr, *d_set = nullptr;
    if ((rc = D.up(seq_v, len, &d_v)) || (rc = D.up((const uint32_t *)gbits, n_gbits, &d_bits)) || (rc = D.up((const uint32_t *)gset, (uint64_t)ncap, &d_set))) return rc;
    trav_launch_commit(d_v, len, in_lo, in_hi, d_bits + gbits_off, d_set, ncap - 1, D.s);
    if ((rc = D.down(gbits, d_bits, n_gbits)) || (rc = D.down(gset, d_set, (uint64_t)ncap))) return rc;
    return D.finish();
}

extern "C" int pag_debug_clear_ranges(uint8_t *buf, uint64_t bytes, const uint64_t *ranges, uint64_t n, int device) {
    if ((bytes && !buf) || (n && !ranges)) return PAG_EINVAL;
    for (uint64_t i = 0; i < n; ++i)
        if (ranges[3 * i] > bytes || ranges[3 * i + 1] > bytes - ranges[3 * i] || ranges[3 * i + 2] > 0xFFFFFFFFull) return PAG_EINVAL;
    DevCall D("test hook");
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault))) return rc;
    uint8_t *d_buf = nullptr;
    TravClear *d_r = nullptr;
    if ((rc = D.up((const uint8_t *)buf, bytes, &d_buf, 256))) return rc;
    if (((uintptr_t)d_buf & 255u) != 0) {
        set_error("pag_debug_clear_ranges: the device buffer does not start on a 256-byte boundary");
        return PAG_EFAULT;
    }
    std::vector<TravClear> rs(n);
    for (uint64_t i = 0; i < n; ++i) rs[i] = TravClear{d_buf + ranges[3 * i], ranges[3 * i + 1], (uint32_t)ranges[3 * i + 2], 0u};
    if ((rc = D.up((const TravClear *)rs.data(), n, &d_r))) return rc;
    if (n && (rc = trav_clear_ranges(d_r, n, D.s))) return rc;
    if ((rc = D.down(buf, d_buf, bytes))) return rc;
    return D.finish();
}

extern "C" int pag_debug_concat_parts(const uint32_t *src_v, const uint32_t *src_s, uint64_t n_src, const uint64_t *parts, uint32_t n_parts, uint32_t *out_v,
                                      uint32_t *out_s, uint64_t n_out, uint32_t first_step, int device) {
    if ((n_src && (!src_v || !src_s)) || (n_parts && !parts) || (n_out && (!out_v || !out_s))) return PAG_EINVAL;
    for (uint32_t i = 0; i < n_parts; ++i) {
        const uint64_t from = parts[3 * i], start = parts[3 * i + 1], m = parts[3 * i + 2];
        if (from > n_src || m > n_src - from || start > n_out || m > n_out - start) return PAG_EINVAL;
    }
    DevCall D("test hook");
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault))) return rc;
    uint32_t *d_sv = nullptr, *d_ss = nullptr, *d_ov = nullptr, *d_os = nullptr;
    TravConcatPart *d_p = nullptr;
    if ((rc = D.up(src_v, n_src, &d_sv)) || (rc = D.up(src_s, n_src, &d_ss)) || (rc = D.up((const uint32_t *)out_v, n_out, &d_ov)) ||
        (rc = D.up((const uint32_t *)out_s, n_out, &d_os)))
        return rc;
    std::vector<TravConcatPart> ps(n_parts);
    for (uint32_t i = 0; i < n_parts; ++i) ps[i] = TravConcatPart{d_sv + parts[3 * i], d_ss + parts[3 * i], parts[3 * i + 1], parts[3 * i + 2]};
    if ((rc = D.up((const TravConcatPart *)ps.data(), (uint64_t)n_parts, &d_p))) return rc;
    trav_launch_concat_parts(d_p, n_parts, d_ov, d_os, first_step, D.s);
    if ((rc = D.down(out_v, d_ov, n_out)) || (rc = D.down(out_s, d_os, n_out))) return rc;
    return D.finish();
}

extern "C" int pag_debug_gathers(const pag_debug_trav_graph *g, int which, const uint32_t *seq_v, const uint32_t *seq_s, uint64_t len, uint32_t max_blocks,
                                 void *out, int device) {
    if (!g || which < 0 || which > 2 || (len && (!seq_v || !out)) || (which == 1 && len && !seq_s) || (which == 2 && len > 0xFFFFFFF0ull)) return PAG_EINVAL;
    if (which == 0 ? !g->upos : (!g->vpos || !g->vcnt || !g->vnode || !g->ncode || (which == 1 && !g->uold))) return PAG_EINVAL;
    for (uint64_t i = 0; i < len; ++i)
        if (seq_v[i] >= g->n_pos) return PAG_EINVAL;
    DevCall D("test hook");
    TravGraph G;
    int rc;
    if ((rc = D.open(device, true, hipStreamDefault)) || (rc = hook_upload_graph(D, g, &G))) return rc;
    uint32_t *d_v = nullptr, *d_s = nullptr;
    if ((rc = D.up(seq_v, len, &d_v)) || (rc = D.up(seq_s, seq_s ? len : 0, &d_s))) return rc;
    if (which == 0) {
        uint32_t *d_out = nullptr;
        if ((rc = D.up((const uint32_t *)out, len, &d_out))) return rc;
        trav_launch_gather_pc(G, d_v, len, d_out, D.s);
        if ((rc = D.down((uint32_t *)out, d_out, len))) return rc;
    } else {
        pag_path_node *d_out = nullptr;
        if ((rc = D.up((const pag_path_node *)out, len, &d_out))) return rc;
        if (which == 1) trav_launch_gather_path(G, d_v, d_s, len, d_out, D.s, max_blocks);
        else trav_launch_gather_vertices(G, d_v, (uint32_t)len, d_out, D.s);
        if ((rc = D.down((pag_path_node *)out, d_out, len))) return rc;
    }
    return D.finish();
}
