// text_tiles.hpp — what the two text renderers (k5_dump.hip: the lines of a path dump, k5_seq.hip: a path's consensus
// sequence) have in common; included by those two files only.
//
// A text is rendered in two launches over tiles of TEXT_TILE items (a line, a vertex), an item per thread.  The measure
// launch (text_measure) leaves every tile's byte count, and the block that finishes last scans the counts into byte offsets
// and the total.  The render launch formats a tile into an LDS staging buffer — every thread at the offset tile_offset gives
// it — and tile_flush copies the staged bytes to the output with 16-byte stores (the tile's unaligned head and tail byte by
// byte).  The output may be pinned host memory: what reaches it are whole 16-byte stores of consecutive lanes.
#pragma once
#include <algorithm>
#include <vector>

#include "dev_call.hpp"
#include "pag_device.hpp"
#include "pag_travel.hpp"

namespace pagdev {

constexpr uint32_t TEXT_TILE = 256;

// ---- where the records come from: an array, or the traversal view and a path's vertex ids
struct PathVertex {
    uint32_t code, ctg, ref, cnt;
    int32_t step;
};
struct PathSrcRecords {
    const pag_path_node *rec;
    __device__ __forceinline__ int32_t step(uint64_t i) const { return rec[i].step; }
    __device__ __forceinline__ PathVertex operator()(uint64_t i) const {
        const pag_path_node n = rec[i];
        return PathVertex{n.code, n.ctg, n.ref, n.cnt, n.step};
    }
};
struct PathSrcPath {  // what k_gather_path (k5_walk_aux.hip) writes for entry i of a path
    TravGraph G;
    const uint32_t *seq_v, *seq_s;
    __device__ __forceinline__ int32_t step(uint64_t i) const { return (int32_t)seq_s[i]; }
    __device__ __forceinline__ PathVertex operator()(uint64_t i) const {
        const uint32_t v = G.uold[seq_v[i]];
        const uint64_t p = G.vpos[v];
        return PathVertex{G.ncode[G.vnode[v]], (uint32_t)(p >> 32), (uint32_t)p, G.vcnt[v], (int32_t)seq_s[i]};
    }
};

// ---- the device scratch of one rendering of n items (its size: text_scratch_bytes, pag_travel.hpp)
struct TextScratch {  // [ticket u32, flag u32][total u64][tile_off u64 x n_tiles][tile_cnt u64 x n_tiles]
    uint32_t *ticket, *flag;  // (flag: the renderer's own — k5_seq.hip's "not renderable"; cleared with the ticket)
    uint64_t *total, *tile_off, *tile_cnt;
    TextScratch(void *p, uint64_t n) {
        ticket = (uint32_t *)p;
        flag = ticket + 1;
        total = (uint64_t *)((char *)p + 8);
        tile_off = (uint64_t *)((char *)p + 16);
        tile_cnt = tile_off + tiles(n);
    }
    static uint64_t tiles(uint64_t n) { return (n + TEXT_TILE - 1) / TEXT_TILE; }
    static size_t bytes(uint64_t n) { return (size_t)((16 + tiles(n) * 16 + 255) & ~(uint64_t)255); }
};

// ---- launches: TEXT_TILE threads, a block per tile up to max_blocks (0: up to 1024)
inline unsigned text_grid(uint64_t n, unsigned max_blocks) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(TextScratch::tiles(n), max_blocks ? max_blocks : 1024u));
}
template <typename Kernel, typename... Args>
int text_launch(Kernel kernel, uint64_t n, unsigned max_blocks, hipStream_t s, Args... args) {
    kernel<<<dim3(text_grid(n, max_blocks)), dim3(TEXT_TILE), 0, s>>>(args...);
    PAG_HIP_TRY(hipGetLastError());
    return PAG_OK;
}
inline int text_scratch_reset(void *scratch, hipStream_t s) {  // (ticket and flag, ahead of a measure launch)
    PAG_HIP_TRY(hipMemsetAsync(scratch, 0, 16, s));
    return PAG_OK;
}

// ---- the body of a measure kernel: byte count of every tile (len_of(i): the bytes of item i); the last block to finish turns
//      them into byte offsets and the total
template <typename Len>
__device__ __forceinline__ void text_measure(uint64_t n, Len len_of, uint64_t *__restrict__ tile_cnt, uint64_t *__restrict__ tile_off, uint32_t *ticket,
                                             uint64_t *total_dev, uint64_t *total_host) {
    __shared__ uint64_t wsum[TEXT_TILE / PAG_WAVE];
    __shared__ uint32_t last;
    const uint64_t n_tiles = (n + TEXT_TILE - 1) / TEXT_TILE;
    const uint32_t wave = threadIdx.x / PAG_WAVE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * TEXT_TILE + threadIdx.x;
        decltype(len_of(i)) len = 0;  // (summed over the wave in len_of's own type: uint32_t where 64 items' bytes fit it)
        if (i < n) len = len_of(i);
        const uint64_t w = wave_sum(len);
        if (lane_id() == 0) wsum[wave] = w;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    // the counts of this block are visible device-wide before its ticket is
    __threadfence();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!last) return;
    __threadfence();
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += TEXT_TILE) {
        const uint64_t t = base + threadIdx.x;
        const uint64_t c = t < n_tiles ? __hip_atomic_load(&tile_cnt[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        uint64_t wtot;
        const uint64_t pre = wave_excl_sum64(c, &wtot);
        if (lane_id() == 0) wsum[wave] = wtot;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
        if (t < n_tiles) tile_off[t] = before + pre;
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total_dev = carry;
        if (total_host) *total_host = carry;
    }
}

// ---- the opening of a render kernel's tile: where this thread's `len` bytes begin inside the tile, and the tile's bytes
//      (T: uint32_t where a tile's bytes are bounded, uint64_t otherwise).  A barrier lies between two calls: tile_flush's, or
//      the caller's own.
__device__ __forceinline__ uint32_t wave_excl_sum_of(uint32_t v, uint32_t *total) { return wave_excl_sum(v, total); }
__device__ __forceinline__ uint64_t wave_excl_sum_of(uint64_t v, uint64_t *total) { return wave_excl_sum64(v, total); }
template <typename T>
__device__ __forceinline__ T tile_offset(T len, T *tile_bytes) {
    __shared__ T wsum[TEXT_TILE / PAG_WAVE];
    const uint32_t wave = threadIdx.x / PAG_WAVE;
    T wtot;
    const T pre = wave_excl_sum_of(len, &wtot);
    if (lane_id() == 0) wsum[wave] = wtot;
    __syncthreads();
    T before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    *tile_bytes = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return before + pre;
}

// ---- a tile is staged at the alignment its bytes have in the output — 16-byte groups of the one are 16-byte groups of the
//      other: the tile whose bytes go to out[o, o + tile_bytes) is formatted into stage[stage_shift(out, o), ...), and stage
//      holds 16 bytes more than the largest tile
__device__ __forceinline__ uint32_t stage_shift(const unsigned char *out, uint64_t o) { return (uint32_t)(((uintptr_t)out + o) & 15u); }
// the staged tile to the output (every thread of the block; the threads' writes to `stage` are waited for here)
__device__ __forceinline__ void tile_flush(const unsigned char *stage, unsigned char *out, uint64_t o, uint32_t tile_bytes) {
    const uint32_t sh = stage_shift(out, o);
    __syncthreads();
    unsigned char *dst = out + o - sh;  // (16-byte aligned; nothing below dst + sh is touched)
    const uint32_t lo = sh, hi = sh + tile_bytes;
    const uint32_t a_lo = (lo + 15u) & ~15u, a_hi = hi & ~15u;
    if (a_lo >= a_hi) {
        for (uint32_t j = lo + threadIdx.x; j < hi; j += TEXT_TILE) dst[j] = stage[j];
    } else {
        if (lo + threadIdx.x < a_lo) dst[lo + threadIdx.x] = stage[lo + threadIdx.x];
        for (uint32_t q = (a_lo >> 4) + threadIdx.x; q < (a_hi >> 4); q += TEXT_TILE) ((uint4 *)dst)[q] = ((const uint4 *)stage)[q];
        if (a_hi + threadIdx.x < hi) dst[a_hi + threadIdx.x] = stage[a_hi + threadIdx.x];
    }
}

// ---- pag_render_dump_lines / pag_render_path_sequence: what such a call has on top of its DevCall (a non-blocking stream; the
//      caller's current device is put back at every exit)
struct TextCall : DevCall {
    pag_path_node *rec = nullptr;  // the records
    uint32_t *tab = nullptr;       // the tables' blob (dump_tables_at)
    explicit TextCall(const char *w) : DevCall(w) {}
    // the device chosen, the stream, room for the records and the tables
    int begin(int device, uint64_t n, const std::vector<uint32_t> &blob) {
        int rc = open(device, true, hipStreamNonBlocking);
        if (!rc) rc = alloc(&rec, n);
        return rc ? rc : alloc(&tab, blob.size(), 16);
    }
    // ... and, when every buffer of the call has been allocated, their upload
    int upload(const pag_path_node *records, uint64_t n, const std::vector<uint32_t> &blob) {
        PAG_HIP_TRY(hipMemcpyAsync(rec, records, n * sizeof(pag_path_node), hipMemcpyHostToDevice, s));
        if (!blob.empty()) PAG_HIP_TRY(hipMemcpyAsync(tab, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, s));
        return PAG_OK;
    }
};

}  // namespace pagdev
