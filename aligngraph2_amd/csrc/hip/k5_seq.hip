// k5_seq.hip — the consensus sequence of a path (PAlgorithm::seqToString, PAlgorithm.cpp:428-489; host restatement:
// csrc/host/traversal.cpp SeqTools::seqToString) rendered on the device.
//
// Vertex 0 contributes its k-mer; vertex i > 0 with step s contributes
//     s <= k : the last s bases of its k-mer, upper case (nothing for s <= 0);
//     s >  k : s - k bases in lower case read out of a contig or a reference sequence along a line from the coordinate of
//              vertex i - 1 to its own — isEdgeSimilar / isPosSimilar choose the coordinate space, singleToDual of both ends
//              gives the sequence, the strand and the slope; the position is an f64 accumulated one addition per base and
//              rounded half away from zero, exactly as the host does it — then its whole k-mer, upper case.
// The text's size is therefore known without rendering: k + the sum of the positive steps behind vertex 0.
//
// Two launches, shaped like k5_dump.hip's.  k_seq_measure: a thread per vertex, a tile of 256 vertices leaves its byte
// count, the block that finishes last scans the tile counts into byte offsets and the total.  k_seq_render: a tile's threads
// write their bases into an LDS staging buffer at their prefix offsets — one thread walks its own step serially — and the
// block copies the staged bytes out with 16-byte stores; a tile with more bytes than the staging buffer holds (one step can be
// thousands of bases) writes straight to the output.  The output may be pinned host memory.
//
// A rounded position that is negative or not finite (or beyond 64 bits) has no defined meaning on the host (a cast to
// size_t): the path is reported as NOT RENDERABLE and the caller renders it elsewhere.  A position past the end of its
// sequence, or a sequence index outside the table (coordinate 0 maps to (0, 0)), is defined: 'n'.
//
// The file relies on -ffp-contract=off (the ratio tests and the accumulated position must not be fused).
#include <algorithm>
#include <vector>

#include "pag_device.hpp"
#include "pag_travel.hpp"

namespace pagdev {

namespace {

constexpr uint32_t SEQ_TILE = 256;
constexpr uint32_t SEQ_STAGE_BYTES = 16384;  // a tile's bytes when they are staged (a tile of short steps: ~1 KB)

struct SeqVertex {
    uint32_t code, ctg, ref;
    int32_t step;
};

// where the records come from
struct SeqSrcRecords {
    const pag_path_node *rec;
    __device__ __forceinline__ int32_t step(uint64_t i) const { return rec[i].step; }
    __device__ __forceinline__ SeqVertex operator()(uint64_t i) const {
        const pag_path_node n = rec[i];
        return SeqVertex{n.code, n.ctg, n.ref, n.step};
    }
};
struct SeqSrcPath {  // what k_gather_path (k5_walk_aux.hip) writes for entry i of a path
    TravGraph G;
    const uint32_t *seq_v, *seq_s;
    __device__ __forceinline__ int32_t step(uint64_t i) const { return (int32_t)seq_s[i]; }
    __device__ __forceinline__ SeqVertex operator()(uint64_t i) const {
        const uint32_t v = G.uold[seq_v[i]];
        const uint64_t p = G.vpos[v];
        return SeqVertex{G.ncode[G.vnode[v]], (uint32_t)(p >> 32), (uint32_t)p, (int32_t)seq_s[i]};
    }
};

__device__ __forceinline__ uint64_t seq_vertex_len(uint64_t i, int32_t step, uint32_t k) { return i == 0 ? (uint64_t)k : (uint64_t)(step > 0 ? step : 0); }

// isPosSimilar / isEdgeSimilar (host_graph.hpp:27-47) of ONE coordinate: the u32 wrap of l + dist and of r - l, the f64 ratio
__device__ __forceinline__ bool pos_similar(uint32_t l, uint32_t r, uint64_t deviation) {
    return l != 0u && r != 0u && (uint64_t)((l > r ? l : r) - (l > r ? r : l)) <= deviation;
}
__device__ __forceinline__ bool edge_similar(uint32_t l, uint32_t r, int32_t dist, uint64_t deviation, double error_rate) {
    const uint32_t moved = l != 0u ? l + (uint32_t)dist : 0u;
    if (pos_similar(moved, r, deviation)) return true;
    return l != 0u && r != 0u && fabs(1.0 - ((double)(uint32_t)(r - l) * 1.0 / (double)dist)) <= error_rate;
}

// the last `n` bases of the k-mer `code` (first base most significant), upper case, to dst[0, n)
__device__ __forceinline__ void put_kmer_tail(unsigned char *dst, uint32_t code, uint32_t n) {
    for (uint32_t j = 0; j < n; ++j) dst[j] = (unsigned char)((0x54474341u >> (((code >> (2u * (n - 1u - j))) & 3u) * 8u)) & 0xFFu);  // "ACGT"
}

// the bytes of vertex i to dst[0, its length); false: a position of its step is not renderable
template <typename Src>
__device__ __forceinline__ bool seq_vertex_write(unsigned char *dst, const Src &src, uint64_t i, const SeqVertex &now, const SeqParams &P, const DumpTables &T,
                                                 const SeqSources &S) {
    const uint32_t k = P.k;
    if (i == 0) {
        put_kmer_tail(dst, now.code, k);
        return true;
    }
    if (now.step <= (int32_t)k) {
        if (now.step > 0) put_kmer_tail(dst, now.code, (uint32_t)now.step);
        return true;
    }
    const SeqVertex prev = src(i - 1);
    const bool s1 = edge_similar(prev.ctg, now.ctg, now.step, P.deviation, P.error_rate);
    const bool s2 = edge_similar(prev.ref, now.ref, now.step, P.deviation, P.error_rate);
    bool use_ctg = s1;
    if (!s1 && !s2) use_ctg = pos_similar(prev.ctg, now.ctg, P.deviation);
    const uint32_t *starts = use_ctg ? T.cstart : T.rstart, *sizes = use_ctg ? T.csize : T.rsize;
    const uint32_t n_seqs = use_ctg ? T.nc : T.nr;
    int32_t s_idx, e_idx;
    int64_t s_off, e_off;
    single_to_dual(starts, sizes, n_seqs, use_ctg ? prev.ctg : prev.ref, &s_idx, &s_off);
    single_to_dual(starts, sizes, n_seqs, use_ctg ? now.ctg : now.ref, &e_idx, &e_off);
    const int64_t pos_dist = e_off - s_off;
    const int64_t sel = (int64_t)(e_idx < 0 ? -(int64_t)e_idx : (int64_t)e_idx) - 1;
    const bool forward = e_idx > 0;
    const double move = (double)pos_dist * 1.0 / (double)now.step;
    double ref_now = (double)(s_off + (int64_t)k);
    const bool have = sel >= 0 && sel < (int64_t)n_seqs;
    const uint64_t len = have ? (uint64_t)sizes[sel] : 0ull;
    const uint8_t *bases = have ? (use_ctg ? S.cpacked + S.coff[sel] : S.rpacked + S.roff[sel]) : nullptr;
    // SeqDb::baseAt: forward = base idx, reverse strand = complement of base len - 1 - idx; here in lower case
    const uint32_t letters = forward ? 0x74676361u : 0x61636774u;  // "acgt" / "tgca"
    const uint32_t n_read = (uint32_t)now.step - k;
    bool ok = true;
    for (uint32_t j = 0; j < n_read; ++j) {
        const double r = round(ref_now);  // (half away from zero)
        unsigned char b = 'n';
        if (!(r >= 0.0) || !(r < 18446744073709551616.0)) {
            ok = false;
        } else {
            const uint64_t at = (uint64_t)r;
            if (at < len) {
                const uint64_t from = forward ? at : len - 1ull - at;
                b = (unsigned char)((letters >> (((bases[from >> 2] >> ((from & 3ull) * 2ull)) & 3u) * 8u)) & 0xFFu);
            }
        }
        dst[j] = b;
        ref_now += move;
    }
    put_kmer_tail(dst + n_read, now.code, k);
    return ok;
}

// byte count of every tile of 256 vertices; the last block to finish turns them into byte offsets and the total
template <typename Src>
__global__ void __launch_bounds__(SEQ_TILE) k_seq_measure(Src src, uint64_t n, uint32_t k, uint64_t *__restrict__ tile_cnt, uint64_t *__restrict__ tile_off,
                                                          uint32_t *ticket, uint64_t *total_dev, uint64_t *total_host) {
    __shared__ uint64_t wsum[SEQ_TILE / PAG_WAVE];
    __shared__ uint32_t last;
    const uint64_t n_tiles = (n + SEQ_TILE - 1) / SEQ_TILE;
    const uint32_t wave = threadIdx.x / PAG_WAVE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * SEQ_TILE + threadIdx.x;
        const uint64_t len = i < n ? seq_vertex_len(i, src.step(i), k) : 0ull;
        uint64_t wtot;
        (void)wave_excl_sum64(len, &wtot);
        if (lane_id() == 0) wsum[wave] = wtot;
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
    for (uint64_t base = 0; base < n_tiles; base += SEQ_TILE) {
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

template <typename Src>
__global__ void __launch_bounds__(SEQ_TILE) k_seq_render(Src src, uint64_t n, SeqParams P, DumpTables T, SeqSources S, const uint64_t *__restrict__ tile_off,
                                                         const uint64_t *__restrict__ total_dev, unsigned char *out, uint64_t cap, uint32_t *bad_dev,
                                                         uint64_t *bad_host) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[SEQ_STAGE_BYTES + 16];  // (+ 16: a tile is staged at the output's alignment)
    __shared__ uint64_t wsum[SEQ_TILE / PAG_WAVE];
    if (*total_dev > cap) return;  // (nothing is written into a buffer that cannot take all of it)
    out = as_global(out);
    const uint64_t n_tiles = (n + SEQ_TILE - 1) / SEQ_TILE;
    const uint32_t wave = threadIdx.x / PAG_WAVE;
    bool ok = true;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * SEQ_TILE + threadIdx.x;
        SeqVertex v{};
        uint64_t len = 0;
        if (i < n) {
            v = src(i);
            len = seq_vertex_len(i, v.step, P.k);
        }
        uint64_t wtot;
        const uint64_t pre = wave_excl_sum64(len, &wtot);
        if (lane_id() == 0) wsum[wave] = wtot;
        __syncthreads();
        uint64_t before = 0;
        for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
        const uint64_t tile_bytes = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        const uint64_t o = tile_off[tile];  // (o + tile_bytes <= total <= cap)
        if (tile_bytes > SEQ_STAGE_BYTES) {
            // more than the staging buffer holds: every thread stores its bytes where they belong
            if (len) ok = seq_vertex_write(out + o + before + pre, src, i, v, P, T, S) && ok;
        } else {
            // the tile is staged at the alignment its bytes have in the output: 16-byte groups of the one are 16-byte groups of the other
            const uint32_t sh = (uint32_t)(((uintptr_t)out + o) & 15u);
            if (len) ok = seq_vertex_write(stage + sh + (uint32_t)(before + pre), src, i, v, P, T, S) && ok;
            __syncthreads();
            unsigned char *dst = out + o - sh;  // (16-byte aligned; nothing below dst + sh is touched)
            const uint32_t lo = sh, hi = sh + (uint32_t)tile_bytes;
            const uint32_t a_lo = (lo + 15u) & ~15u, a_hi = hi & ~15u;
            if (a_lo >= a_hi) {
                for (uint32_t j = lo + threadIdx.x; j < hi; j += SEQ_TILE) dst[j] = stage[j];
            } else {
                if (lo + threadIdx.x < a_lo) dst[lo + threadIdx.x] = stage[lo + threadIdx.x];
                for (uint32_t q = (a_lo >> 4) + threadIdx.x; q < (a_hi >> 4); q += SEQ_TILE) ((uint4 *)dst)[q] = ((const uint4 *)stage)[q];
                if (a_hi + threadIdx.x < hi) dst[a_hi + threadIdx.x] = stage[a_hi + threadIdx.x];
            }
        }
        __syncthreads();
    }
    if (!ok) {  // (every thread that saw one stores the same value)
        *bad_dev = 1u;
        if (bad_host) *bad_host = 1ull;
    }
}

unsigned seq_grid(uint64_t n, unsigned max_blocks) {
    const uint64_t n_tiles = (n + SEQ_TILE - 1) / SEQ_TILE;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_tiles, max_blocks ? max_blocks : 1024u));
}

struct SeqScratch {  // [ticket u32, not renderable u32][total u64][tile_off u64 x n_tiles][tile_cnt u64 x n_tiles]
    uint32_t *ticket, *bad;
    uint64_t *total, *tile_off, *tile_cnt;
    SeqScratch(void *p, uint64_t n) {
        const uint64_t n_tiles = (n + SEQ_TILE - 1) / SEQ_TILE;
        ticket = (uint32_t *)p;
        bad = ticket + 1;
        total = (uint64_t *)((char *)p + 8);
        tile_off = (uint64_t *)((char *)p + 16);
        tile_cnt = tile_off + n_tiles;
    }
};

template <typename Src>
int seq_measure(const Src &src, uint64_t n, uint32_t k, void *scratch, uint64_t *total_host, hipStream_t s, unsigned max_blocks) {
    const SeqScratch X(scratch, n);
    PAG_HIP_TRY(hipMemsetAsync(scratch, 0, 16, s));
    k_seq_measure<Src><<<dim3(seq_grid(n, max_blocks)), dim3(SEQ_TILE), 0, s>>>(src, n, k, X.tile_cnt, X.tile_off, X.ticket, X.total, total_host);
    PAG_HIP_TRY(hipGetLastError());
    return PAG_OK;
}
template <typename Src>
int seq_render(const Src &src, uint64_t n, const SeqParams &P, const DumpTables &T, const SeqSources &S, void *scratch, char *out, uint64_t cap,
               uint64_t *bad_host, hipStream_t s, unsigned max_blocks) {
    const SeqScratch X(scratch, n);
    k_seq_render<Src><<<dim3(seq_grid(n, max_blocks)), dim3(SEQ_TILE), 0, s>>>(src, n, P, T, S, X.tile_off, X.total, (unsigned char *)out, cap, X.bad, bad_host);
    PAG_HIP_TRY(hipGetLastError());
    return PAG_OK;
}

size_t pad16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

// a pag_seqs is usable as a source: arrays present, every sequence inside the packed bytes
bool seqs_well_formed(const pag_seqs *q) {
    if (!q) return false;
    if (q->n_seqs == 0) return true;
    if (!q->byte_off || !q->len || (!q->packed && q->packed_bytes)) return false;
    for (uint64_t i = 0; i < q->n_seqs; ++i) {
        const uint64_t bytes = ((uint64_t)q->len[i] + 3) / 4;
        if (q->byte_off[i] > q->packed_bytes || bytes > q->packed_bytes - q->byte_off[i]) return false;
    }
    return true;
}

size_t seq_scratch_bytes(uint64_t n) { return (size_t)((16 + ((n + SEQ_TILE - 1) / SEQ_TILE) * 16 + 255) & ~(uint64_t)255); }

size_t seq_sources_bytes(const pag_seqs *ctgs, const pag_seqs *refs) {
    return pad16((ctgs->n_seqs + refs->n_seqs) * 8) + pad16(ctgs->packed_bytes) + pad16(refs->packed_bytes) + 16;
}
int seq_sources_upload(void *dev, const pag_seqs *ctgs, const pag_seqs *refs, SeqSources *out, hipStream_t s) {
    char *p = (char *)dev;
    out->coff = (const uint64_t *)p;
    out->roff = out->coff + ctgs->n_seqs;
    p += pad16((ctgs->n_seqs + refs->n_seqs) * 8);
    out->cpacked = (const uint8_t *)p;
    p += pad16(ctgs->packed_bytes);
    out->rpacked = (const uint8_t *)p;
    if (ctgs->n_seqs) PAG_HIP_TRY(hipMemcpyAsync((void *)out->coff, ctgs->byte_off, ctgs->n_seqs * 8, hipMemcpyHostToDevice, s));
    if (refs->n_seqs) PAG_HIP_TRY(hipMemcpyAsync((void *)out->roff, refs->byte_off, refs->n_seqs * 8, hipMemcpyHostToDevice, s));
    if (ctgs->packed_bytes) PAG_HIP_TRY(hipMemcpyAsync((void *)out->cpacked, ctgs->packed, ctgs->packed_bytes, hipMemcpyHostToDevice, s));
    if (refs->packed_bytes) PAG_HIP_TRY(hipMemcpyAsync((void *)out->rpacked, refs->packed, refs->packed_bytes, hipMemcpyHostToDevice, s));
    return PAG_OK;
}

int trav_launch_seq_path(TravGraph G, const uint32_t *seq_v, const uint32_t *seq_s, uint64_t len, const SeqParams &P, const DumpTables &T,
                         const SeqSources &S, void *scratch, char *out, uint64_t cap, uint64_t *head_host, hipStream_t s, unsigned max_blocks) {
    const SeqSrcPath src{G, seq_v, seq_s};
    int rc = seq_measure(src, len, P.k, scratch, head_host, s, max_blocks);
    return rc ? rc : seq_render(src, len, P, T, S, scratch, out, cap, head_host ? head_host + 1 : nullptr, s, max_blocks);
}

}  // namespace pagdev

using namespace pagdev;

extern "C" int pag_render_path_sequence(const pag_path_node *records, uint64_t n, uint32_t k, const pag_seqs *ctgs, const pag_seqs *refs, uint64_t deviation,
                                        double error_rate, char *out, uint64_t cap, uint64_t *bytes, int device) {
    if (bytes) *bytes = 0;
    if (!bytes || (n && !records) || k < 1 || k > 16 || !seqs_well_formed(ctgs) || !seqs_well_formed(refs) || (cap && !out)) {
        set_error("pag_render_path_sequence: bad argument (k = 1..16, `bytes` must be given, every sequence inside its packed bytes)");
        return PAG_EINVAL;
    }
    std::vector<uint32_t> blob;
    if (!dump_tables_build(ctgs->len, ctgs->n_seqs, refs->len, refs->n_seqs, blob)) {
        set_error("pag_render_path_sequence: the coordinate space of the contigs or of the references does not fit 32 bits (or more than %u sequences)", DUMP_MAX_SEQS);
        return PAG_EINVAL;
    }
    uint64_t total = n ? k : 0;  // (known without a device: the measure launch below is what the render launch reads its offsets from)
    for (uint64_t i = 1; i < n; ++i) total += records[i].step > 0 ? (uint64_t)records[i].step : 0ull;
    *bytes = total;
    if (!pag_device_available()) return PAG_ENODEV;  // (no CPU fallback)
    if (n == 0) return PAG_OK;
    if (total > cap) {
        set_error("pag_render_path_sequence: the sequence takes %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)cap);
        return PAG_ERANGE;
    }
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1, (void)hipGetLastError();
    PAG_HIP_TRY(hipSetDevice(device));
    struct Bufs {  // (a stream and the buffers of this one call; the caller's current device is put back at every exit)
        void *rec = nullptr, *tab = nullptr, *seqs = nullptr, *scratch = nullptr, *text = nullptr;
        hipStream_t s = nullptr;
        int back = -1;
        ~Bufs() {
            hipFree(rec), hipFree(tab), hipFree(seqs), hipFree(scratch), hipFree(text);
            if (s) hipStreamDestroy(s);
            if (back >= 0) (void)hipSetDevice(back);
        }
    } b;
    b.back = caller_device == device ? -1 : caller_device;
    PAG_HIP_TRY(hipStreamCreateWithFlags(&b.s, hipStreamNonBlocking));
    PAG_HIP_TRY(hipMalloc(&b.rec, n * sizeof(pag_path_node)));
    PAG_HIP_TRY(hipMalloc(&b.tab, blob.size() * 4 + 16));
    PAG_HIP_TRY(hipMalloc(&b.seqs, seq_sources_bytes(ctgs, refs)));
    PAG_HIP_TRY(hipMalloc(&b.scratch, seq_scratch_bytes(n)));
    PAG_HIP_TRY(hipMalloc(&b.text, total + 16));
    PAG_HIP_TRY(hipMemcpyAsync(b.rec, records, n * sizeof(pag_path_node), hipMemcpyHostToDevice, b.s));
    if (!blob.empty()) PAG_HIP_TRY(hipMemcpyAsync(b.tab, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, b.s));
    SeqSources S{};
    int rc = seq_sources_upload(b.seqs, ctgs, refs, &S, b.s);
    if (rc) return rc;
    const DumpTables T = dump_tables_at((const uint32_t *)b.tab, ctgs->n_seqs, refs->n_seqs);
    const SeqParams P{k, deviation, error_rate};
    const SeqSrcRecords src{(const pag_path_node *)b.rec};
    if ((rc = seq_measure(src, n, k, b.scratch, nullptr, b.s, 0))) return rc;
    if ((rc = seq_render(src, n, P, T, S, b.scratch, (char *)b.text, total, nullptr, b.s, 0))) return rc;
    uint64_t head[2] = {0, 0};  // [ticket, not renderable][total]
    PAG_HIP_TRY(hipMemcpyAsync(head, b.scratch, 16, hipMemcpyDeviceToHost, b.s));
    PAG_HIP_TRY(hipStreamSynchronize(b.s));
    if (head[1] != total) {
        set_error("pag_render_path_sequence: the device measured %llu bytes, the records give %llu", (unsigned long long)head[1], (unsigned long long)total);
        return PAG_EFAULT;
    }
    if (head[0] >> 32) {
        set_error("pag_render_path_sequence: not renderable (a step's rounded position is negative or not finite)");
        return PAG_EDOM;
    }
    PAG_HIP_TRY(hipMemcpy(out, b.text, total, hipMemcpyDeviceToHost));
    return PAG_OK;
}
