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
// Two launches over tiles of 256 vertices, k_seq_measure and k_seq_render, on the skeleton of text_tiles.hpp (shared with
// k5_dump.hip).  In the render launch one thread walks its own step serially; a tile with more bytes than the staging buffer
// holds (one step can be thousands of bases) writes straight to the output.
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
#include "text_tiles.hpp"

namespace pagdev {

namespace {

constexpr uint32_t SEQ_STAGE_BYTES = 16384;  // a tile's bytes when they are staged (a tile of short steps: ~1 KB)

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
__device__ __forceinline__ bool seq_vertex_write(unsigned char *dst, const Src &src, uint64_t i, const PathVertex &now, const SeqParams &P, const DumpTables &T,
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
    const PathVertex prev = src(i - 1);
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
__global__ void __launch_bounds__(TEXT_TILE) k_seq_measure(Src src, uint64_t n, uint32_t k, uint64_t *__restrict__ tile_cnt, uint64_t *__restrict__ tile_off,
                                                           uint32_t *ticket, uint64_t *total_dev, uint64_t *total_host) {
    text_measure(n, [&](uint64_t i) { return seq_vertex_len(i, src.step(i), k); }, tile_cnt, tile_off, ticket, total_dev, total_host);
}

template <typename Src>
__global__ void __launch_bounds__(TEXT_TILE) k_seq_render(Src src, uint64_t n, SeqParams P, DumpTables T, SeqSources S, const uint64_t *__restrict__ tile_off,
                                                          const uint64_t *__restrict__ total_dev, unsigned char *out, uint64_t cap, uint32_t *bad_dev,
                                                          uint64_t *bad_host) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[SEQ_STAGE_BYTES + 16];
    if (*total_dev > cap) return;  // (nothing is written into a buffer that cannot take all of it)
    out = as_global(out);
    const uint64_t n_tiles = (n + TEXT_TILE - 1) / TEXT_TILE;
    bool ok = true;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * TEXT_TILE + threadIdx.x;
        PathVertex v{};
        uint64_t len = 0;
        if (i < n) {
            v = src(i);
            len = seq_vertex_len(i, v.step, P.k);
        }
        uint64_t tile_bytes;
        const uint64_t at = tile_offset(len, &tile_bytes);
        const uint64_t o = tile_off[tile];  // (o + tile_bytes <= total <= cap)
        if (tile_bytes > SEQ_STAGE_BYTES) {
            // more than the staging buffer holds: every thread stores its bytes where they belong
            if (len) ok = seq_vertex_write(out + o + at, src, i, v, P, T, S) && ok;
        } else {
            if (len) ok = seq_vertex_write(stage + stage_shift(out, o) + (uint32_t)at, src, i, v, P, T, S) && ok;
            tile_flush(stage, out, o, (uint32_t)tile_bytes);
        }
        __syncthreads();
    }
    if (!ok) {  // (every thread that saw one stores the same value)
        *bad_dev = 1u;
        if (bad_host) *bad_host = 1ull;
    }
}

template <typename Src>
int seq_measure(const Src &src, uint64_t n, uint32_t k, void *scratch, uint64_t *total_host, hipStream_t s, unsigned max_blocks) {
    const TextScratch X(scratch, n);
    const int rc = text_scratch_reset(scratch, s);
    return rc ? rc : text_launch(k_seq_measure<Src>, n, max_blocks, s, src, n, k, X.tile_cnt, X.tile_off, X.ticket, X.total, total_host);
}
template <typename Src>
int seq_render(const Src &src, uint64_t n, const SeqParams &P, const DumpTables &T, const SeqSources &S, void *scratch, char *out, uint64_t cap,
               uint64_t *bad_host, hipStream_t s, unsigned max_blocks) {
    const TextScratch X(scratch, n);  // (flag: not renderable)
    return text_launch(k_seq_render<Src>, n, max_blocks, s, src, n, P, T, S, X.tile_off, X.total, (unsigned char *)out, cap, X.flag, bad_host);
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
    const PathSrcPath src{G, seq_v, seq_s};
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
    TextCall b("pag_render_path_sequence");
    char *seqs = nullptr, *scratch = nullptr, *text = nullptr;
    int rc = b.begin(device, n, blob);
    if (rc || (rc = b.alloc(&seqs, seq_sources_bytes(ctgs, refs))) || (rc = b.alloc(&scratch, text_scratch_bytes(n))) || (rc = b.alloc(&text, total + 16)) ||
        (rc = b.upload(records, n, blob)))
        return rc;
    SeqSources S{};
    if ((rc = seq_sources_upload(seqs, ctgs, refs, &S, b.s))) return rc;
    const DumpTables T = dump_tables_at(b.tab, ctgs->n_seqs, refs->n_seqs);
    const SeqParams P{k, deviation, error_rate};
    const PathSrcRecords src{b.rec};
    if ((rc = seq_measure(src, n, k, scratch, nullptr, b.s, 0))) return rc;
    if ((rc = seq_render(src, n, P, T, S, scratch, (char *)text, total, nullptr, b.s, 0))) return rc;
    uint64_t head[2] = {0, 0};  // [ticket, not renderable][total]
    PAG_HIP_TRY(hipMemcpyAsync(head, scratch, 16, hipMemcpyDeviceToHost, b.s));
    PAG_HIP_TRY(hipStreamSynchronize(b.s));
    if (head[1] != total) {
        set_error("pag_render_path_sequence: the device measured %llu bytes, the records give %llu", (unsigned long long)head[1], (unsigned long long)total);
        return PAG_EFAULT;
    }
    if (head[0] >> 32) {
        set_error("pag_render_path_sequence: not renderable (a step's rounded position is negative or not finite)");
        return PAG_EDOM;
    }
    PAG_HIP_TRY(hipMemcpy(out, text, total, hipMemcpyDeviceToHost));
    return PAG_OK;
}
