// k5_dump.hip — the body of a per-contig path dump (<prefix><contig>_<0|1>.txt) rendered on the device.
//
// One line per path vertex, in path order (PAssembly.cpp:47-60 through SeqTools::vertexString; host restatement:
// csrc/host/assembly.cpp):
//     <KMER>,<ctg>,<ref>,<cnt>\t<step>\t<cIdx>,<cOff>\t<rIdx>,<rOff>\n
// with (cIdx, cOff) / (rIdx, rOff) = PositionMapper::singleToDual over the contigs / the references.
//
// Two launches over tiles of 256 lines, k_dump_measure and k_dump_render: the skeleton they share with the consensus
// sequence's renderer (k5_seq.hip) is text_tiles.hpp — measure and scan, staging, the copy-out, the sources of the records.
// The lines are formatted from a vertex's values by functions that know nothing of the graph.
#include <algorithm>
#include <vector>

#include "pag_device.hpp"
#include "pag_travel.hpp"
#include "text_tiles.hpp"

namespace pagdev {

namespace {

// the longest line: k = 16, two 10-digit coordinates, a 5-digit count, an 11-character step, and per coordinate space an index
// of at most 10 and an offset of at most 11 characters (dump_tables_build keeps the tables inside those bounds), 9 separators
constexpr uint32_t DUMP_MAX_LINE = 16 + 10 + 10 + 5 + 11 + 2 * (10 + 11) + 9;
static_assert(DUMP_MAX_LINE == 103, "line bound");
constexpr uint32_t DUMP_STAGE_BYTES = TEXT_TILE * 104 + 16;  // (+ 16: a tile is staged at the output's alignment)

struct DumpFields {
    uint32_t code, ctg, ref, cnt;
    int32_t step, cidx, ridx;
    int64_t coff, roff;
};

__device__ __forceinline__ uint32_t digits_u32(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
__device__ __forceinline__ uint32_t digits_u64(uint64_t v) {
    if (v <= 0xFFFFFFFFull) return digits_u32((uint32_t)v);
    uint32_t d = 10;  // (v >= 2^32 > 10^9)
    uint64_t p = 10000000000ull;
    while (d < 20 && v >= p) {
        ++d;
        if (d < 20) p *= 10ull;
    }
    return d;
}
__device__ __forceinline__ uint32_t chars_i64(int64_t v) { return v < 0 ? 1u + digits_u64(0ull - (uint64_t)v) : digits_u64((uint64_t)v); }

__device__ __forceinline__ uint32_t dump_line_len(const DumpFields &f, uint32_t k) {
    return k + 9u + digits_u32(f.ctg) + digits_u32(f.ref) + digits_u32(f.cnt) + chars_i64(f.step) + chars_i64(f.cidx) + chars_i64(f.coff) + chars_i64(f.ridx) +
           chars_i64(f.roff);
}

// decimal digits of v, written backwards from p; returns the new front
__device__ __forceinline__ uint32_t put_back_u64(unsigned char *stage, uint32_t p, uint64_t v) {
    while (v > 0xFFFFFFFFull) {
        const uint64_t q = v / 10ull;
        stage[--p] = (unsigned char)('0' + (uint32_t)(v - q * 10ull));
        v = q;
    }
    uint32_t w = (uint32_t)v;
    do {
        const uint32_t q = w / 10u;
        stage[--p] = (unsigned char)('0' + (w - q * 10u));
        w = q;
    } while (w);
    return p;
}
__device__ __forceinline__ uint32_t put_back_i64(unsigned char *stage, uint32_t p, int64_t v) {
    p = put_back_u64(stage, p, v < 0 ? 0ull - (uint64_t)v : (uint64_t)v);
    if (v < 0) stage[--p] = '-';
    return p;
}
// the line of f into stage[at, at + len): written from its end, so that no field's width has to be known twice
__device__ __forceinline__ void dump_line_write(unsigned char *stage, uint32_t at, uint32_t len, const DumpFields &f, uint32_t k) {
    uint32_t p = at + len;
    stage[--p] = '\n';
    p = put_back_i64(stage, p, f.roff);
    stage[--p] = ',';
    p = put_back_i64(stage, p, f.ridx);
    stage[--p] = '\t';
    p = put_back_i64(stage, p, f.coff);
    stage[--p] = ',';
    p = put_back_i64(stage, p, f.cidx);
    stage[--p] = '\t';
    p = put_back_i64(stage, p, f.step);
    stage[--p] = '\t';
    p = put_back_u64(stage, p, f.cnt);
    stage[--p] = ',';
    p = put_back_u64(stage, p, f.ref);
    stage[--p] = ',';
    p = put_back_u64(stage, p, f.ctg);
    stage[--p] = ',';
    uint32_t c = f.code;  // (HostGraph::kmerString: the first base is the most significant pair)
    for (uint32_t i = 0; i < k; ++i) {
        stage[--p] = (unsigned char)((0x54474341u >> ((c & 3u) * 8u)) & 0xFFu);  // "ACGT"
        c >>= 2;
    }
}

// the start tables of both coordinate spaces in LDS when they fit (DUMP_LDS_STARTS entries), else where they are
template <bool LDS_T>
struct StartTables {
    const uint32_t *c, *r;
    __device__ __forceinline__ StartTables(const DumpTables &T, uint32_t *lds) {
        if (LDS_T) {
            const uint32_t nc = T.nc ? T.nc + 1u : 0u, nr = T.nr ? T.nr + 1u : 0u;
            for (uint32_t i = threadIdx.x; i < nc; i += blockDim.x) lds[i] = T.cstart[i];
            for (uint32_t i = threadIdx.x; i < nr; i += blockDim.x) lds[nc + i] = T.rstart[i];
            __syncthreads();
            c = lds;
            r = lds + nc;
        } else {
            c = T.cstart;
            r = T.rstart;
        }
    }
};

template <typename Src, bool LDS_T>
__device__ __forceinline__ DumpFields dump_fields(const Src &src, uint64_t i, const DumpTables &T, const uint32_t *cst, const uint32_t *rst) {
    const PathVertex n = src(i);
    DumpFields f;
    f.code = n.code;
    f.ctg = n.ctg;
    f.ref = n.ref;
    f.cnt = n.cnt;
    f.step = n.step;
    single_to_dual(cst, T.csize, T.nc, n.ctg, &f.cidx, &f.coff);
    single_to_dual(rst, T.rsize, T.nr, n.ref, &f.ridx, &f.roff);
    return f;
}

// byte count of every tile of 256 lines; the last block to finish turns them into byte offsets and the total
template <typename Src, bool LDS_T>
__global__ void __launch_bounds__(TEXT_TILE) k_dump_measure(Src src, uint64_t n, uint32_t k, DumpTables T, uint64_t *__restrict__ tile_cnt,
                                                            uint64_t *__restrict__ tile_off, uint32_t *ticket, uint64_t *total_dev,
                                                            uint64_t *total_host) {
    __shared__ uint32_t tab[LDS_T ? DUMP_LDS_STARTS : 1];
    const StartTables<LDS_T> st(T, tab);
    text_measure(n, [&](uint64_t i) { return dump_line_len(dump_fields<Src, LDS_T>(src, i, T, st.c, st.r), k); }, tile_cnt, tile_off, ticket, total_dev, total_host);
}

template <typename Src, bool LDS_T>
__global__ void __launch_bounds__(TEXT_TILE) k_dump_render(Src src, uint64_t n, uint32_t k, DumpTables T, const uint64_t *__restrict__ tile_off,
                                                           const uint64_t *__restrict__ total_dev, unsigned char *out, uint64_t cap) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[DUMP_STAGE_BYTES];
    __shared__ uint32_t tab[LDS_T ? DUMP_LDS_STARTS : 1];
    if (*total_dev > cap) return;  // (nothing is written into a buffer that cannot take all of it)
    const StartTables<LDS_T> st(T, tab);
    out = as_global(out);
    const uint64_t n_tiles = (n + TEXT_TILE - 1) / TEXT_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * TEXT_TILE + threadIdx.x;
        uint32_t len = 0;
        DumpFields f{};
        if (i < n) {
            f = dump_fields<Src, LDS_T>(src, i, T, st.c, st.r);
            len = dump_line_len(f, k);
        }
        uint32_t tile_bytes;
        const uint32_t at = tile_offset(len, &tile_bytes);
        const uint64_t o = tile_off[tile];
        if (i < n) dump_line_write(stage, stage_shift(out, o) + at, len, f, k);
        tile_flush(stage, out, o, tile_bytes);
        __syncthreads();
    }
}

template <typename Src>
int dump_measure(const Src &src, uint64_t n, uint32_t k, const DumpTables &T, void *scratch, uint64_t *total_host, hipStream_t s, unsigned max_blocks) {
    const TextScratch S(scratch, n);
    const int rc = text_scratch_reset(scratch, s);
    if (rc) return rc;
    return text_launch(T.in_lds ? k_dump_measure<Src, true> : k_dump_measure<Src, false>, n, max_blocks, s, src, n, k, T, S.tile_cnt, S.tile_off, S.ticket, S.total,
                       total_host);
}
template <typename Src>
int dump_render(const Src &src, uint64_t n, uint32_t k, const DumpTables &T, void *scratch, char *out, uint64_t cap, hipStream_t s, unsigned max_blocks) {
    const TextScratch S(scratch, n);
    return text_launch(T.in_lds ? k_dump_render<Src, true> : k_dump_render<Src, false>, n, max_blocks, s, src, n, k, T, S.tile_off, S.total, (unsigned char *)out, cap);
}

uint32_t dec_digits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) v /= 10, ++d;
    return d;
}

}  // namespace

size_t text_scratch_bytes(uint64_t n) { return TextScratch::bytes(n); }

// PositionMapper's constructor (position_mapper.hpp:18-25) for both spaces, as u32: [cstart nc + 1][csize nc][rstart nr + 1][rsize nr]
bool dump_tables_build(const uint32_t *ctg_len, uint64_t n_ctgs, const uint32_t *ref_len, uint64_t n_refs, std::vector<uint32_t> &blob) {
    blob.clear();
    if (n_ctgs > DUMP_MAX_SEQS || n_refs > DUMP_MAX_SEQS) return false;
    const uint32_t *len[2] = {ctg_len, ref_len};
    const uint64_t cnt[2] = {n_ctgs, n_refs};
    for (int t = 0; t < 2; ++t) {
        const uint64_t n = cnt[t];
        if (n == 0) continue;
        uint64_t start = len[t][0];
        for (uint64_t i = 0; i < n; ++i) {
            if (start > 0xFFFFFFFFull) return false;
            blob.push_back((uint32_t)start);
            start += i + 1 < n ? 3ull * len[t][i] + std::max(len[t][i], len[t][i + 1]) : 4ull * len[t][i];
        }
        if (start > 0xFFFFFFFFull) return false;
        blob.push_back((uint32_t)start);
        for (uint64_t i = 0; i < n; ++i) blob.push_back(len[t][i]);
    }
    return true;
}
DumpTables dump_tables_at(const uint32_t *dev, uint64_t n_ctgs, uint64_t n_refs) {
    DumpTables T{};
    T.nc = (uint32_t)n_ctgs;
    T.nr = (uint32_t)n_refs;
    const uint32_t *p = dev;
    T.cstart = p;
    p += n_ctgs ? n_ctgs + 1 : 0;
    T.csize = p;
    p += n_ctgs;
    T.rstart = p;
    p += n_refs ? n_refs + 1 : 0;
    T.rsize = p;
    T.in_lds = (n_ctgs ? n_ctgs + 1 : 0) + (n_refs ? n_refs + 1 : 0) <= DUMP_LDS_STARTS ? 1u : 0u;
    return T;
}
// an upper bound of a line's length for coordinates that lie inside the tables (a path's vertices); a line beyond it — a
// coordinate before the first start prints a negative offset — makes the text exceed its buffer, and nothing is written
uint32_t dump_line_bound(uint32_t k, const std::vector<uint32_t> &blob, uint64_t n_ctgs, uint64_t n_refs) {
    const uint64_t cextra = n_ctgs ? blob[n_ctgs] : 0, rextra = n_refs ? blob[(n_ctgs ? 2 * n_ctgs + 1 : 0) + n_refs] : 0;
    return k + 9u + 2u * dec_digits(cextra) + 2u * dec_digits(rextra) + 5u + 11u + 1u + dec_digits(n_ctgs + 1) + 1u + dec_digits(n_refs + 1);
}

int trav_launch_dump_path(TravGraph G, const uint32_t *seq_v, const uint32_t *seq_s, uint64_t len, uint32_t k, const DumpTables &T, void *scratch,
                          char *out, uint64_t cap, uint64_t *head_host, hipStream_t s, unsigned max_blocks) {
    const PathSrcPath src{G, seq_v, seq_s};
    int rc = dump_measure(src, len, k, T, scratch, head_host, s, max_blocks);
    return rc ? rc : dump_render(src, len, k, T, scratch, out, cap, s, max_blocks);
}

}  // namespace pagdev

using namespace pagdev;

extern "C" int pag_render_dump_lines(const pag_path_node *records, uint64_t n, uint32_t k, const uint32_t *ctg_len, uint64_t n_ctgs, const uint32_t *ref_len,
                                     uint64_t n_refs, char *out, uint64_t cap, uint64_t *bytes, int device) {
    if (bytes) *bytes = 0;
    if (!bytes || (n && !records) || k < 1 || k > 16 || (n_ctgs && !ctg_len) || (n_refs && !ref_len) || (cap && !out)) {
        set_error("pag_render_dump_lines: bad argument (k = 1..16, `bytes` must be given)");
        return PAG_EINVAL;
    }
    std::vector<uint32_t> blob;
    if (!dump_tables_build(ctg_len, n_ctgs, ref_len, n_refs, blob)) {
        set_error("pag_render_dump_lines: the coordinate space of the contigs or of the references does not fit 32 bits (or more than %u sequences)", DUMP_MAX_SEQS);
        return PAG_EINVAL;
    }
    if (!pag_device_available()) return PAG_ENODEV;  // (no CPU fallback)
    if (n == 0) return PAG_OK;
    TextCall b("pag_render_dump_lines");
    char *scratch = nullptr, *text = nullptr;
    int rc = b.begin(device, n, blob);
    if (rc || (rc = b.alloc(&scratch, text_scratch_bytes(n))) || (rc = b.upload(records, n, blob))) return rc;
    const DumpTables T = dump_tables_at(b.tab, n_ctgs, n_refs);
    const PathSrcRecords src{b.rec};
    if ((rc = dump_measure(src, n, k, T, scratch, nullptr, b.s, 0))) return rc;
    uint64_t total = 0;
    PAG_HIP_TRY(hipMemcpyAsync(&total, (char *)scratch + 8, 8, hipMemcpyDeviceToHost, b.s));
    PAG_HIP_TRY(hipStreamSynchronize(b.s));
    *bytes = total;
    if (total > cap) {
        set_error("pag_render_dump_lines: the text takes %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)cap);
        return PAG_ERANGE;
    }
    if ((rc = b.alloc(&text, total + 16)) || (rc = dump_render(src, n, k, T, scratch, (char *)text, total, b.s, 0))) return rc;
    PAG_HIP_TRY(hipMemcpyAsync(out, text, total, hipMemcpyDeviceToHost, b.s));
    PAG_HIP_TRY(hipStreamSynchronize(b.s));
    return PAG_OK;
}
