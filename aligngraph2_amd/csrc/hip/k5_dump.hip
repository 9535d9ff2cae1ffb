// k5_dump.hip — the body of a per-contig path dump (<prefix><contig>_<0|1>.txt) rendered on the device.
//
// One line per path vertex, in path order (PAssembly.cpp:47-60 through SeqTools::vertexString; host restatement:
// csrc/host/assembly.cpp):
//     <KMER>,<ctg>,<ref>,<cnt>\t<step>\t<cIdx>,<cOff>\t<rIdx>,<rOff>\n
// with (cIdx, cOff) / (rIdx, rOff) = PositionMapper::singleToDual over the contigs / the references.
//
// Two launches.  k_dump_measure: a thread per vertex computes its line's length, a tile of 256 lines leaves its byte count,
// and the block that finishes last scans the tile counts into byte offsets and the total.  k_dump_render: a tile's threads
// format their lines into an LDS staging buffer at their prefix offsets, then the block copies the staged bytes to the output
// with 16-byte stores (the tile's unaligned head and tail byte by byte).  The output may be pinned host memory: what
// reaches it are whole 16-byte stores of consecutive lanes.
//
// The lines are formatted from pag_path_node values by functions that know nothing of the graph; the records come either from
// an array (pag_render_dump_lines) or from the traversal view and a path's vertex ids (pag_travel's deliveries, where they are
// the records k_gather_path writes).
#include <algorithm>
#include <vector>

#include "pag_device.hpp"
#include "pag_travel.hpp"

namespace pagdev {

namespace {

constexpr uint32_t DUMP_TILE = 256;
// the longest line: k = 16, two 10-digit coordinates, a 5-digit count, an 11-character step, and per coordinate space an index
// of at most 10 and an offset of at most 11 characters (dump_tables_build keeps the tables inside those bounds), 9 separators
constexpr uint32_t DUMP_MAX_LINE = 16 + 10 + 10 + 5 + 11 + 2 * (10 + 11) + 9;
static_assert(DUMP_MAX_LINE == 103, "line bound");
constexpr uint32_t DUMP_STAGE_BYTES = DUMP_TILE * 104 + 16;  // (+ 16: a tile is staged at the output's alignment)

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

// where the records come from
struct DumpSrcRecords {
    const pag_path_node *rec;
    __device__ __forceinline__ pag_path_node operator()(uint64_t i) const { return rec[i]; }
};
struct DumpSrcPath {  // what k_gather_path (k5_walk_aux.hip) writes for entry i of a path
    TravGraph G;
    const uint32_t *seq_v, *seq_s;
    __device__ __forceinline__ pag_path_node operator()(uint64_t i) const {
        const uint32_t v = G.uold[seq_v[i]];
        const uint64_t p = G.vpos[v];
        pag_path_node o;
        o.code = G.ncode[G.vnode[v]];
        o.ctg = (uint32_t)(p >> 32);
        o.ref = (uint32_t)p;
        o.cnt = G.vcnt[v];
        o.reserved = 0;
        o.step = (int32_t)seq_s[i];
        o.vid = v;
        return o;
    }
};

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
    const pag_path_node n = src(i);
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
__global__ void __launch_bounds__(DUMP_TILE) k_dump_measure(Src src, uint64_t n, uint32_t k, DumpTables T, uint32_t *__restrict__ tile_cnt,
                                                            uint64_t *__restrict__ tile_off, uint32_t *ticket, uint64_t *total_dev,
                                                            uint64_t *total_host) {
    __shared__ uint32_t tab[LDS_T ? DUMP_LDS_STARTS : 1];
    __shared__ uint64_t wsum[DUMP_TILE / PAG_WAVE];
    __shared__ uint32_t last;
    const StartTables<LDS_T> st(T, tab);
    const uint64_t n_tiles = (n + DUMP_TILE - 1) / DUMP_TILE;
    const uint32_t wave = threadIdx.x / PAG_WAVE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * DUMP_TILE + threadIdx.x;
        uint32_t len = 0;
        if (i < n) len = dump_line_len(dump_fields<Src, LDS_T>(src, i, T, st.c, st.r), k);
        const uint32_t w = wave_sum(len);
        if (lane_id() == 0) wsum[wave] = w;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[tile] = (uint32_t)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        __syncthreads();
    }
    // the counts of this block are visible device-wide before its ticket is
    __threadfence();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!last) return;
    __threadfence();
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += DUMP_TILE) {
        const uint64_t t = base + threadIdx.x;
        const uint64_t c = t < n_tiles ? (uint64_t)__hip_atomic_load(&tile_cnt[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
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

template <typename Src, bool LDS_T>
__global__ void __launch_bounds__(DUMP_TILE) k_dump_render(Src src, uint64_t n, uint32_t k, DumpTables T, const uint64_t *__restrict__ tile_off,
                                                           const uint64_t *__restrict__ total_dev, unsigned char *out, uint64_t cap) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[DUMP_STAGE_BYTES];
    __shared__ uint32_t tab[LDS_T ? DUMP_LDS_STARTS : 1];
    __shared__ uint32_t wsum[DUMP_TILE / PAG_WAVE];
    if (*total_dev > cap) return;  // (nothing is written into a buffer that cannot take all of it)
    const StartTables<LDS_T> st(T, tab);
    out = as_global(out);
    const uint64_t n_tiles = (n + DUMP_TILE - 1) / DUMP_TILE;
    const uint32_t wave = threadIdx.x / PAG_WAVE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t i = tile * DUMP_TILE + threadIdx.x;
        uint32_t len = 0;
        DumpFields f{};
        if (i < n) {
            f = dump_fields<Src, LDS_T>(src, i, T, st.c, st.r);
            len = dump_line_len(f, k);
        }
        uint32_t wtot;
        const uint32_t pre = wave_excl_sum(len, &wtot);
        if (lane_id() == 0) wsum[wave] = wtot;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
        const uint32_t tile_bytes = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        // the tile is staged at the alignment its bytes have in the output: 16-byte groups of the one are 16-byte groups of the other
        const uint64_t o = tile_off[tile];
        const uint32_t sh = (uint32_t)(((uintptr_t)out + o) & 15u);
        if (i < n) dump_line_write(stage, sh + before + pre, len, f, k);
        __syncthreads();
        unsigned char *dst = out + o - sh;  // (16-byte aligned; nothing below dst + sh is touched)
        const uint32_t lo = sh, hi = sh + tile_bytes;
        const uint32_t a_lo = (lo + 15u) & ~15u, a_hi = hi & ~15u;
        if (a_lo >= a_hi) {
            for (uint32_t j = lo + threadIdx.x; j < hi; j += DUMP_TILE) dst[j] = stage[j];
        } else {
            if (lo + threadIdx.x < a_lo) dst[lo + threadIdx.x] = stage[lo + threadIdx.x];
            for (uint32_t q = (a_lo >> 4) + threadIdx.x; q < (a_hi >> 4); q += DUMP_TILE) ((uint4 *)dst)[q] = ((const uint4 *)stage)[q];
            if (a_hi + threadIdx.x < hi) dst[a_hi + threadIdx.x] = stage[a_hi + threadIdx.x];
        }
        __syncthreads();
    }
}

unsigned dump_grid(uint64_t n, unsigned max_blocks) {
    const uint64_t n_tiles = (n + DUMP_TILE - 1) / DUMP_TILE;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n_tiles, max_blocks ? max_blocks : 1024u));
}

struct DumpScratch {  // [ticket u32, pad u32][total u64][tile_off u64 x n_tiles][tile_cnt u32 x n_tiles]
    uint32_t *ticket;
    uint64_t *total, *tile_off;
    uint32_t *tile_cnt;
    DumpScratch(void *p, uint64_t n) {
        const uint64_t n_tiles = (n + DUMP_TILE - 1) / DUMP_TILE;
        ticket = (uint32_t *)p;
        total = (uint64_t *)((char *)p + 8);
        tile_off = (uint64_t *)((char *)p + 16);
        tile_cnt = (uint32_t *)((char *)p + 16 + n_tiles * 8);
    }
};

template <typename Src>
int dump_measure(const Src &src, uint64_t n, uint32_t k, const DumpTables &T, void *scratch, uint64_t *total_host, hipStream_t s, unsigned max_blocks) {
    const DumpScratch S(scratch, n);
    PAG_HIP_TRY(hipMemsetAsync(scratch, 0, 16, s));
    const unsigned grid = dump_grid(n, max_blocks);
    if (T.in_lds) k_dump_measure<Src, true><<<dim3(grid), dim3(DUMP_TILE), 0, s>>>(src, n, k, T, S.tile_cnt, S.tile_off, S.ticket, S.total, total_host);
    else k_dump_measure<Src, false><<<dim3(grid), dim3(DUMP_TILE), 0, s>>>(src, n, k, T, S.tile_cnt, S.tile_off, S.ticket, S.total, total_host);
    PAG_HIP_TRY(hipGetLastError());
    return PAG_OK;
}
template <typename Src>
int dump_render(const Src &src, uint64_t n, uint32_t k, const DumpTables &T, void *scratch, char *out, uint64_t cap, hipStream_t s, unsigned max_blocks) {
    const DumpScratch S(scratch, n);
    const unsigned grid = dump_grid(n, max_blocks);
    if (T.in_lds) k_dump_render<Src, true><<<dim3(grid), dim3(DUMP_TILE), 0, s>>>(src, n, k, T, S.tile_off, S.total, (unsigned char *)out, cap);
    else k_dump_render<Src, false><<<dim3(grid), dim3(DUMP_TILE), 0, s>>>(src, n, k, T, S.tile_off, S.total, (unsigned char *)out, cap);
    PAG_HIP_TRY(hipGetLastError());
    return PAG_OK;
}

uint32_t dec_digits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) v /= 10, ++d;
    return d;
}

}  // namespace

size_t dump_scratch_bytes(uint64_t n) { return (size_t)((16 + ((n + DUMP_TILE - 1) / DUMP_TILE) * 12 + 255) & ~(uint64_t)255); }

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
                          char *out, uint64_t cap, uint64_t *total_host, hipStream_t s, unsigned max_blocks) {
    const DumpSrcPath src{G, seq_v, seq_s};
    int rc = dump_measure(src, len, k, T, scratch, total_host, s, max_blocks);
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
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1, (void)hipGetLastError();
    PAG_HIP_TRY(hipSetDevice(device));
    struct Bufs {  // (a stream and the buffers of this one call; the caller's current device is put back at every exit)
        void *rec = nullptr, *tab = nullptr, *scratch = nullptr, *text = nullptr;
        hipStream_t s = nullptr;
        int back = -1;
        ~Bufs() {
            hipFree(rec), hipFree(tab), hipFree(scratch), hipFree(text);
            if (s) hipStreamDestroy(s);
            if (back >= 0) (void)hipSetDevice(back);
        }
    } b;
    b.back = caller_device == device ? -1 : caller_device;
    PAG_HIP_TRY(hipStreamCreateWithFlags(&b.s, hipStreamNonBlocking));
    PAG_HIP_TRY(hipMalloc(&b.rec, n * sizeof(pag_path_node)));
    PAG_HIP_TRY(hipMalloc(&b.tab, blob.size() * 4 + 16));
    PAG_HIP_TRY(hipMalloc(&b.scratch, dump_scratch_bytes(n)));
    PAG_HIP_TRY(hipMemcpyAsync(b.rec, records, n * sizeof(pag_path_node), hipMemcpyHostToDevice, b.s));
    if (!blob.empty()) PAG_HIP_TRY(hipMemcpyAsync(b.tab, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, b.s));
    const DumpTables T = dump_tables_at((const uint32_t *)b.tab, n_ctgs, n_refs);
    const DumpSrcRecords src{(const pag_path_node *)b.rec};
    int rc = dump_measure(src, n, k, T, b.scratch, nullptr, b.s, 0);
    if (rc) return rc;
    uint64_t total = 0;
    PAG_HIP_TRY(hipMemcpyAsync(&total, (char *)b.scratch + 8, 8, hipMemcpyDeviceToHost, b.s));
    PAG_HIP_TRY(hipStreamSynchronize(b.s));
    *bytes = total;
    if (total > cap) {
        set_error("pag_render_dump_lines: the text takes %llu bytes, the buffer holds %llu", (unsigned long long)total, (unsigned long long)cap);
        return PAG_ERANGE;
    }
    PAG_HIP_TRY(hipMalloc(&b.text, total + 16));
    if ((rc = dump_render(src, n, k, T, b.scratch, (char *)b.text, total, b.s, 0))) return rc;
    PAG_HIP_TRY(hipMemcpyAsync(out, b.text, total, hipMemcpyDeviceToHost, b.s));
    PAG_HIP_TRY(hipStreamSynchronize(b.s));
    return PAG_OK;
}
