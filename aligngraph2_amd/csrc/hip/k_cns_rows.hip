// k_cns_rows.hip — pa_cns's rows on the device (PA_CNS_INGEST=device): every kept slice of the 3-line ALN text is cut
// (slice_bounds) and gap-normalised (normalize_gaps) by the code of cns_rows.hpp, and the rows stay in device memory, where the
// graph kernels (k_cns.hip, k_cns_wave.hip) read them next.
//
// Shape.  The push-right pass of normalize_gaps is a chain of dependent byte accesses: nothing inside a slice can be spread over
// lanes, the parallelism is the number of slices (10^5 - 10^6 per Mb of backbone).  So a LANE runs a slice, 64 slices per
// wavefront, neighbours in text order (records of similar length).  The rows a lane works on — up to twice the slice's columns
// after the mismatch expansion — are kept in a per-wave region of global memory COLUMN BY COLUMN: column i of lane l is byte
// i * 64 + l, so the 64 lanes' accesses at the same column fall into one 64-byte segment instead of 64 cache lines (LDS cannot
// hold them: 64 lanes x 2 rows x 2 x ~5 000 columns is over a megabyte per wave).  The lanes read their input rows from the text
// and write the normalised rows into their pool slots once each, a sequential byte stream per lane.  A fixed number of waves
// walks the groups of 64 slices, so the work rows are allocated once.
//
// A slice with more columns than the work rows hold (PA_CNS_ROWS_STAGE_COLS, expanded columns per lane) is flagged by its lane
// and normalised by the same code on the host; its rows are then uploaded into its slot.  The text goes up in pieces
// (PA_CNS_ROWS_PIECE_BYTES caps a piece; by default what the memory budget, free memory x 0.8, leaves, at most 1 GiB).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "cns_device.hpp"
#include "cns_rows.hpp"

struct pag_cns_rows {
    int device = 0;
    char *d_q = nullptr, *d_t = nullptr;
    uint64_t pool_bytes = 0;
    double s_upload = 0.0, s_kernels = 0.0;
    uint64_t n_pieces = 0, n_oversize = 0;
};

namespace pagdev {

static_assert(sizeof(pag_cns_slice) == sizeof(pagrows::Slice) && sizeof(pag_cns_row) == sizeof(pagrows::Row), "pag_cns_slice / pag_cns_row are pagrows::Slice / Row");

// slices[0 .. n): of one piece of the text (text[0] is byte `base` of the file).  Wave w takes the groups w, w + waves, ...
__global__ __launch_bounds__(64) void cns_rows_kernel(const char *__restrict__ text, uint64_t base, const pagrows::Slice *__restrict__ slices, uint32_t n,
                                                       uint32_t stage_cols, char *__restrict__ work, char *qpool, char *tpool, pagrows::Row *__restrict__ rows) {
    const uint32_t lane = threadIdx.x;
    char *wq = work + (uint64_t)blockIdx.x * 2u * stage_cols * PAG_WAVE + lane;
    char *wt = wq + (uint64_t)stage_cols * PAG_WAVE;
    for (uint64_t g = blockIdx.x; g * PAG_WAVE < n; g += gridDim.x) {
        const uint64_t s = g * PAG_WAVE + lane;
        if (s >= n) continue;
        pagrows::Slice S = slices[s];
        S.q_off -= base;
        S.t_off -= base;
        rows[s] = pagrows::run_slice(text, S, wq, wt, PAG_WAVE, stage_cols, qpool, tpool);
    }
}

namespace {
using Clock = std::chrono::steady_clock;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

struct Buf {  // one device allocation, freed on every way out
    void *p = nullptr;
    ~Buf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    int alloc(size_t bytes) {
        release();
        if (hipMalloc(&p, std::max<size_t>(bytes, 64)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            set_error("pag_cns_normalize: out of device memory (%zu bytes)", bytes);
            return PAG_ENOMEM;
        }
        return PAG_OK;
    }
};

constexpr uint64_t kPieceSlices = 1u << 20;  // descriptors per piece at the most (64 + 24 bytes each)
constexpr uint64_t kMaxWaves = 2048;         // 8 per CU
}  // namespace

static int cns_normalize(int device, const char *text, uint64_t text_bytes, const pag_cns_slice *slices, uint64_t n_slices, pag_cns_row *rows, pag_cns_rows *H) {
    // what the kernel's indices rely on
    uint64_t pool_bytes = 0;
    for (uint64_t s = 0; s < n_slices; ++s) {
        const pag_cns_slice &S = slices[s];
        if (S.t_off < S.q_off || S.t_off > text_bytes || S.n_cols > text_bytes - S.t_off || S.n_cols >= 0x80000000u || S.slot >= n_slices ||
            (s && S.q_off < slices[s - 1].q_off) || S.out_off > (1ull << 62)) {
            set_error("pag_cns_normalize: slice %llu is out of the text, out of order (q_off must not decrease, the target row follows the query row) or names no slot",
                      (unsigned long long)s);
            return PAG_EINVAL;
        }
        pool_bytes = std::max(pool_bytes, S.out_off + S.out_cap);
    }
    H->device = device;
    H->pool_bytes = pool_bytes;
    size_t free_b = 0, total_b = 0;
    PAG_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = (uint64_t)((double)free_b * 0.8);
    if (2 * (pool_bytes + 64) > budget) {
        set_error("pag_cns_normalize: the two pools need %llu bytes of device memory, %llu are free", (unsigned long long)(2 * pool_bytes), (unsigned long long)free_b);
        return PAG_ENOMEM;
    }
    for (char **p : {&H->d_q, &H->d_t})
        if (hipMalloc((void **)p, pool_bytes + 64) != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            set_error("pag_cns_normalize: out of device memory (%llu bytes)", (unsigned long long)pool_bytes);
            return PAG_ENOMEM;
        }
    if (!n_slices) return PAG_OK;
    // the work rows, then the text piece, out of what the budget leaves
    const uint32_t stage_cols = (uint32_t)std::min<long long>(std::max<long long>(env_int("PA_CNS_ROWS_STAGE_COLS", 16384), 2), 1 << 20);
    const uint64_t per_piece = std::min<uint64_t>(n_slices, kPieceSlices), wave_bytes = 2ull * stage_cols * PAG_WAVE;
    const uint64_t fixed = per_piece * (sizeof(pagrows::Slice) + sizeof(pagrows::Row));
    uint64_t rem = budget - 2 * (pool_bytes + 64);
    if (fixed + wave_bytes >= rem) {
        set_error("pag_cns_normalize: %llu bytes of device memory are left for the work rows and the text", (unsigned long long)rem);
        return PAG_ENOMEM;
    }
    rem -= fixed;
    const uint64_t waves = std::max<uint64_t>(1, std::min({kMaxWaves, (per_piece + PAG_WAVE - 1) / PAG_WAVE, rem / 2 / wave_bytes}));
    rem -= waves * wave_bytes;
    const long long piece_env = env_int("PA_CNS_ROWS_PIECE_BYTES", 0);
    const uint64_t piece_bytes = std::max<uint64_t>(1, std::min<uint64_t>(piece_env > 0 ? (uint64_t)piece_env : (1ull << 30), rem));
    Buf work, d_text, d_slices, d_rows;
    int rc;
    if ((rc = work.alloc(waves * wave_bytes)) || (rc = d_slices.alloc(per_piece * sizeof(pagrows::Slice))) || (rc = d_rows.alloc(per_piece * sizeof(pagrows::Row)))) return rc;
    uint64_t text_cap = 0;
    std::vector<pagrows::Row> got;
    std::vector<char> hq, ht;
    for (uint64_t s0 = 0; s0 < n_slices;) {
        // a piece: slices s0 .. s1 whose rows lie in text[base, end)
        const uint64_t base = slices[s0].q_off;
        uint64_t end = base, s1 = s0;
        while (s1 < n_slices && s1 - s0 < kPieceSlices) {
            const uint64_t e2 = slices[s1].t_off + slices[s1].n_cols;  // (<= text_bytes, and the query row ends no later: checked above)
            if (std::max(end, e2) - base > piece_bytes && s1 > s0) break;
            end = std::max(end, e2);
            ++s1;
        }
        const uint64_t n = s1 - s0, bytes = end - base;
        ++H->n_pieces;
        if (bytes > text_cap) {
            if ((rc = d_text.alloc(bytes))) return rc;
            text_cap = bytes;
        }
        auto t0 = Clock::now();
        if (bytes) PAG_HIP_TRY(hipMemcpy(d_text.p, text + base, bytes, hipMemcpyHostToDevice));
        PAG_HIP_TRY(hipMemcpy(d_slices.p, slices + s0, n * sizeof(pagrows::Slice), hipMemcpyHostToDevice));
        H->s_upload += since(t0);
        t0 = Clock::now();
        const uint32_t grid = (uint32_t)std::min<uint64_t>(waves, (n + PAG_WAVE - 1) / PAG_WAVE);
        cns_rows_kernel<<<dim3(grid), dim3(PAG_WAVE), 0, 0>>>((const char *)d_text.p, base, (const pagrows::Slice *)d_slices.p, (uint32_t)n, stage_cols, (char *)work.p,
                                                               H->d_q, H->d_t, (pagrows::Row *)d_rows.p);
        PAG_HIP_TRY(hipGetLastError());
        PAG_HIP_TRY(hipDeviceSynchronize());
        H->s_kernels += since(t0);
        got.resize(n);
        PAG_HIP_TRY(hipMemcpy(got.data(), d_rows.p, n * sizeof(pagrows::Row), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) {
            const pag_cns_slice &S = slices[s0 + i];
            pagrows::Row R = got[i];
            if (R.flag == pagrows::ROW_OVERSIZE) {  // the same code on the host, its rows into the slot
                ++H->n_oversize;
                pagrows::Slice T;
                static_assert(sizeof(T) == sizeof(S), "");
                memcpy(&T, &S, sizeof(T));
                T.out_off = 0;
                hq.resize(std::max<size_t>(T.out_cap, 1));
                ht.resize(std::max<size_t>(T.out_cap, 1));
                R = pagrows::run_slice(text, T, nullptr, nullptr, 1, 0, hq.data(), ht.data());
                R.str_off = S.out_off;
                if (R.flag == pagrows::ROW_OK && R.len) {
                    t0 = Clock::now();
                    PAG_HIP_TRY(hipMemcpy(H->d_q + S.out_off, hq.data(), R.len, hipMemcpyHostToDevice));
                    PAG_HIP_TRY(hipMemcpy(H->d_t + S.out_off, ht.data(), R.len, hipMemcpyHostToDevice));
                    H->s_upload += since(t0);
                }
            }
            if (R.flag != pagrows::ROW_OK) {
                set_error("pag_cns_normalize: slice %llu has %u columns, its slot holds %u (twice the columns are needed)", (unsigned long long)(s0 + i), R.len, S.out_cap);
                return PAG_ERANGE;
            }
            memcpy(&rows[S.slot], &R, sizeof(R));
        }
        s0 = s1;
    }
    return PAG_OK;
}

}  // namespace pagdev

extern "C" int pag_cns_normalize(int device, const char *text, uint64_t text_bytes, const pag_cns_slice *slices, uint64_t n_slices, pag_cns_row *rows,
                                 pag_cns_rows **out) {
    if (!out || (!text && text_bytes) || (n_slices && (!slices || !rows))) return PAG_EINVAL;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        (void)hipGetLastError();
        pagdev::set_error("pag_cns_normalize: no gfx950 device %d (the rows are made on the device; PA_CNS_INGEST=flat makes them on host threads)", device);
        return PAG_ENODEV;
    }
    PAG_HIP_TRY(hipSetDevice(device));
    pag_cns_rows *H = new pag_cns_rows();
    const int rc = pagdev::cns_normalize(device, text, text_bytes, slices, n_slices, rows, H);
    if (rc != PAG_OK) {
        pag_cns_rows_free(H);
        return rc;
    }
    *out = H;
    return PAG_OK;
}

extern "C" uint64_t pag_cns_rows_bytes(const pag_cns_rows *r) { return r ? r->pool_bytes : 0; }

extern "C" void pag_cns_rows_times(const pag_cns_rows *r, double *s_upload, double *s_kernels) {
    if (s_upload) *s_upload = r ? r->s_upload : 0.0;
    if (s_kernels) *s_kernels = r ? r->s_kernels : 0.0;
}

extern "C" void pag_cns_rows_counts(const pag_cns_rows *r, uint64_t *n_pieces, uint64_t *n_oversize) {
    if (n_pieces) *n_pieces = r ? r->n_pieces : 0;
    if (n_oversize) *n_oversize = r ? r->n_oversize : 0;
}

extern "C" int pag_cns_rows_fetch(const pag_cns_rows *r, char *qpool, char *tpool, uint64_t pool_bytes) {
    if (!r || !qpool || !tpool || pool_bytes < r->pool_bytes) return PAG_EINVAL;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || r->device >= n_dev) {
        (void)hipGetLastError();
        pagdev::set_error("pag_cns_rows_fetch: no gfx950 device %d", r->device);
        return PAG_ENODEV;
    }
    PAG_HIP_TRY(hipSetDevice(r->device));
    if (r->pool_bytes) {
        PAG_HIP_TRY(hipMemcpy(qpool, r->d_q, r->pool_bytes, hipMemcpyDeviceToHost));
        PAG_HIP_TRY(hipMemcpy(tpool, r->d_t, r->pool_bytes, hipMemcpyDeviceToHost));
    }
    return PAG_OK;
}

extern "C" void pag_cns_rows_free(pag_cns_rows *r) {
    if (!r) return;
    if (r->d_q) (void)hipFree(r->d_q);
    if (r->d_t) (void)hipFree(r->d_t);
    delete r;
}

extern "C" int pag_cns_consensus_rows(int device, int wave, const char *backbone, uint64_t backbone_len, const pag_cns_part *parts, uint64_t n_parts,
                                      const pag_cns_aln *alns, uint64_t n_alns, const pag_cns_rows *rows, int32_t min_weight, char *out, uint64_t out_bytes,
                                      uint64_t *out_off, uint32_t *out_len, int32_t *part_err) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        (void)hipGetLastError();
        pagdev::set_error("pag_cns_consensus_rows: no gfx950 device %d", device);
        return PAG_ENODEV;
    }
    if (!rows || rows->device != device || !rows->d_q || !rows->d_t) return PAG_EINVAL;
    for (uint64_t a = 0; a < n_alns && alns; ++a)
        if (alns[a].str_off > rows->pool_bytes || alns[a].len > rows->pool_bytes - alns[a].str_off) {
            pagdev::set_error("pag_cns_consensus_rows: alignment %llu lies outside the pools", (unsigned long long)a);
            return PAG_EINVAL;
        }
    return pagdev::cns_consensus_batched("pag_cns_consensus_rows", wave ? pagdev::cns_launcher_wave() : pagdev::cns_launcher_lane(), device, backbone, backbone_len, parts,
                                         n_parts, alns, n_alns, nullptr, nullptr, rows->pool_bytes, min_weight, out, out_bytes, out_off, out_len, part_err, rows->d_q,
                                         rows->d_t);
}
