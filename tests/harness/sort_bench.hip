// Test and development aid (not shipped): times the radix-sort passes of k2_sort.hip on random records and checks
// the result against std::stable_sort on a sample size.  make tests/harness/bin/sort_bench; run on a GPU box:
//   sort_bench [n_records] [key_bits]
//   sort_bench check <keys> <n> <key_bits> [first_bit] [key_offset]     one sort of constructed keys, checked record for record (check_mode)
//   sort_bench scan <n> [offset]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../aligngraph2_amd/csrc/hip/util.hip"
#include "../../aligngraph2_amd/csrc/hip/k2_sort.hip"

using namespace pagdev;

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e = (x);                                                        \
        if (e != hipSuccess) {                                                     \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));            \
            return 2;                                                              \
        }                                                                          \
    } while (0)

// The payload of record i: the low half names the record (the stability check), the high half is a hash of it — non-zero and
// different from record to record, so a sort that drops or mixes the payloads' high halves cannot pass
__host__ __device__ inline uint64_t payload_of(uint64_t i) {
    uint64_t h = (i + 1) * 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    return (h | 0x8000000000000000ull) >> 32 << 32 | i;
}

__global__ void fill_random(uint32_t *k, uint64_t *v, uint64_t n, uint32_t mask) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t x = i * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 32;
        k[i] = (uint32_t)x & mask;
        v[i] = payload_of(i);
    }
}

// sort_bench scan <n> <offset>: scan_u32_to_u64 of n random values read from an array view that starts `offset` elements
// into its allocation (misaligned for the 16-byte path when offset % 4 != 0), against a sequential sum; timed
static int scan_mode(uint64_t n, uint64_t offset) {
    uint32_t *in;
    uint64_t *out, *total;
    void *tmp;
    CK(hipMalloc(&in, (n + offset + 8) * 4));
    CK(hipMalloc(&out, (n + offset + 8) * 8));
    CK(hipMalloc(&total, 8));
    CK(hipMalloc(&tmp, scan_tmp_bytes(n + 1) + 64));
    std::vector<uint32_t> h(n);
    std::mt19937_64 rng(n * 31 + offset);
    for (auto &x : h) x = (rng() % 16 == 0) ? (uint32_t)rng() : (uint32_t)(rng() % 7);  // (large values too: the sums pass 2^32)
    CK(hipMemcpy(in + offset, h.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(out, 0xEE, (n + offset + 8) * 8));
    float best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        hipEvent_t a, b;
        CK(hipEventCreate(&a));
        CK(hipEventCreate(&b));
        CK(hipEventRecord(a, 0));
        if (scan_u32_to_u64(in + offset, out + offset, n, total, tmp, 0) != PAG_OK) return 2;
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, a, b));
        best = std::min(best, ms);
    }
    std::vector<uint64_t> got(n + 1);
    uint64_t tot = 0;
    CK(hipMemcpy(got.data(), out + offset, (n + 1) * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&tot, total, 8, hipMemcpyDeviceToHost));
    uint64_t acc = 0, bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (got[i] != acc) ++bad;
        acc += h[i];
    }
    if (tot != acc) ++bad;
    if (got[n] != 0xEEEEEEEEEEEEEEEEull) ++bad;  // (nothing written past the end)
    std::printf("scan n=%llu offset=%llu: %.3f ms = %.0f GB/s (12 B per element), check: %llu mismatches\n", (unsigned long long)n,
                (unsigned long long)offset, best, n * 12.0 / best / 1e6, (unsigned long long)bad);
    return bad ? 1 : 0;
}

// persistent grid of sort_scatter, computed as sort_pairs computes it
static int scatter_grid_size(int *out) {
    int dev = 0, cus = 0, per_cu = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sort_scatter<8>, ST, 0));
    *out = cus * (per_cu > 0 ? per_cu : 1);
    return 0;
}

// sort_bench check <keys> <n> <key_bits> [first_bit] [key_offset]: one sort_pairs call on constructed keys, compared record for
// record with std::stable_sort on the sorted bit field [first_bit, first_bit + key_bits).
//   keys        uniform | equal | two (two values alternating by lane) | asc | desc | skew90 (nine in ten records hold one key) |
//               low_digit_const (the first pass finds one occupied bin) | top_digit_const (the last pass does); with first_bit > 0 the
//               keys are random 32-bit words whatever the name, and the bits outside the field must be carried along untouched
//   n           a number, or gA:B:D = (A * G + B) tiles of STILE records plus D records, G = the persistent grid of sort_scatter
//   key_offset  all four key arrays start this many elements into their allocation (1 .. 3: not 16-byte aligned, sort_hist's scalar
//               loads), the payload arrays one element (0: aligned).  Every array lies between guard words that must not change.
static int check_mode(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: sort_bench check <keys> <n> <key_bits> [first_bit] [key_offset]\n");
        return 2;
    }
    const std::string dist = argv[2];
    const int bits = std::atoi(argv[4]);
    const int first_bit = argc > 5 ? std::atoi(argv[5]) : 0;
    const uint64_t koff = argc > 6 ? std::strtoull(argv[6], nullptr, 10) : 0, voff = koff ? 1 : 0;
    int G = 0;
    if (scatter_grid_size(&G) != 0) return 2;
    long long n_ll;
    if (argv[3][0] == 'g') {
        long long a = 0, b = 0, d = 0;
        if (std::sscanf(argv[3], "g%lld:%lld:%lld", &a, &b, &d) != 3) return 2;
        n_ll = (a * G + b) * (long long)STILE + d;
    } else
        n_ll = std::atoll(argv[3]);
    if (n_ll <= 0 || n_ll > (1ll << 24) || bits <= 0 || first_bit < 0 || first_bit + bits > 32) {
        std::fprintf(stderr, "check: n = %lld (1 .. 2^24), bits [%d, %d) out of range\n", n_ll, first_bit, first_bit + bits);
        return 2;
    }
    const uint64_t n = (uint64_t)n_ll;
    const uint32_t mask = bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
    const int passes = (bits + 7) / 8, digit = (bits + passes - 1) / passes;
    std::printf("check %s n=%llu = %llu tiles %+lld, G=%d, bits [%d, %d), key offset %llu\n", dist.c_str(), (unsigned long long)n,
                (unsigned long long)((n + STILE - 1) / STILE), (long long)n - (long long)((n + STILE - 1) / STILE * STILE), G, first_bit,
                first_bit + bits, (unsigned long long)koff);
    std::vector<uint32_t> hk(n);
    std::vector<uint64_t> hv(n);
    std::mt19937_64 rng(n * 7 + (uint64_t)bits);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t u = (uint32_t)rng();
        uint32_t k;
        if (first_bit > 0) k = u;
        else if (dist == "uniform") k = u & mask;
        else if (dist == "equal") k = 0x0ABCDEF5u & mask;
        else if (dist == "two") k = ((i & 1u) ? 0x0ABCDEF5u : 0x05A5A5A5u) & mask;
        else if (dist == "asc") k = (uint32_t)((i * ((uint64_t)mask + 1)) / n);
        else if (dist == "desc") k = mask - (uint32_t)((i * ((uint64_t)mask + 1)) / n);
        else if (dist == "skew90") k = (u % 10u) ? (0x0ABCDEF5u & mask) : ((uint32_t)rng() & mask);
        else if (dist == "low_digit_const") k = ((u & mask) & ~((1u << digit) - 1u)) | (0x55u & ((1u << digit) - 1u));
        else if (dist == "top_digit_const") k = (u & (mask >> digit)) | ((0x5u << (bits - digit)) & mask);
        else {
            std::fprintf(stderr, "check: no key distribution '%s'\n", dist.c_str());
            return 2;
        }
        hk[i] = k;
        hv[i] = payload_of(i);
    }
    constexpr uint64_t GUARD = 64;
    const uint64_t kn = GUARD + koff + n + GUARD, vn = GUARD + voff + n + GUARD;
    uint32_t *kbuf[2];
    uint64_t *vbuf[2];
    void *tmp;
    for (int b = 0; b < 2; ++b) {
        CK(hipMalloc(&kbuf[b], kn * 4));
        CK(hipMalloc(&vbuf[b], vn * 8));
        CK(hipMemset(kbuf[b], 0xEE, kn * 4));
        CK(hipMemset(vbuf[b], 0xEE, vn * 8));
    }
    CK(hipMalloc(&tmp, sort_tmp_bytes(n)));
    CK(hipMemcpy(kbuf[0] + GUARD + koff, hk.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(vbuf[0] + GUARD + voff, hv.data(), n * 8, hipMemcpyHostToDevice));
    int in0 = 0, n_passes = 0;
    if (sort_pairs(kbuf[0] + GUARD + koff, vbuf[0] + GUARD + voff, kbuf[1] + GUARD + koff, vbuf[1] + GUARD + voff, n, bits, tmp, &in0, 0, nullptr,
                   &n_passes, first_bit) != PAG_OK) {
        std::fprintf(stderr, "sort failed: %s\n", last_error());
        return 2;
    }
    CK(hipDeviceSynchronize());
    uint64_t bad = 0;
    std::vector<uint32_t> rk(kn);
    std::vector<uint64_t> rv(vn);
    for (int turn = 0; turn < 2; ++turn) {  // (the buffer that holds the result last: it stays in rk / rv)
        const int b = turn == 0 ? (in0 ? 1 : 0) : (in0 ? 0 : 1);
        CK(hipMemcpy(rk.data(), kbuf[b], kn * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(rv.data(), vbuf[b], vn * 8, hipMemcpyDeviceToHost));
        uint64_t touched = 0;
        for (uint64_t i = 0; i < kn; ++i) touched += (i < GUARD + koff || i >= GUARD + koff + n) && rk[i] != 0xEEEEEEEEu;
        for (uint64_t i = 0; i < vn; ++i) touched += (i < GUARD + voff || i >= GUARD + voff + n) && rv[i] != 0xEEEEEEEEEEEEEEEEull;
        if (touched) std::printf("  %llu guard words around the arrays of buffer %d were written\n", (unsigned long long)touched, b);
        bad += touched;
    }
    std::vector<uint64_t> idx(n);
    for (uint64_t i = 0; i < n; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return ((hk[a] >> first_bit) & mask) < ((hk[b] >> first_bit) & mask); });
    uint64_t shown = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t gk = rk[GUARD + koff + i];
        const uint64_t gv = rv[GUARD + voff + i];
        const bool b = gk != hk[idx[i]] || gv != hv[idx[i]];
        if (b && shown++ < 8)
            std::printf("  [%llu] got key %08x val %016llx, expected key %08x val %016llx\n", (unsigned long long)i, gk, (unsigned long long)gv,
                        hk[idx[i]], (unsigned long long)hv[idx[i]]);
        bad += b ? 1 : 0;
    }
    std::printf("passes=%d check: %llu mismatches\n", n_passes, (unsigned long long)bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "check") return check_mode(argc, argv);
    if (argc > 2 && std::string(argv[1]) == "scan")
        return scan_mode(std::strtoull(argv[2], nullptr, 10), argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 0);
    const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 448810094ull;
    const int bits = argc > 2 ? std::atoi(argv[2]) : 28;
    const bool check = n <= (1ull << 24);
    uint32_t *k0, *k1;
    uint64_t *v0, *v1;
    void *tmp;
    CK(hipMalloc(&k0, n * 4));
    CK(hipMalloc(&k1, n * 4));
    CK(hipMalloc(&v0, n * 8));
    CK(hipMalloc(&v1, n * 8));
    CK(hipMalloc(&tmp, sort_tmp_bytes(n)));
    const uint32_t mask = bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
    for (int rep = 0; rep < 3; ++rep) {
        fill_random<<<4096, 256>>>(k0, v0, n, mask);
        CK(hipDeviceSynchronize());
        int in0 = 0, passes = 0;
        float ms = 0;
        auto t0 = std::chrono::steady_clock::now();
        if (sort_pairs(k0, v0, k1, v1, n, bits, tmp, &in0, 0, &ms, &passes) != PAG_OK) {
            std::fprintf(stderr, "sort failed: %s\n", last_error());
            return 2;
        }
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("n=%llu bits=%d passes=%d scatter %.3f ms/pass = %.0f GB/s (%.1f %% of 8 TB/s), whole sort %.2f ms\n",
                    (unsigned long long)n, bits, passes, ms, 24.0 * n / ms * 1e-6, 24.0 * n / ms * 1e-6 / 80.0, wall);
        if (check && rep == 0) {
            std::vector<uint32_t> hk(n), rk(n);
            std::vector<uint64_t> hv(n), rv(n);
            CK(hipMemcpy(rk.data(), in0 ? k0 : k1, n * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(rv.data(), in0 ? v0 : v1, n * 8, hipMemcpyDeviceToHost));
            for (uint64_t i = 0; i < n; ++i) {
                uint64_t x = i * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
                x ^= x >> 29;
                x *= 0xBF58476D1CE4E5B9ull;
                x ^= x >> 32;
                hk[i] = (uint32_t)x & mask;
                hv[i] = payload_of(i);
            }
            std::vector<uint64_t> idx(n);
            for (uint64_t i = 0; i < n; ++i) idx[i] = i;
            std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return hk[a] < hk[b]; });
            uint64_t bad = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const bool b = rk[i] != hk[idx[i]] || rv[i] != hv[idx[i]];
                if (b && bad < 8)
                    std::printf("  [%llu] got key %u val %llu, expected key %u val %llu\n", (unsigned long long)i, rk[i],
                                (unsigned long long)rv[i], hk[idx[i]], (unsigned long long)hv[idx[i]]);
                bad += b ? 1 : 0;
            }
            std::printf("check: %llu mismatches\n", (unsigned long long)bad);
            if (bad) return 1;
        }
    }
    return 0;
}
