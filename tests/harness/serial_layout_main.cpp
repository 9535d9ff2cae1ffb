// tests/harness/serial_layout_main.cpp — test-only, a program of its own.
// The offset arithmetic of a serial-rank run (aligngraph2_amd/csrc/hip/serial_layout.hpp) against the layout written out record
// by record: every record of every (range, owner, stream, pass) is given a name, the owner's buffers and the partitioned
// streams are filled the way their definitions say (include/pagraph_hip.h, pag_shard_*), and every stretch the header computes
// must hold exactly its records.  Meant to be built with -fsanitize=address,undefined and run as it is (tests/test_serial_layout.py).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "serial_layout.hpp"

namespace {

struct Name {
    uint32_t r, o, pass;
    uint64_t i;
    bool operator==(const Name &x) const { return r == x.r && o == x.o && pass == x.pass && i == x.i; }
};

int failures = 0;
void expect(bool ok, const char *what, uint32_t n, uint32_t o, uint32_t r) {
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAIL %s: n = %u, owner %u, range %u\n", what, n, o, r);
}

// stream: 0 tuples, 1 edges
void check(const std::vector<uint64_t> &counts, uint32_t n) {
    auto cnt = [&](uint32_t r, uint32_t o, uint32_t q) { return counts[((size_t)r * n + o) * 4 + q]; };
    for (uint32_t stream = 0; stream < 2; ++stream) {
        // the owners' receive buffers by definition: [pass 1 from range 0] .. [pass 1 from range n-1] [pass 2 from range 0] ..
        for (uint32_t o = 0; o < n; ++o) {
            std::vector<Name> buf;
            for (uint32_t pass = 0; pass < 2; ++pass)
                for (uint32_t r = 0; r < n; ++r)
                    for (uint64_t i = 0; i < cnt(r, o, 2 * stream + pass); ++i) buf.push_back(Name{r, o, pass, i});
            const pagdev::OwnerLayout L = pagdev::owner_layout(counts.data(), n, o);
            const uint64_t total = stream ? L.n_e : L.n_t, first = stream ? L.e1 : L.t1;
            expect(total == buf.size(), "owner_layout: size", n, o, 0);
            uint64_t p1 = 0;
            for (const Name &x : buf) p1 += x.pass == 0;
            expect(first == p1, "owner_layout: pass-1 records", n, o, 0);
            for (uint32_t r = 0; r < n; ++r) {
                const pagdev::RangeSlots S = pagdev::range_slots(counts.data(), n, o, r);
                const uint64_t at[2] = {stream ? S.e_at1 : S.t_at1, stream ? S.e_at2 : S.t_at2};
                for (uint32_t pass = 0; pass < 2; ++pass) {
                    const uint64_t c = cnt(r, o, 2 * stream + pass);
                    bool ok = at[pass] + c <= buf.size();
                    for (uint64_t i = 0; ok && i < c; ++i) ok = buf[(size_t)(at[pass] + i)] == Name{r, o, pass, i};
                    expect(ok, "range_slots", n, o, r);
                }
            }
        }
        // a range's partitioned stream by definition: owners ascending, [its pass-1 records][its pass-2 records]
        for (uint32_t r = 0; r < n; ++r) {
            std::vector<Name> part;
            for (uint32_t o = 0; o < n; ++o)
                for (uint32_t pass = 0; pass < 2; ++pass)
                    for (uint64_t i = 0; i < cnt(r, o, 2 * stream + pass); ++i) part.push_back(Name{r, o, pass, i});
            for (uint32_t o = 0; o < n; ++o) {
                const pagdev::RangeSlots S = pagdev::partitioned_slots(counts.data(), n, o, r);
                const uint64_t at[2] = {stream ? S.e_at1 : S.t_at1, stream ? S.e_at2 : S.t_at2};
                for (uint32_t pass = 0; pass < 2; ++pass) {
                    const uint64_t c = cnt(r, o, 2 * stream + pass);
                    bool ok = at[pass] + c <= part.size();
                    for (uint64_t i = 0; ok && i < c; ++i) ok = part[(size_t)(at[pass] + i)] == Name{r, o, pass, i};
                    expect(ok, "partitioned_slots", n, o, r);
                }
            }
        }
    }
}

}  // namespace

int main() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    int cases = 0;
    for (uint32_t n : {2u, 4u, 8u}) {
        const size_t m = (size_t)n * n * 4;
        check(std::vector<uint64_t>(m, 0), n);  // nothing anywhere
        ++cases;
        for (uint32_t r = 0; r < n; ++r) {  // one range holds everything
            std::vector<uint64_t> c(m, 0);
            for (uint32_t o = 0; o < n; ++o)
                for (uint32_t q = 0; q < 4; ++q) c[((size_t)r * n + o) * 4 + q] = 1 + next() % 9;
            check(c, n);
            ++cases;
        }
        for (uint32_t o = 0; o < n; ++o) {  // one owner takes everything
            std::vector<uint64_t> c(m, 0);
            for (uint32_t r = 0; r < n; ++r)
                for (uint32_t q = 0; q < 4; ++q) c[((size_t)r * n + o) * 4 + q] = 1 + next() % 9;
            check(c, n);
            ++cases;
        }
        for (int rep = 0; rep < 20; ++rep) {  // anything, with zeros among it
            std::vector<uint64_t> c(m);
            for (auto &x : c) x = next() % 3 == 0 ? 0 : next() % 12;
            check(c, n);
            ++cases;
        }
    }
    if (failures) {
        std::fprintf(stderr, "serial_layout: %d failures\n", failures);
        return 1;
    }
    std::printf("serial_layout: %d cases ok\n", cases);
    return 0;
}
