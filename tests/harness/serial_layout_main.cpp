// tests/harness/serial_layout_main.cpp — test-only, a program of its own.
// The offset arithmetic of a serial-rank run (aligngraph2_amd/csrc/hip/serial_layout.hpp) against the layout written out record
// by record: every record of every (range, owner, stream, pass) is given a name, the owner's buffers and the partitioned
// streams are filled the way their definitions say (include/pagraph_hip.h, pag_shard_*), and every stretch the header computes
// must hold exactly its records.  The copy plan of a chunked receive (pag_shard_run) is executed on such names and held
// against the owner's order written down directly.  Meant to be built with -fsanitize=address,undefined and run as it is (tests/test_serial_layout.py).
#include <algorithm>
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
            const pagdev::OwnerLayout L = pagdev::owner_layout(counts.data(), n, o);  // (the square spelling; check_plan uses the general one)
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

// ---- the copy plan of a chunked receive (pag_shard_run): counts[(rank * C + chunk) * W + owner][4]
void expect_plan(bool ok, const char *what, uint32_t W, uint32_t o, uint32_t C) {
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAIL %s: %u ranks, %u chunks, owner %u\n", what, W, C, o);
}

struct Label {
    uint32_t rank, chunk, pass;
    uint64_t i;
    bool operator==(const Label &x) const { return rank == x.rank && chunk == x.chunk && pass == x.pass && i == x.i; }
};

void check_plan(const std::vector<uint64_t> &counts, uint32_t W, uint32_t C) {
    auto cnt = [&](uint32_t rank, uint32_t ch, uint32_t o, uint32_t q) { return counts[(((size_t)rank * C + ch) * W + o) * 4 + q]; };
    for (uint32_t stream = 0; stream < 2; ++stream)
        for (uint32_t o = 0; o < W; ++o) {
            // a chunk's receive array as the exchange fills it: [from rank 0: pass 1, pass 2][from rank 1: ..]
            std::vector<std::vector<Label>> recv(C);
            for (uint32_t ch = 0; ch < C; ++ch)
                for (uint32_t rank = 0; rank < W; ++rank)
                    for (uint32_t pass = 0; pass < 2; ++pass)
                        for (uint64_t i = 0; i < cnt(rank, ch, o, 2 * stream + pass); ++i) recv[ch].push_back(Label{rank, ch, pass, i});
            // the owner's buffer by definition: [pass 1: rank 0 chunk 0, chunk 1, .. rank 1 ..][pass 2: likewise]
            std::vector<Label> want;
            uint64_t want1 = 0;
            for (uint32_t pass = 0; pass < 2; ++pass)
                for (uint32_t rank = 0; rank < W; ++rank)
                    for (uint32_t ch = 0; ch < C; ++ch)
                        for (uint64_t i = 0; i < cnt(rank, ch, o, 2 * stream + pass); ++i) {
                            want.push_back(Label{rank, ch, pass, i});
                            want1 += pass == 0;
                        }
            const pagdev::ReceivePlan P = pagdev::chunked_receive_plan(counts.data(), W, C, o, stream);
            expect_plan(P.n == want.size() && P.n1 == want1, "plan: sizes", W, o, C);
            const pagdev::OwnerLayout L = pagdev::owner_layout(counts.data(), W * C, W, o);
            expect_plan(P.n == (stream ? L.n_e : L.n_t) && P.n1 == (stream ? L.e1 : L.t1), "plan: sizes are owner_layout's", W, o, C);
            // the plan executed on the labels; its stretches tile the sources and the destination exactly once
            std::vector<Label> got(want.size(), Label{~0u, ~0u, ~0u, 0});
            std::vector<int> dst_seen(want.size(), 0);
            std::vector<std::vector<int>> src_seen(C);
            for (uint32_t ch = 0; ch < C; ++ch) src_seen[ch].assign(recv[ch].size(), 0);
            bool inside = true;
            for (const pagdev::ReceivePlan::Copy &cp : P.copies) {
                if (cp.n == 0 || cp.chunk >= C || cp.src + cp.n > recv[cp.chunk].size() || cp.dst + cp.n > got.size()) {
                    inside = false;
                    continue;
                }
                for (uint64_t i = 0; i < cp.n; ++i) {
                    got[(size_t)(cp.dst + i)] = recv[cp.chunk][(size_t)(cp.src + i)];
                    ++dst_seen[(size_t)(cp.dst + i)];
                    ++src_seen[cp.chunk][(size_t)(cp.src + i)];
                }
            }
            expect_plan(inside, "plan: a copy leaves its arrays or is empty", W, o, C);
            expect_plan(got == want, "plan: the owner's order", W, o, C);
            bool once = true;
            for (int x : dst_seen) once = once && x == 1;
            for (const std::vector<int> &v : src_seen)
                for (int x : v) once = once && x == 1;
            expect_plan(once, "plan: every record copied exactly once", W, o, C);
            // the same rule as a serial-rank run's: chunk ch of rank r is range r * C + ch
            for (uint32_t rank = 0; rank < W; ++rank)
                for (uint32_t ch = 0; ch < C; ++ch) {
                    const pagdev::RangeSlots S = pagdev::range_slots(counts.data(), W * C, W, o, pagdev::chunk_range(rank, C, ch));
                    const uint64_t at[2] = {stream ? S.e_at1 : S.t_at1, stream ? S.e_at2 : S.t_at2};
                    for (uint32_t pass = 0; pass < 2; ++pass) {
                        const uint64_t c = cnt(rank, ch, o, 2 * stream + pass);
                        bool ok = at[pass] + c <= want.size();
                        for (uint64_t i = 0; ok && i < c; ++i) ok = want[(size_t)(at[pass] + i)] == Label{rank, ch, pass, i};
                        expect_plan(ok, "plan: range_slots of the chunk", W, o, C);
                    }
                }
        }
}

// per-entry counts around 2^33: only the plan's arithmetic (no record is touched), against sums written out from the definition
void check_plan_arithmetic(const std::vector<uint64_t> &counts, uint32_t W, uint32_t C) {
    auto cnt = [&](uint32_t rank, uint32_t ch, uint32_t o, uint32_t q) { return counts[(((size_t)rank * C + ch) * W + o) * 4 + q]; };
    for (uint32_t stream = 0; stream < 2; ++stream)
        for (uint32_t o = 0; o < W; ++o) {
            const pagdev::ReceivePlan P = pagdev::chunked_receive_plan(counts.data(), W, C, o, stream);
            uint64_t total[2] = {0, 0};
            for (uint32_t rank = 0; rank < W; ++rank)
                for (uint32_t ch = 0; ch < C; ++ch)
                    for (uint32_t pass = 0; pass < 2; ++pass) total[pass] += cnt(rank, ch, o, 2 * stream + pass);
            expect_plan(P.n == total[0] + total[1] && P.n1 == total[0], "big plan: sizes", W, o, C);
            expect_plan(P.n > (1ull << 35) && P.copies.size() == (size_t)2 * W * C, "big plan: beyond 2^35, one copy per (rank, chunk, pass)", W, o, C);
            bool ok = P.copies.size() == (size_t)2 * W * C;
            bool beyond32 = false;
            for (size_t k = 0; ok && k < P.copies.size(); ++k) {  // copy k is (rank, chunk, pass) in that order
                const uint32_t rank = (uint32_t)(k / 2 / C), ch = (uint32_t)(k / 2 % C), pass = (uint32_t)(k % 2);
                uint64_t dst = pass ? total[0] : 0, src = pass ? cnt(rank, ch, o, 2 * stream) : 0;
                for (uint32_t r2 = 0; r2 < W; ++r2)
                    for (uint32_t c2 = 0; c2 < C; ++c2)
                        if (r2 < rank || (r2 == rank && c2 < ch)) dst += cnt(r2, c2, o, 2 * stream + pass);
                for (uint32_t r2 = 0; r2 < rank; ++r2) src += cnt(r2, ch, o, 2 * stream) + cnt(r2, ch, o, 2 * stream + 1);
                const pagdev::ReceivePlan::Copy &cp = P.copies[k];
                ok = cp.chunk == ch && cp.src == src && cp.dst == dst && cp.n == cnt(rank, ch, o, 2 * stream + pass);
                beyond32 = beyond32 || (cp.src >> 32) != 0;
            }
            expect_plan(ok && beyond32, "big plan: offsets", W, o, C);
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
    // the chunked receive: counts from 0..5 with at least a third of them zero.  Draw 0 takes the conditions to the letter — an
    // empty chunk for every rank ("more chunks than a rank has reads"), one rank that sends nothing — which leaves nothing at all
    // where C = 1 or W = 1; the draws after it apply each condition where something is left beside it.
    for (uint32_t W : {1u, 2u, 4u, 8u})
        for (uint32_t C : {1u, 3u, 4u, 64u})
            for (int draw = 0; draw < 3; ++draw) {
                std::vector<uint64_t> c((size_t)W * C * W * 4);
                for (auto &x : c) x = next() % 3 == 0 ? 0 : next() % 6;
                auto zero_chunk = [&](uint32_t rank, uint32_t ch) { std::fill_n(c.begin() + ((size_t)rank * C + ch) * W * 4, (size_t)W * 4, 0); };
                if (draw == 0 || C > 1)
                    for (uint32_t rank = 0; rank < W; ++rank) zero_chunk(rank, (uint32_t)(next() % C));
                if (draw == 0 || W > 1) {
                    const uint32_t silent = (uint32_t)(next() % W);
                    for (uint32_t ch = 0; ch < C; ++ch) zero_chunk(silent, ch);
                }
                size_t zeros = 0;
                for (uint64_t x : c) zeros += x == 0;
                while (zeros * 3 < c.size()) {
                    uint64_t &x = c[(size_t)(next() % c.size())];
                    zeros += x != 0;
                    x = 0;
                }
                check_plan(c, W, C);
                ++cases;
            }
    {
        const uint32_t W = 8, C = 64;
        std::vector<uint64_t> c((size_t)W * C * W * 4);
        for (auto &x : c) x = (1ull << 33) - 1000 + next() % 2000;
        check_plan_arithmetic(c, W, C);
        ++cases;
    }
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
