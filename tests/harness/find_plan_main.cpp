// The host half of pag_find_all_batch (csrc/hip/find_plan.hpp: the checks of the sequences' descriptors and the cut into tiles) as
// a program of its own, for the address and undefined-behaviour sanitizers (built and run by tests/test_find_rule.py; host code
// only).  The lengths are those whose tilings tests/test_gpu_find.py searches — 0, 1, 2, 1 023, 1 024, 1 025 and 2 049 offsets —
// and the ends of the range: 0 and 2^32 - 1 bases.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "find_plan.hpp"

using namespace pagdev;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// the plan of `len` in the strands `rev` against the definition: every offset 0 .. len - k in exactly one tile, in order
static void check_cut(const std::vector<uint32_t> &len, const std::vector<uint8_t> &rev, uint32_t k) {
    FindPlan p;
    find_cut(len.data(), rev.empty() ? nullptr : rev.data(), len.size(), k, &p);
    CHECK(p.seq_tile.size() == len.size() + 1 && p.seq_tile[0] == 0 && p.seq_tile.back() == p.tiles.size());
    for (size_t i = 0; i < len.size(); ++i) {
        const uint64_t offsets = len[i] >= k ? (uint64_t)len[i] - k + 1 : 0;
        CHECK(offsets == find_offsets(len[i], k));
        const uint64_t first = p.seq_tile[i], count = p.seq_tile[i + 1] - first;
        CHECK(count == (offsets + FIND_TILE - 1) / FIND_TILE);
        uint64_t covered = 0;
        for (uint64_t t = 0; t < count; ++t) {
            const FindTile &tile = p.tiles[first + t];
            CHECK(tile.seq == i);
            CHECK((tile.at & 1u) == (!rev.empty() && rev[i] ? 1u : 0u));
            CHECK((tile.at & (FIND_TILE - 1u) & ~1u) == 0u);
            const uint64_t at = tile.at & ~(FIND_TILE - 1u);
            CHECK(at == covered && at < offsets);
            covered += offsets - at < FIND_TILE ? offsets - at : FIND_TILE;
            // what the kernel computes from a tile: the offsets from `at` on, in 32 bits
            const uint32_t rest = len[i] - k + 1u - (uint32_t)at;
            CHECK(rest >= 1u && rest == offsets - at);
        }
        CHECK(covered == offsets);
    }
}

int main() {
    int cases = 0;
    for (uint32_t k : {1u, 9u, 12u, 16u}) {
        std::vector<uint32_t> len = {0u, 0xFFFFFFFFu};
        for (uint32_t offsets : {0u, 1u, 2u, 1023u, 1024u, 1025u, 2049u}) len.push_back(offsets + k - 1);
        check_cut(len, {}, k);
        std::vector<uint8_t> rev(len.size());
        for (size_t i = 0; i < rev.size(); ++i) rev[i] = (uint8_t)(i % 3 == 0 ? 0 : i);
        check_cut(len, rev, k);
        std::vector<uint32_t> back(len.rbegin(), len.rend());
        back.push_back(back[2]);
        back.push_back(back[2]);
        check_cut(back, {}, k);
        cases += 3;
    }
    check_cut({}, {}, 9);
    ++cases;

    // the descriptors: starts on 4-byte boundaries, ends inside packed_bytes
    {
        FindPlan p;
        const uint64_t off[] = {0, 4, 260, 264};
        const uint32_t len[] = {9, 1024, 16, 0};
        CHECK(find_check(off, len, 4, 264, &p));
        CHECK(find_check(off, len, 0, 0, &p));
        CHECK(!find_check(off, len, 4, 263, &p) && p.bad == 2);  // (the third sequence ends at byte 264)
        const uint64_t odd[] = {0, 6};
        CHECK(!find_check(odd, len, 2, 1000, &p) && p.bad == 1);
        const uint64_t far[] = {0, 1000};
        CHECK(find_check(far, len + 3, 1, 0, &p));  // (no base: the start itself must lie inside)
        CHECK(!find_check(far + 1, len + 3, 1, 996, &p) && p.bad == 0);
        const uint64_t big[] = {0xFFFFFFFFFFFFFFFCull, 4};
        const uint32_t longest[] = {0xFFFFFFFFu, 0xFFFFFFFFu};
        CHECK(!find_check(big, longest, 1, 0xFFFFFFFFFFFFFFFFull, &p));       // (byte_off + bytes does not wrap)
        CHECK(!find_check(big + 1, longest, 1, 0x40000003ull, &p));            // (2^30 bytes from byte 4 on: one short)
        CHECK(find_check(big + 1, longest, 1, 0x40000004ull, &p));
        cases += 9;
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("%d cases ok\n", cases);
    return 0;
}
