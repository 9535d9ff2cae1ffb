// walk_round.hpp — the reference's own per-round rules of a traversal (PAlgorithm::travelSequence,
// PAGraph/src/tools/graph/PAlgorithm.cpp:144-426): which of a round's walks is taken, how it is joined to the running path,
// when the contig stops, where the next round's seeds are looked for and in which order they are tried, and what is cut from
// the finished path.  WalkSession (walk_session_*.hpp) calls them between its copies and launches.  No device code, no HIP: plain
// values, vectors and deques in, a small struct out — unit-tested on the CPU (tests/test_walk_round.py, tests/harness/round_test.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <string>
#include <unordered_set>
#include <vector>

#include "pagraph_hip.h"
#include "walk_stitch.hpp"

namespace pagdev::rounds {

// PositionMapper (position/PositionMapper.cpp:16-64) over contig lengths
struct Mapper {
    std::vector<uint64_t> starts, sizes;
    Mapper(const uint32_t *len, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) sizes.push_back(len[i]);
        if (sizes.empty()) return;
        starts.push_back(sizes[0]);
        for (size_t i = 1; i < sizes.size(); ++i) starts.push_back(starts.back() + 3 * sizes[i - 1] + std::max(sizes[i - 1], sizes[i]));
        starts.push_back(starts.back() + 4 * sizes.back());
    }
    uint64_t dualToSingle(int64_t idx, int64_t pos) const {
        if (idx == 0) return 0;
        size_t i = (size_t)(idx > 0 ? idx - 1 : -idx - 1);
        return starts[i] + (idx > 0 ? 0 : 2 * sizes[i]) + (uint64_t)pos;
    }
    std::pair<int64_t, int64_t> singleToDual(uint64_t single) const {
        if (single == 0) return {0, 0};
        auto it = std::upper_bound(starts.begin(), starts.end(), single);
        if (it != starts.begin()) it = std::prev(it);
        int64_t idx = it - starts.begin();
        uint64_t off = single - *it;
        uint64_t sz = (size_t)idx < sizes.size() ? sizes[(size_t)idx] : 0;
        if (off >= 2 * sz) {
            off -= 2 * sz;
            idx = -(idx + 1);
        } else {
            ++idx;
        }
        return {idx, (int64_t)off};
    }
};

inline std::string code2kmer(uint32_t code, uint32_t k) {
    std::string s(k, 'A');
    for (uint32_t i = 0; i < k; ++i) {
        s[k - 1 - i] = "ACGT"[code & 3u];
        code >>= 2;
    }
    return s;
}

// PAlgorithm::editDistance (PAlgorithm.cpp:46-69)
inline size_t edit_distance(const std::string &a, const std::string &b) {
    // (two rows of the table; on the stack for k-mer sized strings: this runs once per re-seed candidate)
    size_t stack_rows[2][40];
    std::vector<size_t> heap_rows;
    size_t *dp[2] = {stack_rows[0], stack_rows[1]};
    if (b.size() + 1 > 40) {
        heap_rows.assign(2 * (b.size() + 1), 0);
        dp[0] = heap_rows.data();
        dp[1] = heap_rows.data() + b.size() + 1;
    }
    size_t flag = 0;
    for (size_t j = 0; j <= b.size(); ++j) dp[flag][j] = j;
    flag ^= 1;
    for (size_t i = 1; i <= a.size(); ++i) {
        for (size_t j = 0; j <= b.size(); ++j) {
            if (j == 0) {
                dp[flag][j] = i;
            } else {
                dp[flag][j] = std::min(dp[flag ^ 1][j] + 1, dp[flag][j - 1] + 1);
                dp[flag][j] = std::min(dp[flag][j], dp[flag ^ 1][j - 1] + (a[i - 1] == b[j - 1] ? 0 : 1));
            }
        }
        flag ^= 1;
    }
    return dp[flag ^ 1][b.size()];
}

// a vertex of a running travel sequence as the per-round control needs it: new id, step, contig coordinate.  The full
// records (k-mer, reference coordinate, abundance) are gathered once, for the finished sequences.
struct LNode {
    uint32_t u;
    int32_t step;
    uint32_t ctg;
    LNode() {}  // (left as it is by vector::resize: a round's path is written over the new elements right away, 14 M of them at configs[1])
    LNode(uint32_t uu, int32_t st, uint32_t c) : u(uu), step(st), ctg(c) {}
};

// ---- the end of a chain: the contig coordinate of its last vertex (0: none), and "the walk ended on another contig, or on the other strand of its own" (PAlgorithm.cpp:251-252)
inline uint32_t end_coord(const stitch::Chain &ch) { return ch.len == 0 ? 0u : ch.parts.back().pc[ch.parts.back().n - 1]; }
inline bool leaves_strand(const Mapper &mapper, uint32_t coord, int64_t chosenOne) { return coord != 0 && mapper.singleToDual(coord).first != chosenOne; }

// ---- the choice among a round's walks (PAlgorithm.cpp:244-265): the first that leaps, else the longest; the walks of later
//      seeds must reach min_len.  chains[sd] is the walk from seeds[sd]; the positions are the chosen seed's offsets.
struct Choice { int chosen = -1; bool leap = false; size_t chooseCtgPos = 0, chooseRefPos = 0; };
inline Choice choose(const std::vector<stitch::Chain> &chains, const std::vector<pag_path_node> &seeds, const Mapper &mapper, const Mapper &refMapper, int64_t chosenOne, uint64_t min_len) {
    Choice P;
    size_t maxLen = 0;
    for (size_t sd = 0; sd < chains.size(); ++sd) {
        const size_t len = chains[sd].size;
        P.leap = leaves_strand(mapper, end_coord(chains[sd]), chosenOne);
        if (!P.leap && sd > 0 && min_len > 0 && len < min_len) continue;
        if (len > maxLen || P.leap) {
            maxLen = len;
            P.chosen = (int)sd;
            P.chooseCtgPos = (size_t)mapper.singleToDual(seeds[sd].ctg).second;
            P.chooseRefPos = (size_t)refMapper.singleToDual(seeds[sd].ref).second;
            if (P.leap) break;
        }
    }
    return P;
}

// ---- appendSeq (PAlgorithm.cpp:110-142) before its copy: the running path loses the vertices at its end without a coordinate or
//      at / beyond the walk's first one (head_ctg); the walk goes to at0, its first step becomes dist (k on an empty path)
struct Trim { int64_t popped; int32_t dist; size_t at0; };  // (popped: the sum of the steps of the vertices taken off)
inline Trim trim_path(std::vector<LNode> &base, uint32_t head_ctg, uint32_t k) {
    int64_t popped = 0;
    while (!base.empty() && (base.back().ctg == 0 || head_ctg <= base.back().ctg)) {
        popped += base.back().step;
        base.pop_back();
    }
    return {popped, base.empty() ? (int32_t)k : (int32_t)(head_ctg - base.back().ctg), base.size()};
}
inline int64_t var_len_gain(const Trim &t, uint64_t walk_size, uint32_t first_step) { return (int64_t)walk_size - t.popped - ((int64_t)first_step - t.dist); }  // (what appendSeq returns)

// ---- the stop rules (PAlgorithm.cpp:280-330): the chosen seeds' offsets of the last four rounds; four within 2 x deviation of each other — on the contig (REPEAT I) or on the reference (REPEAT II) — or a leap end the contig
inline void push_position(std::deque<uint32_t> &q, size_t pos) {
    if (pos != 0) q.push_back((uint32_t)pos);
    while (q.size() > 4) q.pop_front();
}
inline bool repeats(const std::deque<uint32_t> &q, uint64_t deviation) {
    const auto mm = std::minmax_element(q.begin(), q.end());
    return q.size() >= 4 && (uint64_t)(*mm.second - *mm.first) <= 2 * deviation;
}
struct Stop { bool done, finalLeap; };
inline Stop stop_rules(std::deque<uint32_t> &ctgQ, std::deque<uint32_t> &refQ, const Choice &P, uint64_t deviation) {
    push_position(ctgQ, P.chooseCtgPos);
    push_position(refQ, P.chooseRefPos);
    return {repeats(ctgQ, deviation) || repeats(refQ, deviation) || P.leap, P.leap};
}

// ---- the next round's anchor (PAlgorithm.cpp:332-360): the last vertex of the running path on the contig's own strand (its
//      offset there, the vertex — its k-mer orders the next seeds), and the window of offsets the next seeds are looked for in
struct Anchor { uint64_t pos = 0; uint32_t u = 0; bool found = false; };
inline Anchor last_on_strand(const std::vector<LNode> &travel, const Mapper &mapper, int64_t chosenOne) {
    for (auto it = travel.rbegin(); it != travel.rend(); ++it) {
        const auto d = mapper.singleToDual(it->ctg);
        if (it->ctg != 0 && d.first == chosenOne && d.second >= 0) return {(uint64_t)d.second, it->u, true};
    }
    return {};
}
struct Window { uint64_t left, right; };
inline Window seed_window(uint64_t pos, uint64_t deviation) { return {pos - std::min<uint64_t>(pos, 1000 * deviation), pos + 1000 * deviation}; }

// ---- the candidates of one window request, from the words the seed-window kernel wrote for it: `parts` parts of `stride` words, a count and then
//      ids in each, in offset order.  Appended to vids, every id once, where it first occurs (the std::set `unique` of searchPANode2); returns how many.
inline size_t window_candidates(const uint32_t *words, size_t parts, size_t stride, std::vector<uint32_t> &vids) {
    std::unordered_set<uint32_t> seen;
    const size_t before = vids.size();
    for (size_t part = 0; part < parts; ++part) {
        const uint32_t *o = words + part * stride;
        for (uint32_t x = 0; x < o[0]; ++x)
            if (seen.insert(o[1 + x]).second) vids.push_back(o[1 + x]);
    }
    return vids.size() - before;
}

// ---- the order in which the next round tries its seeds (PAlgorithm.cpp:400-406): std::sort with the reference's comparator (edit distance to the parent
//      k-mer; empty without one), unstable, then the first topK.  Precomputed keys give the same comparison outcomes, hence the same permutation.
inline void order_seeds(const pag_path_node *cand, size_t n, const std::string &parent, uint32_t k, size_t topK, std::vector<pag_path_node> &seeds) {
    struct Keyed { size_t d; pag_path_node n; };
    std::vector<Keyed> keyed;
    keyed.reserve(n);
    for (size_t x = 0; x < n; ++x) keyed.push_back({edit_distance(parent, code2kmer(cand[x].code, k)), cand[x]});
    std::sort(keyed.begin(), keyed.end(), [](const Keyed &a, const Keyed &b) { return a.d < b.d; });
    seeds.clear();  // (its room is the last round's: no allocation)
    for (size_t x = 0; x < keyed.size() && x < topK; ++x) seeds.push_back(keyed[x].n);
}

// ---- filterSequence / "Pump it" of a finished contig (PAlgorithm.cpp:27-44, 409-423); ci: the contig's index
inline bool pumped(const Mapper &mapper, uint32_t last_ctg, uint32_t ci, double startSplit) {  // the last vertex of a path that ends in a leap is dropped?
    auto d = mapper.singleToDual(last_ctg);
    uint64_t a = (uint64_t)std::llabs(d.first);
    return a == (uint64_t)ci + 1 || (a >= 1 && a <= mapper.sizes.size() && (double)d.second >= (double)mapper.sizes[a - 1] * (1 - startSplit));
}
inline void filter_travel(std::vector<LNode> &seq, bool finalLeap, const Mapper &mapper, uint32_t ci, double startSplit) {
    const size_t windowSize = 10;
    if (finalLeap) {
        if (!seq.empty() && pumped(mapper, seq.back().ctg, ci, startSplit)) seq.pop_back();
        return;
    }
    if (seq.size() < windowSize) return;
    for (size_t i = seq.size() - seq.size() / 90; i < seq.size() - windowSize + 1; ++i) {
        const uint32_t firstPos = seq[i].ctg, secondPos = seq[std::min(seq.size(), i + windowSize) - 1].ctg;
        if (secondPos != 0 && firstPos != 0 && secondPos < firstPos) {
            seq.resize(i + 1);
            return;
        }
    }
}

}  // namespace pagdev::rounds
