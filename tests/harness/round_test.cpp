// tests/harness/round_test.cpp — TEST SUPPORT (never part of the product).
// C wrappers over the per-round rules of a traversal (aligngraph2_amd/csrc/hip/walk_round.hpp) so that
// tests/test_walk_round.py can drive them on constructed values without a GPU.  Built by the host compiler alone: that this
// file compiles is the check that the header needs no HIP.
#include <algorithm>
#include <cstdint>
#include <deque>
#include <string>
#include <vector>

#include "walk_round.hpp"

using namespace pagdev::rounds;
using pagdev::stitch::Chain;

extern "C" {

int pagt_round_leaves(const uint32_t *ctg_len, uint64_t n_ctgs, uint32_t coord, int64_t chosenOne) {
    return leaves_strand(Mapper(ctg_len, n_ctgs), coord, chosenOne) ? 1 : 0;
}

// Chain c of the round: `vertices[c]` vertices (0: an empty chain), the sum of its steps sizes[c], its last vertex at contig
// coordinate ends[c]; walked from the seed at (seed_ctg[c], seed_ref[c]).  out = chosen, leap, chooseCtgPos, chooseRefPos
void pagt_round_choose(const uint32_t *ctg_len, uint64_t n_ctgs, const uint32_t *ref_len, uint64_t n_refs, uint32_t n_chains, const uint64_t *vertices,
                       const uint64_t *sizes, const uint32_t *ends, const uint32_t *seed_ctg, const uint32_t *seed_ref, int64_t chosenOne, uint64_t min_len,
                       int64_t *out) {
    std::vector<Chain> chains(n_chains);
    std::vector<pag_path_node> seeds(n_chains, pag_path_node{});
    for (uint32_t c = 0; c < n_chains; ++c) {
        chains[c].len = (size_t)vertices[c];
        chains[c].size = sizes[c];
        if (vertices[c]) {  // (the last part's last entry is all end_coord reads: a part of one vertex)
            Chain::Part pt{};
            pt.pc = ends + c;
            pt.n = 1;
            pt.start = (size_t)vertices[c] - 1;
            chains[c].parts.push_back(pt);
        }
        seeds[c].ctg = seed_ctg[c];
        seeds[c].ref = seed_ref[c];
    }
    const Choice P = choose(chains, seeds, Mapper(ctg_len, n_ctgs), Mapper(ref_len, n_refs), chosenOne, min_len);
    out[0] = P.chosen, out[1] = P.leap ? 1 : 0, out[2] = (int64_t)P.chooseCtgPos, out[3] = (int64_t)P.chooseRefPos;
    if (P.chosen >= 0) out[4] = end_coord(chains[(size_t)P.chosen]);
}

// the running path (n vertices: steps, coordinates) meets a walk whose first vertex lies at `head`, whose steps add up to
// walk_size and whose first step is first_step.  out = steps popped, dist, at0, the varLen increment
void pagt_round_trim(const int32_t *step, const uint32_t *ctg, uint64_t n, uint32_t head, uint32_t k, uint64_t walk_size, uint32_t first_step, int64_t *out) {
    std::vector<LNode> base;
    for (uint64_t x = 0; x < n; ++x) base.push_back(LNode((uint32_t)x, step[x], ctg[x]));
    const Trim t = trim_path(base, head, k);
    out[0] = t.popped, out[1] = t.dist, out[2] = (int64_t)t.at0, out[3] = var_len_gain(t, walk_size, first_step);
    out[4] = (int64_t)base.size();
    for (size_t x = 0; x < base.size(); ++x)  // (what is left is the path's beginning, untouched)
        if (base[x].u != (uint32_t)x || base[x].step != step[x] || base[x].ctg != ctg[x]) out[4] = -1;
}

// q_ctg / q_ref: the queues before (n_ctg / n_ref entries, oldest first) and after (at most 4).  Returns done | finalLeap << 1
int pagt_round_stop(uint32_t *q_ctg, uint32_t *n_ctg, uint32_t *q_ref, uint32_t *n_ref, uint64_t ctgPos, uint64_t refPos, int leap, uint64_t deviation) {
    std::deque<uint32_t> a(q_ctg, q_ctg + *n_ctg), b(q_ref, q_ref + *n_ref);
    Choice P;
    P.leap = leap != 0;
    P.chooseCtgPos = (size_t)ctgPos;
    P.chooseRefPos = (size_t)refPos;
    const Stop s = stop_rules(a, b, P, deviation);
    std::copy(a.begin(), a.end(), q_ctg);
    std::copy(b.begin(), b.end(), q_ref);
    *n_ctg = (uint32_t)a.size();
    *n_ref = (uint32_t)b.size();
    return (s.done ? 1 : 0) | (s.finalLeap ? 2 : 0);
}

// out = position, vertex, found, window left, window right
void pagt_round_anchor(const uint32_t *ctg_len, uint64_t n_ctgs, const uint32_t *u, const uint32_t *ctg, uint64_t n, int64_t chosenOne, uint64_t deviation,
                       uint64_t *out) {
    std::vector<LNode> travel;
    for (uint64_t x = 0; x < n; ++x) travel.push_back(LNode(u[x], 1, ctg[x]));
    const Anchor a = last_on_strand(travel, Mapper(ctg_len, n_ctgs), chosenOne);
    const Window w = seed_window(a.pos, deviation);
    out[0] = a.pos, out[1] = a.u, out[2] = a.found ? 1 : 0, out[3] = w.left, out[4] = w.right;
}

// the words of n_req requests; vids: all candidates, request after request; cnt: per request.  Returns their number
uint64_t pagt_round_candidates(const uint32_t *words, uint64_t n_req, uint64_t parts, uint64_t stride, uint32_t *vids, uint64_t *cnt) {
    std::vector<uint32_t> v;
    for (uint64_t q = 0; q < n_req; ++q) cnt[q] = window_candidates(words + q * parts * stride, (size_t)parts, (size_t)stride, v);
    std::copy(v.begin(), v.end(), vids);
    return v.size();
}

// candidates x = 0 .. n-1 with k-mer codes[x], in this initial order; parent: the parent's k-mer, null for none.  order: the
// candidates (their numbers) the next round gets.  reference_form: std::sort over the same initial order with the edit
// distance computed inside the comparator on the k-mer strings, as PAlgorithm.cpp:400-406 has it, then the same cut
uint64_t pagt_round_order_seeds(const uint32_t *codes, uint64_t n, const char *parent, uint32_t k, uint64_t topK, int reference_form, uint32_t *order) {
    std::vector<pag_path_node> cand(n, pag_path_node{});
    for (uint64_t x = 0; x < n; ++x) {
        cand[x].code = codes[x];
        cand[x].vid = (uint32_t)x;
    }
    const std::string parentKmer = parent ? std::string(parent) : std::string();
    std::vector<pag_path_node> seeds;
    if (reference_form) {
        std::sort(cand.begin(), cand.end(), [&](const pag_path_node &lhs, const pag_path_node &rhs) {
            return edit_distance(parentKmer, code2kmer(lhs.code, k)) < edit_distance(parentKmer, code2kmer(rhs.code, k));
        });
        cand.resize(std::min<size_t>(cand.size(), (size_t)topK));
        seeds = cand;
    } else {
        seeds.assign(3, pag_path_node{});  // (what the last round left is replaced)
        order_seeds(cand.data(), cand.size(), parentKmer, k, (size_t)topK, seeds);
    }
    for (size_t x = 0; x < seeds.size(); ++x) order[x] = seeds[x].vid;
    return seeds.size();
}

int pagt_round_pumped(const uint32_t *ctg_len, uint64_t n_ctgs, uint32_t last_ctg, uint32_t ci, double startSplit) {
    return pumped(Mapper(ctg_len, n_ctgs), last_ctg, ci, startSplit) ? 1 : 0;
}
// a finished path of n vertices at coordinates ctg[]: how many are left
uint64_t pagt_round_filter(const uint32_t *ctg_len, uint64_t n_ctgs, const uint32_t *ctg, uint64_t n, int finalLeap, uint32_t ci, double startSplit) {
    std::vector<LNode> seq;
    for (uint64_t x = 0; x < n; ++x) seq.push_back(LNode((uint32_t)x, 1, ctg[x]));
    filter_travel(seq, finalLeap != 0, Mapper(ctg_len, n_ctgs), ci, startSplit);
    for (size_t x = 0; x < seq.size(); ++x)
        if (seq[x].u != (uint32_t)x) return ~0ull;
    return seq.size();
}

}  // extern "C"
