// Kernel-level check of K3/K4 (cluster_short/long, edges_short/long) against a sequential restatement of
// KMerAdjNode::cluster / removeDuplicate on segmented streams.  Test infrastructure (GPU only).
//   seg_kernels_test [n_segments] [seed] [wide] [eps] [whole]     random segment lengths (eps: default 10; whole: coordinates drawn
//                                                                 from the whole 32-bit range)
//   seg_kernels_test case <name> <wide> [eps | all]       one constructed case (see build_case); "all" = every eps of EPS_ALL
//   seg_kernels_test describe <name> <wide>               the shape of a case's segments, from the sequential scan (no device)
//   seg_kernels_test list                                 the names of the constructed cases
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../aligngraph2_amd/csrc/hip/k34_segments.hip"

namespace pagdev {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
const char *last_error() { return ""; }
}  // namespace pagdev

static bool csim(uint32_t a, uint32_t b, uint32_t eps) {
    if (a == 0 || b == 0) return a == 0 && b == 0;
    uint32_t d = a > b ? a - b : b - a;
    return d <= eps;
}
static bool psim(uint64_t x, uint64_t y, uint32_t eps) {
    return csim((uint32_t)(x >> 32), (uint32_t)(y >> 32), eps) && csim((uint32_t)x, (uint32_t)y, eps);
}
#define CK(e)                                                                   \
    do {                                                                        \
        hipError_t r__ = (e);                                                   \
        if (r__ != hipSuccess) {                                                \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r__));            \
            return -1;                                                          \
        }                                                                       \
    } while (0)

// A segmented stream: key = k-mer code (equal inside a segment, rising from one to the next), val = the tuple stream's payload
// (ctg << 32 | ref), eval = the edge stream's (to << 32 | step << 1 | pass).  Both streams share the segmentation here.
struct Stream {
    std::vector<uint32_t> key;
    std::vector<uint64_t> val, eval;
    uint32_t code = 0;
    void begin() { code += 1 + code % 3; }
    void add(uint64_t v, uint64_t e) {
        key.push_back(code);
        val.push_back(v);
        eval.push_back(e);
    }
    // `count` one-record segments: the neighbours of a constructed segment, each with a value of its own that must come back
    // unchanged (count 1, seg_len 1)
    void pad(uint64_t count) {
        for (uint64_t x = 0; x < count; ++x) {
            begin();
            const uint64_t id = key.size();
            add((uint64_t)(0x5E000000u + (uint32_t)id) << 32 | (0x7A000000u + (uint32_t)id), (0xED000000ull + id) << 32 | (id & 7u));
        }
    }
};

static constexpr uint64_t GUARD = 64;  // sentinel elements in front of and behind every array the kernels write

// one stream through launch_cluster (do_cluster) and / or launch_edges (do_edges), every slot compared with the sequential
// expectation; returns the number of mismatches (reported up to a limit), -1 on a runtime error
static int check_stream(const char *label, const Stream &st, uint32_t eps, bool wide, bool do_cluster, bool do_edges) {
    const std::vector<uint32_t> &key = st.key;
    const std::vector<uint64_t> &val = st.val, &eval = st.eval;
    const uint64_t n = key.size();
    // ---- sequential expectation
    std::vector<uint32_t> xlen(n, 0), xelen(n, 0);
    std::vector<uint64_t> xval(n, 0), xeval(n, 0);
    std::vector<uint16_t> xcnt(n, 0);
    uint64_t x_ctg = 0, x_all = 0, x_seg = 0, x_grp = 0, x_grp1 = 0;
    for (uint64_t i = 0; i < n;) {
        uint64_t j = i;
        while (j < n && key[j] == key[i]) ++j;
        if (do_cluster) {
            std::vector<std::pair<uint64_t, uint16_t>> lead;
            for (uint64_t t = i; t < j; ++t) {
                bool hit = false;
                for (auto &l : lead)
                    if (psim(val[t], l.first, eps)) {
                        l.second = (uint16_t)(l.second + 1);
                        hit = true;
                        break;
                    }
                if (!hit) lead.push_back({val[t], 1});
            }
            std::sort(lead.begin(), lead.end());
            xlen[i] = (uint32_t)lead.size();
            for (size_t l = 1; l < lead.size(); ++l) xlen[i + l] = pagdev::SEG_LEADER | (uint32_t)l;  // (the other leader slots are marked)
            for (size_t l = 0; l < lead.size(); ++l) {
                xval[i + l] = lead[l].first;
                xcnt[i + l] = lead[l].second;
                x_ctg += (lead[l].first >> 32) != 0;
            }
            x_all += lead.size();
        }
        x_seg += 1;
        if (do_edges) {
            std::vector<uint64_t> e(eval.begin() + i, eval.begin() + j);
            std::stable_sort(e.begin(), e.end());
            uint32_t p = 0;
            for (size_t a = 0; a < e.size(); ++a)
                if (a == 0 || (e[a] >> 1) != (e[a - 1] >> 1)) {
                    xeval[i + p++] = e[a];
                    x_grp1 += (e[a] & 1) == 0;
                }
            xelen[i] = p;
            x_grp += p;
        }
        i = j;
    }
    // ---- device: every written array lies between two rows of GUARD sentinel elements
    uint32_t *d_key, *d_seg, *d_lc;
    uint64_t *d_val, *d_scr, *d_ll, *d_ctr;
    uint16_t *d_cnt;
    const uint64_t ng = n + 2 * GUARD;
    CK(hipMalloc(&d_key, n * 4));
    CK(hipMalloc(&d_seg, ng * 4));
    CK(hipMalloc(&d_val, ng * 8));
    CK(hipMalloc(&d_scr, n * 12 + 64));
    CK(hipMalloc(&d_ll, n * 8));
    CK(hipMalloc(&d_cnt, ng * 2));
    CK(hipMalloc(&d_lc, 4));
    CK(hipMalloc(&d_ctr, 32));
    CK(hipMemcpy(d_key, key.data(), n * 4, hipMemcpyHostToDevice));
    int bad = 0;
    std::vector<uint32_t> seg(ng);
    std::vector<uint64_t> v(ng), ctr(4);
    std::vector<uint16_t> c(ng);
    auto guards_ok = [&](const char *what) {
        for (uint64_t g = 0; g < GUARD; ++g)
            for (uint64_t at : {g, GUARD + n + g})
                if (seg[at] != 0xEEEEEEEEu || v[at] != 0xEEEEEEEEEEEEEEEEull || c[at] != 0xEEEEu) {
                    printf("%s %s: a word %s the arrays was written (guard %llu)\n", label, what, at < GUARD ? "in front of" : "behind", (unsigned long long)g);
                    return false;
                }
        return true;
    };
    if (do_cluster) {
        CK(hipMemset(d_val, 0xEE, ng * 8));
        CK(hipMemset(d_cnt, 0xEE, ng * 2));
        CK(hipMemset(d_seg, 0xEE, ng * 4));
        CK(hipMemcpy(d_val + GUARD, val.data(), n * 8, hipMemcpyHostToDevice));
        pagdev::ClusterOut co{d_seg + GUARD, d_cnt + GUARD, d_ctr};
        if (pagdev::launch_cluster(d_key, d_val + GUARD, d_scr, n, eps, co, d_ll, d_lc, 0, wide) != 0) return -1;
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(seg.data(), d_seg, ng * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(v.data(), d_val, ng * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(c.data(), d_cnt, ng * 2, hipMemcpyDeviceToHost));
        CK(hipMemcpy(ctr.data(), d_ctr, 32, hipMemcpyDeviceToHost));
        const uint32_t *sg = seg.data() + GUARD;
        const uint64_t *vv = v.data() + GUARD;
        const uint16_t *cc = c.data() + GUARD;
        int shown = 0;
        for (uint64_t i = 0; i < n && shown < 10; ++i) {
            if (sg[i] != xlen[i]) {
                printf("%s cluster seg_len[%llu] = %u want %u\n", label, (unsigned long long)i, sg[i], xlen[i]);
                ++bad, ++shown;
                continue;
            }
            for (uint32_t l = 0; !(xlen[i] & pagdev::SEG_LEADER) && l < xlen[i]; ++l)
                if (vv[i + l] != xval[i + l] || cc[i + l] != xcnt[i + l]) {
                    printf("%s cluster seg %llu slot %u: (%llx,%u) want (%llx,%u)\n", label, (unsigned long long)i, l,
                           (unsigned long long)vv[i + l], cc[i + l], (unsigned long long)xval[i + l], xcnt[i + l]);
                    ++bad, ++shown;
                    break;
                }
        }
        if (ctr[0] != x_ctg || ctr[1] != x_all || ctr[2] != x_seg) {
            printf("%s cluster counters %llu %llu %llu want %llu %llu %llu\n", label, (unsigned long long)ctr[0],
                   (unsigned long long)ctr[1], (unsigned long long)ctr[2], (unsigned long long)x_ctg,
                   (unsigned long long)x_all, (unsigned long long)x_seg);
            ++bad;
        }
        if (!guards_ok("cluster")) ++bad;
    }
    if (do_edges) {
        CK(hipMemset(d_val, 0xEE, ng * 8));
        CK(hipMemset(d_cnt, 0xEE, ng * 2));
        CK(hipMemset(d_seg, 0xEE, ng * 4));
        CK(hipMemcpy(d_val + GUARD, eval.data(), n * 8, hipMemcpyHostToDevice));
        pagdev::EdgeOut eo{d_seg + GUARD, d_ctr};
        if (pagdev::launch_edges(d_key, d_val + GUARD, d_scr, n, eo, d_ll, d_lc, 0, wide) != 0) return -1;
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(seg.data(), d_seg, ng * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(v.data(), d_val, ng * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(c.data(), d_cnt, ng * 2, hipMemcpyDeviceToHost));
        CK(hipMemcpy(ctr.data(), d_ctr, 32, hipMemcpyDeviceToHost));
        const uint32_t *sg = seg.data() + GUARD;
        const uint64_t *vv = v.data() + GUARD;
        int shown = 0;
        for (uint64_t i = 0; i < n && shown < 10; ++i) {
            if (sg[i] != xelen[i]) {
                printf("%s edges seg_len[%llu] = %u want %u\n", label, (unsigned long long)i, sg[i], xelen[i]);
                ++bad, ++shown;
                continue;
            }
            for (uint32_t l = 0; l < xelen[i]; ++l)
                if (vv[i + l] != xeval[i + l]) {
                    printf("%s edges seg %llu slot %u: %llx want %llx\n", label, (unsigned long long)i, l,
                           (unsigned long long)vv[i + l], (unsigned long long)xeval[i + l]);
                    ++bad, ++shown;
                    break;
                }
        }
        if (ctr[0] != x_grp || ctr[1] != x_grp1) {
            printf("%s edges counters %llu %llu want %llu %llu\n", label, (unsigned long long)ctr[0], (unsigned long long)ctr[1],
                   (unsigned long long)x_grp, (unsigned long long)x_grp1);
            ++bad;
        }
        if (!guards_ok("edges")) ++bad;
    }
    CK(hipFree(d_key));
    CK(hipFree(d_seg));
    CK(hipFree(d_val));
    CK(hipFree(d_scr));
    CK(hipFree(d_ll));
    CK(hipFree(d_cnt));
    CK(hipFree(d_lc));
    CK(hipFree(d_ctr));
    return bad;
}

// ---------------------------------------------------------------------------------------- random segment lengths
// whole: the centres of a segment's positions are drawn from the whole 32-bit range instead of a few thousand coordinates (every
// eighth segment around 2^31, its jitter across the top bit), and the spread segments' positions likewise
static void random_stream(Stream &st, uint64_t n_seg_target, unsigned seed, bool whole = false) {
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> &key = st.key;
    std::vector<uint64_t> &val = st.val, &eval = st.eval;
    uint32_t code = 0;
    for (uint64_t sgi = 0; sgi < n_seg_target; ++sgi) {
        code += 1 + (uint32_t)(rng() % 3);
        uint32_t r = (uint32_t)(rng() % 100);
        // (the short path takes segments of up to 64 records, the long path keeps up to 512 leaders / 1 024 edges on chip: lengths on
        // both sides of each limit; "spread": positions far apart, so that nearly every item becomes a leader)
        const bool spread = r >= 98;
        uint32_t len = r < 60 ? 1 + (uint32_t)(rng() % 8) : r < 85 ? 1 + (uint32_t)(rng() % 33) : r < 92 ? 30 + (uint32_t)(rng() % 200) : r < 96 ? 60 + (uint32_t)(rng() % 10)
                       : r < 98 ? 400 + (uint32_t)(rng() % 900) : 300 + (uint32_t)(rng() % 1200);
        uint32_t centers = 1 + (uint32_t)(rng() % 4);
        uint32_t c0[4], r0[4];
        for (int c = 0; c < 4; ++c) {
            c0[c] = 1000 + (uint32_t)(rng() % 300);
            r0[c] = 5000 + (uint32_t)(rng() % 300);
        }
        // (every 40th segment at the ends of the coordinate space: coordinates of 1 .. eps next to "no coordinate" (0), and coordinates
        // within 2 eps of 2^32, which cluster_short's two-subtraction form of the similarity test must leave to the plain predicate)
        if (sgi % 40 == 7)
            for (int c = 0; c < 4; ++c) {
                const bool top = rng() % 2 == 0;
                c0[c] = top ? 0xFFFFFFFFu - 14u - (uint32_t)(rng() % 30) : 1u + (uint32_t)(rng() % 12);
                r0[c] = rng() % 2 ? 0xFFFFFFFFu - 14u - (uint32_t)(rng() % 30) : 1u + (uint32_t)(rng() % 12);
            }
        if (whole && sgi % 40 != 7)
            for (int c = 0; c < 4; ++c) {
                const bool at_top_bit = sgi % 8 == 3;
                c0[c] = at_top_bit ? 0x80000000u - 7u - (uint32_t)(rng() % 8) : 1u + (uint32_t)(rng() % 0xFFFFFFF0ull);
                r0[c] = at_top_bit ? 0x80000000u - 7u - (uint32_t)(rng() % 8) : 1u + (uint32_t)(rng() % 0xFFFFFFF0ull);
            }
        for (uint32_t j = 0; j < len; ++j) {
            uint32_t c = (uint32_t)(rng() % centers);
            bool pass2 = j >= len / 2;
            uint32_t ctg = pass2 ? 0 : c0[c] + (uint32_t)(rng() % 15);
            uint32_t ref = (rng() % 5 == 0) ? 0 : r0[c] + (uint32_t)(rng() % 15);
            if (spread) {
                ctg = pass2 ? 0 : 1000 + (uint32_t)(rng() % 40000);
                ref = 5000 + (uint32_t)(rng() % 40000);
                if (whole) {
                    ctg = pass2 ? 0 : 1u + (uint32_t)(rng() % 0xFFFFFFFEull);
                    ref = 1u + (uint32_t)(rng() % 0xFFFFFFFEull);
                }
            }
            key.push_back(code);
            val.push_back((uint64_t)ctg << 32 | ref);
            uint32_t to = (uint32_t)(rng() % (spread ? 400 : 6)), step = (uint32_t)(rng() % 4);
            eval.push_back((uint64_t)to << 32 | step << 1 | (pass2 ? 1 : 0));
        }
    }
}

// ---------------------------------------------------------------------------------------- constructed cases
// A segment of `len` records around a few centres thousands apart (jitter 15, one ref coordinate in five missing, the second half pass 2:
// ctg == 0): several leaders at a small eps, members that join them, everything in one or two clusters at a large eps
static void clustered_segment(Stream &st, std::mt19937_64 &rng, uint64_t len) {
    st.begin();
    uint32_t c0[4], r0[4];
    for (int c = 0; c < 4; ++c) {
        c0[c] = 1000 + 4000 * (uint32_t)c + (uint32_t)(rng() % 300);
        r0[c] = 50000 + 4000 * (uint32_t)c + (uint32_t)(rng() % 300);
    }
    for (uint64_t j = 0; j < len; ++j) {
        const uint32_t c = (uint32_t)(rng() % 4);
        const bool pass2 = j >= (len + 1) / 2;
        const uint32_t ctg = pass2 ? 0 : c0[c] + (uint32_t)(rng() % 15);
        const uint32_t ref = (rng() % 5 == 0) ? 0 : r0[c] + (uint32_t)(rng() % 15);
        const uint32_t to = (uint32_t)(rng() % 6), step = (uint32_t)(rng() % 4);
        st.add((uint64_t)ctg << 32 | ref, (uint64_t)to << 32 | step << 1 | (pass2 ? 1 : 0));
    }
}

struct Sub {
    std::string label;
    Stream st;
    bool cluster = true, edges = true;  // the kernels the stream goes through
};

// Leader l of a constructed long segment: coordinates 3 eps + 7 apart, so that a member within eps of its own leader is similar to no
// other.  pass 1: both coordinates step; pass 2: ctg == 0 (joined through the "both zero" rule), ref steps.  The coordinates
// run DOWN with l, so the sorted order of the leaders is the reverse of their insertion order.
struct LeaderGrid {
    uint32_t eps, n_leaders;
    bool pass2;
    uint64_t pitch() const { return 3ull * eps + 7; }
    uint64_t leader(uint32_t l) const {
        const uint64_t ref = 900000ull + (uint64_t)(n_leaders - l) * pitch();
        const uint64_t ctg = pass2 ? 0ull : 100000ull + (uint64_t)(n_leaders - l) * pitch();
        return ctg << 32 | ref;
    }
    uint64_t member(uint32_t l, std::mt19937_64 &rng) const {
        const uint64_t v = leader(l);
        const uint32_t w = 2u * eps + 1u;
        const uint32_t ref = (uint32_t)v - eps + (uint32_t)(rng() % w);
        const uint32_t ctg = pass2 ? 0u : (uint32_t)(v >> 32) - eps + (uint32_t)(rng() % w);
        return (uint64_t)ctg << 32 | ref;
    }
};
static uint64_t some_edge(std::mt19937_64 &rng, bool pass2) { return (uint64_t)(rng() % 50) << 32 | (uint32_t)(rng() % 4) << 1 | (pass2 ? 1 : 0); }

// a segment with exactly `n_leaders` leaders, `members` members mixed in behind the leaders they join; last_is_leader: the last leader
// is held back and comes as the very last item of the segment
static void leader_segment(Stream &st, std::mt19937_64 &rng, uint32_t eps, uint32_t n_leaders, uint64_t members, bool pass2, bool last_is_leader) {
    const LeaderGrid G{eps, n_leaders, pass2};
    st.begin();
    const uint32_t early = last_is_leader ? n_leaders - 1 : n_leaders;
    uint64_t left = members;
    for (uint32_t l = 0; l < early; ++l) {
        st.add(G.leader(l), some_edge(rng, pass2));
        uint64_t now = l + 1 == early ? left : std::min<uint64_t>(left, rng() % (2 * members / early + 2));
        left -= now;
        for (; now; --now) st.add(G.member((uint32_t)(rng() % (l + 1)), rng), some_edge(rng, pass2));
    }
    if (last_is_leader) st.add(G.leader(n_leaders - 1), some_edge(rng, pass2));
}

// Items similar to TWO leaders: leader a and leader b are replaced by a pair 2 eps - 1 apart in ref, the items lie between them, eps
// from the one and eps - 1 from the other.  `swap`: the pair's coordinates change places.  The reference's scan joins the item to the
// leader inserted FIRST (the lower index), whichever is nearer or lower.
static void first_wins_segment(Stream &st, std::mt19937_64 &rng, uint32_t eps, uint32_t n_leaders, bool swap) {
    const LeaderGrid G{eps, n_leaders, false};
    const uint32_t pairs[3][2] = {{70, 130}, {71, 100}, {5, 69}};  // (another row of 64 leaders; the same row; lanes 5 of rows 0 and 1)
    std::vector<uint64_t> lv(n_leaders);
    for (uint32_t l = 0; l < n_leaders; ++l) lv[l] = G.leader(l);
    std::vector<uint64_t> both;
    for (auto &pr : pairs) {
        const uint64_t lo = G.leader(pr[0]);                 // (a grid point; the grid point of pr[1] stays empty)
        const uint64_t hi = lo + 2ull * eps - 1;             // (ref + 2 eps - 1: more than eps from lo, less than the pitch)
        lv[pr[0]] = swap ? hi : lo;
        lv[pr[1]] = swap ? lo : hi;
        both.push_back(lo + eps);      // eps from lo, eps - 1 from hi
        both.push_back(lo + eps - 1);  // eps - 1 from lo, eps from hi
    }
    st.begin();
    for (uint32_t l = 0; l < n_leaders; ++l) st.add(lv[l], some_edge(rng, false));
    for (int rep = 0; rep < 5; ++rep)
        for (uint64_t b : both) {
            st.add(b, some_edge(rng, false));
            st.add(G.member(256u + (uint32_t)(rng() % (n_leaders - 256u)), rng), some_edge(rng, false));  // (a member of an untouched leader)
        }
}

// a segment of `len` edge records over `n_to` x `n_step` distinct (to, step), the first half of pass 1 and the second of pass 2 — so most
// groups hold both passes, and duplicates of each
static void edge_segment(Stream &st, std::mt19937_64 &rng, uint64_t len, uint32_t n_to, uint32_t n_step) {
    st.begin();
    for (uint64_t j = 0; j < len; ++j) {
        const bool pass2 = j >= len / 2;
        const uint32_t to = 7u + 3u * (uint32_t)(rng() % n_to), step = (uint32_t)(rng() % n_step);
        st.add((uint64_t)(1000 + (uint32_t)(rng() % 40)) << 32 | (2000 + (uint32_t)(rng() % 40)), (uint64_t)to << 32 | step << 1 | (pass2 ? 1 : 0));
    }
}

static const uint64_t WRAP_SIZES[4] = {65535, 65536, 65537, 131073};  // items of a cluster, leader included: counts 65535, 0, 1, 1

// four segments, one per cluster size: `n_leaders` leaders first, then the members of leader `at` with a few members of other leaders
// among them
static void wrap_segments(Stream &st, std::mt19937_64 &rng, uint32_t eps, uint32_t n_leaders, uint32_t at, bool pass2) {
    for (uint64_t size : WRAP_SIZES) {
        st.pad(3);
        const LeaderGrid G{eps, n_leaders, pass2};
        st.begin();
        for (uint32_t l = 0; l < n_leaders; ++l) st.add(G.leader(l), some_edge(rng, pass2));
        for (uint64_t m = 1; m < size; ++m) {
            st.add(G.member(at, rng), some_edge(rng, pass2));
            if (m % 4096 == 0) {
                uint32_t other = (uint32_t)(rng() % n_leaders);
                if (other == at) other = (other + 1) % n_leaders;
                st.add(G.member(other, rng), some_edge(rng, pass2));
            }
        }
    }
    st.pad(3);
}

static const char *CASE_NAMES[] = {
    "short_at_stream_start", "short_at_last_owned", "short_at_next_tile", "short_end_n1", "short_end_nOWN", "short_end_nOWN1", "short_end_n512",
    "short_end_n513", "short_whole_stream_200000",
    "leaders_511", "leaders_512", "leaders_513", "leaders_513th_is_last_item", "leaders_1500", "first_leader_wins_on_chip",
    "first_leader_wins_on_chip_swapped", "first_leader_wins_in_place", "first_leader_wins_in_place_swapped",
    "edges_1023", "edges_1024", "edges_1025", "edges_100000_of_64_groups",
    "wrap_on_chip_pass1", "wrap_on_chip_pass2", "wrap_in_place_leader0_pass1", "wrap_in_place_leader0_pass2", "wrap_in_place_leader600_pass1",
    "wrap_in_place_leader600_pass2",
};

// the streams of one case; false: no such case.  `short_path`: the case is about cluster_short's masks, so it runs at every eps
static bool build_case(const std::string &name, bool wide, uint32_t eps, std::vector<Sub> &out, bool &short_path) {
    const uint64_t OWN = wide ? pagdev::ShortW<64>::OWN : pagdev::ShortW<32>::OWN;
    const uint32_t LENS[6] = {31, 32, 33, 63, 64, 65};
    std::mt19937_64 rng(std::hash<std::string>{}(name) % 1000003u);
    short_path = name.compare(0, 6, "short_") == 0;
    auto placed = [&](uint64_t head) {  // a segment of each length with its head at record `head`, one-record segments around it
        for (uint32_t len : LENS) {
            out.push_back({"len" + std::to_string(len), Stream()});
            Stream &st = out.back().st;
            st.pad(head);
            clustered_segment(st, rng, len);
            st.pad(40);
        }
    };
    auto at_end = [&](uint64_t n) {  // the segment ends with the stream, at record n
        for (uint32_t len : LENS) {
            if (len > n && len != 31) continue;
            const uint64_t l = std::min<uint64_t>(len, n);
            out.push_back({"len" + std::to_string(l), Stream()});
            Stream &st = out.back().st;
            st.pad(n - l);
            clustered_segment(st, rng, l);
        }
    };
    auto one = [&]() -> Stream & {
        out.push_back({"", Stream()});
        out.back().st.pad(5);
        return out.back().st;
    };
    if (name == "short_at_stream_start") placed(0);
    else if (name == "short_at_last_owned") placed(OWN - 1);  // (the whole body lies in the tile's look-ahead halo)
    else if (name == "short_at_next_tile") placed(OWN);
    else if (name == "short_end_n1") at_end(1);
    else if (name == "short_end_nOWN") at_end(OWN);
    else if (name == "short_end_nOWN1") at_end(OWN + 1);
    else if (name == "short_end_n512") at_end(512);
    else if (name == "short_end_n513") at_end(513);
    else if (name == "short_whole_stream_200000") {
        // (edges_long's rank sort through memory is quadratic in the segment, on one wavefront: 200 000 records took it 50 s on an
        // MI355X, 100 000 take 13 s — so K4 gets a whole stream of its own, of 100 000 records)
        out.push_back({"cluster", Stream(), true, false});
        clustered_segment(out.back().st, rng, 200000);
        out.push_back({"edges_100000", Stream(), false, true});
        clustered_segment(out.back().st, rng, 100000);
    } else if (name == "leaders_511" || name == "leaders_512" || name == "leaders_513" || name == "leaders_1500") {
        const uint32_t nl = (uint32_t)atoi(name.c_str() + 8);
        Stream &st = one();
        leader_segment(st, rng, eps, nl, 3000, false, false);
        st.pad(5);
        leader_segment(st, rng, eps, nl, 3000, true, false);
        st.pad(5);
    } else if (name == "leaders_513th_is_last_item") {
        Stream &st = one();
        leader_segment(st, rng, eps, 513, 3000, false, true);
        st.pad(5);
        leader_segment(st, rng, eps, 513, 3000, true, true);
        st.pad(5);
    } else if (name.compare(0, 17, "first_leader_wins") == 0) {
        Stream &st = one();
        first_wins_segment(st, rng, eps, name.find("in_place") != std::string::npos ? 700 : 300, name.find("swapped") != std::string::npos);
        st.pad(5);
    } else if (name == "edges_1023" || name == "edges_1024" || name == "edges_1025") {
        Stream &st = one();
        edge_segment(st, rng, (uint64_t)atoi(name.c_str() + 6), 30, 8);
        st.pad(5);
    } else if (name == "edges_100000_of_64_groups") {
        Stream &st = one();
        edge_segment(st, rng, 100000, 8, 8);
        st.pad(5);
    } else if (name.compare(0, 5, "wrap_") == 0) {
        const bool pass2 = name.find("pass2") != std::string::npos;
        out.push_back({"", Stream(), true, false});  // (K3 only: K4 would spend 20 s sorting the edge records that pad these segments)
        if (name.find("on_chip") != std::string::npos) wrap_segments(out.back().st, rng, eps, 40, 17, pass2);
        else wrap_segments(out.back().st, rng, eps, 700, name.find("leader600") != std::string::npos ? 600 : 0, pass2);
    } else
        return false;
    return true;
}

// seg_kernels_test describe <name> <wide>: what the case's streams hold, per segment of more than one record, from the sequential scan
// alone (no device): records, leaders, items of the largest cluster, distinct (to, step).  The test asserts from this that a case
// has the shape it is named for.
static int describe_mode(const std::string &name, bool wide) {
    std::vector<Sub> subs;
    bool short_path;
    if (!build_case(name, wide, 10, subs, short_path)) return 2;
    const uint64_t OWN = wide ? pagdev::ShortW<64>::OWN : pagdev::ShortW<32>::OWN;
    for (auto &s : subs) {
        const Stream &st = s.st;
        const uint64_t n = st.key.size();
        printf("stream %s n=%llu\n", s.label.c_str(), (unsigned long long)n);
        for (uint64_t i = 0; i < n;) {
            uint64_t j = i;
            while (j < n && st.key[j] == st.key[i]) ++j;
            if (j - i > 1 || n == 1) {
                std::vector<std::pair<uint64_t, uint64_t>> lead;
                for (uint64_t t = i; t < j; ++t) {
                    bool hit = false;
                    for (auto &l : lead)
                        if (psim(st.val[t], l.first, 10)) {
                            l.second += 1;
                            hit = true;
                            break;
                        }
                    if (!hit) lead.push_back({st.val[t], 1});
                }
                uint64_t biggest = 0;
                for (auto &l : lead) biggest = std::max(biggest, l.second);
                std::vector<uint64_t> e(st.eval.begin() + i, st.eval.begin() + j);
                for (auto &x : e) x >>= 1;
                std::sort(e.begin(), e.end());
                const uint64_t groups = std::unique(e.begin(), e.end()) - e.begin();
                printf("segment head=%llu tile_offset=%llu records=%llu ends_at_n=%d leaders=%llu last_item_is_leader=%d biggest_cluster=%llu edge_groups=%llu\n",
                       (unsigned long long)i, (unsigned long long)(i % OWN), (unsigned long long)(j - i), (int)(j == n), (unsigned long long)lead.size(),
                       (int)(lead.back().first == st.val[j - 1] && lead.back().second == 1), (unsigned long long)biggest, (unsigned long long)groups);
            }
            i = j;
        }
    }
    return 0;
}

static const uint32_t EPS_ALL[6] = {0u, 1u, 10u, 3000u, 1u << 30, (1u << 31) + 5u};

static int case_mode(const std::string &name, bool wide, const char *eps_arg) {
    std::vector<uint32_t> epss;
    bool short_path = false;
    {
        std::vector<Sub> probe;
        if (!build_case(name, wide, 10, probe, short_path)) {
            fprintf(stderr, "no case '%s' (seg_kernels_test list)\n", name.c_str());
            return 2;
        }
    }
    if (eps_arg && strcmp(eps_arg, "all") == 0) {
        if (short_path) epss.assign(EPS_ALL, EPS_ALL + 6);
        else epss.push_back(10);  // (the long-path cases place their coordinates by eps: one eps is every eps)
    } else
        epss.push_back(eps_arg ? (uint32_t)strtoul(eps_arg, nullptr, 10) : 10u);
    int bad = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t e = 0; e < epss.size(); ++e) {
        std::vector<Sub> subs;
        build_case(name, wide, epss[e], subs, short_path);
        for (auto &s : subs) {
            char label[160];
            snprintf(label, sizeof label, "%s%s%s wide=%d eps=%u:", name.c_str(), s.label.empty() ? "" : "/", s.label.c_str(), (int)wide, epss[e]);
            // (K4 does not look at eps: the edge stream of a case goes through once)
            const bool edges = s.edges && e == 0;
            if (!s.cluster && !edges) continue;
            const int r = check_stream(label, s.st, epss[e], wide, s.cluster, edges);
            if (r < 0) return 2;
            bad += r;
        }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%s: case %s wide=%d, %.2f s\n", bad ? "FAIL" : "OK", name.c_str(), (int)wide, sec);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "list") == 0) {
        for (const char *nm : CASE_NAMES) puts(nm);
        return 0;
    }
    if (argc > 3 && strcmp(argv[1], "describe") == 0) return describe_mode(argv[2], atoi(argv[3]) != 0);
    if (argc > 1 && strcmp(argv[1], "case") == 0) {
        if (argc < 4) {
            fprintf(stderr, "usage: seg_kernels_test case <name> <wide> [eps | all]\n");
            return 2;
        }
        return case_mode(argv[2], atoi(argv[3]) != 0, argc > 4 ? argv[4] : nullptr);
    }
    const uint64_t n_seg_target = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
    const unsigned seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1;
    const bool wide = argc > 3 ? atoi(argv[3]) != 0 : false;  // (the short path with 64-record masks instead of 32)
    const uint32_t eps = argc > 4 ? (uint32_t)strtoul(argv[4], nullptr, 10) : 10u;
    const bool whole = argc > 5 && strcmp(argv[5], "whole") == 0;
    Stream st;
    random_stream(st, n_seg_target, seed, whole);
    const int bad = check_stream("random", st, eps, wide, true, true);
    if (bad < 0) return 2;
    uint64_t n_seg = 0, n_top = 0, n_pos = 0;
    for (size_t i = 0; i < st.key.size(); ++i) {
        n_seg += i == 0 || st.key[i] != st.key[i - 1];
        const uint32_t c = (uint32_t)(st.val[i] >> 32), r = (uint32_t)st.val[i];
        n_top += (c >> 31) + (r >> 31);
        n_pos += (c != 0) + (r != 0);
    }
    printf("%s: %llu records, %llu segments, eps %u, %llu of %llu coordinates with the top bit set\n", bad ? "FAIL" : "OK", (unsigned long long)st.key.size(),
           (unsigned long long)n_seg, eps, (unsigned long long)n_top, (unsigned long long)n_pos);
    return bad ? 1 : 0;
}
