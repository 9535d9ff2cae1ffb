// The row code of pa_cns (csrc/hip/cns_rows.hpp: slice_bounds, normalize_gaps, run_slice) against a std::string restatement of the
// reference (AlignData::sliceHelper, AlignData.cpp:11-34; dagcon normalizeGaps, cns/Alignment.cpp:131-217) on seeded rows, as a
// program of its own: built with -fsanitize=address,undefined by tests/test_cns_rows.py, every buffer a heap block of exactly the
// size the contract names (2 x the slice's columns), so that an index past it is a finding.  Host code only.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "cns_rows.hpp"

namespace {

void referenceBounds(const std::string &tstr, std::size_t originStart, std::size_t sliceStart, std::size_t sliceEnd, std::size_t *l, std::size_t *r) {
    std::size_t left, right, cnt = 0;
    for (left = 0; left < tstr.size(); ++left) {
        if (tstr[left] == '-') continue;
        if (originStart + cnt >= sliceStart) break;
        ++cnt;
    }
    for (right = left; right < tstr.size(); ++right) {
        if (tstr[right] == '-') continue;
        if (originStart + cnt >= sliceEnd) break;
        ++cnt;
    }
    *l = left;
    *r = right;
}

void referenceNormalize(std::string qstr, std::string tstr, std::string *qOut, std::string *tOut) {
    std::size_t len = qstr.length();
    std::string qNorm, tNorm;
    for (std::size_t i = 0; i < len; i++) {
        if ('.' == qstr[i]) qstr[i] = '-';
        if ('.' == tstr[i]) tstr[i] = '-';
    }
    for (std::size_t i = 0; i < len; i++) {
        const char qb = qstr[i], tb = tstr[i];
        if (qb != tb && qb != '-' && tb != '-') {
            qNorm += '-';
            qNorm += qb;
            tNorm += tb;
            tNorm += '-';
        } else {
            qNorm += qb;
            tNorm += tb;
        }
    }
    len = qNorm.length();
    for (std::size_t i = 0; len != 0 && i < len - 1; i++) {
        if (tNorm[i] == '-') {
            std::size_t j = i;
            while (++j < len) {
                const char c = tNorm[j];
                if (c != '-') {
                    if (c == qNorm[i]) {
                        tNorm[i] = c;
                        tNorm[j] = '-';
                    }
                    break;
                }
            }
        }
        if (qNorm[i] == '-') {
            std::size_t j = i;
            while (++j < len) {
                const char c = qNorm[j];
                if (c != '-') {
                    if (c == tNorm[i]) {
                        qNorm[i] = c;
                        qNorm[j] = '-';
                    }
                    break;
                }
            }
        }
    }
    qOut->clear();
    tOut->clear();
    for (std::size_t i = 0; i < len; i++)
        if (qNorm[i] != '-' || tNorm[i] != '-') {
            *qOut += qNorm[i];
            *tOut += tNorm[i];
        }
}

int failures = 0;
void fail(const char *what, unsigned long long a, unsigned long long b) {
    if (++failures <= 10) std::printf("FAIL %s (%llu, %llu)\n", what, a, b);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240607);
    const auto pick = [&](std::uint64_t n) { return static_cast<std::uint64_t>(rng() % n); };
    const char alphabet[] = "ACGTACGTACGT---..Nacg\r";
    unsigned long long cases = 0, columns = 0;
    // the column counts around the 64-column chunks, empty rows, and longer ones
    const std::uint32_t lengths[] = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 700, 2000};
    for (int round = 0; round < 60; ++round)
        for (const std::uint32_t n : lengths) {
            // two rows of n columns: homopolymer stretches, gap runs of up to 150 columns, mismatch runs
            std::string q, t;
            while (q.size() < n) {
                const std::uint64_t kind = pick(8), run = 1 + pick(kind == 0 ? 150 : 12);
                const char a = alphabet[pick(sizeof alphabet - 1)], b = alphabet[pick(sizeof alphabet - 1)];
                for (std::uint64_t x = 0; x < run && q.size() < n; ++x) {
                    if (kind == 0) {  // a gap run in one row
                        q += (round & 1) ? '-' : a;
                        t += (round & 1) ? a : '-';
                    } else if (kind == 1) {  // a homopolymer in both
                        q += a;
                        t += a;
                    } else if (kind == 2) {  // a run of mismatches
                        q += a;
                        t += b;
                    } else {
                        q += alphabet[pick(sizeof alphabet - 1)];
                        t += pick(4) ? q.back() : alphabet[pick(sizeof alphabet - 1)];
                    }
                }
            }
            // the record as text: the two rows one after the other, nothing behind them
            const std::size_t bytes = 2 * static_cast<std::size_t>(n) + 1;
            std::unique_ptr<char[]> text(new char[bytes]);
            std::memcpy(text.get(), q.data(), n);
            text[n] = '\n';
            std::memcpy(text.get() + n + 1, t.data(), n);
            std::size_t bases = 0;
            for (char c : t) bases += c != '-';
            const std::uint64_t origin = pick(1000), partLen = 1 + pick(bases + 2);
            for (std::uint64_t part = origin / partLen; part <= (origin + bases + 1) / partLen; ++part) {
                std::size_t l, r;
                referenceBounds(t, origin, part * partLen, (part + 1) * partLen, &l, &r);
                std::uint32_t l2, r2;
                pagrows::slice_bounds(text.get() + n + 1, n, origin, part * partLen, (part + 1) * partLen, &l2, &r2);
                if (l != l2 || r != r2) fail("slice_bounds", l2, r2);
                std::string wantQ, wantT;
                referenceNormalize(q.substr(l, r - l), t.substr(l, r - l), &wantQ, &wantT);
                const std::uint32_t cols = static_cast<std::uint32_t>(r - l), cap = 2 * cols;
                std::uint32_t nIns = 0, nEdge = 0;
                for (std::size_t i = 0; i < wantQ.size(); ++i) {
                    nIns += wantQ[i] != '-' && wantT[i] == '-';
                    nEdge += wantQ[i] != '-';
                }
                pagrows::Slice S{};
                S.q_off = 0;
                S.t_off = n + 1;
                S.origin_start = origin;
                S.slice_start = part * partLen;
                S.slice_end = (part + 1) * partLen;
                S.n_cols = n;
                S.out_cap = cap;
                // (a) the slot itself as the work space, as host threads run it
                {
                    std::unique_ptr<char[]> qo(new char[cap ? cap : 1]), to(new char[cap ? cap : 1]);
                    const pagrows::Row R = pagrows::run_slice(text.get(), S, nullptr, nullptr, 1, 0, qo.get(), to.get());
                    if (R.flag != pagrows::ROW_OK || R.len != wantQ.size() || std::memcmp(qo.get(), wantQ.data(), R.len) || std::memcmp(to.get(), wantT.data(), R.len))
                        fail("run_slice in place", R.len, wantQ.size());
                    if (R.n_ins != nIns || R.n_edge_cols != nEdge) fail("counts", R.n_ins, R.n_edge_cols);
                }
                // (b) work rows column by column among 64 lanes' (stride 64, lane `lane`), of exactly 2 x columns, as the device runs it
                {
                    const std::uint32_t lane = static_cast<std::uint32_t>(pick(64));
                    const std::size_t work = cap ? (static_cast<std::size_t>(cap) - 1) * 64 + lane + 1 : 1;
                    std::unique_ptr<char[]> wq(new char[work]), wt(new char[work]), qo(new char[cap ? cap : 1]), to(new char[cap ? cap : 1]);
                    const pagrows::Row R = pagrows::run_slice(text.get(), S, wq.get() + lane, wt.get() + lane, 64, cap, qo.get(), to.get());
                    if (R.flag != pagrows::ROW_OK || R.len != wantQ.size() || std::memcmp(qo.get(), wantQ.data(), R.len) || std::memcmp(to.get(), wantT.data(), R.len))
                        fail("run_slice strided", R.len, wantQ.size());
                    if (R.n_ins != nIns || R.n_edge_cols != nEdge) fail("counts strided", R.n_ins, R.n_edge_cols);
                    // one column short: flagged, nothing touched
                    if (cap) {
                        const pagrows::Row O = pagrows::run_slice(text.get(), S, wq.get() + lane, wt.get() + lane, 64, cap - 1, qo.get(), to.get());
                        if (O.flag != pagrows::ROW_OVERSIZE) fail("oversize flag", O.flag, cap);
                        pagrows::Slice T = S;
                        T.out_cap = cap - 1;
                        const pagrows::Row E = pagrows::run_slice(text.get(), T, nullptr, nullptr, 1, 0, qo.get(), to.get());
                        if (E.flag != pagrows::ROW_E_SLOT) fail("slot flag", E.flag, cap);
                    }
                }
                ++cases;
                columns += cols;
            }
        }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%llu cases ok (%llu columns)\n", cases, columns);
    return 0;
}
