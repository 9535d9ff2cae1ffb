// oracle/ref_harness/loader_dump.cpp — TEST INFRASTRUCTURE ONLY (built into oracle/_ref/, never shipped).
//
// Drives the REFERENCE's own input readers (compiled from the reference's src/tools, see oracle/Makefile) over ONE file and
// prints what they made of it, as text.  The dumps (tests/golden/loaders/, written by tests/golden/make_loader_golden.py) are
// what pins the product's host loaders (seq_db.cpp, aln_db.cpp) and the ingest kernels (k_ingest.hip) to what the input
// text MEANS to the reference: which bytes are bases, which token is a name, which header is a record, in which order the
// constructor's std::sort leaves records of equal score.
//
// usage: loader_dump <mode> <file>
//   seq     AutoSeqDatabase (seq/AutoSeqDatabase.cpp, SeqHelper.cpp, CompressedSeq.cpp), in database order:
//             R <index> <name> <length> <toString(true)>
//           then the name -> id map, sorted by name (which of two records of one name the map keeps):
//             M <name> <id>
//   mecat   MecatAlignDatabase, mummer   MummerAlignDatabaseV2: the records as the constructor's std::sort leaves them
//             A <index> <queryName> <refName> <F|R> <score> <queryBegin> <queryEnd> <refBegin> <refEnd> <queryDiff> <refDiff>
//   rows    AlignmentHelper::loadFromRefFile + ParseAlignTools::parseDiff, in FILE order, all ten header fields
//             H <index> <queryName> <refName> <F|R> <score text> <queryBegin> <queryEnd> <querySize> <refBegin> <refEnd> <refSize>
//               <queryDiff> <refDiff>
// Names and the score text are printed as lower-case hex of their bytes, `-` when empty; a diff vector as a string of 0 / 1,
// `-` when empty; a sequence of no bases as `-`.
//
// The same source is built a second time under the address and undefined-behaviour sanitizers (oracle/Makefile,
// _ref/loader_dump_san): a file on which the reference's own run is not clean is no fixture.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#define protected public
#include "seq/AutoSeqDatabase.hpp"
#undef protected
#include "align/AlignmentHelper.hpp"
#include "align/MecatAlignDatabase.hpp"
#include "align/MummerAlignDatabaseV2.hpp"
#include "align/ParseAlignTools.hpp"

namespace {

std::string hexOf(const std::string &s) {
    if (s.empty()) return "-";
    static const char *digits = "0123456789abcdef";
    std::string out;
    for (unsigned char c : s) {
        out.push_back(digits[c >> 4]);
        out.push_back(digits[c & 15]);
    }
    return out;
}

std::string bitsOf(const std::vector<bool> &v) {
    if (v.empty()) return "-";
    std::string out(v.size(), '0');
    for (std::size_t i = 0; i < v.size(); ++i)
        if (v[i]) out[i] = '1';
    return out;
}

template <typename Db>
void dumpAlignments(const Db &db) {
    for (std::size_t i = 0; i < db.size(); ++i) {
        const AlignInf &a = db[i];
        std::cout << "A " << i << " " << hexOf(a.getQueryName()) << " " << hexOf(a.getRefName()) << " " << (a.isForward() ? "F" : "R") << " "
                  << a.getScore() << " " << a.getQueryBegin() << " " << a.getQueryEnd() << " " << a.getRefBegin() << " " << a.getRefEnd() << " "
                  << bitsOf(a.getQueryDiff()) << " " << bitsOf(a.getRefDiff()) << "\n";
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: loader_dump seq|mecat|mummer|rows <file>\n");
        return 2;
    }
    const std::string mode = argv[1], path = argv[2];
    if (mode == "seq") {
        AutoSeqDatabase db(path);
        for (std::size_t i = 0; i < db.size(); ++i) {
            const std::string s = db[i].toString(true);
            std::cout << "R " << i << " " << hexOf(db.seqName(i)) << " " << db[i].size() << " " << (s.empty() ? "-" : s) << "\n";
        }
        std::vector<std::pair<std::string, std::size_t>> ids(db._nameToId.begin(), db._nameToId.end());
        std::sort(ids.begin(), ids.end());
        for (auto &p : ids) std::cout << "M " << hexOf(p.first) << " " << p.second << "\n";
    } else if (mode == "mecat") {
        MecatAlignDatabase db(path);
        dumpAlignments(db);
    } else if (mode == "mummer") {
        MummerAlignDatabaseV2 db(path);
        dumpAlignments(db);
    } else if (mode == "rows") {
        std::size_t i = 0;
        AlignmentHelper::loadFromRefFile(path, [&](SimpleAlign &a, const std::string &, const std::string &l2, const std::string &l3) {
            std::vector<bool> q, r;
            ParseAlignTools::parseDiff(l2, l3, q, r);
            std::cout << "H " << i++ << " " << hexOf(a.queryName) << " " << hexOf(a.refName) << " " << (a.forward ? "F" : "R") << " " << hexOf(a.score)
                      << " " << a.queryBegin << " " << a.queryEnd << " " << a.querySize << " " << a.refBegin << " " << a.refEnd << " " << a.refSize << " "
                      << bitsOf(q) << " " << bitsOf(r) << "\n";
        });
    } else {
        std::fprintf(stderr, "loader_dump: unknown mode %s\n", mode.c_str());
        return 2;
    }
    std::cout.flush();
    return std::cout.good() ? 0 : 1;
}
