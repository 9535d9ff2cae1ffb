// pa_cns: from the files to a ROW SET — the kept alignments of every part of one backbone as flat records, their two rows in two
// pools (or on the device), and per part what sizes its graph.  Both ingests make one: ingestHost (readFromRefFile, then the score
// rules per part, then flattenParts) and ingestParallel (PA_CNS_INGEST=flat / device: the file mapped and indexed, only the kept
// slices cut and gap-normalised).  Everything after the ingest reads a row set, whichever ingest made it.  Also here: the device
// library, loaded on demand, and the backbone.  A part of pa_cns_main.cpp, which includes it once, after cns_reference.hpp.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include <unistd.h>

#include "../hip/cns_rows.hpp"
#include "cns_cli.hpp"
#include "cns_reference.hpp"
#include "host_threads.hpp"
#include "line_index.hpp"
#include "pagraph_hip.h"
#include "seq_db.hpp"

namespace {

using Clock = std::chrono::steady_clock;
inline double seconds(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// libpagraph_hip.so, loaded on demand from beside the executable (<dir of /proc/self/exe>/../libpagraph_hip.so: where the program
// IS, whatever it was called as and whatever the working directory) or the loader's search path
struct HipLibrary {
    using ConsensusFn = int (*)(int, const char *, std::uint64_t, const pag_cns_part *, std::uint64_t, const pag_cns_aln *, std::uint64_t, const char *, const char *,
                                std::uint64_t, std::int32_t, char *, std::uint64_t, std::uint64_t *, std::uint32_t *, std::int32_t *);
    using ConsensusRowsFn = int (*)(int, int, const char *, std::uint64_t, const pag_cns_part *, std::uint64_t, const pag_cns_aln *, std::uint64_t, const pag_cns_rows *,
                                    std::int32_t, char *, std::uint64_t, std::uint64_t *, std::uint32_t *, std::int32_t *);
    using NormalizeFn = int (*)(int, const char *, std::uint64_t, const pag_cns_slice *, std::uint64_t, pag_cns_row *, pag_cns_rows **);
    using ErrorFn = const char *(*)();
    void *handle = nullptr;
    ConsensusFn consensus = nullptr, consensus_wave = nullptr;
    ConsensusRowsFn consensus_rows = nullptr;
    NormalizeFn normalize = nullptr;
    std::uint64_t (*rows_bytes)(const pag_cns_rows *) = nullptr;
    void (*rows_times)(const pag_cns_rows *, double *, double *) = nullptr;
    void (*rows_counts)(const pag_cns_rows *, std::uint64_t *, std::uint64_t *) = nullptr;
    int (*rows_fetch)(const pag_cns_rows *, char *, char *, std::uint64_t) = nullptr;
    void (*rows_free)(pag_cns_rows *) = nullptr;
    int (*device_available)() = nullptr;
    ErrorFn last_error = nullptr;
    HipLibrary() {
        char exe[4096];
        const ssize_t n = ::readlink("/proc/self/exe", exe, sizeof exe - 1);
        if (n > 0) {
            std::string dir(exe, static_cast<std::size_t>(n));
            const std::size_t slash = dir.rfind('/');
            if (slash != std::string::npos) handle = dlopen((dir.substr(0, slash) + "/../libpagraph_hip.so").c_str(), RTLD_NOW | RTLD_LOCAL);
        }
        if (!handle) handle = dlopen("libpagraph_hip.so", RTLD_NOW | RTLD_LOCAL);
        if (!handle) throw std::runtime_error(std::string("the device backend needs libpagraph_hip.so: ") + dlerror());
        const auto sym = [&](auto &fn, const char *name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(handle, name));
            if (!fn) throw std::runtime_error(std::string("libpagraph_hip.so does not export ") + name);
        };
        sym(consensus, "pag_cns_consensus");
        sym(consensus_wave, "pag_cns_consensus_wave");
        sym(consensus_rows, "pag_cns_consensus_rows");
        sym(normalize, "pag_cns_normalize");
        sym(rows_bytes, "pag_cns_rows_bytes");
        sym(rows_times, "pag_cns_rows_times");
        sym(rows_counts, "pag_cns_rows_counts");
        sym(rows_fetch, "pag_cns_rows_fetch");
        sym(rows_free, "pag_cns_rows_free");
        sym(device_available, "pag_device_available");
        sym(last_error, "pag_last_error");
    }
    HipLibrary(const HipLibrary &) = delete;
    HipLibrary &operator=(const HipLibrary &) = delete;
    ~HipLibrary() {
        if (handle) dlclose(handle);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The row set
// ---------------------------------------------------------------------------------------------------------------------
// A row pool: bytes that are written once, by whoever was told where.  It is never zero-filled: an ingest reserves what its rows
// need and writes into that, a group of a batch appends its jobs' pools.  `mem` stays null while the bytes are on the device
// (RowSet::dev); `size` says how many there are either way.
struct Pool {
    std::unique_ptr<char, decltype(&std::free)> mem{nullptr, &std::free};
    std::uint64_t size = 0, cap = 0;
    const char *data() const { return mem.get(); }
    void grow(std::uint64_t to) {  // (64 bytes of slack past the end, as the row code's writers have always had)
        char *p = static_cast<char *>(std::realloc(mem.get(), to + 64));
        if (!p) throw std::runtime_error("pa_cns: out of memory for the row pools");
        mem.release();
        mem.reset(p);
        cap = to;
    }
    char *reserve(std::uint64_t bytes) {  // an empty pool becomes `bytes` uninitialised bytes, to be written by the caller
        grow(bytes);
        size = bytes;
        return mem.get();
    }
    void append(const char *from, std::uint64_t bytes) {
        if (!mem || size + bytes > cap) grow(std::max(2 * cap, size + bytes));
        std::memcpy(mem.get() + size, from, bytes);
        size += bytes;
    }
};

struct RowSet {
    std::vector<pag_cns_aln> flat;               // the kept alignments of all parts, part after part, in final (sorted) order
    std::vector<std::uint64_t> partFirst;        // part i's are flat[partFirst[i] .. partFirst[i + 1])
    std::vector<std::uint64_t> nIns, nEdgeCols;  // per part: what sizes its graph
    Pool qpool, tpool;                           // alignment a's two rows: [flat[a].str_off, + flat[a].len) of each
    // PA_CNS_INGEST=device: the rows are on the device, where the graph kernels read them next, and the pools hold nothing.
    // Released with the row set, on every way out (the library outlives it: whoever loads it declares it first).
    std::unique_ptr<pag_cns_rows, void (*)(pag_cns_rows *)> dev{nullptr, nullptr};
};

// where an ingest's seconds went, and for `device` the pieces the text went up in and the slices normalised on the host after all
struct IngestTimes {
    std::string by;  // the ingest that made the rows: host, flat or device
    double sIndex = 0, sHeaders = 0, sLists = 0, sRows = 0, sUpload = 0;
    std::uint64_t nPieces = 0, nOversize = 0;
};

// ---------------------------------------------------------------------------------------------------------------------
// PA_CNS_INGEST=flat / device: the rows without readFromRefFile
// ---------------------------------------------------------------------------------------------------------------------

// With `hip`, the kept slices are normalised on the device and stay there (out.dev); without, on host threads into the pools.
// Returns false, with the reason, when a record is not REGULAR: the file then goes through ingestHost.  Regular: the header
// parsed, 0 < refEnd, refBegin < refEnd, both rows of the same length and under 2^31 columns, every slice at least one column.
// Everything else is where the reference's arithmetic wraps (an all-zero record after a malformed header) or where its
// behaviour is undefined (the len - 1 of an empty slice); the goldens pin the std::string code there.
bool ingestParallel(const std::string &path, const std::string &skeleton, std::size_t partLen, std::size_t topK, std::size_t alpha, HipLibrary *hip, int device,
                    RowSet &out, IngestTimes &times, std::string &why) {
    const auto lap = [](Clock::time_point &t) {
        const auto now = Clock::now();
        const double s = std::chrono::duration<double>(now - t).count();
        t = now;
        return s;
    };
    auto t = Clock::now();
    if (skeleton.empty() || partLen == 0) {
        why = "no backbone";
        return false;
    }
    const std::size_t partNum = (skeleton.size() + partLen - 1) / partLen;
    pagh::FileLines lines;
    const bool opened = lines.load(path);  // (a file that cannot be opened holds no record, AlignData.cpp:36-43)
    const std::size_t nRec = opened ? lines.size() / 3 : 0;  // record r is lines 3r, 3r + 1, 3r + 2; a trailing partial record is dropped
    times.sIndex = lap(t);

    // the headers: the same ten stream extractions, one stringstream per thread
    struct Rec {
        std::uint64_t begin, end;
        unsigned score;
        std::uint32_t nSlices;
    };
    std::vector<Rec> recs(nRec);
    std::atomic<std::size_t> firstBad(SIZE_MAX);
    const auto bad = [&](std::size_t r) {
        std::size_t cur = firstBad.load();
        while (r < cur && !firstBad.compare_exchange_weak(cur, r)) {
        }
    };
    constexpr std::size_t kGrain = 2048;
    pagh::parallelFor((nRec + kGrain - 1) / kGrain, 1, [&](std::size_t c) {
        std::stringstream ss;
        std::string queryName, refName, forward, score;
        for (std::size_t r = c * kGrain, e = std::min(nRec, r + kGrain); r < e; ++r) {
            std::size_t queryBegin = 0, queryEnd = 0, querySize = 0, refBegin = 0, refEnd = 0, refSize = 0;
            ss.clear();
            ss.str(lines.str(3 * r));
            ss >> queryName >> refName >> forward >> score >> queryBegin >> queryEnd >> querySize >> refBegin >> refEnd >> refSize;
            Rec &R = recs[r];
            R = Rec{refBegin, refEnd, 0, 0};
            if (ss.fail() || refEnd == 0 || refBegin >= refEnd || lines.length(3 * r + 1) != lines.length(3 * r + 2) || lines.length(3 * r + 2) >= 0x80000000ull) {
                bad(r);
                continue;
            }
            R.score = static_cast<unsigned>(std::atoi(score.c_str()));
            const std::size_t leftPart = refBegin / partLen, rightPart = std::min((refEnd - 1) / partLen, partNum - 1);
            R.nSlices = rightPart >= leftPart ? static_cast<std::uint32_t>(std::min<std::size_t>(rightPart - leftPart + 1, 0xFFFFFFFFu)) : 0;
        }
    });
    if (firstBad.load() != SIZE_MAX) {
        why = "record " + std::to_string(firstBad.load()) + " is not regular (its header or the lengths of its rows)";
        return false;
    }
    std::vector<std::uint64_t> sliceFirst(nRec + 1, 0);
    for (std::size_t r = 0; r < nRec; ++r) sliceFirst[r + 1] = sliceFirst[r] + recs[r].nSlices;
    const std::uint64_t nSlicesAll = sliceFirst[nRec];
    std::vector<std::uint32_t> sliceCols(nSlicesAll);  // every slice's columns: the slot it needs, and no slice may be empty
    const auto sliceOf = [&](std::size_t r, std::size_t part) {
        pag_cns_slice S{};
        S.q_off = lines.offset(3 * r + 1);
        S.t_off = lines.offset(3 * r + 2);
        S.origin_start = recs[r].begin;
        S.slice_start = part * partLen;
        S.slice_end = std::min((part + 1) * partLen, skeleton.size());
        S.n_cols = static_cast<std::uint32_t>(lines.length(3 * r + 2));
        return S;
    };
    pagh::parallelFor((nRec + kGrain - 1) / kGrain, 1, [&](std::size_t c) {
        for (std::size_t r = c * kGrain, e = std::min(nRec, r + kGrain); r < e; ++r) {
            const std::size_t leftPart = recs[r].begin / partLen;
            for (std::uint32_t k = 0; k < recs[r].nSlices; ++k) {
                const pag_cns_slice S = sliceOf(r, leftPart + k);
                std::uint32_t left, right;
                pagrows::slice_bounds(lines.base() + S.t_off, S.n_cols, S.origin_start, S.slice_start, S.slice_end, &left, &right);
                sliceCols[sliceFirst[r] + k] = right - left;
                if (right == left) bad(r);
            }
        }
    });
    if (firstBad.load() != SIZE_MAX) {
        why = "record " + std::to_string(firstBad.load()) + " is not regular (a slice of it has no column)";
        return false;
    }
    times.sHeaders = lap(t);

    // every part's list in file order, then per part the score rules of the host ingest (keptOrder, weightScores):
    // all from the scores, before any row is normalised (a slice's rows depend on nothing else, so cutting first changes nothing)
    struct Cand {
        unsigned score;
        std::uint32_t k;  // slice k of ...
        std::uint64_t rec;
    };
    std::vector<std::vector<Cand>> lists(partNum);
    for (std::size_t r = 0; r < nRec; ++r) {
        const std::size_t leftPart = recs[r].begin / partLen;
        for (std::uint32_t k = 0; k < recs[r].nSlices; ++k) lists[leftPart + k].push_back(Cand{recs[r].score, k, r});
    }
    std::vector<std::vector<std::size_t>> weights(partNum);
    pagh::parallelFor(partNum, 1, [&](std::size_t i) {
        auto &lst = lists[i];
        std::vector<unsigned> scores(lst.size());
        for (std::size_t x = 0; x < lst.size(); ++x) scores[x] = lst[x].score;
        std::vector<Cand> kept;
        for (std::size_t idx : keptOrder(scores, topK)) kept.push_back(lst[idx]);
        scores.clear();
        for (const Cand &c : kept) scores.push_back(c.score);
        lst.swap(kept);
        weights[i] = weightScores(scores, alpha);
    });
    out.partFirst.assign(partNum + 1, 0);
    for (std::size_t i = 0; i < partNum; ++i) out.partFirst[i + 1] = out.partFirst[i] + lists[i].size();
    const std::uint64_t nKept = out.partFirst[partNum];
    if (nKept >= 0xFFFFFFFFull) throw std::runtime_error("pa_cns: more than 2^32 kept alignments");
    out.flat.assign(nKept, pag_cns_aln{});
    std::vector<pag_cns_slice> slices(nKept);
    std::uint64_t poolBytes = 0;
    for (std::size_t i = 0; i < partNum; ++i)
        for (std::size_t x = 0; x < lists[i].size(); ++x) {
            const Cand &c = lists[i][x];
            const std::uint64_t slot = out.partFirst[i] + x;
            const std::size_t leftPart = recs[c.rec].begin / partLen;
            pag_cns_slice S = sliceOf(c.rec, i);
            S.slot = static_cast<std::uint32_t>(slot);
            S.out_off = poolBytes;
            S.out_cap = 2 * sliceCols[sliceFirst[c.rec] + c.k];  // (every column can become two; columns < 2^31 / 2 or the graph stage refuses the part anyway)
            if (sliceCols[sliceFirst[c.rec] + c.k] > 0x7FFFFFFFu) throw std::runtime_error("pa_cns: a slice with more than 2^31 columns");
            poolBytes += S.out_cap;
            slices[slot] = S;
            pag_cns_aln &f = out.flat[slot];
            f.start = static_cast<std::uint32_t>(i == leftPart ? recs[c.rec].begin - leftPart * partLen + 1 : 1);
            f.weight = static_cast<std::int32_t>(weights[i][x]);
        }
    std::vector<std::vector<Cand>>().swap(lists);
    times.sLists = lap(t);

    // the rows of the kept slices
    std::vector<pag_cns_row> rows(nKept);
    if (!hip) {
        char *const qpool = out.qpool.reserve(poolBytes), *const tpool = out.tpool.reserve(poolBytes);
        static_assert(sizeof(pag_cns_slice) == sizeof(pagrows::Slice) && sizeof(pag_cns_row) == sizeof(pagrows::Row), "pag_cns_slice / pag_cns_row are pagrows::Slice / Row");
        pagh::parallelFor(nKept, 64, [&](std::size_t s) {
            pagrows::Slice S;
            std::memcpy(&S, &slices[s], sizeof S);
            const pagrows::Row R = pagrows::run_slice(lines.base(), S, nullptr, nullptr, 1, 0, qpool, tpool);
            std::memcpy(&rows[s], &R, sizeof R);
        });
        times.sRows = lap(t);
    } else {
        // in text order: the text goes up in pieces with their slices
        std::sort(slices.begin(), slices.end(), [](const pag_cns_slice &l, const pag_cns_slice &r) { return l.q_off != r.q_off ? l.q_off < r.q_off : l.slot < r.slot; });
        pag_cns_rows *dev = nullptr;
        const int rc = hip->normalize(device, lines.base(), lines.bytes(), slices.data(), nKept, rows.data(), &dev);
        out.dev = {dev, hip->rows_free};
        out.qpool.size = out.tpool.size = poolBytes;  // (on the device)
        if (rc != 0) throw std::runtime_error("pag_cns_normalize failed (" + std::to_string(rc) + "): " + hip->last_error());
        hip->rows_times(out.dev.get(), &times.sUpload, nullptr);
        hip->rows_counts(out.dev.get(), &times.nPieces, &times.nOversize);
        times.sRows = lap(t) - times.sUpload;
    }
    out.nIns.assign(partNum, 0);
    out.nEdgeCols.assign(partNum, 0);
    for (std::size_t i = 0; i < partNum; ++i)
        for (std::uint64_t s = out.partFirst[i]; s < out.partFirst[i + 1]; ++s) {
            if (rows[s].flag != 0) throw std::runtime_error("pa_cns: a slice did not fit its slot");
            out.flat[s].str_off = rows[s].str_off;
            out.flat[s].len = rows[s].len;
            out.nIns[i] += rows[s].n_ins;
            out.nEdgeCols[i] += rows[s].n_edge_cols;
        }
    return true;
}

struct Backbone {
    std::string name, seq;
};
// the first sequence of the file; false when there is none (a file that cannot be opened is an empty database in the reference,
// AutoSeqDatabase.cpp:9-22)
bool loadBackbone(const std::string &path, Backbone &bb) {
    pagh::SeqDb seqDatabase;
    try {
        seqDatabase = pagh::SeqDb(path);
    } catch (const std::exception &) {
    }
    if (seqDatabase.size() == 0) return false;
    bb.name = seqDatabase.name(0);
    bb.seq = seqDatabase.toString(0, true);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// PA_CNS_INGEST=host: readFromRefFile's lists as a row set
// ---------------------------------------------------------------------------------------------------------------------
// The sorted and cut lists with their weights as flat arrays: every alignment's two rows in the two pools, and per part what
// sizes its graph.  The lists are released as they are copied: their rows live in the pools then.
RowSet flattenParts(std::vector<std::vector<ScoredAln>> &alignments, const std::vector<std::vector<std::size_t>> &partWeights) {
    const std::size_t partNum = alignments.size();
    RowSet out;
    out.partFirst.assign(partNum + 1, 0);
    out.nIns.assign(partNum, 0);
    out.nEdgeCols.assign(partNum, 0);
    std::uint64_t poolBytes = 0;
    for (std::size_t i = 0; i < partNum; ++i) {
        out.partFirst[i + 1] = out.partFirst[i] + partWeights[i].size();
        for (std::size_t x = 0; x < partWeights[i].size(); ++x) poolBytes += alignments[i][x].aln.qstr.size();
    }
    out.flat.reserve(out.partFirst[partNum]);
    char *const qpool = out.qpool.reserve(poolBytes), *const tpool = out.tpool.reserve(poolBytes);
    std::uint64_t at = 0;
    for (std::size_t i = 0; i < partNum; ++i) {
        const auto &alns = alignments[i];
        for (std::size_t x = 0; x < partWeights[i].size(); ++x) {
            const Aln &a = alns[x].aln;
            pag_cns_aln f{};
            f.str_off = at;
            f.len = static_cast<std::uint32_t>(a.qstr.size());
            f.start = a.start;
            f.weight = static_cast<std::int32_t>(partWeights[i][x]);
            out.flat.push_back(f);
            std::memcpy(qpool + at, a.qstr.data(), a.qstr.size());
            std::memcpy(tpool + at, a.tstr.data(), a.qstr.size());
            at += a.qstr.size();
            for (std::size_t c = 0; c < a.qstr.size(); ++c) {
                const char qb = a.qstr[c], tb = a.tstr[c];
                if (qb != '-' && tb == '-') ++out.nIns[i];
                if (qb != '-') ++out.nEdgeCols[i];
            }
        }
        std::vector<ScoredAln>().swap(alignments[i]);
    }
    return out;
}

// readFromRefFile (under `rows` of the times: reading, slicing and normalising are one loop there), then the score rules per part
// on the thread pool (under `lists`), then flattenParts
RowSet ingestHost(const std::string &path, const std::string &skeleton, std::size_t partLen, std::size_t topK, std::size_t alpha, IngestTimes &times) {
    const auto t0 = Clock::now();
    auto alignments = readFromRefFile(path, skeleton, partLen);
    const auto t1 = Clock::now();
    std::vector<std::vector<std::size_t>> partWeights(alignments.size());
    pagh::parallelFor(alignments.size(), 1, [&](std::size_t i) { partWeights[i] = sortCutWeigh(alignments[i], topK, alpha); });
    times.sRows = seconds(t0, t1);
    times.sLists = seconds(t1, Clock::now());
    return flattenParts(alignments, partWeights);
}

// One job's row set by the resolved ingest (`hip`: the loaded library, for `device`).  A file with a record that is not regular is
// read by the host ingest, whatever the mode, for this job alone; times.by says which ingest made the rows.  `forJob`: what the
// line about that says after "the host ingest" (a batch names the file).
RowSet ingestJob(const std::string &ingest, const std::string &path, const std::string &skeleton, const Options &opt, HipLibrary *hip, int device, bool stageTimes,
                 const std::string &forJob, IngestTimes &times) {
    if (ingest != "host") {
        RowSet rows;
        std::string why;
        times.by = ingest;
        if (ingestParallel(path, skeleton, opt.partLen, opt.topK, opt.alpha, hip, device, rows, times, why)) return rows;
        if (stageTimes) std::cerr << "pa_cns: ingest (" + ingest + ") falls back to the host ingest" + forJob + ": " + why + "\n";
    }
    times = IngestTimes{};
    times.by = "host";
    return ingestHost(path, skeleton, opt.partLen, opt.topK, opt.alpha, times);
}

}  // namespace
