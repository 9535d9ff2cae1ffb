// pa_cns: from a row set to the consensus strings — the parts sized (sizeParts), the graph stage (graphStage: the flat, lane or
// wave backend over a GraphIo; hostStage: the AlnGraph restatement over the host ingest's lists), the results handed back by index
// (handBack), the row dump (RowDump) and a job's output (finishJob).  The single run and the batch both go through these.  A part
// of pa_cns_main.cpp, which includes it once, after cns_cli.hpp and cns_ingest.hpp.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdint>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../hip/cns_graph.hpp"
#include "cns_cli.hpp"
#include "cns_ingest.hpp"
#include "host_threads.hpp"
#include "pagraph_hip.h"

namespace {

// What a graph stage works on: the backbones of its jobs one after the other (one job in a single run), the row set over them
// all, and the parts in the order the backend gets them: parts[k] is part partOf[k] of job jobOf[k].
struct Work {
    std::string backbone;
    RowSet rows;
    std::vector<pag_cns_part> parts;
    std::vector<std::uint32_t> jobOf, partOf;
};

// The parts of one backbone: the regions of every part's graph sized from its columns (include/pagraph_hip.h,
// pag_cns_consensus).  `rows`: the job's own row set; bbBase / alnBase: where the backbone and the alignments of this job start
// in the arrays the backend gets (0 for a single job).  Appends to `work`.
void sizeParts(std::size_t bbLen, std::size_t partLen, const RowSet &rows, std::size_t job, std::uint64_t bbBase, std::uint64_t alnBase, Work &work) {
    const std::size_t partNum = (bbLen + partLen - 1) / partLen;
    for (std::size_t i = 0; i < partNum; ++i) {
        const std::size_t left = i * partLen, right = std::min((i + 1) * partLen, bbLen);
        pag_cns_part P{};
        P.bb_off = bbBase + left;
        P.bb_len = static_cast<std::uint32_t>(right - left);
        P.aln_first = alnBase + rows.partFirst[i];
        P.n_aln = static_cast<std::uint32_t>(rows.partFirst[i + 1] - rows.partFirst[i]);
        const std::uint64_t nodeCap = P.bb_len + 2ull + rows.nIns[i], edgeCap = P.bb_len + 1ull + rows.nEdgeCols[i] + P.n_aln + 4096ull;
        if (nodeCap > 0x7FFFFFFFull || edgeCap > 0x7FFFFFFFull) throw std::runtime_error("pa_cns: a part with more than 2^31 graph slots");
        P.node_cap = static_cast<std::uint32_t>(nodeCap);
        P.edge_cap = static_cast<std::uint32_t>(edgeCap);
        P.aux_cap = static_cast<std::uint32_t>(std::min<std::uint64_t>(4 * nodeCap + 2048, 0x7FFFFFFFull));
        P.out_cap = P.node_cap;
        work.parts.push_back(P);
        work.jobOf.push_back(static_cast<std::uint32_t>(job));
        work.partOf.push_back(static_cast<std::uint32_t>(i));
    }
}

// What a backend call gets and what it leaves: part p's consensus is buf[off[p] .. + len[p]), err[p] != 0 says why there is none
struct GraphIo {
    const char *backbone;
    std::uint64_t backboneLen;
    const std::vector<pag_cns_part> *parts;
    const std::vector<pag_cns_aln> *flat;
    const char *qrows, *trows;  // (null: the rows are on the device, in `dev`, where the kernels read them: no pool is uploaded)
    std::uint64_t poolBytes;
    pag_cns_rows *dev;
    std::vector<char> buf;
    std::uint64_t outBytes = 0;  // the parts' out_cap together (buf holds 16 more)
    std::vector<std::uint64_t> off;
    std::vector<std::uint32_t> len;
    std::vector<std::int32_t> err;
    explicit GraphIo(const Work &w)
        : backbone(w.backbone.data()), backboneLen(w.backbone.size()), parts(&w.parts), flat(&w.rows.flat), qrows(w.rows.qpool.data()), trows(w.rows.tpool.data()),
          poolBytes(w.rows.qpool.size), dev(w.rows.dev.get()) {
        for (const pag_cns_part &P : *parts) outBytes += P.out_cap;
        buf.assign(outBytes + 16, 0);
        off.assign(parts->size() + 1, 0);
        len.assign(parts->size(), 0);
        err.assign(parts->size(), 0);
    }
};

// the host threads of a stage of `parts` parts
unsigned stageThreads(std::size_t parts) {
    return std::max(1u, std::min<unsigned>(std::max(1u, pagh::usableCpus()), static_cast<unsigned>(std::max<std::size_t>(1, parts))));
}

// the device's code (csrc/hip/cns_graph.hpp) on host threads; phaseNs (with PA_CNS_STAGE_TIMES): add_aln, merge_nodes, best_path + trim
void runFlatBackend(GraphIo &io, unsigned nThreads, bool stageTimes, std::atomic<long long> *phaseNs) {
    const std::vector<pag_cns_part> &parts = *io.parts;
    const std::size_t partNum = parts.size();
    std::uint64_t oo = 0;
    for (std::size_t i = 0; i < partNum; ++i) {
        io.off[i] = oo;
        oo += parts[i].out_cap;
    }
    io.off[partNum] = oo;
    std::atomic<std::size_t> nextPart(0);
    auto flatWork = [&]() {
        for (std::size_t i; (i = nextPart.fetch_add(1)) < partNum;) {
            const pag_cns_part &S = parts[i];
            std::vector<std::uint8_t> nb(S.node_cap), nf(S.node_cap), ev(S.edge_cap);
            std::vector<std::int32_t> ncov(S.node_cap), nw(S.node_cap), nbest(S.node_cap), ec(S.edge_cap);
            std::vector<std::uint32_t> nu[7], eu[6], aux(S.aux_cap);
            for (auto &v : nu) v.resize(S.node_cap);
            for (auto &v : eu) v.resize(S.edge_cap);
            std::vector<float> nscore(S.node_cap);
            pagcns::Arrays A{nb.data(), nf.data(), ncov.data(), nw.data(), nu[0].data(), nu[1].data(), nu[2].data(), nu[3].data(), nu[4].data(), nu[5].data(),
                             nu[6].data(), nscore.data(), nbest.data(), eu[0].data(), eu[1].data(), eu[2].data(), eu[3].data(), eu[4].data(), eu[5].data(),
                             ec.data(), ev.data(), aux.data()};
            pagcns::Part P{};
            P.bb_off = S.bb_off;
            P.bb_len = S.bb_len;
            P.n_aln = S.n_aln;
            P.aln_first = S.aln_first;
            P.out_off = io.off[i];
            P.node_cap = S.node_cap;
            P.edge_cap = S.edge_cap;
            P.aux_cap = S.aux_cap;
            P.out_cap = S.out_cap;
            static_assert(sizeof(pag_cns_aln) == sizeof(pagcns::Aln), "pag_cns_aln is pagcns::Aln");
            std::uint32_t len = 0;
            const auto *fa = reinterpret_cast<const pagcns::Aln *>(io.flat->data());
            if (!stageTimes) {
                io.err[i] = pagcns::run_part(A, P, io.backbone, fa, io.qrows, io.trows, 0, io.buf.data(), &len);
            } else {  // run_part's steps with a clock between them
                pagcns::Graph g;
                pagcns::bind(g, A, P);
                const auto t0 = Clock::now();
                pagcns::init_backbone(g, io.backbone + P.bb_off, P.bb_len);
                for (std::uint32_t a = 0; a < P.n_aln && !g.err; ++a) {
                    const pagcns::Aln &al = fa[P.aln_first + a];
                    pagcns::add_aln(g, io.qrows + al.str_off, io.trows + al.str_off, al.len, al.start, al.weight);
                }
                const auto t1 = Clock::now();
                if (!g.err) pagcns::merge_nodes(g);
                const auto t2 = Clock::now();
                if (!g.err) pagcns::consensus(g, 0, io.buf.data() + P.out_off, P.out_cap, &len);
                const auto t3 = Clock::now();
                phaseNs[0] += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
                phaseNs[1] += std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count();
                phaseNs[2] += std::chrono::duration_cast<std::chrono::nanoseconds>(t3 - t2).count();
                io.err[i] = g.err;
            }
            io.len[i] = io.err[i] ? 0 : len;
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nThreads; ++t) pool.emplace_back(flatWork);
    flatWork();
    for (auto &t : pool) t.join();
}

// hip: one device thread per part (csrc/hip/k_cns.hip); wave: a wavefront per part (csrc/hip/k_cns_wave.hip).  The call fails
// without a gfx950 device: there is no silent fallback.
void runDeviceBackend(HipLibrary &hip, bool wave, int device, GraphIo &io) {
    const std::uint64_t outBytes = io.outBytes;
    const int rc = io.dev ? hip.consensus_rows(device, wave ? 1 : 0, io.backbone, io.backboneLen, io.parts->data(), io.parts->size(), io.flat->data(), io.flat->size(),
                                               io.dev, 0, io.buf.data(), outBytes, io.off.data(), io.len.data(), io.err.data())
                          : (wave ? hip.consensus_wave : hip.consensus)(device, io.backbone, io.backboneLen, io.parts->data(), io.parts->size(), io.flat->data(),
                                                                        io.flat->size(), io.qrows, io.trows, io.poolBytes, 0, io.buf.data(), outBytes, io.off.data(),
                                                                        io.len.data(), io.err.data());
    if (rc != 0)
        throw std::runtime_error(std::string(io.dev ? "pag_cns_consensus_rows" : wave ? "pag_cns_consensus_wave" : "pag_cns_consensus") + " failed (" + std::to_string(rc) +
                                 "): " + hip.last_error());
}

// what a part's error code says (the failures a run reports besides a library error)
std::string partFailure(std::size_t part, std::int32_t err) {
    if (err == pagcns::CNS_E_OVERRUN) return "pa_cns: an alignment runs past the end of its part";
    return "pa_cns: part " + std::to_string(part) + " ran out of its graph regions (code " + std::to_string(err) + ")";
}

// one FASTA record, 70 columns, of the parts' consensus strings
std::string fastaText(const std::string &name, std::size_t backboneLen, const std::vector<std::string> &consensusResults) {
    std::string text;
    text.reserve(backboneLen + backboneLen / 70 + name.size() + 8);
    text += ">" + name + "\n";
    std::size_t cnt = 0;
    for (auto &seq : consensusResults)
        for (char ch : seq) {
            text += ch;
            if (++cnt % 70 == 0) {
                text += '\n';
                cnt = 0;
            }
        }
    if (cnt > 0) text += '\n';
    return text;
}

// The graph stage over flat rows: every part's graph on the resolved backend.  The library is loaded when, and only when, a device
// backend runs and nobody has loaded it yet (it throws when it is missing; the call fails without a gfx950 device: there is no
// silent fallback), so the program starts on a machine without the ROCm runtime.  The seconds are a host clock around the backend
// call, which ends in a device synchronise; under PA_CNS_STAGE_TIMES=1 the HIP runtime's start and the code object's load stay out
// of it, and the stage leaves a line on stderr: `before` graph stage (<backend>) <seconds> s `after`; under `flat` with `flatPhases`
// a second one, the thread-seconds of its three phases.
void graphStage(const Modes &mode, GraphIo &io, std::unique_ptr<HipLibrary> &hip, int device, bool stageTimes, const std::string &before = "pa_cns: ",
                  const std::string &after = "", bool flatPhases = true) {
    std::atomic<long long> phaseNs[3] = {{0}, {0}, {0}};  // flat under PA_CNS_STAGE_TIMES: add_aln, merge_nodes, best_path + trim
    auto tGraph = Clock::now();
    if (mode.onDevice()) {
        if (!hip) hip.reset(new HipLibrary());
        if (stageTimes) {
            (void)hip->device_available();
            tGraph = Clock::now();
        }
        runDeviceBackend(*hip, mode.backend == "wave", device, io);
    } else {
        runFlatBackend(io, stageThreads(io.parts->size()), stageTimes, phaseNs);
    }
    if (!stageTimes) return;
    std::cerr << before << "graph stage (" << mode.backend << ") " << seconds(tGraph, Clock::now()) << " s" << after << std::endl;
    if (mode.backend == "flat" && flatPhases)
        std::cerr << "pa_cns: flat phases (thread-seconds) add_aln " << phaseNs[0] * 1e-9 << " merge_nodes " << phaseNs[1] * 1e-9 << " best_path+trim " << phaseNs[2] * 1e-9
                  << std::endl;
}

// PA_CNS_DUMP_ROWS=<file>: part start weight qrow trow, a line per kept alignment, parts in order, alignments in final order —
// what the graphs are built from, whichever ingest made it and whichever backend reads it
struct RowDump {
    const char *path = std::getenv("PA_CNS_DUMP_ROWS");
    std::vector<std::string> text;  // per part
    explicit RowDump(std::size_t partNum) : text(path ? partNum : 0) {}
    void line(std::size_t part, std::uint32_t start, long long weight, const char *q, const char *t, std::size_t len) {
        std::string &to = text[part];
        to += std::to_string(part) + ' ' + std::to_string(start) + ' ' + std::to_string(weight) + ' ';
        to.append(q, len);
        to += ' ';
        to.append(t, len);
        to += '\n';
    }
    // the rows of one job's work (a verification aid: rows that are on the device come back for the dump alone)
    void lines(const Work &w, HipLibrary *hip) {
        const RowSet &rows = w.rows;
        std::vector<char> fq, ft;
        if (rows.dev) {
            fq.resize(rows.qpool.size + 1);
            ft.resize(rows.qpool.size + 1);
            const int rc = hip->rows_fetch(rows.dev.get(), fq.data(), ft.data(), rows.qpool.size);
            if (rc != 0) throw std::runtime_error("pag_cns_rows_fetch failed (" + std::to_string(rc) + "): " + hip->last_error());
        }
        const char *dq = rows.dev ? fq.data() : rows.qpool.data(), *dt = rows.dev ? ft.data() : rows.tpool.data();
        pagh::parallelFor(w.parts.size(), 1, [&](std::size_t i) {
            for (std::uint64_t a = w.parts[i].aln_first; a < w.parts[i].aln_first + w.parts[i].n_aln; ++a)
                line(w.partOf[i], rows.flat[a].start, rows.flat[a].weight, dq + rows.flat[a].str_off, dt + rows.flat[a].str_off, rows.flat[a].len);
        });
    }
    void write() const {
        std::ofstream df(path);
        for (const std::string &t : text) df << t;
        if (!df) throw std::runtime_error(std::string("PA_CNS_DUMP_ROWS: cannot write ") + path);
    }
};

// PA_CNS_BACKEND=host: the graphs on the std::vector / std::map restatement (AlnGraph), straight from the host ingest's lists.
// Per part on the host threads: the score rules, its lines of the dump, its graph; its list is freed when its graph is built.
// The stage's seconds hold the per-part sort.  -> the seconds
double hostStage(std::vector<std::vector<ScoredAln>> &lists, const std::string &backbone, const Options &opt, bool stageTimes, RowDump &dump,
                 std::vector<std::string> &results) {
    const std::size_t partNum = results.size();
    std::atomic<std::size_t> next(0);
    std::atomic<bool> failed(false);
    std::string failure;
    const auto tSort = Clock::now();
    auto work = [&]() {
        for (std::size_t i; (i = next.fetch_add(1)) < partNum;) {
            try {
                auto &alns = lists[i];
                const std::vector<std::size_t> weights = sortCutWeigh(alns, opt.topK, opt.alpha);
                const std::size_t left = i * opt.partLen, right = std::min((i + 1) * opt.partLen, backbone.size());
                if (dump.path)
                    for (std::size_t x = 0; x < weights.size(); ++x)
                        dump.line(i, alns[x].aln.start, static_cast<std::int32_t>(weights[x]), alns[x].aln.qstr.data(), alns[x].aln.tstr.data(), alns[x].aln.qstr.size());
                AlnGraph g(backbone.substr(left, right - left));
                for (std::size_t x = 0; x < weights.size(); ++x) g.addAln(alns[x].aln, static_cast<int>(weights[x]));
                g.mergeNodes();
                results[i] = g.consensus();
                std::vector<ScoredAln>().swap(alns);
            } catch (const std::exception &e) {
                if (!failed.exchange(true)) failure = e.what();
            }
        }
    };
    {
        std::vector<std::thread> pool;
        for (unsigned t = 1, n = stageThreads(partNum); t < n; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
    }
    if (failed) throw std::runtime_error(failure);
    const double sSort = seconds(tSort, Clock::now());
    if (stageTimes) std::cerr << "pa_cns: graph stage (host, with the per-part sort) " << sSort << " s" << std::endl;
    return sSort;
}

// The results of a graph stage back to the jobs by index: part k's consensus is results[jobOf[k]][partOf[k]].  Throws for the
// failing part that comes first in job order, then part order; `jobName(job)` is what its message starts with.
template <typename JobName>
void handBack(const GraphIo &io, const Work &w, std::vector<std::vector<std::string>> &results, JobName jobName) {
    std::size_t badK = SIZE_MAX;
    for (std::size_t k = 0; k < w.parts.size(); ++k) {
        if (io.err[k]) {
            if (badK == SIZE_MAX || std::make_pair(w.jobOf[k], w.partOf[k]) < std::make_pair(w.jobOf[badK], w.partOf[badK])) badK = k;
            continue;
        }
        results[w.jobOf[k]][w.partOf[k]].assign(io.buf.data() + io.off[k], io.len[k]);
    }
    if (badK != SIZE_MAX) throw std::runtime_error(jobName(w.jobOf[badK]) + partFailure(w.partOf[badK], io.err[badK]));
}

// what a job leaves when its parts are done: the two numbers on stdout and the FASTA file
void finishJob(const std::string &out, const std::string &name, std::size_t backboneLen, const std::vector<std::string> &results) {
    std::size_t consensusLen = 0;
    for (const std::string &s : results) consensusLen += s.size();
    std::cout << consensusLen << std::endl;
    std::cout << backboneLen << std::endl;
    std::ofstream of(out);
    of << fastaText(name, backboneLen, results);
}

}  // namespace
