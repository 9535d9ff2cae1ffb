// pa_cns --batch: the jobs of a manifest in one run (runBatch), group after group through the pieces of the single run
// (cns_ingest.hpp, cns_stages.hpp).  A part of pa_cns_main.cpp, which includes it once.
#pragma once
#include <cstdint>
#include <fstream>
#include <future>
#include <iostream>
#include <map>
#include <memory>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cns_cli.hpp"
#include "cns_ingest.hpp"
#include "cns_stages.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// --batch: the jobs of a manifest in one run.  The pipeline calls pa_cns once per new contig (AlignGraph2.py:500-510), a few
// hundred parts each; the device backends pay from thousands of parts on, and every call pays its own start.  Here whole jobs
// are gathered into GROUPS; a group's parts go to the backend in ONE call: the backbones one after the other, one pool pair,
// bb_off / aln_first / str_off rebased.  Every job's output file and stdout lines are what its single run writes.
//
// Host memory: all backbones are loaded before any work (a byte a base, released as their group is built), and at most two
// groups are alive — the one on the device and the one being ingested.  A group closes once it holds PA_CNS_BATCH_PARTS parts
// (default kBatchParts) or its two row pools hold PA_CNS_BATCH_BYTES bytes together (default kBatchBytes), so a group holds at
// most the limit plus one job; while a pool grows it may transiently hold twice that.  The length of the manifest does not enter.
// ---------------------------------------------------------------------------------------------------------------------
constexpr std::size_t kBatchParts = 4096;            // (1 000 parts leave the device three quarters empty, profiles/r07_pa_cns_wave_timing.json)
constexpr std::uint64_t kBatchBytes = 8ull << 30;    // both pools of a group together

// (a failure of one job is a std::runtime_error whose what() starts with the job's backbone path)
struct BatchJob {
    std::size_t line = 0;  // of the manifest, 1-based
    std::string in, align, out;
    Backbone bb;
    std::size_t bbLen = 0, partNum = 0;
};

// The work of the jobs firstJob .. firstJob + nJobs: jobOf counts from firstJob, the parts are by estimated cost, heaviest first.
// (Of its row set the per-part vectors stay empty: the parts were sized job by job.)
struct Group : Work {
    std::size_t firstJob = 0, nJobs = 0;
    double sIngest = 0;
    Clock::time_point ready;
};

// a job's row set and backbone onto the end of a group's: its parts sized, str_off / aln_first / bb_off rebased
void appendJob(Work &g, std::size_t job, const std::string &backbone, std::size_t partLen, const RowSet &rows) {
    const std::uint64_t bbBase = g.backbone.size(), alnBase = g.rows.flat.size(), strBase = g.rows.qpool.size;
    sizeParts(backbone.size(), partLen, rows, job, bbBase, alnBase, g);
    g.rows.flat.reserve(g.rows.flat.size() + rows.flat.size());
    for (pag_cns_aln f : rows.flat) {
        f.str_off += strBase;
        g.rows.flat.push_back(f);
    }
    g.backbone += backbone;
    g.rows.qpool.append(rows.qpool.data(), rows.qpool.size);
    g.rows.tpool.append(rows.tpool.data(), rows.tpool.size);
}

// the jobs from `first` on, ingested one after the other (each on all host threads) until the group closes
Group buildGroup(std::vector<BatchJob> &jobs, std::size_t first, const Options &opt, const std::string &ingest, std::size_t limitParts, std::uint64_t limitBytes,
                 bool stageTimes) {
    const auto t0 = Clock::now();
    Group g;
    g.firstJob = first;
    for (std::size_t j = first; j < jobs.size(); ++j) {
        BatchJob &job = jobs[j];
        try {
            IngestTimes times;
            appendJob(g, j - first, job.bb.seq, opt.partLen, ingestJob(ingest, job.align, job.bb.seq, opt, nullptr, 0, stageTimes, " for " + job.align, times));
            std::string().swap(job.bb.seq);
        } catch (const std::exception &e) {
            throw std::runtime_error(job.in + ": " + e.what());
        }
        ++g.nJobs;
        if (g.parts.size() >= limitParts || g.rows.qpool.size + g.rows.tpool.size >= limitBytes) break;
    }
    // Heaviest first: the kernel's grid takes blocks in array order, and a group's run time ends with its slowest part.  The
    // estimate is the part's alignment columns plus its backbone; ties keep manifest order, then part order (the sort is stable).
    const std::size_t nParts = g.parts.size();
    std::vector<std::uint64_t> cost(nParts);
    for (std::size_t k = 0; k < nParts; ++k) {
        cost[k] = g.parts[k].bb_len;
        for (std::uint64_t a = g.parts[k].aln_first; a < g.parts[k].aln_first + g.parts[k].n_aln; ++a) cost[k] += g.rows.flat[a].len;
    }
    std::vector<std::size_t> order(nParts);
    std::iota(order.begin(), order.end(), std::size_t(0));
    std::stable_sort(order.begin(), order.end(), [&](std::size_t l, std::size_t r) { return cost[l] > cost[r]; });
    std::vector<pag_cns_part> parts(nParts);
    std::vector<std::uint32_t> jobOf(nParts), partOf(nParts);
    for (std::size_t k = 0; k < nParts; ++k) {
        parts[k] = g.parts[order[k]];
        jobOf[k] = g.jobOf[order[k]];
        partOf[k] = g.partOf[order[k]];
    }
    g.parts.swap(parts);
    g.jobOf.swap(jobOf);
    g.partOf.swap(partOf);
    // (the kernels index the arrays by what the parts say: every range is checked here, before anything runs on them)
    for (const pag_cns_part &P : g.parts) {
        bool ok = P.bb_off + P.bb_len <= g.backbone.size() && P.aln_first + P.n_aln <= g.rows.flat.size();
        for (std::uint64_t a = P.aln_first; ok && a < P.aln_first + P.n_aln; ++a) ok = g.rows.flat[a].str_off + g.rows.flat[a].len <= g.rows.qpool.size;
        if (!ok) throw std::logic_error("pa_cns: a part of the group reaches out of the group's arrays");
    }
    g.ready = Clock::now();
    g.sIngest = seconds(t0, g.ready);
    return g;
}

std::vector<BatchJob> readManifest(const std::string &path) {
    std::ifstream in(path);
    if (!in.is_open()) throw std::runtime_error("--batch: cannot read " + path);
    std::vector<BatchJob> jobs;
    std::map<std::string, std::size_t> outputs;
    std::string text;
    for (std::size_t line = 1; std::getline(in, text); ++line) {
        if (!text.empty() && text.back() == '\r') text.pop_back();
        if (text.empty()) continue;
        std::vector<std::string> fields(1);
        for (char c : text) {
            if (c == '\t') fields.emplace_back();
            else fields.back() += c;
        }
        bool ok = fields.size() == 3;
        for (const std::string &f : fields) ok = ok && !f.empty();
        if (!ok)
            throw std::runtime_error(path + " line " + std::to_string(line) + ": a job is three TAB-separated fields (backbone, alignments, output), this line has " +
                                     std::to_string(fields.size()) + (fields.size() == 3 ? ", one of them empty" : ""));
        const auto seen = outputs.emplace(fields[2], line);
        if (!seen.second)
            throw std::runtime_error(path + " line " + std::to_string(line) + ": the output " + fields[2] + " is the output of line " + std::to_string(seen.first->second) + " already");
        BatchJob job;
        job.line = line;
        job.in = fields[0];
        job.align = fields[1];
        job.out = fields[2];
        jobs.push_back(std::move(job));
    }
    return jobs;
}

int runBatch(const Options &opt) {
    try {
        // what a batch cannot run under, before any work (the modes once more below, when the parts are counted: `auto` goes by them)
        (void)resolveModes(true, 0);
        if (std::getenv("PA_CNS_DUMP_ROWS")) throw std::runtime_error("--batch does not take PA_CNS_DUMP_ROWS (the dump is one job's rows): run that job alone");
        if (opt.partLen == 0) throw std::runtime_error("--batch needs a part length (-l) above 0");
        const long long partsEnv = pagh::envInt("PA_CNS_BATCH_PARTS", static_cast<long long>(kBatchParts));
        const long long bytesEnv = pagh::envInt("PA_CNS_BATCH_BYTES", static_cast<long long>(kBatchBytes));
        if (partsEnv < 1 || bytesEnv < 1) throw std::runtime_error("PA_CNS_BATCH_PARTS and PA_CNS_BATCH_BYTES are numbers above 0");
        const std::size_t limitParts = static_cast<std::size_t>(partsEnv);
        const std::uint64_t limitBytes = static_cast<std::uint64_t>(bytesEnv);
        const bool stageTimes = pagh::envInt("PA_CNS_STAGE_TIMES", 0) != 0;
        std::vector<BatchJob> jobs = readManifest(opt.batch);

        // all backbones first: a job without one ends the run before anything is written
        std::size_t totalParts = 0;
        for (BatchJob &job : jobs) {
            if (!loadBackbone(job.in, job.bb)) {
                std::cerr << "[Error] No backbone: " << job.in << std::endl;
                return 2;
            }
            job.bbLen = job.bb.seq.size();
            job.partNum = (job.bbLen + opt.partLen - 1) / opt.partLen;
            totalParts += job.partNum;
        }
        const Modes mode = resolveModes(true, totalParts);
        if (stageTimes)
            std::cerr << "pa_cns: batch of " << jobs.size() << " jobs, " << totalParts << " parts: backend " << mode.backend << (mode.chosen ? " (auto)" : "") << ", ingest "
                      << mode.ingest << std::endl;
        const bool onDevice = mode.onDevice();
        const int device = static_cast<int>(pagh::envInt("PAGRAPH_DEVICE", 0));
        std::unique_ptr<HipLibrary> hip;
        if (onDevice && !jobs.empty()) {
            hip.reset(new HipLibrary());       // (before any job is read: it throws when the library is missing)
            (void)hip->device_available();     // (the HIP runtime's start stays out of the first group's clock)
        }
        const auto build = [&](std::size_t first) { return buildGroup(jobs, first, opt, mode.ingest, limitParts, limitBytes, stageTimes); };

        // Group after group.  With a device backend the next group is ingested on the host threads while this one's call is on the
        // device; with `flat` the host threads are the backend, so the groups run one after the other.
        std::future<Group> nextGroup;
        if (onDevice && !jobs.empty()) nextGroup = std::async(std::launch::async, build, std::size_t(0));
        for (std::size_t first = 0, gi = 0; first < jobs.size(); ++gi) {
            const auto tWait = Clock::now();
            Group g = onDevice ? nextGroup.get() : build(first);
            const double sDeviceWaited = onDevice ? seconds(tWait, Clock::now()) : 0.0;
            const double sIngestWaited = onDevice ? std::max(0.0, seconds(g.ready, tWait)) : 0.0;
            first = g.firstJob + g.nJobs;
            if (onDevice && first < jobs.size()) nextGroup = std::async(std::launch::async, build, first);
            const BatchJob &head = jobs[g.firstJob];
            const std::string groupName = head.in + (g.nJobs > 1 ? " (the first of a group of " + std::to_string(g.nJobs) + " jobs)" : "");

            GraphIo io(g);
            std::ostringstream before, after;  // (one line per group; the flat phases are not reported)
            before << "pa_cns: group " << gi << ": jobs " << g.nJobs << " parts " << g.parts.size() << " ingest " << g.sIngest << " s ";
            after << " device waited " << sDeviceWaited << " s ingest waited " << sIngestWaited << " s";
            try {
                graphStage(mode, io, hip, device, stageTimes, before.str(), after.str(), false);
            } catch (const std::exception &e) {
                throw std::runtime_error(groupName + ": " + e.what());
            }

            // back to the jobs by index; a failing part ends the run before anything of this group is written
            std::vector<std::vector<std::string>> results(g.nJobs);
            for (std::size_t j = 0; j < g.nJobs; ++j) results[j].resize(jobs[g.firstJob + j].partNum);
            handBack(io, g, results, [&](std::size_t j) { return jobs[g.firstJob + j].in + ": "; });
            for (std::size_t j = 0; j < g.nJobs; ++j) {
                const BatchJob &job = jobs[g.firstJob + j];
                std::cout << "PartNum=" << job.partNum << std::endl;
                finishJob(job.out, job.bb.name, job.bbLen, results[j]);
            }
        }
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "pa_cns: " << e.what() << std::endl;
        return 1;
    }
}

}  // namespace
