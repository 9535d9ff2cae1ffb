// pa_cns — drop-in for the consensus step that follows pagraph in the pipeline (reference
// PAGraph/src/main/pa_cns.cpp:12-168): the backbone (first sequence of -i) is cut into parts of -l bases, the alignments of
// -a (3-line ALN) are sliced per part (tools/cns/AlignData.cpp:36-75), gap-normalised (tools/cns/Alignment.cpp:134-215),
// ordered by score, weighted (AlignData.cpp:77-104), threaded through a partial-order alignment graph per part
// (tools/cns/AlnGraphBoost.cpp: addAln / mergeNodes / bestPath / consensus) and the parts' consensus strings are written as
// one FASTA record, 70 columns.
//
// Where the graphs are built (PA_CNS_BACKEND): `hip` — on the device, one lane of a wavefront per part (pag_cns_consensus,
// csrc/hip/k_cns.hip); `wave` — on the device, a wavefront per part whose lanes share the part's work (pag_cns_consensus_wave,
// csrc/hip/k_cns_wave.hip); both fail without a gfx950 device, there is no silent fallback; `flat` — the device's code
// (csrc/hip/cns_graph.hpp: flat arrays, linked edge lists) compiled for the host, on host threads; `host` — the restatement on
// std::vector / std::map (AlnGraph, cns_reference.hpp), host code like the reference's, what the CPU tests pin on the goldens.  `auto` (the
// default) picks `hip` from kDevicePartsMin parts on and `flat` below.  resolveModes (cns_cli.hpp) holds the values, what `auto` means and
// every pair that cannot run.
//
// Where the rows come from (PA_CNS_INGEST): `host` (the default) — ingestHost over readFromRefFile, one thread, std::string, the
// restatement the CPU tests hold to the reference; `flat` — the file mapped and indexed (line_index.hpp), the headers parsed on
// a thread pool, the per-part lists sorted, cut to -k and weighted from the scores alone, and only the kept slices cut and
// gap-normalised, by csrc/hip/cns_rows.hpp on host threads, straight into the two pools; `device` — the same, the kept slices
// normalised on the device (pag_cns_normalize, csrc/hip/k_cns_rows.hip) where the graph kernels read them next.  A file with a
// record that is not regular (ingestParallel, cns_ingest.hpp) goes through `host`: that is where the reference's arithmetic wraps.
//
// Many backbones in one run: --batch <manifest> (runBatch, cns_batch.hpp) gathers the jobs of a manifest into groups and
// hands a group's parts to the backend in one call; every job's file and stdout lines are the single run's.
//
// What has to be reproduced beyond the arithmetic, because it decides ties:
//   * the graph is boost::adjacency_list<vecS, vecS, bidirectionalS>: out- and in-edge lists are vectors in insertion order,
//     clear_vertex() erases entries in place (order of the others kept), edge(u, v) finds the first match in u's out list,
//     add_edge() appends.  AlnGraph keeps exactly that: per vertex two vectors of edge ids.
//   * `_bbMap` is a std::map read with operator[]: a vertex that was never entered (enter / exit vertex) maps to vertex 0.
//   * bestPath(): float scores, `>` keeps the FIRST best out-edge; nodeScore read with operator[] (0.0f when absent).
//   * the per-part std::sort by score is unstable: the same libstdc++ std::sort with the same comparator on a proxy array
//     in the same initial order gives the same permutation (keptOrder, cns_reference.hpp: the one place).
//   * header fields are read with the same stream extractions; a malformed header yields an all-zero record that is still
//     processed (AlignmentHelper.cpp:24-40) with size_t / uint32_t wrap-around as in the reference.
//
// The program is this one translation unit; its parts are headers it includes once: cns_reference.hpp (the restatement of the
// reference and the score rules), cns_cli.hpp (the command line and the modes), cns_ingest.hpp (from the files to a row set),
// cns_stages.hpp (from a row set to the consensus strings) and cns_batch.hpp (--batch).  A run is: parse, then runBatch, or else
// load the backbone, resolve the modes, ingest, dump, size the parts, run the graph stage, write.
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "cns_batch.hpp"
#include "cns_cli.hpp"
#include "cns_ingest.hpp"
#include "cns_reference.hpp"
#include "cns_stages.hpp"

namespace {

// PA_CNS_STAGE_TIMES=1: the ingest's seconds by step.  The host ingest does not split: reading, slicing and normalising are one
// loop (under `rows`), the per-part sort and the weights come after it (under `lists`; with the host backend the graphs are built in
// there too).
void ingestLines(const IngestTimes &t, std::size_t slices) {
    std::cerr << "pa_cns: ingest (" << t.by << ") index " << t.sIndex << " headers " << t.sHeaders << " lists " << t.sLists << " rows " << t.sRows << " upload " << t.sUpload
              << std::endl;
    if (t.by == "device") std::cerr << "pa_cns: rows on the device: " << slices << " slices, " << t.nPieces << " pieces, " << t.nOversize << " oversize" << std::endl;
}

// one backbone: -i, -a, -o
int runSingle(const Options &opt) {
    Backbone bb;
    if (!loadBackbone(opt.in, bb)) {
        std::cerr << "[Error] No backbone" << std::endl;
        return 2;
    }
    std::unique_ptr<HipLibrary> hip;  // (loaded when, and only when, something runs on the device; it outlives the row set)
    Work w;
    w.backbone = std::move(bb.seq);
    const std::size_t partNum = (w.backbone.size() + opt.partLen - 1) / opt.partLen;
    std::cout << "PartNum=" << partNum << std::endl;
    const Modes mode = resolveModes(false, partNum);
    const bool stageTimes = pagh::envInt("PA_CNS_STAGE_TIMES", 0) != 0;
    const int device = static_cast<int>(pagh::envInt("PAGRAPH_DEVICE", 0));
    std::vector<std::vector<std::string>> results(1, std::vector<std::string>(partNum));
    RowDump dump(partNum);
    IngestTimes times;
    if (mode.backend == "host") {  // the one stage that takes the lists: they are sorted, cut and weighted in there
        const auto tRead = Clock::now();
        auto lists = readFromRefFile(opt.align, w.backbone, opt.partLen);
        times.by = "host";
        times.sRows = seconds(tRead, Clock::now());
        times.sLists = hostStage(lists, w.backbone, opt, stageTimes, dump, results[0]);
        if (stageTimes) ingestLines(times, 0);
    } else {
        if (mode.ingest == "device") {
            hip.reset(new HipLibrary());
            if (hip->device_available() == 0)
                throw std::runtime_error("PA_CNS_INGEST=device: no gfx950 device (pag_cns_normalize runs there; PA_CNS_INGEST=flat makes the rows on host threads)");
        }
        w.rows = ingestJob(mode.ingest, opt.align, w.backbone, opt, hip.get(), device, stageTimes, "", times);
        if (stageTimes) ingestLines(times, w.rows.flat.size());
        sizeParts(w.backbone.size(), opt.partLen, w.rows, 0, 0, 0, w);
        if (dump.path) dump.lines(w, hip.get());
        GraphIo io(w);
        graphStage(mode, io, hip, device, stageTimes);
        handBack(io, w, results, [](std::size_t) { return std::string(); });
    }
    if (dump.path) dump.write();
    finishJob(opt.out, bb.name, w.backbone.size(), results[0]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc <= 1) {
        usage(std::cerr);
        return 0;
    }
    Options opt;
    try {
        opt = parseCli(argc, argv);
    } catch (const HelpRequested &) {
        usage(std::cerr);
        return 0;
    } catch (const ParseError &e) {
        std::cerr << e.what() << std::endl;
        usage(std::cerr);
        return 1;
    }
    if (!opt.batch.empty()) return runBatch(opt);
    try {
        return runSingle(opt);
    } catch (const std::exception &e) {
        std::cerr << "pa_cns: " << e.what() << std::endl;
        return 1;
    }
}
