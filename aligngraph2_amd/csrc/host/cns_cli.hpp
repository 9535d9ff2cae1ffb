// pa_cns: what a run is told — the command line (Options, parseCli) and the two mode variables of the environment
// (PA_CNS_BACKEND, PA_CNS_INGEST: resolveModes, with every pair that cannot run).  A part of pa_cns_main.cpp, which includes it
// once.
#pragma once
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// command line (args.hxx surface of pa_cns.cpp:23-46)
// ---------------------------------------------------------------------------------------------------------------------
struct Options {
    unsigned threads = 16;
    std::size_t partLen = 5000, topK = 3000, alpha = 250;
    std::string in, out, align;
    std::string batch;  // --batch: a manifest of jobs (backbone, alignments, output) instead of -i / -a / -o
};
void usage(std::ostream &os) {
    os << "  pa_cns {OPTIONS}\n\n  OPTIONS:\n\n"
          "      -h, --help                        display this help menu\n"
          "      -t[thread_num], --thread=[thread_num]   number of thread\n"
          "      -l[size], --len=[size]            length of part\n"
          "      -k[k], --top_k=[k]                top n\n"
          "      --alpha=[alpha]                   alpha\n"
          "      -i[path], --in=[path]             input of backbone\n"
          "      -o[path], --out=[path]            output of file\n"
          "      -a[path], --align=[path]          alignments file\n"
          "      --batch=[manifest]                many jobs in one run: a line per job, backbone TAB alignments TAB output (instead of -i -a -o)\n";
}
struct ParseError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct HelpRequested {};
template <typename T>
T parseNumber(const std::string &flag, const std::string &v) {
    std::istringstream ss(v);
    T x{};
    ss >> x;
    if (ss.fail() || ss.rdbuf()->in_avail() != 0) throw ParseError("Argument '" + flag + "' received invalid value type '" + v + "'");
    return x;
}
Options parseCli(int argc, char **argv) {
    Options o;
    auto assign = [&](const std::string &name, const std::string &value) {
        if (name == "t" || name == "thread") o.threads = parseNumber<unsigned>(name, value);
        else if (name == "l" || name == "len") o.partLen = parseNumber<std::size_t>(name, value);
        else if (name == "k" || name == "top_k") o.topK = parseNumber<std::size_t>(name, value);
        else if (name == "alpha") o.alpha = parseNumber<std::size_t>(name, value);
        else if (name == "i" || name == "in") o.in = value;
        else if (name == "o" || name == "out") o.out = value;
        else if (name == "a" || name == "align") o.align = value;
        else if (name == "batch") o.batch = value;
        else throw ParseError("Flag could not be matched: " + name);
    };
    auto isLong = [](const std::string &n) {
        for (const char *x : {"thread", "len", "top_k", "alpha", "in", "out", "align", "batch"})
            if (n == x) return true;
        return false;
    };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-h" || a == "--help") throw HelpRequested{};
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            std::string body = a.substr(2), value;
            auto eq = body.find('=');
            if (eq != std::string::npos) {
                value = body.substr(eq + 1);
                body = body.substr(0, eq);
                if (!isLong(body)) throw ParseError("Flag could not be matched: " + body);
            } else {
                if (!isLong(body)) throw ParseError("Flag could not be matched: " + body);
                if (i + 1 >= argc) throw ParseError("Flag '" + body + "' requires an argument but received none");
                value = argv[++i];
            }
            assign(body, value);
        } else if (a.size() >= 2 && a[0] == '-') {
            std::string name(1, a[1]);
            if (std::strchr("tlkioa", a[1]) == nullptr) throw ParseError("Flag could not be matched: '" + name + "'");
            std::string value;
            if (a.size() > 2) value = a.substr(2);
            else {
                if (i + 1 >= argc) throw ParseError("Flag '" + name + "' requires an argument but received none");
                value = argv[++i];
            }
            assign(name, value);
        } else {
            throw ParseError("Passed in argument, but no positional arguments were ready to receive it: " + a);
        }
    }
    if (!o.batch.empty() && !(o.in.empty() && o.out.empty() && o.align.empty()))
        throw ParseError("Flag 'batch' names the inputs and outputs of every job: it cannot be combined with 'i', 'a' or 'o'");
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// The modes of a run: where the per-part graphs are built (PA_CNS_BACKEND) and where the rows come from (PA_CNS_INGEST); the
// head of pa_cns_main.cpp says what each value is.
//
// `auto`, the default backend, goes by the number of parts: a part is a serial chain of dependent accesses, the device wins by
// running thousands side by side, host threads win on the few hundred parts of one contig of the pipeline (AlignGraph2.py:503
// calls pa_cns once per new contig; profiles/r06_pa_cns_timing.json).
// ---------------------------------------------------------------------------------------------------------------------
// parts from which a single run's `auto` is `hip`
constexpr std::size_t kDevicePartsMin = 4096;
// total parts of a batch from which its `auto` is `wave` (`wave` where the single run's auto names `hip`: every row of
// profiles/r07_pa_cns_wave_timing.json has it 2.5x ahead).  Not the single run's 4 096: on 16 CPUs the whole program under `flat`
// is ahead at 250 parts (2.56 s against 2.79 s) and `wave` from 491 on (4.01 s against 4.34 s), 8.8 s against 12.4 s at 1 601
// (profiles/pa_cns_batch_timing.json); the two cross near 350, the constant stays on flat's side of it.
constexpr std::size_t kBatchDevicePartsMin = 400;

struct Modes {
    std::string backend, ingest;  // resolved: hip, wave, flat or host; host, flat or device
    bool chosen = false;          // `auto` named the backend
    bool onDevice() const { return backend == "hip" || backend == "wave"; }
};

// The modes of a single run of `parts` parts, or of a batch of `parts` parts in all; throws for every value and every pair that
// cannot run.  flat and device ingest hand the graph stage flat arrays, so they need a backend that takes them, and so does a
// batch; device ingest leaves the rows on the device, so it needs a backend that runs there, and its rows live in one device pool
// per file, so a batch cannot take it.  No fallback to another mode.  (None of a batch's refusals depends on `parts`.)
Modes resolveModes(bool batch, std::size_t parts) {
    const char *backendEnv = std::getenv("PA_CNS_BACKEND"), *ingestEnv = std::getenv("PA_CNS_INGEST");
    Modes m;
    m.backend = backendEnv ? backendEnv : "auto";
    m.ingest = ingestEnv ? ingestEnv : batch ? "flat" : "host";
    if (batch && m.backend == "host") throw std::runtime_error("--batch hands the graph stage flat rows, which PA_CNS_BACKEND=host does not take: flat, wave, hip or auto");
    m.chosen = m.backend == "auto";
    if (m.chosen) m.backend = batch ? (parts >= kBatchDevicePartsMin ? "wave" : "flat") : (parts >= kDevicePartsMin ? "hip" : "flat");
    if (!m.onDevice() && m.backend != "flat" && m.backend != "host") throw std::runtime_error("PA_CNS_BACKEND must be hip, wave, flat, host or auto");
    if (batch && m.ingest == "device")
        throw std::runtime_error("--batch does not take PA_CNS_INGEST=device (its rows live in one device pool per file, a group's call takes one): flat or host");
    if (m.ingest != "host" && m.ingest != "flat" && m.ingest != "device") throw std::runtime_error("PA_CNS_INGEST must be host, flat or device");
    if (m.ingest != "host" && m.backend == "host")
        throw std::runtime_error("PA_CNS_INGEST=" + m.ingest + " needs a graph backend that takes flat rows: PA_CNS_BACKEND=hip, wave or flat, not host");
    if (m.ingest == "device" && !m.onDevice())
        throw std::runtime_error("PA_CNS_INGEST=device leaves the rows on the device: it needs PA_CNS_BACKEND=hip or wave, not " + m.backend);
    return m;
}

}  // namespace
