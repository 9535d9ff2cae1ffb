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
// std::vector / std::map below (AlnGraph), host code like the reference's, what the CPU tests pin on the goldens.  `auto` (the
// default) picks `hip` from kDevicePartsMin parts on and `flat` below.
//
// Where the rows come from (PA_CNS_INGEST): `host` (the default) — readFromRefFile below, one thread, std::string, the
// restatement the CPU tests hold to the reference; `flat` — the file mapped and indexed (line_index.hpp), the headers parsed on
// a thread pool, the per-part lists sorted, cut to -k and weighted from the scores alone, and only the kept slices cut and
// gap-normalised, by csrc/hip/cns_rows.hpp on host threads, straight into the two pools; `device` — the same, the kept slices
// normalised on the device (pag_cns_normalize, csrc/hip/k_cns_rows.hip) where the graph kernels read them next.  A file with a
// record that is not regular (ingestParallel below) goes through `host`: that is where the reference's arithmetic wraps.
//
// Many backbones in one run: --batch <manifest> (runBatch at the end of this file) gathers the jobs of a manifest into groups and
// hands a group's parts to the backend in one call; every job's file and stdout lines are the single run's.
//
// What has to be reproduced beyond the arithmetic, because it decides ties:
//   * the graph is boost::adjacency_list<vecS, vecS, bidirectionalS>: out- and in-edge lists are vectors in insertion order,
//     clear_vertex() erases entries in place (order of the others kept), edge(u, v) finds the first match in u's out list,
//     add_edge() appends.  Graph below keeps exactly that: per vertex two vectors of edge ids.
//   * `_bbMap` is a std::map read with operator[]: a vertex that was never entered (enter / exit vertex) maps to vertex 0.
//   * bestPath(): float scores, `>` keeps the FIRST best out-edge; nodeScore read with operator[] (0.0f when absent).
//   * the per-part std::sort by score is unstable: the same libstdc++ std::sort with the same comparator on a proxy array
//     in the same initial order gives the same permutation.
//   * header fields are read with the same stream extractions; a malformed header yields an all-zero record that is still
//     processed (AlignmentHelper.cpp:24-40) with size_t / uint32_t wrap-around as in the reference.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include <future>
#include <iostream>
#include <map>
#include <memory>
#include <numeric>
#include <queue>
#include <sstream>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../hip/cns_graph.hpp"
#include "../hip/cns_rows.hpp"
#include "host_threads.hpp"
#include "line_index.hpp"
#include "pagraph_hip.h"
#include "seq_db.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// dagcon::Alignment + normalizeGaps (tools/cns/Alignment.hpp, Alignment.cpp:134-215)
// ---------------------------------------------------------------------------------------------------------------------
struct Aln {
    std::uint32_t tlen = 0, start = 0, end = 0;
    std::string qstr, tstr;
};

Aln normalizeGaps(const Aln &aln) {
    std::size_t len = aln.qstr.length();
    std::string qNorm, tNorm;
    qNorm.reserve(len + 100);
    tNorm.reserve(len + 100);
    std::string qstr = aln.qstr, tstr = aln.tstr;
    for (std::size_t i = 0; i < len; i++) {  // dots to dashes
        if ('.' == qstr[i]) qstr[i] = '-';
        if ('.' == tstr[i]) tstr[i] = '-';
    }
    for (std::size_t i = 0; i < len; i++) {  // mismatches to indels
        char qb = qstr[i], tb = tstr[i];
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
    // push gaps to the right, but not past the end (len - 1 wraps for an empty string exactly as in the reference: size_t)
    for (std::size_t i = 0; i < len - 1 && len != 0; i++) {
        if (tNorm[i] == '-') {
            std::size_t j = i;
            while (++j < len) {
                char c = tNorm[j];
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
                char c = qNorm[j];
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
    Aln out;
    out.start = aln.start;
    out.tlen = aln.tlen;
    for (std::size_t i = 0; i < len; i++)
        if (qNorm[i] != '-' || tNorm[i] != '-') {
            out.qstr += qNorm[i];
            out.tstr += tNorm[i];
        }
    return out;
}

// AlignData::sliceHelper (AlignData.cpp:11-34)
std::pair<std::size_t, std::size_t> sliceHelper(const std::string &tstr, std::size_t originStart, std::size_t sliceStart, std::size_t sliceEnd) {
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
    return {left, right};
}

struct ScoredAln {
    Aln aln;
    unsigned score;
};

// AlignData::readFromRefFile (AlignData.cpp:36-75) over AlignmentHelper::loadFromRefFile (align/AlignmentHelper.cpp:10-48)
std::vector<std::vector<ScoredAln>> readFromRefFile(const std::string &path, const std::string &skeleton, std::size_t partLen) {
    if (skeleton.empty()) return {};
    const std::size_t partNum = (skeleton.size() + partLen - 1) / partLen;
    std::vector<std::vector<ScoredAln>> part(partNum);
    std::ifstream in(path);
    if (!in.is_open()) return part;
    std::stringstream ss;
    std::string queryName, refName, forward, score, line1, line2, line3;
    std::size_t queryBegin = 0, queryEnd = 0, querySize = 0, refBegin = 0, refEnd = 0, refSize = 0;
    std::size_t curBegin = 0, curEnd = 0;
    std::string curScore;
    for (std::size_t lineCount = 0;; ++lineCount) {
        if (lineCount % 3 == 0) {
            if (!std::getline(in, line1)) break;
            ss.clear();
            ss.str(line1);
            ss >> queryName >> refName >> forward >> score >> queryBegin >> queryEnd >> querySize >> refBegin >> refEnd >> refSize;
            if (!ss.fail()) {
                curBegin = refBegin;
                curEnd = refEnd;
                curScore = score;
            } else {
                curBegin = curEnd = 0;
                curScore.clear();
            }
        } else if (lineCount % 3 == 1) {
            if (!std::getline(in, line2)) break;
        } else {
            if (!std::getline(in, line3)) break;
            const std::string &qstr = line2, &tstr = line3;
            const std::size_t toStart = curBegin, toEnd = curEnd;
            const int sc = std::atoi(curScore.c_str());
            const std::size_t leftPart = toStart / partLen;
            const std::size_t rightPart = std::min((toEnd - 1) / partLen, partNum - 1);
            for (std::size_t i = leftPart; i <= rightPart; ++i) {
                Aln a;
                a.start = static_cast<std::uint32_t>(i == leftPart ? toStart - leftPart * partLen + 1 : 1);
                a.end = static_cast<std::uint32_t>(i == rightPart ? toEnd - rightPart * partLen + 1 : partLen);
                a.tlen = static_cast<std::uint32_t>(partLen);
                auto slice = sliceHelper(tstr, toStart, i * partLen, std::min((i + 1) * partLen, skeleton.size()));
                // (std::string::substr throws when the start lies beyond the string, as the reference's does)
                a.qstr = qstr.substr(slice.first, slice.second - slice.first);
                a.tstr = tstr.substr(slice.first, slice.second - slice.first);
                Aln n = normalizeGaps(a);
                n.end = a.end;
                part[i].push_back(ScoredAln{std::move(n), static_cast<unsigned>(sc)});
            }
        }
    }
    return part;
}

// AlignData::weightAln (AlignData.cpp:77-104)
std::vector<std::size_t> weightAln(const std::vector<ScoredAln> &alignment, std::size_t alpha) {
    if (alignment.empty()) return {};
    unsigned maxScore = alignment[0].score, minScore = alignment[0].score;
    for (auto &a : alignment) {
        maxScore = std::max(maxScore, a.score);
        minScore = std::min(minScore, a.score);
    }
    const unsigned scoreRange = maxScore - minScore;
    std::vector<std::size_t> weights;
    weights.reserve(alignment.size());
    for (auto &a : alignment)
        weights.push_back(std::max(static_cast<std::size_t>((a.score - minScore) * 1.0 / std::max(scoreRange, 1U) * alpha), std::size_t(1)));
    return weights;
}

// ---------------------------------------------------------------------------------------------------------------------
// AlnGraphBoost (tools/cns/AlnGraphBoost.{hpp,cpp}) on plain vectors with the adjacency_list<vecS, vecS, bidirectionalS>
// edge-list semantics
// ---------------------------------------------------------------------------------------------------------------------
struct Node {
    char base = 'N';
    int coverage = 0, weight = 0;
    bool backbone = false, deleted = false;
};
struct Edge {
    std::uint32_t src, dst;
    int count = 0;
    bool visited = false;
};

class AlnGraph {
public:
    explicit AlnGraph(const std::string &backbone) {
        const std::size_t blen = backbone.length();
        nodes_.resize(blen + 2);
        out_.resize(blen + 2);
        in_.resize(blen + 2);
        for (std::size_t i = 0; i < blen + 1; i++) addEdgeRaw(static_cast<std::uint32_t>(i), static_cast<std::uint32_t>(i + 1));
        enter_ = 0;
        nodes_[enter_].base = '^';
        nodes_[enter_].backbone = true;
        for (std::size_t i = 0; i < blen; i++) {
            Node &v = nodes_[i + 1];
            v.backbone = true;
            v.weight = 1;
            v.base = backbone[i];
            bbMap_[static_cast<std::uint32_t>(i + 1)] = static_cast<std::uint32_t>(i + 1);
        }
        exit_ = static_cast<std::uint32_t>(blen + 1);
        nodes_[exit_].base = '$';
        nodes_[exit_].backbone = true;
    }

    void addAln(const Aln &aln, int weight) {
        if (weight <= 0) return;
        std::uint32_t bbPos = aln.start;
        std::uint32_t prevVtx = enter_;
        for (std::size_t i = 0; i < aln.qstr.length(); i++) {
            const char queryBase = aln.qstr[i], targetBase = aln.tstr[i];
            const std::uint32_t currVtx = bbPos;
            if (queryBase == targetBase) {  // match
                checkVertex(currVtx);
                Node &bb = nodes_[bbMap_[currVtx]];
                bb.coverage += weight;
                bb.base = targetBase;
                nodes_[currVtx].weight += weight;
                addEdge(prevVtx, currVtx, weight);
                bbPos++;
                prevVtx = currVtx;
            } else if (queryBase == '-' && targetBase != '-') {  // query deletion
                checkVertex(currVtx);
                Node &bb = nodes_[bbMap_[currVtx]];
                bb.coverage += weight;
                bb.base = targetBase;
                bbPos++;
            } else if (queryBase != '-' && targetBase == '-') {  // query insertion
                const std::uint32_t newVtx = static_cast<std::uint32_t>(nodes_.size());
                nodes_.emplace_back();
                out_.emplace_back();
                in_.emplace_back();
                nodes_[newVtx].base = queryBase;
                nodes_[newVtx].weight += weight;
                bbMap_[newVtx] = bbPos;
                addEdge(prevVtx, newVtx, weight);
                prevVtx = newVtx;
            }
        }
        addEdge(prevVtx, exit_, weight);
    }

    void mergeNodes() {
        std::queue<std::uint32_t> seedNodes;
        seedNodes.push(enter_);
        while (!seedNodes.empty()) {
            const std::uint32_t u = seedNodes.front();
            seedNodes.pop();
            mergeInNodes(u);
            mergeOutNodes(u);
            for (std::size_t x = 0; x < out_[u].size(); ++x) {
                Edge &e = edges_[out_[u][x]];
                e.visited = true;
                const std::uint32_t v = e.dst;
                int notVisited = 0;
                for (std::uint32_t ie : in_[v])
                    if (!edges_[ie].visited) notVisited++;
                if (notVisited == 0) seedNodes.push(v);
            }
        }
    }

    std::string consensus(int minWeight = 0) {
        const std::vector<Node> path = bestPath();
        std::string cns;
        int offs = 0, bestOffs = 0, length = 0, idx = 0;
        bool metWeight = false;
        for (const Node &n : path) {
            if (n.base == nodes_[enter_].base || n.base == nodes_[exit_].base) continue;
            cns += n.base;
            if (!metWeight && n.weight >= minWeight) {
                offs = idx;
                metWeight = true;
            } else if (metWeight && n.weight < minWeight) {
                if ((idx - offs) > length) {
                    bestOffs = offs;
                    length = idx - offs;
                }
                metWeight = false;
            }
            idx++;
        }
        if (metWeight && (idx - offs) > length) {
            bestOffs = offs;
            length = idx - offs;
        }
        return cns.substr(bestOffs, length);
    }

private:
    void checkVertex(std::uint32_t v) const {
        // (the reference indexes its vertex vector without a check; an alignment that runs past its part is undefined
        // behaviour there — here it is an error)
        if (v >= nodes_.size()) throw std::runtime_error("pa_cns: an alignment runs past the end of its part");
    }
    std::uint32_t addEdgeRaw(std::uint32_t u, std::uint32_t v) {  // boost::add_edge
        const std::uint32_t id = static_cast<std::uint32_t>(edges_.size());
        edges_.push_back(Edge{u, v, 0, false});
        out_[u].push_back(id);
        in_[v].push_back(id);
        return id;
    }
    void addEdge(std::uint32_t u, std::uint32_t v, int weight) {  // AlnGraphBoost::addEdge (:114-133)
        checkVertex(v);
        bool edgeExists = false;
        for (std::uint32_t ie : in_[v])
            if (edges_[ie].src == u) {
                edges_[ie].count += weight;
                edgeExists = true;
            }
        if (!edgeExists) edges_[addEdgeRaw(u, v)].count += weight;
    }
    int findEdge(std::uint32_t u, std::uint32_t v) const {  // boost::edge(u, v, g): first match in u's out-edge list
        for (std::uint32_t oe : out_[u])
            if (edges_[oe].dst == v) return static_cast<int>(oe);
        return -1;
    }
    void clearVertex(std::uint32_t n) {  // boost::clear_vertex for a bidirectional vecS graph
        for (std::uint32_t oe : out_[n]) {
            auto &lst = in_[edges_[oe].dst];
            lst.erase(std::remove_if(lst.begin(), lst.end(), [&](std::uint32_t x) { return edges_[x].src == n; }), lst.end());
        }
        for (std::uint32_t ie : in_[n]) {
            auto &lst = out_[edges_[ie].src];
            lst.erase(std::remove_if(lst.begin(), lst.end(), [&](std::uint32_t x) { return edges_[x].dst == n; }), lst.end());
        }
        out_[n].clear();
        in_[n].clear();
    }
    void markForReaper(std::uint32_t n) {
        nodes_[n].deleted = true;
        clearVertex(n);
    }

    void mergeInNodes(std::uint32_t n) {
        std::map<char, std::vector<std::uint32_t>> nodeGroups;
        for (std::uint32_t ie : in_[n]) {
            const std::uint32_t inNode = edges_[ie].src;
            if (out_[inNode].size() == 1) nodeGroups[nodes_[inNode].base].push_back(inNode);
        }
        for (auto kvp = nodeGroups.cbegin(); kvp != nodeGroups.cend(); ++kvp) {
            const std::vector<std::uint32_t> nodes = kvp->second;
            if (nodes.size() <= 1) continue;
            const std::uint32_t an = nodes[0];
            for (std::size_t x = 1; x < nodes.size(); ++x) {  // accumulate out edge information
                edges_[out_[an].front()].count += edges_[out_[nodes[x]].front()].count;
                nodes_[an].weight += nodes_[nodes[x]].weight;
            }
            for (std::size_t x = 1; x < nodes.size(); ++x) {  // accumulate in edge information, merge nodes
                const std::uint32_t m = nodes[x];
                for (std::size_t y = 0; y < in_[m].size(); ++y) {
                    const std::uint32_t ie = in_[m][y];
                    const std::uint32_t n1 = edges_[ie].src;
                    const int e = findEdge(n1, an);
                    if (e >= 0) {
                        edges_[e].count += edges_[ie].count;
                    } else {
                        const int cnt = edges_[ie].count;
                        const bool vis = edges_[ie].visited;
                        const std::uint32_t ne = addEdgeRaw(n1, an);
                        edges_[ne].count = cnt;
                        edges_[ne].visited = vis;
                    }
                }
                markForReaper(m);
            }
            mergeInNodes(an);
        }
    }
    void mergeOutNodes(std::uint32_t n) {
        std::map<char, std::vector<std::uint32_t>> nodeGroups;
        for (std::uint32_t oe : out_[n]) {
            const std::uint32_t outNode = edges_[oe].dst;
            if (in_[outNode].size() == 1) nodeGroups[nodes_[outNode].base].push_back(outNode);
        }
        for (auto kvp = nodeGroups.cbegin(); kvp != nodeGroups.cend(); ++kvp) {
            const std::vector<std::uint32_t> nodes = kvp->second;
            if (nodes.size() <= 1) continue;
            const std::uint32_t an = nodes[0];
            for (std::size_t x = 1; x < nodes.size(); ++x) {  // accumulate inner edge information
                edges_[in_[an].front()].count += edges_[in_[nodes[x]].front()].count;
                nodes_[an].weight += nodes_[nodes[x]].weight;
            }
            for (std::size_t x = 1; x < nodes.size(); ++x) {  // accumulate and merge outer edge information
                const std::uint32_t m = nodes[x];
                for (std::size_t y = 0; y < out_[m].size(); ++y) {
                    const std::uint32_t oe = out_[m][y];
                    const std::uint32_t n2 = edges_[oe].dst;
                    const int e = findEdge(an, n2);
                    if (e >= 0) {
                        edges_[e].count += edges_[oe].count;
                    } else {
                        const int cnt = edges_[oe].count;
                        const bool vis = edges_[oe].visited;
                        const std::uint32_t ne = addEdgeRaw(an, n2);
                        edges_[ne].count = cnt;
                        edges_[ne].visited = vis;
                    }
                }
                markForReaper(m);
            }
        }
    }

    std::uint32_t bbOf(std::uint32_t v) {  // _bbMap[v] (std::map::operator[]: 0 for a vertex never entered)
        return bbMap_[v];
    }

    std::vector<Node> bestPath() {
        // (edges(_g) only holds the edges that still exist; the flags of erased ones do not matter)
        for (Edge &e : edges_) e.visited = false;
        std::vector<int> bestEdge(nodes_.size(), -1);
        std::vector<float> nodeScore(nodes_.size(), 0.0f);
        std::queue<std::uint32_t> seedNodes;
        seedNodes.push(exit_);
        while (!seedNodes.empty()) {
            const std::uint32_t n = seedNodes.front();
            seedNodes.pop();
            bool bestEdgeFound = false;
            float bestScore = -FLT_MAX;
            int bestEdgeD = -1;
            for (std::uint32_t oe : out_[n]) {
                const std::uint32_t outNodeD = edges_[oe].dst;
                const Node outNode = nodes_[outNodeD];
                float newScore;
                const float score = nodeScore[outNodeD];
                if (outNode.backbone && outNode.weight == 1) {
                    newScore = score - 10.0f;
                } else {
                    const Node bbNode = nodes_[bbOf(outNodeD)];
                    newScore = edges_[oe].count - bbNode.coverage * 0.5f + score;
                }
                if (newScore > bestScore) {
                    bestScore = newScore;
                    bestEdgeD = static_cast<int>(oe);
                    bestEdgeFound = true;
                }
            }
            if (bestEdgeFound) {
                nodeScore[n] = bestScore;
                bestEdge[n] = bestEdgeD;
            }
            for (std::size_t x = 0; x < in_[n].size(); ++x) {
                Edge &inEdge = edges_[in_[n][x]];
                inEdge.visited = true;
                const std::uint32_t inNode = inEdge.src;
                int notVisited = 0;
                for (std::uint32_t oe : out_[inNode])
                    if (!edges_[oe].visited) notVisited++;
                if (notVisited == 0) seedNodes.push(inNode);
            }
        }
        std::vector<Node> bpath;
        std::uint32_t prev = enter_;
        while (true) {
            bpath.push_back(nodes_[prev]);
            if (bestEdge[prev] < 0) break;
            prev = edges_[bestEdge[prev]].dst;
        }
        return bpath;
    }

    std::vector<Node> nodes_;
    std::vector<Edge> edges_;
    std::vector<std::vector<std::uint32_t>> out_, in_;
    std::map<std::uint32_t, std::uint32_t> bbMap_;
    std::uint32_t enter_ = 0, exit_ = 0;
};

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

}  // namespace

// parts from which the default backend is the device (PA_CNS_BACKEND=auto)
constexpr std::size_t kDevicePartsMin = 4096;

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
// PA_CNS_INGEST=flat / device: the rows without readFromRefFile
// ---------------------------------------------------------------------------------------------------------------------
struct Ingested {
    std::vector<pag_cns_aln> flat;               // the kept alignments of all parts, part after part, in final (sorted) order
    std::vector<std::uint64_t> partFirst;        // part i's are flat[partFirst[i] .. partFirst[i + 1])
    std::vector<std::uint64_t> nIns, nEdgeCols;  // per part: what sizes its graph
    std::unique_ptr<char, decltype(&std::free)> qpool{nullptr, &std::free}, tpool{nullptr, &std::free};  // `flat`
    std::uint64_t poolBytes = 0;
    pag_cns_rows *dev = nullptr;                 // `device`
    double sIndex = 0, sHeaders = 0, sLists = 0, sRows = 0, sUpload = 0;
    std::uint64_t nPieces = 0, nOversize = 0;    // `device`: pieces the text went up in, slices normalised on the host after all
};

// AlignData::weightAln on the scores alone
std::vector<std::size_t> weightScores(const std::vector<unsigned> &scores, std::size_t alpha) {
    if (scores.empty()) return {};
    unsigned maxScore = scores[0], minScore = scores[0];
    for (unsigned sc : scores) {
        maxScore = std::max(maxScore, sc);
        minScore = std::min(minScore, sc);
    }
    const unsigned scoreRange = maxScore - minScore;
    std::vector<std::size_t> weights;
    weights.reserve(scores.size());
    for (unsigned sc : scores) weights.push_back(std::max(static_cast<std::size_t>((sc - minScore) * 1.0 / std::max(scoreRange, 1U) * alpha), std::size_t(1)));
    return weights;
}

// Returns false, with the reason, when a record is not REGULAR: the file then goes through readFromRefFile.  Regular: the header
// parsed, 0 < refEnd, refBegin < refEnd, both rows of the same length and under 2^31 columns, every slice at least one column.
// Everything else is where the reference's arithmetic wraps (an all-zero record after a malformed header) or where its
// behaviour is undefined (the len - 1 of an empty slice); the goldens pin the std::string code there.
bool ingestParallel(const std::string &path, const std::string &skeleton, std::size_t partLen, std::size_t topK, std::size_t alpha, HipLibrary *hip, int device,
                    Ingested &out, std::string &why) {
    using Clock = std::chrono::steady_clock;
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
    out.sIndex = lap(t);

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
    out.sHeaders = lap(t);

    // every part's list in file order, then per part the same proxy std::sort as the host ingest, the cut to -k and the weights:
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
        struct Proxy {
            unsigned score;
            std::size_t idx;
        };
        std::vector<Proxy> proxy(lst.size());
        for (std::size_t x = 0; x < lst.size(); ++x) proxy[x] = Proxy{lst[x].score, x};
        std::sort(proxy.begin(), proxy.end(), [](const Proxy &l, const Proxy &r) { return l.score > r.score; });
        std::vector<Cand> kept;
        std::vector<unsigned> scores;
        kept.reserve(std::min(lst.size(), topK));
        for (std::size_t x = 0; x < proxy.size() && x < topK; ++x) kept.push_back(lst[proxy[x].idx]);
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
    out.poolBytes = poolBytes;
    std::vector<std::vector<Cand>>().swap(lists);
    out.sLists = lap(t);

    // the rows of the kept slices
    std::vector<pag_cns_row> rows(nKept);
    if (!hip) {
        out.qpool.reset(static_cast<char *>(std::malloc(poolBytes + 64)));
        out.tpool.reset(static_cast<char *>(std::malloc(poolBytes + 64)));
        if (!out.qpool || !out.tpool) throw std::runtime_error("pa_cns: out of memory for the row pools");
        static_assert(sizeof(pag_cns_slice) == sizeof(pagrows::Slice) && sizeof(pag_cns_row) == sizeof(pagrows::Row), "pag_cns_slice / pag_cns_row are pagrows::Slice / Row");
        pagh::parallelFor(nKept, 64, [&](std::size_t s) {
            pagrows::Slice S;
            std::memcpy(&S, &slices[s], sizeof S);
            const pagrows::Row R = pagrows::run_slice(lines.base(), S, nullptr, nullptr, 1, 0, out.qpool.get(), out.tpool.get());
            std::memcpy(&rows[s], &R, sizeof R);
        });
        out.sRows = lap(t);
    } else {
        // in text order: the text goes up in pieces with their slices
        std::sort(slices.begin(), slices.end(), [](const pag_cns_slice &l, const pag_cns_slice &r) { return l.q_off != r.q_off ? l.q_off < r.q_off : l.slot < r.slot; });
        const int rc = hip->normalize(device, lines.base(), lines.bytes(), slices.data(), nKept, rows.data(), &out.dev);
        if (rc != 0) throw std::runtime_error("pag_cns_normalize failed (" + std::to_string(rc) + "): " + hip->last_error());
        hip->rows_times(out.dev, &out.sUpload, nullptr);
        hip->rows_counts(out.dev, &out.nPieces, &out.nOversize);
        out.sRows = lap(t) - out.sUpload;
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

// ---------------------------------------------------------------------------------------------------------------------
// The pieces of a run: load the backbone; ingest (ingestParallel above, or readFromRefFile + sortAndCut + flattenParts);
// size the parts; run the graphs; write the output.  main() runs them for one job, runBatch() for the jobs of a manifest.
// ---------------------------------------------------------------------------------------------------------------------
using Clock = std::chrono::steady_clock;
inline double seconds(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

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

// std::sort by score, descending, and the cut to -k: the same algorithm on a proxy array (the tie order is the library's)
void sortAndCut(std::vector<ScoredAln> &alns, std::size_t topK) {
    struct Proxy {
        unsigned score;
        std::size_t idx;
    };
    std::vector<Proxy> proxy(alns.size());
    for (std::size_t x = 0; x < alns.size(); ++x) proxy[x] = Proxy{alns[x].score, x};
    std::sort(proxy.begin(), proxy.end(), [](const Proxy &l, const Proxy &r) { return l.score > r.score; });
    std::vector<ScoredAln> sorted;
    sorted.reserve(std::min(alns.size(), topK));
    for (std::size_t x = 0; x < proxy.size() && x < topK; ++x) sorted.push_back(std::move(alns[proxy[x].idx]));
    alns.swap(sorted);
}

// The host ingest's lists as flat arrays: every alignment's two rows in two pools, and per part what sizes its graph.  (The
// lists are released as they are copied: their rows live in the pools then.)
struct HostRows {
    std::vector<pag_cns_aln> flat;
    std::vector<std::uint64_t> partFirst, nIns, nEdgeCols;
    std::string qpool, tpool;
};
void flattenParts(std::vector<std::vector<ScoredAln>> &alignments, const std::vector<std::vector<std::size_t>> &partWeights, HostRows &out) {
    const std::size_t partNum = alignments.size();
    out.partFirst.assign(partNum + 1, 0);
    out.nIns.assign(partNum, 0);
    out.nEdgeCols.assign(partNum, 0);
    for (std::size_t i = 0; i < partNum; ++i) {
        const auto &alns = alignments[i];
        for (std::size_t x = 0; x < partWeights[i].size(); ++x) {
            const Aln &a = alns[x].aln;
            pag_cns_aln f{};
            f.str_off = out.qpool.size();
            f.len = static_cast<std::uint32_t>(a.qstr.size());
            f.start = a.start;
            f.weight = static_cast<std::int32_t>(partWeights[i][x]);
            out.flat.push_back(f);
            out.qpool += a.qstr;
            out.tpool += a.tstr;
            for (std::size_t c = 0; c < a.qstr.size(); ++c) {
                const char qb = a.qstr[c], tb = a.tstr[c];
                if (qb != '-' && tb == '-') ++out.nIns[i];
                if (qb != '-') ++out.nEdgeCols[i];
            }
        }
        std::vector<ScoredAln>().swap(alignments[i]);
        out.partFirst[i + 1] = out.flat.size();
    }
}

// The parts of one backbone: the regions of every part's graph sized from its columns (include/pagraph_hip.h,
// pag_cns_consensus).  bbBase / alnBase: where the backbone and the alignments of this job start in the arrays the backend
// gets (0 for a single job).  Appends to `parts`.
void sizeParts(std::size_t bbLen, std::size_t partLen, const std::vector<std::uint64_t> &partFirst, const std::vector<std::uint64_t> &nIns,
               const std::vector<std::uint64_t> &nEdgeCols, std::uint64_t bbBase, std::uint64_t alnBase, std::vector<pag_cns_part> &parts) {
    const std::size_t partNum = (bbLen + partLen - 1) / partLen;
    for (std::size_t i = 0; i < partNum; ++i) {
        const std::size_t left = i * partLen, right = std::min((i + 1) * partLen, bbLen);
        pag_cns_part P{};
        P.bb_off = bbBase + left;
        P.bb_len = static_cast<std::uint32_t>(right - left);
        P.aln_first = alnBase + partFirst[i];
        P.n_aln = static_cast<std::uint32_t>(partFirst[i + 1] - partFirst[i]);
        const std::uint64_t nodeCap = P.bb_len + 2ull + nIns[i], edgeCap = P.bb_len + 1ull + nEdgeCols[i] + P.n_aln + 4096ull;
        if (nodeCap > 0x7FFFFFFFull || edgeCap > 0x7FFFFFFFull) throw std::runtime_error("pa_cns: a part with more than 2^31 graph slots");
        P.node_cap = static_cast<std::uint32_t>(nodeCap);
        P.edge_cap = static_cast<std::uint32_t>(edgeCap);
        P.aux_cap = static_cast<std::uint32_t>(std::min<std::uint64_t>(4 * nodeCap + 2048, 0x7FFFFFFFull));
        P.out_cap = P.node_cap;
        parts.push_back(P);
    }
}

// What a backend call gets and what it leaves: part p's consensus is buf[off[p] .. + len[p]), err[p] != 0 says why there is none
struct GraphIo {
    const char *backbone = nullptr;
    std::uint64_t backboneLen = 0;
    const std::vector<pag_cns_part> *parts = nullptr;
    const std::vector<pag_cns_aln> *flat = nullptr;
    const char *qrows = nullptr, *trows = nullptr;  // (null: the rows are on the device, in `dev`)
    std::uint64_t poolBytes = 0;
    pag_cns_rows *dev = nullptr;
    std::vector<char> buf;
    std::uint64_t outBytes = 0;  // the parts' out_cap together (buf holds 16 more)
    std::vector<std::uint64_t> off;
    std::vector<std::uint32_t> len;
    std::vector<std::int32_t> err;
    void prepare() {
        outBytes = 0;
        for (const pag_cns_part &P : *parts) outBytes += P.out_cap;
        buf.assign(outBytes + 16, 0);
        off.assign(parts->size() + 1, 0);
        len.assign(parts->size(), 0);
        err.assign(parts->size(), 0);
    }
};

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

int runBatch(const Options &opt);

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
        Backbone bb;
        if (!loadBackbone(opt.in, bb)) {
            std::cerr << "[Error] No backbone" << std::endl;
            return 2;
        }
        const std::string &name = bb.name, &backbone = bb.seq;
        const std::size_t partLen = opt.partLen;
        const std::size_t partNum = (backbone.size() + partLen - 1) / partLen;
        std::cout << "PartNum=" << partNum << std::endl;
        std::vector<std::string> consensusResults(partNum);
        const char *backendEnv = std::getenv("PA_CNS_BACKEND");
        std::string backend = backendEnv ? backendEnv : "auto";
        if (backend == "auto") backend = partNum >= kDevicePartsMin ? "hip" : "flat";
        if (backend != "hip" && backend != "wave" && backend != "flat" && backend != "host")
            throw std::runtime_error("PA_CNS_BACKEND must be hip, wave, flat, host or auto");
        const bool stageTimes = pagh::envInt("PA_CNS_STAGE_TIMES", 0) != 0;
        // Where the rows come from (the head of this file).  flat and device hand the graph stage flat arrays, so they need a
        // backend that takes them; device leaves the rows on the device, so it needs one that runs there.  No fallback to
        // another mode — but a file with a record that is not regular is read by the host ingest, whatever the mode.
        const char *ingestEnv = std::getenv("PA_CNS_INGEST");
        const std::string ingest = ingestEnv ? ingestEnv : "host";
        if (ingest != "host" && ingest != "flat" && ingest != "device") throw std::runtime_error("PA_CNS_INGEST must be host, flat or device");
        if (ingest != "host" && backend == "host")
            throw std::runtime_error("PA_CNS_INGEST=" + ingest + " needs a graph backend that takes flat rows: PA_CNS_BACKEND=hip, wave or flat, not host");
        if (ingest == "device" && backend != "hip" && backend != "wave")
            throw std::runtime_error("PA_CNS_INGEST=device leaves the rows on the device: it needs PA_CNS_BACKEND=hip or wave, not " + backend);
        const int device = static_cast<int>(pagh::envInt("PAGRAPH_DEVICE", 0));
        std::unique_ptr<HipLibrary> hip;  // (loaded when, and only when, something runs on the device)
        Ingested ing;
        bool ingested = false;
        const auto tIngest = Clock::now();
        if (ingest != "host") {
            if (ingest == "device") {
                hip.reset(new HipLibrary());
                if (hip->device_available() == 0)
                    throw std::runtime_error("PA_CNS_INGEST=device: no gfx950 device (pag_cns_normalize runs there; PA_CNS_INGEST=flat makes the rows on host threads)");
            }
            std::string why;
            ingested = ingestParallel(opt.align, backbone, partLen, opt.topK, opt.alpha, hip.get(), device, ing, why);
            if (!ingested && stageTimes) std::cerr << "pa_cns: ingest (" << ingest << ") falls back to the host ingest: " << why << std::endl;
        }
        auto alignments = ingested ? std::vector<std::vector<ScoredAln>>(partNum) : readFromRefFile(opt.align, backbone, partLen);
        const double sRead = seconds(tIngest, Clock::now());
        const char *dumpRows = std::getenv("PA_CNS_DUMP_ROWS");
        std::vector<std::string> dumpText(dumpRows ? partNum : 0);  // PA_CNS_DUMP_ROWS with the host backend: the parts' lines as they are built
        const auto dumpLine = [](std::string &to, std::size_t part, std::uint32_t start, long long weight, const char *q, const char *t, std::size_t len) {
            to += std::to_string(part) + ' ' + std::to_string(start) + ' ' + std::to_string(weight) + ' ';
            to.append(q, len);
            to += ' ';
            to.append(t, len);
            to += '\n';
        };
        std::atomic<std::size_t> consensusLen(0), next(0);
        std::atomic<bool> failed(false);
        std::string failure;
        // Where the per-part graphs are built.  hip: one device thread per part (csrc/hip/k_cns.hip); wave: a wavefront per part with
        // its lanes on the columns of an alignment and the levels of bestPath (csrc/hip/k_cns_wave.hip) — the library is loaded when,
        // and only when, a device backend runs: the program starts on a machine without the ROCm runtime; flat: the device's code
        // (csrc/hip/cns_graph.hpp) on host threads; host: the std::vector / std::map restatement.  Default: by the number of parts —
        // a part is a serial chain of dependent accesses, the device wins by running thousands side by side, host threads win on
        // the few hundred parts of one contig of the pipeline (AlignGraph2.py:503 calls pa_cns once per new contig;
        // profiles/r06_pa_cns_timing.json).  (The backend is chosen above, before the rows are read.)
        const bool onHost = backend == "host";
        // PA_CNS_STAGE_TIMES=1: the graph stage's seconds on stderr (a host clock around the backend call, which ends in a device
        // synchronise; `host` builds its graphs inside the per-part sort, so its figure holds the sort too) and, for `flat`, the
        // thread-seconds of its three phases; and the ingest's seconds by step
        const auto tSort = Clock::now();
        std::vector<std::vector<std::size_t>> partWeights(partNum);
        auto work = [&]() {
            for (std::size_t i; (i = next.fetch_add(1)) < partNum;) {
                try {
                    auto &alns = alignments[i];
                    sortAndCut(alns, opt.topK);
                    const std::size_t left = i * partLen, right = std::min((i + 1) * partLen, backbone.size());
                    partWeights[i] = weightAln(alns, opt.alpha);
                    if (!onHost) continue;  // (the graphs of all parts are built together below)
                    const auto &weights = partWeights[i];
                    if (dumpRows)
                        for (std::size_t x = 0; x < weights.size(); ++x)
                            dumpLine(dumpText[i], i, alns[x].aln.start, static_cast<std::int32_t>(weights[x]), alns[x].aln.qstr.data(), alns[x].aln.tstr.data(),
                                     alns[x].aln.qstr.size());
                    AlnGraph g(backbone.substr(left, right - left));
                    for (std::size_t x = 0; x < weights.size(); ++x) g.addAln(alns[x].aln, static_cast<int>(weights[x]));
                    g.mergeNodes();
                    consensusResults[i] = g.consensus();
                    consensusLen += consensusResults[i].size();
                    std::vector<ScoredAln>().swap(alns);
                } catch (const std::exception &e) {
                    if (!failed.exchange(true)) failure = e.what();
                }
            }
        };
        const unsigned nThreads = std::max(1u, std::min<unsigned>(std::max(1u, pagh::usableCpus()), static_cast<unsigned>(std::max<std::size_t>(1, partNum))));
        {
            std::vector<std::thread> pool;
            for (unsigned t = 1; t < nThreads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        }
        if (failed) throw std::runtime_error(failure);
        const double sSort = seconds(tSort, Clock::now());
        if (stageTimes && onHost) std::cerr << "pa_cns: graph stage (host, with the per-part sort) " << seconds(tSort, Clock::now()) << " s" << std::endl;
        // the ingest by step.  The host ingest does not split: reading, slicing and normalising are one loop (under `rows`), the
        // per-part sort and the weights come after it (under `lists`; with the host backend the graphs are built in there too)
        if (stageTimes && !ingested)
            std::cerr << "pa_cns: ingest (host) index 0 headers 0 lists " << sSort << " rows " << sRead << " upload 0" << std::endl;
        if (stageTimes && ingested)
            std::cerr << "pa_cns: ingest (" << ingest << ") index " << ing.sIndex << " headers " << ing.sHeaders << " lists " << ing.sLists << " rows " << ing.sRows
                      << " upload " << ing.sUpload << std::endl;
        if (stageTimes && ingested && ingest == "device")
            std::cerr << "pa_cns: rows on the device: " << ing.partFirst[partNum] << " slices, " << ing.nPieces << " pieces, " << ing.nOversize << " oversize" << std::endl;
        if (!onHost) {
            // the parts as flat arrays: every alignment's two rows in two pools, the regions of every part's graph sized from its
            // columns (include/pagraph_hip.h, pag_cns_consensus)
            HostRows hostRows;
            if (!ingested) flattenParts(alignments, partWeights, hostRows);  // (no list here when the rows are in the pools already)
            std::vector<pag_cns_part> parts;
            parts.reserve(partNum);
            sizeParts(backbone.size(), partLen, ingested ? ing.partFirst : hostRows.partFirst, ingested ? ing.nIns : hostRows.nIns,
                      ingested ? ing.nEdgeCols : hostRows.nEdgeCols, 0, 0, parts);
            std::vector<pag_cns_aln> flat;
            flat.swap(ingested ? ing.flat : hostRows.flat);
            const char *qrows = ingested ? ing.qpool.get() : hostRows.qpool.data(), *trows = ingested ? ing.tpool.get() : hostRows.tpool.data();  // (null: the rows are on the device)
            const std::uint64_t poolBytes = ingested ? ing.poolBytes : hostRows.qpool.size();
            if (dumpRows) {
                std::vector<char> fq, ft;
                if (ingested && ing.dev) {  // (a verification aid: the rows come back for the dump alone)
                    fq.resize(poolBytes + 1);
                    ft.resize(poolBytes + 1);
                    const int rc = hip->rows_fetch(ing.dev, fq.data(), ft.data(), poolBytes);
                    if (rc != 0) throw std::runtime_error("pag_cns_rows_fetch failed (" + std::to_string(rc) + "): " + hip->last_error());
                }
                const char *dq = ing.dev ? fq.data() : qrows, *dt = ing.dev ? ft.data() : trows;
                pagh::parallelFor(partNum, 1, [&](std::size_t i) {
                    for (std::uint64_t a = parts[i].aln_first; a < parts[i].aln_first + parts[i].n_aln; ++a)
                        dumpLine(dumpText[i], i, flat[a].start, flat[a].weight, dq + flat[a].str_off, dt + flat[a].str_off, flat[a].len);
                });
            }
            GraphIo io;
            io.backbone = backbone.data();
            io.backboneLen = backbone.size();
            io.parts = &parts;
            io.flat = &flat;
            io.qrows = qrows;
            io.trows = trows;
            io.poolBytes = poolBytes;
            io.dev = ingested ? ing.dev : nullptr;  // (the rows are where the kernels read them: no pool is uploaded)
            io.prepare();
            std::atomic<long long> phaseNs[3] = {{0}, {0}, {0}};  // flat under PA_CNS_STAGE_TIMES: add_aln, merge_nodes, best_path + trim
            auto tGraph = Clock::now();
            if (backend == "hip" || backend == "wave") {
                if (!hip) hip.reset(new HipLibrary());  // (throws when the library is missing; the call fails without a gfx950 device: there is no silent fallback)
                if (stageTimes) {  // (the HIP runtime's start and the code object's load stay out of the stage's clock)
                    (void)hip->device_available();
                    tGraph = Clock::now();
                }
                struct FreeRows {  // (the device rows are released whether the call succeeds or not)
                    HipLibrary &hip;
                    Ingested &ing;
                    ~FreeRows() {
                        if (ing.dev) hip.rows_free(ing.dev);
                        ing.dev = nullptr;
                    }
                } freeRows{*hip, ing};
                runDeviceBackend(*hip, backend == "wave", device, io);
            } else {
                runFlatBackend(io, nThreads, stageTimes, phaseNs);
            }
            if (stageTimes) {
                std::cerr << "pa_cns: graph stage (" << backend << ") " << seconds(tGraph, Clock::now()) << " s" << std::endl;
                if (backend == "flat")
                    std::cerr << "pa_cns: flat phases (thread-seconds) add_aln " << phaseNs[0] * 1e-9 << " merge_nodes " << phaseNs[1] * 1e-9 << " best_path+trim "
                              << phaseNs[2] * 1e-9 << std::endl;
            }
            for (std::size_t i = 0; i < partNum; ++i) {
                if (io.err[i]) throw std::runtime_error(partFailure(i, io.err[i]));
                consensusResults[i].assign(io.buf.data() + io.off[i], io.len[i]);
                consensusLen += io.len[i];
            }
        }
        if (dumpRows) {  // part start weight qrow trow, a line per kept alignment, parts in order, alignments in final order
            std::ofstream df(dumpRows);
            for (const std::string &t : dumpText) df << t;
            if (!df) throw std::runtime_error(std::string("PA_CNS_DUMP_ROWS: cannot write ") + dumpRows);
        }
        std::cout << consensusLen << std::endl;
        std::cout << backbone.size() << std::endl;
        std::ofstream of(opt.out);
        of << fastaText(name, backbone.size(), consensusResults);
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "pa_cns: " << e.what() << std::endl;
        return 1;
    }
}

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
// total parts of a batch from which its `auto` is `wave`.  Not the single run's 4 096: on 16 CPUs the whole program under `flat`
// is ahead at 250 parts (2.56 s against 2.79 s) and `wave` from 491 on (4.01 s against 4.34 s), 8.8 s against 12.4 s at 1 601
// (profiles/pa_cns_batch_timing.json); the two cross near 350, the constant stays on flat's side of it.
constexpr std::size_t kBatchDevicePartsMin = 400;

struct BatchJob {
    std::size_t line = 0;  // of the manifest, 1-based
    std::string in, align, out;
    Backbone bb;
    std::size_t bbLen = 0, partNum = 0;
};
// a failure of one job: what() starts with the job's backbone path
struct JobFailure : std::runtime_error {
    using std::runtime_error::runtime_error;
};

struct Group {
    std::size_t firstJob = 0, nJobs = 0;
    std::string backbone, qpool, tpool;  // the jobs' backbones and row pools, one after the other
    std::vector<pag_cns_aln> flat;
    std::vector<pag_cns_part> parts;           // by estimated cost, heaviest first
    std::vector<std::uint32_t> jobOf, partOf;  // parts[k] is part partOf[k] of job firstJob + jobOf[k]
    double sIngest = 0;
    Clock::time_point ready;
};

// the jobs from `first` on, ingested one after the other (each on all host threads) until the group closes
Group buildGroup(std::vector<BatchJob> &jobs, std::size_t first, const Options &opt, bool flatIngest, std::size_t limitParts, std::uint64_t limitBytes, bool stageTimes) {
    const auto t0 = Clock::now();
    Group g;
    g.firstJob = first;
    std::vector<pag_cns_part> parts;  // in manifest order
    std::vector<std::uint32_t> jobOf, partOf;
    for (std::size_t j = first; j < jobs.size(); ++j) {
        BatchJob &job = jobs[j];
        try {
            Ingested ing;
            HostRows host;
            bool ingested = false;
            if (flatIngest) {
                std::string why;
                ingested = ingestParallel(job.align, job.bb.seq, opt.partLen, opt.topK, opt.alpha, nullptr, 0, ing, why);
                if (!ingested && stageTimes) std::cerr << "pa_cns: ingest (flat) falls back to the host ingest for " + job.align + ": " + why + "\n";
            }
            if (!ingested) {  // a file with a record that is not regular (or PA_CNS_INGEST=host): the host ingest, for this job alone
                auto alignments = readFromRefFile(job.align, job.bb.seq, opt.partLen);
                std::vector<std::vector<std::size_t>> partWeights(job.partNum);
                pagh::parallelFor(job.partNum, 1, [&](std::size_t i) {
                    sortAndCut(alignments[i], opt.topK);
                    partWeights[i] = weightAln(alignments[i], opt.alpha);
                });
                flattenParts(alignments, partWeights, host);
            }
            const std::uint64_t bbBase = g.backbone.size(), alnBase = g.flat.size(), strBase = g.qpool.size();
            sizeParts(job.bbLen, opt.partLen, ingested ? ing.partFirst : host.partFirst, ingested ? ing.nIns : host.nIns, ingested ? ing.nEdgeCols : host.nEdgeCols, bbBase,
                      alnBase, parts);
            for (std::size_t i = 0; i < job.partNum; ++i) {
                jobOf.push_back(static_cast<std::uint32_t>(j - first));
                partOf.push_back(static_cast<std::uint32_t>(i));
            }
            const std::vector<pag_cns_aln> &flat = ingested ? ing.flat : host.flat;
            g.flat.reserve(g.flat.size() + flat.size());
            for (pag_cns_aln f : flat) {
                f.str_off += strBase;
                g.flat.push_back(f);
            }
            g.backbone += job.bb.seq;
            std::string().swap(job.bb.seq);
            if (ingested) {
                g.qpool.append(ing.qpool.get(), ing.poolBytes);
                g.tpool.append(ing.tpool.get(), ing.poolBytes);
            } else {
                g.qpool += host.qpool;
                g.tpool += host.tpool;
            }
        } catch (const std::exception &e) {
            throw JobFailure(job.in + ": " + e.what());
        }
        ++g.nJobs;
        if (parts.size() >= limitParts || g.qpool.size() + g.tpool.size() >= limitBytes) break;
    }
    // Heaviest first: the kernel's grid takes blocks in array order, and a group's run time ends with its slowest part.  The
    // estimate is the part's alignment columns plus its backbone; ties keep manifest order, then part order (the sort is stable).
    std::vector<std::uint64_t> cost(parts.size());
    for (std::size_t k = 0; k < parts.size(); ++k) {
        cost[k] = parts[k].bb_len;
        for (std::uint64_t a = parts[k].aln_first; a < parts[k].aln_first + parts[k].n_aln; ++a) cost[k] += g.flat[a].len;
    }
    std::vector<std::size_t> order(parts.size());
    std::iota(order.begin(), order.end(), std::size_t(0));
    std::stable_sort(order.begin(), order.end(), [&](std::size_t l, std::size_t r) { return cost[l] > cost[r]; });
    g.parts.reserve(parts.size());
    for (std::size_t k : order) {
        g.parts.push_back(parts[k]);
        g.jobOf.push_back(jobOf[k]);
        g.partOf.push_back(partOf[k]);
    }
    // (the kernels index the arrays by what the parts say: every range is checked here, before anything runs on them)
    for (const pag_cns_part &P : g.parts) {
        bool ok = P.bb_off + P.bb_len <= g.backbone.size() && P.aln_first + P.n_aln <= g.flat.size();
        for (std::uint64_t a = P.aln_first; ok && a < P.aln_first + P.n_aln; ++a) ok = g.flat[a].str_off + g.flat[a].len <= g.qpool.size();
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
        // what a batch cannot run under, before any work
        const char *backendEnv = std::getenv("PA_CNS_BACKEND");
        std::string backend = backendEnv ? backendEnv : "auto";
        if (backend == "host") throw std::runtime_error("--batch hands the graph stage flat rows, which PA_CNS_BACKEND=host does not take: flat, wave, hip or auto");
        if (backend != "hip" && backend != "wave" && backend != "flat" && backend != "auto") throw std::runtime_error("PA_CNS_BACKEND must be hip, wave, flat, host or auto");
        const char *ingestEnv = std::getenv("PA_CNS_INGEST");
        const std::string ingest = ingestEnv ? ingestEnv : "flat";
        if (ingest == "device")
            throw std::runtime_error("--batch does not take PA_CNS_INGEST=device (its rows live in one device pool per file, a group's call takes one): flat or host");
        if (ingest != "host" && ingest != "flat") throw std::runtime_error("PA_CNS_INGEST must be host, flat or device");
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
        const bool chosen = backend == "auto";
        // (`wave` where the single run's auto names `hip`: every row of profiles/r07_pa_cns_wave_timing.json has it 2.5x ahead)
        if (chosen) backend = totalParts >= kBatchDevicePartsMin ? "wave" : "flat";
        if (stageTimes)
            std::cerr << "pa_cns: batch of " << jobs.size() << " jobs, " << totalParts << " parts: backend " << backend << (chosen ? " (auto)" : "") << ", ingest " << ingest
                      << std::endl;
        const bool onDevice = backend != "flat";
        const int device = static_cast<int>(pagh::envInt("PAGRAPH_DEVICE", 0));
        std::unique_ptr<HipLibrary> hip;
        if (onDevice && !jobs.empty()) {
            hip.reset(new HipLibrary());       // (throws when the library is missing; the first call fails without a gfx950 device: no silent fallback)
            (void)hip->device_available();     // (the HIP runtime's start stays out of the first group's clock)
        }
        const auto build = [&](std::size_t first) { return buildGroup(jobs, first, opt, ingest == "flat", limitParts, limitBytes, stageTimes); };

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

            GraphIo io;
            io.backbone = g.backbone.data();
            io.backboneLen = g.backbone.size();
            io.parts = &g.parts;
            io.flat = &g.flat;
            io.qrows = g.qpool.data();
            io.trows = g.tpool.data();
            io.poolBytes = g.qpool.size();
            io.prepare();
            std::atomic<long long> phaseNs[3] = {{0}, {0}, {0}};
            const auto tGraph = Clock::now();
            try {
                if (onDevice) {
                    runDeviceBackend(*hip, backend == "wave", device, io);
                } else {
                    const unsigned nThreads = std::max(1u, std::min<unsigned>(std::max(1u, pagh::usableCpus()), static_cast<unsigned>(std::max<std::size_t>(1, g.parts.size()))));
                    runFlatBackend(io, nThreads, stageTimes, phaseNs);
                }
            } catch (const std::exception &e) {
                throw JobFailure(groupName + ": " + e.what());
            }
            const double sGraph = seconds(tGraph, Clock::now());
            if (stageTimes)
                std::cerr << "pa_cns: group " << gi << ": jobs " << g.nJobs << " parts " << g.parts.size() << " ingest " << g.sIngest << " s graph stage (" << backend << ") "
                          << sGraph << " s device waited " << sDeviceWaited << " s ingest waited " << sIngestWaited << " s" << std::endl;

            // back to the jobs by index; a failing part ends the run before anything of this group is written
            std::vector<std::vector<std::string>> results(g.nJobs);
            for (std::size_t j = 0; j < g.nJobs; ++j) results[j].resize(jobs[g.firstJob + j].partNum);
            std::size_t badK = SIZE_MAX;
            for (std::size_t k = 0; k < g.parts.size(); ++k) {
                if (io.err[k]) {  // (the first in manifest order, then part order)
                    if (badK == SIZE_MAX || std::make_pair(g.jobOf[k], g.partOf[k]) < std::make_pair(g.jobOf[badK], g.partOf[badK])) badK = k;
                    continue;
                }
                results[g.jobOf[k]][g.partOf[k]].assign(io.buf.data() + io.off[k], io.len[k]);
            }
            if (badK != SIZE_MAX) throw JobFailure(jobs[g.firstJob + g.jobOf[badK]].in + ": " + partFailure(g.partOf[badK], io.err[badK]));
            for (std::size_t j = 0; j < g.nJobs; ++j) {
                const BatchJob &job = jobs[g.firstJob + j];
                std::size_t consensusLen = 0;
                for (const std::string &s : results[j]) consensusLen += s.size();
                std::cout << "PartNum=" << job.partNum << std::endl;
                std::cout << consensusLen << std::endl;
                std::cout << job.bbLen << std::endl;
                std::ofstream of(job.out);
                of << fastaText(job.bb.name, job.bbLen, results[j]);
            }
        }
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "pa_cns: " << e.what() << std::endl;
        return 1;
    }
}
