// pa_cns: the restatement of the reference on std::string / std::vector / std::map, host code like the reference's and what the
// CPU tests pin on the goldens — the alignment record and its gap normalisation, the slicing of a 3-line ALN file into per-part
// lists (readFromRefFile), the score rules (which alignments of a part are kept, in which order, with which weights) and the
// partial-order alignment graph (AlnGraph).  A part of pa_cns_main.cpp, which includes it once; the head of that file says what
// has to be reproduced beyond the arithmetic.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <map>
#include <queue>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

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

// ---------------------------------------------------------------------------------------------------------------------
// The score rules: what a part keeps of its list, in which order, with which weights (pa_cns.cpp:96-104, AlignData.cpp:77-104).
// Both ingests and the host backend go through these two functions.
// ---------------------------------------------------------------------------------------------------------------------
// From a part's scores in file order: the indices of the alignments it keeps, in final order.  std::sort by score, descending,
// and the cut to -k, on a proxy array (the sort is unstable: the tie order is the library's, and decides output bytes).
std::vector<std::size_t> keptOrder(const std::vector<unsigned> &scores, std::size_t topK) {
    struct Proxy {
        unsigned score;
        std::size_t idx;
    };
    std::vector<Proxy> proxy(scores.size());
    for (std::size_t x = 0; x < scores.size(); ++x) proxy[x] = Proxy{scores[x], x};
    std::sort(proxy.begin(), proxy.end(), [](const Proxy &l, const Proxy &r) { return l.score > r.score; });
    std::vector<std::size_t> kept(std::min(scores.size(), topK));
    for (std::size_t x = 0; x < kept.size(); ++x) kept[x] = proxy[x].idx;
    return kept;
}

// AlignData::weightAln (AlignData.cpp:77-104) on the scores of the kept alignments
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

// a part's list of the host ingest, sorted and cut in place; -> the weights of what is left
std::vector<std::size_t> sortCutWeigh(std::vector<ScoredAln> &alns, std::size_t topK, std::size_t alpha) {
    std::vector<unsigned> scores(alns.size());
    for (std::size_t x = 0; x < alns.size(); ++x) scores[x] = alns[x].score;
    const std::vector<std::size_t> kept = keptOrder(scores, topK);
    std::vector<ScoredAln> sorted;
    std::vector<unsigned> keptScores;
    sorted.reserve(kept.size());
    keptScores.reserve(kept.size());
    for (std::size_t idx : kept) {
        keptScores.push_back(scores[idx]);
        sorted.push_back(std::move(alns[idx]));
    }
    alns.swap(sorted);
    return weightScores(keptScores, alpha);
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

}  // namespace
