"""PAlgorithm::walkStraight (PAlgorithm.tcc:93-170, with classifySuccessors :35-90) and graphTravel (:172-298) composed from it,
in plain Python over the successor lists of tests/succ_rule.py — the yardstick of pag_walk_straight_batch.  Sets, lists and
integers; nothing here knows about lanes, ballots or buffers.

A vertex is an id of a block of succ_rule.load_graph.  A record of a list is (target, step, grade, isEdgeSimilar().first).  A
Frame is what walkStraight's caller fixes for a group of walks: ctgRange, the split, and its parentFilter as data — the other
strand's range, two coordinate hulls (travelSequence's global ctgPosTable, graphTravel's travel one) and a set of vertices (the
callers' unique tables).  graph_travel makes one Frame per round: the travel tables as they stand when the round's walks start.

graph_travel is written over a BACKEND that answers walks and one classification, so that the same composition runs over this
rule (RuleBackend) and over the device call (tests/test_gpu_walk_straight.py): what a backend is asked is a list of walkStraight
calls per round, all under that round's frame.
"""
import gzip
import os

import numpy as np

import goldens
import succ_rule
import walk_rule
from dump_text import Mapper, kmer_code

END, BRANCH, LIMIT, LEAP = 0, 1, 2, 3
LIMIT_MAX = 65536
NONE32 = 0xFFFFFFFF
Window = walk_rule.Window  # a ctgPosTable: the hull of the coordinates added, 0 is never added


class Landing:
    """what the landing rule reads (walk_rule.landing_refused): PositionMapper's tables over the contig lengths; without
    contigs a single start, 0, and every size 0"""

    def __init__(self, ctg_len, leap_min):
        m = Mapper(ctg_len)
        self.starts, self.sizes, self.leap_min = (m.starts or [0]), m.sizes, float(leap_min)


class Frame:
    def __init__(self, ctg_left, ctg_right, rev_left=0, rev_right=0, split_size=0, leap_min=1.0, hulls=((NONE32, 0), (NONE32, 0)), excl=(), ctg_len=()):
        self.ctg_left, self.ctg_right, self.rev_left, self.rev_right = int(ctg_left), int(ctg_right), int(rev_left), int(rev_right)
        self.split_size, self.leap_min = int(split_size), float(leap_min)
        self.hulls = tuple((int(lo), int(hi)) for lo, hi in hulls)
        self.excl = frozenset(excl)
        self.ctg_len = tuple(int(x) for x in ctg_len)
        self.landing = Landing(self.ctg_len, self.leap_min)

    def leaps(self, tc):
        return tc != 0 and (tc < self.ctg_left or tc >= self.ctg_right)

    def with_travel(self, travel, hull):
        """this frame with graphTravel's tables added: the travel set joins excl, the travel hull is hull 1"""
        return Frame(self.ctg_left, self.ctg_right, self.rev_left, self.rev_right, self.split_size, self.leap_min,
                     (self.hulls[0], (hull.lo, hull.hi)), self.excl | frozenset(travel), self.ctg_len)


class Lists:
    """the successor lists of ALL vertices of a block, computed in one vectorised call and sliced; the vertices' contig
    coordinates and counts"""

    def __init__(self, g, deviation, err, counts=None):
        n = len(g["ctg"])
        self.g = g
        self.off, rec = succ_rule.successors(g, np.arange(n), deviation, err)
        self.off, self._rec = self.off.tolist(), rec
        self.ctg = g["ctg"].tolist()
        self.count = [1] * n if counts is None else [int(x) for x in counts]
        self._cache = {}

    def of(self, v):
        r = self._cache.get(v)
        if r is None:
            r = self._cache[v] = [tuple(x) for x in self._rec[self.off[v]:self.off[v + 1]].tolist()]
        return r


def kept_by_frame(L, F, rec):
    """the caller's parentFilter"""
    t, _, _, sim = rec
    tc = L.ctg[t]
    if t in F.excl:
        return False
    if tc != 0 and F.rev_left <= tc < F.rev_right:
        return False
    for lo, hi in F.hulls:
        if not (tc == 0 or sim or not (lo <= tc <= hi)):
            return False
    return True


def classify(L, F, u, can_leap, keep):
    """classifySuccessors (:35-90) over the list of u filtered by keep -> the chosen class in record order"""
    classes = ([], [], [], [])
    for rec in L.of(u):
        if not keep(rec):
            continue
        t, _, grade, _ = rec
        tc = L.ctg[t]
        leap = F.leaps(tc)
        if leap and walk_rule.landing_refused(F.landing, tc):  # :63-68
            continue
        if leap and not can_leap:                              # :70-72
            continue
        if leap or grade == succ_rule.AMAZING:
            classes[0].append(rec)
        elif grade == succ_rule.EXCELLENT:
            classes[1].append(rec)
        elif grade == succ_rule.GOOD:
            classes[2].append(rec)
        elif can_leap and grade == succ_rule.SKIP:
            classes[3].append(rec)
    for c in classes:
        if c:
            return c
    return []


def walk_straight(L, F, start, dist, has_size, limit):
    """-> (path [(vertex, step, count)], status, the chosen class of a BRANCH [(target, step, grade, ctg-similar)])"""
    assert 2 <= limit <= LIMIT_MAX
    path = [(start, dist, L.count[start])]
    now = dist
    c = L.ctg[start]
    if F.leaps(c):  # :111-114
        return path, LEAP, []
    own, hull = {start}, Window()
    hull.add(c)
    cur = start

    def keep(rec):  # :120-134
        t, _, _, sim = rec
        tc = L.ctg[t]
        return kept_by_frame(L, F, rec) and t not in own and (tc == 0 or bool(sim) or not hull.has(tc))

    while True:
        chosen = classify(L, F, cur, has_size + now >= F.split_size, keep)
        if not chosen:
            return path, END, []
        if len(chosen) > 1:
            return path, BRANCH, chosen
        t, step, _, _ = chosen[0]
        own.add(t)
        hull.add(L.ctg[t])
        path.append((t, step, L.count[t]))
        now += step
        if F.leaps(L.ctg[t]):  # :162-164
            return path, LEAP, []
        if len(path) >= limit:  # :166-168
            return path, LIMIT, []
        cur = t


class RuleBackend:
    """graph_travel's questions answered by the rule; `log` receives every walkStraight call as (frame, start, dist, has_size, limit)"""

    def __init__(self, L, log=None):
        self.L, self.log = L, log

    def coord(self, v):
        return self.L.ctg[v]

    def walks(self, F, starts, limit):
        if self.log is not None:
            self.log.extend((F, v, d, h, limit) for v, d, h in starts)
        return [walk_straight(self.L, F, v, d, h, limit)[:2] for v, d, h in starts]

    def classify(self, F, u, total):
        return [(t, s) for t, s, _, _ in classify(self.L, F, u, total >= F.split_size, lambda rec: kept_by_frame(self.L, F, rec))]


def graph_travel(B, base, start, k, has_size=0, limit=LIMIT_MAX, stop_after=None):
    """graphTravel (:172-298) from `start` under the frame `base` (its ctgRange, split, landing tables and the caller's
    parentFilter) -> [(vertex, step)].  stop_after: stop at the first round boundary with that many entries or more."""
    travel, hull = set(), Window()
    hull.add(B.coord(start))
    seq, now = [], k
    chosen = B.walks(base.with_travel(travel, hull), [(start, k, has_size + now)], limit)[0][0]
    while True:
        for v, s, _ in chosen:  # :224-230
            seq.append((v, s))
            travel.add(v)
            now += s
            hull.add(B.coord(v))
        if stop_after is not None and len(seq) >= stop_after:
            break
        last = seq[-1][0]
        if base.leaps(B.coord(last)):
            break
        F = base.with_travel(travel, hull)
        alts = B.classify(F, last, has_size + now)
        if not alts:
            break
        res = B.walks(F, [(v, s, has_size + now) for v, s in alts], limit)
        leap = [i for i, (_, st) in enumerate(res) if st == LEAP]
        tips = [i for i, (_, st) in enumerate(res) if st == END]
        branch = [i for i, (_, st) in enumerate(res) if st not in (LEAP, END)]
        if leap:
            pick = leap[0]
        elif branch:  # the most abundant first vertex, the first wins ties
            pick = branch[0]
            for i in branch[1:]:
                if res[i][0][0][2] > res[pick][0][0][2]:
                    pick = i
        else:  # the longest tip, the first wins ties
            pick = tips[0]
            for i in tips[1:]:
                if len(res[i][0]) > len(res[pick][0]):
                    pick = i
        chosen = res[pick][0]
    return seq


# ---- the goldens: counts, dumps, first-round conditions ---------------------------------------------------------------------------
def load_counts(name):
    """per config block of graph.txt.gz: the count of every P line (succ_rule.load_graph leaves it out)"""
    blocks = []
    for line in gzip.open(os.path.join(goldens.GOLDEN, name, "graph.txt.gz"), "rt"):
        if line[0] == "S":
            blocks.append([])
        elif line[0] == "P":
            blocks[-1].append(int(line.split()[3]))
    return [np.array(b, dtype=np.int64) for b in blocks]


def vertex_index(g):
    """{(code, ctg, ref): vertex id} of a block"""
    code = g["code"][g["node_of_vertex"]].tolist()
    return {(c, a, b): i for i, (c, a, b) in enumerate(zip(code, g["ctg"].tolist(), g["ref"].tolist()))}


def dumps_of(name):
    """{'B_C_O': (block, contig, contig length, [(code, ctg, ref, count, step)], k)} of a golden's path dumps (k: the length of the
    dump's k-mers, 0 for an empty dump), and the contigs' lengths by contig index, from the dumps' header lines"""
    out, lens = {}, {}
    for f, data in sorted(goldens.golden_out_files(name).items()):
        if not f.endswith(".txt") or f == "contig.txt":
            continue
        lines = data.decode().splitlines()
        b, c, _ = (int(x) for x in f[:-4].split("_"))
        n = int(lines[0].split("\t")[1])
        assert lens.setdefault(c, n) == n
        body, k = [], 0
        for ln in lines[1:]:
            head, step = ln.split("\t")[:2]
            kmer, ctg, ref, cnt = head.split(",")
            body.append((kmer_code(kmer), int(ctg), int(ref), int(cnt), int(step)))
            k = len(kmer)
        out[f[:-4]] = (b, c, n, body, k)
    assert sorted(lens) == list(range(len(lens))), "a contig without a dump: its length is not known"
    return out, [lens[c] for c in range(len(lens))]


def first_round_frame(ctg_len, contig, forward, split=0.9):
    """the frame of travelSequence's first graphTravel on a strand: both strand ranges from PositionMapper, splitSize =
    int(len * split), splitMin = 1 - split as a double, global tables empty"""
    m = Mapper(ctg_len)
    n = m.sizes[contig]
    fwd, rev = m.starts[contig], m.starts[contig] + 2 * n
    own, other = (fwd, rev) if forward else (rev, fwd)
    return Frame(own, own + n, other, other + n, int(n * split), 1 - split, ctg_len=ctg_len)


def strand_of(ctg_len, contig, body):
    """True: the dump runs on the contig's forward strand (by its first entry with a contig coordinate)"""
    m = Mapper(ctg_len)
    for _, ctg, _, _, _ in body:
        if ctg != 0:
            idx, _ = m.single_to_dual(ctg)
            assert abs(idx) - 1 == contig
            return idx > 0
    raise AssertionError("a dump without a contig coordinate")
