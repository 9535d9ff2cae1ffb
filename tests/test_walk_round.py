"""CPU: the per-round rules of a traversal (aligngraph2_amd/csrc/hip/walk_round.hpp) on constructed values, through
tests/harness/round_test.cpp.  As in test_walk_stitch.py, the expected values come from a second restatement of every rule,
written here from the reference's text (PAGraph/src/tools/graph/PAlgorithm.cpp: filterSequence :27-44, editDistance :46-69,
appendSeq :110-142, the choice :244-265, the stop rules :280-330, the anchor :332-360, the seeds' order :400-406, "Pump it"
:409-423; position/PositionMapper.cpp:16-64), not from the C++.  The one exception is the order of the next seeds beyond 16
candidates: an unstable std::sort's permutation of ties is libstdc++'s, so there the expectation is the harness's std::sort
in the reference's own form — the edit distance computed inside the comparator — over the same initial order."""
import bisect
import collections
import ctypes as C
import math
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "harness", "bin", "libpagh_round_test.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, LIB[len(ROOT) + 1:]], check=True, capture_output=True)
    L = C.CDLL(LIB)
    P, u32, u64, i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64
    L.pagt_round_leaves.argtypes = [P, u64, u32, i64]
    L.pagt_round_choose.argtypes = [P, u64, P, u64, u32, P, P, P, P, P, i64, u64, P]
    L.pagt_round_trim.argtypes = [P, P, u64, u32, u32, u64, u32, P]
    L.pagt_round_stop.argtypes = [P, P, P, P, u64, u64, C.c_int, u64]
    L.pagt_round_anchor.argtypes = [P, u64, P, P, u64, i64, u64, P]
    L.pagt_round_candidates.argtypes = [P, u64, u64, u64, P, P]
    L.pagt_round_candidates.restype = u64
    L.pagt_round_order_seeds.argtypes = [P, u64, C.c_char_p, u32, u64, C.c_int, P]
    L.pagt_round_order_seeds.restype = u64
    L.pagt_round_pumped.argtypes = [P, u64, u32, u32, C.c_double]
    L.pagt_round_filter.argtypes = [P, u64, P, u64, C.c_int, u32, C.c_double]
    L.pagt_round_filter.restype = u64
    return L


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


class PosMapper:
    """PositionMapper.cpp:16-64.  (A position at or beyond the last start belongs to no sequence: size 0, as the library has it.)"""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        self.starts = []
        if self.sizes:
            self.starts.append(self.sizes[0])
            for i in range(1, len(self.sizes)):
                self.starts.append(self.starts[-1] + 3 * self.sizes[i - 1] + max(self.sizes[i - 1], self.sizes[i]))
            self.starts.append(self.starts[-1] + 4 * self.sizes[-1])

    def d2s(self, idx, pos):
        if idx == 0:
            return 0
        i = idx - 1 if idx > 0 else -idx - 1
        return self.starts[i] + (0 if idx > 0 else 2 * self.sizes[i]) + pos

    def s2d(self, single):
        if single == 0:
            return 0, 0
        it = bisect.bisect_right(self.starts, single)
        if it != 0:
            it -= 1
        idx, off = it, single - self.starts[it]
        sz = self.sizes[idx] if idx < len(self.sizes) else 0
        if off >= 2 * sz:
            return -(idx + 1), off - 2 * sz
        return idx + 1, off


CTGS = [1000, 800, 1200]
REFS = [5000, 3000]
CM, RM = PosMapper(CTGS), PosMapper(REFS)


# ---------------------------------------------------------------------------------------------------------------------
# the end of a chain, the choice among a round's walks
# ---------------------------------------------------------------------------------------------------------------------
def expect_choose(chains, seeds, chosenOne, min_len):
    """chains: (vertices, size, end coordinate); seeds: (ctg, ref).  PAlgorithm.cpp:244-265"""
    maxLen, chosen, leap, cpos, rpos = 0, -1, False, 0, 0
    for i, ((nv, size, end), (sc, sr)) in enumerate(zip(chains, seeds)):
        end = end if nv else 0
        leap = end != 0 and CM.s2d(end)[0] != chosenOne
        if not leap and i > 0 and min_len > 0 and size < min_len:
            continue
        if size > maxLen or leap:
            maxLen, chosen, cpos, rpos = size, i, CM.s2d(sc)[1], RM.s2d(sr)[1]
            if leap:
                break
    return chosen, leap, cpos, rpos


def choose(lib, chains, seeds, chosenOne, min_len):
    out = np.zeros(5, dtype=np.int64)
    nv, sz, end = _u64([c[0] for c in chains]), _u64([c[1] for c in chains]), _u32([c[2] for c in chains])
    sc, sr = _u32([s[0] for s in seeds]), _u32([s[1] for s in seeds])
    cl, rl = _u32(CTGS), _u32(REFS)
    lib.pagt_round_choose(cl.ctypes.data, len(CTGS), rl.ctypes.data, len(REFS), len(chains), nv.ctypes.data, sz.ctypes.data, end.ctypes.data, sc.ctypes.data,
                          sr.ctypes.data, chosenOne, min_len, out.ctypes.data)
    got = int(out[0]), bool(out[1]), int(out[2]), int(out[3])
    assert got == expect_choose(chains, seeds, chosenOne, min_len)
    if got[0] >= 0:  # (the end of a chain: its last vertex's coordinate, 0 for an empty chain)
        assert int(out[4]) == (chains[got[0]][2] if chains[got[0]][0] else 0)
    return got


def on(idx, off):
    return CM.d2s(idx, off)


def test_leaves_strand(lib):
    cl = _u32(CTGS)
    for coord, want in [(0, 0), (on(2, 0), 0), (on(2, 799), 0), (on(-2, 5), 1), (on(1, 5), 1), (on(3, 0), 1), (on(-3, 7), 1)]:
        assert lib.pagt_round_leaves(cl.ctypes.data, len(CTGS), coord, 2) == want
        assert want == int(coord != 0 and CM.s2d(coord)[0] != 2)
    assert lib.pagt_round_leaves(cl.ctypes.data, len(CTGS), on(-2, 5), -2) == 0  # (a reverse strand that is walked is its own)


def test_choose_a_short_leaping_chain_wins_and_ends_the_scan(lib):
    seeds = [(on(2, 10 + i), RM.d2s(1, 100 + i)) for i in range(5)]
    chains = [(50, 900, on(2, 700)), (40, 500, on(2, 600)), (3, 20, on(1, 40)), (90, 5000, on(2, 790)), (2, 10, on(3, 5))]
    assert choose(lib, chains, seeds, 2, 100) == (2, True, 12, 102)


def test_choose_min_len_skips_later_seeds_only(lib):
    seeds = [(on(2, 10), RM.d2s(1, 100)), (on(2, 20), RM.d2s(1, 200)), (on(2, 30), RM.d2s(1, 300))]
    chains = [(5, 50, on(2, 60)), (8, 80, on(2, 90)), (9, 99, on(2, 95))]
    assert choose(lib, chains, seeds, 2, 100) == (0, False, 10, 100)  # (chain 0 under min_len is taken, the longer later ones are not)
    assert choose(lib, chains, seeds, 2, 99) == (2, False, 30, 300)   # (99 reaches 99)
    assert choose(lib, chains, seeds, 2, 0) == (2, False, 30, 300)    # (min_len = 0 skips nothing)


def test_choose_ties_empty_chains_and_coordinate_free_ends(lib):
    seeds = [(on(2, 10), RM.d2s(1, 100)), (on(2, 20), RM.d2s(1, 200)), (on(2, 30), RM.d2s(1, 300))]
    assert choose(lib, [(5, 70, on(2, 60)), (6, 70, on(2, 61)), (7, 70, on(2, 62))], seeds, 2, 0) == (0, False, 10, 100)  # (`>` is strict)
    assert choose(lib, [(0, 0, 0)] * 3, seeds, 2, 0) == (-1, False, 0, 0)
    assert choose(lib, [(0, 0, on(1, 5))], seeds[:1], 2, 0) == (-1, False, 0, 0)  # (an empty chain has no end)
    assert choose(lib, [(4, 30, 0), (5, 40, 0)], seeds[:2], 2, 0) == (1, False, 20, 200)  # (an end without a coordinate is no leap)
    assert choose(lib, [(4, 30, on(2, 50))], seeds[:1], 2, 0) == (0, False, 10, 100)


def test_choose_leaps_and_seed_offsets_on_both_strands(lib):
    fwd = [(on(2, 10), RM.d2s(1, 100)), (on(2, 20), RM.d2s(-2, 200))]
    assert choose(lib, [(4, 30, on(2, 50)), (2, 5, on(-2, 3))], fwd, 2, 0) == (1, True, 20, 200)   # (the other strand of its own contig)
    assert choose(lib, [(4, 30, on(2, 50)), (2, 5, on(3, 3))], fwd, 2, 0) == (1, True, 20, 200)    # (another contig)
    rev = [(on(-2, 15), RM.d2s(-1, 150)), (on(-2, 25), RM.d2s(2, 250))]
    assert choose(lib, [(4, 30, on(-2, 50)), (5, 31, on(-2, 60))], rev, -2, 0) == (1, False, 25, 250)
    assert choose(lib, [(4, 30, on(2, 50)), (5, 31, on(-2, 60))], rev, -2, 0) == (0, True, 15, 150)  # (the forward strand, seen from the reverse one)


def test_choose_sweep(lib):
    rng = random.Random(5)
    for _ in range(400):
        n = rng.randint(1, 8)
        one = rng.choice([2, -2, 1])
        seeds = [(on(one, rng.randint(0, 500)), RM.d2s(rng.choice([1, -1, 2]), rng.randint(0, 900))) for _ in range(n)]
        chains = []
        for _ in range(n):
            nv = rng.choice([0, 1, 7, 30])
            end = rng.choice([0, on(one, rng.randint(0, 700)), on(one, rng.randint(0, 700)), on(-one, 4), on(3, 9)])
            chains.append((nv, rng.choice([0, 10, 50, 50, 120, 400]) if nv else 0, end))
        choose(lib, chains, seeds, one, rng.choice([0, 0, 50, 51, 200]))


# ---------------------------------------------------------------------------------------------------------------------
# appendSeq: the trim of the running path
# ---------------------------------------------------------------------------------------------------------------------
def append_seq(base, tail, k):
    """PAlgorithm.cpp:110-142 on lists of [step, coordinate]; returns dLen"""
    if not tail:
        return 0
    dLen = 0
    head = tail[0]
    dist = k
    while base and (base[-1][1] == 0 or head[1] <= base[-1][1]):
        dLen -= base[-1][0]
        base.pop()
    if base:
        dist = head[1] - base[-1][1]
    for node in tail:
        dLen += node[0]
        base.append(list(node))
    dLen -= base[len(base) - len(tail)][0] - dist
    base[len(base) - len(tail)][0] = dist
    return dLen


def trim(lib, base, tail, k):
    """the library's trim against appendSeq: what is popped, where the walk goes, its first step, the varLen increment"""
    step = np.ascontiguousarray(np.asarray([b[0] for b in base], dtype=np.int32))
    ctg = _u32([b[1] for b in base])
    out = np.zeros(5, dtype=np.int64)
    lib.pagt_round_trim(step.ctypes.data, ctg.ctypes.data, len(base), tail[0][1], k, sum(t[0] for t in tail), tail[0][0], out.ctypes.data)
    want = [list(b) for b in base]
    dLen = append_seq(want, tail, k)
    at0 = len(want) - len(tail)
    assert want[:at0] == [list(b) for b in base[:at0]]
    popped, dist, got_at0, gain, left = (int(x) for x in out)
    assert (popped, dist, got_at0, gain, left) == (sum(b[0] for b in base[at0:]), want[at0][0], at0, dLen, at0)
    return popped, dist, at0, gain


def test_trim_shapes(lib):
    k = 14
    tail = [[14, 500], [3, 503], [2, 505]]
    assert trim(lib, [], tail, k) == (0, k, 0, 14 + 3 + 2 - (14 - k))  # an empty base
    base = [[14, 400], [5, 405], [4, 409]]
    assert trim(lib, base + [[2, 0], [1, 0]], tail, k) == (3, 91, 3, 19 - 3 - (14 - 91))  # coordinate-free vertices at the end
    assert trim(lib, base + [[7, 500]], tail, k) == (7, 91, 3, 19 - 7 - (14 - 91))  # head == back: popped
    assert trim(lib, base + [[7, 499]], tail, k) == (0, 1, 4, 19 - (14 - 1))  # head == back + 1: kept
    assert trim(lib, [[14, 600], [3, 0], [2, 700]], tail, k) == (19, k, 0, 19 - 19 - (14 - k))  # popped to empty: k again
    assert trim(lib, [[14, 0], [3, 0]], tail, k) == (17, k, 0, 19 - 17)


def test_trim_sweep(lib):
    rng = random.Random(11)
    for case in range(400):
        k = rng.choice([10, 14, 16])
        n = rng.randint(0, 40)
        c, base = rng.randint(1, 50), []
        for _ in range(n):
            st = rng.randint(1, 9)
            c += st
            base.append([st, 0 if rng.random() < 0.25 else max(1, c + rng.randint(-6, 6))])
        if base:
            base[0][0] = k
        top = max([b[1] for b in base] + [1])
        head = max(1, rng.choice([top - 30, top - 3, top, top + 1, top + 5, 1, base[rng.randrange(n)][1] if n else 1]))
        tail = [[rng.randint(1, 20), head]] + [[rng.randint(1, 9), head + 1 + j] for j in range(rng.randint(0, 3))]
        trim(lib, base, tail, k)


# ---------------------------------------------------------------------------------------------------------------------
# the stop rules
# ---------------------------------------------------------------------------------------------------------------------
def expect_stop(ctgQ, refQ, cpos, rpos, leap, deviation):
    """PAlgorithm.cpp:280-330 (maxQueSize = 4); returns the queues, done, finalLeap"""
    a, b = collections.deque(ctgQ), collections.deque(refQ)
    if cpos != 0:
        a.append(cpos)
        while len(a) > 4:
            a.popleft()
    if rpos != 0:
        b.append(rpos)
        while len(b) > 4:
            b.popleft()
    ctgRepeat = len(a) >= 4 and max(a) - min(a) <= 2 * deviation
    refRepeat = len(b) >= 4 and max(b) - min(b) <= 2 * deviation
    done = ctgRepeat or refRepeat or leap
    return list(a), list(b), done, bool(done and leap)


def stop(lib, ctgQ, refQ, cpos, rpos, leap, deviation):
    a, b = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    a[:len(ctgQ)], b[:len(refQ)] = ctgQ, refQ
    na, nb = C.c_uint32(len(ctgQ)), C.c_uint32(len(refQ))
    r = lib.pagt_round_stop(a.ctypes.data, C.addressof(na), b.ctypes.data, C.addressof(nb), cpos, rpos, int(leap), deviation)
    got = [int(x) for x in a[:na.value]], [int(x) for x in b[:nb.value]], bool(r & 1), bool(r & 2)
    want = expect_stop(ctgQ, refQ, cpos, rpos, leap, deviation)
    assert got == want
    return got


def test_stop_rules(lib):
    dev = 20
    assert stop(lib, [100, 110], [500], 0, 0, False, dev) == ([100, 110], [500], False, False)  # position 0 is not pushed
    assert stop(lib, [100, 110], [], 120, 0, False, dev)[:3] == ([100, 110, 120], [], False)     # three entries: no repeat
    assert stop(lib, [100, 110, 120], [], 140, 0, False, dev)[:3] == ([100, 110, 120, 140], [], True)    # a spread of exactly 2 x deviation
    assert stop(lib, [100, 110, 120], [], 141, 0, False, dev)[:3] == ([100, 110, 120, 141], [], False)   # ... and one more
    assert stop(lib, [], [900, 910, 905], 0, 940, False, dev)[:3] == ([], [900, 910, 905, 940], True)    # either queue alone
    assert stop(lib, [100, 500, 900], [900, 910, 905], 1300, 941, False, dev)[:3] == ([100, 500, 900, 1300], [900, 910, 905, 941], False)
    assert stop(lib, [10, 500, 510, 520], [], 530, 0, False, dev)[:3] == ([500, 510, 520, 530], [], True)  # a fifth push drops the oldest
    assert stop(lib, [500, 510, 520, 530], [], 990, 0, False, dev)[:3] == ([510, 520, 530, 990], [], False)
    assert stop(lib, [], [], 100, 200, True, dev) == ([100], [200], True, True)  # a leap finishes the contig, finalLeap
    assert stop(lib, [100, 110, 120], [], 130, 0, False, dev) == ([100, 110, 120, 130], [], True, False)  # a repeat does not set it
    rng = random.Random(3)
    for _ in range(300):
        qa = [rng.randint(1, 200) for _ in range(rng.randint(0, 4))]
        qb = [rng.randint(1, 200) for _ in range(rng.randint(0, 4))]
        stop(lib, qa, qb, rng.choice([0, rng.randint(1, 200)]), rng.choice([0, rng.randint(1, 200)]), rng.random() < 0.1, rng.choice([0, 5, 40, 100]))


# ---------------------------------------------------------------------------------------------------------------------
# the next round's anchor and window, the candidates of a window request
# ---------------------------------------------------------------------------------------------------------------------
def expect_anchor(travel, chosenOne, deviation):
    """travel: (vertex, coordinate).  PAlgorithm.cpp:332-350 (flag1), and the window the seed search is given"""
    pos, u, found = 0, 0, False
    for v, c in reversed(travel):
        if c != 0:
            idx, off = CM.s2d(c)
            if idx == chosenOne and off >= 0:
                pos, u, found = off, v, True
                break
    return pos, u, found, pos - min(pos, 1000 * deviation), pos + 1000 * deviation


def anchor(lib, travel, chosenOne, deviation):
    out = np.zeros(5, dtype=np.uint64)
    cl, u, c = _u32(CTGS), _u32([t[0] for t in travel]), _u32([t[1] for t in travel])
    lib.pagt_round_anchor(cl.ctypes.data, len(CTGS), u.ctypes.data, c.ctypes.data, len(travel), chosenOne, deviation, out.ctypes.data)
    got = int(out[0]), int(out[1]), bool(out[2]), int(out[3]), int(out[4])
    assert got == expect_anchor(travel, chosenOne, deviation)
    return got


def test_anchor(lib):
    # behind the last vertex of the own strand: coordinate-free, another contig, the own contig's other strand
    travel = [(7, on(2, 100)), (8, on(2, 650)), (9, on(-2, 30)), (10, on(3, 12)), (11, 0)]
    assert anchor(lib, travel, 2, 20) == (650, 8, True, 0, 20650)           # left clamps at 0
    assert anchor(lib, travel, 2, 0) == (650, 8, True, 650, 650)
    assert anchor(lib, [(7, on(2, 100)), (8, on(2, 799))], 2, 0)[:3] == (799, 8, True)
    assert anchor(lib, travel, -2, 1) == (30, 9, True, 0, 1030)
    assert anchor(lib, [(5, on(1, 900)), (6, on(1, 950))], 1, 0)[:3] == (950, 6, True)
    assert anchor(lib, [(1, 0), (2, on(3, 5)), (3, on(-2, 9))], 2, 20) == (0, 0, False, 0, 20000)  # none found
    assert anchor(lib, [], 2, 20) == (0, 0, False, 0, 20000)
    assert anchor(lib, [(4, on(3, 1100))], 3, 1) == (1100, 4, True, 100, 2100)


def expect_candidates(reqs):
    """reqs: per request a list of parts, each the ids of one part, the parts in offset order: unique, first occurrence kept"""
    vids, cnt = [], []
    for parts in reqs:
        seen, n = set(), 0
        for part in parts:
            for v in part:
                if v not in seen:
                    seen.add(v)
                    vids.append(v)
                    n += 1
        cnt.append(n)
    return vids, cnt


def candidates(lib, reqs, parts, stride):
    words = np.full(len(reqs) * parts * stride, 0xDEAD, dtype=np.uint32)
    for q, req in enumerate(reqs):
        assert len(req) == parts
        for p, ids in enumerate(req):
            at = (q * parts + p) * stride
            words[at] = len(ids)
            words[at + 1:at + 1 + len(ids)] = ids
    vids, cnt = np.zeros(len(words) + 1, dtype=np.uint32), np.zeros(len(reqs), dtype=np.uint64)
    n = lib.pagt_round_candidates(words.ctypes.data, len(reqs), parts, stride, vids.ctypes.data, cnt.ctypes.data)
    got = [int(x) for x in vids[:n]], [int(x) for x in cnt]
    assert got == expect_candidates(reqs)
    return got


def test_window_candidates(lib):
    # an id in two parts is kept once, at its first place; a part with count 0; counts per request
    assert candidates(lib, [[[5, 9, 7], [], [9, 3, 5, 4], [4]]], 4, 8) == ([5, 9, 7, 3, 4], [5])
    assert candidates(lib, [[[5, 9], [9, 3]], [[], []], [[3, 3, 5], [9, 5, 1]]], 2, 4) == ([5, 9, 3, 3, 5, 9, 1], [3, 0, 4])
    rng = random.Random(9)
    for _ in range(50):
        parts = rng.choice([1, 3, 16])
        reqs = [[[rng.randint(0, 30) for _ in range(rng.randint(0, 7))] for _ in range(parts)] for _ in range(rng.randint(1, 3))]
        candidates(lib, reqs, parts, 8)


# ---------------------------------------------------------------------------------------------------------------------
# the order of the next round's seeds
# ---------------------------------------------------------------------------------------------------------------------
def edit_distance(a, b):
    """PAlgorithm.cpp:46-69"""
    dp = [list(range(len(b) + 1)), [0] * (len(b) + 1)]
    flag = 1
    for i in range(1, len(a) + 1):
        for j in range(len(b) + 1):
            if j == 0:
                dp[flag][j] = i
            else:
                dp[flag][j] = min(dp[flag ^ 1][j] + 1, dp[flag][j - 1] + 1)
                dp[flag][j] = min(dp[flag][j], dp[flag ^ 1][j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
        flag ^= 1
    return dp[flag ^ 1][len(b)]


def kmer_code(s):
    code = 0
    for ch in s:
        code = code << 2 | "ACGT".index(ch)
    return code


def near_kmers(rng, parent, n):
    """n k-mers at 0..3 substitutions from the parent (distances 0..3: many ties)"""
    out = []
    for _ in range(n):
        s = list(parent)
        for p in rng.sample(range(len(s)), rng.randint(0, 3)):
            s[p] = rng.choice("ACGT")
        out.append("".join(s))
    return out


def order_seeds(lib, kmers, parent, topK, reference_form):
    k = len(kmers[0]) if kmers else 14
    codes = _u32([kmer_code(s) for s in kmers])
    order = np.zeros(len(kmers) + 1, dtype=np.uint32)
    n = lib.pagt_round_order_seeds(codes.ctypes.data, len(kmers), parent.encode() if parent is not None else None, k, topK, int(reference_form),
                                   order.ctypes.data)
    return [int(x) for x in order[:n]]


@pytest.mark.parametrize("n", [0, 1, 2, 7, 16])
def test_order_seeds_small_is_the_stable_order(lib, n):
    # (libstdc++ sorts up to 16 elements by insertion: ties keep their initial order)
    rng = random.Random(100 + n)
    parent = "".join(rng.choice("ACGT") for _ in range(14))
    kmers = near_kmers(rng, parent, n)
    want = sorted(range(n), key=lambda x: edit_distance(parent, kmers[x]))
    for topK in (1, 8, n + 5):
        assert order_seeds(lib, kmers, parent, topK, False) == want[:topK]
        assert order_seeds(lib, kmers, parent, topK, True) == want[:topK]


@pytest.mark.parametrize("n", [17, 40, 200])
def test_order_seeds_precomputed_keys_permute_as_the_reference_comparator(lib, n):
    for seed in range(6):
        rng = random.Random(1000 * n + seed)
        parent = "".join(rng.choice("ACGT") for _ in range(14))
        kmers = near_kmers(rng, parent, n)
        d = [edit_distance(parent, s) for s in kmers]
        assert len(set(d)) > 1 and max(collections.Counter(d).values()) > n // 8  # (ties, and something to sort)
        for topK in (1, 8, n + 5):
            got = order_seeds(lib, kmers, parent, topK, False)
            assert got == order_seeds(lib, kmers, parent, topK, True)
            # (and what any std::sort gives: the first topK of a permutation in the distances' order)
            assert len(got) == min(n, topK) and len(set(got)) == len(got)
            assert [d[x] for x in got] == sorted(d)[:topK]


def test_order_seeds_without_a_parent(lib):
    rng = random.Random(77)
    kmers = ["".join(rng.choice("ACGT") for _ in range(14)) for _ in range(40)]
    for topK in (1, 8, 45):  # (all keys equal — the distance to the empty string is k: the order is whatever std::sort leaves)
        got = order_seeds(lib, kmers, None, topK, False)
        assert got == order_seeds(lib, kmers, "", topK, True)
        assert len(got) == min(40, topK) and len(set(got)) == len(got)
    assert order_seeds(lib, kmers[:12], None, 8, False) == list(range(8))


# ---------------------------------------------------------------------------------------------------------------------
# filterSequence, "Pump it"
# ---------------------------------------------------------------------------------------------------------------------
def expect_pumped(last_ctg, ci, startSplit):
    """PAlgorithm.cpp:413-422 (a coordinate beyond the last contig belongs to none: kept)"""
    idx, off = CM.s2d(last_ctg)
    if abs(idx) == ci + 1:
        return True
    return 1 <= abs(idx) <= len(CTGS) and off >= CTGS[abs(idx) - 1] * (1 - startSplit)


def expect_filter(ctg, finalLeap, ci, startSplit):
    """PAlgorithm.cpp:27-44 and 409-423; returns the length that is left"""
    n = len(ctg)
    if not finalLeap:
        if n < 10:
            return n
        for i in range(n - n // 90, n - 10 + 1):
            first, second = ctg[i], ctg[min(n, i + 10) - 1]
            if second != 0 and first != 0 and second < first:
                return i + 1
        return n
    return n - 1 if n and expect_pumped(ctg[-1], ci, startSplit) else n


def filt(lib, ctg, finalLeap, ci=1, startSplit=0.9):
    cl, c = _u32(CTGS), _u32(ctg)
    got = lib.pagt_round_filter(cl.ctypes.data, len(CTGS), c.ctypes.data, len(ctg), int(finalLeap), ci, startSplit)
    assert got == expect_filter(ctg, finalLeap, ci, startSplit)
    return got


def test_filter_travel_first_acts_at_900_vertices(lib):
    rising = lambda n: [1000 + 2 * x for x in range(n)]
    ctg = rising(899)
    ctg[898] = ctg[889] - 1  # (a descending last window: at n = 899 the loop does not run, startIdx = 890 = n - 9)
    assert filt(lib, ctg, False) == 899
    ctg = rising(900)
    assert filt(lib, ctg, False) == 900
    ctg[899] = ctg[890] - 1
    assert filt(lib, ctg, False) == 891
    ctg[899] = ctg[890]  # (`<` is strict)
    assert filt(lib, ctg, False) == 900
    ctg[899] = 0  # a zero at either end of the window: no cut
    assert filt(lib, ctg, False) == 900
    ctg[899], ctg[890] = 5, 0
    assert filt(lib, ctg, False) == 900
    ctg = rising(1800)  # windows 1780 .. 1790: the first hit wins
    ctg[1783 + 9] = ctg[1783] - 1
    ctg[1786 + 9] = ctg[1786] - 1
    assert filt(lib, ctg, False) == 1784
    ctg = rising(1800)
    ctg[1779 + 9] = ctg[1779] - 1  # (one before the first window: ctg[1788] closes no other window with a higher start)
    assert filt(lib, ctg, False) == 1800
    ctg = rising(1800)
    ctg[1790 + 9] = ctg[1790] - 1  # the last window
    assert filt(lib, ctg, False) == 1791
    for n in (0, 1, 9, 10, 89, 90):
        assert filt(lib, list(range(n + 5, 5, -1)), False) == n


def test_filter_travel_after_a_leap_only_pumps(lib):
    ctg = [1000 + 2 * x for x in range(900)]
    ctg[899] = on(1, 500)  # (far below ctg[890]: the window filter would cut; after a leap it is not applied)
    assert ctg[899] < ctg[890]
    assert filt(lib, ctg, True) == 899
    ctg[899] = on(1, 5)
    assert filt(lib, ctg, True) == 900
    assert filt(lib, [], True) == 0
    assert filt(lib, [on(2, 3)], True) == 0


def test_pumped(lib):
    cl = _u32(CTGS)

    def pumped(last, ci, split):
        got = bool(lib.pagt_round_pumped(cl.ctypes.data, len(CTGS), last, ci, split))
        assert got == expect_pumped(last, ci, split)
        return got

    assert pumped(on(2, 0), 1, 0.9) and pumped(on(-2, 0), 1, 0.9) and pumped(on(2, 799), 1, 0.9)  # the own contig, either strand
    # another contig: dropped from size x (1 - startSplit) on, the comparison in double
    for idx, split in [(1, 0.9), (-1, 0.9), (3, 0.9), (1, 0.7), (-3, 0.7), (1, 0.5)]:
        thr = math.ceil(CTGS[abs(idx) - 1] * (1 - split))
        assert pumped(on(idx, thr), 1, split) and not pumped(on(idx, thr - 1), 1, split)
    assert 1000 * (1 - 0.7) > 300 and not pumped(on(1, 300), 1, 0.7) and pumped(on(1, 301), 1, 0.7)  # (1 - 0.7 is above 0.3 in double)
    assert 1000 * (1 - 0.9) < 100 and pumped(on(1, 100), 1, 0.9)
    assert not pumped(CM.starts[-1] + 5, 1, 0.9) and not pumped(CM.starts[-1], 2, 0.9)  # beyond the last start: kept
