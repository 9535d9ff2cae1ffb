"""A constructed graph (k = 9, a few dozen nodes) whose walks reach every line of the walkStraight rule, each case named for the
line it reaches, with the answer written out by hand.  tests/test_walk_straight_rule.py holds tests/walk_straight_rule.py to
these answers; tests/test_gpu_walk_straight.py holds pag_walk_straight_batch to the rule on the same cases.

Coordinates: two contigs of 1 000 and 500 bases, so PositionMapper puts contig 0 forward at [1000, 2000), reverse at [3000, 4000),
contig 1 forward at [5000, 5500), reverse at [6000, 6500).  With deviation 10 and error rate 0.15 an edge of step 20 whose target
lies exactly 20 further in both coordinates is Amazing; a target whose contig coordinate is 200 off is Skip, one whose reference
coordinate is 300 off is Excellent (succ_rule.check_position)."""
import numpy as np

from walk_straight_rule import BRANCH, END, LEAP, LIMIT, NONE32, Frame

K, DEVIATION, ERROR_RATE = 9, 10, 0.15
CTG_LEN = (1000, 500)
NEVER = 10 ** 9  # a split size no walk reaches: leaping is not allowed


class Builder:
    """nodes in ascending code: code -> positions [(ctg, ref, count)] and edges [(target code, step)]; a vertex is named (code, index
    of the position)"""

    def __init__(self):
        self.nodes, self.code = {}, 1000

    def node(self, positions):
        self.code += 7
        self.nodes[self.code] = {"pos": list(positions), "edges": []}
        return self.code

    def v(self, ctg, ref, count=1):
        return (self.node([(ctg, ref, count)]), 0)

    def absent(self):
        """a k-mer the graph does not hold"""
        self.code += 7
        return self.code

    def edge(self, a, b, step=20):
        self.nodes[a[0] if isinstance(a, tuple) else a]["edges"].append((b[0] if isinstance(b, tuple) else b, step))

    def chain(self, n, ctg, ref, step=20):
        vs = [self.v(ctg + step * i if ctg else 0, ref + step * i, count=i + 1) for i in range(n)]
        for a, c in zip(vs, vs[1:]):
            self.edge(a, c, step)
        return vs

    def graph(self):
        """-> (the graph in succ_rule's form, counts by vertex id, {vertex name: id})"""
        codes = sorted(self.nodes)
        npos = [len(self.nodes[c]["pos"]) for c in codes]
        pos_off = np.concatenate(([0], np.cumsum(npos))).astype(np.int64)
        flat = [p for c in codes for p in self.nodes[c]["pos"]]
        edges = [e for c in codes for e in self.nodes[c]["edges"]]
        g = {"code": np.array(codes, dtype=np.int64), "pos_off": pos_off, "ctg": np.array([p[0] for p in flat], dtype=np.uint32),
             "ref": np.array([p[1] for p in flat], dtype=np.uint32),
             "child_off": np.concatenate(([0], np.cumsum([len(self.nodes[c]["edges"]) for c in codes]))).astype(np.int64),
             "child_code": np.array([e[0] for e in edges], dtype=np.int64), "child_step": np.array([e[1] for e in edges], dtype=np.uint32),
             "node_of_vertex": np.repeat(np.arange(len(codes)), npos)}
        ids = {(c, j): int(pos_off[i]) + j for i, c in enumerate(codes) for j in range(npos[i])}
        return g, np.array([p[2] for p in flat], dtype=np.int64), ids


class Case:
    def __init__(self, name, start, path, status, alts=(), dist=K, has_size=0, limit=64, **frame):
        self.name, self.start, self.path, self.status, self.alts = name, start, list(path), status, list(alts)
        self.dist, self.has_size, self.limit, self.frame = dist, has_size, limit, frame

    def frame_of(self, ids, moved=None):
        """moved: the frame's keyword arguments translated along the coordinate axis (tests/high_coords.py)"""
        kw = dict(ctg_left=1000, ctg_right=2000, rev_left=3000, rev_right=4000, split_size=NEVER, leap_min=1 - 0.9, ctg_len=CTG_LEN)
        kw.update(self.frame)
        kw["excl"] = [ids[v] for v in kw.get("excl", ())]
        return Frame(**(moved(kw) if moved else kw))


def build():
    """-> (Builder, [Case])"""
    b, cases = Builder(), []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))  # noqa: E731

    # :111-114 — the start's own coordinate lies outside ctgRange
    s = b.v(5100, 9000)
    b.edge(s, b.v(5120, 9020))
    add("start already a leap", s, [s], LEAP, split_size=0)

    # :60-68 — the landing rule: 400 bases into contig 1 is beyond 500 * 0.1, 10 bases is not, on either strand
    a1, far = b.v(1500, 10000), b.v(5400, 10020)
    b.edge(a1, far)
    add("a refused landing", a1, [a1], END, split_size=0)
    a2, near = b.v(1500, 11000), b.v(5010, 11020)
    b.edge(a2, near)
    add("an accepted landing", a2, [a2, near], LEAP, split_size=0)
    add("a leap before the split size is dropped", a2, [a2], END)
    a3, near_rev = b.v(1500, 12000), b.v(6010, 12020)
    b.edge(a3, near_rev)
    add("an accepted landing on a reverse strand", a3, [a3, near_rev], LEAP, split_size=0)

    # :141 — has_size + now crosses split_size in mid-walk: now is 9 + 20 j at c[j]; c[2] and c[4] have a leaping edge besides the chain's
    c = b.chain(6, 1100, 30000)
    l2, l4 = b.v(5010, 30060), b.v(5020, 30100)
    b.edge(c[2], l2)
    b.edge(c[4], l4)
    add("the split size reached exactly at the third vertex", c[0], c[:3], BRANCH, [c[3], l2], split_size=49)
    add("the split size reached one step later", c[0], c[:5], BRANCH, [c[5], l4], split_size=50)
    add("has_size counts towards the split size", c[0], c[:3], BRANCH, [c[3], l2], split_size=50, has_size=1)
    add("the split size never reached", c[0], c, END)

    # :80 — Skip is a class only once leaping is allowed
    s4, t4 = b.v(1600, 40000), b.v(1800, 40020)
    b.edge(s4, t4)
    add("Skip dropped before the split size", s4, [s4], END)
    add("Skip kept once leaping is allowed", s4, [s4, t4], END, split_size=0)

    # :85 — the first non-empty class: Amazing filtered away, Excellent decides
    u, x, y = b.v(1200, 50000), b.v(1220, 50020), b.v(1221, 50320)
    b.edge(u, x)
    b.edge(u, y)
    add("Amazing decides", u, [u, x], END)
    add("Amazing filtered away, Excellent decides", u, [u, y], END, excl=[x])

    # :125 — a cycle: the only successor is on the path
    a, bb = b.v(1300, 60000), b.v(1305, 60005)
    b.edge(a, bb, 5)
    b.edge(bb, a, 5)
    add("a cycle", a, [a, bb], END)

    # :127-133 — the own hull refuses a coordinate inside it unless the edge follows the contig
    p = b.chain(3, 1400, 70000)
    b.edge(p[2], b.v(1410, 70060))
    add("own-hull refusal", p[0], p, END, split_size=0)
    pq = b.chain(3, 1400, 71000)
    z = b.v(1390, 71060)
    b.edge(pq[2], z)
    add("outside the own hull", pq[0], pq + [z], END, split_size=0)
    pr = b.chain(3, 1400, 72000)
    w = b.v(1436, 72045)
    b.edge(pr[2], w, 5)
    add("ctg_similar exempts from the own hull", pr[0], pr + [w], END)

    # a target without a contig coordinate passes every hull
    s8, t8 = b.v(0, 80000), b.v(0, 80020)
    b.edge(s8, t8)
    add("a target without a contig coordinate", s8, [s8, t8], END, hulls=((1, NONE32), (1, NONE32)))

    # the frame's hulls
    s9, t9 = b.v(1600, 90000), b.v(1700, 90020)
    b.edge(s9, t9)
    add("a hit in frame hull 0", s9, [s9], END, split_size=0, hulls=((1690, 1710), (NONE32, 0)))
    add("a hit in frame hull 1", s9, [s9], END, split_size=0, hulls=((NONE32, 0), (1700, 1700)))
    add("beside both frame hulls", s9, [s9, t9], END, split_size=0, hulls=((1701, 1800), (1600, 1699)))

    # the other strand
    s10, t10 = b.v(1900, 100000), b.v(3050, 100020)
    b.edge(s10, t10)
    add("a hit in the rev range", s10, [s10], END, split_size=0)
    add("no rev range", s10, [s10, t10], LEAP, split_size=0, rev_left=0, rev_right=0)

    # the excl slice: its first, a middle and its last entry; an entry with the successor's k-mer at another position is no hit
    ss = [b.v(1200 + 10 * i, 110000 + 1000 * i) for i in range(5)]
    t_first = b.v(1220, 110020)
    o1 = b.v(1999, 5)
    t_mid = b.v(1230, 111020)
    o2 = b.v(1998, 6)
    two = b.node([(1240, 112020, 3), (1240, 119999, 4)])
    t_last = b.v(1250, 113020)
    t_free = b.v(1260, 114020)
    for s_, t_ in zip(ss, (t_first, t_mid, (two, 0), t_last, t_free)):
        b.edge(s_, t_)
    excl = [t_first, o1, t_mid, o2, (two, 1), t_last]
    add("an excl hit at the first entry", ss[0], [ss[0]], END, excl=excl)
    add("an excl hit at a middle entry", ss[1], [ss[1]], END, excl=excl)
    add("the k-mer in excl at another position", ss[2], [ss[2], (two, 0)], END, excl=excl)
    add("an excl hit at the last entry", ss[3], [ss[3]], END, excl=excl)
    add("beside excl", ss[4], [ss[4], t_free], END, excl=excl)

    # :162-168 — the limit, and the leap that wins over it
    add("limit 2", c[0], c[:2], LIMIT, limit=2)
    add("limit 3", c[0], c[:3], LIMIT, limit=3)
    add("limit reached on the step that leaps", a2, [a2, near], LEAP, split_size=0, limit=2)
    add("an alternative's step as dist", c[1], c[1:3], BRANCH, [c[3], l2], dist=20, split_size=40)

    # the list loops turn: a k-mer of 70 edges (the chain's is the 68th), a k-mer of 70 leaders (the chain's is the last), and so
    # more than 64 candidate pairs in the second turn of the edges
    w0 = b.v(1100, 200000, 5)
    many_edges = b.node([(1120, 200020, 6)])
    others = [b.v(1500 + i, 150000 + i) for i in range(4)]
    many_leaders = b.node([(0, 100 + j, 1) for j in range(69)] + [(1140, 200040, 7)])
    w3 = b.v(1160, 200060, 8)
    b.edge(w0, many_edges)
    for i in range(70):
        b.edge(many_edges, many_leaders if i == 67 else (others[i % 4] if i % 3 == 0 else b.absent()), 20 if i == 67 else 1 + i)
    b.edge(many_leaders, w3)
    wide = [w0, (many_edges, 0), (many_leaders, 69), w3]
    add("more than 64 edges, leaders and candidate pairs on the path", w0, wide, END)
    add("a start beyond its k-mer's first 64 leaders", (many_leaders, 69), wide[2:], END)
    return b, cases
