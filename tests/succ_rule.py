"""PABruijnGraph::successors as plain numpy over a golden's graph dump — the yardstick of pag_successors_batch for the
deviations and error rates no golden covers.

The rule (reference PAGraph/src/tools/graph/PABruijnGraph.cpp): searchSuccessors (:167-197) walks the children of the parent's
k-mer in edge order and every position of a child in position order; a pair is a successor when checkPosition (:143-165) is not
Oops.  checkPosition = isEdgeSimilar (:385-400; isPosSimilar :379-383) plus the two un-guarded ratio tests.  Positions are u32:
the differences wrap around, the ratios are f64.  Grades as the reference numbers them: Oops 0, Skip 1, Good 2, Excellent 3,
Amazing 4.

tests/golden/<case>/graph.txt.gz (oracle/ref_harness/graph_dump.cpp): per config block an S line, then per k-mer
`K code n_positions n_children`, its positions `P ctg ref count` in position order and its children `C code step` in edge order.
A vertex is (k-mer, index of the position); its id here is the running number of its P line inside the block, which is the order
of the V lines of succ.txt.gz."""
import gzip
import os

import numpy as np

import goldens

OOPS, SKIP, GOOD, EXCELLENT, AMAZING = range(5)


def load_graph(name):
    """per config block: code[n] of the k-mers in dump order, pos_off[n + 1], ctg / ref[n_pos] (uint32), child_off[n + 1],
    child_code / child_step[n_children]"""
    blocks = []
    for line in gzip.open(os.path.join(goldens.GOLDEN, name, "graph.txt.gz"), "rt"):
        t = line[0]
        if t == "S":
            blocks.append({"code": [], "npos": [], "nchild": [], "ctg": [], "ref": [], "child_code": [], "child_step": []})
            b = blocks[-1]
        elif t == "K":
            b["code"].append(int(line.split()[1]))
            b["npos"].append(0)
            b["nchild"].append(0)
        elif t == "P":
            p = line.split()
            b["ctg"].append(int(p[1]))
            b["ref"].append(int(p[2]))
            b["npos"][-1] += 1
        elif t == "C":
            p = line.split()
            b["child_code"].append(int(p[1]))
            b["child_step"].append(int(p[2]))
            b["nchild"][-1] += 1
    out = []
    for b in blocks:
        g = {"code": np.array(b["code"], dtype=np.int64), "ctg": np.array(b["ctg"], dtype=np.uint32), "ref": np.array(b["ref"], dtype=np.uint32),
             "child_code": np.array(b["child_code"], dtype=np.int64), "child_step": np.array(b["child_step"], dtype=np.uint32)}
        g["pos_off"] = np.concatenate(([0], np.cumsum(np.array(b["npos"], dtype=np.int64))))
        g["child_off"] = np.concatenate(([0], np.cumsum(np.array(b["nchild"], dtype=np.int64))))
        g["node_of_vertex"] = np.repeat(np.arange(len(g["code"])), np.diff(g["pos_off"]))
        assert len(np.unique(g["code"])) == len(g["code"])
        out.append(g)
    return out


def _ratio_ok(d, dist, err):
    """std::abs(1.0 - (d * 1.0 / dist)) <= errorRate, d a u32 difference (a step of 0 divides by zero as the reference does:
    inf or nan, never within the rate)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(1.0 - (d.astype(np.float64) * 1.0 / dist.astype(np.float64))) <= err


def _pos_similar(a, b, deviation):
    big, small = np.maximum(a, b), np.minimum(a, b)
    return (a != 0) & (b != 0) & ((big - small).astype(np.uint64) <= np.uint64(deviation))


def check_position(ac, ar, bc, br, dist, deviation, err):
    """(grade, isEdgeSimilar().first) of the pairs: parent position (ac, ar), child position (bc, br), step dist — uint32 arrays"""
    ac, ar, bc, br, dist = (np.asarray(x, dtype=np.uint32) for x in (ac, ar, bc, br, dist))
    q1, q2 = _ratio_ok(bc - ac, dist, err), _ratio_ok(br - ar, dist, err)  # (u32 arrays: the differences wrap around)
    tc = np.where(ac != 0, ac + dist, np.uint32(0)).astype(np.uint32)
    tr = np.where(ar != 0, ar + dist, np.uint32(0)).astype(np.uint32)
    e1 = _pos_similar(tc, bc, deviation) | ((ac != 0) & (bc != 0) & q1)
    e2 = _pos_similar(tr, br, deviation) | ((ar != 0) & (br != 0) & q2)
    s1, s2 = e1 | q1, e2 | q2
    no_ctg = (ac == 0) | (bc == 0)
    no_ref = (ar == 0) | (br == 0)
    g_no_ctg = np.where(s2, np.where(bc != 0, EXCELLENT, np.where(ac != 0, SKIP, GOOD)), OOPS)
    g_no_ref = np.where(s1, np.where(br != 0, EXCELLENT, GOOD), OOPS)
    g_both = np.where(s1 & s2, AMAZING, np.where(s1, EXCELLENT, np.where(s2, SKIP, OOPS)))
    return np.where(no_ctg, g_no_ctg, np.where(no_ref, g_no_ref, g_both)).astype(np.int64), e1


def candidate_pairs(g):
    """per vertex: the number of (child, position of the child) pairs searchSuccessors examines for it"""
    order = np.argsort(g["code"], kind="stable")
    at = np.searchsorted(g["code"][order], g["child_code"])
    at = np.minimum(at, len(order) - 1)
    node = np.where(g["code"][order][at] == g["child_code"], order[at], -1)
    n_pos = np.where(node >= 0, np.diff(g["pos_off"])[np.maximum(node, 0)], 0)
    run = np.concatenate(([0], np.cumsum(n_pos)))
    return (run[g["child_off"][1:]] - run[g["child_off"][:-1]])[g["node_of_vertex"]]


def successors(g, vertices, deviation, err):
    """the lists of `vertices` (ids of one block `g` of load_graph): off[len + 1] and records [n, 4] = (target vertex id, step,
    grade, isEdgeSimilar().first), in the reference's order"""
    vertices = np.asarray(vertices, dtype=np.int64)
    node = g["node_of_vertex"][vertices]
    # (vertex, child) in edge order
    n_child = g["child_off"][node + 1] - g["child_off"][node]
    owner_e = np.repeat(np.arange(len(vertices)), n_child)
    first = np.cumsum(n_child) - n_child
    e = g["child_off"][node][owner_e] + (np.arange(int(n_child.sum())) - first[owner_e])
    # the child's k-mer among the nodes (a child that is no node has no positions)
    order = np.argsort(g["code"], kind="stable")
    at = np.minimum(np.searchsorted(g["code"][order], g["child_code"][e]), len(order) - 1)
    hit = g["code"][order][at] == g["child_code"][e]
    t_node = order[at]
    n_tpos = np.where(hit, g["pos_off"][t_node + 1] - g["pos_off"][t_node], 0)
    # (vertex, child, position of the child) in position order
    owner_p = np.repeat(np.arange(len(e)), n_tpos)
    first_p = np.cumsum(n_tpos) - n_tpos
    target = g["pos_off"][t_node][owner_p] + (np.arange(int(n_tpos.sum())) - first_p[owner_p])
    src = vertices[owner_e[owner_p]]
    step = g["child_step"][e][owner_p]
    grade, esim = check_position(g["ctg"][src], g["ref"][src], g["ctg"][target], g["ref"][target], step, deviation, err)
    keep = grade != OOPS
    cnt = np.bincount(owner_e[owner_p][keep], minlength=len(vertices))
    off = np.concatenate(([0], np.cumsum(cnt))).astype(np.int64)
    rec = np.stack([target[keep], step[keep].astype(np.int64), grade[keep], esim[keep].astype(np.int64)], axis=1).reshape(-1, 4)
    return off, rec


def reference_dump(name):
    """succ.txt.gz as arrays, per config block: key [n_vertices, 2] = (k-mer code, index of the position) of the V lines, off, and
    records [n, 5] = (target code, target position index, step, grade, ctg-similar) of the T lines"""
    blocks = []
    for line in gzip.open(os.path.join(goldens.GOLDEN, name, "succ.txt.gz"), "rt"):
        p = line.split()
        if p[0] == "B":
            blocks.append({"key": [], "cnt": [], "rec": []})
            b = blocks[-1]
        elif p[0] == "V":
            b["key"].append((int(p[1]), int(p[2])))
            b["cnt"].append(int(p[3]))
        else:
            b["rec"].append(tuple(int(x) for x in p[1:6]))
    for b in blocks:
        b["key"] = np.array(b["key"], dtype=np.int64).reshape(-1, 2)
        b["off"] = np.concatenate(([0], np.cumsum(np.array(b["cnt"], dtype=np.int64))))
        b["rec"] = np.array(b["rec"], dtype=np.int64).reshape(-1, 5)
        assert b["off"][-1] == len(b["rec"])
    return blocks


def vertex_ids(g, code, j):
    """ids of the vertices (k-mer code, index of the position)"""
    order = np.argsort(g["code"], kind="stable")
    at = np.searchsorted(g["code"][order], code)
    assert np.array_equal(g["code"][order][at], code)
    return g["pos_off"][order[at]] + j
