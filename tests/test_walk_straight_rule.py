"""CPU: tests/walk_straight_rule.py — walkStraight and graphTravel in plain Python, the yardstick of pag_walk_straight_batch —
held (a) to hand-written answers on a constructed graph, one case per line of the rule (tests/walk_straight_cases.py), and
(b) to the reference's own path dumps: graphTravel composed from the rule, run under the conditions of travelSequence's first
round from a dump's first vertex, reproduces 16 of the 22 non-empty golden dumps whole and the other 6 over all but their last
entries (where travelSequence's later rounds and tail trims act)."""
import functools

import pytest

import goldens
import succ_rule
import walk_straight_cases as cases
import walk_straight_rule as rule

# ---- (a) the constructed graph ----------------------------------------------------------------------------------------------------
BUILDER, CASES = cases.build()


@functools.lru_cache(maxsize=None)
def constructed():
    g, counts, ids = BUILDER.graph()
    return rule.Lists(g, cases.DEVIATION, cases.ERROR_RATE, counts), ids


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_constructed_case(case):
    L, ids = constructed()
    path, status, alts = rule.walk_straight(L, case.frame_of(ids), ids[case.start], case.dist, case.has_size, case.limit)
    assert [v for v, _, _ in path] == [ids[v] for v in case.path]
    assert status == case.status
    assert [t for t, _, _, _ in alts] == [ids[v] for v in case.alts]
    assert path[0][1] == case.dist and all(n == L.count[v] for v, _, n in path)
    assert (len(alts) >= 2) == (status == rule.BRANCH)


def test_the_cases_are_what_their_names_say():
    L, ids = constructed()
    grade = {(v, t): (g, sim) for v in range(len(L.ctg)) for t, _, g, sim in L.of(v)}
    pair = lambda a, b: grade[(ids[a], ids[b])]  # noqa: E731
    by_name = {c.name: c for c in CASES}
    skip = by_name["Skip kept once leaping is allowed"]
    assert pair(skip.path[0], skip.path[1]) == (succ_rule.SKIP, 0)
    exc = by_name["Amazing filtered away, Excellent decides"]
    assert pair(exc.path[0], exc.path[1])[0] == succ_rule.EXCELLENT and pair(exc.path[0], exc.frame["excl"][0])[0] == succ_rule.AMAZING
    cyc = by_name["a cycle"]
    assert pair(cyc.path[1], cyc.path[0]) == (succ_rule.AMAZING, 1), "the cycle's closing edge is no record"
    sim = by_name["ctg_similar exempts from the own hull"]
    assert pair(sim.path[2], sim.path[3])[1] == 1 and L.ctg[ids[sim.path[0]]] <= L.ctg[ids[sim.path[3]]] <= L.ctg[ids[sim.path[2]]]
    good = by_name["a target without a contig coordinate"]
    assert pair(good.path[0], good.path[1])[0] == succ_rule.GOOD
    wide = by_name["more than 64 edges, leaders and candidate pairs on the path"]
    g = L.g
    node = {v: int(g["node_of_vertex"][ids[v]]) for v in wide.path}
    assert g["child_off"][node[wide.path[1]] + 1] - g["child_off"][node[wide.path[1]]] > 64
    assert g["pos_off"][node[wide.path[2]] + 1] - g["pos_off"][node[wide.path[2]]] > 64 and wide.path[2][1] >= 64
    assert succ_rule.candidate_pairs(g)[ids[wide.path[1]]] > 64
    ex = sorted(ids[v] for v in by_name["an excl hit at the first entry"].frame["excl"])
    hit = lambda name: ex.index(L.of(ids[by_name[name].start])[0][0])  # noqa: E731
    assert (hit("an excl hit at the first entry"), hit("an excl hit at the last entry")) == (0, len(ex) - 1)
    assert 0 < hit("an excl hit at a middle entry") < len(ex) - 1


def test_graph_travel_chooses_leap_then_abundance_then_length():
    """the choice among the walks of a round (:271-294), on answers made up for it"""
    class Made:
        def __init__(self, res):
            self.res = res

        def coord(self, v):
            return 1500

        def walks(self, F, starts, limit):
            return [self.res[v] for v, _, _ in starts]

        def classify(self, F, u, total):
            return [(v, 3) for v in self.alts.pop(0)] if self.alts else []

    base = rule.Frame(1000, 2000)
    path = lambda *vs: [(v, 3, n) for v, n in vs]  # noqa: E731
    res = {0: (path((0, 1)), rule.END),
           1: (path((1, 9), (11, 1), (12, 1)), rule.END), 2: (path((2, 5)), rule.BRANCH), 3: (path((3, 7)), rule.LIMIT), 4: (path((4, 7)), rule.BRANCH),
           5: (path((5, 1)), rule.LEAP), 6: (path((6, 1), (61, 1)), rule.END), 7: (path((7, 1), (71, 1)), rule.END)}
    for alts, want in (([[1, 2, 3, 4]], 3), ([[1, 2, 5, 4]], 5), ([[1, 6, 7]], 1), ([[0, 6, 7]], 6)):
        B = Made(res)
        B.alts = [list(a) for a in alts]
        seq = rule.graph_travel(B, base, 0, 9)
        assert [v for v, _ in seq][1] == want, (alts, seq)


# ---- (b) the reference's dumps ------------------------------------------------------------------------------------------------------
# (case, dump) -> entries the first-round travel must share with the dump from its start; None: the whole dump, and nothing more
COMMON = {
    ("eps20_k11_jitter_t16", "0_0_0"): None, ("eps20_k11_jitter_t16", "0_1_0"): 729,
    ("eps5_k7_repeats_t8", "0_0_1"): None, ("eps5_k7_repeats_t8", "0_1_0"): 1316,
    ("extend_gap_t1", "0_0_0"): None, ("extend_gap_t1", "0_1_0"): None,
    ("ignore_output_t1", "0_0_0"): None, ("ignore_output_t1", "0_1_0"): None,
    ("join_fwd_t1", "0_0_0"): None, ("join_fwd_t1", "0_1_0"): None,
    ("join_rev_t16", "0_0_0"): None, ("join_rev_t16", "0_1_1"): 1437,
    ("messy_inputs_t1", "0_0_0"): None, ("messy_inputs_t1", "0_1_1"): 1479,
    ("succ_corners_t8", "0_0_0"): None, ("succ_corners_t8", "0_1_0"): None,
    ("three_ctg_multi_t4", "0_0_0"): 1088, ("three_ctg_multi_t4", "0_1_1"): None, ("three_ctg_multi_t4", "0_2_0"): None,
    ("two_blocks_both_orient_t16", "0_0_0"): None, ("two_blocks_both_orient_t16", "0_1_1"): 1460,
    ("two_blocks_both_orient_t16", "1_2_0"): None, ("two_blocks_both_orient_t16", "1_3_0"): None,
    ("two_blocks_both_orient_t16", "1_4_1"): 1333,
}
EMPTY = {("two_blocks_both_orient_t16", "1_3_1")}


@functools.lru_cache(maxsize=None)
def golden_lists(name):
    """per block: the lists of every vertex at the reference's parameters, and the vertices by (code, ctg, ref)"""
    eps = goldens.load_spec(name)["epsilon"]
    return [(rule.Lists(g, 2 * eps, 0.15, n), rule.vertex_index(g)) for g, n in zip(succ_rule.load_graph(name), rule.load_counts(name))]


def first_round_travel(name, dump, backend=None, stop_after=None):
    """(graphTravel under the first-round conditions from the dump's first vertex, the dump) as [(vertex, step)]"""
    dumps, ctg_len = rule.dumps_of(name)
    block, contig, n, body, k = dumps[dump]
    assert n == ctg_len[contig]
    L, index = golden_lists(name)[block]
    want = [(index[(c, a, r)], s) for c, a, r, _, s in body]
    base = rule.first_round_frame(ctg_len, contig, rule.strand_of(ctg_len, contig, body))
    return rule.graph_travel(backend or rule.RuleBackend(L), base, want[0][0], k, stop_after=stop_after), want


def test_the_table_names_every_dump():
    names = {n for n, _ in COMMON}
    assert names == set(n for n in goldens.case_names() if rule.dumps_of(n)[0])
    assert set(COMMON) | EMPTY == {(n, d) for n in names for d in rule.dumps_of(n)[0]}


@pytest.mark.parametrize("name,dump", sorted(COMMON), ids=[f"{n}-{d}" for n, d in sorted(COMMON)])
def test_first_round_travel_reproduces_the_dump(name, dump):
    got, want = first_round_travel(name, dump)
    need = COMMON[(name, dump)]
    common = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    print(f"{name} {dump}: dump {len(want)} entries, first-round travel {len(got)}, common prefix {common}")
    if need is None:
        assert got == want, f"{len(got)} entries for the dump's {len(want)}, common prefix {common}"
    else:
        assert common >= need, f"common prefix {common}, the rule and the dump agreed over {need}"
