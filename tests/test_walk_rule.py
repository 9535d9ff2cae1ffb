"""CPU: tests/walk_rule.py and tests/walk_cases.py without a device — every constructed case of tests/test_gpu_walk.py reaches
the path of walk_job it is named for (asserted from the rule's counters), and the rule's choice, landing and hull-gap
functions give the paths written out here on hand-made graphs of five vertices."""
import pytest

import walk_cases as W
import walk_rule as R
from walk_cases import CL, B_START, B_SIZE, Builder

CASES = W.cases()


def test_every_family_of_the_issue_is_present():
    fam = {}
    for c in CASES:
        fam.setdefault(c.family, []).append(c.name)
    assert set(fam) == {"window", "lists", "off_strand", "leaping", "modes", "overflow", "markers", "speculation"}
    assert len(set(c.name for c in CASES)) == len(CASES)
    listed = [c for c in CASES if c.misspec]
    assert len(listed) == 1 and all(c.family == "speculation" for c in listed)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_reaches_what_it_is_named_for(case):
    walks = [R.Walk(case.G, case.C, j) for j in case.jobs]
    results = [w.run() for w in walks]
    assert case.reaches([w.cnt for w in walks], results), (case.name, [(r.seq_len, r.overflow, r.n_main) for r in results], walks[0].cnt)
    assert all(bool(r.overflow) == bool(case.overflow) for r in results)
    if case.misspec:  # a case on the list needs what the code says a mis-speculation needs
        pcs = case.G.succ["pc"]
        wide = (case.G.succ_off[1:] - case.G.succ_off[:-1]).max() > 64
        assert wide or ((pcs != 0) & ((pcs < case.C.ctg_left) | (pcs >= case.C.ctg_right))).any()


def _names(b, r):
    back = {i: n for n, i in b.ids.items()}
    return [back[v] for v in r.seq_v]


def _five(edges, pcs, ab=None, start="S", **ckw):
    b = Builder()
    for n, pc in pcs.items():
        b.v(n, pc, ab=(ab or {}).get(n, 1))
    for a, t, kw in edges:
        b.e(a, t, **kw)
    G, C = b.build(**ckw)
    w = R.Walk(G, C, R.Job(b.old[start]))
    return b, w, w.run()


E = dict(ectg=True)


def test_choice_the_most_abundant_branch_first_wins_ties():
    pcs = dict(S=CL + 10, A=CL + 20, B=CL + 30, C=CL + 40, D=CL + 50)
    edges = [("S", "A", E), ("S", "B", E), ("A", "C", E), ("A", "D", E), ("B", "C", E), ("B", "D", E)]
    b, w, r = _five(edges, pcs, ab=dict(A=3, B=5))
    assert _names(b, r) == ["S", "B", "C"]
    b, w, r = _five(edges, pcs, ab=dict(A=5, B=5))
    assert _names(b, r) == ["S", "A", "C"]
    assert r.n_main == 3 and r.max_chosen == 1 and r.seq_size == 8 + 10 + 20 and r.last_ctg == CL + 40


def test_choice_the_longest_tip_and_a_leap_before_everything():
    pcs = dict(S=CL + 10, A=CL + 20, B=CL + 30, C=CL + 40, D=CL + 50)
    edges = [("S", "A", E), ("S", "B", E), ("B", "C", E), ("C", "D", E)]
    b, w, r = _five(edges, pcs, ab=dict(A=9))
    assert _names(b, r) == ["S", "B", "C", "D"]  # (both dead ends: abundance is not asked)
    b, w, r = _five(edges[:2], pcs)
    assert _names(b, r) == ["S", "A"]            # (equal lengths: the first)
    # B lies on another contig: with leaping allowed it is taken before the branch A, without it is no successor at all
    pcs = dict(S=CL + 10, A=CL + 20, B=B_START + 5, C=CL + 40, D=CL + 50)
    edges = [("S", "A", E), ("S", "B", dict(ectg=False)), ("A", "C", E), ("A", "D", E)]
    b, w, r = _five(edges, pcs, split_size=0)
    assert _names(b, r) == ["S", "B"] and r.last_ctg == B_START + 5
    b, w, r = _five(edges, pcs)
    assert _names(b, r) == ["S", "A", "C"]


def test_landing_rule_at_its_equalities():
    C = R.Contig(CL, W.CR, starts=W.STARTS, sizes=W.SIZES, leap_min=0.8)
    edge = int(B_SIZE * 0.8)
    assert [R.landing_refused(C, B_START + o) for o in (0, edge - 1, edge, edge + 1, B_SIZE, 2 * B_SIZE - 1)] == [False, False, False, True, True, True]
    # the reverse half of the doubled space starts at offset 2 * size and is folded back: the same equality once more
    assert [R.landing_refused(C, B_START + 2 * B_SIZE + o) for o in (-1, 0, edge, edge + 1)] == [True, False, False, True]
    assert R.landing_refused(C, B_START + 4 * B_SIZE) is False       # past the last start: size 0, offset 0
    assert R.landing_refused(C, B_START + 4 * B_SIZE + 1) is True
    assert R.landing_refused(C, CL - 1) is False                     # below the first start: the difference wraps to a negative offset
    assert R.landing_refused(C, CL + 80000) is False and R.landing_refused(C, CL + 80001) is True


def test_hull_gap_a_record_between_the_two_tables_is_refused_at_the_top_level():
    pcs = dict(S=CL + 10, X=CL + 1000, Y=CL + 1001, Q=CL + 500, Z=CL + 2000)
    edges = [("S", "X", E), ("S", "Y", E), ("X", "Q", dict(ectg=False)), ("X", "Y", E), ("Q", "Z", E)]
    b, w, r = _five(edges, pcs)
    # the probe from X accepts Q (outside the travel table [S] and its own [X]) and Y, so X is a branch and beats the dead end Y;
    # with X appended the travel table is the hull [S, X], Q lies inside: Y is the one successor left
    assert _names(b, r) == ["S", "X", "Y"] and w.cnt["hull_gap"] and w.cnt["reuse"] >= 1
    edges[2] = ("X", "Q", E)  # the same record following the contig: no table applies, Q .. Z is the longer dead end
    b, w, r = _five(edges, pcs)
    assert _names(b, r) == ["S", "X", "Q", "Z"] and not w.cnt["hull_gap"]


def test_filter_key_places_a_false_positive():
    c = next(c for c in CASES if c.name == "filter_false_positive_travel")
    fw = R.DEFAULT_GEOMETRY["FILT_WORDS"]
    r = R.run_job(c.G, c.C, c.jobs[0])
    fp = r.seq_v[-2]
    members = [v for v in r.seq_v if v < c.C.in_lo and v != fp]
    word, mask = R.filt_key(fp, fw)
    got = 0
    for v in members:
        w2, m2 = R.filt_key(v, fw)
        got |= m2 if w2 == word else 0
    assert got & mask == mask and fp not in members
