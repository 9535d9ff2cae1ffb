"""CPU: tests/high_coords.py — the translation the GPU tests beyond 2^31 rest on (tests/test_gpu_high_coords.py,
tests/test_gpu_high_coords_view.py) — and the cases built with it, without a device:

  * a shift followed by the inverse shift is the identity, for every kind of thing the helper moves;
  * the lengths it hands to a PositionMapper move every strand by exactly the shift;
  * each rule's answer on a shifted graph is its answer on the graph itself, translated: succ_rule and walk_straight_rule on a
    golden graph, walk_straight_rule on the constructed cases, walk_rule on the walker cases (the iteration log with its clamp);
  * every case still lies where its shift's name says, and the `top` cases really hold sums that pass 2^32, counted."""
import numpy as np
import pytest

import high_coords as hc
import succ_rule
import view_rule
import walk_cases
import walk_rule
import walk_straight_cases as cases
import walk_straight_rule as rule
import test_gpu_high_coords as T
import test_gpu_walk as TW
from test_walk_straight_rule import CASES, constructed, golden_lists

MOVED = ("straddle", "upper")


def _same_graph(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("code", "pos_off", "ctg", "ref", "child_off", "child_code", "child_step"))


def test_a_shift_and_its_inverse_are_the_identity():
    g0 = succ_rule.load_graph("eps5_k7_repeats_t8")[0]
    for which in hc.SHIFTS:
        dc, dr = hc.deltas(which, g0["ctg"], g0["ref"])
        g = hc.shift(g0, dc, dr)
        assert (which == "low") == _same_graph(g, g0)
        assert np.array_equal(g["ctg"] == 0, g0["ctg"] == 0) and np.array_equal(g["ref"] == 0, g0["ref"] == 0), "zero stays no coordinate"
        assert _same_graph(hc.shift(g, -dc, -dr), g0)
        vpos = (g0["ctg"].astype(np.uint64) << np.uint64(32)) | g0["ref"].astype(np.uint64)
        assert np.array_equal(hc.pos(hc.pos(vpos, dc, dr), -dc, -dr), vpos)
        assert hc.name(hc.name((5, int(vpos[7])), dc, dr), -dc, -dr) == (5, int(vpos[7]))
        # the order inside a k-mer's segment is the graph's own: zero sorts first, the rest keep their order
        moved = hc.pos(vpos, dc, dr)
        inner = np.ones(len(vpos) - 1, dtype=bool)
        inner[g0["pos_off"][1:-1] - 1] = False
        assert np.array_equal((np.diff(vpos.astype(object)) > 0)[inner], (np.diff(moved.astype(object)) > 0)[inner])
        iv = np.array([0, 17, 400, 0xFFFFFFFF], dtype=np.uint32)
        assert np.array_equal(hc.intervals(hc.intervals(iv, dc), -dc), iv) and hc.intervals(iv, dc)[0] == 0 and hc.intervals(iv, dc)[3] == 0xFFFFFFFF
        kw = dict(ctg_left=1000, ctg_right=2000, rev_left=0, rev_right=0, hulls=((hc.NONE32, 0), (1600, 1699)), split_size=7)
        assert hc.frame_kwargs(hc.frame_kwargs(kw, dc), -dc) == kw and hc.frame_kwargs(kw, dc)["split_size"] == 7
    with pytest.raises(AssertionError):
        hc.shift(g0, 1 << 32, 0)  # (nothing the helper moves may reach 2^32 unless the case says it wraps)
    assert int(hc.coord(np.array([5], dtype=np.uint32), (1 << 32) - 2, wrap=True)[0]) == 3


@pytest.mark.parametrize("d", [40, (1 << 31) - 12345, 0xC0000000, 0xC0000001, 0xC0000002, 0xC0000003, 0xC0000004, 0xFFFFFFFF - 6010])
def test_leading_lengths_move_every_strand_by_the_shift(d):
    for lengths in ((1000, 500), (8400, 10050), (5,)):
        moved = hc.leading_lengths(d, lengths)
        assert len(moved) == len(lengths) + 2 and max(moved) < (1 << 32)
        assert view_rule.mapper_starts(moved)[2:] == [s + d for s in view_rule.mapper_starts(lengths)]
    assert hc.leading_lengths(0, (1000, 500)) == [1000, 500]


# ---- the golden graphs of the successor tests -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", T.CASE_TABLE)
def test_the_golden_cases_lie_where_their_shift_says(name, which):
    g, dc, dr, vcode, vpos = T.shifted(name, which)  # (asserts hc.reaches on both axes)
    lo, hi = (int(x) for x in (g["ctg"][g["ctg"] != 0].min(), g["ctg"].max()))
    assert {"low": hi < hc.TOP_BIT, "straddle": lo < hc.TOP_BIT <= hi, "upper": lo >= hc.TOP_BIT, "top": hi == hc.NONE32}[which]
    assert (which in hc.WRAP) == (which == "top"), "no more than the top cases are exempt from the translated yardstick"


@pytest.mark.parametrize("which", MOVED)
def test_succ_rule_on_a_shifted_golden_graph_is_its_answer_translated(which):
    name = "eps5_k7_repeats_t8"
    for deviation, err in T.params_of(name):
        off0, rec0 = T.rule_lists(name, "low", deviation, err)
        off, rec = T.rule_lists(name, which, deviation, err)
        assert len(rec0) > 10000 and np.array_equal(off, off0) and np.array_equal(rec, rec0)  # (records name vertices by id: the same)


def test_the_top_cases_hold_sums_that_wrap():
    """counted from the rule alone: accepted pairs whose source's contig coordinate + step passes 2^32 — and the corners the
    golden is there for survive the shift"""
    for name in T.GRAPHS:
        reach = T.reached_by_the_rule(name, "top")
        assert reach["wraps"][0] > 0, (name, reach)
        if name == "succ_corners_t8":
            assert reach["big_step"] >= 1024 and reach["positions"] > 255
    assert T.reached_by_the_rule("eps5_k7_repeats_t8", "upper")["wraps"] == (0, 0)


# ---- walk_straight_rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", hc.SHIFTS)
def test_walk_straight_cases_shifted_give_the_hand_written_answers(which):
    L, dc, dr, ctg_len, moved = T.straight(which)
    ids = constructed()[1]
    picked = T.straight_cases(which)
    if which in hc.WRAP:  # the cases without a leap, by the rule's status
        assert {c.name for c in CASES} - {c.name for c in picked} == {c.name for c in CASES if c.status == rule.LEAP} and len(picked) >= 20
    else:
        assert len(picked) == len(CASES)
    for case in picked:
        path, status, alts = rule.walk_straight(L, case.frame_of(ids, moved), ids[case.start], case.dist, case.has_size, case.limit)
        assert [v for v, _, _ in path] == [ids[v] for v in case.path] and status == case.status, (which, case.name)
        assert [t for t, _, _, _ in alts] == [ids[v] for v in case.alts], (which, case.name)


@pytest.mark.parametrize("which", MOVED)
def test_graph_travel_on_a_shifted_golden_graph_is_its_answer_translated(which):
    name, dump = "eps5_k7_repeats_t8", "0_0_1"
    dumps, ctg_len = rule.dumps_of(name)
    block, contig, n, body, k = dumps[dump]
    L0, index = golden_lists(name)[block]
    g, dc, dr, _, _ = T.shifted(name, which)
    assert block == 0
    L = rule.Lists(g, 2 * 5, 0.15, L0.count)
    b0 = rule.first_round_frame(ctg_len, contig, rule.strand_of(ctg_len, contig, body))
    kw = hc.frame_kwargs(dict(ctg_left=b0.ctg_left, ctg_right=b0.ctg_right, rev_left=b0.rev_left, rev_right=b0.rev_right), dc)
    base = rule.Frame(split_size=b0.split_size, leap_min=b0.leap_min, ctg_len=hc.leading_lengths(dc, ctg_len), **kw)
    start = index[body[0][:3]]
    want = rule.graph_travel(rule.RuleBackend(L0), b0, start, k)
    got = rule.graph_travel(rule.RuleBackend(L), base, start, k)
    assert len(want) > 1000 and got == want, f"first difference at entry {next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))}"


# ---- walk_rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", T.WALK_SHIFTS)
def test_walk_rule_on_shifted_cases_is_its_answer_translated(which):
    picked = T.walk_cases_picked(walk_cases.cases())
    assert {c.family for c in picked} == set(TW.FAMILIES)
    n_logs = clamped = 0
    for case in picked:
        G, Cg, dc = T.walk_shifted(case, which)  # (asserts hc.reaches)
        for j0 in TW._variants(case):
            j = hc.walk_job(j0, dc)
            r0, r = walk_rule.run_job(case.G, case.C, j0), walk_rule.run_job(G, Cg, j)
            for f in ("seq_v", "seq_s", "seq_len", "seq_size", "stopped", "poison", "n_main", "max_chosen", "overflow", "max_back", "max_probe"):
                assert getattr(r, f) == getattr(r0, f), (which, case.name, f)
            for f in hc.WALK_COORDS:
                assert getattr(r, f) == hc.bound(getattr(r0, f), dc), (which, case.name, f)
            assert r.seq_x == {i: hc.log_entry(x, dc) for i, x in r0.seq_x.items()}, (which, case.name)
            if j.exact:
                n_logs += len(r.seq_x)
                clamped += sum(1 for x in r.seq_x.values() if (x >> 32) & 0x7FFFFFFF == hc.LOG_NONE)
    # the log's 31-bit coordinate: below 2^31 some entries hold one, above 2^31 every entry is at the clamp
    assert n_logs >= 3 and ((clamped < n_logs) if which == "low" else (clamped == n_logs if which == "upper" else 0 < clamped))
