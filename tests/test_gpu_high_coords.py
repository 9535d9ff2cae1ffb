"""GPU: the traversal kernels at coordinates beyond 2^31.

Every coordinate is a u32 single coordinate and a human-sized reference reaches past 2^31, but no golden does.  These tests move
small graphs the suite already trusts up the coordinate axis (tests/high_coords.py: `low` the control, `straddle` with the
middle vertex on 2^31, `upper` + 0xC0000000, `top` with the largest coordinate on 2^32 - 1) and hold each kernel, through the
hooks it already has, to two yardsticks, both exactly:

  1. the numpy rule evaluated on the shifted arrays (all four shifts);
  2. the device's own answer on the unshifted graph with the constant added back (`straddle` and `upper`; `top` is a wrap case —
     a step from its largest coordinate passes 2^32 — and is exempt, and nothing else is).

  A. pag_successors_batch (k_succ_query.hip, query_graph.hpp): every vertex's list of two golden graphs, imported shifted;
  B. the successor stage and the coordinate order (k5_succ.hip, k5_view.hip k_order_*): pag_travel_prepare on the same imports,
     the new ids in ascending unsigned contig coordinate, every record and what it says about its target, however the records
     are built (PAG_SUCC_HEAVY) and the order is applied (PAG_ORDER_SLICES); the contig and reference lengths handed over
     describe the shifted layout (two leading sequences, never walked: high_coords.leading_lengths);
  D. pag_walk_straight_batch (k_walk_query.hip): every case of tests/walk_straight_cases.py with graph, frames, contig lengths
     and excl names shifted together; `top` for the cases the rule does not end with a leap;
  E. the walker wave (walk_job of k5_travel.hip, through pag_debug_walk): one case of each family of tests/walk_cases.py, every
     case of the leaping family and every case with a TRAV_MODE_LEAP job, the successor records' coordinate field, the contig
     records and the jobs' bounds shifted by `straddle` and `upper`, exact and speculating; a leap job's iteration log against
     the rule's entry (flag, min(elow, 2^31 - 1), m0) — above 2^31 every entry is at the clamp.

The view's kernels are in tests/test_gpu_high_coords_view.py, the block tables of k_pack_paths in tests/test_gpu_walk_aux.py, the
segment kernels' random mode over the whole range in tests/test_gpu_segment_shapes.py, try_merge_leap at the clamp in
tests/test_walk_stitch.py; tests/test_high_coords.py holds the helper and the cases to what they are named for without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import find_rule
import goldens
import high_coords as hc
import pagctl  # (puts the repository root on the path)
import succ_rule
import view_rule
import walk_straight_cases as cases
import walk_straight_rule as rule
import aligngraph2_amd as ag
from aligngraph2_amd.capi import BuildStats, PagSeqs, ShardSlice, TravelParams
from test_gpu_succ_golden import check_against_reference, device_records, reference_of_rule
from test_gpu_succ_query import assert_lists, rows_of, slice_arrays
from test_gpu_walk_straight import Constructed, answers, arrays_of, assert_answers, by_the_rule
from test_walk_straight_rule import CASES, constructed

GRAPHS = ("succ_corners_t8", "eps5_k7_repeats_t8")
CASE_TABLE = [(name, which) for name in GRAPHS for which in hc.SHIFTS]  # yardstick 2 applies unless which is in hc.WRAP
ORDER_SWITCHES = ("PAG_SUCC_HEAVY", "PAG_ORDER_SLICES", "PAG_TRAVEL_VIEW", "PAG_VIEW_HALO", "PAG_VIEW_MARGIN", "PAG_DEBUG_EMIT_CAP")


def params_of(name):
    """(deviation, error rate): the reference's own and a tight pair"""
    return ((2 * goldens.load_spec(name)["epsilon"], 0.15), (0, 0.05))


@functools.lru_cache(maxsize=None)
def shifted(name, which):
    """block 0 of a golden graph translated: (graph, dc, dr, codes by vertex, positions by vertex)"""
    g0 = succ_rule.load_graph(name)[0]
    dc, dr = hc.deltas(which, g0["ctg"], g0["ref"])
    g = hc.shift(g0, dc, dr)
    assert hc.reaches(which, g["ctg"]) and hc.reaches(which, g["ref"]), f"{name}: shift {which} does not put the graph where its name says"
    vpos = (g["ctg"].astype(np.uint64) << np.uint64(32)) | g["ref"].astype(np.uint64)
    return g, dc, dr, g["code"][g["node_of_vertex"]].astype(np.uint32), vpos


@functools.lru_cache(maxsize=None)
def rule_lists(name, which, deviation, err):
    g = shifted(name, which)[0]
    return succ_rule.successors(g, np.arange(len(g["ctg"])), deviation, err)


class Imported:
    """a graph in succ_rule's form in a fresh handle (pag_shard_import), as test_constructed_graph_with_many_edges does"""

    def __init__(self, g, k):
        self.graph, self.k = g, k

    def __enter__(self):
        import torch
        self.hip = pagctl.hip_lib()
        g = self.graph
        host = slice_arrays(g, np.random.default_rng(31))
        words = np.array([self.k, 1, 2, 3], dtype=np.uint64)
        err = C.c_int()
        self.g = C.c_void_p(self.hip.pag_create(words.ctypes.data, len(words), self.k, 0, C.byref(err)))
        assert self.g, self.hip.pag_last_error()
        self.dev = [torch.from_numpy(a.view(np.uint8).copy()).cuda() for a in host]  # (torch has no unsigned 32 / 64-bit tensors: the bytes go up)
        self.st = BuildStats()
        self.st.n_nodes, self.st.n_pos, self.st.n_uniq_edges = len(g["code"]), len(g["ctg"]), len(g["child_code"])
        self.slice = ShardSlice(len(host[0]), len(host[4]), *[t.data_ptr() for t in self.dev], self.st)
        try:
            self.load()
        except BaseException:
            self.hip.pag_destroy(self.g)
            raise
        return self

    def load(self):
        assert self.hip.pag_shard_import(self.g, C.byref(self.slice), 1, None) == 0, self.hip.pag_last_error()

    def __exit__(self, *exc):
        self.hip.pag_destroy(self.g)


def golden_k(name):
    return goldens.load_spec(name)["spec"]["k"]


# ---- A. successor lists on demand ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_lists(name, which):
    """{(deviation, error rate): (off, records)} of every vertex of the shifted graph, as the device answers"""
    g, dc, dr, vcode, vpos = shifted(name, which)
    out = {}
    with Imported(g, golden_k(name)) as imp:
        for deviation, err in params_of(name):
            off, status, rec = ag.successors_batch(imp.hip, imp.g, vcode, vpos, deviation, err)
            assert not status.any(), f"{name} {which}: {np.count_nonzero(status)} vertices of the graph are not found"
            out[(deviation, err)] = (np.asarray(off).astype(np.int64), rec)
    return out


def reached_by_the_rule(name, which):
    """what the shifted case must still reach, derived from the rule alone"""
    g = shifted(name, which)[0]
    (deviation, err), _ = params_of(name)
    off, rec = rule_lists(name, which, deviation, err)
    src = np.repeat(np.arange(len(g["ctg"])), np.diff(off))
    return {"big_step": int(rec[:, 1].max()), "positions": int(np.diff(g["pos_off"]).max()), "wraps": hc.wrapping_sums(g, (src, rec))}


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", CASE_TABLE)
def test_a_successor_lists_on_demand(name, which):
    g, dc, dr, vcode, vpos = shifted(name, which)
    reach = reached_by_the_rule(name, which)
    if name == "succ_corners_t8":
        assert reach["big_step"] >= 1024, "no accepted pair with a step of 1024 or more"
        assert reach["positions"] > 255, "no k-mer with more than 255 positions"
    if which == "top":
        assert reach["wraps"][0] > 0, f"no accepted pair whose contig coordinate + step wraps: {reach['wraps']}"
    else:
        assert reach["wraps"] == (0, 0)
    got = device_lists(name, which)
    for deviation, err in params_of(name):
        label = f"{name} shift {which} deviation {deviation} error rate {err}"
        w_off, w = rule_lists(name, which, deviation, err)
        off, rec = got[(deviation, err)]
        assert_lists(label + " [the rule on the shifted graph]", off, rec, w_off, rows_of(vcode, vpos, w[:, 0], w[:, 1], w[:, 2], w[:, 3]))
        if which not in hc.WRAP:
            l_off, l_rec = device_lists(name, "low")[(deviation, err)]
            moved = l_rec.copy()
            moved["pos"] = hc.pos(l_rec["pos"], dc, dr)
            assert_lists(label + " [the device's low answer translated]", off, rec, l_off, moved)


# ---- B. the successor stage and the coordinate order ----------------------------------------------------------------------------------
MODES = [(heavy, slices) for heavy in (None, "4", "0") for slices in ("1", "8")]


def input_lengths(name, workdir):
    ind = goldens.materialize_inputs(name, str(workdir / "high_coords" / name / "in"))
    return tuple(np.array([len(s) for _, s in find_rule.read_fasta(os.path.join(ind, f))], dtype=np.int64) for f in ("ctg.fasta", "ref.fasta"))


_prepared_low = {}


def prepared(name, which, workdir, monkeypatch):
    """per mode: (off, recs, code, pos) of pag_travel_prepare's whole view of the shifted graph"""
    g, dc, dr, vcode, vpos = shifted(name, which)
    ctg_len, ref_len = input_lengths(name, workdir)
    ctg_len = np.array(hc.leading_lengths(dc, ctg_len), dtype=np.uint32)
    ref_len = np.array(hc.leading_lengths(dr, ref_len), dtype=np.uint32)
    # (the lengths describe the shifted layout: every strand of the inputs starts dc / dr further on)
    n0c, n0r = len(ctg_len) - (2 if dc else 0), len(ref_len) - (2 if dr else 0)
    assert hc.mapper_starts(ctg_len)[-n0c:] == [s + dc for s in hc.mapper_starts(ctg_len[-n0c:])]
    assert hc.mapper_starts(ref_len)[-n0r:] == [s + dr for s in hc.mapper_starts(ref_len[-n0r:])]
    spec = goldens.load_spec(name)
    ctgs = PagSeqs(len(ctg_len), None, ctg_len.ctypes.data, None, 0)  # (the view is laid out from the lengths alone)
    prm = TravelParams(spec["threads"], 0, 2 * spec["epsilon"], 0.15, 0.90, 50)
    out = {}
    with Imported(g, golden_k(name)) as imp:
        for n_mode, (heavy, slices) in enumerate(MODES):
            for s in ORDER_SWITCHES:
                monkeypatch.delenv(s, raising=False)
            if heavy is not None:
                monkeypatch.setenv("PAG_SUCC_HEAVY", heavy)
            monkeypatch.setenv("PAG_ORDER_SLICES", slices)
            if n_mode:
                imp.load()  # (a fresh graph: nothing prepared is kept)
            assert imp.hip.pag_travel_prepare(imp.g, C.byref(ctgs), ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == 0, imp.hip.pag_last_error()
            out[(heavy, slices)] = device_records(imp.hip, imp.g)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", CASE_TABLE)
def test_b_successor_stage_and_coordinate_order(name, which, workdir, monkeypatch):
    g, dc, dr, vcode, vpos = shifted(name, which)
    deviation, err = params_of(name)[0]
    ref = reference_of_rule(g, *rule_lists(name, which, deviation, err))
    order, n_free = view_rule.order(vpos)
    assert 0 < n_free < len(vpos) and np.all(np.diff((vpos[order[n_free:]] >> np.uint64(32)).astype(np.int64)) >= 0)
    got = prepared(name, which, workdir, monkeypatch)
    if which == "low":
        _prepared_low[name] = got
    elif which not in hc.WRAP and name not in _prepared_low:
        _prepared_low[name] = prepared(name, "low", workdir, monkeypatch)
    for mode, (off, recs, code, pos) in got.items():
        label = f"{name} shift {which} [PAG_SUCC_HEAVY {mode[0] or 'default'}, PAG_ORDER_SLICES {mode[1]}]"
        # the coordinate order: the coordinate-free vertices by reference coordinate, then the rest by contig coordinate, unsigned
        assert len(pos) == len(vpos), f"{label}: the whole view holds {len(pos)} of {len(vpos)} vertices"
        bad = np.flatnonzero((pos != vpos[order]) | (code != vcode[order]))
        assert len(bad) == 0, (f"{label}: new id {int(bad[0])} is vertex ({int(code[bad[0]])}, {int(pos[bad[0]]):#x}), the coordinate order puts "
                               f"({int(vcode[order[bad[0]]])}, {int(vpos[order[bad[0]]]):#x}) there; {len(bad)} ids differ")
        # every list, and what every record says of its target (contig coordinate, first record, record count)
        res = check_against_reference(ref, off, recs, code, pos, True, label)
        assert res["records"] == len(ref["rec"])
        if which not in hc.WRAP:
            l_off, l_recs, l_code, l_pos = _prepared_low[name][mode]
            assert np.array_equal(off, l_off) and np.array_equal(code, l_code), f"{label}: offsets or codes differ from the low run"
            assert np.array_equal(pos, hc.pos(l_pos, dc, dr)), f"{label}: positions differ from the low run's translated"
            want = l_recs.copy()
            want[:, 1] = hc.coord(l_recs[:, 1], dc)
            bad = np.flatnonzero((recs != want).any(axis=1))
            assert len(bad) == 0, f"{label}: record {int(bad[0])} is {recs[bad[0]].tolist()}, the low run's translated {want[bad[0]].tolist()}; {len(bad)} differ"


# ---- D. pag_walk_straight_batch -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def straight(which):
    """the constructed graph of tests/walk_straight_cases.py translated: (lists, dc, dr, contig lengths, frames' translation)"""
    L0, ids = constructed()
    dc, dr = hc.deltas(which, L0.g["ctg"], L0.g["ref"])
    g = hc.shift(L0.g, dc, dr)
    assert hc.reaches(which, g["ctg"]) and hc.reaches(which, g["ref"])
    ctg_len = tuple(hc.leading_lengths(dc, cases.CTG_LEN))
    moved = lambda kw: dict(hc.frame_kwargs(kw, dc), ctg_len=ctg_len)  # noqa: E731
    return rule.Lists(g, cases.DEVIATION, cases.ERROR_RATE, L0.count), dc, dr, ctg_len, moved


def straight_cases(which):
    """the cases that run at a shift: all of them, but at a wrap shift only those the rule does not end with a leap"""
    L, dc, dr, ctg_len, moved = straight(which)
    ids = constructed()[1]
    if which not in hc.WRAP:
        return list(CASES)
    return [c for c in CASES if rule.walk_straight(L, c.frame_of(ids, moved), ids[c.start], c.dist, c.has_size, c.limit)[1] != rule.LEAP]


@pytest.mark.gpu
@pytest.mark.parametrize("which", hc.SHIFTS)
def test_d_walk_straight_every_line_of_the_rule(which):
    L, dc, dr, ctg_len, moved = straight(which)
    picked = straight_cases(which)
    assert len(picked) == len(CASES) if which not in hc.WRAP else 20 <= len(picked) < len(CASES)
    with Constructed(L, ctg_len, moved) as c:
        calls = c.calls(picked)
        want = by_the_rule(c.L, calls, c.name_of)
        got = answers(c.walk(*arrays_of(calls, c.name_of)))
        for case, g, w in zip(picked, got, want):
            assert_answers(f"shift {which}: {case.name}", [g], [w])
            if which in hc.WRAP:
                continue
            # the hand-written answer, translated (name_of names the shifted vertices)
            assert [x[:2] for x in g[0]] == [c.name_of(c.ids[v]) for v in case.path] and g[1] == case.status, f"shift {which}: {case.name}"
            assert [x[:2] for x in g[2]] == [c.name_of(c.ids[v]) for v in case.alts], f"shift {which}: {case.name}"


# ---- E. the walker wave ----------------------------------------------------------------------------------------------------------------
WALK_SHIFTS = ("low", "straddle", "upper")


def walk_cases_picked(all_cases):
    """one case of each family — the one with the fewest vertices (the first of them), which tests/test_walk_rule.py holds to its
    counter like every other — every case of the leaping family, and every case with a job that writes the iteration log"""
    import test_gpu_walk as TW
    picked = []
    for family in TW.FAMILIES:
        mine = [c for c in all_cases if c.family == family]
        picked += mine if family == "leaping" else [min(mine, key=lambda c: c.G.n_pos)]
    # (no case of the leaping family runs a TRAV_MODE_LEAP job: the cases that do, for the iteration log)
    return picked + [c for c in all_cases if c not in picked and any(j.mode & 4 for j in c.jobs)]


def walk_shifted(case, which):
    """(graph, contig, dc) of a case of tests/walk_cases.py translated along the contig axis"""
    pc = (case.G.upos >> np.uint64(32)).astype(np.int64)
    dc = hc.deltas(which, pc, pc)[0]
    G = hc.walk_graph(case.G, dc)
    assert hc.reaches(which, (G.upos >> np.uint64(32)).astype(np.int64)), f"{case.name}: shift {which} does not put the graph where its name says"
    return G, hc.walk_contig(case.C, dc), dc


def walk_translated(label, job, low, got, dc, overflow_case, must_misspeculate):
    """-> the first difference between a device job on the shifted input and the same job's `low` run translated, or None"""
    import test_gpu_walk as TW
    (o, sv, ss, sx, intact), (lo_, lv, ls, lx, _) = got, low
    if overflow_case or must_misspeculate:
        return None if (int(o["overflow"]) & 7) == (int(lo_["overflow"]) & 7) else f"{label}: overflow {int(o['overflow'])}, the low run {int(lo_['overflow'])}"
    n = int(o["seq_len"])
    d = TW._diff(label, "seq_v", sv[:n], lv[:int(lo_["seq_len"])]) or TW._diff(label, "seq_s", ss[:n], ls[:int(lo_["seq_len"])])
    if d:
        return d
    names = ["seq_len", "seq_size", "last_ctg", "stopped", "poison", "n_main", "max_chosen", "overflow"]
    if job.exact:
        names += ["max_back", "max_probe", "wd_below_max", "wd_forced_min"]
    for f in names:
        want = hc.bound(int(lo_[f]), dc) if f in hc.WALK_COORDS else int(lo_[f])
        if int(o[f]) != want:
            return f"{label}: {f} is {int(o[f])}, the low run's translated {want}"
    if job.mode & TW.R.MODE_LEAP and job.exact:
        want = np.array([x if x == TW.SENT or not x >> 63 else hc.log_entry(x, dc) for x in lx.tolist()], dtype=np.uint64)
        return TW._diff(label, "seq_x", sx, want)
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("which", WALK_SHIFTS)
def test_e_walker_wave(which):
    import test_gpu_walk as TW
    import walk_cases as W
    import walk_rule as R
    hip = pagctl.hip_lib()
    out = np.zeros(9, dtype=np.uint32)
    assert hip.pag_debug_walk_geometry(out.ctypes.data, 9) == 0, hip.pag_last_error()
    geom = dict(zip(R.GEOMETRY_NAMES, (int(x) for x in out)))
    picked = walk_cases_picked(W.cases(geom))
    assert {c.family for c in picked} == set(TW.FAMILIES) and sum(c.family == "leaping" for c in picked) >= 15
    bad, n_logs, clamped = [], 0, 0
    for case in picked:
        G, Cg, dc = walk_shifted(case, which)
        jobs0 = TW._variants(case)
        jobs = [hc.walk_job(j, dc) for j in jobs0]
        got = TW.run_jobs(hip, G, Cg, jobs)
        low = TW.run_jobs(hip, case.G, case.C, jobs0) if which != "low" else got
        for i, (j, g, l0) in enumerate(zip(jobs, got, low)):
            rule = R.run_job(G, Cg, j, geom)
            label = f"shift {which}: {case.name}[job {i // 2}, exact = {j.exact}]"
            assert bool(rule.overflow) == bool(case.overflow), label
            miss = case.name in TW.MUST_MISSPECULATE and not j.exact
            d = TW.compare(label + " [the rule on the shifted input]", j, g, rule, overflow_case=case.overflow, must_misspeculate=miss)
            d = d or walk_translated(label + " [the low run translated]", j, l0, g, dc, case.overflow, miss)
            if d:
                bad.append(d)
            if j.mode & R.MODE_LEAP and j.exact:
                n_logs += len(rule.seq_x)
                clamped += sum(1 for x in rule.seq_x.values() if (x >> 32) & 0x7FFFFFFF == 0x7FFFFFFF)
    assert n_logs >= 3, "no TRAV_MODE_LEAP job among the cases: the iteration log was not compared"
    # what the log's 31-bit coordinate does at this shift, from the rule: below 2^31 some entries hold a coordinate, above every one
    # is at the clamp
    assert (clamped < n_logs) if which == "low" else (clamped == n_logs if which == "upper" else clamped > 0), (which, clamped, n_logs)
    assert not bad, f"{len(bad)} differences; the first: {bad[0]}\nall:\n" + "\n".join(bad[:40])
