"""GPU: the walker wave (walk_job of k5_travel.hip, through the one-shot k_walk) held to tests/walk_rule.py on the constructed
graphs of tests/walk_cases.py, every case with exact = 1 and with exact = 0.

Both modes compare exactly and name the first difference: the sequence, seq_len, seq_size, last_ctg, stopped, poison, n_main,
max_chosen, overflow & 3 and the guard entries behind every returned buffer.  Exact mode also compares the splice bookkeeping
(max_back, max_probe, wd_below_max, wd_forced_min, the seq_x log); under speculation the set of examined records is the
kernel's own business and stays unverified.  A case built to overflow asserts overflow & 3 and the guards, nothing about the
path.  Mis-speculation (overflow & 4) must be clear everywhere except on MUST_MISSPECULATE, whose entries must report it;
tests/test_walk_rule.py runs the cases against the shapes they are named for without a device."""
import ctypes as C

import numpy as np
import pytest

import pagctl
import walk_cases as W
import walk_rule as R
from aligngraph2_amd.capi import DTYPES, PAG_DEBUG_WALK_GUARD, DebugTravGraph, DebugWalkContig

pytestmark = pytest.mark.gpu
JOB, OUT = DTYPES["pag_debug_walk_job"], DTYPES["pag_debug_walk_out"]
SENT, GUARD32, GUARD64 = 0xABCD1234, 0xDEADBEEF, 0xDEADBEEFDEADBEEF

# The cases that MUST mis-speculate, each with the reason taken from the code.  This list is a condition, not a measurement: a
# case off it that reports bit 4 is a finding to explain from probe_slots / slots_step.  A case with no record outside
# [ctg_left, ctg_right) and no vertex of more than 64 records can never be on it (tests/test_walk_rule.py asserts that of the
# cases' own flags, which this list must equal).
MUST_MISSPECULATE = {
    "zombie_that_later_leaps": "slots_dominate makes the less abundant, still-walking alternative a zombie once the other has stopped at a "
                               "branch; the zombie then ends in WS_LEAP, which slots_step reports as spec_fail bit 0",
}


@pytest.fixture(scope="module")
def hip():
    return pagctl.hip_lib()


@pytest.fixture(scope="module")
def geom(hip):
    out = np.zeros(9, dtype=np.uint32)
    assert hip.pag_debug_walk_geometry(out.ctypes.data, 9) == 0, hip.pag_last_error()
    g = dict(zip(R.GEOMETRY_NAMES, (int(x) for x in out)))
    assert g["PROBE_GROUPS"] in (4, 8) and g["WIN_IDS"] % 32 == 0 and g["LIST_CAP"] == 64
    return g


@pytest.fixture(scope="module")
def cases(geom):
    return W.cases(geom)


def _gset(members):
    cap = 8
    while cap < 4 * len(members) + 2:
        cap *= 2
    tab = np.full(cap, 0xFFFFFFFF, dtype=np.uint32)
    for v in members:
        s = R.hs_slot(v, cap - 1)
        while tab[s] != 0xFFFFFFFF:
            s = (s + 1) & (cap - 1)
        tab[s] = v
    return tab


def run_jobs(hip, G, Cg, jobs):
    """the jobs through pag_debug_walk -> [(result record, seq_v, seq_s, seq_x of the job's range, guards intact)]"""
    keep = dict(newid=np.ascontiguousarray(G.newid), upos=np.ascontiguousarray(G.upos), ucnt=np.ascontiguousarray(G.ucnt),
                succ_off=np.ascontiguousarray(G.succ_off), succ=np.ascontiguousarray(G.succ))
    if G.incomplete is not None:
        keep["incomplete"] = np.ascontiguousarray(G.incomplete)
    g = DebugTravGraph(n_nodes=0, n_pos=G.n_pos, k=G.k, n_succ=len(G.succ), **{n: (a.ctypes.data if len(a) else None) for n, a in keep.items()})
    starts, sizes = np.array(Cg.starts, dtype=np.uint64), np.array(Cg.sizes, dtype=np.uint64)
    gbits = gset = None
    if Cg.gvisited is not None:
        gbits = np.zeros((Cg.g_hi - Cg.g_lo + 31) // 32 + 1, dtype=np.uint32)
        for v in Cg.gvisited:
            if Cg.g_lo <= v < Cg.g_hi:
                gbits[(v - Cg.g_lo) >> 5] |= np.uint32(1 << ((v - Cg.g_lo) & 31))
        gset = _gset([v for v in Cg.gvisited if not Cg.g_lo <= v < Cg.g_hi])
    ctg = DebugWalkContig(ctg_left=Cg.ctg_left, ctg_right=Cg.ctg_right, rev_left=Cg.rev_left, rev_right=Cg.rev_right, split_size=Cg.split_size,
                          leap_min=Cg.leap_min, n_ctgs=len(sizes), in_lo=Cg.in_lo, in_hi=Cg.in_hi, g_lo=Cg.g_lo, g_hi=Cg.g_hi,
                          gmask=(len(gset) - 1 if gset is not None else 0), gwin_lo=Cg.gwin_lo, gwin_hi=Cg.gwin_hi, starts=starts.ctypes.data,
                          sizes=sizes.ctypes.data, gbits=(gbits.ctypes.data if gbits is not None else None),
                          gset=(gset.ctypes.data if gset is not None else None), n_gbits=(len(gbits) if gbits is not None else 0))
    ja = np.zeros(len(jobs), dtype=JOB)
    off = 0
    for i, j in enumerate(jobs):
        ja[i] = (j.has_size, j.seq_cap, len(j.init), j.set_size, off, 0, j.start, j.exact, j.mode, j.stop_pc, j.win_low)
        off += j.seq_cap + PAG_DEBUG_WALK_GUARD
    sv, ss, sx = np.full(off, SENT, dtype=np.uint32), np.full(off, SENT, dtype=np.uint32), np.full(off, SENT, dtype=np.uint64)
    for i, j in enumerate(jobs):
        o, cap = int(ja[i]["out_off"]), j.seq_cap
        sv[o + cap:o + cap + PAG_DEBUG_WALK_GUARD] = ss[o + cap:o + cap + PAG_DEBUG_WALK_GUARD] = GUARD32
        sx[o + cap:o + cap + PAG_DEBUG_WALK_GUARD] = GUARD64
        for q, (v, s) in enumerate(j.init):
            sv[o + q], ss[o + q] = v, s
    outs = np.zeros(len(jobs), dtype=OUT)
    rc = hip.pag_debug_walk(C.byref(g), C.byref(ctg), 1, ja.ctypes.data, len(jobs), sv.ctypes.data, ss.ctypes.data, sx.ctypes.data, off, outs.ctypes.data, 0)
    assert rc == 0, hip.pag_last_error()
    res = []
    for i, j in enumerate(jobs):
        o, cap = int(ja[i]["out_off"]), j.seq_cap
        gd = slice(o + cap, o + cap + PAG_DEBUG_WALK_GUARD)
        intact = bool((sv[gd] == GUARD32).all() and (ss[gd] == GUARD32).all() and (sx[gd] == GUARD64).all())
        res.append((outs[i], sv[o:o + cap], ss[o:o + cap], sx[o:o + cap], intact))
    return res


def _diff(label, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    m = min(len(got), len(want))
    d = np.flatnonzero(got[:m] != want[:m])
    at = int(d[0]) if len(d) else m
    return f"{label}: {what} differs ({len(got)} entries, the rule has {len(want)}); first at {at}: device {got[at:at + 4].tolist()} rule {want[at:at + 4].tolist()}"


def compare(label, job, got, rule, overflow_case=False, must_misspeculate=False):
    """-> the first difference between a device job and the rule's, or None"""
    o, sv, ss, sx, intact = got
    if not intact:
        return f"{label}: the guard entries behind seq_cap were written"
    ov = int(o["overflow"])
    if overflow_case:
        return None if ov & 3 else f"{label}: built to overflow, overflow = {ov}"
    if must_misspeculate:
        return None if ov & 4 else f"{label}: on the list of cases that must mis-speculate, overflow = {ov} (n_fill = {int(o['n_fill']):#x})"
    if ov & 4:
        return f"{label}: mis-speculated and is not on the list (reasons {int(o['n_fill']) >> 32:#x})"
    if ov & 3:
        return f"{label}: overflow = {ov}, the rule has none"
    n = int(o["seq_len"])
    d = _diff(label, "seq_v", sv[:n], rule.seq_v) or _diff(label, "seq_s", ss[:n], rule.seq_s)
    if d:
        return d
    names = ["seq_len", "seq_size", "last_ctg", "stopped", "poison", "n_main", "max_chosen"]
    if job.exact:
        names += ["max_back", "max_probe", "wd_below_max", "wd_forced_min"]
    for f in names:
        if int(o[f]) != int(getattr(rule, f)):
            return f"{label}: {f} is {int(o[f])}, the rule has {int(getattr(rule, f))}"
    if job.mode & R.MODE_LEAP:
        if job.exact:
            want = np.zeros(job.seq_cap, dtype=np.uint64)
            for i, x in rule.seq_x.items():
                want[i] = x
            return _diff(label, "seq_x", sx, want)
    elif not (sx == SENT).all():
        return f"{label}: seq_x was written by a job that has no log"
    return None


def _variants(case):
    jobs = []
    for j in case.jobs:
        for exact in (1, 0):
            jobs.append(R.Job(j.start, j.has_size, j.seq_cap, exact, j.mode, j.stop_pc, j.win_low, j.init, j.set_size))
    return jobs


FAMILIES = ("window", "lists", "off_strand", "leaping", "modes", "overflow", "markers", "speculation")


def test_the_list_is_the_cases_own(cases):
    assert {c.name for c in cases if c.misspec} == set(MUST_MISSPECULATE) and len(MUST_MISSPECULATE) >= 1
    assert {c.family for c in cases} == set(FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_walker_equals_the_rule(hip, geom, cases, family):
    bad = []
    mine = [c for c in cases if c.family == family]
    assert mine
    for case in mine:
        jobs = _variants(case)
        got = run_jobs(hip, case.G, case.C, jobs)
        for i, (j, g) in enumerate(zip(jobs, got)):
            rule = R.run_job(case.G, case.C, j, geom)
            label = f"{case.name}[job {i // 2}, exact = {j.exact}]"
            assert bool(rule.overflow) == bool(case.overflow), label
            d = compare(label, j, g, rule, overflow_case=case.overflow, must_misspeculate=(case.name in MUST_MISSPECULATE and not j.exact))
            if d:
                bad.append(d)
    assert not bad, f"{len(bad)} differences; the first: {bad[0]}\nall:\n" + "\n".join(bad[:40])


def test_the_hook_refuses_what_would_leave_its_buffers(hip, cases):
    case = next(c for c in cases if c.name == "hull_gap_rejected_and_contig_edge_kept")
    G, Cg, j = case.G, case.C, case.jobs[0]

    def refused(G2=G, C2=Cg, j2=j):
        keep = dict(newid=np.ascontiguousarray(G2.newid), upos=np.ascontiguousarray(G2.upos), ucnt=np.ascontiguousarray(G2.ucnt),
                    succ_off=np.ascontiguousarray(G2.succ_off), succ=np.ascontiguousarray(G2.succ))
        g = DebugTravGraph(n_nodes=0, n_pos=G2.n_pos, k=G2.k, n_succ=len(G2.succ), **{n: a.ctypes.data for n, a in keep.items()})
        starts, sizes = np.array(C2.starts, dtype=np.uint64), np.array(C2.sizes, dtype=np.uint64)
        ctg = DebugWalkContig(ctg_left=C2.ctg_left, ctg_right=C2.ctg_right, split_size=C2.split_size, leap_min=C2.leap_min, n_ctgs=len(sizes),
                              in_lo=C2.in_lo, in_hi=C2.in_hi, g_lo=C2.g_lo, g_hi=C2.g_hi, gwin_lo=C2.gwin_lo, gwin_hi=C2.gwin_hi,
                              starts=starts.ctypes.data, sizes=sizes.ctypes.data)
        ja = np.zeros(1, dtype=JOB)
        ja[0] = (j2.has_size, j2.seq_cap, len(j2.init), j2.set_size, 0, 0, j2.start, 1, j2.mode, j2.stop_pc, j2.win_low)
        n = j2.seq_cap + PAG_DEBUG_WALK_GUARD
        sv, ss, sx = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        for q, (v, s) in enumerate(j2.init):
            sv[q], ss[q] = v, s
        outs = np.zeros(1, dtype=OUT)
        return hip.pag_debug_walk(C.byref(g), C.byref(ctg), 1, ja.ctypes.data, 1, sv.ctypes.data, ss.ctypes.data, sx.ctypes.data, n, outs.ctypes.data, 0)

    assert refused() == 0, hip.pag_last_error()

    def graph(**kw):
        a = dict(k=G.k, upos=G.upos.copy(), ucnt=G.ucnt.copy(), newid=G.newid.copy(), succ_off=G.succ_off.copy(), succ=G.succ.copy())
        a.update(kw)
        return R.Graph(**a)

    def contig(**kw):
        a = dict(ctg_left=Cg.ctg_left, ctg_right=Cg.ctg_right, split_size=Cg.split_size, leap_min=Cg.leap_min, starts=Cg.starts, sizes=Cg.sizes,
                 in_lo=Cg.in_lo, in_hi=Cg.in_hi, g_lo=Cg.g_lo, g_hi=Cg.g_hi)
        a.update(kw)
        return R.Contig(**a)

    EINVAL = -22
    s = G.succ.copy()
    s["tgt"][0] = G.n_pos
    assert refused(G2=graph(succ=s)) == EINVAL
    for field, delta in (("pc", 1), ("toff", 1), ("meta", 1 << 28)):
        s = G.succ.copy()
        s[field][0] += delta
        assert refused(G2=graph(succ=s)) == EINVAL, field
    so = G.succ_off.copy()
    so[3], so[4] = so[4] + 1, so[3]
    assert refused(G2=graph(succ_off=so)) == EINVAL
    nid = G.newid.copy()
    nid[j.start] = G.n_pos
    assert refused(G2=graph(newid=nid)) == EINVAL
    assert refused(C2=contig(in_hi=G.n_pos + 1, g_hi=G.n_pos + 1)) == EINVAL
    assert refused(C2=contig(in_lo=Cg.in_lo + 1)) == EINVAL          # in_lo - g_lo no multiple of 32
    assert refused(C2=contig(g_lo=Cg.in_lo + 32 if Cg.in_lo + 32 <= Cg.in_hi else Cg.in_hi + 1)) == EINVAL  # g_lo above in_lo
    assert refused(C2=contig(starts=(5, 4, 9))) == EINVAL
    assert refused(j2=R.Job(j.start, seq_cap=4, mode=R.MODE_RESUME, init=[(0, 8)] * 5)) == EINVAL
    assert refused(j2=R.Job(j.start, seq_cap=8, mode=R.MODE_RESUME, init=[(G.n_pos, 8)])) == EINVAL
    assert refused(j2=R.Job(j.start, seq_cap=8, mode=R.MODE_RESUME, init=[])) == EINVAL
    assert refused(j2=R.Job(j.start, set_size=24)) == EINVAL
    assert refused(j2=R.Job(j.start, seq_cap=0)) == EINVAL


# =====================================================================================================================
# the rule on real graphs: the record distributions the reference itself produced (the goldens pin them to it end to end)
# =====================================================================================================================
def _real_graph(hip, g, inp, prepared, ctg_len, ref_len, prm):
    """the whole graph's traversal view of a handle as a walk_rule.Graph (new ids; the hook's newid is the identity)"""
    from test_gpu_succ_golden import device_records
    from aligngraph2_amd.capi import PagSeqs
    csr = pagctl._run(hip, "pag", g, inp, False, prepared)["csr"]
    ctgs = PagSeqs(len(ctg_len), None, ctg_len.ctypes.data, None, 0)
    assert hip.pag_travel_prepare(g, C.byref(ctgs), ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
    off, recs, code, pos = device_records(hip, g)
    # abundances: the exported CSR's, matched by (k-mer code, position)
    node = np.repeat(np.arange(len(csr["node_code"])), np.diff(csr["pos_off"].astype(np.int64)))
    key = {(int(c), (int(a) << 32) | int(b)): int(n) for c, a, b, n in zip(csr["node_code"][node], csr["pos_ctg"], csr["pos_ref"], csr["pos_cnt"])}
    ucnt = np.array([key[(int(c), int(p))] for c, p in zip(code, pos)], dtype=np.uint32)
    succ = np.zeros(len(recs), dtype=R.SUCC_DTYPE)
    for i, f in enumerate(("tgt", "pc", "meta", "toff")):
        succ[f] = recs[:, i]
    return R.Graph(inp.k, pos, ucnt, np.arange(len(pos), dtype=np.uint32), off.astype(np.uint32), succ)


@pytest.mark.parametrize("name", ["succ_corners_t8", "two_blocks_both_orient_t16"])
def test_walker_equals_the_rule_on_the_goldens_graphs(hip, geom, name, workdir):
    import os

    import goldens
    from aligngraph2_amd.capi import PagRawInput, TravelParams
    from test_gpu_succ_golden import block_orient
    import walk_aux_rule as A
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / name / "in_walk"))
    ctg_names = [l[1:].split()[0] for l in open(os.path.join(ind, "ctg.fasta")) if l.startswith(">")]
    n_blocks = sum(1 for b in open(os.path.join(ind, "config.txt")).read().split("\n\n") if b.strip())
    start_split = 0.90
    bad, n_jobs, n_steps = [], 0, 0
    for block in range(n_blocks):
        inp = pagctl.LoadedInput(ind, threads=spec["threads"], eps=spec["epsilon"], cov=spec["cov"], block=block)
        err = C.c_int()
        g = C.c_void_p(hip.pag_create(inp.kmer_words, inp.n_kmer_words, inp.k, 0, C.byref(err)))
        assert g, hip.pag_last_error()
        try:
            raw = PagRawInput.from_address(inp.raw_view)
            ctg_len = np.ctypeslib.as_array(C.cast(raw.ctg_len, C.POINTER(C.c_uint32)), shape=(raw.n_ctgs,)).copy()
            ref_len = np.ctypeslib.as_array(C.cast(raw.ref_len, C.POINTER(C.c_uint32)), shape=(raw.n_refs,)).copy()
            prm = TravelParams(spec["threads"], 0, 2 * spec["epsilon"], 0.15, start_split, 50)
            G = _real_graph(hip, g, inp, pagctl._prepared_view(hip, g, inp), ctg_len, ref_len, prm)
        finally:
            hip.pag_destroy(g)
            inp.close()
        # the contig coordinate space from the lengths (Mapper of walk_round.hpp = the reference's PositionMapper)
        sizes = [int(x) for x in ctg_len]
        starts = [sizes[0]]
        for i in range(1, len(sizes)):
            starts.append(starts[-1] + 3 * sizes[i - 1] + max(sizes[i - 1], sizes[i]))
        starts.append(starts[-1] + 4 * sizes[-1])
        orient = block_orient(ind, block, ctg_names)
        for c, o in enumerate(orient):
            for fwd in ([True] if o == 1 else [False] if o == 0 else [True, False] if o == 2 else []):
                left = starts[c] + (0 if fwd else 2 * sizes[c])
                other = starts[c] + (2 * sizes[c] if fwd else 0)
                lo, hi = (int(x) for x in A.id_bounds({"upos": G.upos}, [left, left + sizes[c]]))  # (k_ranges: the ids of the strand)
                if hi - lo < 2:
                    continue
                Cg = R.Contig(left, left + sizes[c], other, other + sizes[c], int(sizes[c] * start_split), 1 - start_split, starts, sizes, lo, hi)
                cap = sizes[c] // 2 + 8192
                sset = 1024
                while sset < cap // 4 + 4096:
                    sset *= 2
                picks = sorted(set(int(x) for x in np.linspace(lo, hi - 1, 12)))
                jobs = [R.Job(u, 0, cap, 1, 0, 0, 0, (), sset) for u in picks]
                got = run_jobs(hip, G, Cg, jobs)
                for u, j, gj in zip(picks, jobs, got):
                    rule = R.run_job(G, Cg, j, geom)
                    assert not rule.overflow
                    d = compare(f"{name} block {block} contig {c} {'+' if fwd else '-'} from id {u}", j, gj, rule)
                    n_jobs += 1
                    n_steps += rule.seq_len
                    if d:
                        bad.append(d)
    print(f"{name}: {n_jobs} walks, {n_steps} vertices walked")
    assert n_jobs >= 12 and n_steps > 10 * n_jobs, (n_jobs, n_steps)
    assert not bad, f"{len(bad)} differences; the first: {bad[0]}\nall:\n" + "\n".join(bad[:20])
