"""GPU: the cut view (k5_view.hip k_view_mark / iv_contains / k_zone_bands / k_mark_incomplete, k_select.hip) at coordinates beyond
2^31 — cases of tests/test_gpu_view_cut.py moved up the coordinate axis together with their interval tables
(tests/high_coords.py), against tests/view_rule.py on the shifted arrays and against the device's own answer below 2^31
translated:

  * pag_debug_trav_compact, one case per branch of k_view_mark's first-of-its-segment test: segments inside one tile, and
    segments placed across tile boundaries; interval tables in LDS (1 000 + 1 000) and in global memory (1 500 + 1 500);
  * pag_debug_zone_bands: zones with positions on both of their ends;
  * pag_shard_select on a golden graph imported shifted: interval ends exactly on vertex coordinates; reference bands whose open
    ends lie exactly a margin (and a margin - 1) away from a coordinate-free vertex — 300 of them, so that k_mark_incomplete's bit
    per vertex decides; and 200 bands (staged in LDS) with the last one's open end at 2^32 - 1."""
import ctypes as C
import functools

import numpy as np
import pytest

import goldens
import high_coords as hc
import pagctl
import succ_rule
import view_rule as R
from aligngraph2_amd import parallel
from aligngraph2_amd.capi import PagSeqs, Region, TravelParams
import test_gpu_succ_golden as SG
import test_gpu_view_cut as VC
from test_gpu_high_coords import Imported, golden_k, input_lengths

SHIFTS = ("low", "straddle", "upper")
U32 = np.uint64(0xFFFFFFFF)


def _deltas(which, tval):
    """the shift of a constructed slice: by the coordinates of its slots, either axis"""
    return hc.deltas(which, (tval >> np.uint64(32)).astype(np.int64), (tval & U32).astype(np.int64))


def _moved(sl, tables, dc, dr):
    out = dict(sl)
    out["tval"] = hc.pos(sl["tval"], dc, dr)
    return out, (hc.intervals(tables[0], dc), hc.intervals(tables[1], dr))


def _assert_translated(label, got, low, dc, dr):
    """a compaction of the shifted slice is the compaction of the slice itself with the vertices' positions translated"""
    assert got["counts"] == low["counts"], f"{label}: (nodes, vertices, edges) {got['counts']}, below 2^31 {low['counts']}"
    VC._first_diff(label, "vpos against the low run's translated", got["vpos"], hc.pos(low["vpos"], dc, dr))
    for name in ("vcnt", "vnode", "ncode", "npos_off", "nedge_off", "eto", "estep"):
        VC._first_diff(label, f"{name} against the low run's", got[name], low[name])


# ---- pag_debug_trav_compact ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inside_a_tile():
    rng = np.random.default_rng(2000 + 2047)
    sl = VC._make_slice(rng, 6, VC._random_lens(rng, 2047, hi=40))
    return sl, VC._make_edges(rng, sl, 60), {kind: VC._tables(rng, kind) for kind in ("1+1", "1000+1000", "1500+1500")}


@functools.lru_cache(maxsize=None)
def _across_tiles():
    rng = np.random.default_rng(2400)
    lens, special = VC._crossings_layout(rng)
    sl = VC._make_slice(rng, 8, lens, all_leaders=[s for s, *_ in special])
    ed = VC._make_edges(rng, sl, 400)
    out = {}
    for kind in ("1000+1000", "1500+1500"):
        civ, riv = VC._tables(rng, kind)
        mine = dict(sl, tval=sl["tval"].copy())
        assert VC._place_crossings(mine, special, civ, riv)
        for what, n in VC._crossing_counts(mine, civ, riv).items():
            assert n >= 8, f"tables {kind}: only {n} segments where {what}"
        out[kind] = (mine, (civ, riv))
    return ed, out


@pytest.mark.gpu
@pytest.mark.parametrize("which", SHIFTS)
def test_c_compact_segments_inside_a_tile(which):
    hip = pagctl.hip_lib()
    sl, ed, tables = _inside_a_tile()
    dc, dr = _deltas(which, sl["tval"])
    for kind, tb in tables.items():
        label = f"shift {which}: 2 047 slots, tables {kind}"
        msl, mtb = _moved(sl, tb, dc, dr)
        c = (msl["tval"] >> np.uint64(32)).astype(np.int64)
        assert hc.reaches(which, c) and hc.reaches(which, (msl["tval"] & U32).astype(np.int64))
        want = VC._check_compact(hip, msl, ed, mtb, label)
        assert 0 < want["counts"][1] < sl["nl"].sum(), f"{label}: the tables decide nothing"
        if which != "low":
            _assert_translated(label, VC._run_compact(hip, msl, ed, mtb), VC._run_compact(hip, sl, ed, tb), dc, dr)


@pytest.mark.gpu
@pytest.mark.parametrize("which", SHIFTS)
def test_c_compact_segments_across_tile_boundaries(which):
    hip = pagctl.hip_lib()
    ed, cases = _across_tiles()
    for kind, (sl, tb) in cases.items():
        label = f"shift {which}: 36 tile boundaries, tables {kind}"
        dc, dr = _deltas(which, sl["tval"])
        msl, mtb = _moved(sl, tb, dc, dr)
        for what, n in VC._crossing_counts(msl, *mtb).items():  # (counted again on the shifted slice, from the rule's keep flags)
            assert n >= 8, f"{label}: only {n} segments where {what}"
        VC._check_compact(hip, msl, ed, mtb, label)
        if which != "low":
            _assert_translated(label, VC._run_compact(hip, msl, ed, mtb), VC._run_compact(hip, sl, ed, tb), dc, dr)


# ---- pag_debug_zone_bands ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", SHIFTS)
def test_c_zone_bands(which):
    hip = pagctl.hip_lib()
    for n_z, T in ((2049, 100_000), (5, 257)):
        rng = np.random.default_rng(1000 + n_z)
        tval, zones, empty = VC._zone_case(rng, n_z, T)
        dc, dr = _deltas(which, tval)
        mt, mz = hc.pos(tval, dc, dr), hc.intervals(zones, dc)
        want_lo, want_hi = R.zone_bands(mt, mz)
        z, c, r = mz.reshape(-1, 2).astype(np.int64), (mt >> np.uint64(32)).astype(np.int64), (mt & U32).astype(np.int64)
        assert (np.isin(c, z[:, 0]) & (r != 0)).any() and (np.isin(c, z[:, 1]) & (r != 0)).any(), "no position on a zone's ends"
        assert want_lo[empty] == 0xFFFFFFFF and want_hi[empty] == 0 and (want_hi != 0).sum() > n_z // 2

        def run(t, zz):
            lo, hi = np.full(n_z, 12345, dtype=np.uint32), np.full(n_z, 12345, dtype=np.uint32)
            assert hip.pag_debug_zone_bands(t.ctypes.data, T, zz.ctypes.data, n_z, lo.ctypes.data, hi.ctypes.data, 0) == 0, hip.pag_last_error()
            return lo, hi

        label = f"shift {which}: {n_z} zones, {T} slots"
        lo, hi = run(mt, mz)
        VC._first_diff(label, "lowest reference coordinate per zone", lo, want_lo)
        VC._first_diff(label, "highest reference coordinate per zone", hi, want_hi)
        if which != "low":
            l_lo, l_hi = run(tval, zones)
            VC._first_diff(label, "lowest reference coordinate against the low run's translated", lo, np.where(l_lo == 0xFFFFFFFF, l_lo, l_lo + np.uint32(dr)))
            VC._first_diff(label, "highest reference coordinate against the low run's translated", hi, hc.coord(l_hi, dr))


# ---- pag_shard_select on an imported golden graph -----------------------------------------------------------------------------------
NAME = "succ_corners_t8"
REGION_KINDS = ("ends on vertices", "ends a margin away", "open end at 2^32 - 1")


def _whole(g):
    """a succ_rule graph as the flat arrays test_gpu_view_cut's helpers take (the imported slices count every vertex once)"""
    return {"code": g["code"][g["node_of_vertex"]].astype(np.uint32), "ctg": g["ctg"], "ref": g["ref"], "cnt": np.ones(len(g["ctg"]), dtype=np.uint16),
            "ecode": np.repeat(g["code"], np.diff(g["child_off"])).astype(np.uint32), "eto": g["child_code"], "estep": g["child_step"]}


@functools.lru_cache(maxsize=None)
def _low_regions():
    """(civ, riv, ropen, placed) per kind, for the unshifted graph: the tables move with the graph"""
    g = succ_rule.load_graph(NAME)[0]
    blk = {"whole": _whole(g), "spec": goldens.load_spec(NAME)}
    uc = np.unique(g["ctg"][g["ctg"] != 0]).astype(np.int64)
    ur = np.unique(g["ref"][(g["ctg"] == 0) & (g["ref"] != 0)]).astype(np.int64)
    ci = [len(uc) // 10, 3 * len(uc) // 10, len(uc) // 2, 7 * len(uc) // 10]
    ri = [len(ur) // 8, 3 * len(ur) // 8, 5 * len(ur) // 8, 7 * len(ur) // 8]
    civ = uc[ci].astype(np.uint32)
    out = {"ends on vertices": (civ, ur[ri].astype(np.uint32), np.array([1, 0, 0, 1], dtype=np.uint8), None)}
    # bands over the coordinate-free vertices' stretch, every other end open or not, the outer ends pinned (test_gpu_view_cut._pin_ends):
    # 300 bands are more than a successor kernel stages in LDS, so k_mark_incomplete's bit per vertex decides; 200 stay in LDS
    for n in (300, 200):
        base = int(ur[:-1][np.diff(ur) == 1][0])
        stride = (int(ur[-1]) + 1 - base) // n
        assert stride >= 4
        lo = base + np.arange(n, dtype=np.int64) * stride
        riv = np.stack([lo, lo + (3 * stride) // 4 + 1], axis=1).astype(np.uint32).reshape(-1)
        ropen = np.random.default_rng(n).integers(0, 2, size=2 * n).astype(np.uint8)
        out[n] = (civ,) + VC._pin_ends(blk, civ, riv, ropen)
    return out


def _region(kind, dc, dr):
    low = _low_regions()[{"ends on vertices": kind, "ends a margin away": 300, "open end at 2^32 - 1": 200}[kind]]
    civ, riv, ropen, placed = hc.intervals(low[0], dc), hc.intervals(low[1], dr), low[2].copy(), low[3]
    if kind == "open end at 2^32 - 1":
        riv[-1], ropen[-1] = 0xFFFFFFFF, 1
    return civ, riv, ropen, placed


def _select_and_prepare(g, civ, riv, ropen, lengths, dc, dr):
    """import g, cut it with pag_shard_select, import the cut, set its region, prepare -> (exported CSR, device records)"""
    hip = pagctl.hip_lib()
    spec = goldens.load_spec(NAME)
    ctg_len = np.array(hc.leading_lengths(dc, lengths[0]), dtype=np.uint32)
    ref_len = np.array(hc.leading_lengths(dr, lengths[1]), dtype=np.uint32)
    region = Region(len(civ) // 2, VC._ptr(civ), len(riv) // 2, VC._ptr(riv), VC._ptr(ropen))
    with Imported(g, golden_k(NAME)) as imp:
        sb = parallel.ShardedBuild(hip, imp.g.value, None, 0, 1, "cuda")
        sl, st = sb.select({"region": region})
        sb.import_all([sl], [st])
        sb.set_region({"region": region})
        csr = VC._exported(hip, imp.g)
        ctgs = PagSeqs(len(ctg_len), None, ctg_len.ctypes.data, None, 0)
        prm = TravelParams(spec["threads"], 0, 2 * spec["epsilon"], 0.15, 0.90, 50)
        assert hip.pag_travel_prepare(imp.g, C.byref(ctgs), ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
        return csr, SG.device_records(hip, imp.g), imp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", REGION_KINDS)
@pytest.mark.parametrize("which", SHIFTS)
def test_c_shard_select_keeps_the_region_and_marks_its_ends(which, kind, workdir, monkeypatch):
    for s in SG.SWITCHES + ("PAG_ORDER_SLICES",):
        monkeypatch.delenv(s, raising=False)
    g0 = succ_rule.load_graph(NAME)[0]
    dc, dr = hc.deltas(which, g0["ctg"], g0["ref"])
    g = hc.shift(g0, dc, dr)
    spec = goldens.load_spec(NAME)
    civ, riv, ropen, placed = _region(kind, dc, dr)
    label = f"{NAME} shift {which} [{kind}]"
    whole = _whole(g)
    cut = VC._cut_of(whole, civ, riv)
    assert 0 < cut["keep"].sum() < len(cut["keep"]), f"{label}: the region keeps {cut['keep'].sum()} of {len(cut['keep'])} vertices"
    if kind == "ends on vertices":
        for iv, x in ((civ, whole["ctg"][whole["ctg"] != 0]), (riv, whole["ref"][whole["ctg"] == 0])):
            assert np.isin(iv, x).all(), f"{label}: an interval end is on no vertex"
    if kind == "ends a margin away":
        assert min(placed) > 0, f"{label}: (hi - r == margin, r - lo == margin - 1, r - lo == margin) placed {placed} times"
    if kind == "open end at 2^32 - 1":
        assert int(riv[-1]) == 0xFFFFFFFF and ropen[-1] == 1
    lengths = input_lengths(NAME, workdir)
    hip = pagctl.hip_lib()
    csr, (off, recs, code, pos), _ = _select_and_prepare(g, civ, riv, ropen, lengths, dc, dr)
    # the imported cut is the rule's cut, vertex for vertex
    VC._first_diff(label, "nodes of the imported graph", csr["node_code"], cut["nodes"])
    for a, b in (("pos_ctg", "ctg"), ("pos_ref", "ref")):
        VC._first_diff(label, a, csr[a], cut[b], lambda i: f"vertex (code, ctg, ref) = ({int(cut['code'][i])}, {int(cut['ctg'][i])}, {int(cut['ref'][i])})")
    # the prepared graph: the coordinate order, the poison and marker records the rule names, every other list the rule's restricted
    deviation = 2 * spec["epsilon"]
    ref = SG.reference_of_rule(g, *succ_rule.successors(g, np.arange(len(g["ctg"])), deviation, 0.15))
    vpos = (cut["ctg"].astype(np.uint64) << np.uint64(32)) | cut["ref"].astype(np.uint64)
    perm, n_zero = R.order(vpos)
    VC._first_diff(label, "k-mer of the vertices in coordinate order", code, cut["code"][perm])
    VC._first_diff(label, "position of the vertices in coordinate order", pos, vpos[perm])
    on_contig = np.arange(len(perm)) >= n_zero
    max_step = int((cut["estep"].astype(np.int64) & R.EDGE_STEP_MASK).max())
    inc = R.incomplete(cut["ref"][perm], on_contig, riv, ropen, R.margin_of(max_step, 0.15, deviation))
    grade = (recs[:, 2].astype(np.int64) >> 24) & 7
    owner = np.repeat(np.arange(len(perm)), np.diff(off))
    poisoned, marked = np.zeros(len(perm), dtype=bool), np.zeros(len(perm), dtype=bool)
    poisoned[owner[grade == 7]] = True
    marked[owner[grade == 6]] = True
    VC._first_diff(label, "poison records (coordinate-free vertices whose successors may lie outside the bands)", poisoned, inc & ~on_contig)
    VC._first_diff(label, "marker records (vertices with a contig coordinate whose reference coordinate is off the bands)", marked, inc & on_contig)
    if placed is not None:  # (the case is there for them: both kinds, and vertices without)
        assert 0 < poisoned.sum() < (~on_contig).sum() and 0 < marked.sum() < on_contig.sum(), f"{label}: the regions decide nothing"
    got = SG.check_against_reference(ref, off, recs, code, pos, False, label)
    assert got["poisoned"] == int(poisoned.sum()) and got["markers"] == int(marked.sum())
    if which != "low":  # the device's own answer below 2^31, translated: the same cut, order, marks and records
        l_civ, l_riv, l_ropen, _ = _region(kind, 0, 0)
        if kind == "open end at 2^32 - 1":
            l_riv = l_riv.copy()
            l_riv[-1] = 0xFFFFFFFF - dr  # (the translated band's end; open either way)
        l_csr, (l_off, l_recs, l_code, l_pos), _ = _select_and_prepare(g0, l_civ, l_riv, l_ropen, lengths, 0, 0)
        assert np.array_equal(off, l_off) and np.array_equal(code, l_code), f"{label}: offsets or codes differ from the low run"
        VC._first_diff(label, "positions against the low run's translated", pos, hc.pos(l_pos, dc, dr))
        want = l_recs.copy()
        want[:, 1] = hc.coord(l_recs[:, 1], dc)
        bad = np.flatnonzero((recs != want).any(axis=1))
        assert len(bad) == 0, f"{label}: record {int(bad[0])} is {recs[bad[0]].tolist()}, the low run's translated {want[bad[0]].tolist()}; {len(bad)} differ"
