"""GPU: the cut of the traversal graph held to its rule, vertex by vertex.

The traversal walks a cut of the finished graph: this handle's own view (pag_travel_prepare_for -> trav_view_region ->
trav_compact, k5_view.hip) or one rank's region of a sharded build (pag_shard_select, k_select.hip).  tests/view_rule.py states
in numpy what such a cut keeps, how its vertices are ordered and which of them carry a poison / marker record (DESIGN.md 3
"The view"); every comparison here is exact:

  (a) k_zone_bands through pag_debug_zone_bands on constructed slots: the LDS reduction and the global atomics (more than 2 048
      zones), both ends of a zone, positions outside every zone, slots without a reference coordinate, an empty zone;
  (b) trav_compact through pag_debug_trav_compact on constructed slice-layout arrays: every tile count around one tile, segments
      that cross tile boundaries in each way k_view_mark tells apart (counted on the numpy side before the device is asked), one
      segment over three tiles, more tiles than the grid has blocks, interval tables in LDS and in global memory, edges through
      the code table (k = 14) and through the three gathers (k = 15, 16);
  (c) pag_shard_select + pag_shard_import + pag_shard_set_region on golden graphs with regions the test chooses (interval ends
      on vertex coordinates, 3 000 contig intervals, 300 / 200 reference bands with mixed open ends: k_mark_incomplete's bit per
      vertex and the bands in LDS): the imported graph, the coordinate order, where poison and marker records stand, and every
      other list against the reference's succ.txt.gz;
  (d) the handle's own view (pag_travel_prepare_for): the tables pag_debug_view_region reports against view_rule.view_tables and
      parallel.regions_for, its bands against the zones' vertices, then the checks of (c) with those tables."""
import ctypes as C
import time

import numpy as np
import pytest

import goldens
import pagctl
import test_gpu_succ_golden as SG
import view_rule as R
from aligngraph2_amd import parallel
from aligngraph2_amd.capi import PagRawInput, PagSeqs, Region, TravelParams

TILE = 2048  # slots a block of k_view_mark / k_view_write takes at a time (VC_TILE)
GRID = 2048  # blocks of their grid at most
U32 = np.uint64(0xFFFFFFFF)


def _ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


def _first_diff(label, what, got, want, describe=None):
    """np.array_equal or an AssertionError that names the first difference"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    m = min(len(got), len(want))
    d = np.flatnonzero(got[:m] != want[:m])
    at = int(d[0]) if len(d) else m
    where = f" ({describe(at)})" if describe and at < len(want) else ""
    raise AssertionError(f"{label}: {what} differs ({len(got)} entries, the rule has {len(want)}); first at {at}{where}: device "
                         f"{got[at:at + 4].tolist()} rule {want[at:at + 4].tolist()}")


# =====================================================================================================================
# (a) k_zone_bands
# =====================================================================================================================
def _zone_case(rng, n_z, T):
    """zones over the contig coordinates [100, ..): zone 1 touches zone 0, one zone is left without a position; positions below the
    first zone, at and beyond the end of the last, on both ends of zones, and without a reference coordinate"""
    pts = np.sort(rng.choice(np.arange(100, 100 + 6 * n_z + 50), size=2 * n_z, replace=False)).astype(np.int64)
    zones = pts.reshape(-1, 2).copy()
    if n_z >= 2:
        zones[1, 0] = zones[0, 1]
    c = rng.integers(0, zones[-1, 1] + 60, size=T).astype(np.int64)
    r = rng.integers(1, 1 << 20, size=T).astype(np.int64)
    r[rng.random(T) < 0.1] = 0
    if T == 1:
        c[0], r[0] = zones[0, 0], 7
    else:
        ends = rng.choice(T, size=min(T, 64), replace=False)
        zi = rng.integers(0, n_z, size=len(ends))
        c[ends] = zones[zi, np.arange(len(ends)) % 2]  # (lo: in the zone; hi: out of it, in the next one where they touch)
        c[ends[-1]] = zones[-1, 1]  # (the end of the last zone: out)
        r[ends[:len(ends) // 2]] |= 1
    empty = n_z // 2 if n_z >= 3 else -1
    if empty >= 0:
        c[(c >= zones[empty, 0]) & (c < zones[empty, 1])] = 0
    tval = (c.astype(np.uint64) << np.uint64(32)) | r.astype(np.uint64)
    return tval, zones.astype(np.uint32).reshape(-1), empty


@pytest.mark.gpu
@pytest.mark.parametrize("n_z", [1, 2048, 2049, 5000])
def test_zone_bands_equal_the_rule(n_z):
    hip = pagctl.hip_lib()
    rng = np.random.default_rng(1000 + n_z)
    for T in (1, 255, 257, 100_000):
        tval, zones, empty = _zone_case(rng, n_z, T)
        want_lo, want_hi = R.zone_bands(tval, zones)
        if T == 100_000:  # what the case is there for, counted before the device is asked
            z = zones.reshape(-1, 2).astype(np.int64)
            c, r = (tval >> np.uint64(32)).astype(np.int64), (tval & U32).astype(np.int64)
            live = r != 0
            assert (np.isin(c, z[:, 0]) & live).any() and (np.isin(c, z[:, 1]) & live).any(), "no position on a zone's ends"
            assert ((c < z[0, 0]) & live).any() and ((c >= z[-1, 1]) & live).any(), "no position outside all zones"
            assert (~live & R.in_intervals(c, zones)).any(), "no slot without a reference coordinate inside a zone"
            if empty >= 0:
                assert want_lo[empty] == 0xFFFFFFFF and want_hi[empty] == 0, "the empty zone is not empty"
                assert z[1, 0] == z[0, 1] and (want_hi[:2] != 0).all(), "the touching zones are not both taken"
            assert (want_hi != 0).sum() > n_z // 2
        lo, hi = np.full(n_z, 12345, dtype=np.uint32), np.full(n_z, 12345, dtype=np.uint32)
        rc = hip.pag_debug_zone_bands(tval.ctypes.data, T, zones.ctypes.data, n_z, lo.ctypes.data, hi.ctypes.data, 0)
        assert rc == 0, hip.pag_last_error()
        label = f"{n_z} zones, {T} slots"
        _first_diff(label, "lowest reference coordinate per zone", lo, want_lo, lambda z_: f"zone {zones[2 * z_:2 * z_ + 2].tolist()}")
        _first_diff(label, "highest reference coordinate per zone", hi, want_hi, lambda z_: f"zone {zones[2 * z_:2 * z_ + 2].tolist()}")


# =====================================================================================================================
# (b) trav_compact
# =====================================================================================================================
CRANGE = 8192  # coordinates of the constructed vertices: [0, CRANGE) on either side — few values, so that interval ends are hit


def _codes(rng, k, n):
    """n distinct ascending k-mer codes, the first and the last code of the 4^k among them"""
    space = 1 << (2 * k)
    assert n <= space - 2
    if n < 2:
        return rng.integers(0, space, size=n).astype(np.uint32)
    inner = rng.choice(space - 2, size=n - 2, replace=False) if space <= (1 << 24) else np.unique(rng.integers(0, space - 2, size=2 * n + 16))
    inner = np.sort(rng.choice(inner, size=n - 2, replace=False)) + 1
    return np.concatenate([[0], inner, [space - 1]]).astype(np.uint32)


def _make_slice(rng, k, seg_lens, all_leaders=()):
    """slice-layout tuple arrays: segment s has seg_lens[s] slots, its leaders first (tseg: their number at the head,
    SEG_LEADER | offset behind it, 0 on the other slots), the coordinate-free leaders first among them; the other slots hold
    positions too (members of the clusters), which the compaction must not take"""
    L = np.asarray(seg_lens, dtype=np.int64)
    S, T = len(L), int(L.sum())
    codes = _codes(rng, k, S)
    assert len(codes) == S
    start = np.cumsum(L) - L
    seg = np.repeat(np.arange(S), L)
    off = np.arange(T) - start[seg]
    nl = np.where(rng.random(S) < 0.8, L, (rng.random(S) * (L + 1)).astype(np.int64))
    nl[list(all_leaders)] = L[list(all_leaders)]
    nfree = (nl * rng.random(S) * 0.6).astype(np.int64)
    c = rng.integers(1, CRANGE, size=T).astype(np.uint64)
    c[off < nfree[seg]] = 0
    c[(off >= nl[seg]) & (rng.random(T) < 0.3)] = 0
    r = rng.integers(1, CRANGE, size=T).astype(np.uint64)
    r[rng.random(T) < 0.02] = 0
    tseg = np.where(off == 0, nl[seg], np.where(off < nl[seg], R.SEG_LEADER | off, 0)).astype(np.uint32)
    return {"k": k, "tkey": codes[seg], "tval": (c << np.uint64(32)) | r, "tseg": tseg, "tcnt": rng.integers(0, 65536, size=T).astype(np.uint16),
            "start": start, "len": L, "nl": nl, "codes": codes}


def _make_edges(rng, sl, n_src):
    """slice-layout edge arrays: segments of 1..6 records whose first eseg[head] are the unique edges; sources with and without
    tuples; targets among the k-mers with the most leaders (nodes with >= 255 positions), any k-mer with tuples, k-mers without"""
    k, codes, nl = sl["k"], sl["codes"], sl["nl"]
    space = 1 << (2 * k)
    absent = np.setdiff1d(np.unique(rng.integers(0, space, size=64)), codes).astype(np.uint32)
    src = np.unique(np.concatenate([rng.choice(codes, size=min(n_src, len(codes)), replace=False), absent[:8]])).astype(np.uint32)
    Ls = rng.integers(1, 7, size=len(src))
    nu = np.minimum(Ls, rng.integers(0, 7, size=len(src)))
    E = int(Ls.sum())
    seg = np.repeat(np.arange(len(src)), Ls)
    off = np.arange(E) - (np.cumsum(Ls) - Ls)[seg]
    big = codes[np.argsort(-nl, kind="stable")[:6]]
    pick = rng.random(E)
    tgt = np.where(pick < 0.3, rng.choice(big, size=E), np.where(pick < 0.85, rng.choice(codes, size=E), rng.choice(absent, size=E))).astype(np.uint64)
    step = np.where(rng.random(E) < 0.1, rng.integers(0, 1 << 24, size=E), rng.integers(0, 2000, size=E)).astype(np.uint64)
    step[rng.random(E) < 0.02] = 0xFFFFFF
    return {"ekey": src[seg], "eval": (tgt << np.uint64(32)) | (step << np.uint64(1)) | rng.integers(0, 2, size=E).astype(np.uint64),
            "eseg": np.where(off == 0, nu[seg], 0).astype(np.uint32)}


def _random_iv(rng, n, lo=1, hi=CRANGE):
    """n sorted disjoint [lo, hi) pairs with ends in [lo, hi), about one in ten touching its successor"""
    pts = np.sort(rng.choice(np.arange(lo, hi), size=2 * n, replace=False)).reshape(-1, 2)
    touch = np.flatnonzero(rng.random(n - 1) < 0.1) if n > 1 else np.zeros(0, dtype=np.int64)
    pts[touch + 1, 0] = pts[touch, 1]
    return pts.astype(np.uint32).reshape(-1)


def _tables(rng, kind):
    """(civ, riv) of a cut, None for the whole graph"""
    e = np.zeros(0, dtype=np.uint32)
    if kind == "whole":
        return None
    if kind == "1+1":
        return np.array([CRANGE // 4, CRANGE // 2], dtype=np.uint32), np.array([CRANGE // 3, 2 * CRANGE // 3], dtype=np.uint32)
    if kind == "no civ":
        return e, _random_iv(rng, 50)
    if kind == "no riv":
        return _random_iv(rng, 50), e
    if kind == "nothing":
        return np.array([CRANGE + 10, CRANGE + 20], dtype=np.uint32), np.array([CRANGE + 10, CRANGE + 20], dtype=np.uint32)
    a, b = (int(x) for x in kind.split("+"))
    return _random_iv(rng, a), _random_iv(rng, b)


ALL_TABLES = ["whole", "1+1", "1000+1000", "1500+1500", "no civ", "no riv", "nothing"]
# 2 (n_civ + n_riv) interval ends against the 4 096 k_view_mark keeps in LDS: the last table that fits and the first that does not
THRESHOLD_TABLES = ["1024+1024", "1024+1025"]


def _run_compact(hip, sl, ed, tables):
    """pag_debug_trav_compact -> the arrays of view_rule.compact"""
    T, E = len(sl["tkey"]), len(ed["ekey"])
    whole = tables is None
    if whole:  # (the graph's own counts, as pag_process's statistics give them to the compaction: exact)
        nn, npos, ne = R.compact(sl["tkey"], sl["tval"], sl["tseg"], sl["tcnt"], ed["ekey"], ed["eval"], ed["eseg"], None, None, True)["counts"]
    else:      # (upper bounds: every leader, every k-mer with one, every unique edge)
        nn, npos, ne = int((sl["nl"] > 0).sum()), int(sl["nl"].sum()), int(ed["eseg"].sum())
    out = {"vpos": np.zeros(npos, np.uint64), "vcnt": np.zeros(npos, np.uint16), "vnode": np.zeros(npos, np.uint32), "ncode": np.zeros(nn, np.uint32),
           "npos_off": np.zeros(nn + 1, np.uint32), "nedge_off": np.zeros(nn + 1, np.uint32), "eto": np.zeros(ne, np.uint32), "estep": np.zeros(ne, np.uint32)}
    counts = (C.c_uint64 * 3)(nn, npos, ne)
    region = None
    if not whole:
        civ, riv = tables
        region = Region(len(civ) // 2, _ptr(civ), len(riv) // 2, _ptr(riv), None)
    rc = hip.pag_debug_trav_compact(sl["k"], _ptr(sl["tkey"]), _ptr(sl["tval"]), _ptr(sl["tseg"]), _ptr(sl["tcnt"]), T, _ptr(ed["ekey"]), _ptr(ed["eval"]),
                                    _ptr(ed["eseg"]), E, C.byref(region) if region is not None else None, *[_ptr(out[n]) for n in
                                    ("vpos", "vcnt", "vnode", "ncode")], out["npos_off"].ctypes.data, out["nedge_off"].ctypes.data, _ptr(out["eto"]),
                                    _ptr(out["estep"]), counts, 0)
    assert rc == 0, hip.pag_last_error()
    n = tuple(int(x) for x in counts)
    got = {"counts": n, "vpos": out["vpos"][:n[1]], "vcnt": out["vcnt"][:n[1]], "vnode": out["vnode"][:n[1]], "ncode": out["ncode"][:n[0]],
           "npos_off": out["npos_off"][:n[0] + 1], "nedge_off": out["nedge_off"][:n[0] + 1], "eto": out["eto"][:n[2]], "estep": out["estep"][:n[2]]}
    return got


def _check_compact(hip, sl, ed, tables, label):
    civ, riv = tables if tables is not None else (None, None)
    want = R.compact(sl["tkey"], sl["tval"], sl["tseg"], sl["tcnt"], ed["ekey"], ed["eval"], ed["eseg"], civ, riv, tables is None)
    got = _run_compact(hip, sl, ed, tables)

    def vertex(i):
        p = int(want["vpos"][i])
        return f"vertex (code, ctg, ref) = ({int(want['ncode'][want['vnode'][i]])}, {p >> 32}, {p & 0xFFFFFFFF})"

    def node(i):
        return f"node of code {int(want['ncode'][min(i, len(want['ncode']) - 1)])}" if len(want["ncode"]) else "no node"

    def edge(i):
        n = int(np.searchsorted(want["nedge_off"], i, side="right")) - 1
        return f"edge {i - int(want['nedge_off'][n])} of code {int(want['ncode'][n])}"

    for name in ("vpos", "vcnt", "vnode"):
        _first_diff(label, name, got[name], want[name], vertex)
    for name in ("ncode", "npos_off", "nedge_off"):
        _first_diff(label, name, got[name], want[name], node)
    for name in ("eto", "estep"):
        _first_diff(label, name, got[name], want[name], edge)
    assert got["counts"] == want["counts"], f"{label}: (nodes, vertices, edges) {got['counts']}, the rule has {want['counts']}"
    return want


def _random_lens(rng, T, hi=300):
    out, left = [], T
    while left:
        out.append(min(left, int(rng.integers(1, hi + 1))))
        left -= out[-1]
    return out


def _crossings_layout(rng, n_bound=36):
    """segment lengths with, at every tile boundary B, a segment placed across it: (segment, kind = boundary % 4, head slot)"""
    lens, special, pos = [], [], 0
    for b in range(1, n_bound + 1):
        B, kind = b * TILE, b % 4
        d, L = {0: (5, 12), 1: (5, 12), 2: (1, 6), 3: (4, 9)}[kind]
        lens += _random_lens(rng, B - d - pos)
        special.append((len(lens), kind, B - d, L, b))
        lens.append(L)
        pos = B - d + L
    return lens + _random_lens(rng, 700), special


def _place_crossings(sl, special, civ, riv):
    """the coordinates of the placed segments under the tables (civ, riv), so that what they keep is
      kind 0: nothing in the head's tile, the first kept vertex in the next one (its slot 0 or 2);
      kind 1: one vertex in the head's tile and one in the next;
      kind 2: the head is the last slot of its tile (kept or not), the next tile keeps vertices;
      kind 3: one vertex alone, slot 0 of the next tile.
    Vertices outside are coordinate-free ones outside riv (they sort first) or ones with a contig coordinate outside civ."""
    c_all, r_all = np.arange(1, CRANGE), np.arange(1, CRANGE)
    c_in, c_out = c_all[R.in_intervals(c_all, civ)], c_all[~R.in_intervals(c_all, civ)]
    r_out = r_all[~R.in_intervals(r_all, riv)]
    if not len(c_in) or not len(c_out) or not len(r_out):
        return False
    tval = sl["tval"]
    for s, kind, h, L, b in special:
        B = h + {0: 5, 1: 5, 2: 1, 3: 4}[kind]
        keep = np.zeros(L, dtype=bool)
        if kind == 0:
            keep[B - h + (0 if b % 8 < 4 else 2):] = True
        elif kind == 1:
            keep[[B - 3 - h, B + 1 - h]] = True
        elif kind == 2:
            keep[1:] = True
            keep[0] = b % 8 >= 4
        else:
            keep[B - h] = True
        free_out = (b // 4) % 2 == 1  # (every other one: what is left out before the first kept vertex has no contig coordinate)
        first = int(np.flatnonzero(keep)[0])
        for j in range(L):
            if keep[j]:
                c, r = int(c_in[(7 * b + j) % len(c_in)]), 1 + (b + j) % 50
            elif free_out and j < first:
                c, r = 0, int(r_out[(5 * b + j) % len(r_out)])
            else:
                c, r = int(c_out[(3 * b + j) % len(c_out)]), 1 + (b + 2 * j) % 50
            tval[h + j] = (c << 32) | r
    return True


def _crossing_counts(sl, civ, riv):
    """segments, under the cut (civ, riv), in each situation k_view_mark tells apart at a tile boundary"""
    tkey, tval = sl["tkey"], sl["tval"]
    keep = R.leaders(tkey, sl["tseg"]) & R.kept(tkey, tval >> np.uint64(32), tval & U32, civ, riv)[0]
    T = len(tkey)
    seg = np.repeat(np.arange(len(sl["len"])), sl["len"])
    head = sl["start"][seg]
    tile, head_tile = np.arange(T) // TILE, head // TILE
    S = len(sl["len"])
    first_kept = np.full(S, T, dtype=np.int64)
    np.minimum.at(first_kept, seg[keep], np.flatnonzero(keep))
    in_head_tile = np.zeros(S, dtype=bool)
    in_head_tile[seg[keep & (tile == head_tile)]] = True
    later = np.zeros(S, dtype=bool)
    later[seg[keep & (tile > head_tile)]] = True
    return {"the head's tile keeps nothing, the next keeps the first vertex": int(((first_kept < T) & (first_kept // TILE > sl["start"] // TILE)).sum()),
            "the head's tile keeps one and so does the next": int((in_head_tile & later).sum()),
            "the head is the last slot of a tile": int(((sl["start"] % TILE == TILE - 1) & later).sum()),
            "a kept leader behind its head is slot 0 of a tile": int((keep & (np.arange(T) % TILE == 0) & (np.arange(T) != head)).sum())}


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2047, 2048, 2049])
def test_compact_around_one_tile(T):
    hip = pagctl.hip_lib()
    rng = np.random.default_rng(2000 + T)
    sl = _make_slice(rng, 6, _random_lens(rng, T, hi=40))
    ed = _make_edges(rng, sl, 60)
    for kind in ALL_TABLES:
        _check_compact(hip, sl, ed, _tables(rng, kind), f"T = {T}, k = 6, tables {kind}")


def _five_tiles(rng, k):
    lens = _random_lens(rng, 5 * TILE - 254 - 255 - 256 + 33)
    at = len(lens) // 2
    lens[at:at] = [254, 255, 256]  # (all leaders: target nodes with 254, 255 = EDGE_Q_MANY and 256 positions)
    sl = _make_slice(rng, k, lens, all_leaders=(at, at + 1, at + 2))
    return sl, _make_edges(rng, sl, 1500)


@pytest.mark.gpu
def test_compact_five_tiles_every_table():
    hip = pagctl.hip_lib()
    rng = np.random.default_rng(2100)
    sl, ed = _five_tiles(rng, 7)
    assert len(sl["tkey"]) == 5 * TILE + 33 and sl["len"].max() <= 300
    for kind in ALL_TABLES + THRESHOLD_TABLES:
        want = _check_compact(hip, sl, ed, _tables(rng, kind), f"5 tiles, k = 7, tables {kind}")
        if kind == "nothing":
            assert want["counts"] == (0, 0, 0)
        elif kind != "whole":
            assert 0 < want["counts"][1] < sl["nl"].sum()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [14, 15, 16])
def test_compact_edges_with_and_without_the_code_table(k):
    """The five-tile case with k-mers of k = 14 (targets through the direct table over the 4^k codes), k = 15 and k = 16 (no table:
    bitmap word, rank, position range — three dependent gathers).  Most of a case is its scratch (the bitmap, the rank directory and
    the scans over them: 2 GB of table at k = 14, 1.5 GB of bitmap, ranks and scans at k = 16).  Measured on the MI355X: 0.01 s for
    the three tables of a case at every k, k = 16 included (printed by the test)."""
    hip = pagctl.hip_lib()
    rng = np.random.default_rng(2200 + k)
    sl, ed = _five_tiles(rng, k)
    assert int(sl["codes"][0]) == 0 and int(sl["codes"][-1]) == 4 ** k - 1
    t0 = time.time()
    for kind in ("whole", "1000+1000", "1500+1500"):
        want = _check_compact(hip, sl, ed, _tables(rng, kind), f"5 tiles, k = {k}, tables {kind}")
        q = want["estep"][want["eto"] != R.PAG_NONE] >> np.uint32(24)
        assert (want["eto"] == R.PAG_NONE).any(), "no edge whose target has no node"
        if kind == "whole":
            npos = np.diff(want["npos_off"].astype(np.int64))
            assert {254, 255, 256} <= set(npos.tolist()) and npos.max() > 255, "no target node around EDGE_Q_MANY positions"
            assert (q == 254).any() and (q == 255).any() and (q < 254).any()
    print(f"k = {k}: {time.time() - t0:.2f} s for three tables")


@pytest.mark.gpu
def test_compact_one_segment_over_three_tiles():
    hip = pagctl.hip_lib()
    rng = np.random.default_rng(2300)
    lens = _random_lens(rng, 1000) + [5000]
    at = len(lens) - 1
    lens += _random_lens(rng, 1200)
    sl = _make_slice(rng, 6, lens, all_leaders=(at,))
    h = int(sl["start"][at])
    assert h // TILE == 0 and (h + 4999) // TILE == 2 and sl["nl"][at] == 5000
    ed = _make_edges(rng, sl, 60)
    for kind in ALL_TABLES:
        _check_compact(hip, sl, ed, _tables(rng, kind), f"a segment of 5 000 leaders, tables {kind}")


@pytest.mark.gpu
def test_compact_segments_across_tile_boundaries():
    """Segments placed across 36 tile boundaries in the four ways k_view_mark's first-of-its-segment test tells apart (the tile's own
    prefix of the keep flags; the slots before the tile re-tested through global memory), at least 8 of each — counted from the
    rule's keep flags before the device is asked."""
    hip = pagctl.hip_lib()
    rng = np.random.default_rng(2400)
    lens, special = _crossings_layout(rng)
    sl = _make_slice(rng, 8, lens, all_leaders=[s for s, *_ in special])
    ed = _make_edges(rng, sl, 400)
    for kind in ("1+1", "1000+1000", "1500+1500", "no riv"):
        civ, riv = _tables(rng, kind)
        assert _place_crossings(sl, special, civ, riv), f"tables {kind}: no coordinate inside / outside to place"
        for what, n in _crossing_counts(sl, civ, riv).items():
            assert n >= 8, f"tables {kind}: only {n} segments where {what}"
        _check_compact(hip, sl, ed, (civ, riv), f"36 tile boundaries, tables {kind}")
    _check_compact(hip, sl, ed, None, "36 tile boundaries, whole")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["1000+1000", "1500+1500"])
def test_compact_more_tiles_than_blocks(kind):
    """T = 2 049 x 2 048 + 5 slots: 2 050 tiles on a grid of 2 048 blocks, so two blocks take a second tile; the interval tables in LDS
    (1 000 + 1 000) and in global memory (1 500 + 1 500).  Measured on the MI355X machine: 0.6 s a case, nearly all of it numpy (the
    slots and the rule); 0.01 s in the hook, uploads and downloads included (printed by the test)."""
    hip = pagctl.hip_lib()
    rng = np.random.default_rng(2500)
    T = 2049 * TILE + 5
    assert (T + TILE - 1) // TILE > GRID
    sl = _make_slice(rng, 8, _random_lens(rng, T))
    ed = _make_edges(rng, sl, 5000)
    civ, riv = _tables(rng, kind)
    t0 = time.time()
    got = _run_compact(hip, sl, ed, (civ, riv))
    print(f"{T} slots, tables {kind}: {time.time() - t0:.2f} s in the hook (uploads and downloads included); {got['counts']}")
    _check_compact(hip, sl, ed, (civ, riv), f"{T} slots, tables {kind}")


# =====================================================================================================================
# (c), (d): golden graphs
# =====================================================================================================================
GOLDENS = ["succ_corners_t8", "two_blocks_both_orient_t16"]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _loaded_inputs():
    yield
    for blocks in _cache.values():
        for blk in blocks:
            blk["inp"].close()
    _cache.clear()


def _golden(name, workdir):
    """per config block of a golden: its loaded input, lengths, orientations, the reference's records, the plain build's CSR"""
    if name in _cache:
        return _cache[name]
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / "view_cut" / name / "in"))
    refs = SG.reference_blocks(name)
    ctg_names = [ln[1:].split()[0] for ln in open(f"{ind}/ctg.fasta") if ln.startswith(">")]
    hip = pagctl.hip_lib()
    blocks = []
    for b, ref in enumerate(refs):
        inp = pagctl.LoadedInput(ind, threads=spec["threads"], eps=spec["epsilon"], cov=spec["cov"], block=b)
        raw = PagRawInput.from_address(inp.raw_view)
        ctg_len = np.ctypeslib.as_array(C.cast(raw.ctg_len, C.POINTER(C.c_uint32)), shape=(raw.n_ctgs,)).copy()
        ref_len = np.ctypeslib.as_array(C.cast(raw.ref_len, C.POINTER(C.c_uint32)), shape=(raw.n_refs,)).copy()
        g = pagctl.hip_create(inp)
        try:
            csr = pagctl.run_on(g, inp)["csr"]
        finally:
            hip.pag_destroy(g)
        blocks.append({"name": name, "block": b, "spec": spec, "inp": inp, "ctg_len": ctg_len, "ref_len": ref_len, "ref": ref,
                       "orient": SG.block_orient(ind, b, ctg_names), "csr": csr, "whole": _vertices(csr)})
    _cache[name] = blocks
    return blocks


def _vertices(csr):
    """a CSR's vertices and edges as flat arrays (code, ctg, ref, cnt per vertex; source code, target, step per edge)"""
    return {"code": np.repeat(csr["node_code"], np.diff(csr["pos_off"].astype(np.int64))), "ctg": csr["pos_ctg"], "ref": csr["pos_ref"], "cnt": csr["pos_cnt"],
            "ecode": np.repeat(csr["node_code"], np.diff(csr["edge_off"].astype(np.int64))), "eto": csr["edge_to"], "estep": csr["edge_step"]}


def _cut_of(whole, civ, riv):
    """what a cut with the tables (civ, riv) keeps of the whole graph's vertices and edges (view_rule.kept)"""
    keep, nodes = R.kept(whole["code"], whole["ctg"], whole["ref"], civ, riv)
    ekeep = np.isin(whole["ecode"], nodes)
    return {"keep": keep, "nodes": nodes, "code": whole["code"][keep], "ctg": whole["ctg"][keep], "ref": whole["ref"][keep], "cnt": whole["cnt"][keep],
            "ecode": whole["ecode"][ekeep], "eto": whole["eto"][ekeep], "estep": whole["estep"][ekeep]}


def _exported(hip, g):
    nn, npos, ne = C.c_uint64(), C.c_uint64(), C.c_uint64()
    hip.pag_csr_sizes(g, C.byref(nn), C.byref(npos), C.byref(ne))
    out = {"node_code": np.zeros(nn.value, np.uint32), "pos_off": np.zeros(nn.value + 1, np.uint64), "pos_ctg": np.zeros(npos.value, np.uint32),
           "pos_ref": np.zeros(npos.value, np.uint32), "pos_cnt": np.zeros(npos.value, np.uint16), "edge_off": np.zeros(nn.value + 1, np.uint64),
           "edge_to": np.zeros(ne.value, np.uint32), "edge_step": np.zeros(ne.value, np.int32)}
    csr = pagctl.Csr(nn.value, npos.value, ne.value, *[out[k].ctypes.data for k in ("node_code", "pos_off", "pos_ctg", "pos_ref", "pos_cnt", "edge_off",
                                                                                     "edge_to", "edge_step")])
    assert hip.pag_export_csr(g, C.byref(csr)) == 0, hip.pag_last_error()
    return out


def _margin(cut, blk):
    max_step = int((cut["estep"].astype(np.int64) & R.EDGE_STEP_MASK).max()) if len(cut["estep"]) else 0
    return R.margin_of(max_step, 0.15, 2 * blk["spec"]["epsilon"])


def _check_prepared(hip, g, blk, cut, riv, ropen, label, need_marks=False):
    """the prepared traversal graph of a cut: its vertices in the rule's order, a poison record exactly on the coordinate-free
    vertices the rule names, a marker record exactly on the named vertices with a contig coordinate (behind their list), every
    other list the reference's restricted to the kept targets"""
    off, recs, code, pos = SG.device_records(hip, g)
    vpos = (cut["ctg"].astype(np.uint64) << np.uint64(32)) | cut["ref"].astype(np.uint64)
    perm, n_zero = R.order(vpos)

    def vertex(u):
        v = perm[u]
        return f"new id {u}: vertex (code, ctg, ref) = ({int(cut['code'][v])}, {int(cut['ctg'][v])}, {int(cut['ref'][v])})"

    _first_diff(label, "k-mer of the vertices in coordinate order", code, cut["code"][perm], vertex)
    _first_diff(label, "position of the vertices in coordinate order", pos, vpos[perm], vertex)
    on_contig = np.arange(len(perm)) >= n_zero
    assert np.array_equal(on_contig, cut["ctg"][perm] != 0)
    inc = R.incomplete(cut["ref"][perm], on_contig, riv, ropen, _margin(cut, blk))
    grade = (recs[:, 2].astype(np.int64) >> 24) & 7
    owner = np.repeat(np.arange(len(perm)), np.diff(off))
    poisoned, marked = np.zeros(len(perm), dtype=bool), np.zeros(len(perm), dtype=bool)
    poisoned[owner[grade == 7]] = True
    marked[owner[grade == 6]] = True
    _first_diff(label, "poison records (coordinate-free vertices whose successors may lie outside the bands)", poisoned, inc & ~on_contig, vertex)
    _first_diff(label, "marker records (vertices with a contig coordinate whose reference coordinate is off the bands)", marked, inc & on_contig, vertex)
    if need_marks:  # (the case is there for them: both kinds, and vertices without)
        free = ~on_contig
        assert 0 < poisoned.sum() < free.sum() and 0 < marked.sum() < on_contig.sum(), \
            f"{label}: {poisoned.sum()} of {free.sum()} poisoned, {marked.sum()} of {on_contig.sum()} marked: the regions decide nothing"
    got = SG.check_against_reference(blk["ref"], off, recs, code, pos, False, label)
    assert got["poisoned"] == int(poisoned.sum()) and got["markers"] == int(marked.sum())
    return got


def _travel_args(blk):
    ctgs = PagSeqs(len(blk["ctg_len"]), None, blk["ctg_len"].ctypes.data, None, 0)
    prm = TravelParams(blk["spec"]["threads"], 0, 2 * blk["spec"]["epsilon"], 0.15, 0.90, 50)
    return ctgs, prm


def _pin_ends(blk, civ, riv, ropen):
    """the outer band ends placed on the edge of the rule: the first band's low end open, exactly margin - 1 before one
    coordinate-free vertex and so margin before the next (r - lo < margin: within reach; == margin: out of it), its high end
    closed; the last band's high end open, exactly margin beyond the last coordinate-free vertex (hi - r <= margin: still within
    reach), its low end closed.  The margin follows from the cut graph's longest step, which the bands themselves can change:
    placed, then counted again.  Returns the bands, the flags and how often each of the three distances occurs."""
    whole = blk["whole"]
    riv = riv.astype(np.int64).reshape(-1, 2).copy()
    ropen = ropen.copy()
    ropen[[0, 1, -2, -1]] = [1, 0, 0, 1]
    ur = np.unique(whole["ref"][(whole["ctg"] == 0) & (whole["ref"] != 0)]).astype(np.int64)
    r1, r_last = int(riv[0, 0]), int(ur[-1])
    assert r1 in ur and r1 + 1 in ur and r1 + 1 < riv[0, 1], "the first band does not begin with two coordinate-free vertices on consecutive reference coordinates"
    for _ in range(6):
        m = _margin(_cut_of(whole, civ, riv.astype(np.uint32).reshape(-1)), blk)
        new = (r1 - (m - 1), r_last + m)
        if (int(riv[0, 0]), int(riv[-1, 1])) == new:
            break
        riv[0, 0], riv[-1, 1] = new
    assert 1 <= riv[0, 0] < riv[0, 1] and riv[-1, 0] < riv[-1, 1] < (1 << 32)
    riv32 = riv.astype(np.uint32).reshape(-1)
    cut = _cut_of(whole, civ, riv32)
    m = _margin(cut, blk)
    r = cut["ref"][cut["ctg"] == 0].astype(np.int64)
    j = np.searchsorted(riv[:, 0], r, side="right") - 1
    op = ropen.reshape(-1, 2).astype(bool)
    lo, hi, olo, ohi = riv[j, 0], riv[j, 1], op[j, 0], op[j, 1]
    return riv32, ropen, (int((ohi & (hi - r == m)).sum()), int((olo & (r - lo == m - 1)).sum()), int((olo & (r - lo == m)).sum()))


def _regions(blk, kind):
    """(civ, riv, ropen, placed ends) of the region `kind` for a golden block"""
    whole = blk["whole"]
    ctg_len, ref_len, orient = [int(x) for x in blk["ctg_len"]], [int(x) for x in blk["ref_len"]], [int(x) for x in blk["orient"]]
    walked = [c for c in range(len(ctg_len)) if orient[c] >= 0]
    rst = parallel.mapper_starts(ref_len)
    # where a contig maps to: the forward-strand reference coordinates of the vertices on its strands
    cst = parallel.mapper_starts(ctg_len)
    alns = []
    for c in walked:
        on = (whole["ctg"] >= cst[c]) & (whole["ctg"] < cst[c] + 3 * ctg_len[c]) & (whole["ref"] != 0)
        for ri, n in enumerate(ref_len):
            r = whole["ref"][on & (whole["ref"] >= rst[ri]) & (whole["ref"] < rst[ri] + n)].astype(np.int64)
            if len(r):
                alns.append((c, ri, int(r.min()) - rst[ri], int(r.max()) + 1 - rst[ri]))
    base = parallel.regions_for([walked[:1], walked[1:]], ctg_len, orient, alns, ref_len, halo=300)[0]
    civ0, riv0, ropen0 = base["ctg_iv"].copy(), base["ref_iv"].copy(), base["ref_open"].copy()
    uc = np.unique(whole["ctg"][whole["ctg"] != 0]).astype(np.int64)
    ur = np.unique(whole["ref"][(whole["ctg"] == 0) & (whole["ref"] != 0)]).astype(np.int64)
    if kind == "regions_for":
        return civ0, riv0, ropen0, None
    if kind == "ends on vertices":  # (a vertex at lo is in, a vertex at hi is out)
        ci = [len(uc) // 10, 3 * len(uc) // 10, len(uc) // 2, 7 * len(uc) // 10]
        ri = [len(ur) // 8, 3 * len(ur) // 8, 5 * len(ur) // 8, 7 * len(ur) // 8]
        return uc[ci].astype(np.uint32), ur[ri].astype(np.uint32), np.array([1, 0, 0, 1], dtype=np.uint8), None
    if kind == "3000 contig intervals":
        stride = (int(uc[-1]) - int(uc[0])) // 3000
        assert stride >= 3
        lo = int(uc[0]) + np.arange(3000, dtype=np.int64) * stride
        civ = np.stack([lo, lo + max(1, stride // 2)], axis=1).astype(np.uint32).reshape(-1)
        return civ, riv0, ropen0, None
    n = int(kind.split()[0])  # "300 bands" / "200 bands": over the coordinate-free vertices' stretch, every other end open or not
    base = int(ur[:-1][np.diff(ur) == 1][0])  # (the first two coordinate-free vertices on consecutive reference coordinates: see _pin_ends)
    stride = (int(ur[-1]) + 1 - base) // n
    assert stride >= 4
    lo = base + np.arange(n, dtype=np.int64) * stride
    riv = np.stack([lo, lo + (3 * stride) // 4 + 1], axis=1).astype(np.uint32).reshape(-1)
    ropen = np.random.default_rng(n).integers(0, 2, size=2 * n).astype(np.uint8)
    riv, ropen, placed = _pin_ends(blk, civ0, riv, ropen)
    return civ0, riv, ropen, placed


REGION_KINDS = ["regions_for", "ends on vertices", "3000 contig intervals", "300 bands", "200 bands"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", REGION_KINDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_shard_select_keeps_the_region_and_marks_its_ends(name, kind, workdir, monkeypatch):
    """One owner builds the block (parallel.ShardedBuild, a world of one), pag_shard_select cuts it to a region the test chooses,
    the cut is imported and its region set: the imported graph is the rule's cut of the plain build's graph, array for array, and
    the prepared traversal graph orders and marks it as the rule says.  300 bands: more than a successor kernel stages in LDS
    (INC_LDS_MAX = 256), so k_mark_incomplete's bit per vertex is what the records are made from; 200: the bands in LDS."""
    for s in SG.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    hip = pagctl.hip_lib()
    for blk in _golden(name, workdir):
        label = f"{name} block {blk['block']} [{kind}]"
        civ, riv, ropen, placed = _regions(blk, kind)
        if placed is not None:
            assert min(placed) > 0, f"{label}: (hi - r == margin, r - lo == margin - 1, r - lo == margin) placed {placed} times"
        cut = _cut_of(blk["whole"], civ, riv)
        assert 0 < cut["keep"].sum() < len(cut["keep"]), f"{label}: the region keeps {cut['keep'].sum()} of {len(cut['keep'])} vertices"
        if kind == "ends on vertices":
            w = blk["whole"]
            for iv, x in ((civ, w["ctg"][w["ctg"] != 0]), (riv, w["ref"][w["ctg"] == 0])):
                assert np.isin(iv, x).all(), f"{label}: an interval end is on no vertex"
        region = Region(len(civ) // 2, _ptr(civ), len(riv) // 2, _ptr(riv), _ptr(ropen))
        g = pagctl.hip_create(blk["inp"])
        try:
            prepared = pagctl._prepared_view(hip, g, blk["inp"])
            sb = parallel.ShardedBuild(hip, g, prepared, 0, 1, "cuda")
            counts, tuples, edges = sb.extract()
            allc = counts[None]
            rt, t1 = parallel.exchange_stream(tuples, allc[:, :, 0:2], 0, 1, peers=[tuples])
            re_, e1 = parallel.exchange_stream(edges, allc[:, :, 2:4], 0, 1, peers=[edges])
            sb.build(rt, t1, re_, e1, prepared.eps)
            sl, st = sb.select({"region": region})
            sb.import_all([sl], [st])
            sb.set_region({"region": region})
            got = _exported(hip, g)
            kcode = cut["code"]

            def vertex(i):
                return f"vertex (code, ctg, ref) = ({int(kcode[i])}, {int(cut['ctg'][i])}, {int(cut['ref'][i])})"

            _first_diff(label, "nodes of the imported graph", got["node_code"], cut["nodes"])
            for a, b in (("pos_ctg", "ctg"), ("pos_ref", "ref"), ("pos_cnt", "cnt")):
                _first_diff(label, a, got[a], cut[b], vertex)
            _first_diff(label, "pos_off", got["pos_off"], np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(cut["nodes"], kcode), minlength=len(cut["nodes"])))]))
            _first_diff(label, "edge_off", got["edge_off"], np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(cut["nodes"], cut["ecode"]), minlength=len(cut["nodes"])))]))
            _first_diff(label, "edge_to", got["edge_to"], cut["eto"], lambda i: f"an edge of code {int(cut['ecode'][i])}")
            _first_diff(label, "edge_step", got["edge_step"], cut["estep"], lambda i: f"an edge of code {int(cut['ecode'][i])}")
            ctgs, prm = _travel_args(blk)
            assert hip.pag_travel_prepare(g, C.byref(ctgs), blk["ref_len"].ctypes.data, len(blk["ref_len"]), C.byref(prm), None) == 0, hip.pag_last_error()
            _check_prepared(hip, g, blk, cut, riv, ropen, label, need_marks=placed is not None)
        finally:
            hip.pag_destroy(g)


VIEW_MODES = [("default", {}, 100_000, None), ("tight", {"PAG_VIEW_HALO": "300", "PAG_VIEW_MARGIN": "50"}, 300, 50)]


def _strands(ref_len):
    """[lo, hi) of every reference strand in the single-coordinate space (forward at the start, reverse two lengths on)"""
    rst = parallel.mapper_starts([int(x) for x in ref_len])
    out = []
    for i, n in enumerate(ref_len):
        out += [(rst[i], rst[i] + int(n)), (rst[i] + 2 * int(n), rst[i] + 3 * int(n))]
    return sorted(out)


def _band_of(zone_lo, zone_hi, whole, halo, strands, eps):
    """[min ref - halo, max ref + halo + 1) of the vertices with a contig coordinate in [zone_lo, zone_hi) (and a reference
    coordinate), clipped to the strands the two ends lie on, every coordinate widened by eps; None: no such vertex"""
    m = (whole["ctg"] >= max(zone_lo - eps, 1)) & (whole["ctg"] < zone_hi + eps) & (whole["ref"] != 0)
    if not m.any():
        return None
    lo, hi = int(whole["ref"][m].min()) - eps, int(whole["ref"][m].max()) + eps
    s_lo = next((a for a, b in strands if a <= lo + eps < b), 0)
    s_hi = next((b for a, b in strands if a <= hi - eps < b), 1 << 32)
    return max(lo - halo, s_lo), min(hi + halo + 1, s_hi)


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True], ids=["as configured", "one contig both ways"])
@pytest.mark.parametrize("mode", VIEW_MODES, ids=[m[0] for m in VIEW_MODES])
@pytest.mark.parametrize("name", GOLDENS)
def test_the_handle_s_own_view_is_the_rule_s_cut(name, mode, both, workdir, monkeypatch):
    """pag_travel_prepare_for with the block's orientations (and with one contig set to PAG_ORIENT_BOTH), default and tight margins.

    The tables (pag_debug_view_region): civ is view_rule.view_tables' and parallel.regions_for's with every contig dealt to one
    rank; ropen says "this band end is not a strand end".  The bands come from k_zone_bands, which reads EVERY tuple slot of the
    built graph, not the leaders alone.  What K3 (k34_segments.hip) leaves behind a segment's leaders are tuples of the same
    k-mer, each within epsilon of a leader of that segment on both coordinates (pos_sim) — of a leader that may itself lie just
    outside the zone.  So a band must CONTAIN [min ref - halo, max ref + halo + 1) of the zone's vertices, clipped to their
    reference strand, and may exceed it by no more than what the vertices within epsilon of the zone, their reference coordinates
    widened by epsilon, would give; both are asserted.  Then, with the device's own tables, the checks of the regional graph: kept
    set, order, poison and marker placement, every list."""
    for s in SG.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    _, env, halo, view_margin = mode
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    hip = pagctl.hip_lib()
    for blk in _golden(name, workdir):
        label = f"{name} block {blk['block']} [{mode[0]}{', both' if both else ''}]"
        orient = blk["orient"].copy()
        if both:
            orient[int(np.flatnonzero(orient >= 0)[0])] = 2
        whole, eps = blk["whole"], blk["spec"]["epsilon"]
        ctg_len, ref_len = blk["ctg_len"], blk["ref_len"]
        g = pagctl.hip_create(blk["inp"])
        try:
            prepared = pagctl._prepared_view(hip, g, blk["inp"])
            st = pagctl.BuildStats()
            assert hip.pag_process(g, C.byref(prepared), C.byref(st)) == 0, hip.pag_last_error()
            cap = 4096
            civ, riv, ropen, sizes = np.zeros(2 * cap, np.uint32), np.zeros(2 * cap, np.uint32), np.zeros(2 * cap, np.uint8), (C.c_uint64 * 2)()
            rc = hip.pag_debug_view_region(g, ctg_len.ctypes.data, len(ctg_len), orient.ctypes.data, ref_len.ctypes.data, len(ref_len), 0.90,
                                           civ.ctypes.data, riv.ctypes.data, ropen.ctypes.data, sizes, cap)
            assert rc == 0, hip.pag_last_error()
            civ, riv, ropen = civ[:2 * sizes[0]].copy(), riv[:2 * sizes[1]].copy(), ropen[:2 * sizes[1]].copy()
            # ---- the contig side: one rule, stated three times
            want_civ, zones = R.view_tables(ctg_len, orient, 0.90, view_margin)
            _first_diff(label, "contig intervals against view_rule.view_tables", civ, want_civ)
            walked = [c for c in range(len(ctg_len)) if orient[c] >= 0]
            by_ranks = parallel.regions_for([walked], [int(x) for x in ctg_len], [int(x) for x in orient], [], [int(x) for x in ref_len])[0]["ctg_iv"]
            _first_diff(label, "contig intervals against parallel.regions_for", civ, by_ranks)
            # ---- the bands
            bands = riv.astype(np.int64).reshape(-1, 2)
            assert (bands[:, 0] < bands[:, 1]).all() and (bands[1:, 0] > bands[:-1, 1]).all(), f"{label}: bands not sorted and disjoint: {bands.tolist()}"
            strands = _strands(ref_len)
            least = [b for b in (_band_of(lo, hi, whole, halo, strands, 0) for lo, hi in zones) if b]
            most = R.merge([b for b in (_band_of(lo, hi, whole, halo, strands, eps) for lo, hi in zones) if b])
            assert least, f"{label}: no zone has a vertex with a reference coordinate"
            for lo, hi in least:
                assert ((bands[:, 0] <= lo) & (hi <= bands[:, 1])).any(), f"{label}: no band contains [{lo}, {hi}) of a zone's vertices: {bands.tolist()}"
            for lo, hi in bands:
                assert any(a <= lo and hi <= b for a, b in most), f"{label}: the band [{lo}, {hi}) exceeds what the zones' tuples can give: {most}"
            starts, ends = {a for a, _ in strands}, {b for _, b in strands}
            want_open = np.array([[lo not in starts, hi not in ends] for lo, hi in bands], dtype=np.uint8).reshape(-1)
            _first_diff(label, "open band ends", ropen, want_open, lambda i: f"band {bands[i // 2].tolist()}")
            # ---- the cut itself, with the device's tables
            ctgs, prm = _travel_args(blk)
            rc = hip.pag_travel_prepare_for(g, C.byref(ctgs), orient.ctypes.data, ref_len.ctypes.data, len(ref_len), C.byref(prm), None)
            assert rc == 0, hip.pag_last_error()
            cut = _cut_of(whole, civ, riv)
            got = _check_prepared(hip, g, blk, cut, riv, ropen, label)
            n = [C.c_uint64() for _ in range(3)]
            is_cut = C.c_int()
            assert hip.pag_travel_view_sizes(g, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), None, C.byref(is_cut), None) == 0
            assert is_cut.value == 1 and (n[0].value, n[1].value, n[2].value) == (len(cut["nodes"]), int(cut["keep"].sum()), len(cut["eto"])), label
            if mode[0] == "tight":
                assert got["vertices"] < len(whole["code"]), f"{label}: the tight view kept every vertex"
        finally:
            hip.pag_destroy(g)
