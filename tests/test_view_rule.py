"""CPU: tests/view_rule.py — the numpy statement of the cut that tests/test_gpu_view_cut.py holds the kernels to — against the same
rule written as plain loops over small random inputs, and its contig tables against parallel.regions_for."""
import numpy as np
import pytest

import view_rule as R
from aligngraph2_amd import parallel


def _inside(x, iv):
    return any(iv[2 * i] <= x < iv[2 * i + 1] for i in range(len(iv) // 2))


def _tables(rng, n, hi):
    pts = np.sort(rng.choice(np.arange(1, hi), size=2 * n, replace=False)).reshape(-1, 2)
    if n > 1:
        pts[1, 0] = pts[0, 1]  # (two that touch)
    return pts.astype(np.uint32).reshape(-1)


@pytest.mark.parametrize("seed", range(6))
def test_compact_equals_the_loops(seed):
    rng = np.random.default_rng(seed)
    civ, riv = (_tables(rng, 5, 60), _tables(rng, 4, 60)) if seed % 3 else (np.zeros(0, np.uint32), _tables(rng, 4, 60))
    whole = seed == 5
    tkey, tval, tseg, tcnt = [], [], [], []
    codes = np.sort(rng.choice(64, size=20, replace=False))
    for code in codes:
        L = int(rng.integers(1, 9))
        nl = int(rng.integers(0, L + 1))
        for j in range(L):
            tkey.append(code)
            tval.append((0 if j < nl // 2 else int(rng.integers(1, 64))) << 32 | int(rng.integers(0, 64)))
            tseg.append(nl if j == 0 else (R.SEG_LEADER | j if j < nl else 0))
            tcnt.append(int(rng.integers(0, 65536)))
    ekey, ev, eseg = [], [], []
    for code in np.sort(rng.choice(64, size=25, replace=False)):
        L = int(rng.integers(1, 5))
        nu = int(rng.integers(0, L + 1))
        for j in range(L):
            ekey.append(code)
            ev.append(int(rng.integers(0, 64)) << 32 | int(rng.integers(0, 1 << 25)))
            eseg.append(nu if j == 0 else 0)
    got = R.compact(np.array(tkey, np.uint32), np.array(tval, np.uint64), np.array(tseg, np.uint32), np.array(tcnt, np.uint16),
                    np.array(ekey, np.uint32), np.array(ev, np.uint64), np.array(eseg, np.uint32), civ, riv, whole)
    # ---- the loops
    vpos, vcnt, vnode, ncode, npos_off = [], [], [], [], []
    for i in range(len(tkey)):
        head = i == 0 or tkey[i - 1] != tkey[i]
        leader = tseg[i] != 0 if head else bool(tseg[i] & R.SEG_LEADER)
        c, r = tval[i] >> 32, tval[i] & 0xFFFFFFFF
        if not leader or not (whole or (_inside(c, civ) if c else _inside(r, riv))):
            continue
        if not ncode or ncode[-1] != tkey[i]:
            ncode.append(tkey[i])
            npos_off.append(len(vpos))
        vpos.append(tval[i])
        vcnt.append(tcnt[i])
        vnode.append(len(ncode) - 1)
    npos_off.append(len(vpos))
    nedge_off, eto, estep = [0], [], []
    for n, code in enumerate(ncode):
        heads = [j for j in range(len(ekey)) if ekey[j] == code and (j == 0 or ekey[j - 1] != code)]
        for j in heads:
            for v in ev[j:j + eseg[j]]:
                t, step = v >> 32, ((v & 0xFFFFFFFF) >> 1) & 0xFFFFFF
                if t in ncode:
                    m = ncode.index(t)
                    eto.append(npos_off[m])
                    estep.append(step | min(npos_off[m + 1] - npos_off[m], 255) << 24)
                else:
                    eto.append(R.PAG_NONE)
                    estep.append(step)
        nedge_off.append(len(eto))
    want = {"vpos": vpos, "vcnt": vcnt, "vnode": vnode, "ncode": ncode, "npos_off": npos_off, "nedge_off": nedge_off, "eto": eto, "estep": estep}
    for name, w in want.items():
        assert got[name].tolist() == [int(x) for x in w], name
    assert got["counts"] == (len(ncode), len(vpos), len(eto))
    # kept() on the leaders says the same
    lead = R.leaders(np.array(tkey, np.uint32), np.array(tseg, np.uint32))
    if not whole:
        tv = np.array(tval, np.uint64)[lead]
        keep, nodes = R.kept(np.array(tkey)[lead], tv >> np.uint64(32), tv & np.uint64(0xFFFFFFFF), civ, riv)
        assert tv[keep].tolist() == vpos and nodes.tolist() == [int(x) for x in ncode]


def test_node_with_255_positions_and_more():
    for n, q in ((254, 254), (255, 255), (256, 255), (700, 255)):
        tkey = np.full(n, 3, np.uint32)
        tseg = np.where(np.arange(n) == 0, n, R.SEG_LEADER | np.arange(n)).astype(np.uint32)
        got = R.compact(tkey, np.arange(1, n + 1, dtype=np.uint64), tseg, np.ones(n, np.uint16), np.array([9], np.uint32),
                        np.array([(3 << 32) | (17 << 1) | 1], np.uint64), np.array([1], np.uint32), None, None, True)
        assert got["counts"] == (1, n, 0)  # (k-mer 9 owns no node: its edge is not taken)
        got = R.compact(tkey, np.arange(1, n + 1, dtype=np.uint64), tseg, np.ones(n, np.uint16), np.array([3], np.uint32),
                        np.array([(3 << 32) | (17 << 1) | 1], np.uint64), np.array([1], np.uint32), None, None, True)
        assert got["eto"].tolist() == [0] and got["estep"].tolist() == [17 | q << 24]


def test_order_and_incomplete_equal_the_loops():
    rng = np.random.default_rng(3)
    vpos = (np.where(rng.random(300) < 0.4, 0, rng.integers(1, 40, size=300)).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 40, size=300).astype(np.uint64)
    perm, n_zero = R.order(vpos)
    want = sorted(range(300), key=lambda v: (1, int(vpos[v]) >> 32, v) if int(vpos[v]) >> 32 else (0, int(vpos[v]) & 0xFFFFFFFF, v))
    assert perm.tolist() == want and n_zero == int(((vpos >> np.uint64(32)) == 0).sum())
    riv = np.array([10, 20, 20, 26, 30, 38], np.uint32)
    ropen = np.array([1, 0, 0, 1, 1, 1], np.uint8)
    ref = np.arange(0, 45)
    for margin in (0, 1, 3, 100):
        for on_contig in (False, True):
            got = R.incomplete(ref, np.full(len(ref), on_contig), riv, ropen, margin)
            for r in ref:
                bad = True
                for i in range(3):
                    lo, hi = int(riv[2 * i]), int(riv[2 * i + 1])
                    if lo <= r < hi:
                        bad = bool((ropen[2 * i] and r - lo < margin) or (ropen[2 * i + 1] and hi - r <= margin))
                if on_contig and r == 0:
                    bad = False
                assert got[r] == bad, (margin, on_contig, r)
    assert R.incomplete(ref, np.zeros(len(ref), bool), np.zeros(0, np.uint32), np.zeros(0, np.uint8), 5).all()
    assert R.margin_of(1000, 0.15, 20) == 1150 + 22 and R.margin_of(0, 0.15, 0) == 2


def test_zone_bands_equal_the_loops():
    rng = np.random.default_rng(4)
    zones = np.array([5, 9, 9, 12, 20, 21, 30, 40], np.uint32)
    tval = (rng.integers(0, 45, size=400).astype(np.uint64) << np.uint64(32)) | np.where(rng.random(400) < 0.2, 0, rng.integers(1, 99, size=400)).astype(np.uint64)
    tval = tval[(tval >> np.uint64(32)) != 20]  # (a zone without a position)
    lo, hi = R.zone_bands(tval, zones)
    for z in range(4):
        r = [int(p) & 0xFFFFFFFF for p in tval if zones[2 * z] <= int(p) >> 32 < zones[2 * z + 1] and int(p) & 0xFFFFFFFF]
        assert (int(lo[z]), int(hi[z])) == ((min(r), max(r)) if r else (0xFFFFFFFF, 0))
    assert (int(lo[2]), int(hi[2])) == (0xFFFFFFFF, 0)


@pytest.mark.parametrize("orient", [[1, 0, -1, 2], [2, 2, 2, 2], [-1, -1, 1, -1]])
def test_view_tables_state_the_contig_rule_of_regions_for(orient):
    ctg_len = [5000, 731, 12000, 64]
    assert R.mapper_starts(ctg_len) == parallel.mapper_starts(ctg_len)[:-1]
    civ, zones = R.view_tables(ctg_len, orient, 0.90)
    walked = [c for c in range(4) if orient[c] >= 0]
    assert civ.tolist() == parallel.regions_for([walked], ctg_len, orient, [], [1000])[0]["ctg_iv"].tolist()
    st = R.mapper_starts(ctg_len)
    assert len(zones) == sum({-1: 0, 0: 1, 1: 1, 2: 2}[o] for o in orient)
    for lo, hi in zones:  # a zone ends with its strand and begins max(4000, 3 %) before 90 % of it (at its start when that is more)
        c, rev = next((c, rev) for c in range(4) for rev in (0, 1) if st[c] + 2 * rev * ctg_len[c] + ctg_len[c] == hi)
        left = st[c] + 2 * rev * ctg_len[c]
        assert lo == left + max(0, int(ctg_len[c] * 0.9) - max(4000, int(ctg_len[c] * 0.03)))
    tight = R.view_tables(ctg_len, orient, 0.90, 50)[1]
    assert all(b[1] == a[1] and b[0] >= a[0] for a, b in zip(zones, tight))
