"""The cut of the traversal graph, stated once more and independently of the device code (numpy only, no device).

The traversal walks a CUT of the finished graph: this handle's own view (pag_travel_prepare_for -> trav_view_region ->
trav_compact, k5_view.hip) or one rank's region of a sharded build (pag_shard_select, k_select.hip).  Both rest on DESIGN.md 3
"The view": the cut keeps exactly the vertices whose coordinate lies in its interval tables, with all edges of the k-mers that
keep a vertex, and it is never silently wrong — a coordinate-free vertex within a successor's reach of an open band end
carries a poison record, a strand vertex whose reference coordinate lies in no band a marker record.  This module is that
rule in a page; tests/test_gpu_view_cut.py holds the kernels to it vertex by vertex.

Interval tables are flat arrays of sorted, disjoint [lo, hi) pairs, as the C ABI takes them (pag_region)."""
import numpy as np

PAG_NONE = 0xFFFFFFFF
SEG_LEADER = 0x80000000
EDGE_STEP_MASK = 0xFFFFFF
EDGE_Q_MANY = 255


def in_intervals(x, iv):
    """x[i] lies in one of the [lo, hi) pairs of iv (lo in, hi out)"""
    x = np.asarray(x, dtype=np.int64)
    iv = np.asarray(iv, dtype=np.int64).reshape(-1, 2)
    if len(iv) == 0:
        return np.zeros(len(x), dtype=bool)
    j = np.searchsorted(iv[:, 0], x, side="right") - 1  # last pair with lo <= x
    jj = np.maximum(j, 0)
    return (j >= 0) & (x < iv[jj, 1])


def kept(code, ctg, ref, civ, riv):
    """which vertices (code, ctg, ref) a cut with the tables civ / riv keeps, and its nodes (ascending codes)"""
    ctg = np.asarray(ctg)
    keep = np.where(ctg != 0, in_intervals(ctg, civ), in_intervals(ref, riv))
    return keep, np.unique(np.asarray(code)[keep])


def leaders(tkey, tseg):
    """the slots of a slice that hold a vertex: a segment head with tseg != 0, a later slot with SEG_LEADER set"""
    tkey, tseg = np.asarray(tkey), np.asarray(tseg)
    head = np.ones(len(tkey), dtype=bool)
    head[1:] = tkey[1:] != tkey[:-1]
    return np.where(head, tseg != 0, (tseg & np.uint32(SEG_LEADER)) != 0)


def compact(tkey, tval, tseg, tcnt, ekey, eval_, eseg, civ, riv, whole):
    """what trav_compact must make of slice-layout arrays: dict(vpos, vcnt, vnode, ncode, npos_off, nedge_off, eto, estep,
    counts = (nodes, vertices, edges))"""
    tkey, tval, tcnt = np.asarray(tkey, dtype=np.uint32), np.asarray(tval, dtype=np.uint64), np.asarray(tcnt, dtype=np.uint16)
    ekey, eval_, eseg = np.asarray(ekey, dtype=np.uint32), np.asarray(eval_, dtype=np.uint64), np.asarray(eseg, dtype=np.uint32)
    keep = leaders(tkey, tseg)
    if not whole:
        keep &= kept(tkey, tval >> np.uint64(32), tval & np.uint64(0xFFFFFFFF), civ, riv)[0]
    vpos, vcnt, vcode = tval[keep], tcnt[keep], tkey[keep]
    ncode, first, vnode = np.unique(vcode, return_index=True, return_inverse=True)  # (the slice is ascending in the code)
    n_nodes, n_pos = len(ncode), len(vpos)
    npos_off = np.concatenate([first, [n_pos]]).astype(np.uint32)
    # edges: the segments (eseg at the head = how many unique edges follow it) of the codes that own a node
    ehead = np.ones(len(ekey), dtype=bool)
    ehead[1:] = ekey[1:] != ekey[:-1]
    hj = np.flatnonzero(ehead)
    hn = np.searchsorted(ncode, ekey[hj])
    own = (hn < n_nodes) & (ncode[np.minimum(hn, max(n_nodes - 1, 0))] == ekey[hj]) if n_nodes else np.zeros(len(hj), dtype=bool)
    hj, hn = hj[own], hn[own]
    lens = eseg[hj].astype(np.int64)
    necnt = np.zeros(n_nodes + 1, dtype=np.int64)
    necnt[hn] = lens
    nedge_off = np.concatenate([[0], np.cumsum(necnt[:n_nodes])]).astype(np.uint32)
    n_edges = int(lens.sum())
    src = np.repeat(hj - (np.cumsum(lens) - lens), lens) + np.arange(n_edges)
    ev = eval_[src]
    step = ((ev & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).astype(np.uint32) & np.uint32(EDGE_STEP_MASK)
    tcode = (ev >> np.uint64(32)).astype(np.uint32)
    tn = np.searchsorted(ncode, tcode)
    has = (tn < n_nodes) & (ncode[np.minimum(tn, max(n_nodes - 1, 0))] == tcode) if n_nodes else np.zeros(n_edges, dtype=bool)
    tn = np.where(has, tn, 0)
    q = (npos_off[tn + 1].astype(np.int64) - npos_off[tn]) if n_nodes else np.zeros(n_edges, dtype=np.int64)
    eto = np.where(has, npos_off[tn] if n_nodes else 0, PAG_NONE).astype(np.uint32)
    estep = np.where(has, step | (np.minimum(q, EDGE_Q_MANY).astype(np.uint32) << np.uint32(24)), step).astype(np.uint32)
    return {"vpos": vpos, "vcnt": vcnt, "vnode": vnode.astype(np.uint32), "ncode": ncode, "npos_off": npos_off, "nedge_off": nedge_off,
            "eto": eto, "estep": estep, "counts": (n_nodes, n_pos, n_edges)}


def order(vpos):
    """the coordinate order of the view's vertices: new id -> k-mer-major id, [ctg == 0 by ref] ++ [the rest by ctg], equal keys
    in k-mer-major order; and the size of the first group"""
    vpos = np.asarray(vpos, dtype=np.uint64)
    ctg, ref = (vpos >> np.uint64(32)).astype(np.int64), (vpos & np.uint64(0xFFFFFFFF)).astype(np.int64)
    free, rest = np.flatnonzero(ctg == 0), np.flatnonzero(ctg != 0)
    return np.concatenate([free[np.argsort(ref[free], kind="stable")], rest[np.argsort(ctg[rest], kind="stable")]]), len(free)


def margin_of(max_step, err, dev):
    """how far a successor's coordinate can lie from its source's (checkPosition): max_step over the CUT graph's edges"""
    return min(int(float(max_step) * (1.0 + err)) + int(dev) + 2, 0x7FFFFFFF)


def incomplete(ref, on_contig, riv, ropen, margin):
    """the vertices whose successors may lie outside the bands riv (ropen[2 i], [2 i + 1]: the graph goes on beyond that end): the
    reference coordinate lies in no band, or within `margin` of an open end — r - lo < margin at a low end, hi - r <= margin at a
    high one.  A vertex with a contig coordinate and no reference coordinate has no successor found through one."""
    r = np.asarray(ref, dtype=np.int64)
    on_contig = np.asarray(on_contig, dtype=bool)
    iv = np.asarray(riv, dtype=np.int64).reshape(-1, 2)
    op = np.asarray(ropen, dtype=bool).reshape(-1, 2)
    if len(iv) == 0:
        bad = np.ones(len(r), dtype=bool)
    else:
        j = np.searchsorted(iv[:, 0], r, side="right") - 1
        jj = np.maximum(j, 0)
        inside = (j >= 0) & (r < iv[jj, 1])
        near = (op[jj, 0] & (r - iv[jj, 0] < margin)) | (op[jj, 1] & (iv[jj, 1] - r <= margin))
        bad = ~inside | near
    return bad & ~(on_contig & (r == 0))


def zone_bands(tval, zones):
    """per zone (flat [lo, hi) pairs of contig coordinates): lowest / highest reference coordinate among the slots whose contig
    coordinate lies in it, slots without a reference coordinate aside; (all ones, 0) for a zone without one"""
    tval = np.asarray(tval, dtype=np.uint64)
    z = np.asarray(zones, dtype=np.int64).reshape(-1, 2)
    c, r = (tval >> np.uint64(32)).astype(np.int64), (tval & np.uint64(0xFFFFFFFF)).astype(np.int64)
    lo, hi = np.full(len(z), 0xFFFFFFFF, dtype=np.int64), np.zeros(len(z), dtype=np.int64)
    if len(z):
        j = np.searchsorted(z[:, 0], c, side="right") - 1
        ok = (j >= 0) & (c < z[np.maximum(j, 0), 1]) & (r != 0)
        np.minimum.at(lo, j[ok], r[ok])
        np.maximum.at(hi, j[ok], r[ok])
    return lo.astype(np.uint32), hi.astype(np.uint32)


def mapper_starts(lengths):
    """PositionMapper: sequence i's forward strand begins at starts[i], its reverse strand at starts[i] + 2 len"""
    st = []
    for i, n in enumerate(lengths):
        st.append(int(n) if i == 0 else st[-1] + 3 * int(lengths[i - 1]) + max(int(lengths[i - 1]), int(n)))
    return st


def merge(ivs):
    out = []
    for lo, hi in sorted(ivs):
        if hi <= lo:
            continue
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def view_tables(ctg_len, orient, start_split, view_margin=None):
    """the contig side of a handle's own view: the contig intervals (landing zone — the first 1 - start_split — of EVERY strand, and
    the strands orient walks: 1 forward, 0 reverse, 2 both) and the zones (from view_margin — default: 3 % of the contig, at
    least 4000 — before start_split of a walked strand to its end) whose vertices say which reference bands the view takes.
    Returns (civ flat u32, zones as a sorted list of (lo, hi))."""
    st = mapper_starts(ctg_len)
    civ, zones = [], []
    for c, n in enumerate(ctg_len):
        n = int(n)
        z = min(n, int(float(n) * (1.0 - start_split)) + 2)
        for rev in (0, 1):
            left = st[c] + (2 * n if rev else 0)
            civ.append((left, left + z))
            if not (orient[c] == 2 or (orient[c] == 1 and not rev) or (orient[c] == 0 and rev)):
                continue
            civ.append((left, left + n))
            split = int(float(n) * start_split)
            m = max(4000, int(float(n) * 0.03)) if view_margin is None else int(view_margin)
            zones.append((left + (split - m if split > m else 0), left + n))
    return np.array(merge(civ), dtype=np.uint32).reshape(-1), sorted(zones)
