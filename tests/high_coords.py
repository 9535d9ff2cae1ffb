"""Translation of a graph along the coordinate axes (plain numpy, no test, no device).

Every contig and reference coordinate is a u32 "single coordinate", a vertex position is ctg << 32 | ref, and the rules compute
differences that wrap around in 32 bits.  Adding one constant to every non-zero contig coordinate and another to every non-zero
reference coordinate changes no rule's answer except by that constant, as long as no sum passes 2^32: the differences are the
same, zero stays "no coordinate", and the order inside a k-mer's segment is the same (zero sorts first, the rest keep theirs).
So a small graph the suite already trusts can be moved to where the top bit is set, and every kernel asked there for the answer
the rule gives.

The shifts (SHIFTS): `low` the control, `straddle` puts the middle vertex on 2^31, `upper` adds 0xC0000000, `top` puts the
largest coordinate on 2^32 - 1 — a WRAP case: a step from there passes 2^32, so only the rule evaluated on the shifted arrays
is its yardstick, never the translated `low` answer."""
import numpy as np

TOP_BIT, NONE32, SPACE = 1 << 31, 0xFFFFFFFF, 1 << 32
SHIFTS = ("low", "straddle", "upper", "top")
WRAP = {"top"}  # the shifts exempt from "the device's own answer on the unshifted graph, with the constant added back"


def coord(x, d, wrap=False):
    """non-zero coordinates (array or scalar) moved by d; zero stays zero.  Nothing may reach 2^32 unless the case is a wrap case"""
    a = np.asarray(x).astype(np.int64)
    out = np.where(a != 0, a + int(d), 0)
    assert wrap or (out.size == 0) or (int(out.max()) < SPACE and int(out.min()) >= 0), "a shifted coordinate leaves the 32-bit space"
    out = out & NONE32
    return out.astype(np.uint32) if isinstance(x, np.ndarray) else int(out)


def bound(x, d):
    """an interval end, a hull end, a strand range's end: 0 (none) and all ones (open, or an empty hull's low end) stay"""
    x = int(x)
    if x in (0, NONE32):
        return x
    assert 0 <= x + int(d) < SPACE, "a shifted bound leaves the 32-bit space"
    return x + int(d)


def shift(g, dc, dr, wrap=False):
    """a succ_rule.load_graph dict with ctg / ref translated where non-zero (a copy: the arrays of g are left alone)"""
    out = dict(g)
    out["ctg"], out["ref"] = coord(g["ctg"], dc, wrap), coord(g["ref"], dr, wrap)
    return out


def pos(p, dc, dr, wrap=False):
    """packed positions ctg << 32 | ref (array or int) translated"""
    a = np.asarray(p, dtype=np.uint64)
    c = coord((a >> np.uint64(32)).astype(np.uint32).reshape(-1), dc, wrap).astype(np.uint64)
    r = coord((a & np.uint64(NONE32)).astype(np.uint32).reshape(-1), dr, wrap).astype(np.uint64)
    out = ((c << np.uint64(32)) | r).reshape(a.shape)
    return out if isinstance(p, np.ndarray) else int(out)


def name(code_pos, dc, dr, wrap=False):
    """a (code, pos) name translated"""
    return (int(code_pos[0]), pos(int(code_pos[1]), dc, dr, wrap))


def intervals(iv, d):
    """a pag_region table (flat [lo, hi) pairs, u32) translated; an end of 0 or all ones stays"""
    return np.array([bound(x, d) for x in np.asarray(iv).reshape(-1).tolist()], dtype=np.uint32)


def frame_kwargs(kw, dc):
    """the coordinates of a walk frame (walk_straight_rule.Frame's keyword arguments: both strand ranges, both hulls) translated;
    split_size is a size, leap_min a ratio, excl holds vertices: they stay"""
    out = dict(kw)
    for f in ("ctg_left", "ctg_right", "rev_left", "rev_right"):
        if f in out:
            out[f] = bound(out[f], dc)
    if "hulls" in out:
        out["hulls"] = tuple((bound(lo, dc), bound(hi, dc)) for lo, hi in out["hulls"])
    return out


def leading_lengths(d, lengths):
    """sequence lengths whose PositionMapper layout is that of `lengths` moved up by d: two leading sequences, never walked, of
    lengths L1 >= L2 with 1 <= L2 <= 5 <= lengths[0] (start of lengths[0] = 5 L1 + 3 L2 + lengths[0], so d = 5 L1 + 3 L2)"""
    lengths = [int(x) for x in lengths]
    d = int(d)
    if d == 0:
        return lengths
    assert lengths[0] >= 5 and d >= 40
    l2 = next(x for x in range(1, 6) if (d - 3 * x) % 5 == 0)
    l1 = (d - 3 * l2) // 5
    assert l1 >= l2 and l1 < SPACE
    return [l1, l2] + lengths


def mapper_starts(lengths):
    """PositionMapper's forward-strand starts of `lengths` (unbounded integers)"""
    st = []
    for i, n in enumerate(lengths):
        st.append(int(n) if i == 0 else st[-1] + 3 * int(lengths[i - 1]) + max(int(lengths[i - 1]), int(n)))
    return st


def deltas(which, ctg, ref):
    """(dc, dr) of the shift `which` for the coordinates ctg / ref (zeros aside): straddle puts the middle one of each axis on 2^31,
    top the largest one on 2^32 - 1"""
    c, r = np.asarray(ctg, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    c, r = np.sort(c[c != 0]), np.sort(r[r != 0])
    if which == "low":
        return 0, 0
    if which == "straddle":
        return TOP_BIT - int(c[len(c) // 2]), TOP_BIT - int(r[len(r) // 2])
    if which == "upper":
        return 0xC0000000, 0xC0000000
    if which == "top":
        return NONE32 - int(c[-1]), NONE32 - int(r[-1])
    raise KeyError(which)


def reaches(which, x):
    """does the shifted coordinate array x (zeros aside) lie where the shift's name says"""
    x = np.asarray(x, dtype=np.int64)
    x = x[x != 0]
    if which == "low":
        return bool((x < TOP_BIT).all())
    if which == "straddle":
        return bool((x < TOP_BIT).any() and (x >= TOP_BIT).any() and min((x < TOP_BIT).mean(), (x >= TOP_BIT).mean()) >= 0.25)
    if which == "upper":
        return bool((x >= TOP_BIT).all())
    return bool(x.max() == NONE32)


def wrapping_sums(g, rec):
    """how many of the accepted pairs `rec` (succ_rule.successors' records on g, with their sources) have a source coordinate
    whose sum with the step passes 2^32: rec = (source vertex ids, records [n, 4])"""
    src, r = rec
    step = r[:, 1].astype(np.int64)
    ac, ar = g["ctg"][src].astype(np.int64), g["ref"][src].astype(np.int64)
    return int(((ac != 0) & (ac + step >= SPACE)).sum()), int(((ar != 0) & (ar + step >= SPACE)).sum())


# ---- the walker wave's inputs and results (tests/walk_rule.py) ---------------------------------------------------------------------
LOG_NONE = 0x7FFFFFFF  # the iteration log's 31-bit coordinate field: the clamp, and what "none examined" is recorded as


def walk_graph(G, dc, dr=0):
    """a walk_rule.Graph with its vertices' coordinates and the coordinate field of its successor records translated (a marker
    record's field is 0 and stays)"""
    import walk_rule as R
    succ = G.succ.copy()
    succ["pc"] = coord(G.succ["pc"], dc)
    return R.Graph(G.k, pos(G.upos, dc, dr), G.ucnt, G.newid, G.succ_off, succ, G.incomplete)


def walk_contig(C, dc):
    """a walk_rule.Contig translated: both strand ranges, the mapper's start table, the global coordinate window"""
    import walk_rule as R
    return R.Contig(bound(C.ctg_left, dc), bound(C.ctg_right, dc), bound(C.rev_left, dc), bound(C.rev_right, dc), C.split_size, C.leap_min,
                    [s + int(dc) for s in C.starts], C.sizes, C.in_lo, C.in_hi, C.g_lo, C.g_hi, C.gvisited, bound(C.gwin_lo, dc), bound(C.gwin_hi, dc))


def walk_job(J, dc):
    """a walk_rule.Job translated: its stop coordinate and the forced lower end of its travel window"""
    import walk_rule as R
    return R.Job(J.start, J.has_size, J.seq_cap, J.exact, J.mode, bound(J.stop_pc, dc), bound(J.win_low, dc), J.init, J.set_size)


def log_entry(x, dc):
    """an iteration log entry (flag << 63 | min(elow, 2^31 - 1) << 32 | m0) of a walk BELOW 2^31 - 1, as the translated walk
    records it: the coordinate moved, then clamped; "none" stays"""
    x = int(x)
    if not x >> 63:
        return x
    e = (x >> 32) & LOG_NONE
    if e != LOG_NONE:
        e = min(e + int(dc), LOG_NONE)
    return (1 << 63) | (e << 32) | (x & NONE32)


WALK_COORDS = ("last_ctg", "wd_below_max", "wd_forced_min")  # the coordinates among a walk's results; the rest are sizes, counts, ids
