"""Constructed graphs for the walker wave (tests/test_gpu_walk.py, tests/test_walk_rule.py): a builder that lays out strand
vertices by contig coordinate and coordinate-free vertices below them and writes consistent successor records (pc, toff and
the count nibble are derived, never typed in), and the cases, each named for the path of walk_job it is built to reach.
A case says what it reaches as a check over the counters of the rule (walk_rule.Walk.cnt) and the rule's result."""
import numpy as np

import walk_rule as R
from walk_rule import GRADE_AMAZING as AMAZ, GRADE_EXCELLENT as EXC, GRADE_GOOD as GOOD, GRADE_SKIP as SKIP

# the coordinate space of every case: contig 0 (100 000 bases) is the traversed one, its forward strand [CL, CR), the
# opposite strand behind it; contig 1 (50 000 bases) is where leaps land
CL, CR, REV_R = 1000, 101000, 201000
B_START, B_SIZE = 201000, 50000
# (contig 1 has the mapper's own spacing: forward half [B_START, + B_SIZE), reverse half from B_START + 2 B_SIZE, the next start
# 4 B_SIZE on, so an offset at or above twice the size is one on the reverse half, folded back before the landing rule)
STARTS, SIZES = (CL, B_START, B_START + 4 * B_SIZE), (100000, B_SIZE)
NEVER = 1 << 40  # a split size no walk reaches


class Builder:
    def __init__(self, k=8):
        self.k, self.vs, self.es, self.order = k, {}, {}, []

    def v(self, name, pc=0, ab=1, fid=None):
        """a vertex: pc != 0 on a strand (ids by ascending pc), pc == 0 coordinate-free (fid: at that id among the free ones)"""
        assert name not in self.vs, name
        self.vs[name] = dict(pc=pc, ab=ab, fid=fid)
        self.es[name] = []
        self.order.append(name)
        return name

    def e(self, a, b, step=None, grade=AMAZ, ectg=None):
        self.es[a].append((b, step, grade, ectg))

    def chain(self, prefix, n, pc0, dpc=1, ab=1, ectg=None):
        """n strand vertices prefix0 .. at pc0, pc0 + dpc, .., each the one successor of the one before"""
        names = [self.v(f"{prefix}{i}", pc0 + i * dpc, ab) for i in range(n)]
        for a, b in zip(names, names[1:]):
            self.e(a, b, ectg=ectg)
        return names

    def free_chain(self, prefix, n, fids=None):
        names = [self.v(f"{prefix}{i}", 0, fid=None if fids is None else fids[i]) for i in range(n)]
        for a, b in zip(names, names[1:]):
            self.e(a, b, grade=GOOD)
        return names

    def build(self, n_free_min=0, **ckw):
        free = [n for n in self.order if self.vs[n]["pc"] == 0]
        fixed = {self.vs[n]["fid"]: n for n in free if self.vs[n]["fid"] is not None}
        nz = max([len(free), n_free_min] + [f + 1 for f in fixed])
        slots, rest = [None] * nz, [n for n in free if self.vs[n]["fid"] is None]
        for f, n in fixed.items():
            slots[f] = n
        it = iter(rest)
        for i in range(nz):
            if slots[i] is None:
                slots[i] = next(it, None)
        assert next(it, None) is None
        strand = sorted((n for n in self.order if self.vs[n]["pc"] != 0), key=lambda n: self.vs[n]["pc"])
        names = slots + strand
        ids = {n: i for i, n in enumerate(names) if n is not None}
        n_pos = len(names)
        upos = np.zeros(n_pos, dtype=np.uint64)
        ucnt = np.ones(n_pos, dtype=np.uint32)
        for n, i in ids.items():
            upos[i] = (self.vs[n]["pc"] << 32) | (i + 1)  # (the reference coordinate is not read by a walk)
            ucnt[i] = self.vs[n]["ab"]
        counts = np.array([len(self.es[n]) if n is not None else 0 for n in names], dtype=np.int64)
        succ_off = np.zeros(n_pos + 1, dtype=np.uint32)
        succ_off[1:] = np.cumsum(counts)
        succ = np.zeros(int(succ_off[-1]), dtype=R.SUCC_DTYPE)
        at = 0
        for n in names:
            for b, step, grade, ectg in self.es.get(n, []):
                t, pa, pb = ids[b], self.vs[n]["pc"], self.vs[b]["pc"]
                if step is None:
                    step = pb - pa if pa and pb > pa else 1
                if ectg is None:
                    ectg = bool(pa and pb > pa and CL <= pb < CR)
                marker = grade >= R.GRADE_POISON_IF_LEAP
                succ[at] = (t, 0 if marker else pb, step | (grade << 24) | (int(ectg) << 27) | (min(int(counts[t]), 15) << 28), succ_off[t])
                at += 1
        old_of_new = np.arange(n_pos)[::-1].copy()  # old (k-mer-major) ids: any permutation will do for a walk
        newid = np.zeros(n_pos, dtype=np.uint32)
        newid[old_of_new] = np.arange(n_pos)
        G = R.Graph(self.k, upos, ucnt, newid, succ_off, succ)
        pcs = np.array([x >> 32 for x in upos.tolist()])
        on = np.nonzero((pcs >= CL) & (pcs < CR))[0]
        in_lo, in_hi = (int(on[0]), int(on[-1]) + 1) if len(on) else (nz, nz)
        kw = dict(ctg_left=CL, ctg_right=CR, rev_left=CR, rev_right=REV_R, split_size=NEVER, leap_min=0.8, starts=STARTS, sizes=SIZES,
                  in_lo=in_lo, in_hi=in_hi, g_lo=in_lo, g_hi=in_hi)
        gv = ckw.pop("gvisited", None)
        inc = ckw.pop("incomplete", None)
        if inc is not None:  # TravGraph::incomplete: the walker reads the marker records, the bitmap only travels with the graph
            G.incomplete = np.zeros((n_pos + 31) // 32, dtype=np.uint32)
            for n in inc:
                G.incomplete[ids[n] >> 5] |= np.uint32(1 << (ids[n] & 31))
        seg = ckw.pop("in_lo_above", 0)
        kw.update(ckw)
        kw["in_lo"] += seg
        C = R.Contig(gvisited=None if gv is None else [ids[n] for n in gv], **kw)
        self.ids, self.old = ids, {n: int(old_of_new[i]) for n, i in ids.items()}
        return G, C


class Case:
    def __init__(self, name, family, G, C, jobs, reaches, misspec=None, overflow=False):
        self.name, self.family, self.G, self.C, self.jobs, self.reaches = name, family, G, C, jobs, reaches
        self.misspec, self.overflow = misspec, overflow  # misspec: the reason this case must mis-speculate (None: it must not)

    def __repr__(self):
        return self.name


def _tips(b, hub, n, grade=AMAZ, longest=None, prefix="t"):
    """n coordinate-free alternatives of `hub`, dead ends of one vertex, the one at `longest` two vertices longer"""
    for i in range(n):
        t = b.v(f"{hub}_{prefix}{i}")
        b.e(hub, t, grade=grade)
        if i == longest:
            x = b.free_chain(f"{hub}_{prefix}{i}x", 2)
            b.e(t, x[0], grade=GOOD)


def cases(geom=None):
    g = dict(R.DEFAULT_GEOMETRY if geom is None else geom)
    WIN_IDS, WIN_REC, PG, PB, BR, LIST = g["WIN_IDS"], g["WIN_REC"], g["PROBE_GROUPS"], g["PB_CAP"], g["BR_CAP"], g["LIST_CAP"]
    out = []

    def job(b, start, **kw):
        return R.Job(b.old[start], **kw)

    # ================================================================ window
    for n in (WIN_IDS - 1, WIN_IDS, WIN_IDS + 1, 2 * WIN_IDS + 1):
        b = Builder()
        c = b.chain("s", n, CL + 10)
        G, C = b.build()
        out.append(Case(f"window_chain_{n}", "window", G, C, [job(b, c[0]), job(b, c[n // 2])],
                        lambda cn, rs, n=n: rs[0].seq_len == n and cn[0]["hops"] == {0, 1} and rs[1].seq_len == n - n // 2))
    for back in (63, 64, 65):
        # up the strand in strides, every stride entered at its top by a forward hop and left by a backward hop of `back` ids
        b = Builder()
        n = 4 * 70
        c = [b.v(f"s{i}", CL + 10 + i) for i in range(n)]
        order, at = [0], 0
        for _ in range(3):
            top = at + back + 1
            order += [top + 1, top + 1 - back] + list(range(top + 2 - back, top + 1))
            at = top + 1
        for a, d in zip(order, order[1:]):
            b.e(c[a], c[d], ectg=True)
        assert len(set(order)) == len(order)
        G, C = b.build()
        out.append(Case(f"window_back_hop_{back}", "window", G, C, [job(b, c[0])],
                        lambda cn, rs, back=back, L=len(order): rs[0].seq_len == L and -back in cn[0]["hops"]))
    far = 3 * WIN_IDS + 7
    b = Builder()
    c = [b.v(f"s{i}", CL + 10 + i) for i in range(far + 40)]
    order = list(range(0, 10)) + [far, 10] + list(range(11, 30)) + [far + 1] + list(range(far + 2, far + 40))
    for a, d in zip(order, order[1:]):
        b.e(c[a], c[d], ectg=True)
    G, C = b.build()
    out.append(Case("window_far_hop_and_back", "window", G, C, [job(b, c[0])],
                    lambda cn, rs, far=far, L=len(order): rs[0].seq_len == L and {far - 9, 10 - far} <= cn[0]["hops"]))
    # 14 records a vertex: the window's records run out before its ids (13 of them Skip grades, not admitted before leaping)
    b = Builder()
    n = WIN_IDS + 40
    assert 14 * WIN_IDS > WIN_REC
    c = [b.v(f"s{i}", CL + 10 + i) for i in range(n)]
    junk = b.v("junk")
    for i in range(n - 1):
        for q in range(13):
            if q == 6:
                b.e(c[i], c[i + 1])
            b.e(c[i], junk, grade=SKIP)
    G, C = b.build()
    out.append(Case("window_records_cut_short", "window", G, C, [job(b, c[0]), job(b, c[WIN_IDS // 2])],
                    lambda cn, rs, n=n: rs[0].seq_len == n and cn[0]["l2_records"] == 14 and cn[0]["skip_dropped"]))
    for lead in (1, 2, 3):
        for which in (0, 1):
            # a branch decided by abundance, the two deciding vertices at the first and at the last id of the window the walk
            # fills at its start; `lead` coordinate-free vertices in front shift the strand against the 16-byte rows of ucnt
            b = Builder()
            for i in range(lead):
                b.v(f"f{i}")
            n = 2 * WIN_IDS
            d = WIN_IDS // 2 + 5
            d0 = (d - g["WIN_BACK"]) & ~31
            first, last = d0, d0 + WIN_IDS - 1
            c = [b.v(f"s{i}", CL + 10 + i, ab=(9 if i in (first + 1, last - 1, first - 1, last + 1) else 1)) for i in range(n)]
            b.vs[c[first]]["ab"] = 5 if which == 0 else 4
            b.vs[c[last]]["ab"] = 4 if which == 0 else 5
            b.e(c[d], c[last], ectg=True)
            b.e(c[d], c[first], ectg=True)
            for x, base in ((first, d + 10), (last, d + 20)):  # both alternatives stop at a branch of their own
                b.e(c[x], c[base], ectg=True)
                b.e(c[x], c[base + 1], ectg=True)
            G, C = b.build()
            want = c[first] if which == 0 else c[last]
            out.append(Case(f"window_abundance_edge_lead{lead}_{'first' if which == 0 else 'last'}", "window", G, C, [job(b, c[d])],
                            lambda cn, rs, w=b.ids[want]: rs[0].seq_v[1] == w and "lockstep" in cn[0]["modes"]))

    # ================================================================ list widths
    def hub_case(R_n, n_top, via_probe):
        """a vertex of R_n records, n_top of them in the best class (dead ends, the third the longest), the rest a class below"""
        b = Builder()
        s = b.chain("s", 3, CL + 10)
        hub = b.v("hub", CL + 20)
        if via_probe:  # the hub is met by a probe: one of two alternatives leads to it
            a1, a2 = b.v("a1", CL + 14), b.v("a2", CL + 15)
            b.e(s[2], a1)
            b.e(s[2], a2)
            b.e(a1, hub)
        else:
            b.e(s[2], hub)
        for i in range(R_n):
            t = b.v(f"t{i}")
            b.e("hub", t, grade=AMAZ if i % (R_n // n_top) == 0 and i // (R_n // n_top) < n_top else GOOD)
            if i == 2 * (R_n // n_top):
                x = b.free_chain(f"x{i}", 2)
                b.e(t, x[0], grade=GOOD)
        G, C = b.build()
        # (top level: the job takes the path up to the hub over, so that graphTravel itself classifies the hub first)
        init = None if via_probe else [(b.ids[x], 8 if i == 0 else 1) for i, x in enumerate(s)] + [(b.ids["hub"], 8)]
        return b, G, C, s, init

    for R_n in (LIST - 1, LIST, LIST + 1, 2 * LIST + 2):
        for n_top in (1, 5, LIST, BR + 1):
            if n_top > R_n:
                continue
            for via in (False, True):
                b, G, C, s, init = hub_case(R_n, n_top, via)
                if via:
                    out.append(Case(f"list_probe_{R_n}_records_{n_top}_chosen", "lists", G, C, [job(b, s[0])],
                                    lambda cn, rs, R_n=R_n, n_top=n_top: cn[0]["l2_records"] == R_n and cn[0]["fanout"] == max(n_top, 2)
                                    and ("wide_fallback" in cn[0]["modes"]) == (R_n > LIST)))
                else:
                    out.append(Case(f"list_top_{R_n}_records_{n_top}_chosen", "lists", G, C, [job(b, s[0], mode=R.MODE_RESUME, init=init)],
                                    lambda cn, rs, R_n=R_n, n_top=n_top: cn[0]["l1_records"] == R_n and cn[0]["fanout"] == n_top
                                    and cn[0]["br_global"] == (n_top > BR) and cn[0]["wide_list"] == (R_n > LIST)))
    for fan in (1, 2, PG, PG + 1, BR + 1):
        b = Builder()
        s = b.chain("s", 3, CL + 10)
        hub = b.v("hub", CL + 20)
        b.e(s[2], hub)
        _tips(b, "hub", fan, longest=min(fan - 1, 3))
        G, C = b.build()
        mode = "single" if fan == 1 else "lockstep" if fan <= PG else "sequential"
        init = [(b.ids[x], 8 if i == 0 else 1) for i, x in enumerate(s)] + [(b.ids["hub"], 8)]
        out.append(Case(f"fanout_{fan}", "lists", G, C, [job(b, s[0], mode=R.MODE_RESUME, init=init)],
                        lambda cn, rs, fan=fan, mode=mode: cn[0]["fanout"] == fan and mode in cn[0]["modes"]))
    for acc in (PB - 1, PB, PB + 1):
        # a probe (one of two alternatives) stops at a vertex with `acc` accepted records: kept for the top level up to PB_CAP
        b = Builder()
        s = b.chain("s", 3, CL + 10)
        a1, a2, p = b.v("a1", CL + 14), b.v("a2", CL + 15), b.v("p", CL + 16)
        b.e(s[2], a1)
        b.e(s[2], a2)
        b.e(a1, p)
        _tips(b, "p", acc, longest=1)
        b.e("p", s[1], grade=AMAZ, ectg=True)  # (visited: refused.  Examined again at the top level only when the probe's list was not
        G, C = b.build()                       # kept: the log of a LEAP job shows which, through the lowest contig-following coordinate)
        out.append(Case(f"probe_stop_{acc}_accepted", "lists", G, C, [job(b, s[0]), job(b, s[0], mode=R.MODE_LEAP)],
                        lambda cn, rs, acc=acc: cn[0]["pb"] == acc and (cn[0]["reuse"] >= 1) == (acc <= PB) and (cn[0]["reuse_refused"] >= 1) == (acc > PB)))
    b = Builder()
    s = b.chain("s", 2, CL + 10)
    x, y = b.v("x", CL + 1000), b.v("y", CL + 1001)
    b.e(s[1], x, ectg=True)
    b.e(s[1], y, ectg=True)
    x2, p = b.v("x2", CL + 1002), b.v("p", CL + 1003)
    b.e(x, x2)
    b.e(x2, p)
    q1, q2 = b.v("q1", CL + 500), b.v("q2", CL + 1500)
    b.e(p, q1, ectg=False)  # between the travel table and the probe's: accepted by the probe, refused by graphTravel
    qa = b.chain("qa", 3, CL + 501)
    b.e(q1, qa[0])          # (the longest dead end of all, had q1 been kept)
    b.e(p, q2, ectg=True)
    b.e(p, y, ectg=True)    # inside the probe's own table, but the edge follows the contig: kept
    b.e(y, b.v("y2", CL + 1600), ectg=True)
    G, C = b.build()
    out.append(Case("hull_gap_rejected_and_contig_edge_kept", "lists", G, C, [job(b, s[0])],
                    lambda cn, rs, ids=dict(b.ids): cn[0]["hull_gap"] and cn[0]["reuse"] >= 1
                    and rs[0].seq_v == [ids[n] for n in ("s0", "s1", "x", "x2", "p", "y", "y2")]))

    # ================================================================ off the strand
    for n_free in (1, 2, 3, 40):
        b = Builder()
        s = b.chain("s", 3, CL + 10)
        f = b.free_chain("f", n_free)
        g2 = b.free_chain("g", 1)
        b.e(s[2], f[0], grade=GOOD)
        b.e(s[2], g2[0], grade=GOOD)
        back = b.v("back", CL + 30)
        b.e(f[-1], back, grade=EXC)
        b.e(f[-1], f[0], grade=EXC)  # (marked by this very probe: its first outside vertex ..
        b.e(f[-1], f[-1], grade=EXC)  # .. and its latest)
        b.e(back, b.v("b1", CL + 31))
        b.e(back, b.v("b2", CL + 32))
        b.e("b1", f[0], grade=GOOD)     # (appended in an earlier iteration)
        b.e("b1", b.v("b3", CL + 40))
        b.e("b2", b.v("b4", CL + 41))
        b.e("b2", b.v("b5", CL + 42))
        G, C = b.build()
        out.append(Case(f"off_strand_probe_{n_free}", "off_strand", G, C, [job(b, s[0])],
                        lambda cn, rs, n_free=n_free: cn[0]["probe_out"] == n_free and cn[0]["pvis_out_hit"] and cn[0]["tvis_out_hit"]
                        and rs[0].seq_len == 3 + n_free + 3))
    for which in ("travel", "global"):
        # a coordinate-free vertex that is in no set while two members of the set have set both of its filter bits
        fw = g["FILT_WORDS"]
        pool, trip = 4000, None
        by_word = {}
        for v in range(pool):
            by_word.setdefault(R.filt_key(v, fw)[0], []).append(v)
        for w, vs in sorted(by_word.items()):
            for f in vs:
                mf = R.filt_key(f, fw)[1]
                for a in vs:
                    for c2 in vs:
                        if len({a, c2, f}) == 3 and ((R.filt_key(a, fw)[1] | R.filt_key(c2, fw)[1]) & mf) == mf \
                                and (R.filt_key(a, fw)[1] & mf) != mf and (R.filt_key(c2, fw)[1] & mf) != mf:
                            trip = (f, a, c2)
                            break
                    if trip:
                        break
                if trip:
                    break
            if trip:
                break
        assert trip, "no filter false positive among the first ids"
        f, a, c2 = trip
        b = Builder()
        s = b.chain("s", 3, CL + 10)
        va, vc, vf = b.v("ma", fid=a), b.v("mc", fid=c2), b.v("fp", fid=f)
        t = b.v("t", CL + 30)
        if which == "travel":  # the walk appends both members, a later iteration examines a record to the false positive
            b.e(s[2], va, grade=GOOD)
            b.e(va, vc, grade=GOOD)
            b.e(vc, t, grade=EXC)
            gv = None
        else:
            b.e(s[2], t)
            gv = ["ma", "mc"]
        u1, u2 = b.v("u1", CL + 31), b.v("u2", CL + 32)
        b.e(t, u1)
        b.e(t, u2)
        b.e(u1, vf, grade=GOOD)
        b.e(u1, va, grade=GOOD)  # (a member: refused)
        b.e(vf, b.v("end", CL + 50), grade=EXC)
        G, C = b.build(n_free_min=max(trip) + 1, gvisited=gv)
        out.append(Case(f"filter_false_positive_{which}", "off_strand", G, C, [job(b, s[0])],
                        lambda cn, rs, ids=dict(b.ids), which=which: rs[0].seq_v[-2:] == [ids["fp"], ids["end"]]
                        and (cn[0]["tvis_out_hit"] if which == "travel" else "off" in cn[0]["gvis_hit"])))
    b = Builder()
    n = 2 * WIN_IDS
    c = b.chain("s", 20, CL + 10)
    rest = [b.v(f"r{i}", CL + 100 + i) for i in range(n)]
    b.e(c[19], rest[5], ectg=True)           # globally visited, inside the window
    b.e(c[19], rest[n - 1], ectg=True)       # globally visited, on the strand but far outside the window
    b.e(c[19], rest[7], ectg=True)
    b.e(rest[7], rest[8])
    G, C = b.build(gvisited=["r5", f"r{n - 1}"])
    out.append(Case("gbits_inside_and_outside_the_window", "off_strand", G, C, [job(b, c[0])],
                    lambda cn, rs, ids=dict(b.ids), lo=C.in_lo, n=n: rs[0].seq_len == 22 and cn[0]["gvis_hit"] == {"in"}
                    # the window is filled once, at the start vertex, for ids [in_lo, in_lo + WIN_IDS): no vertex the walk classifies
                    # comes within WIN_AHEAD of its end, r5 lies inside it and the last r a whole window beyond
                    and max(rs[0].seq_v) - lo + g["WIN_AHEAD"] <= WIN_IDS and ids["r5"] - lo < WIN_IDS and ids[f"r{n - 1}"] - lo >= 2 * WIN_IDS))
    for above in (32, 64):
        # a segment job: the direct-mapped marks start `above` ids into the strand; what lies below is kept like a vertex off it
        b = Builder()
        low = [b.v(f"l{i}", CL + 10 + i) for i in range(above + 8)]
        c = b.chain("s", 10, CL + 500)
        b.e(c[9], low[3], ectg=True)   # globally visited: the strand's bitmap below the job's range
        b.e(c[9], low[4], ectg=True)
        b.e(low[4], low[5])
        b.e(low[5], low[4], ectg=True)  # (marked by the walk itself, outside the job's range)
        b.e(low[5], c[2], ectg=True)
        G, C = b.build(gvisited=["l3"], in_lo_above=above)
        out.append(Case(f"segment_in_lo_{above}_above_g_lo", "off_strand", G, C, [job(b, c[0])],
                        lambda cn, rs: rs[0].seq_len == 12 and cn[0]["gvis_hit"] == {"strand"} and cn[0]["walk_out"] == 2))
    b = Builder()
    c = b.chain("s", 5, CL + 10)
    b.e(c[4], b.v("in_gwin", CL + 300), ectg=False)
    b.e(c[4], b.v("edge_gwin", CL + 310), ectg=True)  # inside the global table too, but the edge follows the contig
    G, C = b.build(gwin_lo=CL + 300, gwin_hi=CL + 310)
    out.append(Case("gwin_rejection", "off_strand", G, C, [job(b, c[0])],
                    lambda cn, rs, ids=dict(b.ids): cn[0]["gwin_hit"] and rs[0].seq_v[-1] == ids["edge_gwin"]))

    # ================================================================ leaping
    def leap_graph(land_pc):
        b = Builder()
        c = b.chain("s", 6, CL + 10, dpc=10)  # steps of 10: now_size = k + k + 10 * (vertices - 1)
        land = b.v("land", land_pc)
        b.e(c[3], land, grade=SKIP, ectg=False)
        return b, c
    for delta in (-1, 0, 1):
        b, c = leap_graph(B_START + 100)
        G, C = b.build(split_size=100 + 8 + 8 + 30 - delta)  # reached exactly at s3 when delta == 0
        out.append(Case(f"leap_threshold_{'below' if delta < 0 else 'at' if delta == 0 else 'above'}", "leaping", G, C, [job(b, c[0], has_size=100)],
                        lambda cn, rs, delta=delta, ids=dict(b.ids): (rs[0].seq_v[-1] == ids["land"]) == (delta >= 0) and cn[0]["landing_ok"]))
    edge = int(B_SIZE * 0.8)
    # the forward half at the rule's equality; the end of the doubled space proper (refused as it stands); the reverse half from
    # offset 2 * size on, folded back to 0 .. and met by the same equality
    for off, ok in ((edge - 1, True), (edge, True), (edge + 1, False), (B_SIZE + 5, False), (2 * B_SIZE - 1, False), (2 * B_SIZE, True),
                    (2 * B_SIZE + edge, True), (2 * B_SIZE + edge + 1, False)):
        b, c = leap_graph(B_START + off)
        G, C = b.build(split_size=0)
        out.append(Case(f"landing_offset_{off}", "leaping", G, C, [job(b, c[0])],
                        lambda cn, rs, ok=ok, ids=dict(b.ids): (rs[0].seq_v[-1] == ids["land"]) == ok and cn[0]["landing_refused"] == (not ok)))
    for pc, name, lands in ((CR + 50, "reverse_strand", False), (CL - 5, "below_ctg_left", True), (CR, "at_ctg_right", False)):
        b, c = leap_graph(pc)
        G, C = b.build(split_size=0, rev_left=CR + 10)
        out.append(Case(f"leap_{name}", "leaping", G, C, [job(b, c[0])],
                        lambda cn, rs, lands=lands, ids=dict(b.ids), name=name: (rs[0].seq_v[-1] == ids["land"]) == lands
                        and (cn[0]["rev_hit"] if name == "reverse_strand" else True)))
    b = Builder()
    land = b.v("land", B_START + 7)
    b.e(land, b.v("after", B_START + 8))
    G, C = b.build(split_size=0)
    out.append(Case("start_vertex_is_a_leap", "leaping", G, C, [job(b, land)], lambda cn, rs: rs[0].seq_len == 1 and cn[0]["leap_start"]))
    b = Builder()
    c = b.chain("s", 3, CL + 10)
    b.e(c[2], b.v("l1", B_START + 7), ectg=False)
    b.e(c[2], b.v("l2", B_START + 9), ectg=False)
    b.e(c[2], b.v("n1", CL + 50))
    G, C = b.build(split_size=0)
    out.append(Case("alternatives_start_with_leaps", "leaping", G, C, [job(b, c[0])],
                    lambda cn, rs, ids=dict(b.ids): rs[0].seq_v[-1] == ids["l1"] and cn[0]["leap_start"] and cn[0]["fanout"] == 3 and cn[0]["killed"] == 1))
    for fan in (PG, PG + 1):
        # the alternatives of one vertex, one of them on another contig BELOW the strand: whether they walk in lockstep or one
        # after the other, the coordinate that alternative starts on is one the iteration's probes visited (max_back)
        b = Builder()
        c = b.chain("s", 3, CL + 10)
        hub = b.v("hub", CL + 20)
        b.e(c[2], hub)
        _tips(b, "hub", fan - 1)
        b.e(hub, b.v("low", CL - 5), ectg=False)
        G, C = b.build(split_size=0)
        out.append(Case(f"leap_start_counts_in_max_back_{'lockstep' if fan <= PG else 'sequential'}", "leaping", G, C, [job(b, c[0])],
                        lambda cn, rs, fan=fan, ids=dict(b.ids): rs[0].seq_v[-1] == ids["low"] and rs[0].max_back == 25
                        and ("lockstep" if fan <= PG else "sequential") in cn[0]["modes"] and cn[0]["leap_start"]))
    for split, kept in ((NEVER, False), (0, True)):
        b = Builder()
        c = b.chain("s", 3, CL + 10)
        b.e(c[2], b.v("sk", 0), grade=SKIP)
        G, C = b.build(split_size=split)
        out.append(Case(f"skip_grade_{'after' if kept else 'before'}_threshold", "leaping", G, C, [job(b, c[0])],
                        lambda cn, rs, kept=kept: rs[0].seq_len == (4 if kept else 3) and cn[0]["skip_kept"] == kept and cn[0]["skip_dropped"] == (not kept)))

    # ================================================================ modes
    def mode_graph():
        b = Builder()
        c = b.chain("s", 40, CL + 10, dpc=10)
        # a side branch every ten vertices (an iteration boundary each), a window-dependent record and a coordinate-free one
        for i in (9, 19, 29):
            t = b.v(f"side{i}", CL + 15 + 10 * i)
            b.e(c[i], t, ectg=True)
            b.e(c[i + 1], b.v(f"wd{i}", CL + 5 + 10 * (i - 5)), ectg=False)
            b.e(c[i + 2], b.v(f"fr{i}"), grade=SKIP)
        b.e(c[39], b.v("land", B_START + 10), grade=SKIP, ectg=False)
        return b, c
    b, c = mode_graph()
    G, C = b.build(split_size=300)
    seed = c[12]
    out.append(Case("mode_spec_never_leaps", "modes", G, C, [job(b, c[0], mode=R.MODE_SPEC), job(b, c[0])],
                    lambda cn, rs, ids=dict(b.ids): rs[0].seq_v[-1] != ids["land"] and rs[1].seq_v[-1] == ids["land"]))
    out.append(Case("mode_leap_win_low_below_and_above_the_seed", "modes", G, C,
                    [job(b, seed, mode=R.MODE_LEAP, win_low=CL + 60), job(b, seed, mode=R.MODE_LEAP, win_low=CL + 200), job(b, seed, mode=R.MODE_LEAP)],
                    lambda cn, rs: len(rs[0].seq_x) >= 3 and rs[1].wd_below_max != 0 and rs[0].wd_forced_min != R.NONE32 and rs[0].wd_below_max == 0
                    and any((x & 0xFFFFFFFF) != R.NONE32 for x in rs[0].seq_x.values()) and cn[0]["skip_kept"]))
    full = R.run_job(G, C, R.Job(b.old[c[0]], mode=R.MODE_SPEC))
    for n0 in (1, 63, 64, 65, 257):
        if n0 <= 40:
            init = list(zip(full.seq_v[:n0], full.seq_s[:n0]))
            out.append(Case(f"mode_resume_{n0}", "modes", G, C, [job(b, c[0], mode=R.MODE_RESUME, init=init)],
                            lambda cn, rs, ids=dict(b.ids): rs[0].seq_v[-1] == ids["land"] and rs[0].seq_len == 41))
        else:
            b2 = Builder()
            c2 = b2.chain("s", n0 + 20, CL + 10)
            b2.e(c2[-1], b2.v("a", CL + 5000), ectg=True)
            b2.e(c2[-1], b2.v("b", CL + 5001), ectg=True)
            G2, C2 = b2.build()
            init = [(b2.ids[x], 8 if i == 0 else 1) for i, x in enumerate(c2[:n0])]
            out.append(Case(f"mode_resume_{n0}", "modes", G2, C2, [job(b2, c2[0], mode=R.MODE_RESUME, init=init)],
                            lambda cn, rs, n0=n0: rs[0].seq_len == n0 + 21 and rs[0].max_chosen == n0))
    out.append(Case("mode_stop_pc_exact_and_overshot", "modes", G, C,
                    [job(b, c[0], stop_pc=CL + 10 + 10 * 9, mode=R.MODE_SPEC), job(b, c[0], stop_pc=CL + 10 + 10 * 9 + 3, mode=R.MODE_SPEC),
                     job(b, c[0], stop_pc=CL + 10 + 10 * 9 + 7, mode=R.MODE_SPEC)],
                    lambda cn, rs: [r.stopped for r in rs] == [1, 1, 1] and rs[0].last_ctg == CL + 100 and rs[1].last_ctg > CL + 103 and rs[2].seq_len > rs[1].seq_len - 1))
    init = list(zip(full.seq_v[:5], full.seq_s[:5]))
    out.append(Case("mode_resume_until_leap", "modes", G, C, [job(b, c[0], mode=R.MODE_RESUME | R.MODE_UNTIL_LEAP, init=init)],
                    lambda cn, rs, ids=dict(b.ids): rs[0].stopped == 1 and rs[0].seq_v[-1] != ids["land"] and rs[0].seq_len < 41))

    # ================================================================ overflow
    b = Builder()
    c = b.chain("s", 30, CL + 10)
    b.e(c[29], b.v("a", CL + 100), ectg=True)
    b.e(c[29], b.v("bb", CL + 200), ectg=True)
    a_chain = b.chain("ax", 20, CL + 101)
    b.e("a", a_chain[0])
    G, C = b.build()
    out.append(Case("overflow_seq_cap_one_too_small", "overflow", G, C, [job(b, c[0], seq_cap=30 + 21 - 1)], lambda cn, rs: rs[0].overflow == 1, overflow=True))
    out.append(Case("no_overflow_seq_cap_exact", "overflow", G, C, [job(b, c[0], seq_cap=30 + 21)], lambda cn, rs: rs[0].overflow == 0 and rs[0].seq_len == 51))
    b = Builder()
    c = b.chain("s", 3, CL + 10)
    b.e(c[2], b.v("a", CL + 100), ectg=True)
    b.e(c[2], b.v("bb", CL + 200), ectg=True)
    a_chain = b.chain("ax", 20, CL + 101)
    b.e("a", a_chain[0])
    G, C = b.build()
    out.append(Case("overflow_arena_share_one_too_small", "overflow", G, C, [job(b, c[0], seq_cap=20)], lambda cn, rs: rs[0].overflow == 1, overflow=True))
    b = Builder()
    s = b.chain("s", 3, CL + 10)
    hub = b.v("hub", CL + 20)
    b.e(s[2], hub)
    _tips(b, "hub", LIST + 6)
    G, C = b.build()
    out.append(Case("overflow_room_behind_the_sequence_one_too_small", "overflow", G, C, [job(b, s[0], seq_cap=4 + LIST + 6 - 1)],
                    lambda cn, rs: rs[0].overflow == 1 and cn[0]["wide_list"], overflow=True))
    out.append(Case("no_overflow_room_behind_the_sequence_exact", "overflow", G, C, [job(b, s[0], seq_cap=4 + LIST + 6)],
                    lambda cn, rs: rs[0].overflow == 0 and cn[0]["wide_list"] and rs[0].seq_len == 5))
    for n_free, over in ((3, False), (4, True)):  # a set of 8: (po.n + 1) * 2 > 7 refuses a probe its fourth outside vertex
        b = Builder()
        s = b.chain("s", 3, CL + 10)
        f = b.free_chain("f", n_free)
        b.e(s[2], f[0], grade=GOOD)
        b.e(s[2], b.v("g0"), grade=GOOD)
        G, C = b.build()
        out.append(Case(f"outside_sets_load_factor_{n_free}", "overflow", G, C, [job(b, s[0], set_size=8)],
                        lambda cn, rs, over=over: rs[0].overflow == int(over), overflow=over))
    # the travel set's own guard: three outside vertices appended by one iteration, the fourth by the next (4 * 2 > 7)
    b = Builder()
    s = b.chain("s", 3, CL + 10)
    f = b.free_chain("f", 3)
    b.e(s[2], f[0], grade=GOOD)
    b.e(s[2], b.v("g0"), grade=GOOD)
    b.e(f[2], b.v("h0"), grade=GOOD)
    b.e(f[2], b.v("h1"), grade=GOOD)
    G, C = b.build()
    out.append(Case("outside_sets_travel_load_factor", "overflow", G, C, [job(b, s[0], set_size=8)],
                    lambda cn, rs: rs[0].overflow == 1 and cn[0]["walk_out"] == 4 and cn[0]["probe_out"] == 3, overflow=True))
    out.append(Case("outside_sets_travel_load_factor_fits", "overflow", G, C, [job(b, s[0], set_size=16)],
                    lambda cn, rs: rs[0].overflow == 0 and cn[0]["walk_out"] == 4))

    # ================================================================ markers
    b = Builder()
    c = b.chain("s", 4, CL + 10)
    b.e(c[3], c[3], step=1, grade=R.GRADE_POISON, ectg=False)
    G, C = b.build(incomplete=[c[3]])
    out.append(Case("marker_grade_7_examined", "markers", G, C, [job(b, c[0])], lambda cn, rs: rs[0].poison == 1 and cn[0]["marker7"] >= 1 and rs[0].seq_len == 4))
    for split, after in ((NEVER, False), (0, True)):
        b = Builder()
        c = b.chain("s", 4, CL + 10)
        b.e(c[1], c[1], step=1, grade=R.GRADE_POISON_IF_LEAP, ectg=False)
        G, C = b.build(split_size=split, incomplete=[c[1]])
        out.append(Case(f"marker_grade_6_{'after' if after else 'before'}_threshold", "markers", G, C, [job(b, c[0])],
                        lambda cn, rs, after=after: rs[0].poison == int(after) and cn[0]["marker6"] == {after} and rs[0].seq_len == 4))

    # ================================================================ speculation
    # Two alternatives: the first, more abundant, stops at a branch of its own at once; the second walks on — a step of 60 000
    # bases takes it past the split size — and ends in a leap.  The exact walk waits for it and takes the leap (the first to
    # leap wins over every branch).  The speculating walk goes on with the first while the second is still walking
    # (slots_dominate: lower abundance, far below the split size) and reports the leap when the zombie makes it.
    b = Builder()
    c = b.chain("s", 3, CL + 10)
    a, z = b.v("a", CL + 100, ab=9), b.v("z", CL + 200, ab=2)
    b.e(c[2], a, ectg=True)
    b.e(c[2], z, ectg=True)
    b.e(a, b.v("a1", CL + 101))
    b.e(a, b.v("a2", CL + 102))
    zc = b.chain("zc", 6, CL + 201)
    b.e(z, zc[0])
    b.e(zc[5], b.v("zfar", CL + 60300), step=60000, ectg=True)
    b.e("zfar", b.v("land", B_START + 10), ectg=False)
    b.e("a1", b.v("a1x", CL + 110))
    G, C = b.build(split_size=60100)
    out.append(Case("zombie_that_later_leaps", "speculation", G, C, [job(b, c[0])],
                    lambda cn, rs, ids=dict(b.ids): rs[0].seq_v[-1] == ids["land"] and cn[0]["fanout"] == 2,
                    misspec="a still-walking alternative that later leaps (slots_step: a zombie's WS_LEAP sets spec_fail bit 0)"))
    return out
