"""The rule a walker wave (walk_job, k5_travel.hip) is held to: graphTravel / walkStraight / classifySuccessors over the
successor records of a traversal graph, in plain Python — sets, lists, integers.  Written from the record fields and the
contracts in pag_travel.hpp (SuccRec, TravContig, TravJob, TravJobOut), the grades of trav_device.hpp and the marker grades
of walk_note_record; nothing here knows about lanes, windows, stamps, filters or hash sets.

What the rule does know about the kernel is its SCHEDULE, because the splice bookkeeping of an exact job (max_back,
max_probe, wd_*, the seq_x log) is defined over "the records examined" and the schedule decides which those are:
  * a single alternative is walked alone; 2 .. PROBE_GROUPS alternatives walk in lockstep, one classification per turn,
    a vertex with more records than a slot has lanes walked to its end at once, and an alternative behind one that has
    leapt is dropped where it stands; more alternatives, or any vertex of more than LIST_CAP records on the way, are walked
    one after the other to their ends (the reference's own order);
  * after a lockstep or single probe, graphTravel's classification of the last vertex re-examines only the records the
    probe accepted there (at most PB_CAP, otherwise all of them).
The sequence itself does not depend on any of this.  Under speculation (exact = 0) only the sequence is defined.
"""
import numpy as np

MODE_SPEC, MODE_RESUME, MODE_LEAP, MODE_UNTIL_LEAP = 1, 2, 4, 8
END, BRANCH, LEAP = 0, 1, 3
NONE32 = 0xFFFFFFFF
GRADE_SKIP, GRADE_GOOD, GRADE_EXCELLENT, GRADE_AMAZING, GRADE_POISON_IF_LEAP, GRADE_POISON = 1, 2, 3, 4, 6, 7
SUCC_DTYPE = np.dtype([("tgt", "<u4"), ("pc", "<u4"), ("meta", "<u4"), ("toff", "<u4")])

GEOMETRY_NAMES = ("LIST_CAP", "BR_CAP", "PB_CAP", "PROBE_GROUPS", "WIN_IDS", "WIN_REC", "WIN_BACK", "WIN_AHEAD", "FILT_WORDS")
# the default build (make WALK_WINDOW=tiny); the GPU tests take the values from pag_debug_walk_geometry instead
DEFAULT_GEOMETRY = dict(zip(GEOMETRY_NAMES, (64, 64, 16, 8, 256, 832, 32, 64, 128)))


def filt_key(v, filt_words):
    """the two bits of vertex v in a membership filter of filt_words 64-bit words (filt_key of k5_travel.hip) -> (word, mask)"""
    v = (v * 0x85EBCA6B) & 0xFFFFFFFF
    v ^= v >> 15
    return v & (filt_words - 1), (1 << ((v >> 10) & 63)) | (1 << ((v >> 16) & 63))


def hs_slot(key, mask):
    """home slot of a key in the open-addressing sets (hs_hash of trav_device.hpp)"""
    return ((key * 2654435761) & 0xFFFFFFFF) & mask


class Graph:
    """k, upos[n] (ctg << 32 | ref by new id), ucnt[n], newid[n], succ_off[n + 1], succ (SUCC_DTYPE)"""

    def __init__(self, k, upos, ucnt, newid, succ_off, succ, incomplete=None):
        self.k = int(k)
        self.incomplete = None if incomplete is None else np.asarray(incomplete, dtype=np.uint32)  # (bit u: the records of u are a marker)
        self.upos = np.asarray(upos, dtype=np.uint64)
        self.ucnt = np.asarray(ucnt, dtype=np.uint32)
        self.newid = np.asarray(newid, dtype=np.uint32)
        self.succ_off = np.asarray(succ_off, dtype=np.uint32)
        self.succ = np.asarray(succ, dtype=SUCC_DTYPE)
        self.n_pos = len(self.upos)
        self._pc = [int(x) >> 32 for x in self.upos]
        self._recs = {}

    def pc(self, v):
        return self._pc[v]

    def records(self, u):
        """[(tgt, pc, step, grade, follows the contig)] of vertex u, in record order"""
        r = self._recs.get(u)
        if r is None:
            a, b = int(self.succ_off[u]), int(self.succ_off[u + 1])
            r = [(int(t), int(p), int(m) & 0xFFFFFF, (int(m) >> 24) & 7, bool((int(m) >> 27) & 1)) for t, p, m, _ in self.succ[a:b].tolist()]
            self._recs[u] = r
        return r


class Contig:
    def __init__(self, ctg_left, ctg_right, rev_left=0, rev_right=0, split_size=0, leap_min=1.0, starts=(0,), sizes=(), in_lo=0, in_hi=0,
                 g_lo=None, g_hi=None, gvisited=None, gwin_lo=NONE32, gwin_hi=0):
        self.ctg_left, self.ctg_right, self.rev_left, self.rev_right = ctg_left, ctg_right, rev_left, rev_right
        self.split_size, self.leap_min = int(split_size), float(leap_min)
        self.starts, self.sizes = [int(x) for x in starts], [int(x) for x in sizes]
        self.in_lo, self.in_hi = in_lo, in_hi
        self.g_lo, self.g_hi = (in_lo if g_lo is None else g_lo), (in_hi if g_hi is None else g_hi)
        self.gvisited = None if gvisited is None else set(gvisited)  # globalUniqueTable (None: before the first commit)
        self.gwin_lo, self.gwin_hi = gwin_lo, gwin_hi                # ctgGlobalPosTable


class Job:
    def __init__(self, start, has_size=0, seq_cap=4096, exact=1, mode=0, stop_pc=0, win_low=0, init=(), set_size=1024):
        self.start, self.has_size, self.seq_cap, self.exact, self.mode = start, int(has_size), int(seq_cap), exact, mode
        self.stop_pc, self.win_low, self.init, self.set_size = stop_pc, win_low, list(init), int(set_size)


class Overflow(Exception):
    pass


class Window:
    """a coordinate table (ctgPosTable): the hull of the coordinates added, 0 = no coordinate"""

    def __init__(self, lo=NONE32, hi=0):
        self.lo, self.hi = lo, hi

    def add(self, p):
        if p != 0:
            self.lo, self.hi = min(self.lo, p), max(self.hi, p)

    def has(self, p):
        return self.lo <= p <= self.hi

    def copy(self):
        return Window(self.lo, self.hi)


def landing_refused(C, pc):
    """the landing rule: singleToDual over the start table, refused when the offset lies beyond size * leap_min"""
    lo, hi = 0, C_n(C) + 1
    while lo < hi:  # upper_bound(starts, pc)
        mid = (lo + hi) >> 1
        if C.starts[mid] <= pc:
            lo = mid + 1
        else:
            hi = mid
    idx = lo - 1 if lo else 0
    off = (pc - C.starts[idx]) & 0xFFFFFFFFFFFFFFFF
    sz = C.sizes[idx] if idx < C_n(C) else 0
    if off >= 2 * sz:  # the second half of the doubled space (and everything the unsigned difference wraps to)
        off = (off - 2 * sz) & 0xFFFFFFFFFFFFFFFF
    if off >= 1 << 63:
        off -= 1 << 64
    return float(off) > float(sz) * C.leap_min


def C_n(C):
    return len(C.sizes)


class Result:
    pass


class Walk:
    def __init__(self, G, C, J, geom=None):
        self.G, self.C, self.J = G, C, J
        self.geom = dict(DEFAULT_GEOMETRY if geom is None else geom)
        self.PG = self.geom["PROBE_GROUPS"]
        self.GL = 64 // self.PG
        self.split = (1 << 64) - 1 if J.mode & MODE_SPEC else C.split_size
        if J.mode & MODE_LEAP:
            self.split = 0
        self.force_low = J.win_low if J.mode & MODE_LEAP else 0
        self.tvis = set()
        self.win_t = Window()
        self.win_g = Window(C.gwin_lo, C.gwin_hi)
        # splice bookkeeping
        self.x_elow = self.x_m0 = self.x_forced = NONE32
        self.x_below = 0
        self.poison = 0
        self.max_probe = 0
        self.seq_x = {}
        # what the cases are named for
        self.cnt = dict(l1_records=0, l2_records=0, fanout=0, pb=0, probe_out=0, walk_out=0, hull_gap=False, landing_refused=False,
                        landing_ok=False, hops=set(), modes=set(), reuse=0, reuse_refused=0, br_global=False, wide_list=False, killed=0,
                        marker6=set(), marker7=0, skip_kept=False, skip_dropped=False, rev_hit=False, gwin_hit=False, gvis_hit=set(),
                        tvis_out_hit=False, pvis_out_hit=False, leap_start=False)
        self._last_classified = None

    # ---- the rule --------------------------------------------------------------------------------------------------------
    def in_range(self, v):
        return self.C.in_lo <= v < self.C.in_hi

    def is_leap(self, pc):
        return pc != 0 and (pc < self.C.ctg_left or pc >= self.C.ctg_right)

    def note(self, v, pc, ectg, grade=0, can_leap=False):
        """walk_note_record: every examined record passes here"""
        if grade == GRADE_POISON or (grade == GRADE_POISON_IF_LEAP and can_leap):
            self.poison = 1
        if grade >= GRADE_POISON_IF_LEAP:
            if grade == GRADE_POISON:
                self.cnt["marker7"] += 1
            else:
                self.cnt["marker6"].add(bool(can_leap))
            return
        if pc == 0:
            self.x_m0 = min(self.x_m0, v)
        elif ectg:
            self.x_elow = min(self.x_elow, pc)
        else:  # window-dependent: a coordinate, and the edge does not follow the contig
            if pc < self.force_low:
                self.x_below = max(self.x_below, pc)
            else:
                self.x_forced = min(self.x_forced, pc)

    def parent_filter(self, rec, win_t):
        """graphTravel's filter: the global tables, the reverse strand, the travel tables"""
        v, pc, _, _, ectg = rec
        free = pc == 0 or ectg  # no coordinate, or the edge follows the contig: the coordinate tables do not apply
        if self.C.gvisited is not None and v in self.C.gvisited:
            self.cnt["gvis_hit"].add("in" if self.in_range(v) else ("strand" if self.C.g_lo <= v < self.C.g_hi else "off"))
            return False
        if not free and self.win_g.has(pc):
            self.cnt["gwin_hit"] = True
            return False
        if pc != 0 and self.C.rev_left <= pc < self.C.rev_right:
            self.cnt["rev_hit"] = True
            return False
        if v in self.tvis:
            if not self.in_range(v):
                self.cnt["tvis_out_hit"] = True
            return False
        if not free and win_t.has(pc):
            return False
        return True

    def classify(self, u, can_leap, filt, level):
        """classifySuccessors over the records of u -> (the chosen class in record order, [(record, class)] of every accepted one)"""
        recs = self.G.records(u)
        key = "l1_records" if level == 1 else "l2_records"
        self.cnt[key] = max(self.cnt[key], len(recs))
        if self.in_range(u) and self._last_classified is not None and self.in_range(self._last_classified):
            self.cnt["hops"].add(u - self._last_classified)
        self._last_classified = u
        accepted = []
        for rec in recs:
            v, pc, _, grade, ectg = rec
            ok = filt(rec)
            self.note(v, pc, ectg, grade, can_leap)
            leap = self.is_leap(pc)
            if ok and leap:
                if landing_refused(self.C, pc):
                    self.cnt["landing_refused"] = True
                    ok = False
                else:
                    self.cnt["landing_ok"] = True
                    ok = can_leap
            if leap:
                cls = 0
            elif grade == GRADE_AMAZING:
                cls = 0
            elif grade == GRADE_EXCELLENT:
                cls = 1
            elif grade == GRADE_GOOD:
                cls = 2
            elif grade == GRADE_SKIP and can_leap:
                cls = 3
            else:
                cls = None  # Oops never gets a record; Skip before leaping is allowed; the marker grades 6 and 7
                if grade == GRADE_SKIP and ok:
                    self.cnt["skip_dropped"] = True
            if ok and cls is not None:
                if cls == 3:
                    self.cnt["skip_kept"] = True
                accepted.append((rec, cls))
        for c in range(4):
            chosen = [r for r, cl in accepted if cl == c]
            if chosen:
                return chosen, accepted
        return [], accepted

    # ---- walkStraight, one classification at a time --------------------------------------------------------------------
    class Probe:
        def __init__(self, W, v0, s0, has, cap, win_t):
            self.W, self.has, self.cap, self.win_t = W, has, cap, win_t
            self.path, self.size, self.status, self.pb = [(v0, s0)], s0, None, None
            self.win, self.pvis, self.n_out, self.ab = Window(), set(), 0, int(W.G.ucnt[v0])
            W.max_probe = max(W.max_probe, s0)
            if cap == 0:
                raise Overflow()
            c = W.G.pc(v0)
            if W.is_leap(c):
                self.status = LEAP
                W.cnt["leap_start"] = True
                self.win.add(c)  # (visited, as TravJobOut::max_back counts it; nothing is classified against this table)
                return
            self.win.add(c)
            self.pvis.add(v0)
            self.n_out += 0 if W.in_range(v0) else 1
            self.cur = v0

        def n_records(self):
            return len(self.W.G.records(self.cur))

        def filt(self, rec):
            W = self.W
            v, pc, _, _, ectg = rec
            if not W.parent_filter(rec, self.win_t):
                return False
            if v in self.pvis:
                if not W.in_range(v):
                    W.cnt["pvis_out_hit"] = True
                return False
            return pc == 0 or ectg or not self.win.has(pc)

        def step(self):
            W = self.W
            chosen, accepted = W.classify(self.cur, self.has + self.size >= W.split, self.filt, 2)
            if len(chosen) != 1:
                self.status = END if not chosen else BRANCH
                self.pb = accepted
                W.cnt["pb"] = max(W.cnt["pb"], len(accepted))
            else:
                if len(self.path) >= self.cap or (self.n_out + 1) * 2 > W.J.set_size - 1:
                    raise Overflow()
                v, pc, s, _, _ = chosen[0]
                self.pvis.add(v)
                self.path.append((v, s))
                self.n_out += 0 if W.in_range(v) else 1
                self.win.add(pc)
                self.size += s
                if W.is_leap(pc):
                    self.status = LEAP
                else:
                    self.cur = v
            if self.status is not None:
                W.max_probe = max(W.max_probe, self.size)
                W.cnt["probe_out"] = max(W.cnt["probe_out"], self.n_out)

        def run(self):
            while self.status is None:
                self.step()
            return self

    def walk_straight(self, v0, s0, has, cap):
        return Walk.Probe(self, v0, s0, has, cap, self.win_t).run()

    # ---- the alternatives of one iteration ---------------------------------------------------------------------------
    def probe_all(self, alts, has_now, lc):
        """-> (chosen probe, fast: the probe's last classification is at hand, lowest coordinate the probes visited)"""
        m, cap = len(alts), self.J.seq_cap
        LIST = self.geom["LIST_CAP"]
        low = NONE32
        if m <= self.PG:
            ps = [Walk.Probe(self, v, s, has_now, cap, self.win_t) for v, _, s, _, _ in alts]
            wide = False
            if m == 1:
                self.cnt["modes"].add("single")
                p = ps[0]
                while p.status is None and not wide:
                    if p.n_records() > LIST:
                        wide = True
                    else:
                        p.step()
            else:
                self.cnt["modes"].add("lockstep")

                def dominate():
                    leapt = [i for i, p in enumerate(ps) if p.status == LEAP]
                    if leapt:
                        for p in ps[leapt[0] + 1:]:
                            if p.status is None:
                                p.status = "dropped"
                                self.cnt["killed"] += 1
                dominate()
                while any(p.status is None for p in ps) and not wide:
                    for p in ps:  # slots too wide for their lanes: to their end, one at a time
                        if p.status is None and p.n_records() > self.GL:
                            while p.status is None and not wide:
                                if p.n_records() > LIST:
                                    wide = True
                                else:
                                    p.step()
                    if wide:
                        break
                    for p in ps:
                        if p.status is None:
                            p.step()
                    dominate()
            if not wide:
                for p in ps:
                    low = min(low, p.win.lo)
                fin = [p for p in ps if p.status != "dropped"]
                return self.choose(fin), True, low
            self.cnt["modes"].add("wide_fallback")
        self.cnt["modes"].add("sequential")
        ps, used = [], 0
        for v, _, s, _, _ in alts:
            p = self.walk_straight(v, s, has_now, self.PG * cap - used)
            used += len(p.path)
            low = min(low, p.win.lo)
            ps.append(p)
        return self.choose(ps), False, low

    @staticmethod
    def choose(ps):
        """the first that leaps; else the branch whose first vertex is most abundant; else the longest tip; first wins ties"""
        for p in ps:
            if p.status == LEAP:
                return p
        best = None
        for p in ps:
            if p.status == BRANCH and (best is None or p.ab > best.ab):
                best = p
        if best is not None:
            return best
        for p in ps:
            if best is None or len(p.path) > len(best.path):
                best = p
        return best

    # ---- graphTravel ---------------------------------------------------------------------------------------------------
    def run(self):
        G, C, J = self.G, self.C, self.J
        R = Result()
        seq, seq_size, now_size, n_out = [], 0, G.k, 0
        max_back = max_chosen = stopped = n_main = 0
        overflow = 0
        leap_log = bool(J.mode & MODE_LEAP)
        log_idx = None
        start = int(G.newid[J.start])
        self.win_t.add(G.pc(start))
        if leap_log and J.win_low != 0 and J.win_low < self.win_t.lo:
            self.win_t.lo = J.win_low

        def flush_log():
            if log_idx is not None:
                self.seq_x[log_idx] = (1 << 63) | (min(self.x_elow, 0x7FFFFFFF) << 32) | self.x_m0
            self.x_elow = self.x_m0 = NONE32
        try:
            fast, reuse = False, None
            if not (J.mode & MODE_RESUME):
                p = Walk.Probe(self, start, G.k, J.has_size + now_size, self.PG * J.seq_cap, self.win_t).run()
                chosen = p.path
                c0 = G.pc(start)
                if p.win.lo < c0:
                    max_back = max(max_back, c0 - p.win.lo)
            else:
                chosen = list(J.init)
            while True:
                n_main += 1
                if leap_log:
                    flush_log()
                if len(seq) + len(chosen) > J.seq_cap:
                    raise Overflow()
                max_chosen = max(max_chosen, len(chosen))
                for v, s in chosen:
                    seq.append((v, s))
                    self.tvis.add(v)
                    now_size += s
                    seq_size += s
                    n_out += 0 if self.in_range(v) else 1
                    self.win_t.add(G.pc(v))
                self.cnt["walk_out"] = n_out
                if n_out * 2 > J.set_size - 1:
                    raise Overflow()
                last = seq[-1][0]
                lc = G.pc(last)
                log_idx = len(seq) - 1
                if self.is_leap(lc):
                    break
                if J.stop_pc != 0 and lc >= J.stop_pc:
                    stopped = 1
                    break
                if (J.mode & MODE_UNTIL_LEAP) and J.has_size + now_size >= self.split:
                    stopped = 1
                    break
                can_leap = J.has_size + now_size >= self.split
                win_t = self.win_t
                if fast and reuse is not None and len(reuse) <= self.geom["PB_CAP"]:
                    # the probe's own last classification minus the records in the hull gap: only those are examined again
                    self.cnt["reuse"] += 1
                    saved = (self.x_elow, self.x_m0, self.x_below, self.x_forced, self.poison)
                    alts, _ = self.classify(last, can_leap, lambda r: self.parent_filter(r, win_t), 1)
                    self.x_elow, self.x_m0, self.x_below, self.x_forced, self.poison = saved
                    for rec, _ in reuse:
                        self.note(rec[0], rec[1], rec[4])
                        if not self.parent_filter(rec, win_t):  # accepted by the probe, inside the merged travel table now
                            self.cnt["hull_gap"] = True
                else:
                    if fast and reuse is not None:
                        self.cnt["reuse_refused"] += 1
                    alts, _ = self.classify(last, can_leap, lambda r: self.parent_filter(r, win_t), 1)
                    if len(G.records(last)) > self.geom["LIST_CAP"]:
                        self.cnt["wide_list"] = True
                        if len(alts) > 1 and len(alts) > J.seq_cap - len(seq):
                            raise Overflow()
                m = len(alts)
                if m == 0:
                    break
                self.cnt["fanout"] = max(self.cnt["fanout"], m)
                if m > self.geom["BR_CAP"]:
                    self.cnt["br_global"] = True
                p, fast, low = self.probe_all(alts, J.has_size + now_size, lc)
                it_low = min(lc if lc != 0 else NONE32, low)
                if it_low < lc:
                    max_back = max(max_back, lc - it_low)
                chosen = p.path
                reuse = p.pb if (fast and p.status in (END, BRANCH)) else None
        except Overflow:
            overflow = 1
        if leap_log:
            flush_log()
        R.seq_v, R.seq_s = [v for v, _ in seq], [s for _, s in seq]
        R.seq_len, R.seq_size = len(seq), seq_size
        R.last_ctg = G.pc(seq[-1][0]) if seq else 0
        R.stopped, R.poison, R.n_main, R.max_chosen, R.overflow = stopped, self.poison, n_main, max_chosen, overflow
        R.max_back, R.max_probe, R.wd_below_max, R.wd_forced_min, R.seq_x = max_back, self.max_probe, self.x_below, self.x_forced, dict(self.seq_x)
        R.counters = self.cnt
        return R


def run_job(G, C, J, geom=None):
    return Walk(G, C, J, geom).run()
