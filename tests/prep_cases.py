"""Inputs that make the two stages in front of K1 do their work: the read->reference coverage filter (cov_mark / cov_count_low /
cov_flag, csrc/hip/util.hip) and pag_prepare (csrc/hip/k_prepare.hip).

A case = a synth.Spec plus a deterministic REWRITE of the written <block>.ctg.ref / <block>.ref.ref files (one case also takes a
contig off config.txt).  The rewrites draw nothing from synth's generator, so no existing fixture drifts.  Every record stays a
syntactically valid 3-line ALN record: only names, scores and header coordinates change (and, for the shortened records, the
columns are cut to match the shortened header).

  list_lengths  read r gets r % 19 extra copies of each of its records in both read databases, scores s - 1, s, s + 1 cycling:
                kept per-read lists of every length 1..19 (the device's insertion sort up to 16, the host's std::sort from 17),
                ties in every list, read strands with exactly 15 and 16 active alignments (K1's fast_counts switch)
  cov_only      read->reference records renamed to a read that is not in the FASTQ, and copies shortened below read_to_ref_ratio
                (0.10) of their read: both count for coverage only (Aligner::covInfHelper, Aligner.cpp:70-82)
  other_ref     read->reference records retargeted to the decoy references (header coordinates kept: intervals that run past the
                shorter decoy's end are clamped, on a reference that is not the accepted one), read->contig records retargeted to
                a contig the block does not list and to a name that is no contig at all
  reject        the probe input with all of the above (but for the unlisted contig: its two contigs are both listed) and, for three
                reads in four, the front quarter of the read->reference alignment scored ABOVE the whole one (head_first: a list whose
                first entries the filter can reject while it keeps later ones), at a -v that rejects about half of pass 2

The shapes each case promises are asserted on the CPU by tests/test_prep_cases.py.
"""
import os
from dataclasses import dataclass

import numpy as np

import synth

GAP = ord("-")
GHOST = "ghost"          # a read name no FASTQ has
NO_CONTIG = "ctg_none"   # a target name no FASTA has
SHORT_RATIO = 0.08       # query interval of a shortened record over its read's length (read_to_ref_ratio is 0.10)

PROBE = dict(seed=61, ref_len=8193, n_reads=120, read_len=700, read_len_jitter=0.5, k=8, n_refs=3,
             contigs=[(100, 3900, False), (4200, 8000, True)], dup_read_aln=True)
# (the third contig is the one other_ref's block does not list)
THREE_CTGS = dict(PROBE, seed=62, contigs=[(100, 3900, False), (4200, 6100, True), (6300, 8000, False)])


@dataclass(frozen=True)
class Case:
    spec: dict
    rewrites: tuple
    threads: int
    eps: int
    cov: int
    unlisted_ctg: str = ""  # a contig of ctg.fasta taken off config.txt


# `reject`'s cov: by the C oracle, pass 2 emits 148 789 tuples at -v 80 against 223 321 at -v 0 (67 %) — test_prep_cases.py
# recomputes both and asserts the 10 % .. 90 % window.  The other covs sit inside their case's coverage range too (cov_only: 66 of
# 102 listed records pass at 11; other_ref: 100 of 137 at 9).
CASES = {
    "list_lengths": Case(PROBE, ("list_lengths",), 16, 10, 2),
    "cov_only": Case(PROBE, ("cov_only",), 5, 10, 11),
    "other_ref": Case(THREE_CTGS, ("other_ref",), 7, 10, 9, unlisted_ctg="ctg2"),
    "reject": Case(PROBE, ("other_ref", "cov_only", "head_first", "list_lengths"), 4, 10, 80),
}


# ---- records ---------------------------------------------------------------------------------------------------------------
# a record = [header fields (list of str), query row, reference row]
# header: qName rName F|R score qBegin qEnd qSize rBegin rEnd rSize
def read_records(path):
    lines = open(path).read().splitlines()
    assert len(lines) % 3 == 0, path
    return [[lines[i].split(), lines[i + 1], lines[i + 2]] for i in range(0, len(lines), 3)]


def write_records(path, recs):
    with open(path, "w") as f:
        for h, q, r in recs:
            f.write(" ".join(h) + "\n" + q + "\n" + r + "\n")


def _cut(rec, hi):
    """the record cut to its leading `hi` columns (it starts, as before, and must end on a column with both bases present): header
    intervals and score follow — what synth does for its dup_read_aln halves"""
    h, q, r = rec
    qa, ra = np.frombuffer(q.encode(), np.uint8)[:hi], np.frombuffer(r.encode(), np.uint8)[:hi]
    assert qa[-1] != GAP and ra[-1] != GAP
    nq, nr = int((qa != GAP).sum()), int((ra != GAP).sum())
    h2 = list(h)
    if h[2] == "F":
        h2[5] = str(int(h[4]) + nq)
    else:  # (query coordinates are on the read's forward strand: the leading columns are the END of a reverse read's interval)
        h2[4] = str(int(h[5]) - nq)
    h2[8] = str(int(h[7]) + nr)
    h2[3] = str(int((qa == ra).sum()))
    return [h2, qa.tobytes().decode(), ra.tobytes().decode()]


def _both_present(rec):
    qa, ra = np.frombuffer(rec[1].encode(), np.uint8), np.frombuffer(rec[2].encode(), np.uint8)
    return np.flatnonzero((qa != GAP) & (ra != GAP)), np.cumsum(qa != GAP)


def _shortened(rec):
    """_cut, so that the query interval is SHORT_RATIO of the read"""
    both, n_q = _both_present(rec)
    ends = both[n_q[both] <= max(2, int(SHORT_RATIO * int(rec[0][6])))]
    if len(ends) < 2:
        return None
    short = _cut(rec, int(ends[-1]) + 1)
    assert (int(short[0][5]) - int(short[0][4])) / int(rec[0][6]) < 0.10
    return short


def _front_quarter(rec, score_plus):
    """_cut to the first quarter of the columns, scored `score_plus` above the WHOLE record"""
    both, _ = _both_present(rec)
    ends = both[both < len(rec[1]) // 4]
    if len(ends) < 2:
        return None
    head = _cut(rec, int(ends[-1]) + 1)
    head[0][3] = str(int(rec[0][3]) + score_plus)
    return head


def _rw_list_lengths(ctg, ref, ctx):
    def grow(recs):
        out = []
        for h, q, r in recs:
            out.append([h, q, r])
            if not h[0].isdigit():
                continue
            s = int(h[3])
            for j in range(int(h[0]) % 19):
                h2 = list(h)
                h2[3] = str(s - 1 + j % 3)
                out.append([h2, q, r])
        return out
    return grow(ctg), grow(ref)


def _rw_cov_only(ctg, ref, ctx):
    out = []
    i = -1
    for rec in ref:
        h = rec[0]
        if h[1] != ctx["accepted"]:  # (counted over the accepted reference's records, whatever an earlier rewrite put between them)
            out.append(rec)
            continue
        i += 1
        if i % 4 == 1:  # the read is unknown: reference name known, query not
            out.append([[GHOST + h[0]] + h[1:], rec[1], rec[2]])
            continue
        out.append(rec)
        if i % 4 == 2:  # ... and a second, short alignment of a known read: filtered out by the ratio
            short = _shortened(rec)
            if short is not None:
                out.append(short)
    return ctg, out


def _rw_other_ref(ctg, ref, ctx):
    decoys = ctx["decoys"]
    out = []
    for i, rec in enumerate(ref):
        out.append(rec)
        if i % 3 == 0:  # a copy on a decoy, header coordinates as they were (the decoys are shorter: many run past the end)
            h = list(rec[0])
            h[1] = decoys[(i // 3) % len(decoys)]
            out.append([h, rec[1], rec[2]])
    out_c = []
    for i, rec in enumerate(ctg):
        h = list(rec[0])
        if i % 5 == 0 and ctx["unlisted_ctg"]:
            h[1] = ctx["unlisted_ctg"]
            out_c.append([h, rec[1], rec[2]])
        elif i % 5 == 1:
            h[1] = NO_CONTIG
            out_c.append([h, rec[1], rec[2]])
        out_c.append(rec)
    return out_c, out


def _rw_head_first(ctg, ref, ctx):
    out = []
    for rec in ref:
        h = rec[0]
        if h[1] == ctx["accepted"] and h[0].isdigit() and int(h[0]) % 4 != 1 and len(rec[1]) > 400:
            # the front quarter of the alignment, scored above it: the list's first entry ends earlier on the reference than the
            # second, so the coverage filter can reject the first and keep the second (what a topk must not count)
            head = _front_quarter(rec, 5)
            if head is not None:
                out.append(head)
        out.append(rec)
    return ctg, out


REWRITES = {"list_lengths": _rw_list_lengths, "cov_only": _rw_cov_only, "other_ref": _rw_other_ref, "head_first": _rw_head_first}


def apply_rewrites(d, rewrites, unlisted_ctg="", block=0):
    """the named rewrites, in order, on the read databases of input directory d"""
    names = [l[1:].strip() for l in open(os.path.join(d, "ref.fasta")) if l.startswith(">")]
    ctx = {"accepted": names[0], "decoys": names[1:], "unlisted_ctg": unlisted_ctg}
    pc, pr = os.path.join(d, f"{block}.ctg.ref"), os.path.join(d, f"{block}.ref.ref")
    ctg, ref = read_records(pc), read_records(pr)
    for name in rewrites:
        ctg, ref = REWRITES[name](ctg, ref, ctx)
    write_records(pc, ctg)
    write_records(pr, ref)
    if unlisted_ctg:
        cfg = open(os.path.join(d, "config.txt")).read().split("\n")
        i = cfg.index(unlisted_ctg)
        del cfg[i:i + 2]
        open(os.path.join(d, "config.txt"), "w").write("\n".join(cfg))


def generate(name, dest):
    """-> (dest, Case): the case's input directory written into dest"""
    case = CASES[name]
    synth.generate(synth.Spec(**case.spec), dest)
    apply_rewrites(dest, case.rewrites, case.unlisted_ctg)
    return dest, case


# ---- what the tests read off a loaded case -----------------------------------------------------------------------------------
def host_view(inp):
    """the host restatement's arrays of a pagctl.LoadedInput (copies)"""
    import ctypes as C

    from aligngraph2_amd.workload import ALN_DTYPE, CTG_DTYPE, REF_DTYPE, PagBuildInput
    v = C.cast(inp.view, C.POINTER(PagBuildInput)).contents

    def arr(ptr, n, dt):
        if not n:
            return np.zeros(0, dt)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dt).itemsize,)).view(dt).copy()
    nr = v.reads.n_seqs
    return {"n_reads": nr, "read_len": arr(v.reads.len, nr, "<u4"), "ctgs": arr(v.ctgs, v.n_ctgs, CTG_DTYPE), "refs": arr(v.refs, v.n_refs, REF_DTYPE),
            "aln1": arr(v.read_to_ctg.aln, v.read_to_ctg.n_aln, ALN_DTYPE), "qoff1": arr(v.read_to_ctg.query_off, nr + 1, "<u8"),
            "aln2": arr(v.read_to_ref.aln, v.read_to_ref.n_aln, ALN_DTYPE), "qoff2": arr(v.read_to_ref.query_off, nr + 1, "<u8")}


def raw_records(inp):
    """the parser's records of both read databases, database order (copies): what pag_prepare starts from"""
    import ctypes as C

    from aligngraph2_amd.workload import RAW_DTYPE, PagRawInput
    v = C.cast(inp.raw_view, C.POINTER(PagRawInput)).contents

    def arr(db):
        if not db.n:
            return np.zeros(0, RAW_DTYPE)
        return np.ctypeslib.as_array(C.cast(db.rec, C.POINTER(C.c_uint8)), shape=(db.n * RAW_DTYPE.itemsize,)).view(RAW_DTYPE).copy()
    return arr(v.read_to_ctg), arr(v.read_to_ref)


def active_per_strand(aln, qoff, n_reads):
    """[n_reads, 2]: alignments of the kept lists that put positions on each read strand (what K1's for_active counts without a
    coverage verdict or a topk)"""
    from aligngraph2_amd.workload import FLAG_ELIG, FLAG_REV, PAG_NONE
    out = np.zeros((n_reads, 2), np.int64)
    listed = aln[:int(qoff[-1])]
    act = ((listed["flags"] & FLAG_ELIG) != 0) & (listed["q_start"] != PAG_NONE) & (listed["n_valid"] > 0)
    np.add.at(out, (listed["query"][act].astype(np.int64), ((listed["flags"][act] & FLAG_REV) != 0).astype(np.int64)), 1)
    return out


def numpy_cov_verdicts(aln, refs, F):
    """the coverage filter by its definition (Aligner.cpp:58-88, Aligner.tcc:140-149, quirk Q3), NOT the kernel's shortcut:
    coverage per base from every record with a known target, sorted ascending, verdict = max(sorted[t_begin:t_end]) >= F; an empty
    interval passes only at F = 0.  -> (uint8 verdict per record (0 where the target is unknown), sorted coverage per reference)"""
    from aligngraph2_amd.workload import PAG_NONE
    known = aln["target"] != PAG_NONE
    sorted_cov = []
    ok = np.zeros(len(aln), np.uint8)
    for r in range(len(refs)):
        n = int(refs["len"][r])
        diff = np.zeros(n + 1, np.int64)
        m = np.flatnonzero(known & (aln["target"] == r))
        b, e = aln["t_begin"][m].astype(np.int64), aln["t_end"][m].astype(np.int64)
        assert (b <= e).all() and (e <= n).all()
        np.add.at(diff, b, 1)
        np.add.at(diff, e, -1)
        s = np.sort(np.cumsum(diff)[:n])
        sorted_cov.append(s)
        # max(s[b:e]) for every record at once: maximum.reduceat over the index pairs (b, e) gives it at the even places where
        # b < e (a closing 0 makes e = n a valid index); an empty interval has no maximum and counts as 0
        mx = np.zeros(len(m), np.int64)
        if len(m):
            mx = np.maximum.reduceat(np.append(s, 0), np.stack([b, e], 1).ravel())[::2]
            mx[b >= e] = 0
        ok[m] = mx >= F
    return ok, sorted_cov
