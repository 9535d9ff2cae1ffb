"""What the two pa_cns ingest test files share (tests/test_pa_cns_ingest.py on the CPU, tests/test_gpu_pa_cns_ingest.py on the
device): how bin/pa_cns is run with an ingest mode and a row dump, and the seeded 3-line ALN file aimed at the row code
(csrc/hip/cns_rows.hpp: slice_bounds, normalize_gaps)."""
import os
import subprocess

import numpy as np

import cns_cases
import pagctl

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pa_cns")
REF = os.path.join(pagctl.REF_DIR, "pa_cns")
GOLD = os.path.join(pagctl.ROOT, "tests", "golden", "pa_cns")
ACGT = "ACGT"
ENV_NAMES = ("PA_CNS_BACKEND", "PA_CNS_INGEST", "PA_CNS_DUMP_ROWS", "PA_CNS_STAGE_TIMES", "PA_CNS_ROWS_STAGE_COLS", "PA_CNS_ROWS_PIECE_BYTES")


def ensure_built():
    if not (os.path.exists(pagctl.HIP_LIB) and os.path.exists(EXE)):
        subprocess.run(["make", "-C", pagctl.ROOT, "product"], check=True, capture_output=True)


def run(exe, d, tag, case, threads=4, **env_vars):
    """-> (CompletedProcess, FASTA bytes or None, dump bytes or None); env_vars: ingest=, backend=, stage_cols=, piece_bytes="""
    env = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    out, dump = os.path.join(d, tag + ".fasta"), os.path.join(d, tag + ".rows")
    names = dict(ingest="PA_CNS_INGEST", backend="PA_CNS_BACKEND", stage_cols="PA_CNS_ROWS_STAGE_COLS", piece_bytes="PA_CNS_ROWS_PIECE_BYTES")
    for k, v in env_vars.items():
        env[names[k]] = str(v)
    if exe == EXE:
        env.update(PA_CNS_DUMP_ROWS=dump, PA_CNS_STAGE_TIMES="1")
    r = subprocess.run(cns_cases.argv(exe, d, out, case, threads), capture_output=True, text=True, timeout=900, env=env)
    read = lambda p: open(p, "rb").read() if os.path.exists(p) else None
    return r, read(out), read(dump)


# ---- the seeded file -------------------------------------------------------------------------------------------------------
def write_rows(d, bb, records):
    """a backbone and 3-line ALN records (tBegin, query row, target row, score).  A target row's symbols other than '-' are the
    bases from bb[tBegin] on, as AlignData::sliceHelper counts them ('.' is a base there), so tEnd = tBegin + their number."""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "backbone.fasta"), "w") as f:
        f.write(">P_1 seeded\n" + "\n".join(bb[i:i + 80] for i in range(0, len(bb), 80)) + "\n")
    with open(os.path.join(d, "reads.ref"), "w") as f:
        for k, (tb, qrow, trow, score) in enumerate(records):
            assert len(qrow) == len(trow)
            n, q = len(trow.replace("-", "")), qrow.replace("-", "").replace(".", "")
            assert 0 < n and tb + n <= len(bb)
            f.write(f"r{k} P_1 F {score} 0 {len(q)} {len(q)} {tb} {tb + n} {len(bb)}\n{qrow}\n{trow}\n")
    return d


def rows(rs, seg, ins=(), dels=(), sub=0.0, subs=()):
    """query / target rows over the target segment: insertion runs {offset: length} before seg[offset], deletions at offsets,
    substitutions at rate `sub` and at the offsets `subs`"""
    ins = dict(ins)
    q, t = [], []
    for j, b in enumerate(seg):
        if j in ins:
            q += [ACGT[x] for x in rs.integers(0, 4, ins[j])]
            t += ["-"] * ins[j]
        if j in dels:
            q.append("-")
        elif j in subs or rs.random() < sub:
            q.append(ACGT[(ACGT.index(b) + int(rs.integers(1, 4))) % 4])
        else:
            q.append(b)
        t.append(b)
    return "".join(q), "".join(t)


PART = 500
SEEDED_CASE = dict(part=PART, top_k=3000, alpha=250)
SEEDED_CASE_CUT = dict(part=PART, top_k=4, alpha=250)  # most slices are cut before they are normalised


def seeded_records():
    """-> (backbone, records): 6 parts of 500 bases"""
    rs = np.random.default_rng(31)
    bb = list("".join(ACGT[x] for x in rs.integers(0, 4, 6 * PART)))
    for lo, n, b in [(1200, 40, "A"), (1260, 25, "T"), (2480, 45, "G")]:  # homopolymers, one across the boundary at 2500
        bb[lo:lo + n] = b * n
    bb = "".join(bb)
    recs = []
    add = lambda tb, q, t, score: recs.append((tb, q, t, score))
    # records that start and end exactly on part boundaries, one over one part, one over two, one over all six
    for tb, n in [(0, 500), (500, 1000), (1500, 500), (0, 3000), (2500, 500)]:
        q, t = rows(rs, bb[tb:tb + n], ins={100: 3}, dels={250, 251}, sub=0.03)
        add(tb, q, t, 900)
    # three and more parts, not on boundaries
    for tb, n in [(400, 1300), (130, 2600), (990, 1020)]:
        q, t = rows(rs, bb[tb:tb + n], ins={77: 5, 600: 2}, dels={300, 900}, sub=0.04)
        add(tb, q, t, 850)
    # insertion runs that end at a part boundary (the gap columns just before base 500 / 1000 belong to the earlier slice), runs
    # on both sides of it, and runs before the first and after the last base of the record
    for k in range(6):
        tb = 300 + 11 * k
        at = 500 - tb
        q, t = rows(rs, bb[tb:tb + 900], ins={at: 4 + k, at + 1: 2, at - 1: 3, at + 500: 7}, dels={at - 3, at + 2}, sub=0.02)
        add(tb, q, t, 800 + k)
    # leading and trailing gap columns in the target row
    for k in range(4):
        tb = 700 + 200 * k
        q, t = rows(rs, bb[tb:tb + 450], ins={200: 2}, sub=0.02)
        lead, trail = "ACGTA"[:k + 1], "TTGCA"[:k + 2]
        add(tb, lead + q + trail, "-" * len(lead) + t + "-" * len(trail), 780)
    # runs of mismatches
    for k in range(4):
        tb = 100 + 600 * k
        q, t = rows(rs, bb[tb:tb + 520], subs=set(range(50, 62)) | set(range(300, 340)) | {0, 1, 518, 519}, dels={62, 299})
        add(tb, q, t, 760)
    # '.' in either row, lower case and N
    for k in range(4):
        tb = 250 + 500 * k
        q, t = rows(rs, bb[tb:tb + 700], ins={90: 4, 400: 6}, dels={100, 101, 102, 500}, sub=0.03)
        q = q.replace("-", ".", 3) if k % 2 == 0 else q
        t = t.replace("-", ".", 2) if k >= 1 else t
        q = q[:40].lower() + q[40:]
        q = q.replace("A", "N", 4) if k >= 2 else q
        t = (t[:300] + t[300:].replace("C", "c", 3)) if k == 3 else t
        add(tb, q, t, 740)
    # homopolymer stretches with indels: pushes cascade along the run
    for k in range(8):
        tb = 1150 + 3 * k
        at = 1200 - tb
        q, t = rows(rs, bb[tb:tb + 220], ins={at + 5: 2, at + 20: 1, at + 70: 3}, dels={at + 2, at + 9, at + 10, at + 33, at + 62, at + 80}, sub=0.02)
        add(tb, q, t, 720 + k)
        tb = 2400 + 5 * k
        at = 2480 - tb
        q, t = rows(rs, bb[tb:tb + 200], ins={at + 19: 2, at + 21: 2}, dels={at + 1, at + 18, at + 22, at + 40}, sub=0.02)
        add(tb, q, t, 715)
    # gap runs longer than 64 and longer than 128 columns, in the target row (insertions) and in the query row (deletions): a push
    # that looks past any 64-column chunk
    for k, (run, where) in enumerate([(70, 200), (140, 200), (66, 30), (130, 400), (200, 250)]):
        tb = 50 + 480 * k
        q, t = rows(rs, bb[tb:tb + 600], ins={where: run}, dels=set(range(where + 20, where + 20 + run)), sub=0.02)
        add(tb, q, t, 700)
        # ... and the base after the run equals the one before it, so that the push fires across the whole run
        seg = bb[tb:tb + 300]
        t2 = seg[:100] + "-" * run + seg[100:]
        q2 = seg[:100] + seg[100] + "".join(ACGT[x] for x in rs.integers(0, 4, run - 1)) + "-" + seg[101:]
        add(tb, q2, t2, 690)
    # slices of 1, 2, 63, 64, 65, 127, 128 and 129 columns: records of that many columns inside a part, and records that reach
    # that many columns into the next part
    for k, n in enumerate([1, 2, 63, 64, 65, 127, 128, 129]):
        tb = 520 + 7 * k
        add(tb, bb[tb:tb + n], bb[tb:tb + n], 650 + k)
        tb = 1000 - 100
        q, t = rows(rs, bb[tb:tb + 100 + n], sub=0.0)
        add(tb, q, t, 640 + k)
    # a background, so that every part has more than -k = 4 alignments and a consensus with a body
    for k in range(40):
        tb = int(rs.integers(0, 2400))
        n = int(rs.integers(200, 600))
        q, t = rows(rs, bb[tb:tb + n], ins={int(rs.integers(1, n - 1)): int(rs.integers(1, 6))}, dels={int(rs.integers(1, n - 1))}, sub=0.03)
        add(tb, q, t, 400 + 10 * (k % 7))
    return bb, recs


def slice_columns(dump):
    """the normalised rows' lengths in a dump, per line"""
    return [len(ln.split(b" ")[3]) for ln in dump.splitlines()]
