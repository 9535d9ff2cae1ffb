"""GPU: pa_cns with its graph stage on the device, the lanes of a wavefront sharing a part's work (PA_CNS_BACKEND=wave;
pag_cns_consensus_wave, csrc/hip/k_cns_wave.hip: the columns of an alignment 64 at a time in addAln, the nodes of a level in
bestPath).  Every case runs `wave`, `hip` (one lane per part) and `flat` (the serial graph code on host threads) and compares
all three; the golden outputs and the reference binary where they apply; seeded inputs aimed at the chunking of the columns
(insertion runs across chunk boundaries, alignments of 63 / 64 / 65 columns, alignments that fill their part, repeated
alignments); and parts whose regions are too small, which must report the one-lane kernel's error code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cns_cases
import pagctl
from aligngraph2_amd.capi import CnsAln, CnsPart

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pa_cns")
REF = os.path.join(pagctl.REF_DIR, "pa_cns")
GOLD = os.path.join(pagctl.ROOT, "tests", "golden", "pa_cns")
BACKENDS = ("wave", "hip", "flat")
ACGT = "ACGT"


def run(exe, d, out, case, threads=4, backend=None):
    env = dict(os.environ)
    env.pop("PA_CNS_BACKEND", None)
    if backend:
        env["PA_CNS_BACKEND"] = backend
    return subprocess.run(cns_cases.argv(exe, d, out, case, threads), capture_output=True, text=True, timeout=900, env=env)


def run_three(d, case, tmp_path, threads=4):
    """(stdout, FASTA bytes) of `wave`, after checking that `hip` and `flat` give the same"""
    got = {}
    for be in BACKENDS:
        out = str(tmp_path / (be + ".fasta"))
        r = run(EXE, d, out, case, threads, backend=be)
        assert r.returncode == 0, (be, r.stderr[-800:])
        got[be] = (r.stdout, open(out, "rb").read())
    assert got["wave"] == got["hip"], "wave and hip differ"
    assert got["wave"] == got["flat"], "wave and flat differ"
    return got["wave"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cns_cases.CASES))
def test_wave_matches_golden_reference_and_the_other_backends(name, tmp_path):
    case = cns_cases.CASES[name]
    d = cns_cases.write_case(case, str(tmp_path / "in"))
    stdout, fasta = run_three(d, case, tmp_path)
    assert fasta == open(os.path.join(GOLD, name + ".fasta"), "rb").read()
    assert stdout == open(os.path.join(GOLD, name + ".stdout")).read()
    if os.path.exists(REF):
        r = run(REF, d, str(tmp_path / "ref.fasta"), case, threads=5)
        assert r.returncode == 0 and r.stdout == stdout
        assert fasta == open(tmp_path / "ref.fasta", "rb").read()


@pytest.mark.gpu
def test_wave_at_pipeline_settings(tmp_path):
    case = cns_cases.DEEP_CASE
    d = cns_cases.write_case(case, str(tmp_path / "in"))
    stdout, fasta = run_three(d, case, tmp_path, threads=16)
    want_exe, want_be = (REF, None) if os.path.exists(REF) else (EXE, "host")
    r = run(want_exe, d, str(tmp_path / "want.fasta"), case, threads=16, backend=want_be)
    assert r.returncode == 0 and r.stdout == stdout
    assert fasta == open(tmp_path / "want.fasta", "rb").read()


@pytest.mark.gpu
def test_wave_many_parts(tmp_path):
    case = dict(seed=11, backbone=30000, n_reads=900, read_len=1200, part=500, top_k=3000, alpha=250, score_classes=3)
    d = cns_cases.write_case(case, str(tmp_path / "in"))
    stdout, fasta = run_three(d, case, tmp_path, threads=8)
    assert stdout.startswith("PartNum=61")
    r = run(EXE, d, str(tmp_path / "host.fasta"), case, threads=8, backend="host")
    assert r.returncode == 0 and r.stdout == stdout
    assert fasta == open(tmp_path / "host.fasta", "rb").read()


# ---- seeded inputs aimed at the column chunks -------------------------------------------------------------------------------
def write_rows(d, bb, records):
    """a backbone and 3-line ALN records (tBegin, query row, target row, score); a target row's bases are bb[tBegin:]"""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "backbone.fasta"), "w") as f:
        f.write(">P_1 seeded\n" + "\n".join(bb[i:i + 80] for i in range(0, len(bb), 80)) + "\n")
    with open(os.path.join(d, "reads.ref"), "w") as f:
        for k, (tb, qrow, trow, score) in enumerate(records):
            n, q = len(trow.replace("-", "")), qrow.replace("-", "")
            assert trow.replace("-", "") == bb[tb:tb + n]
            f.write(f"r{k} P_1 F {score} 0 {len(q)} {len(q)} {tb} {tb + n} {len(bb)}\n{qrow}\n{trow}\n")
    return d


def rows(rs, seg, ins=(), dels=(), sub=0.0):
    """query / target rows over the target segment: insertion runs {offset: length} before seg[offset], deletions at offsets,
    substitutions at rate `sub`"""
    ins = dict(ins)
    q, t = [], []
    for j, b in enumerate(seg):
        if j in ins:
            q += [ACGT[x] for x in rs.integers(0, 4, ins[j])]
            t += ["-"] * ins[j]
        if j in dels:
            q.append("-")
        elif rs.random() < sub:
            q.append(ACGT[(ACGT.index(b) + int(rs.integers(1, 4))) % 4])
        else:
            q.append(b)
        t.append(b)
    return "".join(q), "".join(t)


def backbone(rs, n):
    return "".join(ACGT[x] for x in rs.integers(0, 4, n))


def check_seeded(tmp_path, bb, records, part, alpha=250):
    case = dict(part=part, top_k=3000, alpha=alpha)
    d = write_rows(str(tmp_path / "in"), bb, records)
    stdout, fasta = run_three(d, case, tmp_path)
    r = run(EXE, d, str(tmp_path / "host.fasta"), case, backend="host")
    assert r.returncode == 0 and r.stdout == stdout
    assert fasta == open(tmp_path / "host.fasta", "rb").read()
    assert len(fasta) > len(bb) // 2


@pytest.mark.gpu
def test_wave_insertion_runs_across_chunk_boundaries(tmp_path):
    rs = np.random.default_rng(21)
    bb = backbone(rs, 3000)
    recs = []
    for k in range(60):
        tb = int(rs.integers(0, 2200))
        n = int(rs.integers(300, 800))
        seg = bb[tb:tb + n]
        # runs that start just below a multiple of 64 columns, one longer than a chunk, one of exactly a chunk
        ins = {60: 6, 120: 9, 180: 70, 300: 64, int(rs.integers(1, n - 1)): int(rs.integers(1, 20))}
        dels = set(int(x) for x in rs.integers(1, n - 1, 6))
        qrow, trow = rows(rs, seg, ins={o: L for o, L in ins.items() if o < n}, dels=dels, sub=0.03)
        recs.append((tb, qrow, trow, 500 + 100 * (k % 4)))
    check_seeded(tmp_path, bb, recs, part=1000)


@pytest.mark.gpu
def test_wave_alignments_of_63_64_65_columns(tmp_path):
    rs = np.random.default_rng(22)
    bb = backbone(rs, 2000)
    recs = []
    for k, n in enumerate([63, 64, 65, 127, 128, 129, 1, 2] * 6):
        tb = int(rs.integers(0, 2000 - n))
        seg = bb[tb:tb + n]
        recs.append((tb, seg, seg, 400 + 50 * (k % 5)))
    for k in range(20):  # and a background of ordinary reads so that the consensus has a body
        tb = int(rs.integers(0, 1400))
        seg = bb[tb:tb + 600]
        qrow, trow = rows(rs, seg, ins={int(rs.integers(1, 599)): 3}, dels={int(rs.integers(1, 599))}, sub=0.02)
        recs.append((tb, qrow, trow, 600))
    check_seeded(tmp_path, bb, recs, part=700)


@pytest.mark.gpu
def test_wave_alignments_that_fill_their_part_and_repeat(tmp_path):
    rs = np.random.default_rng(23)
    bb = backbone(rs, 3000)
    recs = []
    # from a part's first column to its last, and across all parts; each one three times over, so that edges gain weight
    for tb, n in [(0, 1000), (1000, 1000), (2000, 1000), (0, 3000), (500, 1000)]:
        qrow, trow = rows(rs, bb[tb:tb + n], ins={64: 5, 500: 2}, dels={200, 201}, sub=0.02)
        recs += [(tb, qrow, trow, 700)] * 3
    for k in range(30):
        tb = int(rs.integers(0, 2500))
        seg = bb[tb:tb + 500]
        qrow, trow = rows(rs, seg, ins={int(rs.integers(1, 499)): 2}, sub=0.03)
        recs.append((tb, qrow, trow, 500 + 10 * k))
    check_seeded(tmp_path, bb, recs, part=1000)


# ---- the C ABI: regions too small --------------------------------------------------------------------------------------------
def consensus(fn, bb, parts, alns, qpool, tpool):
    n = len(parts)
    P = (CnsPart * n)(*parts)
    A = (CnsAln * max(1, len(alns)))(*alns)
    out_bytes = sum(p.out_cap for p in parts)
    out = C.create_string_buffer(out_bytes + 16)
    off, ln, err = (C.c_uint64 * (n + 1))(), (C.c_uint32 * n)(), (C.c_int32 * n)()
    rc = fn(0, bb, len(bb), C.cast(P, C.c_void_p), n, C.cast(A, C.c_void_p), len(alns), qpool, tpool, len(qpool), 0,
            C.cast(out, C.c_void_p), out_bytes, C.cast(off, C.c_void_p), C.cast(ln, C.c_void_p), C.cast(err, C.c_void_p))
    assert rc == 0
    return [out.raw[off[i]:off[i] + ln[i]] for i in range(n)], list(err)


@pytest.mark.gpu
def test_wave_reports_the_error_codes_of_the_one_lane_kernel():
    import aligngraph2_amd
    lib = aligngraph2_amd.load_hip()
    fns = [lib.pag_cns_consensus, lib.pag_cns_consensus_wave]
    rs = np.random.default_rng(24)
    L = 150
    bb = backbone(rs, L)
    qpool, tpool, alns = [], [], []

    def add(start, qrow, trow, weight):
        alns.append(CnsAln(sum(map(len, qpool)), len(qrow), start, weight, 0))
        qpool.append(qrow)
        tpool.append(trow)

    # the rows of one part (gap-normalised already: matches, deletions, insertion runs; one across the first chunk boundary)
    for k in range(8):
        s = int(rs.integers(0, 40))
        qrow, trow = rows(rs, bb[s:s + 100], ins={30: 4, 61: 10}, dels={45})
        add(s + 1, qrow, trow, 3 + k)
    n_main = len(alns)
    n_ins = sum(r.count("-") for r in tpool)
    past = bb[L - 6:] + "ACGTACGTAC"  # matches from position L - 5 on, past the exit vertex: an overrun
    add(L - 5, past, past, 2)
    node_cap = L + 2 + n_ins
    edge_cap = L + 1 + sum(len(q) - q.count("-") for q in qpool) + len(alns) + 4096

    def part(first=0, n_aln=n_main, **caps):
        c = dict(node_cap=node_cap, edge_cap=edge_cap, aux_cap=4 * node_cap + 2048, out_cap=node_cap)
        c.update(caps)
        return CnsPart(0, L, n_aln, first, c["node_cap"], c["edge_cap"], c["aux_cap"], c["out_cap"])

    parts = [part(),                               # 0: fits
             part(node_cap=L + 2 + 3),             # 1: nodes run out in addAln
             part(node_cap=L + 1),                 # 2: nodes run out in the backbone
             part(edge_cap=L + 1 + 5),             # 3: edges run out in addAln
             part(edge_cap=L),                     # 4: edges run out in the backbone
             part(aux_cap=2),                      # 5: the merge stack runs out
             part(aux_cap=2 * node_cap),           # 6: a queue that holds exactly every node: the serial bestPath, same result
             part(out_cap=5),                      # 7: the output runs out
             part(first=n_main, n_aln=1)]          # 8: an alignment that runs past its part
    args = (bb.encode(), parts, alns, "".join(qpool).encode(), "".join(tpool).encode())
    out_lane, err_lane = consensus(fns[0], *args)
    out_wave, err_wave = consensus(fns[1], *args)
    assert err_lane == [0, 1, 1, 2, 2, 4, 0, 6, 5]
    assert err_wave == err_lane
    assert out_wave == out_lane and len(out_lane[0]) > 50 and out_lane[6] == out_lane[0]
