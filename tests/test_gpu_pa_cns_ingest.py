"""GPU: bin/pa_cns with its rows made on the device (PA_CNS_INGEST=device; pag_cns_normalize, csrc/hip/k_cns_rows.hip over
csrc/hip/cns_rows.hpp) and left there for the graph kernels (pag_cns_consensus_rows), under both device backends: FASTA and
stdout against the goldens and the reference binary, the rows (PA_CNS_DUMP_ROWS) against the host ingest's byte for byte, on
the suite's cases and on the seeded file of tests/cns_ingest_cases.py; the C ABI through ctypes; the kernel's work rows forced
small, so that the longer slices take the host path; and the text forced up in several pieces."""
import ctypes as C
import os
import re

import pytest

import cns_cases
import cns_ingest_cases as ic
from aligngraph2_amd.capi import CnsRow, CnsSlice
from cns_ingest_cases import EXE, GOLD, PART, REF

CASES = dict(cns_cases.CASES, deep=cns_cases.DEEP_CASE)
COUNTS = re.compile(r"pa_cns: rows on the device: (\d+) slices, (\d+) pieces, (\d+) oversize")
_host = {}


def host_run(key, d, case, threads=4, ingest="host"):
    """the host (or flat) ingest's (stdout, FASTA, dump) under the flat backend, once per input"""
    key = (key, ingest)
    if key not in _host:
        r, fasta, dump = ic.run(EXE, d, ingest, case, threads, ingest=ingest, backend="flat")
        assert r.returncode == 0 and dump, r.stderr[-500:]
        _host[key] = (r.stdout, fasta, dump)
    return _host[key]


def device_run(d, case, backend, threads=4, **kw):
    r, fasta, dump = ic.run(EXE, d, "dev_" + backend, case, threads, ingest="device", backend=backend, **kw)
    assert r.returncode == 0, r.stderr[-800:]
    assert "pa_cns: ingest (device) index " in r.stderr and "falls back" not in r.stderr, r.stderr[-500:]
    m = COUNTS.search(r.stderr)
    assert m, r.stderr[-500:]
    return (r.stdout, fasta, dump), tuple(map(int, m.groups()))


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["wave", "hip"])
@pytest.mark.parametrize("name", list(CASES))
def test_device_ingest_matches_goldens_reference_and_host_rows(name, backend, tmp_path):
    case = CASES[name]
    threads = 16 if name == "deep" else 4
    d = cns_cases.write_case(case, str(tmp_path))
    want = host_run((name, str(tmp_path)), d, case, threads)
    got, (n_slices, _, oversize) = device_run(d, case, backend, threads)
    assert got[2] == want[2], "the rows made on the device differ from the host ingest's"
    assert got == want
    assert n_slices == len(want[2].splitlines()) and oversize == 0
    stdout, fasta, _ = got
    if name != "deep":
        assert fasta == open(os.path.join(GOLD, name + ".fasta"), "rb").read()
        assert stdout == open(os.path.join(GOLD, name + ".stdout")).read()
    if os.path.exists(REF):
        r, ref_fasta, _ = ic.run(REF, d, "ref", case, threads=5)
        assert r.returncode == 0 and r.stdout == stdout and ref_fasta == fasta


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    bb, recs = ic.seeded_records()
    d = ic.write_rows(str(tmp_path_factory.mktemp("seeded")), bb, recs)
    return bb, recs, d


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["wave", "hip"])
@pytest.mark.parametrize("case", [ic.SEEDED_CASE, ic.SEEDED_CASE_CUT], ids=["all_kept", "cut_to_4"])
def test_device_ingest_rows_on_the_seeded_file(case, backend, seeded):
    bb, recs, d = seeded
    want = host_run(("seeded", case["top_k"]), d, case)
    got, (n_slices, _, oversize) = device_run(d, case, backend)
    assert got[2] == want[2], "the rows made on the device differ from the host ingest's"
    assert got == want and oversize == 0
    assert n_slices == (6 * case["top_k"] if case["top_k"] < 3000 else len(want[2].splitlines()))
    if os.path.exists(REF):
        r, ref_fasta, _ = ic.run(REF, d, "ref", case, threads=5)
        assert r.returncode == 0 and r.stdout == got[0] and ref_fasta == got[1]


def slices_of(recs, bb_len):
    """every slice of every record as (record, part, start, columns before normalisation): AlignData.cpp:11-34, :51-61 restated"""
    out = []
    n_parts = (bb_len + PART - 1) // PART
    for r, (tb, _, t, _) in enumerate(recs):
        te = tb + len(t.replace("-", ""))
        lp, rp = tb // PART, min((te - 1) // PART, n_parts - 1)
        for p in range(lp, rp + 1):
            lo, hi, cnt, left = p * PART, min((p + 1) * PART, bb_len), 0, 0
            while left < len(t) and (t[left] == "-" or tb + cnt < lo):
                cnt += t[left] != "-"
                left += 1
            right = left
            while right < len(t) and (t[right] == "-" or tb + cnt < hi):
                cnt += t[right] != "-"
                right += 1
            out.append((r, p, tb - lp * PART + 1 if p == lp else 1, right - left))
    return out


@pytest.mark.gpu
def test_work_rows_forced_small_send_the_longer_slices_to_the_host(seeded):
    bb, recs, d = seeded
    case = ic.SEEDED_CASE
    want = host_run(("seeded", case["top_k"]), d, case)
    got, (n_slices, _, oversize) = device_run(d, case, "wave", stage_cols=128)  # 128 expanded columns: slices of up to 64
    longer = sum(1 for s in slices_of(recs, len(bb)) if s[3] > 64)
    assert 0 < longer < n_slices and oversize == longer
    assert got == want


@pytest.mark.gpu
def test_text_forced_up_in_pieces(seeded):
    bb, recs, d = seeded
    case = ic.SEEDED_CASE
    want = host_run(("seeded", case["top_k"]), d, case)
    size = os.path.getsize(os.path.join(d, "reads.ref"))
    got, (_, pieces, oversize) = device_run(d, case, "wave", piece_bytes=size // 5)
    assert pieces >= 3 and oversize == 0
    assert got == want


@pytest.mark.gpu
def test_normalize_and_fetch_through_the_c_abi(seeded):
    import aligngraph2_amd
    lib = aligngraph2_amd.load_hip()
    bb, recs, d = seeded
    case = ic.SEEDED_CASE
    want = host_run(("seeded", case["top_k"]), d, case, ingest="flat")  # (-k keeps everything: the dump holds every slice's rows, the flat code's)
    text = open(os.path.join(d, "reads.ref"), "rb").read()
    starts = [0]
    for ln in text.splitlines(keepends=True):
        starts.append(starts[-1] + len(ln))
    sl = slices_of(recs, len(bb))
    S = (CnsSlice * len(sl))()
    off = 0
    for k, (r, p, _, _) in enumerate(sl):  # (record order is text order)
        n_cols = len(recs[r][2])
        S[k] = CnsSlice(starts[3 * r + 1], starts[3 * r + 2], recs[r][0], p * PART, min((p + 1) * PART, len(bb)), off, n_cols, 2 * n_cols, k, 0)
        off += 2 * n_cols
    R = (CnsRow * len(sl))()
    handle = C.c_void_p()
    rc = lib.pag_cns_normalize(0, text, len(text), C.cast(S, C.c_void_p), len(sl), C.cast(R, C.c_void_p), C.byref(handle))
    assert rc == 0, lib.pag_last_error()
    try:
        assert lib.pag_cns_rows_bytes(handle) == off
        q, t = C.create_string_buffer(off), C.create_string_buffer(off)
        assert lib.pag_cns_rows_fetch(handle, C.cast(q, C.c_void_p), C.cast(t, C.c_void_p), off) == 0
        assert lib.pag_cns_rows_fetch(handle, C.cast(q, C.c_void_p), C.cast(t, C.c_void_p), off - 1) == -22
    finally:
        lib.pag_cns_rows_free(handle)
    got = []
    for k, (r, p, start, _) in enumerate(sl):
        assert R[k].flag == 0 and R[k].str_off == S[k].out_off
        qrow, trow = q.raw[R[k].str_off:R[k].str_off + R[k].len], t.raw[R[k].str_off:R[k].str_off + R[k].len]
        assert R[k].n_ins == sum(1 for a, b in zip(qrow, trow) if a != 45 and b == 45)
        assert R[k].n_edge_cols == sum(1 for a in qrow if a != 45)
        got.append((p, start, qrow, trow))
    expected = []
    for ln in want[2].splitlines():
        p, start, _, qrow, trow = ln.split(b" ")
        expected.append((int(p), int(start), qrow, trow))
    assert sorted(got) == sorted(expected)  # (rows, and with them lengths and both counts, are the flat code's)
