"""CPU: bin/pa_cns's parallel ingest (PA_CNS_INGEST=flat: the file mapped and indexed, the headers parsed on a thread pool, the
per-part lists sorted, cut and weighted from the scores, and only the kept slices cut and gap-normalised by
csrc/hip/cns_rows.hpp) against the host ingest (the std::string restatement the goldens pin): the FASTA and stdout of every
case, the rows themselves (PA_CNS_DUMP_ROWS) byte for byte on the cases and on a seeded file aimed at the row code, the
fallback for files with a record that is not regular, the combinations that cannot run, and the library's entry points.
The device runs the same in tests/test_gpu_pa_cns_ingest.py."""
import os

import pytest

import cns_cases
import cns_ingest_cases as ic
from cns_ingest_cases import EXE, GOLD, REF

CASES = dict(cns_cases.CASES, deep=cns_cases.DEEP_CASE)


@pytest.fixture(scope="module", autouse=True)
def built():
    ic.ensure_built()


def check_against_host(d, case, threads=4):
    """flat ingest == host ingest (both under the flat graph backend): stdout, FASTA and the row dump; -> (stdout, FASTA)"""
    rh, fasta_h, dump_h = ic.run(EXE, d, "host", case, threads, ingest="host", backend="flat")
    rf, fasta_f, dump_f = ic.run(EXE, d, "flat", case, threads, ingest="flat", backend="flat")
    assert rh.returncode == 0 and rf.returncode == 0, (rh.stderr[-500:], rf.stderr[-500:])
    assert "pa_cns: ingest (flat) index " in rf.stderr and "falls back" not in rf.stderr, rf.stderr[-500:]
    assert dump_h and dump_f == dump_h, "the rows of the flat ingest differ from the host ingest's"
    assert rf.stdout == rh.stdout and fasta_f == fasta_h
    return rf.stdout, fasta_f


@pytest.mark.parametrize("name", list(CASES))
def test_flat_ingest_matches_goldens_reference_and_host_rows(name, tmp_path):
    case = CASES[name]
    d = cns_cases.write_case(case, str(tmp_path))
    stdout, fasta = check_against_host(d, case, threads=16 if name == "deep" else 4)
    if name != "deep":
        assert fasta == open(os.path.join(GOLD, name + ".fasta"), "rb").read()
        assert stdout == open(os.path.join(GOLD, name + ".stdout")).read()
    if os.path.exists(REF):
        r, ref_fasta, _ = ic.run(REF, d, "ref", case, threads=5)
        assert r.returncode == 0 and r.stdout == stdout and ref_fasta == fasta


@pytest.mark.parametrize("case", [ic.SEEDED_CASE, ic.SEEDED_CASE_CUT], ids=["all_kept", "cut_to_4"])
def test_flat_ingest_rows_on_the_seeded_file(case, tmp_path):
    bb, recs = ic.seeded_records()
    d = ic.write_rows(str(tmp_path), bb, recs)
    stdout, fasta = check_against_host(d, case)
    dump = open(os.path.join(d, "flat.rows"), "rb").read()
    lines = dump.splitlines()
    n_slices = sum((tb + len(t.replace("-", "")) - 1) // ic.PART - tb // ic.PART + 1 for tb, _, t, _ in recs)
    if case["top_k"] >= 3000:
        assert len(lines) == n_slices
        cols = set(ic.slice_columns(dump))
        assert {1, 2, 63, 64, 65, 127, 128, 129} <= cols, "the seeded file no longer holds the slice lengths it is about"
    else:
        assert len(lines) == 6 * case["top_k"] and n_slices > 3 * len(lines)
    assert [int(ln.split(b" ")[0]) for ln in lines] == sorted(int(ln.split(b" ")[0]) for ln in lines)
    assert len(fasta) > len(bb) // 2
    if os.path.exists(REF):
        r, ref_fasta, _ = ic.run(REF, d, "ref", case, threads=5)
        assert r.returncode == 0 and r.stdout == stdout and ref_fasta == fasta


@pytest.mark.parametrize("name", list(cns_cases.CASES))
def test_host_backend_dumps_the_rows_the_flat_backend_gets(name, tmp_path):
    # the dump is one thing whichever backend builds the graphs: the host backend's, from its lists, is the flat backend's, from
    # the flattened rows of the same host ingest
    case = cns_cases.CASES[name]
    d = cns_cases.write_case(case, str(tmp_path))
    rh, fasta_h, dump_h = ic.run(EXE, d, "host", case, ingest="host", backend="host")
    rf, fasta_f, dump_f = ic.run(EXE, d, "flat", case, ingest="host", backend="flat")
    assert rh.returncode == 0 and rf.returncode == 0, (rh.stderr[-500:], rf.stderr[-500:])
    assert "graph stage (host, with the per-part sort)" in rh.stderr, rh.stderr[-500:]
    assert dump_h and dump_f == dump_h, "the rows the host backend dumps differ from the flat backend's"
    assert fasta_h and fasta_f == fasta_h and rf.stdout == rh.stdout


def _case_with_extra_record(tmp_path, extra):
    case = cns_cases.CASES["three_parts_ties"]
    d = cns_cases.write_case(case, str(tmp_path))
    path = os.path.join(d, "reads.ref")
    text = open(path).read().splitlines(keepends=True)
    text[30:30] = extra(d)  # (after the tenth record)
    open(path, "w").write("".join(text))
    return case, d


def check_fallback(case, d):
    rh, fasta_h, dump_h = ic.run(EXE, d, "host", case, ingest="host", backend="flat")
    rf, fasta_f, dump_f = ic.run(EXE, d, "flat", case, ingest="flat", backend="flat")
    assert rh.returncode == 0 and rf.returncode == 0, (rh.stderr[-500:], rf.stderr[-500:])
    assert "pa_cns: ingest (flat) falls back to the host ingest: record 10 is not regular" in rf.stderr, rf.stderr[-500:]
    assert (rf.stdout, fasta_f, dump_f) == (rh.stdout, fasta_h, dump_h)
    return rf.stdout, fasta_f


def test_a_malformed_header_takes_the_host_ingest(tmp_path):
    # the header's queryBegin is no number: an all-zero record that is still processed, from backbone position 0 over every part
    # (AlignmentHelper.cpp:24-40); its rows cover the whole backbone, so that no slice of it is empty
    def extra(d):
        bb = "".join(ln.strip() for ln in open(os.path.join(d, "backbone.fasta")).read().splitlines()[1:])
        return [f"bad P_1 F 77 x {len(bb)} {len(bb)} 0 {len(bb)} {len(bb)}\n", bb + "\n", bb + "\n"]
    case, d = _case_with_extra_record(tmp_path, extra)
    stdout, fasta = check_fallback(case, d)
    if os.path.exists(REF):
        r, ref_fasta, _ = ic.run(REF, d, "ref", case, threads=5)
        assert r.returncode == 0 and r.stdout == stdout and ref_fasta == fasta


def test_rows_of_unequal_length_take_the_host_ingest(tmp_path):
    # ... in a record no slice reaches: it lies past the last part (leftPart > rightPart), so the host ingest never looks at its rows
    case, d = _case_with_extra_record(tmp_path, lambda d: ["far P_1 F 500 0 9 9 3100 3109 3200\n", "ACGTACGTA\n", "ACGT\n"])
    check_fallback(case, d)


@pytest.mark.parametrize("env_vars, words", [
    (dict(ingest="bogus", backend="flat"), "PA_CNS_INGEST must be host, flat or device"),
    (dict(ingest="flat", backend="host"), "PA_CNS_INGEST=flat needs a graph backend"),
    (dict(ingest="device", backend="flat"), "PA_CNS_INGEST=device leaves the rows on the device"),
])
def test_combinations_that_cannot_run_exit_1_with_one_line(env_vars, words, tmp_path):
    case = cns_cases.CASES["one_part"]
    d = cns_cases.write_case(case, str(tmp_path))
    r, fasta, dump = ic.run(EXE, d, "o", case, **env_vars)
    assert r.returncode == 1, r.stderr[-500:]
    assert words in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr[-500:]
    assert not fasta and not dump


def test_device_ingest_without_a_device_exits_1_with_the_reason(tmp_path):
    import aligngraph2_amd
    if aligngraph2_amd.load_hip().pag_device_available() != 0:
        pytest.skip("a gfx950 device is present: tests/test_gpu_pa_cns_ingest.py runs the mode")
    case = cns_cases.CASES["one_part"]
    d = cns_cases.write_case(case, str(tmp_path))
    r, fasta, _ = ic.run(EXE, d, "o", case, ingest="device", backend="wave")
    assert r.returncode == 1, r.stderr[-500:]
    assert "PA_CNS_INGEST=device" in r.stderr and "no gfx950 device" in r.stderr, r.stderr[-500:]
    assert not fasta


def test_library_exports_the_row_entry_points():
    import aligngraph2_amd
    lib = aligngraph2_amd.load_hip()
    for f in ("pag_cns_normalize", "pag_cns_rows_fetch", "pag_cns_rows_free", "pag_cns_rows_bytes", "pag_cns_rows_times", "pag_cns_rows_counts",
              "pag_cns_consensus_rows", "pag_cns_consensus", "pag_cns_consensus_wave"):
        assert hasattr(lib, f), f
