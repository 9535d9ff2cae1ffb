"""CPU: the row code of pa_cns (csrc/hip/cns_rows.hpp — slice_bounds, normalize_gaps, run_slice: what PA_CNS_INGEST=flat runs on
host threads and PA_CNS_INGEST=device on the lanes of a wavefront) against a std::string restatement of the reference on seeded
rows, in a program of its own (tests/harness/cns_rows_main.cpp, its own main) built with the address and undefined-behaviour
sanitizers: every buffer is a heap block of exactly the size the contract names, so an index past it is a finding.  Host code
only, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED = os.path.join(ROOT, "tests", "harness", "bin", "cns_rows_sanitized")


def test_row_code_against_the_restatement_under_the_sanitizers():
    subprocess.run(["make", "-C", ROOT, SANITIZED[len(ROOT) + 1:]], check=True, capture_output=True)
    r = subprocess.run([SANITIZED], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
