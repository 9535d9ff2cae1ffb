"""CPU: the C oracle's graph build against the compiled reference's on inputs too heavy for the walk tests
(tests/golden/graph_only/, recorded results only: the dumps are megabytes)."""
import hashlib
import os
import subprocess

import pytest

import heavy_cases
import pagctl

BIN = os.path.join(pagctl.ROOT, "tests", "harness", "bin")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.run(["make", "-C", pagctl.ROOT, "harness"], check=True, capture_output=True)


def _oracle_dump(ind, out, spec, cov):
    os.makedirs(out, exist_ok=True)
    subprocess.run([os.path.join(BIN, "oracle_graph_dump"), "-k", ind + "/kmer.bin", "-c", ind + "/ctg.fasta", "-R", ind + "/ref.fasta",
                    "-p", ind, "-a", ind + "/aln", "-o", out, "-t", str(spec["threads"]), "--epsilon", str(spec["epsilon"]), "-v",
                    str(cov)], check=True)
    assert os.listdir(out) == ["0.graph.txt"]
    return open(os.path.join(out, "0.graph.txt"), "rb").read()


def test_cov_reject_graph_equals_reference_graph(workdir):
    """tests/prep_cases.py's `reject` at its -v (80): the sorted-coverage filter (quirk Q3) takes a third of pass 2 away, with
    coverage-only records, records on the decoy references and per-read lists of up to 60 alignments in the input.  The oracle's
    dump has the length and SHA-256 of the compiled reference's; at -v 0 its count line is the reference's too, and another."""
    name = "cov_reject_t4"
    spec, golden = heavy_cases.load(name)
    assert spec["rewrite"] and spec["cov"] > 0
    ind = heavy_cases.materialize(name, str(workdir / name / "in"))
    got = _oracle_dump(ind, str(workdir / name / "graph"), spec, spec["cov"])
    assert got.split(b"\n", 1)[0] == b"S " + b" ".join(b"%d" % c for c in golden["counts"])
    assert len(got) == golden["bytes"]
    assert hashlib.sha256(got).hexdigest() == golden["sha256"]
    assert got.count(b"\nK ") == golden["n_nodes"]
    got0 = _oracle_dump(ind, str(workdir / name / "graph0"), spec, 0)
    assert got0.split(b"\n", 1)[0] == b"S " + b" ".join(b"%d" % c for c in golden["counts_cov0"])
    # the filter removed something: fewer positions after pass 2 (the fifth number), the same after pass 1 (the second)
    assert golden["counts"][4] < golden["counts_cov0"][4] and golden["counts"][1] == golden["counts_cov0"][1]


def test_count_wrap_graph_equals_reference_graph(workdir):
    """A poly-A k-mer with 151 049 tuples, 85 513 of them left in its counts: the reference's u16 CountType wrapped once.  The oracle's
    dump has the length and SHA-256 of the reference's (byte-identical), and the input still makes a count wrap."""
    name = "count_wrap_t8"
    spec, golden = heavy_cases.load(name)
    ind = heavy_cases.materialize(name, str(workdir / name / "in"))
    out = str(workdir / name / "graph")
    os.makedirs(out, exist_ok=True)
    subprocess.run([os.path.join(BIN, "oracle_graph_dump"), "-k", ind + "/kmer.bin", "-c", ind + "/ctg.fasta", "-R", ind + "/ref.fasta",
                    "-p", ind, "-a", ind + "/aln", "-o", out, "-t", str(spec["threads"]), "--epsilon", str(spec["epsilon"]), "-v",
                    str(spec["cov"])], check=True)
    assert os.listdir(out) == ["0.graph.txt"]
    got = open(os.path.join(out, "0.graph.txt"), "rb").read()
    assert got.split(b"\n", 1)[0] == b"S " + b" ".join(b"%d" % c for c in golden["counts"])
    assert len(got) == golden["bytes"]
    assert hashlib.sha256(got).hexdigest() == golden["sha256"]

    # the condition on the input, from the oracle's own arrays: a node whose counts sum to its raw tuples minus k * 65 536, k > 0
    inp = pagctl.LoadedInput(ind, threads=spec["threads"], eps=spec["epsilon"], cov=spec["cov"])
    try:
        res = pagctl.run_oracle(inp, streams=True)
    finally:
        inp.close()
    assert len(res["csr"]["node_code"]) == golden["n_nodes"]
    deficits = heavy_cases.count_deficits(res)
    assert deficits and all(raw > s and (raw - s) % 65536 == 0 for _, raw, s in deficits), deficits
    assert [{"code": c, "count_sum": s, "raw_tuples": raw, "deficit": raw - s} for c, raw, s in deficits] == golden["wrapped_nodes"]
