"""CPU: the golden case messy_inputs_t1 (tests/messy_cases.py, tests/golden/make_messy_golden.py) holds what it is named for.
Counted from the COMMITTED input files: lower-case bases, N / R / Y / K / M, CR bytes at the end of sequence lines, ALN columns that
mismatch by case alone.  Every test that iterates goldens.case_names() runs the case against the reference's recorded outputs;
this file only makes sure that those runs see the messy bytes, and that the reference's recorded results depend on them."""
import hashlib
import os

import goldens
import messy_cases


def test_the_committed_inputs_hold_what_the_case_is_named_for(tmp_path):
    ind = goldens.materialize_inputs(messy_cases.NAME, str(tmp_path / "in"))
    counts = messy_cases.census(ind)
    print(counts)
    for what in ("lower_case_bases", "iupac_bases", "cr_bytes_in_sequence_lines", "case_only_mismatch_columns"):
        assert counts[what] > 0, what
    assert counts["lower_case_ref_row_letters"] == 0  # (query rows only: a lower-case stretch is never lower-case on both rows)
    assert counts == goldens.load_spec(messy_cases.NAME)["census"]
    # every read and both contigs end in a CR, which the reference's reader takes for a base: one per record
    fq = open(os.path.join(ind, "0.new.fastq"), "rb").read().split(b"\n")
    assert all(ln.endswith(b"\r") for ln in fq[1:-1:4]) and len(fq[1:-1:4]) == messy_cases.SPEC["n_reads"]
    ctg = [ln for ln in open(os.path.join(ind, "ctg.fasta"), "rb").read().split(b"\n") if ln]
    assert len(ctg) == 2 * len(messy_cases.SPEC["contigs"]) and all(ln.endswith(b"\r") for ln in ctg)
    assert b"\r" not in open(os.path.join(ind, "ref.fasta"), "rb").read()
    for f in ("0.ctg.ref", "0.ref.ref", "aln"):
        assert b"\r" not in open(os.path.join(ind, f), "rb").read()


def test_the_generator_still_writes_the_committed_inputs(tmp_path):
    import json
    d = messy_cases.generate(str(tmp_path / "gen"))
    want = json.load(open(os.path.join(goldens.GOLDEN, messy_cases.NAME, "inputs.sha256")))
    assert {f: hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d))} == want


def test_the_reference_s_results_depend_on_the_messy_bytes():
    """spec.json records the SHA-256 of the reference's outputs and graph for the rewritten inputs and for the same Spec
    without the rewrite: the first set is what is committed, and the second differs from it"""
    spec = goldens.load_spec(messy_cases.NAME)
    messy, clean = spec["sha256"]["messy"], spec["sha256"]["clean"]
    assert {f: hashlib.sha256(data).hexdigest() for f, data in goldens.golden_out_files(messy_cases.NAME).items()} == messy["out"]
    assert hashlib.sha256(goldens.golden_graph(messy_cases.NAME)).hexdigest() == messy["graph"]
    assert messy["graph"] != clean["graph"]
    differing = [f for f in messy["out"] if f != "contig.txt" and clean["out"].get(f) != messy["out"][f]]
    assert differing, "no output file of the reference changed with the rewrite"
    assert spec["threads"] == 1
    assert goldens.case_names().index(messy_cases.NAME) > goldens.case_names().index("join_rev_t16")  # (the [:3] subsets keep their cases)
