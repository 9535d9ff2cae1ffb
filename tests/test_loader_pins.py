"""CPU: the host loaders (seq_db.cpp, aln_db.cpp) against what the REFERENCE's own readers make of the same files.  The
committed dumps under tests/golden/loaders/ were printed by oracle/ref_harness/loader_dump.cpp over AutoSeqDatabase,
MecatAlignDatabase and MummerAlignDatabaseV2 (tests/golden/make_loader_golden.py; each file first under the sanitizers); the
product's databases are printed in the same format (pagt_seqdb_dump, pagt_alndb_dump) and must give the same bytes, on every
path a constructor can take: the thread-pool loaders, the sequential loops (PAGH_SEQUENTIAL_LOADERS=1), a second construction
from the packed sidecar the first one wrote (PAGRAPH_ALN_SIDECAR=1), Mecat under an AlnRecordFilter.  Record order is part
of the bytes: the permutation the reference's std::sort leaves records of equal score in is what AlnDb::sortByScore claims
to reproduce (same libstdc++, same comparator, same initial order).

The files are in tests/loader_cases.py: CRLF (a CR is a base, and a column), text before the first header, `;` lines, blank and
empty headers, duplicate names, partial records, headers of nine fields, signed / exponent / 19- and 20-digit numbers, ties."""
import os
import subprocess

import pytest

import loader_cases
import loader_pins
import pagctl

SEQ = sorted(loader_cases.SEQ_CASES)
ALN = sorted(loader_cases.ALN_CASES)
DB_DUMPS = [(n, "seq") for n in SEQ] + [(n, m) for n in ALN for m in ("mecat", "mummer")]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """the product's text of every file, once per path"""
    d = tmp_path_factory.mktemp("loader_pins")
    out = {}
    for path, env, twice in (("pool", None, False), ("sequential", {"PAGH_SEQUENTIAL_LOADERS": "1"}, False), ("sidecar", {"PAGRAPH_ALN_SIDECAR": "1"}, True)):
        ind, outd = str(d / (path + "_in")), str(d / (path + "_out"))
        if env is None:
            assert "PAGH_SEQUENTIAL_LOADERS" not in os.environ and os.environ.get("PAGRAPH_ALN_SIDECAR") != "1"
            how = loader_pins.dump_all(ind, outd)
        else:
            how = loader_pins.dump_all_in_child(ind, outd, env, twice=twice)
        out[path] = (outd, how)
    return out


def _text(dumps, path, name, mode):
    return open(os.path.join(dumps[path][0], f"{name}.{mode}.txt"), "rb").read()


def test_every_case_has_its_committed_dump_and_no_other():
    want = {f"{n}.{m}.txt" for n, m in loader_cases.all_dumps()}
    have = {f[:-3] if f.endswith(".gz") else f for f in os.listdir(loader_pins.GOLDEN)}
    assert have == want
    for f in os.listdir(loader_pins.GOLDEN):
        assert os.path.getsize(os.path.join(loader_pins.GOLDEN, f)) < (1 << 20)


def test_the_committed_dumps_say_what_the_issue_table_says():
    """a few of the reference's less obvious readings, spelled out (the dumps themselves are the full statement)"""
    g = loader_pins.golden
    assert g("crlf.fa", "seq").splitlines()[:2] == [b"R 0 7231 10 ACGTATTGAA", b"R 1 7232 3 CCA"]          # a CR is a base, packed as A
    assert g("crlf.fq", "seq").splitlines()[0] == b"R 0 61 5 ACGTA"
    assert g("prefix.fa", "seq").splitlines()[0].split()[3] == b"27"                                      # the `;` line is sequence
    assert [ln.split()[2] for ln in g("blank_header.fq", "seq").splitlines()[:3]] == [b"61", b"61", b"-"]  # `a`, `a` again, empty
    assert g("dup.fa", "seq").splitlines()[-1] == b"M 73616d65 1"                                         # the later `same` wins
    assert g("odd_numbers.aln", "mecat").splitlines()[0].split()[5] == str(2 ** 64 - 7).encode()          # score -7 sorts first
    assert g("crlf.aln", "mecat").splitlines()[1].split()[10:] == [b"00100", b"00000"]                    # CR = CR is a match
    order = [bytes.fromhex(ln.split()[2].decode()) for ln in g("ties40.aln", "mecat").splitlines()[:8]]
    assert order == [b"q29", b"q20", b"q17", b"q23", b"q14", b"q26", b"q11", b"q8"]                       # far from file order
    assert g("ties40.aln", "mummer") != g("ties40.aln", "mecat")


@pytest.mark.parametrize("path", ["pool", "sequential"])
@pytest.mark.parametrize("name,mode", DB_DUMPS)
def test_the_product_s_database_is_the_reference_s(dumps, path, name, mode):
    assert dumps[path][1][f"{name}.{mode}"] == [0], "the hook failed, or an alignment database did not come from its text"
    loader_pins.assert_same_text(_text(dumps, path, name, mode), loader_pins.golden(name, mode), f"{name} ({mode}, {path} loaders)")


@pytest.mark.parametrize("name", ALN)
@pytest.mark.parametrize("mode", ["mecat", "mummer"])
def test_a_database_loaded_from_its_sidecar_is_the_reference_s(dumps, name, mode):
    """PAGRAPH_ALN_SIDECAR=1: the first construction parses the text and writes <file>.pagaln, the second one loads it"""
    assert dumps["sidecar"][1][f"{name}.{mode}"] == [0, 1]
    loader_pins.assert_same_text(_text(dumps, "sidecar", name, mode), loader_pins.golden(name, mode), f"{name} ({mode}, from the sidecar)")


@pytest.mark.parametrize("path", ["pool", "sequential"])
@pytest.mark.parametrize("name", ALN)
def test_a_filtered_mecat_database_keeps_headers_and_its_own_columns(dumps, path, name):
    """AlnRecordFilter (aln_db.hpp): the kept records are the reference's, the others keep their header fields and their place in
    the sorted order, and have no columns"""
    assert dumps[path][1][name + ".mecat_filtered"] == [0]
    want, _, _ = loader_pins.filtered_expectation(name)
    loader_pins.assert_same_text(_text(dumps, path, name, "mecat_filtered"), want, f"{name} (mecat, filtered, {path} loaders)")


def test_the_filter_of_the_hook_splits_the_fixtures():
    kept = dropped = 0
    for name in ALN:
        _, k, d = loader_pins.filtered_expectation(name)
        kept, dropped = kept + k, dropped + d
    assert kept >= 20 and dropped >= 20


@pytest.mark.parametrize("name", [n for n in SEQ if loader_cases.SEQ_CASES[n][:1] in (b">", b";")])
def test_the_tests_own_fasta_reader_is_the_reference_s(name, tmp_path):
    """goldens.reference_fasta — what the Python restatements of the suite (dump_text, seq_text, find_rule) read contigs and
    references with — gives the reference's names, lengths and stored letters on every FASTA file of the pins"""
    import goldens
    path = tmp_path / name
    path.write_bytes(loader_cases.SEQ_CASES[name])
    got = [b"R %d %s %d %s" % (i, n.encode().hex().encode() or b"-", len(s), s.encode() or b"-") for i, (n, s) in enumerate(goldens.reference_fasta(str(path)))]
    assert got == [ln for ln in loader_pins.golden(name, "seq").splitlines() if ln.startswith(b"R ")]


def test_the_committed_dumps_are_what_the_reference_prints_today(tmp_path):
    """where the reference's readers were built (oracle/_ref/loader_dump): every committed dump, byte for byte"""
    exe = os.path.join(pagctl.REF_DIR, "loader_dump")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/loader_dump was not built (needs the reference's sources at build time)")
    loader_cases.write_inputs(str(tmp_path))
    for name, mode in loader_cases.all_dumps():
        r = subprocess.run([exe, mode, str(tmp_path / name)], capture_output=True)
        assert r.returncode == 0 and not r.stderr, (name, mode, r.stderr[-500:])
        loader_pins.assert_same_text(loader_pins.golden(name, mode), r.stdout, f"{name} ({mode}): committed dump against the reference")
