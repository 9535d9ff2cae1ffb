"""CPU: bin/pa_cns --batch <manifest> — the jobs of many contigs in one run, their parts gathered into groups and handed to the
graph stage in one call per group (runBatch in csrc/host/pa_cns_main.cpp), here under PA_CNS_BACKEND=flat.  Every job's output
file and the whole stdout are what the single runs (pa_cns -i B -a A -o O, same flags) write: the same binary's under
PA_CNS_BACKEND=host and the compiled reference's; however the jobs are grouped and whichever ingest reads them; and on the goldens.
What a batch refuses, the Python helper, and the program itself under the address and undefined-behaviour sanitizers.
The device backends run the same manifest in tests/test_gpu_pa_cns_batch.py."""
import os
import subprocess

import pytest

import cns_batch_cases as bc
import cns_cases
from cns_batch_cases import EXE, GOLD, REF

SANITIZED = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "harness", "bin", "pa_cns_sanitized")


@pytest.fixture(scope="module")
def eight(tmp_path_factory):
    """the eight jobs and their single runs under the host backend: (jobs, stdout, {name: FASTA})"""
    bc.ensure_built()
    root = str(tmp_path_factory.mktemp("batch"))
    jobs = bc.write_jobs(os.path.join(root, "in"))
    stdout, fastas = bc.singles(EXE, jobs, os.path.join(root, "single"), PA_CNS_BACKEND="host")
    assert [int(ln[8:]) for ln in stdout.splitlines() if ln.startswith("PartNum=")] == [bc.PARTS[n] for n in bc.ORDER]
    assert sum(bc.PARTS.values()) == 41
    return jobs, stdout, fastas


def check(r, got, stdout, fastas):
    assert r.returncode == 0, r.stderr[-800:]
    assert r.stdout == stdout
    for name, fasta in fastas.items():
        assert got[name] == fasta, name


def test_eight_job_batch_equals_the_single_runs_and_the_reference(eight, tmp_path):
    jobs, stdout, fastas = eight
    r, got = bc.run_batch(EXE, jobs, str(tmp_path), PA_CNS_BACKEND="flat", PA_CNS_STAGE_TIMES=1)
    check(r, got, stdout, fastas)
    assert "pa_cns: group 0: jobs 8 parts 41 " in r.stderr and "group 1" not in r.stderr, r.stderr[-800:]
    # an empty and a missing alignment file are valid jobs: the backbone comes back
    for name in ("empty_aln", "missing_aln"):
        bb = "".join(open(dict((j[0], j[1]) for j in jobs)[name]).read().splitlines()[1:])
        assert b"".join(got[name].splitlines()[1:]).decode() == bb
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/pa_cns was not built: the half against the compiled reference is skipped")
    ref_stdout, ref_fastas = bc.singles(REF, jobs, str(tmp_path / "ref"))
    check(r, got, ref_stdout, ref_fastas)


@pytest.mark.parametrize("env, groups", [
    (dict(PA_CNS_BATCH_PARTS=1), 8),           # a group per job
    (dict(PA_CNS_BATCH_PARTS=5), 5),           # 3+4 | 3+3 | 18 | 4+3 | 3
    (dict(PA_CNS_BATCH_BYTES=4096), 7),        # every job with rows closes its group; the one with an empty file (no rows) joins the next
    (dict(PA_CNS_INGEST="host"), 1),
], ids=["group_per_job", "parts_5", "bytes_small", "ingest_host"])
def test_grouping_and_ingest_variants_give_the_same_bytes(eight, env, groups, tmp_path):
    jobs, stdout, fastas = eight
    r, got = bc.run_batch(EXE, jobs, str(tmp_path), PA_CNS_BACKEND="flat", PA_CNS_STAGE_TIMES=1, **env)
    check(r, got, stdout, fastas)
    n_groups = sum(1 for ln in r.stderr.splitlines() if ln.startswith("pa_cns: group "))
    assert n_groups == groups, r.stderr[-1500:]
    assert ("ingest host" if "PA_CNS_INGEST" in env else "ingest flat") in r.stderr


@pytest.mark.parametrize("name", list(cns_cases.CASES))
def test_one_job_batch_equals_the_golden(name, tmp_path):
    bc.ensure_built()
    case = cns_cases.CASES[name]
    d = cns_cases.write_case(case, str(tmp_path / "in"))
    job = (name, os.path.join(d, "backbone.fasta"), os.path.join(d, "reads.ref"))
    r, got = bc.run_batch(EXE, [job], str(tmp_path), flags=case, PA_CNS_BACKEND="flat")
    assert r.returncode == 0, r.stderr[-500:]
    assert got[name] == open(os.path.join(GOLD, name + ".fasta"), "rb").read()
    assert r.stdout == open(os.path.join(GOLD, name + ".stdout")).read()


def test_a_job_with_an_irregular_record_takes_the_host_ingest_alone(eight, tmp_path):
    # the malformed header of tests/test_pa_cns_ingest.py: queryBegin is no number, an all-zero record that is still processed
    jobs, _, _ = eight
    case = cns_cases.CASES["three_parts_ties"]
    d = cns_cases.write_case(case, str(tmp_path / "irregular"))
    bb = "".join(ln.strip() for ln in open(os.path.join(d, "backbone.fasta")).read().splitlines()[1:])
    path = os.path.join(d, "reads.ref")
    text = open(path).read().splitlines(keepends=True)
    text[30:30] = [f"bad P_1 F 77 x {len(bb)} {len(bb)} 0 {len(bb)} {len(bb)}\n", bb + "\n", bb + "\n"]
    open(path, "w").write("".join(text))
    three = [jobs[0], ("irregular", os.path.join(d, "backbone.fasta"), path), jobs[2]]
    stdout, fastas = bc.singles(EXE, three, str(tmp_path / "single"), PA_CNS_BACKEND="host")
    r, got = bc.run_batch(EXE, three, str(tmp_path), PA_CNS_BACKEND="flat", PA_CNS_STAGE_TIMES=1)
    check(r, got, stdout, fastas)
    falls = [ln for ln in r.stderr.splitlines() if "falls back to the host ingest" in ln]
    assert len(falls) == 1 and path in falls[0] and "record 10 is not regular" in falls[0], r.stderr[-800:]


def refused(r, got, code, words):
    assert r.returncode == code, (r.returncode, r.stderr[-500:])
    lines = r.stderr.strip().splitlines()
    assert words in r.stderr, r.stderr[-500:]
    assert all(v is None for v in got.values()) and r.stdout == ""
    return lines


def test_batch_with_an_input_flag_is_a_parse_error(eight, tmp_path):
    jobs, _, _ = eight
    outs = bc.write_manifest(str(tmp_path / "m.tsv"), jobs[:2], str(tmp_path / "out"))
    r = subprocess.run([EXE, *bc.flag_argv(bc.FLAGS), "--batch", str(tmp_path / "m.tsv"), "-i", jobs[0][1]], capture_output=True, text=True, env=bc.clean_env(PA_CNS_BACKEND="flat"))
    assert r.returncode == 1 and r.stderr.splitlines()[0].startswith("Flag 'batch'") and "--batch=[manifest]" in r.stderr, r.stderr[-800:]
    assert not any(os.path.exists(p) for p in outs.values())
    usage = subprocess.run([EXE, "-h"], capture_output=True, text=True).stderr
    assert sum("--batch" in ln for ln in usage.splitlines()) == 1


@pytest.mark.parametrize("lines, words", [
    (["{bb}\t{aln}\t{out}", "{bb}\t{out}2"], "line 2: a job is three TAB-separated fields"),
    (["{bb}\t{aln}\t{out}", "", "{bb}\t{aln}\t{out}2\textra"], "line 3: a job is three TAB-separated fields"),
    (["{bb}\t{aln}\t{out}", "{bb}\t{aln}\t{out}2", "", "{bb}\t{aln}\t{out}"], "line 4: the output"),
], ids=["two_fields", "four_fields", "duplicate_output"])
def test_malformed_manifests_exit_1_with_one_line_naming_the_line(eight, lines, words, tmp_path):
    jobs, _, _ = eight
    _, bb, aln = jobs[0]
    out = str(tmp_path / "o.fasta")
    open(tmp_path / "m.tsv", "w").write("".join(ln.format(bb=bb, aln=aln, out=out) + "\n" for ln in lines))
    r = subprocess.run([EXE, *bc.flag_argv(bc.FLAGS), "--batch", str(tmp_path / "m.tsv")], capture_output=True, text=True, env=bc.clean_env(PA_CNS_BACKEND="flat"))
    assert r.returncode == 1 and words in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr[-500:]
    assert r.stdout == "" and not os.path.exists(out) and not os.path.exists(out + "2")


@pytest.mark.parametrize("env, words", [
    (dict(PA_CNS_BACKEND="host"), "PA_CNS_BACKEND=host"),
    (dict(PA_CNS_BACKEND="flat", PA_CNS_INGEST="device"), "PA_CNS_INGEST=device"),
    (dict(PA_CNS_BACKEND="flat", PA_CNS_DUMP_ROWS="rows.txt"), "PA_CNS_DUMP_ROWS"),
], ids=["backend_host", "ingest_device", "dump_rows"])
def test_what_a_batch_does_not_take_exits_1_with_one_line(eight, env, words, tmp_path):
    jobs, _, _ = eight
    r, got = bc.run_batch(EXE, jobs[:3], str(tmp_path), **env)
    assert len(refused(r, got, 1, words)) == 1
    assert not os.path.exists("rows.txt")


def test_a_job_without_a_backbone_among_good_ones_exits_2_before_any_work(eight, tmp_path):
    jobs, _, _ = eight
    open(tmp_path / "empty.fasta", "w").close()
    for bad in (str(tmp_path / "missing.fasta"), str(tmp_path / "empty.fasta")):
        mixed = [jobs[0], jobs[1], ("nobb", bad, jobs[2][2]), jobs[2]]
        r, got = bc.run_batch(EXE, mixed, str(tmp_path / ("run_" + os.path.basename(bad))), PA_CNS_BACKEND="flat", PA_CNS_BATCH_PARTS=1)
        lines = refused(r, got, 2, "[Error] No backbone")
        assert len(lines) == 1 and bad in lines[0]


def test_a_failing_job_ends_the_run_and_the_finished_groups_stay(eight, tmp_path):
    # a record whose query row is shorter than its target row, over two parts: the host ingest's substr throws for the second
    # part, as the reference's does — a failure the single run reports with exit 1
    jobs, stdout, fastas = eight
    case = cns_cases.CASES["three_parts_ties"]
    d = cns_cases.write_case(case, str(tmp_path / "failing"))
    bb = "".join(ln.strip() for ln in open(os.path.join(d, "backbone.fasta")).read().splitlines()[1:])
    with open(os.path.join(d, "reads.ref"), "a") as f:
        f.write(f"short P_1 F 500 0 4 4 0 1400 {len(bb)}\nACGT\n{bb[:1400]}\n")
    bad = ("failing", os.path.join(d, "backbone.fasta"), os.path.join(d, "reads.ref"))
    alone = bc.run_single(EXE, bad, str(tmp_path / "alone.fasta"), PA_CNS_BACKEND="host")
    assert alone.returncode == 1 and not os.path.exists(tmp_path / "alone.fasta"), alone.stderr[-500:]
    four = [jobs[0], jobs[1], bad, jobs[2]]
    r, got = bc.run_batch(EXE, four, str(tmp_path), PA_CNS_BACKEND="flat", PA_CNS_BATCH_PARTS=1)
    assert r.returncode == 1, r.stderr[-500:]
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("pa_cns: " + bad[1] + ": "), r.stderr[-500:]
    assert got[jobs[0][0]] == fastas[jobs[0][0]] and got[jobs[1][0]] == fastas[jobs[1][0]]
    assert got["failing"] is None and got[jobs[2][0]] is None
    assert r.stdout == "".join(stdout.splitlines(keepends=True)[:6])
    # ... and in one group with the others nothing is written at all
    r, got = bc.run_batch(EXE, four, str(tmp_path / "one_group"), PA_CNS_BACKEND="flat")
    assert r.returncode == 1 and all(v is None for v in got.values()) and r.stdout == "", r.stderr[-500:]


def test_a_device_backend_without_a_device_exits_1_with_the_library_s_reason(eight, tmp_path):
    import aligngraph2_amd
    if aligngraph2_amd.load_hip().pag_device_available() != 0:
        pytest.skip("a gfx950 device is present: tests/test_gpu_pa_cns_batch.py runs the backend")
    jobs, _, _ = eight
    r, got = bc.run_batch(EXE, jobs[:3], str(tmp_path), PA_CNS_BACKEND="wave")
    lines = refused(r, got, 1, "pag_cns_consensus_wave")
    assert len(lines) == 1 and jobs[0][1] in lines[0] and "no gfx950 device" in lines[0], r.stderr[-500:]


def test_python_helper_runs_two_jobs(eight, tmp_path):
    import aligngraph2_amd
    jobs, _, fastas = eight
    assert aligngraph2_amd.PA_CNS == EXE
    two = [(jobs[1][1], jobs[1][2], str(tmp_path / "a.fasta")), (jobs[5][1], jobs[5][2], str(tmp_path / "b.fasta"))]
    r = aligngraph2_amd.run_pa_cns_batch(two, part_len=700, top_k=3000, alpha=250, threads=4, capture_output=True, text=True,
                                         env=bc.clean_env(PA_CNS_BACKEND="flat"))
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout.splitlines()[0::3] == [f"PartNum={bc.PARTS[jobs[1][0]]}", f"PartNum={bc.PARTS[jobs[5][0]]}"]
    assert open(two[0][2], "rb").read() == fastas[jobs[1][0]] and open(two[1][2], "rb").read() == fastas[jobs[5][0]]


def test_the_program_under_the_sanitizers_runs_the_batch_clean(eight, tmp_path):
    # a program of its own (its own main), built with -fsanitize=address,undefined and run as it is: host code only
    jobs, stdout, fastas = eight
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", root, SANITIZED[len(root) + 1:]], check=True, capture_output=True)
    r, got = bc.run_batch(SANITIZED, jobs, str(tmp_path), PA_CNS_BACKEND="flat", PA_CNS_BATCH_PARTS=5)
    check(r, got, stdout, fastas)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-2000:]
