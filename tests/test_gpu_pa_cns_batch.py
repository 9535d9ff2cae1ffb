"""GPU: bin/pa_cns --batch with the graph stage on the device (PA_CNS_BACKEND=wave / hip): the eight jobs of
tests/cns_batch_cases.py as one manifest — one backend call per group over the concatenated backbones and one pool pair, the
parts in cost order — against the single runs of the same binary on a CPU backend: every output file and the whole stdout.
With several groups the next group's ingest runs beside the device call.  `auto` chooses by the batch's part count.
The CPU side (flat backend, refusals, sanitizers): tests/test_pa_cns_batch.py."""
import os
import re

import pytest

import cns_batch_cases as bc
from cns_batch_cases import EXE

pytestmark = pytest.mark.gpu

GROUP = re.compile(r"pa_cns: group (\d+): jobs (\d+) parts (\d+) ingest \S+ s graph stage \((\w+)\) \S+ s device waited \S+ s ingest waited \S+ s")


@pytest.fixture(scope="module")
def eight(tmp_path_factory):
    bc.ensure_built()
    root = str(tmp_path_factory.mktemp("batch_gpu"))
    jobs = bc.write_jobs(os.path.join(root, "in"))
    stdout, fastas = bc.singles(EXE, jobs, os.path.join(root, "single"), PA_CNS_BACKEND="host")
    return jobs, stdout, fastas


def check(r, got, stdout, fastas):
    assert r.returncode == 0, r.stderr[-800:]
    assert r.stdout == stdout
    for name, fasta in fastas.items():
        assert got[name] == fasta, name


@pytest.mark.parametrize("env, groups", [(dict(), [(8, 41)]), (dict(PA_CNS_BATCH_PARTS=5), [(2, 7), (2, 6), (1, 18), (2, 7), (1, 3)])], ids=["one_group", "parts_5"])
@pytest.mark.parametrize("backend", ["wave", "hip"])
def test_device_batch_equals_the_cpu_single_runs(eight, backend, env, groups, tmp_path):
    jobs, stdout, fastas = eight
    r, got = bc.run_batch(EXE, jobs, str(tmp_path), PA_CNS_BACKEND=backend, PA_CNS_STAGE_TIMES=1, **env)
    check(r, got, stdout, fastas)
    seen = [(int(m.group(2)), int(m.group(3)), m.group(4)) for m in GROUP.finditer(r.stderr)]
    assert seen == [(j, p, backend) for j, p in groups], r.stderr[-1500:]


def test_device_batch_of_one_job(eight, tmp_path):
    jobs, stdout, fastas = eight
    deep = [j for j in jobs if j[0] == "deep"]
    r, got = bc.run_batch(EXE, deep, str(tmp_path), PA_CNS_BACKEND="wave")
    assert r.returncode == 0, r.stderr[-800:]
    assert got["deep"] == fastas["deep"] and r.stdout.splitlines()[0] == "PartNum=18" and r.stdout in stdout


def test_auto_chooses_flat_for_41_parts_and_says_so(eight, tmp_path):
    jobs, stdout, fastas = eight
    r, got = bc.run_batch(EXE, jobs, str(tmp_path), PA_CNS_STAGE_TIMES=1)
    check(r, got, stdout, fastas)
    assert "pa_cns: batch of 8 jobs, 41 parts: backend flat (auto), ingest flat" in r.stderr, r.stderr[-800:]
    assert [m.group(4) for m in GROUP.finditer(r.stderr)] == ["flat"]
