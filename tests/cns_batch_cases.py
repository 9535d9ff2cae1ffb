"""What the two pa_cns --batch test files share (tests/test_pa_cns_batch.py on the CPU, tests/test_gpu_pa_cns_batch.py on the
device): the eight jobs, how a manifest is written and run, and the single runs a batch is held to.

The jobs: the five cns_cases.CASES and cns_cases.DEEP_CASE, all at the common flags -t 4 -l 700 -k 3000 --alpha 250 (3, 4, 3, 4, 3
and 18 parts), the `one_part` backbone with an EMPTY alignment file and with a MISSING one (3 parts each, the backbone comes
back): 41 parts.  The deep case stands in the middle of the manifest, so that the order by cost the engine runs the parts in
differs from manifest order and a wrong mapping back shows."""
import os
import subprocess

import cns_cases
import pagctl

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pa_cns")
REF = os.path.join(pagctl.REF_DIR, "pa_cns")
GOLD = os.path.join(pagctl.ROOT, "tests", "golden", "pa_cns")
FLAGS = dict(part=700, top_k=3000, alpha=250)
ORDER = ("one_part", "three_parts_ties", "topk_cut", "empty_aln", "deep", "low_cov_quirks", "boundary_ends", "missing_aln")
PARTS = dict(one_part=3, three_parts_ties=4, topk_cut=3, empty_aln=3, deep=18, low_cov_quirks=4, boundary_ends=3, missing_aln=3)
ENV_NAMES = ("PA_CNS_BACKEND", "PA_CNS_INGEST", "PA_CNS_DUMP_ROWS", "PA_CNS_STAGE_TIMES", "PA_CNS_ROWS_STAGE_COLS", "PA_CNS_ROWS_PIECE_BYTES",
             "PA_CNS_BATCH_PARTS", "PA_CNS_BATCH_BYTES")


def ensure_built():
    if not (os.path.exists(pagctl.HIP_LIB) and os.path.exists(EXE)):
        subprocess.run(["make", "-C", pagctl.ROOT, "product"], check=True, capture_output=True)


def clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    env.update({k: str(v) for k, v in extra.items()})
    return env


def write_jobs(root):
    """-> [(name, backbone path, alignment path)] in manifest order"""
    jobs = []
    for name in ORDER:
        d = os.path.join(root, name)
        if name in cns_cases.CASES or name == "deep":
            cns_cases.write_case(cns_cases.DEEP_CASE if name == "deep" else cns_cases.CASES[name], d)
        else:
            cns_cases.write_case(cns_cases.CASES["one_part"], d)
            os.remove(os.path.join(d, "reads.ref"))
            if name == "empty_aln":
                open(os.path.join(d, "reads.ref"), "w").close()
        jobs.append((name, os.path.join(d, "backbone.fasta"), os.path.join(d, "reads.ref")))
    return jobs


def flag_argv(flags, threads=4):
    return ["-t", str(threads), "-l", str(flags["part"]), "-k", str(flags["top_k"]), "--alpha", str(flags["alpha"])]


def run_single(exe, job, out, flags=FLAGS, **env):
    _, bb, aln = job
    return subprocess.run([exe, *flag_argv(flags), "-i", bb, "-o", out, "-a", aln], capture_output=True, text=True, timeout=600, env=clean_env(**env))


def singles(exe, jobs, d, **env):
    """every job alone -> (the stdouts one after the other, {name: FASTA bytes})"""
    os.makedirs(d, exist_ok=True)
    stdout, fastas = "", {}
    for job in jobs:
        out = os.path.join(d, job[0] + ".fasta")
        r = run_single(exe, job, out, **env)
        assert r.returncode == 0, (job[0], r.stderr[-500:])
        stdout += r.stdout
        fastas[job[0]] = open(out, "rb").read()
    return stdout, fastas


def write_manifest(path, jobs, out_dir):
    """-> {name: output path}"""
    os.makedirs(out_dir, exist_ok=True)
    outs = {name: os.path.join(out_dir, name + ".fasta") for name, _, _ in jobs}
    with open(path, "w") as f:
        for name, bb, aln in jobs:
            f.write(f"{bb}\t{aln}\t{outs[name]}\n")
    return outs


def run_batch(exe, jobs, d, flags=FLAGS, **env):
    """the jobs as one manifest -> (CompletedProcess, {name: FASTA bytes or None})"""
    os.makedirs(d, exist_ok=True)
    outs = write_manifest(os.path.join(d, "manifest.tsv"), jobs, os.path.join(d, "out"))
    r = subprocess.run([exe, *flag_argv(flags), "--batch", os.path.join(d, "manifest.tsv")], capture_output=True, text=True, timeout=600, env=clean_env(**env))
    return r, {name: (open(p, "rb").read() if os.path.exists(p) else None) for name, p in outs.items()}
