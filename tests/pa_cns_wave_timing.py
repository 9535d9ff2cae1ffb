"""GPU box: bin/pa_cns's graph stage by backend — `wave` (a wavefront per part, its lanes on the columns of an alignment and the
levels of bestPath), `hip` (one lane per part), `flat` (the same serial code on host threads), `host` (the std::vector / std::map
restatement) — and the compiled reference `oracle/_ref/pa_cns -t 16`, at the pipeline's settings (part 5 000, top 3 000, alpha
250, ~190x) on backbones of 1 Mb (200 parts) and 5 Mb (1 000 parts).  Per run, best of 2: the whole-program wall clock and the
graph stage alone (PA_CNS_STAGE_TIMES=1: a host clock around the backend call, which ends in a device synchronise; parsing and
slicing are the same for every backend), `flat`'s three phases in thread-seconds, and the output compared byte for byte with
the reference's.

    python tests/pa_cns_wave_timing.py OUT.json [--backbones 1000000 5000000] [--threads 16]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGE = re.compile(r"pa_cns: graph stage \(([^)]*)\) ([0-9.eE+-]+) s")
PHASES = re.compile(r"pa_cns: flat phases \(thread-seconds\) add_aln ([0-9.eE+-]+) merge_nodes ([0-9.eE+-]+) best_path\+trim ([0-9.eE+-]+)")


def one_backbone(length, coverage, threads):
    import cns_cases
    case = dict(seed=11, backbone=length, n_reads=int(length * coverage / 1500), read_len=1500, part=5000, top_k=3000, alpha=250)
    d = tempfile.mkdtemp(prefix="pacns_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    t0 = time.perf_counter()
    cns_cases.write_case(case, d)
    rec = {"case": case, "parts": (length + 4999) // 5000, "threads": threads, "s_generate": time.perf_counter() - t0,
           "aln_bytes": os.path.getsize(os.path.join(d, "reads.ref")), "runs": []}
    ref_exe = os.path.join(ROOT, "oracle", "_ref", "pa_cns")
    ours = os.path.join(ROOT, "aligngraph2_amd", "bin", "pa_cns")
    outs = {}
    for label, exe, backend in [("reference -t %d" % threads, ref_exe, None), ("wave", ours, "wave"), ("hip", ours, "hip"), ("flat", ours, "flat"),
                                ("host", ours, "host")]:
        if not os.path.exists(exe):
            rec["runs"].append({"label": label, "skipped": os.path.relpath(exe, ROOT) + " missing"})
            continue
        out = os.path.join(d, "out_" + label.split()[0] + ".fasta")
        e = dict(os.environ)
        e.pop("PA_CNS_BACKEND", None)
        if backend:
            e.update(PA_CNS_BACKEND=backend, PA_CNS_STAGE_TIMES="1")
        best, stage, phases = None, None, None
        for rep in range(2):
            t1 = time.perf_counter()
            r = subprocess.run(cns_cases.argv(exe, d, out, case, threads=threads), capture_output=True, text=True, env=e, timeout=3000)
            dt = time.perf_counter() - t1
            assert r.returncode == 0, label + ": " + r.stderr[-1500:]
            best = dt if best is None else min(best, dt)
            m = STAGE.search(r.stderr)
            if m:
                s = float(m.group(2))
                stage = s if stage is None else min(stage, s)
            m = PHASES.search(r.stderr)
            if m and (phases is None or sum(map(float, m.groups())) < sum(phases.values())):
                phases = dict(zip(("add_aln", "merge_nodes", "best_path_trim"), map(float, m.groups())))
        outs[label] = open(out, "rb").read()
        run = {"label": label, "s_wall_best_of_2": best, "stdout_tail": r.stdout[-200:]}
        if stage is not None:
            run["s_graph_stage_best_of_2"] = stage
        if phases is not None:
            run["flat_phase_thread_seconds"] = phases
        rec["runs"].append(run)
        print(f"{length} bp {label}: wall {best:.2f} s" + (f", graph stage {stage:.3f} s" if stage is not None else ""), flush=True)
    ref = next((v for k, v in outs.items() if k.startswith("reference")), None)
    for run in rec["runs"]:
        if run["label"] in outs:
            run["identical_to_reference"] = (outs[run["label"]] == ref) if ref is not None else None
    if ref is None:  # (without the reference binary: every backend against `host`)
        rec["identical_to_host"] = {k: v == outs.get("host") for k, v in outs.items()}
    shutil.rmtree(d, ignore_errors=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--backbones", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--coverage", type=float, default=190.0)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    rec = {"what": "bin/pa_cns graph stage by backend (wave / hip / flat / host) and the compiled reference at the pipeline's settings; "
                   "whole-program wall clock and graph-stage seconds, best of 2",
           "cpus": len(os.sched_getaffinity(0)), "backbones": []}
    for length in args.backbones:
        rec["backbones"].append(one_backbone(length, args.coverage, args.threads))
        with open(args.out, "w") as f:  # (written after every backbone: a call that ends early keeps what it measured)
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
