"""GPU box: where bin/pa_cns's time goes by ingest mode (PA_CNS_INGEST) — `host` (one thread, std::string), `flat` (the file
mapped and indexed, headers on a thread pool, only the kept slices normalised, csrc/hip/cns_rows.hpp on host threads) and
`device` (the kept slices normalised by csrc/hip/k_cns_rows.hip, the rows left on the device) under PA_CNS_BACKEND=wave, and
`flat` under the `flat` backend — on the two inputs of tests/pa_cns_wave_timing.py (1 Mb / 201 parts and 5 Mb / 1 005 parts at
~190x, seed 11, -t 16).  Per run, best of 2: the whole-program wall clock, the ingest line and the graph-stage line of
PA_CNS_STAGE_TIMES=1, and the FASTA compared byte for byte with the first run's.  With --parent the binary of the parent commit
runs on the same files in the same session, and so does this tree with the variable unset: the default path may not be slower
than the parent by more than the parent's own two runs differ.

Every run is a process of its own under its own time limit; a run that ends on a signal, a time limit or an abort ends the
script (nothing more is started on the device after a fault).

    python tests/pa_cns_ingest_timing.py OUT.json [--backbones 1000000 5000000] [--threads 16] [--parent PATH/pa_cns]"""
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
INGEST = re.compile(r"pa_cns: ingest \((\w+)\) index ([0-9.eE+-]+) headers ([0-9.eE+-]+) lists ([0-9.eE+-]+) rows ([0-9.eE+-]+) upload ([0-9.eE+-]+)")
COUNTS = re.compile(r"pa_cns: rows on the device: (\d+) slices, (\d+) pieces, (\d+) oversize")
ENV_NAMES = ("PA_CNS_BACKEND", "PA_CNS_INGEST", "PA_CNS_DUMP_ROWS", "PA_CNS_STAGE_TIMES", "PA_CNS_ROWS_STAGE_COLS", "PA_CNS_ROWS_PIECE_BYTES")


class Stop(Exception):
    pass


def one_backbone(length, coverage, threads, parent, limit):
    import cns_cases
    case = dict(seed=11, backbone=length, n_reads=int(length * coverage / 1500), read_len=1500, part=5000, top_k=3000, alpha=250)
    d = tempfile.mkdtemp(prefix="pacns_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        t0 = time.perf_counter()
        cns_cases.write_case(case, d)
        rec = {"case": case, "parts": (length + 4999) // 5000, "threads": threads, "s_generate": time.perf_counter() - t0,
               "aln_bytes": os.path.getsize(os.path.join(d, "reads.ref")), "runs": []}
        ours = os.path.join(ROOT, "aligngraph2_amd", "bin", "pa_cns")
        plan = []
        if parent:
            plan.append(("parent, variable unset, wave", parent, None, "wave"))
        plan += [("variable unset, wave", ours, None, "wave"), ("host ingest, wave", ours, "host", "wave"), ("flat ingest, wave", ours, "flat", "wave"),
                 ("device ingest, wave", ours, "device", "wave"), ("flat ingest, flat", ours, "flat", "flat")]
        first = None
        for label, exe, ingest, backend in plan:
            out = os.path.join(d, "out.fasta")
            e = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
            e.update(PA_CNS_BACKEND=backend, PA_CNS_STAGE_TIMES="1")
            if ingest:
                e["PA_CNS_INGEST"] = ingest
            walls, stage, split, counts = [], None, None, None
            for rep in range(2):
                if os.path.exists(out):
                    os.remove(out)
                t1 = time.perf_counter()
                try:
                    r = subprocess.run(cns_cases.argv(exe, d, out, case, threads=threads), capture_output=True, text=True, env=e, timeout=limit)
                except subprocess.TimeoutExpired:
                    raise Stop(f"{label}: no end after {limit} s")
                walls.append(time.perf_counter() - t1)
                if r.returncode != 0:
                    raise Stop(f"{label}: exit {r.returncode}: {r.stderr[-1500:]}")
                m = STAGE.search(r.stderr)
                if m:
                    stage = float(m.group(2)) if stage is None else min(stage, float(m.group(2)))
                m = INGEST.search(r.stderr)
                if m and (split is None or sum(map(float, m.groups()[1:])) < sum(v for k, v in split.items() if k != "mode")):
                    split = dict(zip(("index", "headers", "lists", "rows", "upload"), map(float, m.groups()[1:])), mode=m.group(1))
                m = COUNTS.search(r.stderr)
                if m:
                    counts = dict(zip(("slices", "pieces", "oversize"), map(int, m.groups())))
            fasta = open(out, "rb").read()
            first = fasta if first is None else first
            run = {"label": label, "s_wall_best_of_2": min(walls), "s_wall_both": walls, "identical_to_first_run": fasta == first, "stdout_tail": r.stdout[-200:]}
            if stage is not None:
                run["s_graph_stage_best_of_2"] = stage
            if split is not None:
                run["s_ingest_best_of_2"] = split
            if counts is not None:
                run["device_rows"] = counts
            rec["runs"].append(run)
            print(f"{length} bp {label}: wall {min(walls):.2f} s (both {walls[0]:.2f} {walls[1]:.2f})" + (f", graph stage {stage:.3f} s" if stage is not None else "") +
                  (f", ingest {split}" if split else ""), flush=True)
        by = {r["label"]: r for r in rec["runs"]}
        if parent:
            p, u = by["parent, variable unset, wave"], by["variable unset, wave"]
            rec["default_path"] = {"s_parent_both": p["s_wall_both"], "s_this_tree_both": u["s_wall_both"],
                                   "parent_spread": abs(p["s_wall_both"][0] - p["s_wall_both"][1]),
                                   "this_minus_parent_best": u["s_wall_best_of_2"] - p["s_wall_best_of_2"]}
            rec["default_path"]["within_parent_spread"] = rec["default_path"]["this_minus_parent_best"] <= rec["default_path"]["parent_spread"]
        return rec
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--backbones", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--coverage", type=float, default=190.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent", default=None, help="bin/pa_cns built from the parent commit")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a single run may take")
    args = ap.parse_args()
    rec = {"what": "bin/pa_cns by ingest mode (PA_CNS_INGEST host / flat / device under the wave backend, flat under flat): whole-program wall clock, "
                   "the ingest by step and the graph stage, best of 2; the parent commit's binary on the same files",
           "cpus": len(os.sched_getaffinity(0)), "backbones": []}
    for length in args.backbones:
        try:
            rec["backbones"].append(one_backbone(length, args.coverage, args.threads, args.parent, args.limit))
        except Stop as e:
            rec["stopped"] = str(e)
            print("stopped:", e, flush=True)
        with open(args.out, "w") as f:  # (written after every backbone: a call that ends early keeps what it measured)
            json.dump(rec, f, indent=1)
        if "stopped" in rec:
            sys.exit(1)


if __name__ == "__main__":
    main()
