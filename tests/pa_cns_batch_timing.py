"""GPU box: the consensus step for the new contigs of one pipeline round — one `pa_cns` run per contig (AlignGraph2.py:500-510)
against one `pa_cns --batch` run over all of them.  The inputs come from the generator of tests/pa_cns_wave_timing.py
(cns_cases.write_case at the pipeline's settings: part 5 000, top 3 000, alpha 250, ~190x): 16 backbones between 125 kb and
1 Mb, about 8 Mb and 1 600 parts in all.  Whole-program wall clock, best of 2:

    (a) loop, default   the per-contig loop with default settings (--parent: the parent commit's binary; this one's otherwise)
    (b) loop, wave      the same loop under PA_CNS_BACKEND=wave
    (c) batch, flat     --batch under PA_CNS_BACKEND=flat
    (d) batch, wave     --batch under PA_CNS_BACKEND=wave, default groups
    (e) batch, wave, groups of 400 parts   (PA_CNS_BATCH_PARTS=400: the next group's ingest beside the device call)

with the per-group lines of the batch runs (PA_CNS_STAGE_TIMES=1) and a digest of all output files per row, which must agree.

    python tests/pa_cns_batch_timing.py OUT.json [--threads 16] [--parent PATH/pa_cns] [--scale 1.0]"""
import argparse
import concurrent.futures
import hashlib
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

KB = (125, 150, 200, 250, 300, 350, 400, 450, 500, 550, 600, 650, 700, 800, 900, 1000)
GROUP = re.compile(r"pa_cns: group (\d+): jobs (\d+) parts (\d+) ingest ([0-9.eE+-]+) s graph stage \((\w+)\) ([0-9.eE+-]+) s device waited ([0-9.eE+-]+) s "
                   r"ingest waited ([0-9.eE+-]+) s")
ENV_NAMES = ("PA_CNS_BACKEND", "PA_CNS_INGEST", "PA_CNS_STAGE_TIMES", "PA_CNS_BATCH_PARTS", "PA_CNS_BATCH_BYTES", "PA_CNS_DUMP_ROWS")


def case_of(i, length, coverage):
    return dict(seed=11 + i, backbone=length, n_reads=int(length * coverage / 1500), read_len=1500, part=5000, top_k=3000, alpha=250)


def generate(args):
    import cns_cases
    case, d = args
    cns_cases.write_case(case, d)
    return d


def flags(threads):
    return ["-t", str(threads), "-l", "5000", "-k", "3000", "--alpha", "250"]


def digest(paths):
    h = hashlib.sha256()
    for p in paths:
        h.update(open(p, "rb").read())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--coverage", type=float, default=190.0)
    ap.add_argument("--scale", type=float, default=1.0, help="every backbone length times this (a quick look at a small size)")
    ap.add_argument("--parent", default=None, help="bin/pa_cns built from the parent commit, for row (a)")
    ap.add_argument("--rows", default="abcde")
    args = ap.parse_args()
    ours = os.path.join(ROOT, "aligngraph2_amd", "bin", "pa_cns")
    root = tempfile.mkdtemp(prefix="pacns_batch_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        cases = [case_of(i, int(kb * 1000 * args.scale), args.coverage) for i, kb in enumerate(KB)]
        t0 = time.perf_counter()
        with concurrent.futures.ProcessPoolExecutor(max_workers=min(8, args.threads)) as pool:
            dirs = list(pool.map(generate, [(c, os.path.join(root, "job%02d" % i)) for i, c in enumerate(cases)]))
        rec = {"what": "the consensus step for 16 contigs: one pa_cns run per contig against one pa_cns --batch run; whole-program wall clock, best of 2",
               "cpus": len(os.sched_getaffinity(0)), "threads": args.threads, "backbones": [c["backbone"] for c in cases],
               "parts_nominal": sum((c["backbone"] + 4999) // 5000 for c in cases), "s_generate": time.perf_counter() - t0,
               "aln_bytes": sum(os.path.getsize(os.path.join(d, "reads.ref")) for d in dirs), "rows": []}
        base = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
        rows = [("a", "loop, default" + (" (parent binary)" if args.parent else ""), args.parent or ours, False, {}),
                ("b", "loop, wave", ours, False, dict(PA_CNS_BACKEND="wave")),
                ("c", "batch, flat", ours, True, dict(PA_CNS_BACKEND="flat")),
                ("d", "batch, wave", ours, True, dict(PA_CNS_BACKEND="wave")),
                ("e", "batch, wave, groups of 400 parts", ours, True, dict(PA_CNS_BACKEND="wave", PA_CNS_BATCH_PARTS="400"))]
        for key, label, exe, batch, env in rows:
            if key not in args.rows:
                continue
            outs = [os.path.join(root, "out_%s_%02d.fasta" % (key, i)) for i in range(len(dirs))]
            e = dict(base, PA_CNS_STAGE_TIMES="1", **env)
            best, groups = None, None
            for rep in range(2):
                t1 = time.perf_counter()
                if batch:
                    manifest = os.path.join(root, "manifest_%s.tsv" % key)
                    with open(manifest, "w") as f:
                        for d, o in zip(dirs, outs):
                            f.write("%s\t%s\t%s\n" % (os.path.join(d, "backbone.fasta"), os.path.join(d, "reads.ref"), o))
                    r = subprocess.run([exe, *flags(args.threads), "--batch", manifest], capture_output=True, text=True, env=e, timeout=3000)
                    assert r.returncode == 0, label + ": " + r.stderr[-1500:]
                    stderr = r.stderr
                else:
                    stderr = ""
                    for d, o in zip(dirs, outs):
                        r = subprocess.run([exe, *flags(args.threads), "-i", os.path.join(d, "backbone.fasta"), "-o", o, "-a", os.path.join(d, "reads.ref")],
                                           capture_output=True, text=True, env=e, timeout=3000)
                        assert r.returncode == 0, label + ": " + r.stderr[-1500:]
                dt = time.perf_counter() - t1
                if best is None or dt < best:
                    best = dt
                    groups = [dict(group=int(m.group(1)), jobs=int(m.group(2)), parts=int(m.group(3)), s_ingest=float(m.group(4)), backend=m.group(5),
                                   s_graph_stage=float(m.group(6)), s_device_waited=float(m.group(7)), s_ingest_waited=float(m.group(8)))
                              for m in GROUP.finditer(stderr)]
            row = {"row": key, "label": label, "s_wall_best_of_2": best, "sha256_of_outputs": digest(outs)}
            if batch:
                row["groups"] = groups
                rec["parts"] = sum(g["parts"] for g in groups)  # (the generated backbones differ from their nominal lengths by a few bases)
            rec["rows"].append(row)
            print(f"({key}) {label}: wall {best:.2f} s", flush=True)
            with open(args.out, "w") as f:  # (written after every row: a call that ends early keeps what it measured)
                json.dump(rec, f, indent=1)
        digests = {r["sha256_of_outputs"] for r in rec["rows"]}
        rec["identical_outputs"] = len(digests) == 1
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        assert rec["identical_outputs"], "the rows' outputs differ"
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
