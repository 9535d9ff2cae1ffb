#!/usr/bin/env python3
"""Generates the graph-only golden fixtures under tests/golden/graph_only/ by running the COMPILED REFERENCE's graph_dump
(oracle/_ref/graph_dump, built from the reference by oracle/Makefile) — where the reference is present only.

These cases pin the graph BUILD alone on inputs too heavy for the walk tests, so they live one directory down: goldens.case_names()
lists the directories directly under tests/golden/ and does not see them.  The dump itself (megabytes) is not committed; per case
<name>/:
  spec.json        generator parameters (tests/synth.py) + the graph flags; "rewrite" / "unlisted_ctg": the rewrites of
                   tests/prep_cases.py applied to the generated read databases (heavy_cases.materialize applies them again)
  inputs.sha256    hash of every generated input file, after the rewrites (detects generator drift)
  graph.json       recorded results of the reference's dump: byte length, SHA-256, the six count lines ("S" line), the number of nodes,
                   and every node whose u16 counts sum to less than its raw tuple count: k-mer code, sum of the counts (both from the
                   dump), raw tuples and the deficit.  The raw tuple count is not in the dump: it is the length of the k-mer's segment
                   in the C oracle's tuple stream (tests/pagctl.py) — the generator refuses to write a golden unless the oracle's
                   counts equal the reference's for every node, so the deficit is the reference's own.
                   counts_cov0 (cases with a rewrite): the "S" line of the reference's dump of the same input at -v 0.

usage: python tests/golden/make_graph_only_golden.py        (re-creates everything deterministically)
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import pagctl  # noqa: E402
from heavy_cases import count_deficits  # noqa: E402
import prep_cases  # noqa: E402
import synth  # noqa: E402
from make_golden import REF, run, sha_dir  # noqa: E402

OUT = os.path.join(HERE, "graph_only")

def _prep(name):
    c = prep_cases.CASES[name]
    return (c.spec, c.threads, c.eps, c.cov, list(c.rewrites), c.unlisted_ctg)


# name -> (Spec kwargs, threads, epsilon, cov[, rewrites of tests/prep_cases.py, contig taken off config.txt])
CASES = {
    # a 2 600-base poly-A tract under 2 500-base reads: one k-mer with 151 049 raw tuples in 6 leaders, one of them past 65 535 members —
    # the reference's CountType (u16) wraps once
    "count_wrap_t8": (dict(seed=131, ref_len=9000, n_reads=700, read_len=2500, k=9, solid_min_abundance=2,
                           contigs=[(200, 4200, False), (4500, 8800, False)], homopolymer=(1000, 2600)), 8, 3000, 2),
    # prep_cases' `reject`: coverage-only records, records on the decoy references, lists of up to 60 alignments with ties, and a -v
    # at which the sorted-coverage filter (quirk Q3) rejects a third of pass 2
    "cov_reject_t4": _prep("reject"),
}


def parse_dump(data):
    """-> (the six counts, [(code, n_positions, sum of counts)] per node)"""
    counts, nodes = None, []
    for line in data.split(b"\n"):
        if line.startswith(b"P "):
            nodes[-1][2] += int(line.rsplit(b" ", 1)[1])
        elif line.startswith(b"K "):
            _, code, n_pos, _ = line.split()
            nodes.append([int(code), int(n_pos), 0])
        elif line.startswith(b"S "):
            counts = [int(x) for x in line.split()[1:]]
    return counts, nodes


def wrapped_nodes(ind, threads, eps, cov, ref_nodes):
    inp = pagctl.LoadedInput(ind, threads=threads, eps=eps, cov=cov)
    try:
        res = pagctl.run_oracle(inp, streams=True)
    finally:
        inp.close()
    csr = res["csr"]
    sums = np.add.reduceat(csr["pos_cnt"].astype(np.uint64), csr["pos_off"][:-1].astype(np.int64))
    mine = [[int(c), int(n), int(s)] for c, n, s in zip(csr["node_code"], np.diff(csr["pos_off"].astype(np.int64)), sums)]
    if mine != ref_nodes:
        raise RuntimeError("the oracle's counts differ from the reference's: no golden written")
    return [{"code": c, "count_sum": s, "raw_tuples": r, "deficit": r - s} for c, r, s in count_deficits(res)]


def main():
    only = set(sys.argv[1:])
    for name, (kw, threads, eps, cov, *rw) in CASES.items():
        if only and name not in only:
            continue
        rewrites, unlisted = rw if rw else ([], "")
        case = os.path.join(OUT, name)
        shutil.rmtree(case, ignore_errors=True)
        os.makedirs(case)
        with tempfile.TemporaryDirectory() as tmp:
            ind = os.path.join(tmp, "in")
            synth.generate(synth.Spec(**kw), ind)
            spec = {"spec": kw, "threads": threads, "epsilon": eps, "cov": cov}
            if rewrites:
                prep_cases.apply_rewrites(ind, rewrites, unlisted)
                spec.update(rewrite=rewrites, unlisted_ctg=unlisted)
            json.dump(spec, open(os.path.join(case, "spec.json"), "w"), indent=1)
            json.dump(sha_dir(ind), open(os.path.join(case, "inputs.sha256"), "w"), indent=1)

            def reference_dump(v):
                gd = os.path.join(tmp, f"gd{v}")
                os.makedirs(gd)
                run([os.path.join(REF, "graph_dump"), "-t", str(threads), "-k", ind + "/kmer.bin", "-c", ind + "/ctg.fasta",
                     "-R", ind + "/ref.fasta", "-p", ind, "-a", ind + "/aln", "-o", gd, "--epsilon", str(eps), "-v", str(v)], threads)
                dumps = sorted((f for f in os.listdir(gd) if f.endswith(".graph.txt")), key=lambda f: int(f.split(".")[0]))
                return b"".join(open(os.path.join(gd, f), "rb").read() for f in dumps)
            data = reference_dump(cov)
            counts, nodes = parse_dump(data)
            wrapped = wrapped_nodes(ind, threads, eps, cov, nodes)
            golden = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest(), "counts": counts, "n_nodes": len(nodes),
                      "wrapped_nodes": wrapped}
            if rewrites:
                golden["counts_cov0"] = parse_dump(reference_dump(0))[0]
            json.dump(golden, open(os.path.join(case, "graph.json"), "w"), indent=1)
        print(name, len(data), counts)


if __name__ == "__main__":
    main()
