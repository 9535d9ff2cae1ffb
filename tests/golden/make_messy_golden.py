#!/usr/bin/env python3
"""Writes tests/golden/messy_inputs_t1/: one end-to-end golden whose inputs hold lower-case bases, N / R / Y / K / M, CRLF
sequence files and ALN rows that mismatch by case alone (tests/messy_cases.py: a synth.Spec and a deterministic rewrite of
the written files), recorded from the COMPILED REFERENCE (oracle/_ref/*, built by oracle/Makefile) like make_golden.py's cases:

  spec.json        the Spec, the pagraph flags, and the SHA-256 of every recorded output and of the graph dump, for the messy inputs
                   and for the SAME Spec without the rewrite
  inputs.sha256    hash of every input file
  inputs.tar.gz    the input files themselves (the Spec alone cannot regenerate them)
  out/             the reference pagraph's complete -o directory (contig.txt sorted)
  graph.txt.gz     the reference's complete graph (graph_dump), succ.txt.gz: its successor lists (graph_dump --succ 1)

Before anything is recorded the reference pagraph runs ONCE on these inputs under the address and undefined-behaviour sanitizers
(oracle/_ref/pagraph_san, a stand-alone host program; -t 1, no library preloaded): a non-zero exit, a sanitizer report or outputs
other than the plain build's end this script — a feature of the rewrite on which the reference's behaviour is undefined does
not belong in a fixture.  The reference also runs on the un-rewritten inputs, and both its outputs and its graph must DIFFER
from the messy run's: otherwise the messy bytes would not matter to anything downstream.

usage: python tests/golden/make_messy_golden.py      (re-creates the directory byte for byte)"""
import gzip
import hashlib
import io
import json
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import messy_cases  # noqa: E402
import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def sha_dir(d):
    return {f: sha(open(os.path.join(d, f), "rb").read()) for f in sorted(os.listdir(d))}


def run(argv):
    r = subprocess.run(argv, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{argv[0]} failed ({r.returncode}): {r.stderr[-3000:]}")
    return r


def reference_run(exe, ind, out):
    """the reference pagraph's -o directory (contig.txt sorted: it is a set, written in hash order)"""
    os.makedirs(out)
    r = run(synth.pagraph_argv(os.path.join(REF, exe), ind, out, threads=messy_cases.THREADS, epsilon=messy_cases.EPS, cov=messy_cases.COV))
    ct = os.path.join(out, "contig.txt")
    lines = sorted(open(ct).read().split())
    open(ct, "w").write("".join(x + "\n" for x in lines))
    return r


def graph_dump(ind, gd):
    os.makedirs(gd)
    run([os.path.join(REF, "graph_dump"), "-t", str(messy_cases.THREADS), "-k", ind + "/kmer.bin", "-c", ind + "/ctg.fasta", "-R", ind + "/ref.fasta",
         "-p", ind, "-a", ind + "/aln", "-o", gd, "--epsilon", str(messy_cases.EPS), "-v", str(messy_cases.COV), "--succ", "1"])
    return open(os.path.join(gd, "0.graph.txt"), "rb").read(), b"B 0\n" + open(os.path.join(gd, "0.succ.txt"), "rb").read()


def write_tar(path, ind):
    """the input files, byte for byte the same archive on every run (no times, no owners)"""
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for f in sorted(os.listdir(ind)):
            data = open(os.path.join(ind, f), "rb").read()
            ti = tarfile.TarInfo(f)
            ti.size, ti.mode, ti.mtime = len(data), 0o644, 0
            tf.addfile(ti, io.BytesIO(data))
    with open(path, "wb") as fh, gzip.GzipFile(filename="", fileobj=fh, mode="wb", compresslevel=9, mtime=0) as gz:
        gz.write(raw.getvalue())


def main():
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/pagraph", "_ref/graph_dump", "_ref/pagraph_san"], check=True, capture_output=True)
    case = os.path.join(HERE, messy_cases.NAME)
    with tempfile.TemporaryDirectory() as tmp:
        ind, clean = messy_cases.generate(os.path.join(tmp, "in")), messy_cases.generate(os.path.join(tmp, "clean"), messy=False)
        counts = messy_cases.census(ind)
        if min(v for k, v in counts.items() if k != "lower_case_ref_row_letters") <= 0 or counts["lower_case_ref_row_letters"] != 0:
            sys.exit(f"the rewrite did not leave what the case is named for: {counts}")

        # 1. the reference under the sanitizers, once
        san = reference_run("pagraph_san", ind, os.path.join(tmp, "san_out"))
        if "Sanitizer" in san.stderr or "runtime error" in san.stderr:
            sys.exit("the reference's sanitized run on the messy inputs is not clean:\n" + san.stderr[-4000:])

        # 2. the plain reference: messy and clean
        reference_run("pagraph", ind, os.path.join(tmp, "out"))
        reference_run("pagraph", clean, os.path.join(tmp, "clean_out"))
        out_messy, out_clean = sha_dir(os.path.join(tmp, "out")), sha_dir(os.path.join(tmp, "clean_out"))
        if sha_dir(os.path.join(tmp, "san_out")) != out_messy:
            sys.exit("the sanitized and the plain build of the reference write different outputs")
        graph, succ = graph_dump(ind, os.path.join(tmp, "gd"))
        graph_clean, _ = graph_dump(clean, os.path.join(tmp, "gd_clean"))
        if sha(graph) == sha(graph_clean) or all(out_clean.get(f) == h for f, h in out_messy.items() if f != "contig.txt"):
            sys.exit("the messy bytes do not matter: the reference's graph or outputs equal those of the un-rewritten inputs")

        shutil.rmtree(case, ignore_errors=True)
        os.makedirs(case)
        shutil.copytree(os.path.join(tmp, "out"), os.path.join(case, "out"))
        json.dump({"spec": messy_cases.SPEC, "threads": messy_cases.THREADS, "epsilon": messy_cases.EPS, "cov": messy_cases.COV,
                   "rewrite": "tests/messy_cases.py", "census": counts,
                   "sha256": {"messy": {"out": out_messy, "graph": sha(graph)}, "clean": {"out": out_clean, "graph": sha(graph_clean)}}},
                  open(os.path.join(case, "spec.json"), "w"), indent=1)
        json.dump(sha_dir(ind), open(os.path.join(case, "inputs.sha256"), "w"), indent=1)
        write_tar(os.path.join(case, "inputs.tar.gz"), ind)
        for f, data in (("graph.txt.gz", graph), ("succ.txt.gz", succ)):
            with gzip.GzipFile(os.path.join(case, f), "wb", compresslevel=9, mtime=0) as dst:
                dst.write(data)
    for f in sorted(os.listdir(case)):
        p = os.path.join(case, f)
        if os.path.isfile(p):
            assert os.path.getsize(p) < (1 << 20), f"{f} is over the size limit of a committed file"
    print(messy_cases.NAME, sorted(os.listdir(os.path.join(case, "out"))), counts)


if __name__ == "__main__":
    main()
