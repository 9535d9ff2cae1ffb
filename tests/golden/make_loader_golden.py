#!/usr/bin/env python3
"""Writes tests/golden/loaders/<file>.<mode>.txt[.gz]: what the REFERENCE's own readers make of every file of
tests/loader_cases.py (oracle/_ref/loader_dump, built by `make -C oracle ref` from oracle/ref_harness/loader_dump.cpp; the
reference's sources are compiled where they lie, nothing of them is stored here).  Data only.

Every (file, mode) is first run through the sanitized build of the same program (oracle/_ref/loader_dump_san: address and
undefined-behaviour sanitizers, libstdc++ assertions).  A run that exits non-zero or prints anything to stderr ends this
script: a file on which the reference's behaviour is undefined is not a fixture (tests/loader_cases.py names the ones that
were left out for it).  The sanitized and the plain build must print the same bytes.  Nothing here starts a thread, so no
library is preloaded into either program.

Dumps above 200 kB are stored gzipped (compresslevel 9, mtime 0), as make_golden.py stores its large files.

usage: python tests/golden/make_loader_golden.py [--check]      (--check: compare with the committed files, write nothing)"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loader_cases  # noqa: E402

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "loaders")
GZ_ABOVE = 200_000


def dump(exe, mode, path):
    return subprocess.run([os.path.join(REF_DIR, exe), mode, path], capture_output=True, timeout=300)


def main():
    check = "--check" in sys.argv[1:]
    for exe in ("loader_dump", "loader_dump_san"):
        if not os.path.exists(os.path.join(REF_DIR, exe)):
            sys.exit(f"oracle/_ref/{exe} is missing: run `make -C oracle ref` first")
    os.makedirs(OUT, exist_ok=True)
    written, drift = [], []
    with tempfile.TemporaryDirectory() as d:
        loader_cases.write_inputs(d)
        for name, mode in loader_cases.all_dumps():
            path = os.path.join(d, name)
            san = dump("loader_dump_san", mode, path)
            if san.returncode != 0 or san.stderr:
                sys.exit(f"{name} ({mode}): the reference's sanitized run is not clean (exit {san.returncode}); not a fixture\n"
                         + san.stderr.decode(errors="replace")[-4000:])
            plain = dump("loader_dump", mode, path)
            if plain.returncode != 0 or plain.stderr or plain.stdout != san.stdout:
                sys.exit(f"{name} ({mode}): the plain build exits {plain.returncode} or prints other bytes than the sanitized one")
            base = os.path.join(OUT, f"{name}.{mode}.txt")
            target = base + ".gz" if len(plain.stdout) > GZ_ABOVE else base
            other = base if target.endswith(".gz") else base + ".gz"
            if check:
                have = None
                if os.path.exists(target):
                    have = gzip.open(target, "rb").read() if target.endswith(".gz") else open(target, "rb").read()
                if have != plain.stdout or os.path.exists(other):
                    drift.append(os.path.basename(target))
                continue
            if os.path.exists(other):
                os.remove(other)
            if target.endswith(".gz"):
                with gzip.GzipFile(target, "wb", compresslevel=9, mtime=0) as f:
                    f.write(plain.stdout)
            else:
                with open(target, "wb") as f:
                    f.write(plain.stdout)
            written.append(os.path.basename(target))
    if check:
        if drift:
            sys.exit("differs from the committed dump: " + ", ".join(drift))
        print(f"{len(loader_cases.all_dumps())} dumps equal the committed ones; every sanitized run was clean")
    else:
        print(f"wrote {len(written)} dumps to {os.path.relpath(OUT, ROOT)}; every sanitized run was clean")


if __name__ == "__main__":
    main()
