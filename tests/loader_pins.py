"""Helpers of the loader pins (tests/test_loader_pins.py, tests/test_gpu_loader_pins.py): the committed dumps of the reference's
readers (tests/golden/loaders/, see tests/golden/make_loader_golden.py) and the product's databases written in the same text
format by the harness hooks pagt_seqdb_dump / pagt_alndb_dump (tests/harness/pagh_test.cpp)."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import loader_cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "loaders")


def golden(name, mode):
    """the reference's dump of a file of loader_cases, as bytes"""
    base = os.path.join(GOLDEN, f"{name}.{mode}.txt")
    if os.path.exists(base + ".gz"):
        return gzip.open(base + ".gz", "rb").read()
    return open(base, "rb").read()


def golden_lines(name, mode):
    return [ln.split(b" ") for ln in golden(name, mode).splitlines()]


def assert_same_text(got: bytes, want: bytes, label: str):
    """equal, or an AssertionError that names the first differing line"""
    if got == want:
        return
    g, w = got.splitlines(), want.splitlines()
    for i in range(max(len(g), len(w))):
        a = g[i] if i < len(g) else b"<no line>"
        b = w[i] if i < len(w) else b"<no line>"
        if a != b:
            raise AssertionError(f"{label}: line {i + 1} differs ({len(g)} lines, the reference has {len(w)})\n  product  : {a[:300]!r}\n  reference: {b[:300]!r}")
    raise AssertionError(f"{label}: same lines, other line ends")


def _lib():
    import pagctl
    lib = pagctl.test_lib()
    lib.pagt_seqdb_dump.argtypes = [C.c_char_p, C.c_char_p]
    lib.pagt_seqdb_dump.restype = C.c_int
    lib.pagt_alndb_dump.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    lib.pagt_alndb_dump.restype = C.c_int
    return lib


FLAVORS = {"mecat": 0, "mummer": 1}


def dump_all(in_dir, out_dir, twice=False):
    """Every file of loader_cases through the product's loaders, as this process's environment makes them run: <out_dir>/
    <file>.seq.txt, <file>.mecat.txt, <file>.mummer.txt and <file>.mecat_filtered.txt (Mecat under the hook's AlnRecordFilter),
    and how.json: per dump, the hook's return values (alignment databases: 0 = parsed from the text, 1 = loaded from a packed
    sidecar).  twice: every alignment database is constructed a second time and the SECOND one is what is written."""
    lib = _lib()
    loader_cases.write_inputs(in_dir)
    os.makedirs(out_dir, exist_ok=True)
    how = {}
    for name in sorted(loader_cases.SEQ_CASES):
        rc = lib.pagt_seqdb_dump(os.path.join(in_dir, name).encode(), os.path.join(out_dir, name + ".seq.txt").encode())
        how[name + ".seq"] = [rc]
    for name in sorted(loader_cases.ALN_CASES):
        src = os.path.join(in_dir, name).encode()
        for mode, flavor in FLAVORS.items():
            out = os.path.join(out_dir, f"{name}.{mode}.txt").encode()
            how[f"{name}.{mode}"] = [lib.pagt_alndb_dump(src, flavor, 0, out) for _ in range(2 if twice else 1)]
        if not twice:
            how[name + ".mecat_filtered"] = [lib.pagt_alndb_dump(src, 0, 1, os.path.join(out_dir, name + ".mecat_filtered.txt").encode())]
    with open(os.path.join(out_dir, "how.json"), "w") as f:
        json.dump(how, f)
    return how


def dump_all_in_child(in_dir, out_dir, env, twice=False):
    """dump_all in a fresh process with `env` added to the environment (the loaders read their switches from it)"""
    code = "import sys; sys.path.insert(0, %r); import loader_pins; loader_pins.dump_all(%r, %r, twice=%r)" % (HERE, in_dir, out_dir, twice)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.load(open(os.path.join(out_dir, "how.json")))


def filtered_expectation(name):
    """the Mecat dump of a file as a database under pagt_alndb_dump's filter must print it: the records whose query name ends
    in a byte of odd value as they are, every other record with its header fields and no columns.  -> (text, kept, dropped)"""
    out, kept, dropped = [], 0, 0
    for f in golden_lines(name, "mecat"):
        qname = b"" if f[2] == b"-" else bytes.fromhex(f[2].decode())
        if qname and qname[-1] & 1:
            kept += 1
        else:
            dropped += 1
            f = f[:10] + [b"-", b"-"]
        out.append(b" ".join(f) + b"\n")
    return b"".join(out), kept, dropped
