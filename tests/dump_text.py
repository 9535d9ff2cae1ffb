"""The body of a per-contig path dump (<prefix><contig>_<0|1>.txt) restated in Python — the line format and PositionMapper
(csrc/host/position_mapper.hpp) — plus the ctypes side of pag_render_dump_lines.  tests/test_dump_render.py pins the
restatement to every line of the reference's golden dumps, so that it can stand as the oracle for records no golden has
(tests/test_gpu_dump_render.py)."""
import bisect
import ctypes as C
import os

import numpy as np

import goldens
import pagctl  # noqa: F401  (puts the repository root on sys.path)

from aligngraph2_amd import capi
from aligngraph2_amd.capi import PAG_EINVAL, PAG_ENODEV, PAG_ERANGE, PAG_OK  # noqa: F401  (the tests take them from here)

# pag_path_node (include/pagraph_hip.h)
NODE = capi.DTYPES["pag_path_node"]
assert NODE.itemsize == 24

M64 = (1 << 64) - 1


class Mapper:
    """PositionMapper: the constructor (:18-25) and singleToDual (:33-47) with its unsigned 64-bit arithmetic.  Past the last
    start the size reads as 0 (the reference reads past its table there; the library's own Mapper does the same)."""

    def __init__(self, sizes):
        self.sizes = [int(x) for x in sizes]
        self.starts = []
        if not self.sizes:
            return
        self.starts.append(self.sizes[0])
        for i in range(1, len(self.sizes)):
            self.starts.append(self.starts[-1] + 3 * self.sizes[i - 1] + max(self.sizes[i - 1], self.sizes[i]))
        self.starts.append(self.starts[-1] + 4 * self.sizes[-1])

    def extra_start(self):
        return self.starts[-1] if self.starts else 0

    def single_to_dual(self, single):
        if single == 0:
            return 0, 0
        i = bisect.bisect_right(self.starts, single)  # upper_bound
        if i != 0:
            i -= 1
        start = self.starts[i] if self.starts else 0
        size = self.sizes[i] if i < len(self.sizes) else 0
        off = (single - start) & M64  # unsigned subtraction first
        if off >= 2 * size:
            off = (off - 2 * size) & M64
            idx = -(i + 1)
        else:
            idx = i + 1
        if off >= 1 << 63:  # printed as the signed 64-bit value it is cast to
            off -= 1 << 64
        return idx, off


def kmer_string(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmer_code(s):
    c = 0
    for ch in s:
        c = (c << 2) | "ACGT".index(ch)
    return c


def render_line(rec, k, cm, rm):
    """rec: (code, ctg, ref, cnt, step)"""
    code, ctg, ref, cnt, step = (int(x) for x in rec)
    ci, co = cm.single_to_dual(ctg)
    ri, ro = rm.single_to_dual(ref)
    return f"{kmer_string(code, k)},{ctg},{ref},{cnt}\t{step}\t{ci},{co}\t{ri},{ro}\n"


def parse_line(line):
    """a body line -> (k, (code, ctg, ref, cnt, step)): the record the line was rendered from"""
    head, step, _, _ = line.rstrip("\n").split("\t")
    kmer, ctg, ref, cnt = head.split(",")
    return len(kmer), (kmer_code(kmer), int(ctg), int(ref), int(cnt), int(step))


def render(records, k, cm, rm):
    return "".join(render_line((r["code"], r["ctg"], r["ref"], r["cnt"], r["step"]), k, cm, rm) for r in records).encode()


def to_records(tuples):
    a = np.zeros(len(tuples), dtype=NODE)
    for i, (code, ctg, ref, cnt, step) in enumerate(tuples):
        a[i] = (code, ctg, ref, cnt, 0, step, i)
    return a


def fasta_lengths(path):
    """the lengths of a FASTA file's records as the reference's reader counts them (a CR of a sequence line is a base)"""
    return [len(seq) for _, seq in goldens.reference_fasta(path)]


def dump_cases():
    """the golden cases that have path dumps"""
    return [n for n in goldens.case_names() if any(f.endswith(".txt") and f != "contig.txt" for f in goldens.golden_out_files(n))]


def golden_dumps(name):
    """{file: (header line, [body lines])} of a golden's dump files"""
    out = {}
    for f, data in goldens.golden_out_files(name).items():
        if not f.endswith(".txt") or f == "contig.txt":
            continue
        lines = data.decode().splitlines(keepends=True)
        out[f] = (lines[0], lines[1:])
    return out


def case_lengths(name, work):
    ind = goldens.materialize_inputs(name, os.path.join(str(work), "dump_in_" + name))
    return fasta_lengths(os.path.join(ind, "ctg.fasta")), fasta_lengths(os.path.join(ind, "ref.fasta"))


GUARD = 64


def device_render(lib, records, k, ctg_len, ref_len, cap=None):
    """-> (rc, bytes needed, what the buffer holds up to `cap`, True if the guard bytes behind `cap` are untouched); cap None:
    asked for first (a call with cap 0), then rendered into exactly that many bytes"""
    records = np.ascontiguousarray(records, dtype=NODE)
    cl = np.ascontiguousarray(ctg_len, dtype=np.uint32)
    rl = np.ascontiguousarray(ref_len, dtype=np.uint32)
    need = C.c_uint64(0)
    if cap is None:
        rc = lib.pag_render_dump_lines(records.ctypes.data, len(records), k, cl.ctypes.data, len(cl), rl.ctypes.data, len(rl), None, 0, C.byref(need), 0)
        assert rc in (PAG_OK, PAG_ERANGE), rc
        assert (rc == PAG_OK) == (need.value == 0)
        cap = need.value
    buf = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    rc = lib.pag_render_dump_lines(records.ctypes.data, len(records), k, cl.ctypes.data, len(cl), rl.ctypes.data, len(rl), buf.ctypes.data, cap,
                                   C.byref(need), 0)
    return rc, need.value, buf[:cap].tobytes(), bool((buf[cap:] == 0xA5).all())
