"""The consensus sequence of a path (PAlgorithm::seqToString, csrc/host/traversal.cpp) restated in Python from pag_path_node
records — on tests/dump_text.py's Mapper, parse_line and golden_dumps — plus the ctypes side of pag_render_path_sequence.
tests/test_seq_render.py pins the restatement to every golden .fasta: the pieces a chain's .con names, rendered from the
records of their golden dump files, concatenated, are the FASTA body.  It then stands as the oracle for records no golden has
(tests/test_gpu_seq_render.py)."""
import ctypes as C
import math
import os

import numpy as np

import dump_text
import goldens

from aligngraph2_amd import capi
from aligngraph2_amd.capi import PAG_EDOM, PAG_EINVAL, PAG_ENODEV, PAG_ERANGE, PAG_OK  # noqa: F401  (the tests take them from here)

NODE = dump_text.NODE
M32 = (1 << 32) - 1
ERROR_RATE = 0.15  # (pagraph_driver.cpp, traverse_api.cpp: not a command-line parameter)
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def is_pos_similar(l, r, deviation):
    """host_graph.hpp:27-33"""
    return tuple(l[t] != 0 and r[t] != 0 and abs(l[t] - r[t]) <= deviation for t in (0, 1))


def is_edge_similar(l, r, dist, deviation, error_rate):
    """host_graph.hpp:35-47: the u32 wrap of l + dist and of r - l, the f64 ratio tests"""
    tmp = tuple((l[t] + dist) & M32 if l[t] != 0 else 0 for t in (0, 1))
    s = is_pos_similar(tmp, r, deviation)
    return tuple(s[t] or (l[t] != 0 and r[t] != 0 and abs(1.0 - (((r[t] - l[t]) & M32) * 1.0 / dist)) <= error_rate) for t in (0, 1))


def round_half_away(x):
    """std::round of a finite double, as an int"""
    a = abs(x)
    f = math.floor(a)
    r = f + 1 if a - f >= 0.5 else f  # (a - f is exact)
    return -r if x < 0 else r


def base_at(seqs, idx, pos, forward):
    """SeqDb::baseAt behind seqToString's index test, lower case: 'n' outside the table or past the sequence's end"""
    if idx < 0 or idx >= len(seqs) or pos >= len(seqs[idx]):
        return "n"
    s = seqs[idx]
    return (s[pos] if forward else COMPLEMENT[s[len(s) - 1 - pos]]).lower()


class Counts:
    """what the rendered paths went through: vertices whose step the k-mer covers, longer steps, where their bases came from, and
    the positions rounded exactly at .5"""

    def __init__(self):
        self.short = self.long = self.long_bases = self.ctg = self.ref = self.reverse = self.half = self.pos_similar = 0


def render(records, k, ctg_seqs, ref_seqs, cm, rm, deviation, error_rate=ERROR_RATE, counts=None):
    """records: (code, ctg, ref, cnt, step) tuples or a NODE array -> the sequence as bytes; None: not renderable (a rounded
    position is negative or not finite — the host's cast to size_t is undefined there)"""
    if isinstance(records, np.ndarray):
        records = [(int(r["code"]), int(r["ctg"]), int(r["ref"]), int(r["cnt"]), int(r["step"])) for r in records]
    if not records:
        return b""
    out = [dump_text.kmer_string(records[0][0], k)]
    for i in range(1, len(records)):
        code, ctg, ref, _, step = records[i]
        kmer = dump_text.kmer_string(code, k)
        if step <= k:
            if step > 0:
                out.append(kmer[k - step:])
            if counts:
                counts.short += 1
            continue
        prev, now = (records[i - 1][1], records[i - 1][2]), (ctg, ref)
        sim = is_edge_similar(prev, now, step, deviation, error_rate)
        use_ctg = sim[0]
        if not sim[0] and not sim[1]:
            use_ctg = is_pos_similar(prev, now, deviation)[0]
        seqs, mapper = (ctg_seqs, cm) if use_ctg else (ref_seqs, rm)
        s_idx, s_off = mapper.single_to_dual(prev[0] if use_ctg else prev[1])
        e_idx, e_off = mapper.single_to_dual(now[0] if use_ctg else now[1])
        pos_dist = e_off - s_off
        sel, forward = abs(e_idx) - 1, e_idx > 0
        move = pos_dist * 1.0 / step
        ref_now = float(s_off + k)
        piece, half = [], 0
        for _ in range(step - k):
            if not math.isfinite(ref_now):
                return None
            pos = round_half_away(ref_now)
            if pos < 0 or pos >= 1 << 64:
                return None
            half += abs(ref_now - math.floor(ref_now)) == 0.5
            piece.append(base_at(seqs, sel, pos, forward))
            ref_now += move
        out.append("".join(piece))
        out.append(kmer)
        if counts:
            counts.long += 1
            counts.long_bases += step - k
            counts.ctg += use_ctg
            counts.ref += not use_ctg
            counts.reverse += not forward and sel >= 0
            counts.half += half
            counts.pos_similar += not sim[0] and not sim[1]
    return "".join(out).encode()


def expected_bytes(records, k):
    """the size of the text, known without rendering: k + the sum of the positive steps behind the first vertex"""
    steps = [int(r[4]) for r in records] if not isinstance(records, np.ndarray) else [int(x) for x in records["step"]]
    return k + sum(max(s, 0) for s in steps[1:]) if steps else 0


def read_fasta(path):
    """the sequences of a FASTA file as the reference stores them (goldens.reference_fasta)"""
    return [seq for _, seq in goldens.reference_fasta(path)]


def case_sequences(name, work):
    ind = goldens.materialize_inputs(name, os.path.join(str(work), "seq_in_" + name))
    return read_fasta(os.path.join(ind, "ctg.fasta")), read_fasta(os.path.join(ind, "ref.fasta"))


def fasta_cases():
    """the golden cases that have a chain's .fasta"""
    return [n for n in goldens.case_names() if any(f.endswith(".fasta") for f in goldens.golden_out_files(n))]


def golden_pieces(name):
    """{fasta file: (FASTA body as one line, [(dump file, k, records)] of the pieces its .con names, in chain order)}"""
    files = goldens.golden_out_files(name)
    dumps = dump_text.golden_dumps(name)
    out = {}
    for f, data in files.items():
        if not f.endswith(".fasta"):
            continue
        block = f.split("_", 1)[0]
        lines = data.decode().splitlines()
        assert lines[0].startswith(">")
        con = files[f[:-len(".fasta")] + ".con"].decode().splitlines()
        pieces = []
        for ln in con[1:]:
            ctg, orient, _ = ln.split("\t")
            suffix = {"FORWARD": "_0.txt", "REV": "_1.txt"}[orient]
            hits = [d for d, (header, _) in dumps.items() if d.startswith(block + "_") and d.endswith(suffix) and header.split("\t")[0] == ctg]
            assert len(hits) == 1, (name, f, ln, hits)
            parsed = [dump_text.parse_line(x) for x in dumps[hits[0]][1]]
            assert parsed and all(p[0] == parsed[0][0] for p in parsed)
            pieces.append((hits[0], parsed[0][0], [p[1] for p in parsed]))
        assert int(con[0].split("\t")[1]) == sum(len(x) for x in lines[1:])
        out[f] = ("".join(lines[1:]), pieces)
    return out


def golden_paths(name):
    """[(dump file, k, records)] of every non-empty golden dump of a case"""
    out = []
    for f, (_, body) in dump_text.golden_dumps(name).items():
        if body:
            parsed = [dump_text.parse_line(x) for x in body]
            out.append((f, parsed[0][0], [p[1] for p in parsed]))
    return out


def deviation_of(name):
    return 2 * int(goldens.load_spec(name)["epsilon"])  # (assemble() is called with epsilon * 2)


# ---- the ctypes side ---------------------------------------------------------------------------------------------------------

class Packed:
    """sequences as a pag_seqs: 2 bits per base, base i of a sequence in bits 2 * (i & 3) of its byte i >> 2"""

    def __init__(self, seqs):
        self.len = np.array([len(s) for s in seqs], dtype=np.uint32)
        nbytes = [4 * ((len(s) + 15) // 16) for s in seqs]  # (every sequence starts on a 4-byte boundary)
        self.byte_off = np.array([0] + list(np.cumsum(nbytes, dtype=np.uint64))[:-1] if seqs else [], dtype=np.uint64)
        self.packed = np.zeros(int(sum(nbytes)) + 16, dtype=np.uint8)
        for s, off in zip(seqs, self.byte_off):
            codes = np.frombuffer(s.encode().translate(bytes.maketrans(b"ACGT", bytes(range(4)))), dtype=np.uint8)
            assert codes.size == 0 or codes.max() < 4, "ACGT only"
            pad = np.zeros(4 * ((len(s) + 3) // 4), dtype=np.uint8)
            pad[:len(s)] = codes
            q = pad.reshape(-1, 4)
            self.packed[int(off):int(off) + q.shape[0]] = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)
        self.c = capi.PagSeqs(len(seqs), self.byte_off.ctypes.data, self.len.ctypes.data, self.packed.ctypes.data, self.packed.size)


GUARD = 64


def device_render(lib, records, k, ctgs, refs, deviation, error_rate=ERROR_RATE, cap=None):
    """ctgs, refs: Packed.  -> (rc, bytes needed, what the buffer holds up to `cap`, True if the guard bytes behind `cap` are
    untouched); cap None: asked for first (a call with cap 0), then rendered into exactly that many bytes"""
    records = np.ascontiguousarray(records, dtype=NODE)
    need = C.c_uint64(0)
    args = (records.ctypes.data, len(records), k, C.byref(ctgs.c), C.byref(refs.c), deviation, error_rate)
    if cap is None:
        rc = lib.pag_render_path_sequence(*args, None, 0, C.byref(need), 0)
        assert rc in (PAG_OK, PAG_ERANGE), rc
        assert (rc == PAG_OK) == (need.value == 0)
        cap = need.value
    buf = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    rc = lib.pag_render_path_sequence(*args, buf.ctypes.data, cap, C.byref(need), 0)
    return rc, need.value, buf[:cap].tobytes(), bool((buf[cap:] == 0xA5).all())
