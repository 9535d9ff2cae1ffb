"""Inputs as sequencing pipelines leave them, for one end-to-end golden (tests/golden/messy_inputs_t1, made by
tests/golden/make_messy_golden.py): a synth.Spec plus a deterministic REWRITE of the written files.  tests/synth.py itself never
emits a lower-case base, an N, a CR or anything but clean rows, so without this case no run against the reference contains one.
The rewrite draws from a generator of its own, so no existing fixture drifts.

  bases     in the reads (<block>.new.fastq), the contigs (ctg.fasta) and the references (ref.fasta): about 10 % of the bases
            lower-cased, about 1 % turned into N / R / Y / K / M (CompressedSeq packs every such letter as A);
  rows      in the query rows of the three ALN files (<block>.ctg.ref, <block>.ref.ref, aln): stretches lower-cased, so that case
            alone makes mismatch columns (parseDiff compares characters); reference rows and headers are not touched;
  crlf      the FASTQ and the contig FASTA written with CRLF line ends, the contigs one line per record: the CR of a sequence line
            is a base to the reference's reader (it packs as A), so every read and every contig gains ONE trailing A.  ref.fasta
            keeps its LF line ends: its records are multi-line, and every line's CR would be a base in the middle of the sequence.

What the rewrite leaves alone is pinned at function level (tests/test_loader_pins.py): ALN headers, `;` lines, blank headers.
tests/test_messy_case.py asserts from the committed inputs that the case holds what it is named for."""
import os

import numpy as np

import synth

SPEC = dict(seed=211, ref_len=9000, n_reads=230, read_len=900, k=8, contigs=[(150, 4200, False), (4450, 8850, True)])
THREADS, EPS, COV = 1, 10, 2
NAME = "messy_inputs_t1"

IUPAC = np.frombuffer(b"NRYKM", dtype=np.uint8)
LOWER_FRAC, IUPAC_FRAC = 0.10, 0.01
ROW_STRETCH_EVERY = 3      # one ALN record in three gets lower-case stretches in its query row


def _messy_bases(rng, seq: bytes) -> bytes:
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    letters = (a >= ord("A")) & (a <= ord("Z"))
    odd = letters & (rng.random(len(a)) < IUPAC_FRAC)
    a[odd] = IUPAC[rng.integers(0, len(IUPAC), int(odd.sum()))]
    low = letters & (rng.random(len(a)) < LOWER_FRAC)
    a[low] |= 0x20
    return a.tobytes()


def _rewrite_fastq(rng, path, crlf):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    lines.pop()
    for i in range(1, len(lines), 4):
        lines[i] = _messy_bases(rng, lines[i])
    end = b"\r\n" if crlf else b"\n"
    open(path, "wb").write(b"".join(ln + end for ln in lines))


def _rewrite_fasta(rng, path, single_line_crlf):
    recs, name, parts = [], None, []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            if name is not None:
                recs.append((name, parts))
            name, parts = ln, []
        elif ln:
            parts.append(ln)
    recs.append((name, parts))
    out = []
    for name, parts in recs:
        messy = _messy_bases(rng, b"".join(parts))
        if single_line_crlf:
            out.append(name + b"\r\n" + messy + b"\r\n")
        else:  # (the line lengths as they were)
            out.append(name + b"\n")
            at = 0
            for p in parts:
                out.append(messy[at:at + len(p)] + b"\n")
                at += len(p)
    open(path, "wb").write(b"".join(out))


def _rewrite_aln(rng, path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 3 == 0
    lines.pop()
    for r in range(0, len(lines) // 3, ROW_STRETCH_EVERY):
        q = bytearray(lines[3 * r + 1])
        for _ in range(1 + len(q) // 400):
            n = int(rng.integers(5, 30))
            at = int(rng.integers(0, max(1, len(q) - n)))
            q[at:at + n] = bytes(q[at:at + n]).lower()
        lines[3 * r + 1] = bytes(q)
    open(path, "wb").write(b"".join(ln + b"\n" for ln in lines))


def rewrite(d, block=0, seed=977):
    """the rewrite described above, on the files of input directory d, in a fixed order"""
    rng = np.random.default_rng(seed)
    _rewrite_fastq(rng, os.path.join(d, f"{block}.new.fastq"), crlf=True)
    _rewrite_fasta(rng, os.path.join(d, "ctg.fasta"), single_line_crlf=True)
    _rewrite_fasta(rng, os.path.join(d, "ref.fasta"), single_line_crlf=False)
    for f in (f"{block}.ctg.ref", f"{block}.ref.ref", "aln"):
        _rewrite_aln(rng, os.path.join(d, f))


def generate(dest, messy=True):
    """the case's input directory written into dest (messy=False: the same Spec without the rewrite)"""
    synth.generate(synth.Spec(**{**SPEC, "contigs": [tuple(c) for c in SPEC["contigs"]]}), dest)
    if messy:
        rewrite(dest)
    return dest


# ---- what a test can count in an input directory ------------------------------------------------------------------------------
def _seq_lines(path):
    data = open(path, "rb").read()
    lines = data.split(b"\n")
    if data[:1] == b"@":
        return lines[1::4]
    return [ln for ln in lines if ln and not ln.startswith(b">")]


def census(d, block=0):
    """counts of what the case is named for, over the files of input directory d"""
    out = {"lower_case_bases": 0, "iupac_bases": 0, "cr_bytes_in_sequence_lines": 0, "case_only_mismatch_columns": 0, "lower_case_ref_row_letters": 0}
    for f in (f"{block}.new.fastq", "ctg.fasta", "ref.fasta"):
        for ln in _seq_lines(os.path.join(d, f)):
            a = np.frombuffer(ln, dtype=np.uint8)
            out["lower_case_bases"] += int(((a >= ord("a")) & (a <= ord("z"))).sum())
            out["iupac_bases"] += int(np.isin(a & 0xDF, IUPAC).sum())
            out["cr_bytes_in_sequence_lines"] += int((a == 13).sum())
    for f in (f"{block}.ctg.ref", f"{block}.ref.ref", "aln"):
        lines = open(os.path.join(d, f), "rb").read().split(b"\n")
        for r in range((len(lines) - 1) // 3):
            q, t = np.frombuffer(lines[3 * r + 1], dtype=np.uint8), np.frombuffer(lines[3 * r + 2], dtype=np.uint8)
            assert len(q) == len(t)
            out["case_only_mismatch_columns"] += int(((q != t) & ((q | 0x20) == (t | 0x20)) & (q != ord("-")) & (t != ord("-"))).sum())
            out["lower_case_ref_row_letters"] += int(((t >= ord("a")) & (t <= ord("z"))).sum())
    return out
