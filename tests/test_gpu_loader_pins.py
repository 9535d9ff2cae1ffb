"""GPU: the ingest kernels (k_ingest.hip) against what the REFERENCE's own readers make of the same files.  The expectation is
not restated here: it is read from the committed dumps under tests/golden/loaders/ (oracle/ref_harness/loader_dump.cpp over
AutoSeqDatabase and over AlignmentHelper::loadFromRefFile + ParseAlignTools::parseDiff; tests/golden/make_loader_golden.py).
The test finds the lines of a file by plain splitting at `\\n`, as std::getline does, and hands the spans to the kernels:

  pag_pack_text_seqs     every FASTQ file of tests/loader_cases.py and every FASTA file whose records are single-line: a span is as
                         long as the reference's record (a CR counts as a base), and packs to the bytes the reference's base string
                         gives by A C G T -> 0 1 2 3, zero up to the stored size, nothing written behind the last sequence;
  pag_classify_columns   every ALN file against its `rows` dump (file order): the class of a column is queryDiff + 2 refDiff, the
                         two per-record counts are the columns of class != 1 and != 2, nothing written behind the last word;
  pag_classify_columns_host   the same through the entry that brings the results back to host arrays.

`widths.aln` / `widths.fq` carry the sizes at which these kernels take another turn: 16 columns per word, 64 lanes, 256 threads
(rows of 0 ... 1025 columns), a reference row one shorter and one longer than its query row."""
import numpy as np
import pytest

import loader_cases
import loader_pins
import pagctl


def lines_of(data: bytes):
    """(offset, length) of every line as std::getline returns them: no `\\n`, a `\\r` stays, a last line without `\\n` counts"""
    out, at = [], 0
    parts = data.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    for p in parts:
        out.append((at, len(p)))
        at += len(p) + 1
    return out


def seq_spans(data: bytes):
    """the sequence line of every record, or None for a FASTA file with a record that is not one header and one line"""
    ln = lines_of(data)
    if data[:1] in (b">", b";"):
        if len(ln) % 2:
            return None
        for i, (at, _) in enumerate(ln):
            if (data[at:at + 1] == b">") != (i % 2 == 0):
                return None
        return ln[1::2]
    return [ln[4 * r + 1] for r in range(len(ln) // 4)]


PACKABLE = [name for name in sorted(loader_cases.SEQ_CASES) if seq_spans(loader_cases.SEQ_CASES[name]) is not None]


def test_the_packable_files_are_the_ones_meant():
    assert [n for n in PACKABLE if n.endswith(".fa")] == ["crlf_single.fa", "empty.fa", "empty_names.fa", "nonl.fa"]
    assert [n for n in sorted(loader_cases.SEQ_CASES) if n.endswith(".fq")] == [n for n in PACKABLE if n.endswith(".fq")]


CODE = np.zeros(256, dtype=np.uint8)
for _ch, _v in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3)):
    CODE[_ch[0]] = _v


def stored_bytes(n):
    return ((n + 3) // 4 + 3) & ~3


def pack_reference_string(s: bytes) -> np.ndarray:
    """the reference's toString(true) of a record -> its stored bytes (pag_seqs: 4 bases per byte, base i at bits 2 (i & 3))"""
    assert set(s) <= set(b"ACGT")
    codes = np.zeros(stored_bytes(len(s)) * 4, dtype=np.uint8)
    codes[:len(s)] = CODE[np.frombuffer(s, dtype=np.uint8)]
    c = codes.reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [True, False], ids=["text_on_device", "text_on_host"])
@pytest.mark.parametrize("name", PACKABLE)
def test_text_records_pack_to_the_reference_s_sequences(name, on_device):
    import torch
    hip = pagctl.hip_lib()
    data = loader_cases.SEQ_CASES[name]
    spans = seq_spans(data)
    recs = [f for f in loader_pins.golden_lines(name, "seq") if f[0] == b"R"]
    assert len(spans) == len(recs), "records found by line splitting against the reference's"
    for i, ((_, n), f) in enumerate(zip(spans, recs)):
        assert n == int(f[3]), f"record {i}: the span has {n} characters, the reference's sequence {int(f[3])} bases"
    off = np.array([a for a, _ in spans], dtype=np.uint64)
    ln = np.array([n for _, n in spans], dtype=np.uint32)
    boff = np.concatenate([[0], np.cumsum([stored_bytes(int(n)) for n in ln])]).astype(np.uint64)
    total = int(boff[-1])
    out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    tbuf = np.frombuffer(data, dtype=np.uint8)
    if on_device:
        tdev = torch.from_numpy(tbuf.copy()).cuda() if len(data) else torch.zeros(4, dtype=torch.uint8, device="cuda")
        tptr = tdev.data_ptr()
    else:
        tptr = tbuf.ctypes.data if len(data) else 0
    boff0 = np.ascontiguousarray(boff[:-1])
    rc = hip.pag_pack_text_seqs(tptr, 1 if on_device else 0, len(data), off.ctypes.data, ln.ctypes.data, len(spans), boff0.ctypes.data, out.data_ptr(), total, 0)
    assert rc == 0, hip.pag_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, f in enumerate(recs):
        want = pack_reference_string(b"" if f[4] == b"-" else f[4])
        assert np.array_equal(got[int(boff[i]):int(boff[i + 1])], want), f"record {i} ({int(f[3])} bases)"
    assert (got[total:] == 0xAB).all()  # (nothing written behind the last sequence)


def _bits(field: bytes) -> np.ndarray:
    return np.zeros(0, dtype=np.uint32) if field == b"-" else (np.frombuffer(field, dtype=np.uint8) - ord("0")).astype(np.uint32)


def rows_expectation(name):
    """per record of the `rows` dump: (class words, columns that emit a query base, columns that advance the reference)"""
    out = []
    for f in loader_pins.golden_lines(name, "rows"):
        assert len(f) == 14 and f[0] == b"H"
        qd, rd = _bits(f[12]), _bits(f[13])
        assert len(qd) == len(rd)
        cls = qd | (rd << 1)
        padded = np.zeros((len(cls) + 15) // 16 * 16, dtype=np.uint64)
        padded[:len(cls)] = cls
        words = (padded.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
        out.append((words, int((cls != 1).sum()), int((cls != 2).sum()), len(cls)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["text_on_device", "text_on_host", "results_to_host"])
@pytest.mark.parametrize("name", sorted(loader_cases.ALN_CASES))
def test_alignment_rows_classify_to_the_reference_s_diff_vectors(name, route):
    import torch
    hip = pagctl.hip_lib()
    data = loader_cases.ALN_CASES[name]
    ln = lines_of(data)
    n_recs = len(ln) // 3
    want = rows_expectation(name)
    assert n_recs == len(want), "records found by line splitting against the reference's"
    q, r = [ln[3 * i + 1] for i in range(n_recs)], [ln[3 * i + 2] for i in range(n_recs)]
    for i in range(n_recs):
        assert q[i][1] == want[i][3], f"record {i}: one column per character of the query row"
    a = lambda x, dt: np.array(x, dtype=dt)  # noqa: E731
    qo, ql, ro, rl = a([x for x, _ in q], np.uint64), a([n for _, n in q], np.uint32), a([x for x, _ in r], np.uint64), a([n for _, n in r], np.uint32)
    doff = np.concatenate([[0], np.cumsum([(n + 15) // 16 for _, n in q])]).astype(np.uint64)
    total = int(doff[-1])
    doff0 = np.ascontiguousarray(doff[:-1])
    tbuf = np.frombuffer(data, dtype=np.uint8)
    if route == "results_to_host":
        diff = np.full(total + 8, 0x5A5A5A5A, dtype=np.uint32)
        ne, nr = np.full(n_recs + 2, 0x5A5A5A5A, dtype=np.uint32), np.full(n_recs + 2, 0x5A5A5A5A, dtype=np.uint32)
        rc = hip.pag_classify_columns_host(tbuf.ctypes.data if len(data) else 0, len(data), qo.ctypes.data, ql.ctypes.data, ro.ctypes.data, rl.ctypes.data,
                                           doff0.ctypes.data, n_recs, diff.ctypes.data, total, ne.ctypes.data, nr.ctypes.data, 0)
        assert rc == 0, hip.pag_last_error()
        assert (ne[n_recs:] == 0x5A5A5A5A).all() and (nr[n_recs:] == 0x5A5A5A5A).all()
        got, got_e, got_r = diff, ne[:n_recs], nr[:n_recs]
    else:
        d_diff = torch.full((total + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_ne = torch.zeros(max(n_recs, 1), dtype=torch.int32, device="cuda")
        d_nr = torch.zeros(max(n_recs, 1), dtype=torch.int32, device="cuda")
        if route == "text_on_device":
            tdev = torch.from_numpy(tbuf.copy()).cuda() if len(data) else torch.zeros(4, dtype=torch.uint8, device="cuda")
            tptr = tdev.data_ptr()
        else:
            tptr = tbuf.ctypes.data if len(data) else 0
        rc = hip.pag_classify_columns(tptr, 1 if route == "text_on_device" else 0, len(data), qo.ctypes.data, ql.ctypes.data, ro.ctypes.data, rl.ctypes.data,
                                      doff0.ctypes.data, n_recs, d_diff.data_ptr(), total, d_ne.data_ptr(), d_nr.data_ptr(), 0)
        assert rc == 0, hip.pag_last_error()
        torch.cuda.synchronize()
        got = d_diff.cpu().numpy().view(np.uint32)
        got_e, got_r = d_ne.cpu().numpy().view(np.uint32)[:n_recs], d_nr.cpu().numpy().view(np.uint32)[:n_recs]
    for i, (words, e, rr, n) in enumerate(want):
        assert np.array_equal(got[int(doff[i]):int(doff[i + 1])], words), f"record {i} ({n} columns): class words"
        assert (int(got_e[i]), int(got_r[i])) == (e, rr), f"record {i} ({n} columns): counts"
    assert (got[total:] == 0x5A5A5A5A).all()  # (nothing written behind the last word)
