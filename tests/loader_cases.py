"""Input files for the loader pins (tests/test_loader_pins.py, tests/test_gpu_loader_pins.py): sequence files and 3-line ALN
files as byte strings, each written out and read by the REFERENCE's own readers once (oracle/ref_harness/loader_dump.cpp,
tests/golden/make_loader_golden.py -> tests/golden/loaders/<file>.<mode>.txt) and by the product's loaders and ingest kernels in
every test run.  The files are ours; what the reference made of them is the committed dump.

Left out on purpose, because the reference's own run on them is not defined (make_loader_golden.py refuses such a file):
  * an ALN record whose reference row is shorter than its query row by TWO or more: parseDiff reads operator[] past size()
    (one shorter reads the terminating NUL, which is defined; `widths.aln` has that one);
  * a sequence file whose first record has no header token at all (a first line that is empty or blank): AutoSeqDatabase takes
    substr(1) of an empty string and throws."""


def _lcg(seed):
    state = seed & 0xFFFFFFFFFFFFFFFF
    while True:
        state = (state * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        yield state >> 33


def _row_pair(n, rng, alphabet=b"ACGT-acgtN"):
    """a query row of n characters and a reference row that differs from it in about 20 % of the columns"""
    q = bytes(alphabet[next(rng) % len(alphabet)] for _ in range(n))
    r = bytes(alphabet[next(rng) % len(alphabet)] if next(rng) % 5 == 0 else c for c in q)
    return q, r


def _aln(records):
    return b"".join(h + b"\n" + q + b"\n" + r + b"\n" for h, q, r in records)


WIDTHS = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)


def _widths_aln():
    rng = _lcg(11)
    recs = []
    for i, n in enumerate(WIDTHS):
        q, r = _row_pair(n, rng)
        recs.append((b"w%d ctg F %d 0 %d %d 0 %d %d" % (i, 100 + i, n, n, n, n), q, r))
    q, r = _row_pair(70, rng)
    recs.append((b"short ctg R 7 0 70 70 0 69 69", q, r[:-1]))      # the reference row ONE shorter: its NUL is a mismatch column
    q, r = _row_pair(33, rng)
    recs.append((b"long ctg F 8 0 33 33 0 50 50", q, r + b"ACGTACGTACGTACGTA"))  # ... and a longer one: ignored past the query row
    return _aln(recs)


def _ties_aln(n):
    """n records with scores i % 3 (Mecat) and queryEnd - queryBegin = (5 i) % 4 (Mummer): the order std::sort leaves"""
    recs = []
    for i in range(n):
        q = (b"ACGTTGCA" * 2)[i % 5: i % 5 + 4 + i % 4]
        r = q[:1] + b"-" + q[2:] if i % 2 else q
        recs.append((b"q%d ctg%d %s %d %d %d 99 %d %d 99" % (i, i % 4, b"FR"[i % 2:i % 2 + 1], i % 3, i, i + (5 * i) % 4, 2 * i, 2 * i + len(q)), q, r))
    return _aln(recs)


def _widths_fq():
    rng = _lcg(23)
    alphabet = b"ACGTacgtNnRYKM"
    out = b""
    for i, n in enumerate((0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)):
        sq = bytes(alphabet[next(rng) % len(alphabet)] for _ in range(n))
        out += b"@w%d len=%d\n%s\n+\n%s\n" % (i, n, sq, b"I" * n)
    return out


# ---- sequence files (FASTA / FASTQ): mode `seq`
SEQ_CASES = {
    # the nine files of tests/test_loaders.py
    "plain.fa": b">a desc\nACGTACGTAC\nGGTT\n>b\nTTTT\n",
    "prefix.fa": b";comment first\nGATTACA\n>first rec\nACGT\nAC\n>second\n\nGG\n\n",
    "crlf.fa": b">r1\r\nACGT\r\nTTGA\r\n>r2\r\nCC\r\n",
    "nonl.fa": b">only\nACGTNNNNacgtRYKM",
    "dup.fa": b">same\nAAAA\n>same\nCCCCCC\n>other\n>empty_next\n\n>last\nT",
    "long.fa": b">big one\n" + b"\n".join((b"ACGTTGCAAGCT" * 9)[:100] for _ in range(5000)) + b"\nACG\n>tail\nA\n",
    "reads.fq": b"".join(b"@r%d extra\n%s\n+\n%s\n" % (i, (b"ACGTTGCA" * (i % 7 + 1))[: 5 + i % 11], b"I" * (5 + i % 11)) for i in range(300)),
    "partial.fq": b"@a\nACGT\n+\nIIII\n@b\nGG\n+\n",
    "empty.fa": b"",
    # what the reference makes of these is neither obvious nor (before these pins) tested
    "crlf.fq": b"@a\r\nACGT\r\n+\r\nIIII\r\n",                                   # the CR is a base
    "crlf_single.fa": b">c1 x\r\nACGTTGCAACGTTGCAA\r\n>c2\r\nGG\r\n",            # ... in single-line FASTA records too
    "blank_header.fq": b"@a x\nACGT\n+\nIIII\n\nGGN\n+\nIII\n@\nTT\n+\nII\n",      # a blank header re-uses the previous token
    "space_header.fq": b"@\nAC\n+\nII\n   \nGG\n+\nII\n",
    "empty_names.fa": b">\tq1 d\nAC\n> \nGG\n",
    "dup.fq": b"@same\nAAAA\n+\nIIII\n@other\nGG\n+\nII\n@same\nCCCCCC\n+\nIIIIII\n",  # the later record of a name wins the map
    "semicolon_mid.fa": b">a\nAC\n;not a header\nGT\n>b\nTT\n",                   # `;` starts a record nowhere
    "unknown_type.fq": b"xq1 d\nACGT\n+\nIIII\nyq2\nGGC\n+\nIII\n",                # neither `>` nor `@`: read as FASTQ
    "nonl.fq": b"@a\nACGTN\n+\nIIIII\n@b\ngattaca\n+\nIIIIIII",                   # no final newline: the last record counts
    "widths.fq": _widths_fq(),                                                     # word edges of the packers, lower case, N, IUPAC
}

# ---- 3-line ALN files: modes `mecat`, `mummer`, `rows`
ALN_CASES = {
    "plain.aln": _aln([(b"q1 ctg F 30 0 8 8 10 18 40", b"ACGT-CGTA", b"ACGTACG-A"),
                       (b"q2 ctg R 45 2 9 9 0 7 40", b"acgtACG", b"ACGTACG"),       # case alone is a mismatch
                       (b"q1 ref F 12 1 5 8 3 7 50", b"ANNT", b"AnNT")]),
    "crlf.aln": b"q1 r F 5 0 4 4 0 4 4\r\nAC-T\r\nACGT\r\n" + b"q2 r R 9 0 2 2 0 2 2\r\nGG\r\nGC\r\n",  # a CR column that matches
    "nine_fields.aln": _aln([(b"q1 r F 7 0 4 4 0 4 4", b"ACGT", b"ACGA"),
                             (b"q2 r F 9 1 4 4 0 3", b"AC-T", b"ACGT"),             # Mecat: zeroed, rows still parsed; Mummer: good
                             (b"q3 r R 3 0 2 2 0 2 2", b"GG", b"G-"),
                             (b"q4 r F 8 0", b"TTT", b"TAT"),                        # bad for both; Mummer drops it
                             (b"q5 r F 1 2 6 9 0 4 4", b"ACGT", b"ACGT")]),
    "odd_numbers.aln": _aln([(b"q3 r F 1e3 -1 +3 3 0 3 9 extra", b"ACG", b"ACG"),    # atoll("1e3") = 1, -1 wraps, extra field ignored
                             (b"q4 r F -7 0 3 3 0 3 9", b"AC-", b"ACG"),             # (size_t)atoll = 2^64 - 7: sorts first
                             (b"q5 r F 4 0 99999999999999999999 3 0 3 9", b"A-G", b"ACG"),    # 20 digits: extraction fails, zeroed
                             (b"q6 r F 4 0 18446744073709551615 3 0 3 9", b"ACT", b"ACG"),    # 2^64 - 1 parses
                             (b"q7 r F 4 0 18446744073709551616 3 0 3 9", b"TCT", b"ACG"),    # 2^64 does not
                             (b"q8 r F 4 0 9999999999999999999 3 5 3 9", b"AGT", b"ACG"),     # 19 digits parse
                             (b"q9 r F 2 0x10 3 3 0 3 9", b"A", b"C"),                        # `0x10` reads 0 and fails on `x`
                             (b"q10 r FF 2 007 3 3 0 3 9", b"AA", b"CA"),                     # forward only for exactly `F`
                             (b"  q11\tr  F 6  1 3\t3 0 3 9  ", b"GA", b"GA")]),              # blanks and tabs between the fields
    "ties40.aln": _ties_aln(40),
    "ties16.aln": _ties_aln(16),                                                    # (std::sort's insertion-sort range)
    "trailing_header.aln": _aln([(b"q1 r F 5 0 4 4 0 4 4", b"ACGT", b"ACCT")]) + b"q2 r F 9 0 2 2 0 2 2\n",
    "trailing_header_row.aln": _aln([(b"q1 r F 5 0 4 4 0 4 4", b"ACGT", b"ACCT")]) + b"q2 r F 9 0 2 2 0 2 2\nGG\n",
    "nonl.aln": b"q1 r F 5 0 4 4 0 4 4\nACGT\nAC-T",                                # no final newline: the record counts
    "empty.aln": b"",
    "widths.aln": _widths_aln(),
}

ALN_MODES = ("mecat", "mummer", "rows")


def all_dumps():
    """(file name, mode) of every committed dump"""
    return [(name, "seq") for name in sorted(SEQ_CASES)] + [(name, mode) for name in sorted(ALN_CASES) for mode in ALN_MODES]


def write_inputs(directory):
    import os
    os.makedirs(directory, exist_ok=True)
    for name, data in list(SEQ_CASES.items()) + list(ALN_CASES.items()):
        with open(os.path.join(directory, name), "wb") as f:
            f.write(data)
