"""CPU: PAlgorithm::seqToString restated in Python from path records (tests/seq_text.py) against every golden .fasta, and the C
ABI of the device renderer (pag_render_path_sequence, pag_travel_seq_sources, pag_travel_seq_text, PAG_TRAVEL_RENDER_SEQS)."""
import ctypes as C
import os
import subprocess

import pytest

import dump_text
import pagctl
import seq_text
from aligngraph2_amd import capi


def test_restatement_reproduces_every_golden_fasta_from_the_golden_dumps(workdir):
    """For every golden .fasta: the pieces its .con names, each rendered from the records parsed out of its golden dump
    file, concatenated, are the FASTA body.  That pins the restatement to the reference's outputs; the GPU tests then use it as
    the oracle for records no golden has.  The counts say what the goldens reach: steps read through the contig space, through
    the reference space, on a reverse strand, and positions rounded exactly at .5."""
    cases = seq_text.fasta_cases()
    assert len(cases) == 8
    counts = seq_text.Counts()
    n_files = n_pieces = n_bases = 0
    for name in cases:
        ctgs, refs = seq_text.case_sequences(name, workdir)
        cm, rm = dump_text.Mapper([len(s) for s in ctgs]), dump_text.Mapper([len(s) for s in refs])
        for f, (body, pieces) in seq_text.golden_pieces(name).items():
            got = []
            for dump, k, records in pieces:
                text = seq_text.render(records, k, ctgs, refs, cm, rm, seq_text.deviation_of(name), counts=counts)
                assert text is not None, f"{name}/{dump}: not renderable"
                assert len(text) == seq_text.expected_bytes(records, k)
                got.append(text)
                n_pieces += 1
            assert b"".join(got).decode() == body, f"{name}/{f}"
            n_files += 1
            n_bases += len(body)
    assert n_files == 9
    assert n_pieces == 20
    assert n_bases == 90258
    assert (counts.short, counts.long, counts.long_bases) == (25371, 496, 6575)
    assert (counts.ctg, counts.ref, counts.reverse, counts.half) == (472, 24, 2, 14)
    assert counts.pos_similar == 0  # (no golden decides by isPosSimilar: the constructed records of the GPU tests do)


def test_restatement_at_its_corners():
    ctgs, refs = ["ACGTACGTAC" * 3, "TTTTGGGGCC"], ["ACGT" * 20]
    cm, rm = dump_text.Mapper([len(s) for s in ctgs]), dump_text.Mapper([len(s) for s in refs])
    k = 3
    c0 = cm.starts[0]
    code = dump_text.kmer_code
    # steps <= k: the k-mer's tail; <= 0: nothing
    recs = [(code("ACG"), c0, 0, 1, 3), (code("CGT"), c0 + 1, 0, 1, 1), (code("TAC"), c0 + 3, 0, 1, 2), (code("GGG"), c0 + 3, 0, 1, 0),
            (code("CCC"), c0 + 2, 0, 1, -3), (code("TTT"), c0 + 6, 0, 1, 3)]
    assert seq_text.render(recs, k, ctgs, refs, cm, rm, 4) == b"ACG" + b"T" + b"AC" + b"" + b"" + b"TTT"
    assert seq_text.expected_bytes(recs, k) == 9
    # a long step along the forward strand of contig 0: bases 3 .. 6 behind the previous k-mer, then the k-mer
    recs = [(code("ACG"), c0, 0, 1, 3), (code("ACG"), c0 + 8, 0, 1, 8)]
    assert seq_text.render(recs, k, ctgs, refs, cm, rm, 4) == b"ACG" + b"tacgt" + b"ACG"
    # ... along its reverse strand: complement of base len - 1 - idx
    r0 = c0 + 2 * len(ctgs[0])
    recs = [(code("GTA"), r0, 0, 1, 3), (code("GTA"), r0 + 8, 0, 1, 8)]
    assert seq_text.render(recs, k, ctgs, refs, cm, rm, 4) == b"GTA" + b"cgtac" + b"GTA"
    # both coordinates 0: every base 'n'
    recs = [(code("AAA"), 0, 0, 1, 3), (code("CCC"), 0, 0, 1, 7)]
    assert seq_text.render(recs, k, ctgs, refs, cm, rm, 4) == b"AAA" + b"nnnn" + b"CCC"
    # a line that dips below 0 is not renderable: the reference coordinate 5 lies before the first start (offset -235 of
    # strand -1), the step's line runs from offset 1 + k down to it
    r0 = rm.starts[0]
    assert rm.single_to_dual(5) == (-1, 5 - r0 - 2 * len(refs[0]))
    recs = [(code("AAA"), 0, r0 + 1, 1, 3), (code("CCC"), 0, 5, 1, 40)]
    assert seq_text.render(recs, k, ctgs, refs, cm, rm, 4) is None
    assert seq_text.round_half_away(2.5) == 3 and seq_text.round_half_away(-2.5) == -3 and seq_text.round_half_away(0.49999999999999994) == 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pagctl.HIP_LIB):
        subprocess.run(["make", "-C", pagctl.ROOT, "product"], check=True, capture_output=True)
    return capi.bind(C.CDLL(pagctl.HIP_LIB))


def test_library_exports_the_renderer_and_capi_declares_it(lib):
    for f, n_args in (("pag_render_path_sequence", 11), ("pag_travel_seq_sources", 2), ("pag_travel_seq_text", 4)):
        assert hasattr(lib, f), f"libpagraph_hip.so does not export {f}"
        assert f in capi.SIGNATURES and len(capi.SIGNATURES[f][1]) == n_args
    assert capi.SIGNATURES["pag_travel_seq_text"][0] is C.c_void_p
    assert capi.PAG_TRAVEL_RENDER_SEQS == 2 and capi.PAG_TRAVEL_RENDER_DUMPS == 1
    assert capi.PAG_EDOM == -33 and capi.PAG_EDOM not in (capi.PAG_OK, capi.PAG_ERANGE, capi.PAG_EINVAL, capi.PAG_ENODEV, capi.PAG_EFAULT, capi.PAG_ENOMEM)
    host = C.CDLL(os.path.join(pagctl.ROOT, "aligngraph2_amd", "libpagraph_host.so"))
    assert hasattr(host, "pagh_assemble_paths_seq") and len(capi.SIGNATURES["pagh_assemble_paths_seq"][1]) == 20
    # the sources and the text of a handle that does not exist
    n = C.c_uint64(7)
    assert lib.pag_travel_seq_text(None, 0, 1, C.byref(n)) is None and n.value == 0
    assert lib.pag_travel_seq_sources(None, None) == capi.PAG_EINVAL


def test_renderer_has_no_cpu_fallback(lib):
    """Without a gfx950 device the call fails with PAG_ENODEV (bad arguments are refused before the device is looked for);
    with one it renders."""
    ctgs, refs = seq_text.Packed(["ACGTACGTACGT"]), seq_text.Packed(["ACGTACGT"])
    c0 = 12
    recs = dump_text.to_records([(dump_text.kmer_code("ACG"), c0, 0, 1, 3), (dump_text.kmer_code("ACG"), c0 + 8, 0, 1, 8)])
    need = C.c_uint64(7)
    args = (recs.ctypes.data, 2)
    tail = (C.byref(ctgs.c), C.byref(refs.c), 4, 0.15)
    assert lib.pag_render_path_sequence(*args, 17, *tail, None, 0, C.byref(need), 0) == capi.PAG_EINVAL and need.value == 0
    assert lib.pag_render_path_sequence(*args, 0, *tail, None, 0, C.byref(need), 0) == capi.PAG_EINVAL
    assert lib.pag_render_path_sequence(*args, 3, *tail, None, 0, None, 0) == capi.PAG_EINVAL
    assert lib.pag_render_path_sequence(*args, 3, None, C.byref(refs.c), 4, 0.15, None, 0, C.byref(need), 0) == capi.PAG_EINVAL
    rc, n, text, guard_ok = seq_text.device_render(lib, recs, 3, ctgs, refs, 4, cap=64)
    if lib.pag_device_available():
        assert rc == capi.PAG_OK and guard_ok and n == 11
        assert text[:n] == b"ACG" + b"tacgt" + b"ACG"
    else:
        assert rc == capi.PAG_ENODEV and guard_ok
        assert n == 11, "the size is a sum over the records: reported without a device too"
