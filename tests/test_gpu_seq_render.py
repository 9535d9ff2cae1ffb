"""GPU: the consensus sequences of the paths rendered on the device (csrc/hip/k5_seq.hip) — records -> text through
pag_render_path_sequence against the golden FASTA pieces and, on constructed records, against the Python restatement that
tests/test_seq_render.py pins to those goldens; pag_travel with PAG_TRAVEL_RENDER_SEQS; then bin/pagraph with
PAGRAPH_DEVICE_SEQS=1 on every route to a chain's .fasta."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import dump_text
import goldens
import pagctl
import seq_text
import synth
from aligngraph2_amd import capi

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pagraph")
TILE = 256          # vertices per tile of the render kernels
STAGE = 16384       # bytes of a tile the render kernel stages in LDS (more: straight to the output)
DEV, ERR = 20, seq_text.ERROR_RATE


@pytest.fixture(scope="module")
def lib():
    return capi.bind(C.CDLL(pagctl.HIP_LIB))


_case_cache = {}


def case(name, workdir):
    """(contig strings, reference strings, their Packed forms, both Mappers) of a golden case, made once"""
    if name not in _case_cache:
        ctgs, refs = seq_text.case_sequences(name, workdir)
        _case_cache[name] = (ctgs, refs, seq_text.Packed(ctgs), seq_text.Packed(refs), dump_text.Mapper([len(s) for s in ctgs]),
                             dump_text.Mapper([len(s) for s in refs]))
    return _case_cache[name]


def first_difference(got, want):
    if got == want:
        return None
    at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return f"first difference at byte {at}: {got[max(0, at - 40):at + 40]!r} != {want[max(0, at - 40):at + 40]!r}"


# ---- 1. the golden records: every path, and the FASTA bodies from their pieces

@pytest.mark.gpu
@pytest.mark.parametrize("name", goldens.case_names())
def test_device_renders_every_golden_path_and_fasta(name, lib, workdir):
    ctgs, refs, pc, pr, cm, rm = case(name, workdir)
    dev = seq_text.deviation_of(name)
    rendered = {}
    for f, k, records in seq_text.golden_paths(name):
        rc, need, got, guard_ok = seq_text.device_render(lib, dump_text.to_records(records), k, pc, pr, dev)
        assert rc == capi.PAG_OK and guard_ok, f"{name}/{f}: rc {rc}"
        want = seq_text.render(records, k, ctgs, refs, cm, rm, dev)
        assert want is not None and need == len(want) == seq_text.expected_bytes(records, k)
        assert first_difference(got, want) is None, f"{name}/{f}: {first_difference(got, want)}"
        rendered[f] = got
    for f, (body, pieces) in seq_text.golden_pieces(name).items():
        assert b"".join(rendered[dump] for dump, _, _ in pieces).decode() == body, f"{name}/{f}: the device's pieces are not the golden FASTA"


# ---- 2. constructed records against the restatement

CTG_LEN, REF_LEN = [36000, 2500, 900], [40000, 3000]


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(5)
    ctgs = ["".join("ACGT"[x] for x in rng.integers(0, 4, n)) for n in CTG_LEN]
    refs = ["".join("ACGT"[x] for x in rng.integers(0, 4, n)) for n in REF_LEN]
    return ctgs, refs, seq_text.Packed(ctgs), seq_text.Packed(refs), dump_text.Mapper(CTG_LEN), dump_text.Mapper(REF_LEN)


def long_step_ends(variant, L, k, cm, rm):
    """((ctg, ref) of the vertex before, (ctg, ref) of the vertex) that send a step of L bases the given way"""
    c0, c1, r0 = cm.starts[0], cm.starts[1], rm.starts[0]
    if variant == "forward contig":
        return (c0 + 50, 0), (c0 + 50 + L, 0)
    if variant == "reverse-strand contig":
        return (c0 + 2 * CTG_LEN[0] + 100, 0), (c0 + 2 * CTG_LEN[0] + 100 + L, 0)
    if variant == "reference":
        return (0, r0 + 70), (0, r0 + 70 + L)
    if variant == "isPosSimilar":  # neither coordinate edge-similar (for L well above the deviation), the contig coordinates 5 apart
        return (c0 + 900, r0 + 100), (c0 + 905, r0 + 103)
    if variant == "isPosSimilar says no":  # ... 50 apart: the reference it is
        return (c0 + 900, r0 + 100), (c0 + 950, r0 + 103)
    if variant == "both 0":
        return (0, 0), (0, 0)
    if variant == "past the end":
        return (c1 + CTG_LEN[1] - 10, 0), (c1 + CTG_LEN[1] - 10 + L, 0)
    if variant == "into the next sequence":
        return (c1 + 100 - L, 0), (c1 + 100, 0)
    if variant == "half steps":  # posDist * 2 == step: every other position exactly at .5
        return (0, r0 + 200), (0, r0 + 200 + L // 2)
    raise KeyError(variant)


VARIANTS = ["forward contig", "reverse-strand contig", "reference", "isPosSimilar", "isPosSimilar says no", "both 0", "past the end",
            "into the next sequence", "half steps"]


def constructed(n, k, cm, rm, seed):
    """n records: short steps -3, 0, 1, k in turn; from record 4 on every ninth record (record 256, the first of the second
    tile, among them) takes a long step — k + 1, 1 500 or, once per variant, 30 000 bases — through the variants in turn"""
    rng = np.random.default_rng(seed)
    short = [1, k, 0, -3, max(1, k // 2)]
    tuples, ways = [], []
    for i in range(n):
        tuples.append([int(rng.integers(0, 1 << (2 * k))), cm.starts[0] + 3 * i, rm.starts[0] + 3 * i, i & 0xFFFF, k if i == 0 else short[i % len(short)]])
    e = 0
    for i in range(4, n, 9):
        variant = VARIANTS[e % len(VARIANTS)]
        L = 30000 if e < len(VARIANTS) else (k + 1, 1500)[(e // len(VARIANTS)) % 2]
        if variant == "half steps" and L % 2:
            L += 1
        (pc, pr), (nc, nr) = long_step_ends(variant, L, k, cm, rm)
        tuples[i - 1][1:3] = [pc, pr]
        tuples[i][1:3] = [nc, nr]
        tuples[i][4] = L
        ways.append((variant, L))
        e += 1
    return [tuple(t) for t in tuples], ways


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 7, 16])
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_constructed_records_against_the_restatement(n, k, lib, world):
    ctgs, refs, pc, pr, cm, rm = world
    tuples, ways = constructed(n, k, cm, rm, 100 * n + k)
    counts = seq_text.Counts()
    want = seq_text.render(tuples, k, ctgs, refs, cm, rm, DEV, ERR, counts=counts)
    assert want is not None and len(want) == seq_text.expected_bytes(tuples, k)
    if n >= TILE - 1:  # the records reach what they were made for
        assert {w for w, _ in ways} == set(VARIANTS) and {L for _, L in ways} >= {30000, 1500, k + 1}
        assert counts.ctg and counts.ref and counts.reverse and counts.half and counts.pos_similar >= 2
        assert b"n" * 100 in want and 30000 > STAGE
    if n > TILE:
        assert tuples[TILE][4] > k  # a long step whose previous vertex lies in the tile before
    rc, need, got, guard_ok = seq_text.device_render(lib, dump_text.to_records(tuples), k, pc, pr, DEV, ERR)  # (cap exact)
    assert rc == capi.PAG_OK, f"rc {rc}"
    assert need == len(want)
    assert guard_ok, "bytes behind the buffer were written"
    assert first_difference(got, want) is None, first_difference(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("L", [1500, 30000])
def test_one_long_step_each_way(variant, L, lib, world):
    """three records, the long step alone in its path: staged (1 500 bases) and beyond the staging buffer (30 000)"""
    ctgs, refs, pc, pr, cm, rm = world
    k = 7
    (c_prev, r_prev), (c_now, r_now) = long_step_ends(variant, L, k, cm, rm)
    tuples = [(5, cm.starts[0], rm.starts[0], 1, k), (77, c_prev, r_prev, 2, 3), (1234, c_now, r_now, 3, L)]
    want = seq_text.render(tuples, k, ctgs, refs, cm, rm, DEV, ERR)
    assert want is not None
    rc, need, got, guard_ok = seq_text.device_render(lib, dump_text.to_records(tuples), k, pc, pr, DEV, ERR)
    assert rc == capi.PAG_OK and need == len(want) == k + 3 + L and guard_ok
    assert first_difference(got, want) is None, f"{variant}: {first_difference(got, want)}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, TILE + 1, 3 * TILE + 5])
def test_buffer_one_byte_short_fails_and_writes_nothing(n, lib, world):
    """the utility knows the size from the records and refuses before any launch: this covers the call's contract, not the
    render kernel's own guard against a text larger than its buffer (only pag_travel's bound for a path's tail can reach that)"""
    ctgs, refs, pc, pr, cm, rm = world
    tuples, _ = constructed(n, 7, cm, rm, n)
    want = seq_text.render(tuples, 7, ctgs, refs, cm, rm, DEV, ERR)
    rc, need, got, guard_ok = seq_text.device_render(lib, dump_text.to_records(tuples), 7, pc, pr, DEV, ERR, cap=len(want) - 1)
    assert rc == capi.PAG_ERANGE
    assert need == len(want)
    assert guard_ok, "bytes behind the buffer were written"
    assert got == bytes([0xA5]) * (len(want) - 1), "a buffer that cannot take the text must be left alone"
    rc, need, got, guard_ok = seq_text.device_render(lib, dump_text.to_records(tuples), 7, pc, pr, DEV, ERR, cap=len(want))
    assert rc == capi.PAG_OK and got == want and guard_ok


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, TILE + 40])
def test_a_line_that_dips_below_zero_is_not_renderable(n, lib, world):
    """the reference coordinate 5 lies before the first start: singleToDual gives it a negative offset, the step's line runs
    down to it and its rounded positions turn negative — the host's cast of those is undefined, the device reports the path
    and writes nothing"""
    ctgs, refs, pc, pr, cm, rm = world
    k = 7
    tuples, _ = constructed(n, k, cm, rm, n)
    tuples = list(tuples)
    at = n - 1
    tuples[at - 1] = tuples[at - 1][:1] + (0, rm.starts[0] + 1) + tuples[at - 1][3:]
    tuples[at] = tuples[at][:1] + (0, 5, 9, 400)
    assert seq_text.render(tuples, k, ctgs, refs, cm, rm, DEV, ERR) is None
    cap = seq_text.expected_bytes(tuples, k)
    rc, need, got, guard_ok = seq_text.device_render(lib, dump_text.to_records(tuples), k, pc, pr, DEV, ERR, cap=cap)
    assert rc == capi.PAG_EDOM, f"rc {rc}"
    assert need == cap and guard_ok
    assert got == bytes([0xA5]) * cap, "nothing of a path that is not renderable may be written"
    # ... and the same records without that step render
    tuples[at] = tuples[at][:4] + (3,)
    want = seq_text.render(tuples, k, ctgs, refs, cm, rm, DEV, ERR)
    rc, need, got, guard_ok = seq_text.device_render(lib, dump_text.to_records(tuples), k, pc, pr, DEV, ERR)
    assert rc == capi.PAG_OK and got == want and guard_ok


# ---- 3. pag_travel with PAG_TRAVEL_RENDER_SEQS on every golden

def block_orientations(name, n_ctgs):
    """{block: PAG_ORIENT_* per contig} from the golden's dump files (<block>_<contig>_<0 forward | 1 reverse>.txt)"""
    out = {}
    for f in dump_text.golden_dumps(name):
        block, ctg, rev = (int(x) for x in f[:-len(".txt")].split("_"))
        o = out.setdefault(block, np.full(n_ctgs, capi.PAG_ORIENT_NONE, dtype=np.int32))
        mine = capi.PAG_ORIENT_REVERSE if rev else capi.PAG_ORIENT_FORWARD
        o[ctg] = mine if o[ctg] in (capi.PAG_ORIENT_NONE, mine) else capi.PAG_ORIENT_BOTH
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", goldens.case_names())
def test_pag_travel_renders_the_sequence_of_every_path(name, workdir):
    hip = pagctl.hip_lib()
    ctgs, refs, pc, pr, cm, rm = case(name, workdir)
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / "devseq" / "travel" / name))
    ref_len = np.array([len(s) for s in refs], dtype=np.uint32)
    n_paths = 0
    for block, orient in sorted(block_orientations(name, len(ctgs)).items()):
        inp = pagctl.LoadedInput(ind, threads=spec["threads"], eps=spec["epsilon"], cov=spec["cov"], block=block)
        g = pagctl.hip_create(inp)
        try:
            pagctl.run_on(g, inp)
            k = inp.k
            for flag in (capi.PAG_TRAVEL_RENDER_SEQS, 0, capi.PAG_TRAVEL_RENDER_SEQS | capi.PAG_TRAVEL_RENDER_DUMPS):
                prm = capi.TravelParams(spec["threads"], flag, 2 * spec["epsilon"], ERR, 0.90, 50)
                assert hip.pag_travel_seq_sources(g, C.byref(pr.c)) == capi.PAG_OK
                rc = hip.pag_travel(g, C.byref(pc.c), orient.ctypes.data, ref_len.ctypes.data, len(ref_len), C.byref(prm), None)
                assert rc == capi.PAG_OK, hip.pag_last_error()
                for c in range(len(ctgs)):
                    for fwd in (1, 0):
                        n, nb = C.c_uint64(), C.c_uint64(7)
                        p = hip.pag_travel_path_oriented(g, c, fwd, C.byref(n))
                        t = hip.pag_travel_seq_text(g, c, fwd, C.byref(nb))
                        if not flag or not p or n.value == 0:
                            assert t is None and nb.value == 0
                            continue
                        records = np.frombuffer(C.string_at(p, n.value * 24), dtype=dump_text.NODE)
                        want = seq_text.render(records, k, ctgs, refs, cm, rm, 2 * spec["epsilon"])
                        assert want is not None, "the goldens hold no path that is not renderable"
                        assert t is not None, f"{name} block {block} contig {c} forward {fwd}: no text for a path of {n.value} vertices"
                        got = C.string_at(t, nb.value)
                        assert first_difference(got, want) is None, f"{name} block {block} contig {c} forward {fwd}: {first_difference(got, want)}"
                        n_paths += 1
            # the flag without the sources: nothing is rendered, and it is no error
            prm = capi.TravelParams(spec["threads"], capi.PAG_TRAVEL_RENDER_SEQS, 2 * spec["epsilon"], ERR, 0.90, 50)
            assert hip.pag_travel(g, C.byref(pc.c), orient.ctypes.data, ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == capi.PAG_OK
            assert all(hip.pag_travel_seq_text(g, c, fwd, None) is None for c in range(len(ctgs)) for fwd in (1, 0))
        finally:
            hip.pag_destroy(g)
            inp.close()
    assert n_paths > 0


# ---- 4. bin/pagraph with PAGRAPH_DEVICE_SEQS=1

TIMING_LINE = re.compile(r"chain pieces: device-rendered (\d+) (\d+); host-rendered (\d+) (\d+); render")


def rendered(stderr):
    """sums over the "[timing] chain pieces" lines of a run: device pieces, device bases, host pieces, host bases, lines seen"""
    tot = [0, 0, 0, 0, 0]
    for m in TIMING_LINE.finditer(stderr):
        for i in range(4):
            tot[i] += int(m.group(i + 1))
        tot[4] += 1
    return tot


_want_cache = {}


def fasta_pieces_and_bases(name, workdir):
    """pieces and bases of a golden's chains — after the restatement has said that every one of them is renderable"""
    if name not in _want_cache:
        n_pieces = n_bases = 0
        if name in seq_text.fasta_cases():
            ctgs, refs, _, _, cm, rm = case(name, workdir)
            for body, pieces in seq_text.golden_pieces(name).values():
                for _, k, records in pieces:
                    assert seq_text.render(records, k, ctgs, refs, cm, rm, seq_text.deviation_of(name)) is not None
                n_pieces += len(pieces)
                n_bases += len(body)
        _want_cache[name] = (n_pieces, n_bases)
    return _want_cache[name]


def walk_env(mode=None, **extra):
    env = dict(os.environ)
    for v in ("PAG_WALK_EXACT", "PAG_SEG_LEN", "PAG_SEG_OVERLAP", "PAG_SEG_SAFETY", "PAG_WALK_PIECES", "PAG_LEAP_PIECES", "PAGRAPH_DEVICE_DUMPS",
              "PAGRAPH_DEVICE_SEQS", "PAG_DEBUG_DELIVER_LATE", "PAG_VIEW_HALO", "PAG_VIEW_MARGIN", "PAG_TRAVEL_VIEW"):
        env.pop(v, None)
    if mode == "pieces":  # (the environment tests/test_gpu_cli.py runs that mode with)
        env.update(PAG_SEG_LEN="400", PAG_SEG_OVERLAP="150", PAG_SEG_SAFETY="200", PAG_DEBUG_CHECK_AGGS="1")
    if mode == "exact":
        env["PAG_WALK_EXACT"] = "1"
    env["PAGRAPH_TIMING"] = "1"
    env.update(extra)
    return env


def run_case(name, workdir, tag, env, times=1):
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / "devseq" / tag / name / "in"))
    if times > 1:
        goldens.repeat_config(ind, times)
    out = str(workdir / "devseq" / tag / name / "out")
    os.makedirs(out, exist_ok=True)
    argv = synth.pagraph_argv(EXE, ind, out, threads=spec["threads"], epsilon=spec["epsilon"], cov=spec["cov"])
    r = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    return out, r.stderr


def all_from_the_device(name, workdir, err, times=1):
    """every piece and every FASTA base device-rendered and ZERO host-rendered: the fallback must not carry the test"""
    n_pieces, n_bases = fasta_pieces_and_bases(name, workdir)
    got = rendered(err)
    assert got[4] >= 1, err[-1500:]
    assert got[:4] == [times * n_pieces, times * n_bases, 0, 0], err[-1500:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["speculative", "pieces", "exact"])
@pytest.mark.parametrize("name", goldens.case_names())
def test_pagraph_with_device_seqs_matches_golden(name, mode, workdir):
    out, err = run_case(name, workdir, "e2e_" + mode, walk_env(mode, PAGRAPH_DEVICE_SEQS="1"))
    goldens.compare_out_dir(name, out)
    all_from_the_device(name, workdir, err)


@pytest.mark.gpu
def test_device_seqs_in_the_overlapped_and_the_serial_schedule(workdir):
    """four blocks (the two-block golden written twice over): the host half of block b puts the chains together from the
    device's text while block b + 1 is built and prepared; then one block after the other"""
    name = "two_blocks_both_orient_t16"
    for tag, on in (("overlap", "1"), ("serial", "0")):
        out, err = run_case(name, workdir, tag, walk_env(PAGRAPH_DEVICE_SEQS="1", PAGRAPH_OVERLAP=on, PAGRAPH_PREFETCH=on), times=2)
        goldens.compare_repeated_blocks(name, out, 4)
        all_from_the_device(name, workdir, err, times=2)
        assert rendered(err)[4] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_fwd_t1", "two_blocks_both_orient_t16"])
def test_device_seqs_are_those_of_the_walk_again(name, workdir):
    """without halo and margin a walk leaves the cut view and pag_travel walks again on the whole graph: the text handed out is
    the final walk's, and the references' bases are still there for it"""
    out, err = run_case(name, workdir, "again", walk_env(PAGRAPH_DEVICE_SEQS="1", PAG_VIEW_HALO="0", PAG_VIEW_MARGIN="0"))
    assert err.count("a walk left the view") > 0, "the walk-again path did not run"
    goldens.compare_out_dir(name, out)
    all_from_the_device(name, workdir, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_fwd_t1", "three_ctg_multi_t4", "two_blocks_both_orient_t16"])
def test_device_seqs_rendered_in_the_epilogue(name, workdir):
    """PAG_DEBUG_DELIVER_LATE=1: no contig is delivered while the walks run, every text is rendered behind the epilogue's gather"""
    out, err = run_case(name, workdir, "late", walk_env(PAGRAPH_DEVICE_SEQS="1", PAG_DEBUG_DELIVER_LATE="1"))
    goldens.compare_out_dir(name, out)
    all_from_the_device(name, workdir, err)
    n_text = n_epi = 0
    for m in re.finditer(r"sequence text: (\d+) paths rendered \((\d+) of them in the epilogue\), (\d+) left to the host", err):
        n_text += int(m.group(1))
        n_epi += int(m.group(2))
        assert int(m.group(3)) == 0
    assert n_text > 0 and n_epi == n_text, err[-1500:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_rev_t16", "two_blocks_both_orient_t16"])
def test_both_device_switches_together(name, workdir):
    out, err = run_case(name, workdir, "both", walk_env(PAGRAPH_DEVICE_SEQS="1", PAGRAPH_DEVICE_DUMPS="1"))
    goldens.compare_out_dir(name, out)
    all_from_the_device(name, workdir, err)
    dumps = dump_text.golden_dumps(name)
    m = [re.search(r"path dumps: device-rendered (\d+) bytes (\d+) vertices; host-rendered (\d+) contigs", ln) for ln in err.splitlines()]
    m = [x for x in m if x]
    assert sum(int(x.group(1)) for x in m) == sum(len(ln) for _, body in dumps.values() for ln in body)
    assert sum(int(x.group(3)) for x in m) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_fwd_t1", "three_ctg_multi_t4"])
def test_both_device_switches_rendered_in_the_epilogue(name, workdir):
    """both switches and PAG_DEBUG_DELIVER_LATE=1: the epilogue carves ONE scratch buffer for the dump and the sequence of every
    contig, and renders both texts of every path behind its gather"""
    out, err = run_case(name, workdir, "both_late", walk_env(PAGRAPH_DEVICE_SEQS="1", PAGRAPH_DEVICE_DUMPS="1", PAG_DEBUG_DELIVER_LATE="1"))
    goldens.compare_out_dir(name, out)
    for what in (r"dump text: (\d+) contigs", r"sequence text: (\d+) paths"):
        n_text = n_epi = 0
        for m in re.finditer(what + r" rendered \((\d+) of them in the epilogue\), (\d+) left to the host", err):
            n_text += int(m.group(1))
            n_epi += int(m.group(2))
            assert int(m.group(3)) == 0
        assert n_text > 0 and n_epi == n_text, err[-1500:]
    all_from_the_device(name, workdir, err)  # (chain pieces: nothing host-rendered)
    dumps = dump_text.golden_dumps(name)
    m = [re.search(r"path dumps: device-rendered (\d+) bytes (\d+) vertices; host-rendered (\d+) contigs", ln) for ln in err.splitlines()]
    m = [x for x in m if x]
    assert sum(int(x.group(1)) for x in m) == sum(len(ln) for _, body in dumps.values() for ln in body)
    assert sum(int(x.group(3)) for x in m) == 0


@pytest.mark.gpu
def test_device_seqs_switch_is_harmless_in_a_sharded_run(workdir):
    """PAGRAPH_SHARD: rank 0 builds the chains from the gathered paths of both ranks and renders their pieces on the host; the
    switch changes nothing there (set up as tests/test_gpu_cli.py::test_one_block_built_by_several_pagraph_processes)"""
    name, world = "three_ctg_multi_t4", 2
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / "devseq" / "shard" / "in"))
    out = str(workdir / "devseq" / "shard" / "out")
    os.makedirs(out, exist_ok=True)
    argv = synth.pagraph_argv(EXE, ind, out, threads=spec["threads"], epsilon=spec["epsilon"], cov=spec["cov"])
    rdv = tempfile.mkdtemp(prefix="pagshard_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    procs = []
    for r in range(world):
        env = walk_env(PAGRAPH_DEVICE_SEQS="1", PAGRAPH_SHARD=f"{r}/{world}", PAGRAPH_SHARD_DIR=rdv, PAGRAPH_SHARD_TRANSPORT="host",
                       PAG_COMM_TIMEOUT_S="120", PAG_DEVICE_SHARERS=str(world))
        procs.append(subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    for r, pr in enumerate(procs):
        so, se = pr.communicate(timeout=300)
        assert pr.returncode == 0, f"rank {r}: " + se[-2000:] + so[-1000:]
    goldens.compare_out_dir(name, out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_rev_t16"])
def test_default_run_renders_on_the_host(name, workdir):
    """the variable unset (and set to something other than 1): the golden bytes, every piece from seqToString"""
    n_pieces, n_bases = fasta_pieces_and_bases(name, workdir)
    for tag, extra in (("unset", {}), ("zero", {"PAGRAPH_DEVICE_SEQS": "0"})):
        out, err = run_case(name, workdir, "default_" + tag, walk_env(**extra))
        goldens.compare_out_dir(name, out)
        assert rendered(err)[:4] == [0, 0, n_pieces, n_bases], err[-1500:]
        assert "sequence text:" not in err
