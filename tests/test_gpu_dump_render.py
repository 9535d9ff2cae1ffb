"""GPU: the bodies of the per-contig path dumps rendered on the device (csrc/hip/k5_dump.hip) — records -> text through
pag_render_dump_lines against the golden dumps and, on constructed records, against the Python restatement that
tests/test_dump_render.py pins to those goldens; then bin/pagraph with PAGRAPH_DEVICE_DUMPS=1 on every route to a dump file."""
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
from aligngraph2_amd import capi
import synth

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pagraph")
TILE = 256  # lines per tile of the render kernels
I32_MIN, I32_MAX, U32_MAX = -(1 << 31), (1 << 31) - 1, (1 << 32) - 1


@pytest.fixture(scope="module")
def lib():
    return capi.bind(C.CDLL(pagctl.HIP_LIB))


def check(lib, tuples, k, ctg_len, ref_len, label):
    recs = dump_text.to_records(tuples)
    want = dump_text.render(recs, k, dump_text.Mapper(ctg_len), dump_text.Mapper(ref_len))
    rc, need, got, guard_ok = dump_text.device_render(lib, recs, k, ctg_len, ref_len)
    assert rc == dump_text.PAG_OK, f"{label}: rc {rc}"
    assert need == len(want), f"{label}: {need} bytes reported, the text has {len(want)}"
    assert guard_ok, f"{label}: bytes behind the buffer were written"
    if got != want:
        at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
        ln = want.count(b"\n", 0, at)
        raise AssertionError(f"{label}: first difference in line {ln}: {got[max(0, at - 60):at + 60]!r} != {want[max(0, at - 60):at + 60]!r}")


# ---- 1. the golden records: every file, every line

@pytest.mark.gpu
@pytest.mark.parametrize("name", dump_text.dump_cases())
def test_device_renders_every_golden_dump_from_its_records(name, lib, workdir):
    ctg_len, ref_len = dump_text.case_lengths(name, workdir)
    n_files = 0
    for f, (header, body) in dump_text.golden_dumps(name).items():
        if not body:
            continue
        parsed = [dump_text.parse_line(ln) for ln in body]
        k = parsed[0][0]
        assert all(p[0] == k for p in parsed)
        rc, need, got, guard_ok = dump_text.device_render(lib, dump_text.to_records([p[1] for p in parsed]), k, ctg_len, ref_len)
        assert rc == dump_text.PAG_OK and guard_ok
        assert got == "".join(body).encode(), f"{name}/{f}"
        n_files += 1
    assert n_files > 0


# ---- 2. constructed records against the restatement

def digit_boundaries():
    v = [0, 1]
    for d in range(1, 10):
        v += [10 ** d - 1, 10 ** d]
    return v + [U32_MAX - 1, U32_MAX]


# one contig / one reference whose coordinate space ends exactly at 2^32 - 1 (5 * 858993459): every u32 is a coordinate of it or lies
# before its first start (a wrapped, negative offset) or at its very end (index -(n + 1))
WIDE = [858993459]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 17))
def test_every_k(k, lib):
    rng = np.random.default_rng(k)
    codes = [0, (1 << (2 * k)) - 1, 1, 1 << (2 * k - 2)] + [int(x) for x in rng.integers(0, 1 << (2 * k), 60)]
    tuples = [(c, 1000 + 7 * i, 2000 + 3 * i, i, k if i == 0 else i) for i, c in enumerate(codes)]
    check(lib, tuples, k, [5000, 300], [4000], f"k = {k}")


@pytest.mark.gpu
def test_digit_boundaries_counts_and_steps(lib):
    vals = digit_boundaries()
    tuples = []
    for i, v in enumerate(vals):
        tuples.append((i, v, vals[-1 - i], 0, 5))        # ctg at a boundary, ref at the mirrored one
        tuples.append((i, vals[-1 - i], v, 65535, -1))
    for cnt in (0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535):
        tuples.append((3, 858993459, 858993460, cnt, 0))
    for step in (0, -1, 1, 9, 10, -9, -10, -99, -100, I32_MIN, I32_MAX, I32_MIN + 1, 999999999, 1000000000, -999999999, -1000000000):
        tuples.append((2, 900000000, 900000001, 12, step))
    tuples += [(1, 0, 0, 1, 1), (1, 0, 858993459, 1, 1), (1, 858993459, 0, 1, 1)]  # no coordinate on either side
    check(lib, tuples, 16, WIDE, WIDE, "digit boundaries")
    check(lib, tuples, 1, WIDE, [1000, 2000, 3000], "digit boundaries, small reference space")


def strand_corners(sizes):
    """single coordinates of the first and last base of every forward and reverse strand, the gaps around them, the end"""
    m = dump_text.Mapper(sizes)
    out = []
    for i, sz in enumerate(sizes):
        s = m.starts[i]
        out += [s, s + sz - 1, s + sz, s + 2 * sz - 1, s + 2 * sz, s + 3 * sz - 1, s + 3 * sz, m.starts[i + 1] - 1]
    out += [m.starts[0] - 1, 1, m.extra_start(), m.extra_start() + 1]
    return [x for x in out if 0 <= x <= U32_MAX]


@pytest.mark.gpu
@pytest.mark.parametrize("n_ctgs,n_refs", [(1, 1), (3, 2), (5056, 24), (6000, 24), (6000, 7000)])
def test_strand_corners_of_every_sequence(n_ctgs, n_refs, lib):
    """... the last contig and the last reference among them; 5 056 contigs and 24 references (BASELINE configs[3]) is the
    largest table pair the kernels keep in LDS, 6 000 contigs read their starts from global memory"""
    rng = np.random.default_rng(n_ctgs)
    ctg_len = [int(x) for x in rng.integers(1, 3000, n_ctgs)]
    ref_len = [int(x) for x in rng.integers(1, 90000, n_refs)]
    cc, rc = strand_corners(ctg_len), strand_corners(ref_len)
    n = max(len(cc), len(rc))
    tuples = [(i & 0xFFFF, cc[i % len(cc)], rc[(7 * i) % len(rc)], i & 0xFFFF, (i % 19) - 3) for i in range(n)]
    check(lib, tuples, 8, ctg_len, ref_len, f"{n_ctgs} contigs, {n_refs} references")


def random_records(rng, n, k, ctg_space, ref_space):
    """random field widths: every number's digit count is drawn first, so that line lengths vary from record to record"""
    def widths(hi, size):
        d = rng.integers(1, len(str(hi)) + 1, size)
        return np.minimum((rng.random(size) * (10.0 ** d)).astype(np.uint64), hi)
    a = np.zeros(n, dtype=dump_text.NODE)
    a["code"] = rng.integers(0, 1 << (2 * k), n, dtype=np.uint64)
    a["ctg"] = widths(ctg_space, n)
    a["ref"] = widths(ref_space, n)
    a["cnt"] = widths(65535, n)
    a["step"] = (widths(I32_MAX, n).astype(np.int64) * rng.choice([1, 1, 1, -1], n)).astype(np.int32)
    a["vid"] = np.arange(n, dtype=np.uint32)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 5 * TILE + 17])
def test_record_counts_around_wave_and_tile_edges(n, lib):
    rng = np.random.default_rng(1000 + n)
    ctg_len, ref_len = [70000, 1234, 99], [500000, 42]
    recs = random_records(rng, n, 11, dump_text.Mapper(ctg_len).extra_start(), dump_text.Mapper(ref_len).extra_start())
    want = dump_text.render(recs, 11, dump_text.Mapper(ctg_len), dump_text.Mapper(ref_len))
    rc, need, got, guard_ok = dump_text.device_render(lib, recs, 11, ctg_len, ref_len)
    assert rc == dump_text.PAG_OK and need == len(want) and guard_ok
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_ctgs", [(300000, 40), (200000, 6000)])
def test_many_records_with_random_line_lengths(n, n_ctgs, lib):
    """a few hundred thousand lines whose lengths vary at random: every tile's offset in the output is unaligned somewhere"""
    rng = np.random.default_rng(n)
    ctg_len = [int(x) for x in rng.integers(50, 200000, n_ctgs)]
    ref_len = [int(x) for x in rng.integers(1000, 3000000, 24)]
    cm, rm = dump_text.Mapper(ctg_len), dump_text.Mapper(ref_len)
    recs = random_records(rng, n, 14, cm.extra_start() + 1000, rm.extra_start() + 1000)
    want = dump_text.render(recs, 14, cm, rm)
    lens = np.diff(np.flatnonzero(np.frombuffer(want, dtype=np.uint8) == 10), prepend=-1)
    assert len(lens) == n and lens.min() < 35 and lens.max() > 70
    offs = np.cumsum(lens)[TILE - 1::TILE]
    assert len(set(int(x) & 15 for x in offs)) == 16  # tile offsets of every alignment
    rc, need, got, guard_ok = dump_text.device_render(lib, recs, 14, ctg_len, ref_len)
    assert rc == dump_text.PAG_OK and need == len(want) and guard_ok
    if got != want:
        at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i])
        raise AssertionError(f"first difference at byte {at} (line {want.count(bytes([10]), 0, at)}): {got[at - 50:at + 50]!r} != {want[at - 50:at + 50]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, TILE + 3, 4000])
def test_buffer_one_byte_short_fails_and_writes_nothing(n, lib):
    rng = np.random.default_rng(n)
    ctg_len, ref_len = [70000, 1234], [500000]
    recs = random_records(rng, n, 9, 300000, 2000000)
    want = dump_text.render(recs, 9, dump_text.Mapper(ctg_len), dump_text.Mapper(ref_len))
    rc, need, got, guard_ok = dump_text.device_render(lib, recs, 9, ctg_len, ref_len, cap=len(want) - 1)
    assert rc == dump_text.PAG_ERANGE
    assert need == len(want)
    assert guard_ok, "bytes behind the buffer were written"
    assert got == bytes([0xA5]) * (len(want) - 1), "a buffer that cannot take the text must be left alone"
    rc, need, got, guard_ok = dump_text.device_render(lib, recs, 9, ctg_len, ref_len, cap=len(want))
    assert rc == dump_text.PAG_OK and got == want and guard_ok


# ---- 3.-5. bin/pagraph with PAGRAPH_DEVICE_DUMPS=1

TIMING_LINE = re.compile(r"path dumps: device-rendered (\d+) bytes (\d+) vertices; host-rendered (\d+) contigs (\d+) vertices")


def rendered(stderr):
    """sums over the "[timing] path dumps" lines of a run: device bytes, device vertices, host contigs, lines seen"""
    tot = [0, 0, 0, 0]
    for m in TIMING_LINE.finditer(stderr):
        tot[0] += int(m.group(1))
        tot[1] += int(m.group(2))
        tot[2] += int(m.group(3))
        tot[3] += 1
    return tot


def dump_body_bytes(name):
    """total size of the bodies of a golden's dump files, and their lines"""
    d = dump_text.golden_dumps(name)
    return sum(len(ln) for _, body in d.values() for ln in body), sum(len(body) for _, body in d.values())


def walk_env(mode=None, **extra):
    env = dict(os.environ)
    for v in ("PAG_WALK_EXACT", "PAG_SEG_LEN", "PAG_SEG_OVERLAP", "PAG_SEG_SAFETY", "PAG_WALK_PIECES", "PAG_LEAP_PIECES", "PAGRAPH_DEVICE_DUMPS",
              "PAG_DEBUG_DELIVER_LATE", "PAG_VIEW_HALO", "PAG_VIEW_MARGIN", "PAG_TRAVEL_VIEW"):
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
    ind = goldens.materialize_inputs(name, str(workdir / "devdump" / tag / name / "in"))
    if times > 1:
        goldens.repeat_config(ind, times)
    out = str(workdir / "devdump" / tag / name / "out")
    os.makedirs(out, exist_ok=True)
    argv = synth.pagraph_argv(EXE, ind, out, threads=spec["threads"], epsilon=spec["epsilon"], cov=spec["cov"])
    r = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    return out, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["speculative", "pieces", "exact"])
@pytest.mark.parametrize("name", goldens.case_names())
def test_pagraph_with_device_dumps_matches_golden(name, mode, workdir):
    out, err = run_case(name, workdir, "e2e_" + mode, walk_env(mode, PAGRAPH_DEVICE_DUMPS="1"))
    goldens.compare_out_dir(name, out)
    dev_bytes, dev_vertices, host_contigs, n_lines = rendered(err)
    want_bytes, want_lines = dump_body_bytes(name)
    assert n_lines >= 1, err[-1500:]
    # the device path ran, not the host one: every byte of every body came from the device, no contig fell back (the arena of
    # these few-kb contigs has room for all of them)
    assert (dev_bytes, dev_vertices, host_contigs) == (want_bytes, want_lines, 0), err[-1500:]


@pytest.mark.gpu
def test_device_dumps_in_the_overlapped_schedule(workdir):
    """four blocks (the two-block golden written twice over), the host half of block b writing the device's text while block
    b + 1 is built and prepared"""
    name = "two_blocks_both_orient_t16"
    out, err = run_case(name, workdir, "overlap", walk_env(PAGRAPH_DEVICE_DUMPS="1", PAGRAPH_OVERLAP="1", PAGRAPH_PREFETCH="1"), times=2)
    goldens.compare_repeated_blocks(name, out, 4)
    want_bytes, want_lines = dump_body_bytes(name)
    assert rendered(err) == [2 * want_bytes, 2 * want_lines, 0, 4], err[-1500:]
    # ... and one block after the other
    out, err = run_case(name, workdir, "serial", walk_env(PAGRAPH_DEVICE_DUMPS="1", PAGRAPH_OVERLAP="0", PAGRAPH_PREFETCH="0"), times=2)
    goldens.compare_repeated_blocks(name, out, 4)
    assert rendered(err) == [2 * want_bytes, 2 * want_lines, 0, 4], err[-1500:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_fwd_t1", "two_blocks_both_orient_t16"])
def test_device_dumps_are_those_of_the_walk_again(name, workdir):
    """without halo and margin a walk leaves the cut view and pag_travel walks again on the whole graph (tests/test_gpu_cli.py):
    the text handed out is the final walk's"""
    out, err = run_case(name, workdir, "again", walk_env(PAGRAPH_DEVICE_DUMPS="1", PAG_VIEW_HALO="0", PAG_VIEW_MARGIN="0"))
    assert err.count("a walk left the view") > 0, "the walk-again path did not run"
    goldens.compare_out_dir(name, out)
    want_bytes, want_lines = dump_body_bytes(name)
    assert rendered(err)[:3] == [want_bytes, want_lines, 0], err[-1500:]


@pytest.mark.gpu
def test_device_dumps_of_a_block_built_by_two_processes(workdir):
    """PAGRAPH_SHARD: every rank writes the dumps of the contigs it walked, from the text its own pag_travel rendered (set up
    as tests/test_gpu_cli.py::test_one_block_built_by_several_pagraph_processes)"""
    name, world = "three_ctg_multi_t4", 2
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / "devdump" / "shard" / "in"))
    out = str(workdir / "devdump" / "shard" / "out")
    os.makedirs(out, exist_ok=True)
    argv = synth.pagraph_argv(EXE, ind, out, threads=spec["threads"], epsilon=spec["epsilon"], cov=spec["cov"])
    rdv = tempfile.mkdtemp(prefix="pagshard_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    procs = []
    for r in range(world):
        env = walk_env(PAGRAPH_DEVICE_DUMPS="1", PAGRAPH_SHARD=f"{r}/{world}", PAGRAPH_SHARD_DIR=rdv, PAGRAPH_SHARD_TRANSPORT="host",
                       PAG_COMM_TIMEOUT_S="120", PAG_DEVICE_SHARERS=str(world))
        procs.append(subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    tot = [0, 0, 0]
    per_rank = []
    for r, pr in enumerate(procs):
        so, se = pr.communicate(timeout=300)
        assert pr.returncode == 0, f"rank {r}: " + se[-2000:] + so[-1000:]
        got = rendered(se)
        per_rank.append(got)
        tot = [a + b for a, b in zip(tot, got[:3])]
    goldens.compare_out_dir(name, out)
    want_bytes, want_lines = dump_body_bytes(name)
    assert tot == [want_bytes, want_lines, 0], per_rank
    assert all(g[0] > 0 for g in per_rank), per_rank  # both ranks walked contigs and wrote their text


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_fwd_t1", "three_ctg_multi_t4", "two_blocks_both_orient_t16"])
def test_device_dumps_rendered_in_the_epilogue(name, workdir):
    """A delivery is left to pag_travel's epilogue when the walk arena has no room for it, which neither a caller of pag_travel
    nor the environment of bin/pagraph can bring about on these few-kb contigs.  PAG_DEBUG_DELIVER_LATE=1 is the test switch
    for it: no contig is delivered while the walks run and every text is rendered behind the epilogue's gather."""
    out, err = run_case(name, workdir, "late", walk_env(PAGRAPH_DEVICE_DUMPS="1", PAG_DEBUG_DELIVER_LATE="1"))
    goldens.compare_out_dir(name, out)
    want_bytes, want_lines = dump_body_bytes(name)
    assert rendered(err)[:3] == [want_bytes, want_lines, 0], err[-1500:]
    n_text = n_epi = 0
    for m in re.finditer(r"dump text: (\d+) contigs rendered \((\d+) of them in the epilogue\), (\d+) left to the host", err):
        n_text += int(m.group(1))
        n_epi += int(m.group(2))
        assert int(m.group(3)) == 0
    assert n_text > 0 and n_epi == n_text, err[-1500:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join_rev_t16", "two_blocks_both_orient_t16"])
def test_default_run_renders_on_the_host(name, workdir):
    """the variable unset (and set to something other than 1): the golden bytes, and the timing line reports nothing from the device"""
    for tag, extra in (("unset", {}), ("zero", {"PAGRAPH_DEVICE_DUMPS": "0"})):
        out, err = run_case(name, workdir, "default_" + tag, walk_env(**extra))
        goldens.compare_out_dir(name, out)
        dev_bytes, dev_vertices, host_contigs, n_lines = rendered(err)
        want_bytes, want_lines = dump_body_bytes(name)
        assert n_lines >= 1 and (dev_bytes, dev_vertices) == (0, 0) and host_contigs > 0, err[-1500:]
        assert "dump text:" not in err
        host_vertices = sum(int(m.group(4)) for m in TIMING_LINE.finditer(err))
        assert host_vertices == want_lines
