"""CPU: where one owner's records land when a serial-rank run gathers them from several extractions
(aligngraph2_amd/csrc/hip/serial_layout.hpp, used by pag_shard_run_serial), through tests/harness/serial_layout_test.cpp.

counts[r][o] = (tuples pass 1, tuples pass 2, edges pass 1, edges pass 2) that read range r sends owner o.  The expected
values are a second restatement, written here from the definition in include/pagraph_hip.h (pag_shard_*): an owner builds from
[pass 1 from range 0] .. [pass 1 from range N-1] [pass 2 from range 0] ..; a range's partitioned stream is, owners ascending,
[its pass-1 records][its pass-2 records].  The same cases run once more as a program of its own under the address and
undefined-behaviour sanitizers (tests/harness/serial_layout_main.cpp: host code, nothing loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "harness", "bin", "libpagh_serial_layout_test.so")
SANITIZED = os.path.join(ROOT, "tests", "harness", "bin", "serial_layout_sanitized")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, LIB[len(ROOT) + 1:]], check=True, capture_output=True)
    L = C.CDLL(LIB)
    P, u32 = C.c_void_p, C.c_uint32
    L.pagt_owner_layout.argtypes = [P, u32, u32, P]
    L.pagt_range_slots.argtypes = [P, u32, u32, u32, P]
    L.pagt_partitioned_slots.argtypes = [P, u32, u32, u32, P]
    return L


def expected(counts):
    """{(o, r): (owner sizes, slots in the owner's buffers, slots in range r's partitioned streams)} by cumulative sums"""
    n = counts.shape[0]
    out = {}
    for o in range(n):
        t1, t2 = int(counts[:, o, 0].sum()), int(counts[:, o, 1].sum())
        e1, e2 = int(counts[:, o, 2].sum()), int(counts[:, o, 3].sum())
        for r in range(n):
            slots = (int(counts[:r, o, 0].sum()), t1 + int(counts[:r, o, 1].sum()), int(counts[:r, o, 2].sum()), e1 + int(counts[:r, o, 3].sum()))
            tb, eb = int(counts[r, :o, 0:2].sum()), int(counts[r, :o, 2:4].sum())
            part = (tb, tb + int(counts[r, o, 0]), eb, eb + int(counts[r, o, 2]))
            out[(o, r)] = ((t1 + t2, t1, e1 + e2, e1), slots, part)
    return out


def cases(n):
    rng = np.random.default_rng(100 + n)
    yield "nothing", np.zeros((n, n, 4), dtype=np.uint64)
    for r in range(n):
        c = np.zeros((n, n, 4), dtype=np.uint64)
        c[r] = rng.integers(1, 1000, size=(n, 4))
        yield f"range {r} holds everything", c
    for o in range(n):
        c = np.zeros((n, n, 4), dtype=np.uint64)
        c[:, o] = rng.integers(1, 1000, size=(n, 4))
        yield f"owner {o} takes everything", c
    for rep in range(10):
        c = rng.integers(0, 50, size=(n, n, 4)).astype(np.uint64)
        c[rng.random((n, n, 4)) < 0.3] = 0
        yield f"random {rep}", c
    yield "beyond 32 bits", rng.integers(1 << 31, 1 << 33, size=(n, n, 4)).astype(np.uint64)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_slots_equal_the_cumulative_sums(lib, n):
    for label, counts in cases(n):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        want = expected(counts)
        got = (C.c_uint64 * 4)()
        for o in range(n):
            for r in range(n):
                sizes, slots, part = want[(o, r)]
                lib.pagt_owner_layout(counts.ctypes.data, n, o, got)
                assert tuple(got) == sizes, f"N = {n}, {label}: sizes of owner {o}"
                lib.pagt_range_slots(counts.ctypes.data, n, o, r, got)
                assert tuple(got) == slots, f"N = {n}, {label}: range {r}'s slots in owner {o}'s buffers"
                lib.pagt_partitioned_slots(counts.ctypes.data, n, o, r, got)
                assert tuple(got) == part, f"N = {n}, {label}: owner {o}'s stretches of range {r}'s partitioned streams"


@pytest.mark.parametrize("n", [2, 4, 8])
def test_stretches_tile_the_owner_buffers(lib, n):
    """the 2 N stretches of a stream tile the owner's buffer: none overlaps, nothing is left over"""
    rng = np.random.default_rng(7 * n)
    counts = np.ascontiguousarray(rng.integers(0, 30, size=(n, n, 4)), dtype=np.uint64)
    got = (C.c_uint64 * 4)()
    for o in range(n):
        lib.pagt_owner_layout(counts.ctypes.data, n, o, got)
        n_t, _, n_e, _ = tuple(got)
        for stream, total in ((0, n_t), (1, n_e)):
            seen = np.zeros(total, dtype=np.int32)
            for r in range(n):
                lib.pagt_range_slots(counts.ctypes.data, n, o, r, got)
                for ps in (0, 1):
                    at, c = got[2 * stream + ps], int(counts[r, o, 2 * stream + ps])
                    seen[at:at + c] += 1
            assert (seen == 1).all()


def test_the_same_cases_under_the_sanitizers():
    """a program of its own (its own main), built with -fsanitize=address,undefined and run as it is"""
    subprocess.run(["make", "-C", ROOT, SANITIZED[len(ROOT) + 1:]], check=True, capture_output=True)
    r = subprocess.run([SANITIZED], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
