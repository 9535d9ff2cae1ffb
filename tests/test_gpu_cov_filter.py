"""GPU: the read->reference coverage filter alone (cov_mark / cov_count_low / cov_flag behind launch_cov_filter,
csrc/hip/util.hip; entry pag_debug_cov_filter) against its DEFINITION in numpy (prep_cases.numpy_cov_verdicts): coverage per
base from every record with a known target, np.sort, verdict = max(sorted[t_begin:t_end]) >= F, an empty interval passes only at
F = 0 (Aligner.cpp:58-88, Aligner.tcc:140-149, quirk Q3) — not the kernel's shortcut through nLow = #{bases with coverage < F}.

Shapes around SCAN_TILE (4096 bases per block of cov_count_low): one reference of 1, 4095, 4096, 4097, 12 289 bases; three
references [4097, 1000, 4096] with the first accepted (its slice of the difference array is 16-byte aligned: the scan's vector
loads), the third (its slice starts at word 5 099: the scalar loads) and all three.  Records per reference: random intervals,
[0, len), [0, 1), [len - 1, len), empty ones, records without a query (they count), records without a target (they do not),
intervals that begin in one tile and end in a later one (a tile with more ends than beginnings: its sum wraps), and a probe
[e - 1, e) for every e — so that for every F with 0 < nLow < len compared records sit at t_end - 1 = nLow - 1 and = nLow, where
the verdict turns.  Every record keeps the entry's precondition t_begin <= t_end <= len.

Wall time: not measured on an MI355X yet; on the CPU, making a shape's records
and its numpy verdicts for all F takes under 0.1 s, and a shape has at most 14 727 records and 13 launches of the filter.
"""

import numpy as np
import pytest

import pagctl
import prep_cases
from aligngraph2_amd.workload import ALN_DTYPE, PAG_NONE, REF_DTYPE

SCAN_TILE = 4096
GUARD = 64

SHAPES = {
    "len1": ([1], [1]),
    "len4095": ([4095], [1]),
    "len4096": ([4096], [1]),
    "len4097": ([4097], [1]),
    "len12289": ([12289], [1]),
    "three_first": ([4097, 1000, 4096], [1, 0, 0]),
    "three_third": ([4097, 1000, 4096], [0, 0, 1]),
    "three_all": ([4097, 1000, 4096], [1, 1, 1]),
}


def make_records(lens, seed):
    rng = np.random.default_rng(seed)
    rows = []  # (query, target, t_begin, t_end)
    for r, L in enumerate(lens):
        iv = []
        n_rand = 1500 if L > 1 else 40
        b = rng.integers(0, L, n_rand)
        long_ = rng.random(n_rand) < 0.5
        e = np.where(long_, rng.integers(b, L + 1), np.minimum(L, b + rng.integers(0, 65, n_rand)))
        iv += list(zip(b.tolist(), e.tolist()))
        iv += [(0, L), (0, 1), (L - 1, L), (0, 0), (L, L), (L // 2, L // 2)] * 3
        # begin in one tile of the scan, end in a later one
        for t in range(0, (L - 1) // SCAN_TILE):
            bb = rng.integers(t * SCAN_TILE, (t + 1) * SCAN_TILE, 300)
            ee = rng.integers((t + 1) * SCAN_TILE, L + 1, 300)
            iv += list(zip(bb.tolist(), ee.tolist()))
        iv += [(x - 1, x) for x in range(1, L + 1)]  # the probes
        q = np.where(rng.random(len(iv)) < 0.2, PAG_NONE, rng.integers(0, 1000, len(iv)))
        rows += [(int(qq), r, bb, ee) for qq, (bb, ee) in zip(q.tolist(), iv)]
        rows += [(int(rng.integers(0, 1000)), PAG_NONE, int(x), int(x) + 5) for x in rng.integers(0, max(1, L - 5), 20)]
    order = rng.permutation(len(rows))
    aln = np.zeros(len(rows), ALN_DTYPE)
    arr = np.array(rows, dtype=np.uint64)[order]
    for i, f in enumerate(("query", "target", "t_begin", "t_end")):
        aln[f] = arr[:, i].astype(np.uint32)
    return aln


def test_vectorised_definition_equals_the_loop():
    """prep_cases.numpy_cov_verdicts takes all the maxima at once (np.maximum.reduceat): the same as the definition record by
    record"""
    lens, acc = SHAPES["three_all"]
    aln = make_records(lens, 3)[:3000]
    refs = np.array([(n, a, 0, 0) for n, a in zip(lens, acc)], REF_DTYPE)
    for F in (0, 1, 300, 700):
        ok, sorted_cov = prep_cases.numpy_cov_verdicts(aln, refs, F)
        for i in range(len(aln)):
            t = int(aln["target"][i])
            if t == PAG_NONE:
                assert ok[i] == 0
                continue
            sl = sorted_cov[t][int(aln["t_begin"][i]):int(aln["t_end"][i])]
            assert ok[i] == ((int(sl.max()) if len(sl) else 0) >= F), (i, F)


def device_verdicts(aln, refs, F):
    lib = pagctl.hip_lib()
    ok = np.full(len(aln) + GUARD, 0x5A, np.uint8)
    rc = lib.pag_debug_cov_filter(aln.ctypes.data, len(aln), refs.ctypes.data, len(refs), F, ok.ctypes.data, 0)
    assert rc == 0, lib.pag_last_error()
    assert (ok[len(aln):] == 0x5A).all(), "bytes behind ok[n_aln] were written"
    return ok[:len(aln)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_cov_filter_equals_its_definition(shape):
    lens, acc = SHAPES[shape]
    aln = make_records(lens, 100 + len(shape))
    refs = np.array([(n, a, 0, 0) for n, a in zip(lens, acc)], REF_DTYPE)
    known = aln["target"] != PAG_NONE
    tgt = np.where(known, aln["target"], 0).astype(np.int64)
    assert (aln["t_begin"][known] <= aln["t_end"][known]).all() and (aln["t_end"][known] <= refs["len"][tgt[known]]).all()
    compared = known & (refs["accepted"][tgt] == 1)
    _, sorted_cov = prep_cases.numpy_cov_verdicts(aln, refs, 0)
    maxcov = max(int(sorted_cov[r].max()) for r in range(len(lens)) if acc[r])
    median = int(np.median(sorted_cov[int(np.flatnonzero(acc)[0])]))
    edge_seen = 0
    for F in sorted({0, 1, maxcov - 1, maxcov, maxcov + 1, 2 ** 31 + 5, median}):
        want, _ = prep_cases.numpy_cov_verdicts(aln, refs, F)
        got = device_verdicts(aln, refs, F)
        assert ((got == 0) | (got == 1)).all(), f"{shape} F={F}: a verdict byte is neither 0 nor 1"
        bad = np.flatnonzero(compared & (got != want))
        assert len(bad) == 0, (f"{shape} F={F}: {len(bad)} of {int(compared.sum())} verdicts differ, first: record {bad[0]} "
                               f"{aln[bad[0]][['query', 'target', 't_begin', 't_end']]} device {got[bad[0]]} definition {want[bad[0]]}")
        if F == 0:
            assert want[compared].all()
        if F > maxcov:
            assert not want[compared].any()
        # where the verdict turns: compared records whose last base sits at sorted index nLow - 1 (rejected) and nLow (accepted)
        for r in np.flatnonzero(acc):
            n_low = int((sorted_cov[r] < F).sum())
            if not 0 < n_low < lens[r]:
                continue
            mine = compared & (aln["target"] == r) & (aln["t_begin"] < aln["t_end"])
            last = aln["t_end"].astype(np.int64) - 1
            at, below = mine & (last == n_low), mine & (last == n_low - 1)
            assert at.any() and below.any()
            assert want[at].all() and not want[below].any()
            edge_seen += 1
    if max(l for l, a in zip(lens, acc) if a) > 1:
        assert edge_seen >= 2, "no F put nLow inside a reference"


@pytest.mark.gpu
def test_cov_filter_entry_rejects_records_outside_their_reference():
    """the entry's precondition (the difference array of a reference has len + 1 slots) is checked on the host, before any launch"""
    refs = np.array([(100, 1, 0, 0)], REF_DTYPE)
    lib = pagctl.hip_lib()
    for b, e, t in ((0, 101, 0), (60, 50, 0), (0, 10, 1)):
        aln = np.zeros(1, ALN_DTYPE)
        aln["target"], aln["t_begin"], aln["t_end"] = t, b, e
        ok = np.zeros(1 + GUARD, np.uint8)
        assert lib.pag_debug_cov_filter(aln.ctypes.data, 1, refs.ctypes.data, 1, 3, ok.ctypes.data, 0) == -22
