"""CPU: tests/walk_aux_rule.py against itself — every vectorised rule against a plain loop on small random cases, and every
constructed case of tests/test_gpu_walk_aux.py against the shape it is named for (the constructors assert it; here they run
without a device)."""
import numpy as np
import pytest

import walk_aux_rule as R
from aligngraph2_amd.capi import DTYPES


def _small_graph(rng):
    return R.random_graph(rng, int(rng.integers(1, 40)), [0, 7, 7, 9, 30, 31], free=0.3)


@pytest.mark.parametrize("seed", range(5))
def test_graph_is_well_formed_and_id_bounds_equal_the_loop(seed):
    rng = np.random.default_rng(seed)
    G = _small_graph(rng)
    c = R.ctg_of(G["upos"])
    assert (c[:G["n_zero"]] == 0).all() and (c[G["n_zero"]:] != 0).all() and (np.diff(c) >= 0).all()
    assert np.array_equal(G["newid"][G["uold"]], np.arange(G["n_pos"])) and np.array_equal(G["vpos"][G["uold"]], G["upos"])
    assert np.array_equal(np.repeat(np.arange(G["n_nodes"]), np.diff(G["npos_off"].astype(np.int64))), G["vnode"])
    xs = [0, 1, 6, 7, 8, 9, 31, 32, 1000]
    assert np.array_equal(R.id_bounds(G, xs), R.id_bounds_loop(G, xs))
    assert R.id_bounds(G, [0])[0] == 0 and R.id_bounds(G, [1])[0] == G["n_zero"] and R.id_bounds(G, [32])[0] == G["n_pos"]


@pytest.mark.parametrize("k", [3, 8])
def test_code_bitmap_equals_the_loop(k):
    rng = np.random.default_rng(k)
    space = 1 << (2 * k)
    codes = np.unique(np.concatenate([[0, space - 1], rng.integers(0, space, size=20)]))
    bitmap, rank = R.code_bitmap(codes, k)
    for code in range(min(space, 4096)):
        own = (int(bitmap[code >> 6]) >> (code & 63)) & 1
        assert own == int(code in codes)
        if own:
            below = bin(int(bitmap[code >> 6]) & ((1 << (code & 63)) - 1)).count("1")
            assert int(rank[code >> 6]) + below == int(np.searchsorted(codes, code))


def test_ctg_nodes_reads_both_strands():
    ncode = np.array([R.kmer_code("ACG"), R.kmer_code("CGT"), R.kmer_code("TTT")], dtype=np.uint32)
    assert list(ncode) == sorted(ncode)
    assert R.ctg_nodes("ACGTT", True, 3, ncode).tolist() == [0, 1, R.PAG_NONE]
    assert R.ctg_nodes("AAACG", False, 3, ncode).tolist() == [1, R.PAG_NONE, 2]  # (CGTTT)
    assert len(R.ctg_nodes("AC", True, 3, ncode)) == 0
    assert R.pack_bases("CAGT").tolist() == [1 | (2 << 4) | (3 << 6), 0, 0, 0]


@pytest.mark.parametrize("seed", range(4))
def test_pack_job_equals_the_loop(seed):
    rng = np.random.default_rng(seed)
    G = R.random_graph(rng, 60, [0, 5, 5, 8], free=0.4)
    for n in (1, 63, 64, 65, 200):
        v = rng.integers(0, G["n_pos"], size=n).astype(np.uint32)
        s = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        x = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) | (rng.integers(0, 2, size=n).astype(np.uint64) << np.uint64(63))
        x[rng.random(n) < 0.3] = 0
        for xx in (None, x):
            got = R.pack_job(G, v, s, xx)
            assert len(got) == R.pack_words(n, xx is not None)
            assert np.array_equal(got, R.pack_job_loop(G, v, s, xx))


@pytest.mark.parametrize("in_lo,n", [(0, 45), (32, 100), (37, 70)])
def test_commit_equals_the_loop(in_lo, n):
    rng = np.random.default_rng(in_lo)
    v = rng.integers(0, in_lo + n + 40, size=500)
    words, outside = R.commit(v, in_lo, in_lo + n)
    lw, lo = R.commit_loop(v, in_lo, in_lo + n)
    assert np.array_equal(words, lw) and np.array_equal(outside, lo)
    assert np.array_equal(np.flatnonzero(R.bits_to_bool(words, n)) + in_lo, np.unique(v[(v >= in_lo) & (v < in_lo + n)]))


def test_clear_and_concat_rules_on_small_cases():
    buf = np.full(64, 0xA5, dtype=np.uint8)
    out = R.clear_ranges(buf, [(5, 9, 0x04030201), (32, 4, 0xFFFFFFFF), (40, 0, 0)])
    assert out[5:14].tolist() == [2, 3, 4, 1, 2, 3, 4, 1, 2] and out[32:36].tolist() == [255] * 4
    assert (out[:5] == 0xA5).all() and (out[14:32] == 0xA5).all() and (out[36:] == 0xA5).all()
    sv, ss = np.arange(10, 20, dtype=np.uint32), np.arange(110, 120, dtype=np.uint32)
    ov, os_ = R.concat_parts(sv, ss, [(4, 0, 2), (0, 2, 3)], np.zeros(6, np.uint32), np.zeros(6, np.uint32), 77)
    assert ov.tolist() == [14, 15, 10, 11, 12, 0] and os_.tolist() == [77, 115, 110, 111, 112, 0]


def test_gather_records_follow_the_graph():
    rng = np.random.default_rng(3)
    G = _small_graph(rng)
    rec = R.gather_records(G, np.arange(G["n_pos"]), np.zeros(G["n_pos"]), DTYPES["pag_path_node"])
    for v in range(G["n_pos"]):
        node = int(np.searchsorted(G["npos_off"], v, side="right")) - 1
        assert (rec["code"][v], rec["ctg"][v], rec["ref"][v], rec["cnt"][v]) == (G["ncode"][node], int(G["vpos"][v]) >> 32, int(G["vpos"][v]) & R.U32, G["vcnt"][v])


# ---- the constructed cases ----------------------------------------------------------------------------------------------------
def test_seed_first_cases_have_their_shapes():
    cases = R.seed_first_cases()
    assert len({name for name, *_ in cases}) == len(cases) >= 16
    assert {len(C["nodes"]) for _, _, C, _, _ in cases} >= {1, 63, 64, 65, 200}
    assert {stride for *_, stride in cases} >= {4, 8}


def test_seed_window_case_has_its_shapes_and_the_parts_make_the_list():
    G, C, dev, pos, _ = R.seed_window_case()
    R.check_window_requests(G, C, dev, pos)
    spans = {min(right + 1, len(C["nodes"])) - left for (left, right), _ in R.WINDOW_REQUESTS if left < len(C["nodes"])}
    assert spans >= {1, 16, 1023, 1024, 1025, 3000}
    for label, D in R.window_states(G, C, dev, pos):
        for (left, right), name in R.WINDOW_REQUESTS:
            lo, hi = R.window_bounds(D, left, right)
            parts = [R.seed_window_range(G, D, a, b, pos, dev) for a, b in R.window_split(lo, hi)]
            whole = R.seed_window_range(G, D, lo, hi, pos, dev)
            assert [p for part in parts for p in part] == whole, (label, name)
            words = R.seed_window_words(parts, 64, np.zeros(16 * 64, np.uint32))
            assert R.window_candidates(words, 64) == list(dict.fromkeys(whole)), (label, name)
    assert len(set(R.seed_window_range(G, C, 0, 3100, pos, dev))) < len(R.seed_window_range(G, C, 0, 3100, pos, dev)), "no vertex twice in a window"
    # the clip: 20 matches against a stride of 8 — the count says 20, seven ids are written, the rest stays
    ids = R.seed_window_range(G, C, 1400, 1410, pos, dev)
    w = R.seed_window_words([ids] + [[]] * 15, 8, np.full(16 * 8, 9, np.uint32))
    assert w[0] == 20 and w[1:8].tolist() == ids[:7] and w[8] == 0 and (w[9:16] == 9).all()


def test_checkpoint_case_has_its_shapes():
    G, C, dev, reqs = R.checkpoint_case()
    assert {min(r, len(C["nodes"]) - 1) - l + 1 for l, r, *_ in reqs if l < len(C["nodes"])} >= {1, 64, 65, 130}
    assert len(C["nodes"]) < (1 << 20) and np.diff(G["npos_off"].astype(np.int64)).max() < (1 << 20)
    # a visited candidate of higher abundance exists in the window where it must lose
    assert any(R.visited(G, C, p) and G["vcnt"][p] == 8000 for p in R.vertices_at(G, C, 61))


def test_pack_batches_have_their_shapes():
    rng = np.random.default_rng(11)
    G = R.random_graph(rng, 900, [0] + list(range(1000, 1040)))
    for batch in R.pack_batches(rng, G):
        offs, total = R.pack_layout(batch)
        ends = [o + R.pack_words(len(j[0]), j[2] is not None) for o, j in zip(offs, batch)]
        assert all(e + 1 == o for e, o in zip(ends, offs[1:])) and ends[-1] + 1 == total
        assert {j[2] is None for j in batch} == {True, False}
    lens = sorted({len(j[0]) for batch in R.pack_batches(rng, G) for j in batch})
    assert lens == [1, 63, 64, 65, 16384, 16385, 40000]
