"""GPU: pag_find_all_batch (csrc/hip/k_find.hip) — the graph's vertices along a list of sequences, against tests/find_rule.py
(PABruijnGraph::findAll in numpy over the reference's graph dumps; tests/test_find_rule.py holds the rule itself).  Every
comparison is exact.

Every test builds its graph with pag_process alone (Built of test_gpu_succ_query.py) or imports a constructed one.

  1. every golden block: all contigs in both strands and the references forward, in ONE call, field for field;
  2. the names close the loop: every (code, pos) the call returns is a vertex pag_successors_batch knows, with the reference's list;
  3. shapes: 0, 1, 2, 1 023, 1 024, 1 025 and 2 049 offsets, both strands, repeated and reversed lists, a packed start that is
     4-byte but not 8-byte aligned, no sequence at all, a handle whose every k-mer is solid;
  4. constructed graphs (pag_shard_import) at k = 12, 14 and 16 — the goldens stop at k = 11 — for what no golden holds: code 0,
     the last slot of tkey, lower bounds at 0 and at n_t, nodes of exactly 64 / 65 / 129 positions, tiles of exactly 64 / 65 / 0
     hits, codes >= 2^31;
  5. buffers: the sizing call, either buffer one short, hits only, pag_find_all_batch_bytes;
  6. the call leaves the handle as it found it;
  7. refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import find_rule
import goldens
import pagctl  # (puts the repository root on the path)
import aligngraph2_amd as ag
from aligngraph2_amd import capi
from aligngraph2_amd.capi import BuildStats, PagSeqs, Region, ShardSlice
from test_gpu_succ_query import Built, assert_lists, golden, lists_of

HIT, VERTEX = capi.FIND_HIT_DTYPE, capi.FIND_VERTEX_DTYPE
OK, EINVAL, ERANGE = capi.PAG_OK, capi.PAG_EINVAL, capi.PAG_ERANGE


def assert_found(label, got, want):
    """(hit_off, hits, vertices) of the call against the rule's, field for field"""
    for what, g, w in zip(("hit_off", "hits", "vertices"), got, want):
        assert len(g) == len(w), f"{label}: {len(g)} {what}, the rule has {len(w)}"
    assert np.array_equal(got[0].astype(np.int64), want[0].astype(np.int64)), f"{label}: hit_off differs, first at {int(np.flatnonzero(got[0] != want[0])[0])}"
    for what, g, w in (("hit", got[1], want[1]), ("vertex", got[2], want[2])):
        for f in g.dtype.names:
            bad = np.flatnonzero(g[f] != w[f])
            assert len(bad) == 0, f"{label}: field {f} differs in {len(bad)} of {len(g)}, first at {what} {int(bad[0])}: {g[bad[0]]} for {w[bad[0]]}"


def search(b_hip, g, seqs, reverse, pick=None):
    """ag.find_all_batch of the strings `seqs` (pick: the list names these of them, in this order)"""
    packed, byte_off, lengths = find_rule.pack(seqs)
    pick = np.arange(len(seqs)) if pick is None else np.asarray(pick)
    return ag.find_all_batch(b_hip, g, packed, byte_off[pick], lengths[pick], np.asarray(reverse, dtype=np.uint8))


def block_strings(b):
    """what test 1 searches in a block: every contig forward, every contig reverse, every reference forward"""
    ctgs = [s for _, s in find_rule.read_fasta(os.path.join(b.ind, "ctg.fasta"))]
    refs = [s for _, s in find_rule.read_fasta(os.path.join(b.ind, "ref.fasta"))]
    return ctgs + ctgs + refs, [0] * len(ctgs) + [1] * len(ctgs) + [0] * len(refs)


# ---- 1. the goldens -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", goldens.case_names())
def test_every_contig_and_reference_of_the_goldens(name, workdir):
    for block, table in enumerate(find_rule.node_tables(name)):
        with Built(name, block, workdir) as b:
            seqs, rev = block_strings(b)
            want = find_rule.find_all(table, find_rule.solid_codes(b.inp), b.inp.k, seqs, rev)
            assert len(want[1]) > 1000 and len(want[2]) > 1000 and (want[1]["n_pos"] == 0).any(), "the case says too little"
            assert_found(f"{name} block {block}", search(b.hip, b.g, seqs, rev), want)
            if name == "succ_corners_t8":
                assert want[1]["n_pos"].max() > 255, "no hit whose vertices take more than one turn of the lanes"
            if name in ("succ_corners_t8", "eps5_k7_repeats_t8"):
                # (eps5_k7_repeats_t8's heaviest node has 25 positions: its copies take more than one turn because 64 hits
                # have more than 64 positions between them)
                off, n_pos = want[0].astype(np.int64), want[1]["n_pos"].astype(np.int64)
                turns = [int(n_pos[lo:lo + 64].sum()) for s in range(len(off) - 1) for lo in range(int(off[s]), int(off[s + 1]), 64)]
                assert max(turns) > 128, "no turn of 64 hits whose vertex copy goes round more than twice"


# ---- 2. the names close the loop --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["extend_gap_t1", "eps20_k11_jitter_t16"])
def test_the_names_are_those_pag_successors_batch_takes(name, workdir):
    ref = golden(name)[0]
    with Built(name, 0, workdir) as b:
        seqs, rev = block_strings(b)
        hit_off, hits, vert = search(b.hip, b.g, seqs, rev)
        code = np.repeat(hits["code"], hits["n_pos"])
        assert len(code) == len(vert) > 0
        names = np.unique(np.stack([code.astype(np.uint64), vert["pos"]], axis=1), axis=0)
        # where the dump has each of them (its V lines are in ref["v"] order)
        index = {(int(c), int(p)): i for i, (c, p) in enumerate(zip(ref["vcode"][ref["v"]], ref["vpos"][ref["v"]]))}
        pick = np.array([index[(int(c), int(p))] for c, p in names])
        assert len(pick) > len(index) // 4, "the contigs and the reference name a good part of the graph"
        off, status, rec = ag.successors_batch(b.hip, b.g, names[:, 0].astype(np.uint32), names[:, 1], 2 * b.spec["epsilon"], 0.15)
        assert not status.any(), f"{np.count_nonzero(status)} names are no vertex to pag_successors_batch"
        w_off, want = lists_of(ref["off"], ref["rows"], pick)
        assert_lists(name, off, rec, w_off, want)


# ---- 3. shapes --------------------------------------------------------------------------------------------------------------------
OFFSETS = (0, 1, 2, 1023, 1024, 1025, 2049)


@pytest.mark.gpu
def test_shapes_of_a_call(workdir):
    name = "extend_gap_t1"
    table = find_rule.node_tables(name)[0]
    with Built(name, 0, workdir) as b:
        k = b.inp.k
        solid = find_rule.solid_codes(b.inp)
        ctg = find_rule.read_fasta(os.path.join(b.ind, "ctg.fasta"))[1][1]
        assert len(ctg) >= 2049 + k - 1 + 7 * len(OFFSETS)
        cut = [ctg[7 * i:7 * i + n + k - 1] for i, n in enumerate(OFFSETS)]  # (n offsets each; n = 0: k - 1 bases)
        seqs, rev = cut + cut, [0] * len(cut) + [1] * len(cut)
        packed, byte_off, lengths = find_rule.pack(seqs)
        assert (byte_off % 8 == 4).any() and (byte_off % 16 == 4).any(), "no start that is 4-byte but not 8-byte aligned"
        want = find_rule.find_all(table, solid, k, seqs, rev)
        cnt = np.diff(want[0].astype(np.int64))
        assert (cnt <= np.array(OFFSETS * 2)).all() and cnt[0] == 0 and cnt[len(OFFSETS) - 1] > 1024 and cnt[-1] > 64
        assert_found("every length, both strands", search(b.hip, b.g, seqs, rev), want)
        # the list reversed, the longest sequence named three times (twice forward, once reverse)
        pick = list(range(len(seqs)))[::-1] + [len(cut) - 1, len(cut) - 1, 2 * len(cut) - 1]
        want = find_rule.find_all(table, solid, k, [seqs[i] for i in pick], [rev[i] for i in pick])
        assert_found("reversed and repeated", search(b.hip, b.g, seqs, [rev[i] for i in pick], pick), want)
        # one k-mer: find
        kmer = ctg[100:100 + k]
        want = find_rule.find_all(table, solid, k, [kmer], [0])
        assert len(want[1]) == 1 and want[1]["n_pos"][0] >= 1
        assert_found("find", search(b.hip, b.g, [kmer], [0]), want)
        # no sequence at all
        hit_off, hits, vert = ag.find_all_batch(b.hip, b.g, np.zeros(0, dtype=np.uint8), [], [])
        assert hit_off.tolist() == [0] and len(hits) == 0 and len(vert) == 0
        # only sequences without an offset
        assert_found("nothing to search", search(b.hip, b.g, [cut[0], ""], [0, 1]), find_rule.find_all(table, solid, k, [cut[0], ""], [0, 1]))
        # a handle whose every k-mer is solid: every offset is a hit (the node table is the handle's own exported graph here:
        # no dump of the reference holds that graph)
        g2 = C.c_void_p(pagctl.hip_create(b.inp, solid_bitmap=np.full(4 ** k // 32, 0xFFFFFFFF, dtype=np.uint32)))
        try:
            table2 = find_rule.table_of_csr(pagctl.run_on(g2, b.inp)["csr"])
            want = find_rule.find_all(table2, None, k, seqs, rev)
            assert np.array_equal(np.diff(want[0].astype(np.int64)), np.array(OFFSETS * 2))
            assert_found("every k-mer solid", search(b.hip, g2, seqs, rev), want)
        finally:
            b.hip.pag_destroy(g2)


# ---- 4. constructed graphs --------------------------------------------------------------------------------------------------------
def distinct_kmer_string(rng, n, k):
    """n random bases whose k-mers, forward and reverse, are 2 (n - k + 1) different codes"""
    for _ in range(200):
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))
        c = np.concatenate((find_rule.codes(s, k), find_rule.codes(s, k, reverse=True)))
        if len(np.unique(c)) == len(c) and c.min() > 0 and c.max() < 4 ** k - 2:
            return s
    raise AssertionError("no such string")


def import_graph(hip, words, k, nodes, rng):
    """a handle with the solid set of `words` and the graph `nodes` = [(code, positions u64, counts)] in ascending code, through
    pag_shard_import: segments longer than their leaders, fillers behind them — none behind the last node"""
    import torch
    tkey, tval, tseg, tcnt = [], [], [], []
    for i, (c, p, n) in enumerate(nodes):
        extra = 0 if i == len(nodes) - 1 else int(rng.integers(0, 4))
        tkey += [c] * (len(p) + extra)
        tval += [int(x) for x in p] + [int(p[0])] * extra
        tseg += [len(p)] + [0x80000000 | j for j in range(1, len(p))] + [0] * extra
        tcnt += [int(x) for x in n] + [0] * extra
    c0 = nodes[0][0]
    host = (np.array(tkey, dtype=np.uint32), np.array(tval, dtype=np.uint64), np.array(tseg, dtype=np.uint32), np.array(tcnt, dtype=np.uint16),
            np.array([c0], dtype=np.uint32), np.array([(c0 << 32) | (1 << 1)], dtype=np.uint64), np.array([1], dtype=np.uint32))
    words = np.ascontiguousarray(words, dtype=np.uint64)
    err = C.c_int()
    h = C.c_void_p(hip.pag_create(words.ctypes.data, len(words), k, 0, C.byref(err)))
    assert h, hip.pag_last_error()
    dev = [torch.from_numpy(a.view(np.uint8).copy()).cuda() for a in host]  # (torch has no unsigned 32 / 64-bit tensors: the bytes go up)
    st = BuildStats()
    st.n_nodes, st.n_pos, st.n_uniq_edges = len(nodes), sum(len(p) for _, p, _ in nodes), 1
    sl = ShardSlice(len(host[0]), len(host[4]), *[t.data_ptr() for t in dev], st)
    rc = hip.pag_shard_import(h, C.byref(sl), 1, None)
    if rc != 0:
        hip.pag_destroy(h)
        raise AssertionError(hip.pag_last_error())
    return h, len(host[0])


def constructed_case(k, rng):
    """(solid-set words, nodes for import_graph, sequences, strands, what the rule finds) — and the asserts that the case is what
    it says it is, by the rule alone"""
    top = 4 ** k - 1
    # a string of 3 full tiles and a part of a fourth.  Forward: tile 0 has exactly 64 hits, tile 1 none, tile 2 exactly 65, tile
    # 3 a few; reverse: tile 0 exactly 65, tile 1 exactly 64, tile 2 none, tile 3 one
    n_off = 3 * 1024 + 40
    s = distinct_kmer_string(rng, n_off + k - 1, k)
    fwd, bwd = find_rule.codes(s, k), find_rule.codes(s, k, reverse=True)
    inner = lambda lo, n: lo + 1 + np.sort(rng.choice(1022, size=n, replace=False))  # noqa: E731  (n offsets strictly inside the tile at lo)
    f_at = np.concatenate(([0], inner(0, 62), [1023], [2048], inner(2048, 63), [3071], [3072, 3080, n_off - 1]))
    b_at = np.concatenate(([0], inner(0, 63), [1023], [1024], inner(1024, 62), [2047], [n_off - 1]))
    solid_s = np.concatenate((fwd[f_at], bwd[b_at]))
    # the nodes: most of the string's solid k-mers, with 1 .. 5 positions; four heavy ones in the tile of 65 hits; code 0 (k != 12)
    # and the largest code of the graph in the last slot of tkey; solid k-mers without a node below (k = 12: code 0), between and
    # above (4^k - 1) the graph's codes
    with_zero = k != 12
    n_pos = {int(c): int(rng.integers(1, 6)) for c in solid_s if rng.random() < 0.8}
    for c, n in zip(fwd[f_at[(f_at >= 2048) & (f_at < 3072)]][[3, 4, 30, 64]], (64, 65, 129, 300)):
        n_pos[int(c)] = n
    last = top - 1  # (distinct_kmer_string keeps the string's k-mers below it)
    n_pos[last] = 1
    if with_zero:
        n_pos[0] = 3
    elif 0 in n_pos:
        del n_pos[0]
    assert top not in n_pos
    nodes = []
    for c in sorted(n_pos):
        p = np.unique(rng.integers(1, 2 ** 63, size=n_pos[c], dtype=np.uint64))  # (contig << 32 | reference, in ascending order)
        assert len(p) == n_pos[c]
        nodes.append((c, p, rng.integers(1, 65536, size=n_pos[c])))
    words = np.concatenate((np.array([k], dtype=np.uint64), solid_s.astype(np.uint64), np.array([0, last, top], dtype=np.uint64)))  # (the header word k is a solid k-mer too: quirk Q1)
    solid = find_rule.solid_of_words(words, k)
    table = find_rule.make_table([c for c, _, _ in nodes], [len(p) for _, p, _ in nodes], np.concatenate([p for _, p, _ in nodes]),
                                 np.concatenate([n for _, _, n in nodes]))
    kmer_of = lambda c: "".join("ACGT"[(c >> (2 * (k - 1 - i))) & 3] for i in range(k))  # noqa: E731
    heavy = [int(c) for c in n_pos if n_pos[c] >= 64]
    seqs = [s, s, "N" * (k + 3), "N" * (k + 3), kmer_of(last), kmer_of(k)] + [kmer_of(c) for c in heavy]
    rev = [0, 1, 0, 1, 0, 0] + [0] * len(heavy)
    want = find_rule.find_all(table, solid, k, seqs, rev)
    # the case is what it says it is (by the rule, whatever the device says)
    off, hits = want[0].astype(np.int64), want[1]
    per_tile = lambda i: np.bincount(hits["offset"][off[i]:off[i + 1]] // 1024, minlength=4).tolist()  # noqa: E731
    assert per_tile(0) == [64, 0, 65, 3] and per_tile(1) == [65, 64, 0, 1]
    assert sorted(n for n in n_pos.values() if n >= 64) == [64, 65, 129, 300]
    nul, tee = hits[off[2]:off[3]], hits[off[3]:off[4]]
    assert nul["code"].tolist() == [0] * 4 and nul["n_pos"].tolist() == ([3] * 4 if with_zero else [0] * 4)  # (without: a lower bound at 0)
    assert tee["code"].tolist() == [top] * 4 and tee["n_pos"].tolist() == [0] * 4                             # (a lower bound at n_t)
    assert hits[off[4]]["code"] == last == table["code"][-1] and hits[off[4]]["n_pos"] == 1
    assert k != 16 or (hits["code"] >= 2 ** 31).sum() > 10
    assert len(solid) == len(np.unique(words))
    return words, nodes, seqs, rev, want


@pytest.mark.gpu
@pytest.mark.parametrize("k", [12, 14, 16])
def test_constructed_graph(k):
    rng = np.random.default_rng(1000 + k)
    hip = pagctl.hip_lib()
    words, nodes, seqs, rev, want = constructed_case(k, rng)
    h, n_t = import_graph(hip, words, k, nodes, rng)
    try:
        assert n_t > sum(len(p) for _, p, _ in nodes), "no filler slot behind any node's leaders"
        assert hip.pag_solid_count(h) == len(np.unique(words))
        assert_found(f"constructed graph, k = {k}", search(hip, h, seqs, rev), want)
    finally:
        hip.pag_destroy(h)


# ---- 5. buffers -------------------------------------------------------------------------------------------------------------------
def raw_call(hip, g, packed, byte_off, lengths, reverse, hit_cap, vert_cap, hits_only=False):
    """the C call itself with sentinel-filled buffers: (rc, hit_off, hits, vertices, n_hits, n_vert, ms_kernels)"""
    padded = np.concatenate((packed, np.zeros(16, dtype=np.uint8)))
    seqs = PagSeqs(len(lengths), byte_off.ctypes.data, lengths.ctypes.data, padded.ctypes.data, len(packed))
    rev = np.ascontiguousarray(reverse, dtype=np.uint8)
    hit_off = np.full(len(lengths) + 1, 0xDEAD, dtype=np.uint64)
    hits = np.full(max(hit_cap, 1) * HIT.itemsize, 0xA5, dtype=np.uint8)
    vert = np.full(max(vert_cap, 1) * VERTEX.itemsize, 0xA5, dtype=np.uint8)
    n_hits, n_vert, ms = C.c_uint64(12345), C.c_uint64(12345), C.c_double(-1.0)
    rc = hip.pag_find_all_batch(g, C.byref(seqs), rev.ctypes.data, hit_off.ctypes.data, hits.ctypes.data if hit_cap else None, hit_cap,
                                None if hits_only or not vert_cap else vert.ctypes.data, 0 if hits_only else vert_cap, C.byref(n_hits), C.byref(n_vert), C.byref(ms))
    return rc, hit_off, hits, vert, n_hits.value, n_vert.value, ms.value


@pytest.mark.gpu
def test_buffers(workdir):
    name = "eps5_k7_repeats_t8"
    table = find_rule.node_tables(name)[0]
    with Built(name, 0, workdir) as b:
        seqs, rev = block_strings(b)
        want = find_rule.find_all(table, find_rule.solid_codes(b.inp), b.inp.k, seqs, rev)
        nh, nv = len(want[1]), len(want[2])
        packed, byte_off, lengths = find_rule.pack(seqs)
        args = (b.hip, b.g, packed, byte_off, lengths, rev)
        untouched = lambda a: bool((a == 0xA5).all())  # noqa: E731
        # the sizing call: PAG_ERANGE with the totals and the complete hit_off
        rc, hit_off, hits, vert, n_hits, n_vert, ms = raw_call(*args, 0, 0)
        assert rc == ERANGE and (n_hits, n_vert) == (nh, nv) and np.array_equal(hit_off, want[0]) and ms > 0.0
        assert b"hits" in b.hip.pag_last_error()
        # either buffer one short
        for hit_cap, vert_cap in ((nh - 1, nv), (nh, nv - 1)):
            rc, hit_off, hits, vert, n_hits, n_vert, ms = raw_call(*args, hit_cap, vert_cap)
            assert rc == ERANGE and (n_hits, n_vert) == (nh, nv) and np.array_equal(hit_off, want[0])
            assert untouched(hits) and untouched(vert), "something was written although a buffer was too small"
        # both exact
        rc, hit_off, hits, vert, n_hits, n_vert, ms_full = raw_call(*args, nh, nv)
        assert rc == OK, b.hip.pag_last_error()
        assert_found("exact buffers", (hit_off, hits.view(HIT), vert.view(VERTEX)), want)
        assert ms_full > 0.0
        # hits only: first and n_pos as in the full call, no vertex is copied
        rc, hit_off, hits, vert, n_hits, n_vert, ms = raw_call(*args, nh + 5, 0, hits_only=True)
        assert rc == OK and (n_hits, n_vert) == (nh, nv), b.hip.pag_last_error()
        assert np.array_equal(hits.view(HIT)[:nh], want[1]) and untouched(hits[nh * HIT.itemsize:]) and untouched(vert)
        # what the call's device memory is stated to be grows with every argument (its booking is not exposed)
        size = b.hip.pag_find_all_batch_bytes
        base = size(len(lengths), len(packed), nh, nv)
        assert base >= len(packed) + 12 * len(lengths) + nh * HIT.itemsize + nv * VERTEX.itemsize
        assert size(len(lengths) + 1000, len(packed), nh, nv) > base and size(len(lengths), len(packed) + 4096, nh, nv) > base
        assert size(len(lengths), len(packed), nh + 1, nv) == base + HIT.itemsize and size(len(lengths), len(packed), nh, nv + 1) == base + VERTEX.itemsize
        assert size(0, 0, 0, 0) == 0


def test_arguments_are_checked_before_a_device_is_touched():
    """(runs without a GPU)"""
    hip = pagctl.hip_lib()
    n_hits, n_vert = C.c_uint64(5), C.c_uint64(6)
    off = np.zeros(1, dtype=np.uint64)
    empty = PagSeqs(0, None, None, None, 0)
    assert hip.pag_find_all_batch(None, C.byref(empty), None, off.ctypes.data, None, 0, None, 0, C.byref(n_hits), C.byref(n_vert), None) == EINVAL
    assert (n_hits.value, n_vert.value) == (0, 0) and b"null" in hip.pag_last_error()
    size = hip.pag_find_all_batch_bytes
    assert size(0, 1000, 10, 10) == 0
    assert size(100, 1 << 20, 10, 20) >= (1 << 20) + 100 * 12 + 10 * HIT.itemsize + 20 * VERTEX.itemsize


# ---- 6. the handle is left as found -----------------------------------------------------------------------------------------------
def delivered_paths(hip, g, n_ctgs):
    out = []
    for c in range(n_ctgs):
        for fwd in (1, 0):
            n = C.c_uint64()
            p = hip.pag_travel_path_oriented(g, c, fwd, C.byref(n))
            out.append(C.string_at(p, n.value * 24) if p and n.value else b"")
    return out


def export(hip, g):
    nn, npos, ne = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert hip.pag_csr_sizes(g, C.byref(nn), C.byref(npos), C.byref(ne)) == 0
    out = [np.zeros(nn.value, np.uint32), np.zeros(nn.value + 1, np.uint64), np.zeros(npos.value, np.uint32), np.zeros(npos.value, np.uint32),
           np.zeros(npos.value, np.uint16), np.zeros(nn.value + 1, np.uint64), np.zeros(ne.value, np.uint32), np.zeros(ne.value, np.int32)]
    csr = capi.Csr(nn.value, npos.value, ne.value, *[a.ctypes.data for a in out])
    assert hip.pag_export_csr(g, C.byref(csr)) == 0, hip.pag_last_error()
    return out


@pytest.mark.gpu
def test_the_call_leaves_the_handle_alone(workdir, monkeypatch):
    import seq_text
    from test_gpu_succ_golden import block_orient
    for s in ("PAG_SUCC_HEAVY", "PAG_TRAVEL_VIEW", "PAG_VIEW_HALO", "PAG_VIEW_MARGIN"):
        monkeypatch.delenv(s, raising=False)
    name = "extend_gap_t1"
    paths = []
    for with_call in (True, False):
        with Built(name, 0, workdir) as b:
            hip, g = b.hip, b.g
            ctgs = find_rule.read_fasta(os.path.join(b.ind, "ctg.fasta"))
            refs = find_rule.read_fasta(os.path.join(b.ind, "ref.fasta"))
            pc = seq_text.Packed([s for _, s in ctgs])
            ref_len = np.array([len(s) for _, s in refs], dtype=np.uint32)
            orient = block_orient(b.ind, 0, [n for n, _ in ctgs])
            prm = capi.TravelParams(b.spec["threads"], 0, 2 * b.spec["epsilon"], 0.15, 0.90, 50)
            seqs, rev = block_strings(b)
            if with_call:
                before = export(hip, g)
                first = search(hip, g, seqs, rev)
                assert len(first[1]) > 1000
                for a, c in zip(before, export(hip, g)):
                    assert np.array_equal(a, c), "pag_export_csr gives another graph after the call"
            assert hip.pag_travel_prepare(g, C.byref(pc.c), ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
            assert hip.pag_travel(g, C.byref(pc.c), orient.ctypes.data, ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
            if with_call:
                again = search(hip, g, seqs, rev)  # (beside a prepared view, after walks that marked vertices used)
                for a, c in zip(first, again):
                    assert np.array_equal(a, c), "the call answers differently after pag_travel"
            paths.append(delivered_paths(hip, g, len(ctgs)))
    assert any(paths[0]) and paths[0] == paths[1], "pag_travel delivers other paths after the call"


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(workdir):
    name = "extend_gap_t1"
    with Built(name, 0, workdir) as b:
        hip = b.hip
        seqs, rev = block_strings(b)
        packed, byte_off, lengths = find_rule.pack(seqs)

        def one_line(rc, want, word):
            msg = hip.pag_last_error()
            assert rc == want and word in msg and b"\n" not in msg and 0 < len(msg) < 400, (rc, msg)

        # a handle before pag_process
        fresh = C.c_void_p(pagctl.hip_create(b.inp))
        try:
            rc, hit_off, hits, vert, n_hits, n_vert, ms = raw_call(hip, fresh, packed, byte_off, lengths, rev, 10, 10)
            one_line(rc, EINVAL, b"no finished graph")
            assert (n_hits, n_vert) == (0, 0)
        finally:
            hip.pag_destroy(fresh)
        # a start that is no multiple of 4; a sequence that ends beyond packed_bytes
        odd = byte_off.copy()
        odd[1] += 2
        one_line(raw_call(hip, b.g, packed, odd, lengths, rev, 10, 10)[0], EINVAL, b"sequence 1")
        far = byte_off.copy()
        far[2] = len(packed)
        one_line(raw_call(hip, b.g, packed, far, lengths, rev, 10, 10)[0], EINVAL, b"sequence 2")
        with pytest.raises(RuntimeError):
            ag.find_all_batch(hip, b.g, packed, odd, lengths, rev)
        # a null handle; a buffer with room and no address
        n = C.c_uint64()
        assert hip.pag_find_all_batch(None, None, None, None, None, 0, None, 0, C.byref(n), C.byref(n), None) == EINVAL
        off1 = np.zeros(1, dtype=np.uint64)
        empty = PagSeqs(0, None, None, None, 0)
        one_line(hip.pag_find_all_batch(b.g, C.byref(empty), None, off1.ctypes.data, None, 5, None, 0, C.byref(n), C.byref(n), None), EINVAL, b"null")
        assert hip.pag_find_all_batch(b.g, C.byref(empty), None, off1.ctypes.data, None, 0, None, 0, C.byref(n), C.byref(n), None) == OK
        # the handle still answers
        assert raw_call(hip, b.g, packed, byte_off, lengths, rev, 0, 0)[0] == ERANGE
        # a regional handle
        riv, ropen = np.array([1, 1000], dtype=np.uint32), np.array([0, 1], dtype=np.uint8)
        assert hip.pag_shard_set_region(b.g, C.byref(Region(0, None, 1, riv.ctypes.data, ropen.ctypes.data))) == 0
        rc, hit_off, hits, vert, n_hits, n_vert, ms = raw_call(hip, b.g, packed, byte_off, lengths, rev, 10, 10)
        one_line(rc, ERANGE, b"region")
        assert (n_hits, n_vert) == (0, 0)
        with pytest.raises(RuntimeError):
            ag.find_all_batch(hip, b.g, packed, byte_off, lengths, rev)
