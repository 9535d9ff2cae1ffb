"""GPU: a block as N ranks that take turns on ONE device and ONE handle — PAGRAPH_SERIAL_RANKS in bin/pagraph, pag_shard_run_serial
and pag_shard_extract_for in the library, the stable compaction of one owner's records (k_owner_pick.hip) through its hook.

Every expectation is somebody else's result: the reference's golden files for the executable; the Python prototype
(rank_serial.run, which the suite holds to the one-GPU run) for the library's schedule; the emulated N-rank build of
tests/test_gpu_shards.py (N handles, pag_shard_extract / _build / _select / _import) for what one turn leaves in the handle;
pag_shard_extract_range + pag_shard_take_part for pag_shard_extract_for; numpy for the compaction."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import goldens
import pagctl
import synth

sys.path.insert(0, pagctl.ROOT)
import aligngraph2_amd  # noqa: E402
from aligngraph2_amd import capi, parallel  # noqa: E402

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pagraph")
TILE = 2048  # k_owner_pick.hip: PK_T x PK_R records per tile


# ------------------------------------------------------------------------------------------------------------------------------
# bin/pagraph under PAGRAPH_SERIAL_RANKS: the reference's golden files, N lines of the turns per block
# ------------------------------------------------------------------------------------------------------------------------------
def _n_blocks(name):
    return len(goldens.load_spec(name).get("blocks", [0]))


def _run_exe(name, work, extra):
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, os.path.join(work, "in"))
    out = os.path.join(work, "out")
    os.makedirs(out, exist_ok=True)
    argv = synth.pagraph_argv(EXE, ind, out, threads=spec["threads"], epsilon=spec["epsilon"], cov=spec["cov"])
    env = dict(os.environ)
    for v in ("PAGRAPH_SERIAL_RANKS", "PAGRAPH_SHARD", "PAGRAPH_OVERLAP", "PAGRAPH_DEVICE_DUMPS", "PAGRAPH_DEVICE_SEQS", "PAGRAPH_TIMING"):
        env.pop(v, None)
    env.update(extra)
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300), out


def _turn_lines(stderr):
    return [ln for ln in stderr.splitlines() if ln.startswith("[serial ranks] block ")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,extra", [
    ("join_fwd_t1", 2, {}), ("join_fwd_t1", 4, {}),
    ("join_rev_t16", 2, {}), ("join_rev_t16", 4, {}),
    ("three_ctg_multi_t4", 2, {}), ("three_ctg_multi_t4", 4, {"PAGRAPH_DEVICE_DUMPS": "1", "PAGRAPH_DEVICE_SEQS": "1"}),
    ("two_blocks_both_orient_t16", 2, {"PAGRAPH_OVERLAP": "0"}), ("two_blocks_both_orient_t16", 4, {}),
    ("eps5_k7_repeats_t8", 8, {}),  # (k = 7: a 14-bit code, owner ranges can be empty)
    ("succ_corners_t8", 2, {}),
])
def test_serial_ranks_reproduce_the_golden(name, n, extra, workdir):
    tag = f"serial_{name}_{n}_" + "_".join(sorted(extra))
    r, out = _run_exe(name, str(workdir / tag), dict(extra, PAGRAPH_SERIAL_RANKS=str(n), PAGRAPH_TIMING="1"))
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    goldens.compare_out_dir(name, out)
    lines = _turn_lines(r.stderr)
    for b in range(_n_blocks(name)):
        mine = [ln for ln in lines if ln.startswith(f"[serial ranks] block {b} turn ")]
        assert [ln.split()[5] for ln in mine] == [f"{d}/{n}:" for d in range(n)], lines
    assert len(lines) == n * _n_blocks(name), lines
    for ln in lines:
        for field in ("held_vertices", "held_edges", "tuples_in", "edges_in", "region_bytes", "s_extract", "s_build", "s_select", "s_import", "s_walk"):
            assert f" {field} " in ln, ln


@pytest.mark.gpu
def test_serial_ranks_refusals_and_one_rank(workdir):
    r, _ = _run_exe("join_fwd_t1", str(workdir / "serial_refuse3"), {"PAGRAPH_SERIAL_RANKS": "3"})
    assert r.returncode == 1 and "PAGRAPH_SERIAL_RANKS must be 2, 4 or 8" in r.stderr, r.stderr[-1000:]
    assert len(r.stderr.strip().splitlines()) == 1
    r, _ = _run_exe("join_fwd_t1", str(workdir / "serial_refuse_both"), {"PAGRAPH_SERIAL_RANKS": "2", "PAGRAPH_SHARD": "0/2"})
    assert r.returncode == 1 and "PAGRAPH_SERIAL_RANKS and PAGRAPH_SHARD exclude each other" in r.stderr, r.stderr[-1000:]
    assert len(r.stderr.strip().splitlines()) == 1
    # 1 = unset: the ordinary path
    r, out = _run_exe("join_fwd_t1", str(workdir / "serial_one"), {"PAGRAPH_SERIAL_RANKS": "1", "PAGRAPH_TIMING": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert not _turn_lines(r.stderr)
    goldens.compare_out_dir("join_fwd_t1", out)


@pytest.mark.gpu
def test_a_walk_that_leaves_its_region_names_the_halo(workdir):
    """no halo around the reference bands: the walks of the leaping zones leave them (as in
    test_ranks_hold_their_region_only_and_walk_the_same_paths) — reported with the way out, or no output differs"""
    r, out = _run_exe("three_ctg_multi_t4", str(workdir / "serial_nohalo"), {"PAGRAPH_SERIAL_RANKS": "2", "PAG_SHARD_HALO": "0"})
    if r.returncode == 0:
        goldens.compare_out_dir("three_ctg_multi_t4", out)
    else:
        assert r.returncode == 1 and "left the region" in r.stderr and "raise PAG_SHARD_HALO" in r.stderr, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------------------
# the library against the prototype
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """the workload of test_rank_serial_run_equals_the_one_gpu_run (3 Mb reference, 12 000 reads), made once"""
    import torch
    import bench
    import biggen
    hip, host = bench.load_libs()
    capi.bind(hip)
    capi.bind(host)
    sp = biggen.BigSpec(seed=13, ref_len=3_000_000, n_reads=12000, read_span=4000, k=14, eps=10, ctg_len=250_000, gap_lo=300, gap_hi=3000,
                        rev_ctg_frac=0.3, threads=16, cov=2, solid_min_abundance=2, chunk_reads=512)
    w = biggen.BigWorkload(sp, device="cuda")
    torch.cuda.synchronize()
    inp = w.build_input()
    ctg_seqs, k1 = bench.host_seqs(w.contig_codes())
    ref_seqs, k2 = bench.host_seqs([w.ref.cpu().numpy()])
    ctg_len = [e - s for s, e, _ in w.ctgs]
    g2r = w.g2r.cpu().numpy()
    alns = [(c, 0, int(g2r[s]), int(g2r[e - 1]) + 1) for c, (s, e, _) in enumerate(w.ctgs)]
    orient = [0 if r else 1 for _, _, r in w.ctgs]

    def make_handle():
        err = C.c_int()
        g = hip.pag_create_from_bitmap(w.solid_bits.data_ptr(), w.n_solid, sp.k, 1, 0, C.byref(err))
        assert g, hip.pag_last_error()
        return g

    return dict(hip=hip, host=host, sp=sp, w=w, inp=inp, ctg_seqs=ctg_seqs, ref_seqs=ref_seqs, keep=(k1, k2), ctg_len=ctg_len, alns=alns,
                orient=orient, make_handle=make_handle)


@pytest.mark.gpu
@pytest.mark.parametrize("n_ranks", [2, 4])
def test_run_native_equals_the_prototype(n_ranks, big, workdir):
    from aligngraph2_amd import rank_serial
    sp, w = big["sp"], big["w"]
    kw = dict(n_ranks=n_ranks, eps=sp.eps, k=sp.k, threads=sp.threads, ctgs=big["ctg_len"], ctg_alns=big["alns"], ref_lens=[len(w.ref)],
              ctg_seqs=big["ctg_seqs"], ref_seqs=big["ref_seqs"], orient=big["orient"], device="cuda:0", halo=60_000)
    proto = rank_serial.run(big["hip"], big["host"], big["make_handle"], big["inp"], out_dir=str(workdir / f"sn{n_ranks}_proto"), **kw)
    native = rank_serial.run_native(big["hip"], big["host"], big["make_handle"], big["inp"], out_dir=str(workdir / f"sn{n_ranks}_native"), **kw)
    print({kk: [round(r[kk], 3) for r in native["ranks"]] for kk in ("held_fraction", "s_recompute_extract", "s_recompute_build", "s_turn")},
          "prototype s_total", round(proto["s_total"], 2), "native s_total", round(native["s_total"], 2))
    assert native["outputs_sha256"] == proto["outputs_sha256"]
    assert native["count_lines_sum_over_owners"] == proto["count_lines_sum_over_owners"]
    assert (native["path_nodes"], native["path_bases"]) == (proto["path_nodes"], proto["path_bases"])
    assert native["vertices_total"] == proto["vertices_total"]
    for d in range(n_ranks):
        assert (native["ranks"][d]["held_vertices"], native["ranks"][d]["held_edges"]) == (proto["ranks"][d]["held_vertices"], proto["ranks"][d]["held_edges"]), d
        assert native["ranks"][d]["path_nodes"] == proto["ranks"][d]["path_nodes"], d
    assert max(r["held_fraction"] for r in native["ranks"]) < 1.0 / n_ranks + 0.15


@pytest.mark.gpu
def test_a_turn_without_turn_zero_and_bad_rank_counts_are_refused(big):
    hip = big["hip"]
    n = 2
    deal = parallel.deal_contigs(big["ctg_len"], n, ref_begin=[a[2] for a in big["alns"]])
    regions = parallel.regions_for(deal, big["ctg_len"], big["orient"], big["alns"], [len(big["w"].ref)], halo=60_000)
    arr = (capi.Region * n)(*[d["region"] for d in regions])
    g = big["make_handle"]()
    try:
        tot, st = capi.BuildStats(), capi.SerialStats()
        assert hip.pag_shard_run_serial(C.c_void_p(g), C.byref(big["inp"]), arr, n, 1, C.byref(tot), C.byref(st)) == capi.PAG_EINVAL
        assert b"turn 0" in hip.pag_last_error()
        for bad_n, turn in ((3, 0), (1, 0), (16, 0), (2, 2)):
            assert hip.pag_shard_run_serial(C.c_void_p(g), C.byref(big["inp"]), arr, bad_n, turn, C.byref(tot), C.byref(st)) == capi.PAG_EINVAL
    finally:
        hip.pag_destroy(C.c_void_p(g))  # (a refused call leaves the handle destroyable)


# ------------------------------------------------------------------------------------------------------------------------------
# one turn = one rank of the sharded build (the helper pattern of tests/test_gpu_shards.py, restated for a prepared golden)
# ------------------------------------------------------------------------------------------------------------------------------
def _csr(hip, g):
    nn, npos, ne = C.c_uint64(), C.c_uint64(), C.c_uint64()
    hip.pag_csr_sizes(C.c_void_p(g), C.byref(nn), C.byref(npos), C.byref(ne))
    arrs = {"node_code": np.zeros(nn.value + 1, np.uint32), "pos_off": np.zeros(nn.value + 1, np.uint64),
            "pos_ctg": np.zeros(npos.value + 1, np.uint32), "pos_ref": np.zeros(npos.value + 1, np.uint32),
            "pos_cnt": np.zeros(npos.value + 1, np.uint16), "edge_off": np.zeros(nn.value + 1, np.uint64),
            "edge_to": np.zeros(ne.value + 1, np.uint32), "edge_step": np.zeros(ne.value + 1, np.int32)}
    csr = capi.Csr(nn.value, npos.value, ne.value, *[arrs[k].ctypes.data for k in ("node_code", "pos_off", "pos_ctg", "pos_ref", "pos_cnt",
                                                                                  "edge_off", "edge_to", "edge_step")])
    assert hip.pag_export_csr(C.c_void_p(g), C.byref(csr)) == 0, hip.pag_last_error()
    return (nn.value, npos.value, ne.value), arrs


def _emulated_ranks(hip, make_handle, inp, n, regions, eps):
    """N handles play the N ranks: extract + partition, the exchange by slicing, K2-K4, every selection, the imports.
    -> the handles (handle d holds rank d's region) and the count lines"""
    gs = [make_handle() for _ in range(n)]
    sbs = [parallel.ShardedBuild(hip, g, inp, r, n, "cuda") for r, g in enumerate(gs)]
    ext = [sb.extract() for sb in sbs]
    allc = np.stack([e[0] for e in ext])
    slices, stats = [], []
    for r, sb in enumerate(sbs):
        rt, t1 = parallel.exchange_stream(ext[r][1], allc[:, :, 0:2], r, n, peers=[e[1] for e in ext])
        re_, e1 = parallel.exchange_stream(ext[r][2], allc[:, :, 2:4], r, n, peers=[e[2] for e in ext])
        sb.build(rt, t1, re_, e1, eps)
        sl, st = zip(*[sb.select(regions[d]) for d in range(n)])
        slices.append(sl)
        stats.append(st)
    totals = []
    for d, sb in enumerate(sbs):
        totals.append(sb.import_all([slices[o][d] for o in range(n)], [stats[o][d] for o in range(n)]))
        sb.set_region(regions[d])
    return gs, totals


def _golden_regions(inp, n):
    """regions over a golden's block: its selected contigs dealt round-robin, contig c's band a stretch of the first reference
    that depends on c (the walks are not run here: the regions only have to differ from rank to rank and cut the graph)"""
    raw = C.cast(inp.raw_view, C.POINTER(capi.PagRawInput)).contents
    ctg_len = [int(x) for x in np.ctypeslib.as_array(C.cast(raw.ctg_len, C.POINTER(C.c_uint32)), (raw.n_ctgs,))]
    ref_len = [int(x) for x in np.ctypeslib.as_array(C.cast(raw.ref_len, C.POINTER(C.c_uint32)), (raw.n_refs,))]
    sel = np.ctypeslib.as_array(C.cast(raw.ctg_selected, C.POINTER(C.c_uint8)), (raw.n_ctgs,))
    fwd = np.ctypeslib.as_array(C.cast(raw.ctg_forward, C.POINTER(C.c_uint8)), (raw.n_ctgs,))
    orient = [(1 if fwd[c] else 0) if sel[c] else -1 for c in range(len(ctg_len))]
    chosen = [c for c in range(len(ctg_len)) if sel[c]]
    deal = [[c for i, c in enumerate(chosen) if i % n == r] for r in range(n)]
    third = ref_len[0] // 3
    alns = [(c, 0, (i % 3) * third, (i % 3) * third + third // 2) for i, c in enumerate(chosen)]
    return parallel.regions_for(deal, ctg_len, orient, alns, ref_len, halo=50)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 4])
def test_one_turn_holds_what_a_rank_of_the_sharded_build_holds(n, workdir):
    name = "three_ctg_multi_t4"
    hip = capi.bind(pagctl.hip_lib())
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / f"turn_rank_{n}" / "in"))
    inp = pagctl.LoadedInput(ind, threads=spec["threads"], eps=spec["epsilon"], cov=spec["cov"])
    handles = []

    def make_handle():
        handles.append(pagctl.hip_create(inp))
        return handles[-1]

    try:
        g = make_handle()
        prepared = pagctl._prepared_view(hip, g, inp)  # (device arrays that belong to g: the turns must leave them alone)
        regions = _golden_regions(inp, n)
        arr = (capi.Region * n)(*[d["region"] for d in regions])
        gs, totals = _emulated_ranks(hip, make_handle, prepared, n, regions, prepared.eps)
        want = [_csr(hip, gr) for gr in gs]
        assert len({w[0] for w in want}) > 1 or n == 1, "the regions do not differ: the test would not tell the turns apart"
        g2 = make_handle()  # (the other way to an owner's records: partition + copy)
        for d in range(n):
            tot, st = capi.BuildStats(), capi.SerialStats()
            assert hip.pag_shard_run_serial(C.c_void_p(g), C.byref(prepared), arr, n, d, C.byref(tot), C.byref(st)) == 0, hip.pag_last_error()
            sizes, got = _csr(hip, g)
            assert sizes == want[d][0], f"turn {d}"
            for kk in got:
                assert np.array_equal(got[kk], want[d][1][kk]), f"turn {d}: CSR array {kk} differs from rank {d} of the sharded build"
            assert tot.counts() == totals[d].counts()
            assert (st.held_vertices, st.held_edges) == (sizes[1], sizes[2])
            assert st.tuples_in == sum(totals[d].n_tuples) and st.edges_in == sum(totals[d].n_edges)
            tot2, st2 = capi.BuildStats(), capi.SerialStats()
            assert hip.pag_debug_shard_run_serial(C.c_void_p(g2), C.byref(prepared), arr, n, d, C.byref(tot2), C.byref(st2), 1) == 0, hip.pag_last_error()
            sizes2, got2 = _csr(hip, g2)
            assert sizes2 == sizes and all(np.array_equal(got2[kk], got[kk]) for kk in got)
            assert (st2.tuples_in, st2.edges_in, st2.region_bytes) == (st.tuples_in, st.edges_in, st.region_bytes)
    finally:
        for h in handles:
            hip.pag_destroy(C.c_void_p(h))
        inp.close()


# ------------------------------------------------------------------------------------------------------------------------------
# pag_shard_extract_for = pag_shard_extract_range + pag_shard_take_part of the owner's two stretches
# ------------------------------------------------------------------------------------------------------------------------------
def _extract_both_ways(hip, g, inp, n_reads, n, ranges):
    import torch
    dev = "cuda"
    for lo, hi in ranges:
        counts = (C.c_uint64 * (4 * n))()
        for o in range(n):
            # the partition, then the owner's stretches ([its pass 1][its pass 2], owners ascending)
            assert hip.pag_shard_extract_range(C.c_void_p(g), C.byref(inp), lo, hi, n, counts) == 0, hip.pag_last_error()
            c = np.array(list(counts), dtype=np.int64).reshape(n, 4)
            t_n, e_n = int(c[o, 0] + c[o, 1]), int(c[o, 2] + c[o, 3])
            t_off, e_off = int(c[:o, 0:2].sum()), int(c[:o, 2:4].sum())
            want = [torch.zeros(t_n, dtype=torch.int32, device=dev), torch.zeros(t_n, dtype=torch.int64, device=dev),
                    torch.zeros(e_n, dtype=torch.int32, device=dev), torch.zeros(e_n, dtype=torch.int64, device=dev)]
            assert hip.pag_shard_take_part(C.c_void_p(g), t_off, t_n, want[0].data_ptr(), want[1].data_ptr(), e_off, e_n, want[2].data_ptr(),
                                           want[3].data_ptr()) == 0, hip.pag_last_error()
            # the compaction: pass 1 at slot 3, pass 2 right behind it at the far end of a buffer with 5 spare slots around them
            t_cap, e_cap = t_n + 8, e_n + 8
            got = [torch.full((t_cap,), -7, dtype=torch.int32, device=dev), torch.full((t_cap,), -7, dtype=torch.int64, device=dev),
                   torch.full((e_cap,), -7, dtype=torch.int32, device=dev), torch.full((e_cap,), -7, dtype=torch.int64, device=dev)]
            t_at1, t_at2, e_at1, e_at2 = 3, 3 + int(c[o, 0]) + 2, 3, 3 + int(c[o, 2]) + 2
            four = (C.c_uint64 * 4)()
            assert hip.pag_shard_extract_for(C.c_void_p(g), C.byref(inp), lo, hi, n, o, got[0].data_ptr(), got[1].data_ptr(), t_cap, t_at1, t_at2,
                                             got[2].data_ptr(), got[3].data_ptr(), e_cap, e_at1, e_at2, four) == 0, hip.pag_last_error()
            torch.cuda.synchronize()
            assert list(four) == [int(x) for x in c[o]], (lo, hi, o)
            for arrs, w, at1, at2, n1, n2 in ((got[0:2], want[0:2], t_at1, t_at2, int(c[o, 0]), int(c[o, 1])),
                                              (got[2:4], want[2:4], e_at1, e_at2, int(c[o, 2]), int(c[o, 3]))):
                for a, b in zip(arrs, w):
                    assert torch.equal(a[at1:at1 + n1], b[:n1]) and torch.equal(a[at2:at2 + n2], b[n1:n1 + n2]), (lo, hi, o)
                    untouched = torch.ones_like(a, dtype=torch.bool)
                    untouched[at1:at1 + n1] = False
                    untouched[at2:at2 + n2] = False
                    assert bool((a[untouched] == -7).all()), (lo, hi, o)
            if hi > lo:
                assert c.sum() > 0
            # a destination that is too small is refused before anything is written
            if t_n:
                small = [torch.full((max(t_n - 1, 1),), -7, dtype=torch.int32, device=dev), torch.full((max(t_n - 1, 1),), -7, dtype=torch.int64, device=dev)]
                rc = hip.pag_shard_extract_for(C.c_void_p(g), C.byref(inp), lo, hi, n, o, small[0].data_ptr(), small[1].data_ptr(), t_n - 1, 0, int(c[o, 0]),
                                               got[2].data_ptr(), got[3].data_ptr(), e_cap, e_at1, e_at2, four)
                torch.cuda.synchronize()
                assert rc == capi.PAG_ERANGE and bool((small[0] == -7).all())


@pytest.mark.gpu
def test_extract_for_equals_partition_and_take_part_on_the_big_workload(big):
    hip = big["hip"]
    n_reads = big["sp"].n_reads
    g = big["make_handle"]()
    try:
        _extract_both_ways(hip, g, big["inp"], n_reads, 4, [(n_reads // 4, n_reads // 2), (100, 100), (0, 1)])
    finally:
        hip.pag_destroy(C.c_void_p(g))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_ctg_multi_t4", "two_blocks_both_orient_t16"])
def test_extract_for_equals_partition_and_take_part_on_goldens(name, workdir):
    hip = capi.bind(pagctl.hip_lib())
    spec = goldens.load_spec(name)
    ind = goldens.materialize_inputs(name, str(workdir / f"extract_for_{name}" / "in"))
    inp = pagctl.LoadedInput(ind, threads=spec["threads"], eps=spec["epsilon"], cov=spec["cov"])
    g = pagctl.hip_create(inp)
    try:
        prepared = pagctl._prepared_view(hip, g, inp)
        n_reads = int(prepared.reads.n_seqs)
        _extract_both_ways(hip, g, prepared, n_reads, 4, [(0, n_reads), (n_reads // 3, 2 * n_reads // 3), (n_reads, n_reads)])
    finally:
        hip.pag_destroy(C.c_void_p(g))
        inp.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the compaction through its hook, against numpy
# ------------------------------------------------------------------------------------------------------------------------------
def _pick(hip, key, val, n1, shift, owner, cap, at1, at2):
    out_key = np.full(cap, 0xDEADBEEF, dtype=np.uint32)
    out_val = np.full(cap, 0xFEEDFACECAFEF00D, dtype=np.uint64)
    counts = (C.c_uint64 * 2)()
    rc = hip.pag_debug_owner_pick(key.ctypes.data, val.ctypes.data, len(key), n1, shift, owner, out_key.ctypes.data, out_val.ctypes.data, cap, at1, at2,
                                  counts, 0)
    return rc, out_key, out_val, list(counts)


def _key_patterns(rng, n, n_owners, shift, owner):
    low = rng.integers(0, 1 << shift, size=n, dtype=np.uint64)
    others = [o for o in range(n_owners) if o != owner]
    yield "all one owner", np.full(n, owner, dtype=np.uint64) << np.uint64(shift) | low
    yield "no record of the owner", rng.choice(others, size=n).astype(np.uint64) << np.uint64(shift) | low
    yield "alternating owners", (np.arange(n, dtype=np.uint64) % np.uint64(n_owners)) << np.uint64(shift) | low
    runs = np.repeat(rng.integers(0, n_owners, size=n // (TILE + 300) + 2), TILE + 300)[:n].astype(np.uint64)  # runs longer than a tile
    yield "runs longer than a tile", runs << np.uint64(shift) | low
    yield "random", rng.integers(0, n_owners, size=n).astype(np.uint64) << np.uint64(shift) | low


@pytest.mark.gpu
@pytest.mark.parametrize("n_owners", [2, 4, 8])
def test_compaction_equals_numpy(n_owners):
    hip = capi.bind(pagctl.hip_lib())
    rng = np.random.default_rng(n_owners)
    shift = 28 - {2: 1, 4: 2, 8: 3}[n_owners]  # k = 14
    checked = 0
    for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17):
        val = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)  # unique: a misplaced record shows
        assert len(np.unique(val)) == n
        n1s = sorted({x for x in (0, n, 1, 64, 64 + 37, TILE // 2 + 5, TILE, 2 * TILE) if x <= n})
        for owner in sorted({0, n_owners - 1, n_owners // 2}):
            for label, key64 in _key_patterns(rng, n, n_owners, shift, owner):
                key = np.ascontiguousarray(key64, dtype=np.uint32)
                hit = (key >> np.uint32(shift)) == owner
                for n1 in n1s:
                    idx1, idx2 = np.flatnonzero(hit[:n1]), n1 + np.flatnonzero(hit[n1:])
                    at1, at2 = 5, 5 + len(idx1) + 3
                    cap = at2 + len(idx2) + 4
                    rc, ok, ov, counts = _pick(hip, key, val, n1, shift, owner, cap, at1, at2)
                    what = f"{n_owners} owners, n = {n}, n1 = {n1}, owner {owner}, {label}"
                    assert rc == 0, what + ": " + hip.pag_last_error().decode()
                    assert counts == [len(idx1), len(idx2)], what
                    want_k = np.full(cap, 0xDEADBEEF, dtype=np.uint32)
                    want_v = np.full(cap, 0xFEEDFACECAFEF00D, dtype=np.uint64)
                    want_k[at1:at1 + len(idx1)], want_v[at1:at1 + len(idx1)] = key[idx1], val[idx1]
                    want_k[at2:at2 + len(idx2)], want_v[at2:at2 + len(idx2)] = key[idx2], val[idx2]
                    assert np.array_equal(ok, want_k) and np.array_equal(ov, want_v), what  # (also: nothing outside the two stretches was touched)
                    checked += 1
    assert checked > 300


@pytest.mark.gpu
def test_compaction_refuses_what_does_not_fit_and_writes_nothing():
    hip = capi.bind(pagctl.hip_lib())
    n, shift = TILE + 100, 26
    key = np.full(n, 1 << shift, dtype=np.uint32)
    val = np.arange(n, dtype=np.uint64)
    for cap, at1, at2 in ((n - 1, 0, 70), (n, 0, 60), (n + 10, 0, n)):  # too small; the stretches run into each other; pass 2 past the end
        rc, ok, ov, counts = _pick(hip, key, val, 70, shift, 1, cap, at1, at2)
        assert rc == capi.PAG_ERANGE and counts == [70, n - 70], (cap, at1, at2)
        assert (ok == 0xDEADBEEF).all() and (ov == 0xFEEDFACECAFEF00D).all()
    rc, _, _, _ = _pick(hip, key, val, n + 1, shift, 1, n, 0, 0)
    assert rc == capi.PAG_EINVAL
    rc, _, _, _ = _pick(hip, key, val, 0, 32, 1, n, 0, 0)
    assert rc == capi.PAG_EINVAL
