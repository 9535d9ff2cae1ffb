"""GPU: pag_successors_batch (csrc/hip/k_succ_query.hip) — successor lists on demand from the finished graph.

Every test builds its graph with pag_process alone (or imports a constructed one): no pag_travel_prepare* unless the test is
about the call beside one.

  1. every vertex of every golden block in ONE call at the reference's own parameters (deviation 2 * epsilon, error rate 0.15)
     against tests/golden/<case>/succ.txt.gz, record for record and in order;
  2. the caller's parameters — deviations and error rates no golden covers — against tests/succ_rule.py, which
     tests/test_succ_rule.py holds to the same dumps;
  3. the shapes of a call: list lengths around the wave width, repeated and reversed queries, vertices that do not exist, a buffer
     one record short, the sizing call, candidate-pair counts around one and two turns of the lanes;
  4. the call leaves the handle as it found it;
  5. a regional handle is refused;
  6. a constructed graph (pag_shard_import) for what no golden holds: k-mers with more than 64 edges (a second turn of the edge
     loop), exactly 64 and 65, targets the graph lacks, candidate-pair counts of exactly 128."""
import ctypes as C
import functools

import numpy as np
import pytest

import goldens
import pagctl  # (puts the repository root on the path)
import succ_rule
import aligngraph2_amd as ag
from aligngraph2_amd import capi
from aligngraph2_amd.capi import BuildStats, PagRawInput, PagSeqs, PagSucc, PagSuccQuery, Region, ShardSlice, TravelParams
from test_gpu_succ_golden import block_orient, device_records

Q_DTYPE, REC_DTYPE = np.dtype(PagSuccQuery), np.dtype(PagSucc)


@functools.lru_cache(maxsize=None)
def golden(name):
    """per config block: the graph dump, the reference's dump, the dump's vertices as ids / codes / positions, their lists as
    (target code, target position, step, grade, ctg-similar) rows"""
    out = []
    for g, d in zip(succ_rule.load_graph(name), succ_rule.reference_dump(name)):
        vpos = (g["ctg"].astype(np.uint64) << np.uint64(32)) | g["ref"].astype(np.uint64)
        vcode = g["code"][g["node_of_vertex"]].astype(np.uint32)
        v = succ_rule.vertex_ids(g, d["key"][:, 0], d["key"][:, 1])
        t = succ_rule.vertex_ids(g, d["rec"][:, 0], d["rec"][:, 1])
        out.append({"g": g, "vpos": vpos, "vcode": vcode, "v": v, "off": d["off"], "rows": rows_of(vcode, vpos, t, d["rec"][:, 2], d["rec"][:, 3], d["rec"][:, 4])})
    return out


def rows_of(vcode, vpos, target, step, grade, esim):
    rec = np.zeros(len(target), dtype=REC_DTYPE)
    rec["code"], rec["pos"], rec["step"], rec["grade"], rec["ctg_similar"] = vcode[target], vpos[target], step, grade, esim
    return rec


def lists_of(off, rows, pick):
    """(off, rows) of the lists `pick` out of a list of lists"""
    cnt = (off[1:] - off[:-1])[pick]
    idx = np.repeat(off[:-1][pick] - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
    return np.concatenate(([0], np.cumsum(cnt))).astype(np.int64), rows[idx]


class Built:
    """a golden block's graph in a fresh handle: pag_prepare + pag_process, nothing else"""

    def __init__(self, name, block, workdir):
        self.hip = pagctl.hip_lib()
        self.spec = goldens.load_spec(name)
        self.ind = goldens.materialize_inputs(name, str(workdir / "succ_query" / name / "in"))
        self.block = block
        self.inp = pagctl.LoadedInput(self.ind, threads=self.spec["threads"], eps=self.spec["epsilon"], cov=self.spec["cov"], block=block)
        self.g = None

    def __enter__(self):
        self.g = C.c_void_p(pagctl.hip_create(self.inp))
        self.prepared = pagctl._prepared_view(self.hip, self.g, self.inp)
        self.process()
        return self

    def process(self):
        st = BuildStats()
        assert self.hip.pag_process(self.g, C.byref(self.prepared), C.byref(st)) == 0, self.hip.pag_last_error()

    def travel_args(self):
        raw = PagRawInput.from_address(self.inp.raw_view)
        self.ctg_len = np.ctypeslib.as_array(C.cast(raw.ctg_len, C.POINTER(C.c_uint32)), shape=(raw.n_ctgs,)).copy()
        self.ref_len = np.ctypeslib.as_array(C.cast(raw.ref_len, C.POINTER(C.c_uint32)), shape=(raw.n_refs,)).copy()
        ctgs = PagSeqs(raw.n_ctgs, None, self.ctg_len.ctypes.data, None, 0)
        prm = TravelParams(self.spec["threads"], 0, 2 * self.spec["epsilon"], 0.15, 0.90, 50)
        return ctgs, prm

    def __exit__(self, *exc):
        if self.g:
            self.hip.pag_destroy(self.g)
        self.inp.close()


def raw_call(hip, g, codes, pos, deviation, err, cap):
    """the C call itself: (rc, off, status, out, n_total, ms_kernels)"""
    q = np.zeros(len(codes), dtype=Q_DTYPE)
    q["code"], q["pos"] = codes, pos
    off = np.full(len(codes) + 1, 0xDEAD, dtype=np.uint64)
    status = np.full(len(codes), 77, dtype=np.int32)
    out = np.zeros(cap, dtype=REC_DTYPE)
    total, ms = C.c_uint64(12345), C.c_double(-1.0)
    rc = hip.pag_successors_batch(g, q.ctypes.data, len(q), deviation, err, off.ctypes.data, status.ctypes.data, out.ctypes.data if cap else None, cap,
                                  C.byref(total), C.byref(ms))
    return rc, off.astype(np.int64), status, out, total.value, ms.value


def assert_lists(label, got_off, got_rec, want_off, want_rec):
    assert np.array_equal(got_off.astype(np.int64), want_off), \
        f"{label}: list lengths differ, first at query {int(np.flatnonzero(np.diff(got_off.astype(np.int64)) != np.diff(want_off))[0])}"
    assert len(got_rec) == len(want_rec)
    for f in REC_DTYPE.names:
        bad = np.flatnonzero(got_rec[f] != want_rec[f])
        assert len(bad) == 0, f"{label}: field {f} differs in {len(bad)} records, first {int(bad[0])}: {got_rec[bad[0]]} for {want_rec[bad[0]]}"


# ---- 1. the whole graph against the reference's dumps ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", goldens.case_names())
def test_every_list_of_the_graph_equals_the_reference_s_dump(name, workdir):
    for block, ref in enumerate(golden(name)):
        with Built(name, block, workdir) as b:
            v = ref["v"]
            assert len(v) == len(ref["vpos"]), "the dump holds every vertex"
            off, status, rec = ag.successors_batch(b.hip, b.g, ref["vcode"][v], ref["vpos"][v], 2 * b.spec["epsilon"], 0.15)
            assert not status.any(), f"{name} block {block}: {np.count_nonzero(status)} vertices of the dump are not in the graph"
            assert int(off[-1]) == len(ref["rows"]) == len(rec)
            assert_lists(f"{name} block {block}", off, rec, ref["off"], ref["rows"])
            assert b.hip.pag_successors(b.g, 0, 0, None, 0) == -22  # (nothing was prepared, and nothing is now)
    if name == "succ_corners_t8":
        g = golden(name)[0]["g"]
        assert np.diff(g["pos_off"]).max() > 255, "no k-mer with more than 255 positions"
        assert succ_rule.candidate_pairs(g).max() > 64, "no vertex with more than one turn of candidate pairs"
        assert golden(name)[0]["rows"]["step"].max() >= 1024, "no record with a step of 1024 or more"
        assert np.diff(g["child_off"]).max() > 6, "no k-mer whose edges' targets are looked up one per lane"


# ---- 2. the caller's parameters -----------------------------------------------------------------------------------------------
PARAMS = [(0, 0.15), (0, 0.0), (200, 0.15), (None, 0.4)]  # (None: 2 * epsilon)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["extend_gap_t1", "eps20_k11_jitter_t16"])
def test_the_caller_s_deviation_and_error_rate_decide(name, workdir):
    ref = golden(name)[0]
    cnt = np.diff(ref["off"])
    order = np.argsort(-cnt, kind="stable")
    pick = np.concatenate((order[:40], order[-20:], np.random.default_rng(11).choice(len(cnt), size=5000, replace=False)))
    v = ref["v"][pick]
    lengths = {}
    with Built(name, 0, workdir) as b:
        for dev, err in PARAMS:
            dev = 2 * b.spec["epsilon"] if dev is None else dev
            w_off, w = succ_rule.successors(ref["g"], v, dev, err)
            want = rows_of(ref["vcode"], ref["vpos"], w[:, 0], w[:, 1], w[:, 2], w[:, 3])
            off, status, rec = ag.successors_batch(b.hip, b.g, ref["vcode"][v], ref["vpos"][v], dev, err)
            assert not status.any()
            assert_lists(f"{name} deviation {dev} error rate {err}", off, rec, w_off, want)
            lengths[(dev, err)] = len(rec)
    # the cases tell the parameters apart (by the rule, whatever the device says): the deviation moves the lists on both
    # goldens, the error rate at deviation 0 does
    eps2 = 2 * goldens.load_spec(name)["epsilon"]
    assert lengths[(0, 0.15)] != lengths[(eps2, 0.4)] and lengths[(200, 0.15)] != lengths[(0, 0.15)], lengths
    assert lengths[(0, 0.0)] != lengths[(0, 0.15)], lengths


# ---- 3. shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_shapes_of_a_call(workdir):
    name = "succ_corners_t8"
    ref = golden(name)[0]
    g, codes, pos, v_all = ref["g"], ref["vcode"], ref["vpos"], ref["v"]
    with Built(name, 0, workdir) as b:
        dev = 2 * b.spec["epsilon"]
        for n in (0, 1, 63, 64, 65, 257):
            rc, off, status, out, total, ms = raw_call(b.hip, b.g, codes[v_all[:n]], pos[v_all[:n]], dev, 0.15, int(ref["off"][n]))
            assert rc == 0, (n, b.hip.pag_last_error())
            assert total == ref["off"][n] and not status.any()
            assert_lists(f"{n} queries", off, out, ref["off"][:n + 1], ref["rows"][:ref["off"][n]])
            assert ms >= 0.0 and (n == 0 or ms > 0.0)
        # the same vertex three times; the dump's order reversed; the first and the last k-mer of the graph
        first, last = int(np.flatnonzero(codes[v_all] == codes.min())[0]), int(np.flatnonzero(codes[v_all] == codes.max())[-1])
        long_one = int(np.argmax(np.diff(ref["off"])))
        for label, pick in (("three times", np.array([long_one, 5, long_one, long_one])), ("reversed", np.arange(300)[::-1]), ("ends", np.array([first, last]))):
            w_off, want = lists_of(ref["off"], ref["rows"], pick)
            off, status, rec = ag.successors_batch(b.hip, b.g, codes[v_all[pick]], pos[v_all[pick]], dev, 0.15)
            assert not status.any()
            assert_lists(label, off, rec, w_off, want)
        # vertices the graph does not hold: a k-mer it lacks (below, between and above its k-mers), a k-mer at a position it does not have
        have = set(int(c) for c in g["code"])
        absent = [c for c in (0, int(g["code"].min()) + 1, int(g["code"].max()) + 1, 4 ** b.inp.k - 1) if c not in have]
        assert len(absent) >= 2
        mix_c = np.concatenate((codes[v_all[:3]], np.array(absent, dtype=np.uint32), codes[v_all[3:6]], codes[v_all[6:7]]))
        mix_p = np.concatenate((pos[v_all[:3]], np.full(len(absent), pos[v_all[0]]), pos[v_all[3:6]] + np.uint64(1 << 40), pos[v_all[6:7]]))
        held = set(zip(codes.tolist(), pos.tolist()))
        assert not any((int(c), int(p)) in held for c, p in zip(mix_c[3:-1], mix_p[3:-1]))
        rc, off, status, out, total, ms = raw_call(b.hip, b.g, mix_c, mix_p, dev, 0.15, int(ref["off"][7]))
        assert rc == 0, b.hip.pag_last_error()
        n_bad = len(absent) + 3
        assert status.tolist() == [0] * 3 + [-22] * n_bad + [0]
        pick = np.array([0, 1, 2, 6])
        w_off, want = lists_of(ref["off"], ref["rows"], pick)
        assert np.array_equal(np.diff(off), np.concatenate((np.diff(w_off)[:3], np.zeros(n_bad, dtype=np.int64), np.diff(w_off)[3:])))
        assert_lists("beside missing vertices", np.concatenate(([0], np.cumsum(np.diff(off)[[0, 1, 2, -1]]))), out[:total], w_off, want)
        # a buffer one record short: PAG_ERANGE, off[] complete; the sizing call gives the same off[]
        n = 257
        want_off = ref["off"][:n + 1]
        rc, off, status, out, total, ms = raw_call(b.hip, b.g, codes[v_all[:n]], pos[v_all[:n]], dev, 0.15, int(want_off[-1]) - 1)
        assert rc == -34 and total == want_off[-1] and np.array_equal(off, want_off) and not status.any()
        assert not out.view(np.uint8).any(), "records were written although the buffer was too small"
        rc, off, status, out, total, ms = raw_call(b.hip, b.g, codes[v_all[:n]], pos[v_all[:n]], dev, 0.15, 0)
        assert rc == -34 and total == want_off[-1] and np.array_equal(off, want_off)
        # candidate-pair counts around one and two turns of the lanes, wherever the golden has them
        pairs = succ_rule.candidate_pairs(g)[v_all]
        found = []
        for n_pairs in (63, 64, 65, 128, 129):
            pick = np.flatnonzero(pairs == n_pairs)[:8]
            if len(pick):
                found.append(n_pairs)
                w_off, want = lists_of(ref["off"], ref["rows"], pick)
                off, status, rec = ag.successors_batch(b.hip, b.g, codes[v_all[pick]], pos[v_all[pick]], dev, 0.15)
                assert_lists(f"{n_pairs} candidate pairs", off, rec, w_off, want)
        assert found == [63, 64, 65, 129], found  # (128: test_constructed_graph_with_many_edges)


def test_arguments_are_checked_before_a_device_is_touched():
    """(runs without a GPU; a handle that holds no graph yet: test_constructed_graph_with_many_edges)"""
    hip = pagctl.hip_lib()
    total = C.c_uint64(5)
    off = np.zeros(2, dtype=np.uint64)
    assert hip.pag_successors_batch(None, None, 0, 0, 0.15, off.ctypes.data, None, None, 0, C.byref(total), None) == -22
    assert b"null" in hip.pag_last_error()
    assert total.value == 0
    assert hip.pag_successors_batch_bytes(0, 0) == 0
    assert hip.pag_successors_batch_bytes(1000, 10) >= 1000 * (16 + 8 + 4 + 4) + 10 * 24


# ---- 4. the handle is left alone ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_call_leaves_the_handle_alone(workdir, monkeypatch):
    for s in ("PAG_SUCC_HEAVY", "PAG_TRAVEL_VIEW", "PAG_VIEW_HALO", "PAG_VIEW_MARGIN"):
        monkeypatch.delenv(s, raising=False)
    name = "extend_gap_t1"
    ref = golden(name)[0]
    v = ref["v"]
    with Built(name, 0, workdir) as b:
        hip, g = b.hip, b.g
        ctgs, prm = b.travel_args()
        dev = 2 * b.spec["epsilon"]

        def prepare():
            assert hip.pag_travel_prepare(g, C.byref(ctgs), b.ref_len.ctypes.data, len(b.ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
            return device_records(hip, g)

        plain = prepare()
        b.process()
        first = ag.successors_batch(hip, g, ref["vcode"][v], ref["vpos"][v], dev, 0.15)
        for a, c in zip(plain, prepare()):
            assert np.array_equal(a, c), "pag_travel_prepare builds other records after a batch call"
        assert hip.pag_successors(g, int(ref["vcode"][v[0]]), int(ref["vpos"][v[0]]), None, 0) == ref["off"][1]
        again = ag.successors_batch(hip, g, ref["vcode"][v], ref["vpos"][v], dev, 0.15)  # (beside a prepared whole view)
        for a, c in zip(prepare(), plain):
            assert np.array_equal(a, c)
        names = [ln[1:].split()[0] for ln in open(f"{b.ind}/ctg.fasta") if ln.startswith(">")]
        orient = block_orient(b.ind, 0, names)
        b.process()
        assert hip.pag_travel_prepare_for(g, C.byref(ctgs), orient.ctypes.data, b.ref_len.ctypes.data, len(b.ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
        cut = device_records(hip, g)
        beside_cut = ag.successors_batch(hip, g, ref["vcode"][v], ref["vpos"][v], dev, 0.15)  # (pag_successors answers -34 here)
        assert hip.pag_successors(g, int(ref["vcode"][v[0]]), int(ref["vpos"][v[0]]), None, 0) == -34
        for a, c in zip(cut, device_records(hip, g)):
            assert np.array_equal(a, c)
        for other in (again, beside_cut):
            for a, c in zip(first, other):
                assert np.array_equal(a, c)
        assert_lists("after pag_travel_prepare_for", beside_cut[0], beside_cut[2], ref["off"], ref["rows"])


# ---- 5. a regional handle -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_regional_handle_is_refused(workdir):
    ref = golden("extend_gap_t1")[0]
    with Built("extend_gap_t1", 0, workdir) as b:
        riv, ropen = np.array([1, 1000], dtype=np.uint32), np.array([0, 1], dtype=np.uint8)
        assert b.hip.pag_shard_set_region(b.g, C.byref(Region(0, None, 1, riv.ctypes.data, ropen.ctypes.data))) == 0
        rc, off, status, out, total, ms = raw_call(b.hip, b.g, ref["vcode"][:4], ref["vpos"][:4], 20, 0.15, 64)
        assert rc == -34 and total == 0 and b"region" in b.hip.pag_last_error()
        with pytest.raises(RuntimeError):
            ag.successors_batch(b.hip, b.g, ref["vcode"][:4], ref["vpos"][:4], 20, 0.15)


# ---- 6. a constructed graph ---------------------------------------------------------------------------------------------------
def constructed_graph(rng, k=9):
    """a graph in succ_rule's form whose hubs have 64, 65, 130 and 200 edges, with targets of 1..5 positions and targets that are
    no k-mer of the graph; positions near where a step would put them, some without a contig or a reference coordinate"""
    n_nodes = 400
    code = np.sort(rng.choice(4 ** k, size=n_nodes, replace=False)).astype(np.int64)
    lacking = np.setdiff1d(rng.choice(4 ** k, size=40, replace=False), code)
    npos = rng.integers(1, 6, size=n_nodes)
    npos[:4] = 2  # the hubs' targets: 2 positions each where the pair count is to be exact
    pos_off = np.concatenate(([0], np.cumsum(npos)))
    base = rng.integers(1000, 1060, size=n_nodes)
    ctg = np.repeat(base, npos) + rng.integers(0, 60, size=pos_off[-1])
    ref = np.repeat(base, npos) + 5000 + rng.integers(0, 60, size=pos_off[-1])
    ctg[rng.random(len(ctg)) < 0.25] = 0
    ref[rng.random(len(ref)) < 0.15] = 0
    # distinct positions inside a k-mer
    for n in range(n_nodes):
        s = slice(pos_off[n], pos_off[n + 1])
        while len(set(zip(ctg[s].tolist(), ref[s].tolist()))) < npos[n]:
            ref[s] = ref[s] + np.arange(npos[n]) + 1
    n_child = rng.integers(0, 9, size=n_nodes)
    hubs = {10: 64, 20: 65, 30: 130, 40: 200, 50: 64}
    for h, n in hubs.items():
        n_child[h] = n
    child_off = np.concatenate(([0], np.cumsum(n_child)))
    child_code = code[rng.integers(0, n_nodes, size=child_off[-1])]
    miss = rng.random(len(child_code)) < 0.1
    child_code[miss] = rng.choice(lacking, size=int(miss.sum()))
    child_step = rng.integers(1, 80, size=len(child_code)).astype(np.uint32)
    s = slice(child_off[50], child_off[51])  # hub 50: 64 edges to k-mers of 2 positions each = exactly 128 candidate pairs
    child_code[s] = code[rng.integers(0, 4, size=64)]
    g = {"code": code, "pos_off": pos_off, "ctg": ctg.astype(np.uint32), "ref": ref.astype(np.uint32), "child_off": child_off, "child_code": child_code,
         "child_step": child_step, "node_of_vertex": np.repeat(np.arange(n_nodes), npos)}
    return g, hubs


def slice_arrays(g, rng):
    """the graph as pag_shard_import takes it: segments longer than their leaders / unique edges, fillers behind them"""
    tkey, tval, tseg, tcnt, ekey, ev, eseg = [], [], [], [], [], [], []
    vpos = (g["ctg"].astype(np.uint64) << np.uint64(32)) | g["ref"].astype(np.uint64)
    for n, c in enumerate(g["code"]):
        p = vpos[g["pos_off"][n]:g["pos_off"][n + 1]]
        extra = int(rng.integers(0, 4))
        tkey += [c] * (len(p) + extra)
        tval += p.tolist() + [int(p[0])] * extra
        tseg += [len(p)] + [0x80000000 | i for i in range(1, len(p))] + [0] * extra
        tcnt += [1] * len(p) + [0] * extra
        lo, hi = g["child_off"][n], g["child_off"][n + 1]
        if hi > lo:
            extra = int(rng.integers(0, 3))
            e = (g["child_code"][lo:hi].astype(np.uint64) << np.uint64(32)) | (g["child_step"][lo:hi].astype(np.uint64) << np.uint64(1)) | rng.integers(0, 2, size=hi - lo).astype(np.uint64)
            ekey += [c] * (hi - lo + extra)
            ev += e.tolist() + [int(e[0])] * extra
            eseg += [hi - lo] + [0] * (hi - lo - 1 + extra)
    return (np.array(tkey, dtype=np.uint32), np.array(tval, dtype=np.uint64), np.array(tseg, dtype=np.uint32), np.array(tcnt, dtype=np.uint16),
            np.array(ekey, dtype=np.uint32), np.array(ev, dtype=np.uint64), np.array(eseg, dtype=np.uint32))


@pytest.mark.gpu
def test_constructed_graph_with_many_edges():
    import torch
    rng = np.random.default_rng(64)
    g, hubs = constructed_graph(rng)
    pairs = succ_rule.candidate_pairs(g)
    assert (pairs == 128).any() and np.diff(g["child_off"]).max() == 200
    hip = pagctl.hip_lib()
    words = np.array([9, 1, 2, 3], dtype=np.uint64)
    err = C.c_int()
    h = C.c_void_p(hip.pag_create(words.ctypes.data, len(words), 9, 0, C.byref(err)))
    assert h, hip.pag_last_error()
    try:
        vcode = g["code"][g["node_of_vertex"]].astype(np.uint32)
        vpos = (g["ctg"].astype(np.uint64) << np.uint64(32)) | g["ref"].astype(np.uint64)
        rc, off, status, out, total, ms = raw_call(hip, h, vcode[:4], vpos[:4], 20, 0.15, 64)
        assert rc == -22 and total == 0 and b"no finished graph" in hip.pag_last_error()
        host = slice_arrays(g, rng)
        # (torch has no unsigned 32 / 64-bit tensors to copy from: the bytes go up)
        dev = [torch.from_numpy(a.view(np.uint8).copy()).cuda() for a in host]
        st = BuildStats()
        st.n_nodes, st.n_pos, st.n_uniq_edges = len(g["code"]), len(g["ctg"]), len(g["child_code"])
        sl = ShardSlice(len(host[0]), len(host[4]), *[t.data_ptr() for t in dev], st)
        assert hip.pag_shard_import(h, C.byref(sl), 1, None) == 0, hip.pag_last_error()
        v = np.arange(len(vcode))
        for deviation, rate in ((20, 0.15), (3, 0.05)):
            w_off, w = succ_rule.successors(g, v, deviation, rate)
            off, status, rec = ag.successors_batch(hip, h, vcode, vpos, deviation, rate)
            assert not status.any()
            assert_lists(f"constructed graph, deviation {deviation}", off, rec, w_off, rows_of(vcode, vpos, w[:, 0], w[:, 1], w[:, 2], w[:, 3]))
            for hub in hubs:  # (the lists behind the hubs' edges are not empty: the comparison above says something about them)
                lo, hi = g["pos_off"][hub], g["pos_off"][hub + 1]
                assert deviation != 20 or w_off[hi] > w_off[lo]
    finally:
        hip.pag_destroy(h)
