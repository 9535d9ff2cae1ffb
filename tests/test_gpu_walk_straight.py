"""GPU: pag_walk_straight_batch (csrc/hip/k_walk_query.hip) — walkStraight on demand from the finished graph, held to
tests/walk_straight_rule.py exactly: every path entry, abundance, status and alternative.  tests/test_walk_straight_rule.py holds
the rule itself to hand-written answers and to the reference's path dumps.

Every test builds its graph with pag_process alone (Built of test_gpu_succ_query.py) or imports a constructed one.

  1. replay: every walkStraight call graphTravel makes on the CPU for three dumps, with its round's frame, in ONE call per dump;
  2. graphTravel composed on the device — a host loop over the call — reproduces a dump's first 300 entries;
  3. the constructed graph of tests/walk_straight_cases.py: one case per line of the rule, the list loops' second turns, vertices
     the graph does not hold;
  4. the shapes of a call: no query, sizing calls, each buffer one short, a query named twice, frames sharing an excl slice,
     pag_walk_straight_batch_bytes;
  5. arguments are refused before a device is touched (no GPU needed); a regional handle;
  6. the call leaves the handle as it found it."""
import ctypes as C
import os

import numpy as np
import pytest

import find_rule
import goldens
import pagctl  # (puts the repository root on the path)
import walk_straight_cases as cases
import walk_straight_rule as rule
import aligngraph2_amd as ag
from aligngraph2_amd import capi
from aligngraph2_amd.capi import BuildStats, Region, ShardSlice
from test_gpu_find import delivered_paths, export
from test_gpu_succ_query import Built, golden, slice_arrays
from test_walk_straight_rule import BUILDER, CASES, constructed, first_round_travel, golden_lists

QUERY, FRAME, NODE, EXCL, ALT = capi.WALK_QUERY_DTYPE, capi.WALK_FRAME_DTYPE, capi.WALK_NODE_DTYPE, capi.SUCC_QUERY_DTYPE, capi.SUCC_DTYPE
OK, EINVAL, ERANGE = capi.PAG_OK, capi.PAG_EINVAL, capi.PAG_ERANGE


def arrays_of(calls, name_of):
    """calls [(Frame, start, dist, has_size, limit)] as the call's arrays: one frame and one excl slice per distinct Frame object,
    each slice the frame's set named by name_of (vertex -> (code, pos)) in ascending order"""
    q = np.zeros(len(calls), dtype=QUERY)
    frame_at, frames, slices, n_excl = {}, [], [], 0
    for i, (F, v, dist, has_size, limit) in enumerate(calls):
        if id(F) not in frame_at:
            frame_at[id(F)] = len(frames)
            ex = np.zeros(len(F.excl), dtype=EXCL)
            if len(F.excl):
                names = np.array(sorted(name_of(x) for x in F.excl), dtype=np.uint64)
                ex["code"], ex["pos"] = names[:, 0], names[:, 1]
            frames.append((F.ctg_left, F.ctg_right, F.rev_left, F.rev_right, F.split_size, F.leap_min, [F.hulls[0][0], F.hulls[1][0]],
                           [F.hulls[0][1], F.hulls[1][1]], n_excl, len(ex)))
            slices.append(ex)
            n_excl += len(ex)
        code, pos = name_of(v)
        q[i] = (code, dist, pos, has_size, frame_at[id(F)], limit)
    return q, np.array(frames, dtype=FRAME), (np.concatenate(slices) if slices else np.zeros(0, dtype=EXCL))


def answers(out):
    """(node_off, nodes, alt_off, alts, status) -> per query (path [(code, pos, step, abundance)], status, alts [(code, pos, step, grade, ctg-similar)])"""
    node_off, nodes, alt_off, alts, status = out
    res = []
    for i in range(len(status)):
        n, a = nodes[int(node_off[i]):int(node_off[i + 1])], alts[int(alt_off[i]):int(alt_off[i + 1])]
        res.append((list(zip(n["code"].tolist(), n["pos"].tolist(), n["step"].tolist(), n["abundance"].tolist())), int(status[i]),
                    list(zip(a["code"].tolist(), a["pos"].tolist(), a["step"].tolist(), a["grade"].tolist(), a["ctg_similar"].tolist()))))
    assert not nodes["reserved"].any()
    return res


def by_the_rule(L, calls, name_of):
    """the same calls answered by the rule, in the device's terms"""
    res = []
    for F, v, dist, has_size, limit in calls:
        path, status, alts = rule.walk_straight(L, F, v, dist, has_size, limit)
        res.append(([name_of(x) + (s, n) for x, s, n in path], status, [name_of(t) + (s, g, sim) for t, s, g, sim in alts]))
    return res


def assert_answers(label, got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], f"{label}: query {i} ended with status {g[1]}, the rule with {w[1]} (path of {len(g[0])} for {len(w[0])})"
        assert g[0] == w[0], f"{label}: query {i}: the paths differ, first at entry {next((j for j, (a, b) in enumerate(zip(g[0], w[0])) if a != b), min(len(g[0]), len(w[0])))}"
        assert g[2] == w[2], f"{label}: query {i}: the alternatives differ: {g[2]} for {w[2]}"


# ---- 1. replay ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,dump", [("join_rev_t16", "0_1_1"), ("eps5_k7_repeats_t8", "0_0_1"), ("three_ctg_multi_t4", "0_0_0")])
def test_replay_of_a_travel_s_walks_in_one_call(name, dump, workdir):
    block = rule.dumps_of(name)[0][dump][0]
    L, _ = golden_lists(name)[block]
    ref = golden(name)[block]
    name_of = lambda v: (int(ref["vcode"][v]), int(ref["vpos"][v]))  # noqa: E731
    log = []
    seq, _ = first_round_travel(name, dump, backend=rule.RuleBackend(L, log))
    want = by_the_rule(L, log, name_of)
    assert len(log) > 400 and len({id(c[0]) for c in log}) > 100, "the travel says too little"
    assert {w[1] for w in want} >= {rule.END, rule.BRANCH} and (name != "eps5_k7_repeats_t8" or any(w[1] == rule.LEAP for w in want))
    ctg_len = rule.dumps_of(name)[1]
    q, frames, excl = arrays_of(log, name_of)
    with Built(name, block, workdir) as b:
        got = answers(ag.walk_straight_batch(b.hip, b.g, q, frames, excl, ctg_len, 2 * b.spec["epsilon"], 0.15))
    assert_answers(f"{name} {dump}", got, want)


# ---- 2. graphTravel as a host loop over the call ----------------------------------------------------------------------------------------
class DeviceBackend:
    """graph_travel's questions answered by pag_walk_straight_batch: a vertex is (code, pos); the alternatives of a round go in one
    call; the classification of the last vertex is a walk of limit 2 from it (its own tables hold nothing the travel tables lack:
    alts for a Branch, the second entry for a single successor)"""

    def __init__(self, hip, g, ctg_len, deviation, error_rate):
        self.hip, self.g, self.ctg_len, self.deviation, self.error_rate, self.calls = hip, g, ctg_len, deviation, error_rate, 0

    def coord(self, v):
        return v[1] >> 32

    def ask(self, calls):
        self.calls += 1
        q, frames, excl = arrays_of(calls, lambda v: v)
        return answers(ag.walk_straight_batch(self.hip, self.g, q, frames, excl, self.ctg_len, self.deviation, self.error_rate))

    def walks(self, F, starts, limit):
        return [([((c, p), s, n) for c, p, s, n in path], status) for path, status, _ in self.ask([(F, v, d, h, limit) for v, d, h in starts])]

    def classify(self, F, u, total):
        path, status, alts = self.ask([(F, u, 0, total, 2)])[0]
        if status == rule.BRANCH:
            return [((c, p), s) for c, p, s, _, _ in alts]
        return [((c, p), s) for c, p, s, _ in path[1:]]


@pytest.mark.gpu
def test_graph_travel_composed_on_the_device_reproduces_the_dump(workdir):
    name, dump = "extend_gap_t1", "0_1_0"
    dumps, ctg_len = rule.dumps_of(name)
    block, contig, _, body, k = dumps[dump]
    want = [((c, (a << 32) | r), s) for c, a, r, _, s in body]
    base = rule.first_round_frame(ctg_len, contig, rule.strand_of(ctg_len, contig, body))
    with Built(name, block, workdir) as b:
        B = DeviceBackend(b.hip, b.g, ctg_len, 2 * b.spec["epsilon"], 0.15)
        seq = rule.graph_travel(B, base, want[0][0], k, stop_after=300)
    assert len(seq) >= 300 and B.calls > 20
    assert seq[:300] == want[:300], f"first difference at entry {next(i for i, (a, c) in enumerate(zip(seq, want)) if a != c)}"


# ---- 3. the constructed graph -----------------------------------------------------------------------------------------------------------
class Constructed:
    """the graph of tests/walk_straight_cases.py in a handle (pag_shard_import; test_gpu_find.import_graph gives a graph one
    edge: this one needs its edges, and its counts in tcnt)"""

    def __init__(self, L=None, ctg_len=cases.CTG_LEN, moved=None):
        """L: the same graph's lists with its coordinates translated, ctg_len and moved (Case.frame_of) the layout and the frames
        that go with them (tests/high_coords.py)"""
        self.L, self.ids = (L, constructed()[1]) if L is not None else constructed()
        self.ctg_len, self.moved = ctg_len, moved

    def __enter__(self):
        import torch
        self.hip = pagctl.hip_lib()
        g = self.L.g
        rng = np.random.default_rng(9)
        host = list(slice_arrays(g, rng))
        assert int((host[3] == 1).sum()) == len(self.L.count)
        host[3][host[3] == 1] = np.array(self.L.count, dtype=np.uint16)  # (the leaders, in vertex order)
        words = np.array([cases.K, 1, 2, 3], dtype=np.uint64)
        err = C.c_int()
        self.g = C.c_void_p(self.hip.pag_create(words.ctypes.data, len(words), cases.K, 0, C.byref(err)))
        assert self.g, self.hip.pag_last_error()
        self.dev = [torch.from_numpy(a.view(np.uint8).copy()).cuda() for a in host]  # (torch has no unsigned 32 / 64-bit tensors: the bytes go up)
        st = BuildStats()
        st.n_nodes, st.n_pos, st.n_uniq_edges = len(g["code"]), len(g["ctg"]), len(g["child_code"])
        sl = ShardSlice(len(host[0]), len(host[4]), *[t.data_ptr() for t in self.dev], st)
        rc = self.hip.pag_shard_import(self.g, C.byref(sl), 1, None)
        if rc != 0:
            self.hip.pag_destroy(self.g)
            raise AssertionError(self.hip.pag_last_error())
        self.vcode = g["code"][g["node_of_vertex"]]
        self.vpos = (g["ctg"].astype(np.uint64) << np.uint64(32)) | g["ref"].astype(np.uint64)
        return self

    def name_of(self, v):
        return (int(self.vcode[v]), int(self.vpos[v]))

    def calls(self, picked=CASES):
        return [(c.frame_of(self.ids, self.moved), self.ids[c.start], c.dist, c.has_size, c.limit) for c in picked]

    def walk(self, q, frames, excl):
        return ag.walk_straight_batch(self.hip, self.g, q, frames, excl, self.ctg_len, cases.DEVIATION, cases.ERROR_RATE)

    def __exit__(self, *exc):
        self.hip.pag_destroy(self.g)


@pytest.mark.gpu
def test_constructed_graph_every_line_of_the_rule():
    with Constructed() as c:
        calls = c.calls()
        want = by_the_rule(c.L, calls, c.name_of)
        got = answers(c.walk(*arrays_of(calls, c.name_of)))
        for case, g, w in zip(CASES, got, want):
            assert_answers(case.name, [g], [w])
            assert [x[:2] for x in g[0]] == [c.name_of(c.ids[v]) for v in case.path] and g[1] == case.status, case.name  # (the hand-written answer)
        # vertices the graph does not hold: a k-mer it lacks, a k-mer at a position it does not have — beside ones it holds
        q, frames, excl = arrays_of(calls[:3], c.name_of)
        q = np.concatenate((q[:1], q[:1], q[1:2], q[1:2], q[2:]))
        q["code"][1] = BUILDER.absent()
        q["pos"][3] += np.uint64(1 << 40)
        got = answers(c.walk(q, frames, excl))
        assert [g[1] for g in got] == [want[0][1], EINVAL, want[1][1], EINVAL, want[2][1]]
        assert got[1] == ([], EINVAL, []) and got[3] == ([], EINVAL, [])
        assert_answers("beside missing vertices", [got[0], got[2], got[4]], want[:3])


# ---- 4. shapes ------------------------------------------------------------------------------------------------------------------------
def raw_call(hip, g, q, frames, excl, node_cap, alt_cap, ctg_len=cases.CTG_LEN):
    """the C call itself with sentinel-filled buffers: (rc, node_off, nodes, alt_off, alts, status, n_nodes, n_alts, ms_kernels)"""
    lens = np.array(ctg_len, dtype=np.uint32)
    node_off, alt_off = np.full(len(q) + 1, 0xDEAD, dtype=np.uint64), np.full(len(q) + 1, 0xDEAD, dtype=np.uint64)
    nodes, alts = np.full(max(node_cap, 1) * NODE.itemsize, 0xA5, dtype=np.uint8), np.full(max(alt_cap, 1) * ALT.itemsize, 0xA5, dtype=np.uint8)
    status = np.full(len(q), 77, dtype=np.int32)
    n_nodes, n_alts, ms = C.c_uint64(12345), C.c_uint64(12345), C.c_double(-1.0)
    rc = hip.pag_walk_straight_batch(g, q.ctypes.data if len(q) else None, len(q), frames.ctypes.data if len(frames) else None, len(frames),
                                     excl.ctypes.data if len(excl) else None, len(excl), lens.ctypes.data, len(lens), cases.DEVIATION, cases.ERROR_RATE,
                                     node_off.ctypes.data, nodes.ctypes.data if node_cap else None, node_cap, alt_off.ctypes.data,
                                     alts.ctypes.data if alt_cap else None, alt_cap, status.ctypes.data, C.byref(n_nodes), C.byref(n_alts), C.byref(ms))
    return rc, node_off, nodes, alt_off, alts, status, n_nodes.value, n_alts.value, ms.value


@pytest.mark.gpu
def test_shapes_of_a_call():
    untouched = lambda a: bool((a == 0xA5).all())  # noqa: E731
    with Constructed() as c:
        calls = c.calls()
        want = by_the_rule(c.L, calls, c.name_of)
        q, frames, excl = arrays_of(calls, c.name_of)
        nn, na = sum(len(w[0]) for w in want), sum(len(w[2]) for w in want)
        want_node_off = np.concatenate(([0], np.cumsum([len(w[0]) for w in want])))
        want_alt_off = np.concatenate(([0], np.cumsum([len(w[2]) for w in want])))
        assert na >= 4
        # no query
        rc, node_off, _, alt_off, _, _, n_nodes, n_alts, ms = raw_call(c.hip, c.g, q[:0], frames, excl, 0, 0)
        assert rc == OK and (n_nodes, n_alts, node_off[0], alt_off[0]) == (0, 0, 0, 0)
        # the sizing call: PAG_ERANGE with the totals, both offset arrays and the statuses complete
        rc, node_off, nodes, alt_off, alts, status, n_nodes, n_alts, ms = raw_call(c.hip, c.g, q, frames, excl, 0, 0)
        assert rc == ERANGE and (n_nodes, n_alts) == (nn, na) and ms > 0.0 and b"room for" in c.hip.pag_last_error()
        assert np.array_equal(node_off, want_node_off) and np.array_equal(alt_off, want_alt_off) and status.tolist() == [w[1] for w in want]
        # either buffer one short: nothing is written
        for node_cap, alt_cap in ((nn - 1, na), (nn, na - 1)):
            rc, node_off, nodes, alt_off, alts, status, n_nodes, n_alts, ms = raw_call(c.hip, c.g, q, frames, excl, node_cap, alt_cap)
            assert rc == ERANGE and (n_nodes, n_alts) == (nn, na) and np.array_equal(node_off, want_node_off) and np.array_equal(alt_off, want_alt_off)
            assert untouched(nodes) and untouched(alts), "something was written although a buffer was too small"
        # both exact, with room behind: nothing is written beyond the totals
        rc, node_off, nodes, alt_off, alts, status, n_nodes, n_alts, ms = raw_call(c.hip, c.g, q, frames, excl, nn + 3, na + 3)
        assert rc == OK, c.hip.pag_last_error()
        assert untouched(nodes[nn * NODE.itemsize:]) and untouched(alts[na * ALT.itemsize:])
        assert_answers("exact buffers", answers((node_off, nodes.view(NODE)[:nn], alt_off, alts.view(ALT)[:na], status)), want)
        # a query named twice (and the order reversed); two frames sharing one excl slice
        twice = np.concatenate((q[::-1], q[:5], q[:5]))
        got = answers(c.walk(twice, frames, excl))
        assert_answers("named twice", got, want[::-1] + want[:5] + want[:5])
        with_excl = [i for i, case in enumerate(CASES) if "excl" in case.name and "first" in case.name or "last entry" in case.name]
        assert len(with_excl) == 2 and frames["excl_n"][q["frame"][with_excl[0]]] == frames["excl_n"][q["frame"][with_excl[1]]] > 2
        shared = frames.copy()
        shared["excl_off"][q["frame"][with_excl[1]]] = shared["excl_off"][q["frame"][with_excl[0]]]
        assert_answers("a shared excl slice", answers(c.walk(q, shared, excl)), want)
        # what the call's device memory is stated to be
        size = c.hip.pag_walk_straight_batch_bytes
        base = size(len(q), len(frames), len(excl), nn, na)
        assert base >= len(q) * (QUERY.itemsize + 28) + len(frames) * FRAME.itemsize + len(excl) * EXCL.itemsize + nn * NODE.itemsize + na * ALT.itemsize
        assert size(len(q), len(frames), len(excl), nn + 1, na) == base + NODE.itemsize and size(len(q), len(frames), len(excl), nn, na + 1) == base + ALT.itemsize
        assert size(len(q) + 1000, len(frames), len(excl), nn, na) > base and size(len(q), len(frames) + 100, len(excl), nn, na) > base
        assert size(len(q), len(frames), len(excl) + 1000, nn, na) > base and size(0, 5, 5, 0, 0) == 0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_a_device_is_touched():
    """(runs without a GPU: the arguments are checked before the handle is looked at, and no handle exists without a device)"""
    hip = pagctl.hip_lib()
    q = np.zeros(2, dtype=QUERY)
    q["limit"] = 2
    frames = np.zeros(1, dtype=FRAME)
    excl = np.zeros(3, dtype=EXCL)
    excl["code"] = [5, 5, 7]
    excl["pos"] = [1, 2, 0]
    frames["excl_n"] = 3

    def refused(word, q=q, frames=frames, excl=excl, null=None, **caps):
        lens = np.array([100], dtype=np.uint32)
        node_off, alt_off = np.zeros(len(q) + 1, dtype=np.uint64), np.zeros(len(q) + 1, dtype=np.uint64)
        n_nodes, n_alts = C.c_uint64(5), C.c_uint64(6)
        args = dict(q=q.ctypes.data, frames=frames.ctypes.data, excl=excl.ctypes.data, node_off=node_off.ctypes.data, alt_off=alt_off.ctypes.data,
                    n_nodes=C.byref(n_nodes), n_alts=C.byref(n_alts), nodes=None, alts=None, node_cap=0, alt_cap=0)
        args.update(caps)
        if null:
            args[null] = None
        rc = hip.pag_walk_straight_batch(None, args["q"], len(q), args["frames"], len(frames), args["excl"], len(excl), lens.ctypes.data, 1, 10, 0.15,
                                         args["node_off"], args["nodes"], args["node_cap"], args["alt_off"], args["alts"], args["alt_cap"], None,
                                         args["n_nodes"], args["n_alts"], None)
        msg = hip.pag_last_error()
        assert rc == EINVAL and word in msg and b"\n" not in msg, (rc, msg)
        if args["n_nodes"] is not None and args["n_alts"] is not None:
            assert (n_nodes.value, n_alts.value) == (0, 0)

    refused(b"null handle")  # (everything else in order)
    for name in ("q", "frames", "excl", "node_off", "alt_off", "n_nodes", "n_alts"):
        refused(b"null argument", null=name)
    refused(b"null argument", node_cap=4)
    refused(b"null argument", alt_cap=4)
    bad = q.copy()
    bad["frame"][1] = 1
    refused(b"query 1 names frame 1", q=bad)
    for limit in (0, 1, 65537):
        bad = q.copy()
        bad["limit"][1] = limit
        refused(b"query 1 has limit", q=bad)
    bad = q.copy()
    bad["limit"] = 65536
    refused(b"null handle", q=bad)
    for code, pos in (([5, 5, 7], [2, 1, 0]), ([5, 5, 7], [1, 1, 0]), ([5, 7, 5], [1, 0, 2])):
        unsorted = excl.copy()
        unsorted["code"], unsorted["pos"] = code, pos
        refused(b"not strictly ascending", excl=unsorted)
    for off, n in ((0, 4), (3, 1), (4, 0), (2 ** 63, 2 ** 63)):
        beyond = frames.copy()
        beyond["excl_off"], beyond["excl_n"] = off, n
        refused(b"frame 0: excl", frames=beyond)
    assert hip.pag_walk_straight_batch_bytes(0, 0, 0, 0, 0) == 0


@pytest.mark.gpu
def test_a_handle_without_a_graph_and_a_regional_handle_are_refused(workdir):
    ref = golden("extend_gap_t1")[0]
    q = np.zeros(1, dtype=QUERY)
    q["code"], q["pos"], q["dist"], q["limit"] = ref["vcode"][0], ref["vpos"][0], 9, 8
    frames = np.zeros(1, dtype=FRAME)
    frames["ctg_right"] = 0xFFFFFFFF
    none = np.zeros(0, dtype=EXCL)
    with Built("extend_gap_t1", 0, workdir) as b:
        fresh = C.c_void_p(pagctl.hip_create(b.inp))
        try:
            rc = raw_call(b.hip, fresh, q, frames, none, 8, 8)
            assert rc[0] == EINVAL and rc[6:8] == (0, 0) and b"no finished graph" in b.hip.pag_last_error()
        finally:
            b.hip.pag_destroy(fresh)
        assert raw_call(b.hip, b.g, q, frames, none, 8, 8)[0] == OK
        riv, ropen = np.array([1, 1000], dtype=np.uint32), np.array([0, 1], dtype=np.uint8)
        assert b.hip.pag_shard_set_region(b.g, C.byref(Region(0, None, 1, riv.ctypes.data, ropen.ctypes.data))) == 0
        rc = raw_call(b.hip, b.g, q, frames, none, 8, 8)
        assert rc[0] == ERANGE and rc[6:8] == (0, 0) and b"region" in b.hip.pag_last_error()
        with pytest.raises(RuntimeError):
            ag.walk_straight_batch(b.hip, b.g, q, frames, none, cases.CTG_LEN, 20, 0.15)


# ---- 6. the handle is left as found -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_call_leaves_the_handle_alone(workdir, monkeypatch):
    import seq_text
    from test_gpu_succ_golden import block_orient
    for s in ("PAG_SUCC_HEAVY", "PAG_TRAVEL_VIEW", "PAG_VIEW_HALO", "PAG_VIEW_MARGIN"):
        monkeypatch.delenv(s, raising=False)
    name, dump = "extend_gap_t1", "0_0_0"
    dumps, ctg_len = rule.dumps_of(name)
    _, contig, _, body, k = dumps[dump]
    ref = golden(name)[0]
    base = rule.first_round_frame(ctg_len, contig, rule.strand_of(ctg_len, contig, body))
    starts = [(base, (c, (a << 32) | r), k, 0, 64) for c, a, r, _, _ in body[::7]]
    q, frames, excl = arrays_of(starts, lambda v: v)
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
            walk = lambda: ag.walk_straight_batch(hip, g, q, frames, excl, ctg_len, 2 * b.spec["epsilon"], 0.15)  # noqa: E731
            lists = lambda: ag.successors_batch(hip, g, ref["vcode"][:2000], ref["vpos"][:2000], 2 * b.spec["epsilon"], 0.15)  # noqa: E731
            if with_call:
                before, lists_before = export(hip, g), lists()
                first = walk()
                assert len(first[1]) > 2 * len(q) and (first[4] >= 0).all()
                for a, c in zip(before, export(hip, g)):
                    assert np.array_equal(a, c), "pag_export_csr gives another graph after the call"
                for a, c in zip(lists_before, lists()):
                    assert np.array_equal(a, c), "pag_successors_batch answers differently after the call"
            assert hip.pag_travel_prepare(g, C.byref(pc.c), ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
            assert hip.pag_travel(g, C.byref(pc.c), orient.ctypes.data, ref_len.ctypes.data, len(ref_len), C.byref(prm), None) == 0, hip.pag_last_error()
            if with_call:
                for a, c in zip(first, walk()):  # (beside a prepared view, after walks that marked vertices used)
                    assert np.array_equal(a, c), "the call answers differently after pag_travel"
            paths.append(delivered_paths(hip, g, len(ctgs)))
    assert any(paths[0]) and paths[0] == paths[1], "pag_travel delivers other paths after the call"
