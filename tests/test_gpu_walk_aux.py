"""GPU: the kernels around the walker waves held to their rules, one by one, on constructed graphs.

k5_walk_aux.hip and k_ctg_nodes (k5_view.hip) feed and empty the walker; end to end they run only at the shapes the goldens
have.  Here each runs through its PRODUCTION launcher on host arrays (the hooks of include/pagraph_debug.h: pag_debug_trav_bounds,
pag_debug_ctg_nodes, pag_debug_trav_seeds, pag_debug_pack_paths, pag_debug_commit, pag_debug_clear_ranges, pag_debug_concat_parts,
pag_debug_gathers) against tests/walk_aux_rule.py.  Every comparison is exact, and a failure names the first difference.  Output
buffers go in filled with sentinels and come back whole, so what a kernel must NOT write is compared too.  The constructed cases
assert their own shapes in walk_aux_rule (tests/test_walk_aux_rule.py runs that without a device)."""
import ctypes as C

import numpy as np
import pytest

import pagctl
import walk_aux_rule as R
from aligngraph2_amd.capi import DTYPES, PAG_DEBUG_NULL, DebugTravGraph

pytestmark = pytest.mark.gpu
NODE = DTYPES["pag_path_node"]
SENT = 0xABCD1234  # what output buffers hold before a kernel runs


def _ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


def _first_diff(label, what, got, want, describe=None):
    """np.array_equal or an AssertionError that names the first difference"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    m = min(len(got), len(want))
    d = np.flatnonzero(got[:m] != want[:m])
    at = int(d[0]) if len(d) else m
    where = f" ({describe(at)})" if describe and at < len(want) else ""
    raise AssertionError(f"{label}: {what} differs ({len(got)} entries, the rule has {len(want)}); first at {at}{where}: device "
                         f"{got[at:at + 4].tolist()} rule {want[at:at + 4].tolist()}")


def _cgraph(G, bitmap=None, rank=None):
    """(pag_debug_trav_graph, the arrays it points into)"""
    keep = {n: np.ascontiguousarray(G[n], dtype=t) for n, t in (("ncode", np.uint32), ("npos_off", np.uint32), ("vpos", np.uint64), ("vcnt", np.uint16),
                                                               ("vnode", np.uint32), ("uold", np.uint32), ("newid", np.uint32), ("upos", np.uint64),
                                                               ("ucnt", np.uint32))}
    keep["bitmap"], keep["rank"] = bitmap, rank
    g = DebugTravGraph(n_nodes=G["n_nodes"], n_pos=G["n_pos"], k=G["k"], **{n: (a.ctypes.data if a is not None else None) for n, a in keep.items()})
    return g, keep


def _ok(hip, rc):
    assert rc == 0, hip.pag_last_error()


@pytest.fixture(scope="module")
def hip():
    return pagctl.hip_lib()


# =====================================================================================================================
# k_ranges, k_id_bounds
# =====================================================================================================================
def _bounds(hip, G, coords, ranges):
    g, keep = _cgraph(G)
    coords = np.asarray(coords, dtype=np.uint32)
    out = np.full(len(coords) + 2, SENT, dtype=np.uint32)
    ctgs = np.zeros(len(ranges), dtype=DTYPES["pag_debug_trav_contig"])
    for f in ("in_lo", "in_hi", "g_lo", "g_hi"):
        ctgs[f] = SENT
    ctgs["ctg_left"], ctgs["ctg_right"] = [r[0] for r in ranges], [r[1] for r in ranges]
    _ok(hip, hip.pag_debug_trav_bounds(C.byref(g), _ptr(coords), len(coords), out.ctypes.data, _ptr(ctgs), len(ctgs), 0))
    return out, ctgs


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_id_bounds_and_ranges_equal_the_rule(hip, n):
    rng = np.random.default_rng(n)
    values = [40, 41, 41, 41, 50, 50, 77, 90]
    G = R.random_graph(rng, 300, values, free=0.3)
    c = R.ctg_of(G["upos"])
    assert (c == 41).sum() > 3 and G["n_zero"] > 0
    # 0, 1, below the lowest coordinate, between two, on a coordinate several vertices share, one above the highest
    edges = [0, 1, 39, 45, 41, 50, 91, 90, 77, 0xFFFFFFFF]
    coords = np.array((edges * 7)[:n] if n > 1 else [41], dtype=np.uint32)
    want = R.id_bounds(G, coords)
    if n >= 63:
        assert want[4] == np.flatnonzero(c == 41)[0] and want[6] == G["n_pos"] and want[1] == G["n_zero"] == want[2] and want[0] == 0
    ranges = [(int(coords[i]), int(coords[(i + 3) % n])) for i in range(n)]
    out, ctgs = _bounds(hip, G, coords, ranges)
    label = f"{n} requests"
    _first_diff(label, "k_id_bounds (and the words behind its output)", out, np.concatenate([want, [SENT, SENT]]), lambda i: f"x = {coords[i]}")
    lo, hi = R.id_bounds(G, [r[0] for r in ranges]), R.id_bounds(G, [r[1] for r in ranges])
    for f, w in (("in_lo", lo), ("in_hi", hi), ("g_lo", lo), ("g_hi", hi)):
        _first_diff(label, f"k_ranges {f}", ctgs[f], w, lambda i: f"[{ranges[i][0]}, {ranges[i][1]})")


def test_id_bounds_on_graphs_without_contig_coordinates_and_without_vertices(hip):
    rng = np.random.default_rng(5)
    G = R.random_graph(rng, 100, [], free=1.0)
    assert G["n_zero"] == G["n_pos"] > 100
    coords = np.array([0, 1, 5, 0xFFFFFFFF], dtype=np.uint32)
    out, ctgs = _bounds(hip, G, coords, [(1, 9), (0, 1)])
    _first_diff("no vertex has a contig coordinate", "k_id_bounds", out[:4], [0, G["n_pos"], G["n_pos"], G["n_pos"]])
    _first_diff("no vertex has a contig coordinate", "k_ranges", np.stack([ctgs["in_lo"], ctgs["in_hi"]]).reshape(-1), [G["n_pos"], 0, G["n_pos"], G["n_pos"]])
    E = {"k": 8, "n_nodes": 0, "n_pos": 0, "n_zero": 0, "npos_off": np.zeros(1, np.uint32), **{n: np.zeros(0, np.uint64) for n in ("ncode", "vpos", "vcnt", "vnode", "uold", "newid", "upos", "ucnt")}}
    out, ctgs = _bounds(hip, E, coords, [(1, 9)])
    _first_diff("n_pos = 0", "k_id_bounds", out[:4], [0, 0, 0, 0])
    assert (ctgs["in_lo"][0], ctgs["in_hi"][0], ctgs["g_lo"][0], ctgs["g_hi"][0]) == (0, 0, 0, 0)


# =====================================================================================================================
# k_ctg_nodes
# =====================================================================================================================
@pytest.mark.parametrize("k", [8, 13, 14, 15, 16])
def test_ctg_nodes_equal_the_rule(hip, k):
    rng = np.random.default_rng(k)
    # strand lengths: k - 1 (nothing written), k, k + 1, the last k-mer's first base at positions 15, 16, 17 of a 16-base word, and
    # one of more than a block of k-mers (the grid is sized by the longest); the first and the last code of the 4^k in a strand
    lens = [k - 1, k, k + 1, k + 15, k + 16, k + 17, 300 + k]
    seqs = ["".join(rng.choice(list(R.BASES), size=n)) for n in lens]
    seqs[1], seqs[2] = "A" * k, "T" * k + "G"
    seqs[6] = seqs[6][:100] + "T" * k + seqs[6][100 + k:-k] + "A" * k
    jobs = [(s, fwd) for s in seqs for fwd in (1, 0)]
    codes = sorted({R.kmer_code(s[i:i + k]) for s in seqs + [R.revcomp(s) for s in seqs] for i in range(len(s) - k + 1)} | {0, (1 << (2 * k)) - 1})
    ncode = np.array(codes[::2] + ([codes[-1]] if len(codes) % 2 == 0 else []), dtype=np.uint32)  # (every other k-mer owns no node)
    assert ncode[0] == 0 and ncode[-1] == (1 << (2 * k)) - 1 and len(ncode) < len(codes)
    bitmap, rank = R.code_bitmap(ncode, k)
    g = DebugTravGraph(n_nodes=len(ncode), n_pos=0, k=k, bitmap=bitmap.ctypes.data, rank=rank.ctypes.data)
    chunks, byte_off, rows, want, at = [], 0, [], [np.array([SENT], dtype=np.uint32)], 1
    for s, fwd in jobs:
        p = R.pack_bases(s)
        w = R.ctg_nodes(s, fwd, k, ncode)
        rows.append((byte_off, at, len(s), fwd))
        chunks.append(p)
        byte_off += len(p)
        want += [w, np.array([SENT], dtype=np.uint32)]  # (a word between two jobs that nobody may write)
        at += len(w) + 1
    want = np.concatenate(want)
    assert (want == R.PAG_NONE).any() and (want == 0).any() and (want == len(ncode) - 1).any(), "k-mers without a node, the first and the last code"
    packed = np.concatenate(chunks + [np.zeros(16, dtype=np.uint8)])  # (pag_seqs: 16 readable bytes behind the last strand)
    jobs_a = np.array(rows, dtype=np.uint64).reshape(-1)
    out = np.full(len(want), SENT, dtype=np.uint32)
    _ok(hip, hip.pag_debug_ctg_nodes(C.byref(g), packed.ctypes.data, len(packed), jobs_a.ctypes.data, len(rows), max(lens), out.ctypes.data, len(out), 0))
    owner = np.repeat(np.arange(len(rows)), [max(r[2] - k + 1, 0) + 1 for r in rows])
    _first_diff(f"k = {k}", "node ids of the strands' k-mers", out[1:], want[1:],
                lambda i: f"job {owner[i]}: {len(jobs[owner[i]][0])} bases, {'forward' if jobs[owner[i]][1] else 'reverse'}")
    assert out[0] == SENT


# =====================================================================================================================
# the seed family, with visited states made by k_commit
# =====================================================================================================================
def _pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def _commit(hip, seq_u, in_lo, in_hi, front=0, label="commit"):
    """k_commit through its hook on an empty state -> (bitmap words with `front` zero words before and one behind, the hash
    table), after both were held to the rule"""
    seq_u = np.ascontiguousarray(seq_u, dtype=np.uint32)
    want_bits, want_set = R.commit(seq_u, in_lo, in_hi)
    ncap = _pow2(max(4 * len(want_set), 8))  # (the host: at least four slots per entry)
    bits = np.zeros(front + len(want_bits) + 1, dtype=np.uint32)
    bits[-1] = SENT
    table = np.full(ncap, 0xFFFFFFFF, dtype=np.uint32)
    _ok(hip, hip.pag_debug_commit(_ptr(seq_u), len(seq_u), in_lo, in_hi, bits.ctypes.data, len(bits), front, table.ctypes.data, ncap, 0))
    _first_diff(label, "visited bitmap (then the word behind it)", bits[front:], np.concatenate([want_bits, [SENT]]), lambda w: f"ids {in_lo + 32 * w}..")
    assert (bits[:front] == 0).all(), f"{label}: a word before the bitmap was written"
    _first_diff(label, "hash set, sorted", np.sort(table[table != 0xFFFFFFFF]), want_set)
    return bits, table


def _seeds(hip, G, which, contigs, reqs, dev, stride, out):
    """contigs: rule dicts (walk_aux_rule), their device state under "dev_bits" = (words, word offset) / "dev_set" -> out, filled"""
    g, keep = _cgraph(G)
    rec = np.zeros(len(contigs), dtype=DTYPES["pag_debug_trav_contig"])
    nodes, bits, sets = [], [np.zeros(1, np.uint32)], [np.zeros(1, np.uint32)]
    n_at, b_at, s_at = 0, 1, 1
    for i, D in enumerate(contigs):
        rec[i]["nodes_off"], rec[i]["n_kmers"] = n_at, len(D["nodes"])
        nodes.append(np.asarray(D["nodes"], dtype=np.uint32))
        n_at += len(D["nodes"])
        for f in ("ctg_left", "ctg_right", "g_lo", "g_hi"):
            rec[i][f] = D[f]
        rec[i]["in_lo"], rec[i]["in_hi"] = D.get("in_lo", D["g_lo"]), D["g_hi"]  # (in_lo: what the commit wrote its bits relative to)
        rec[i]["gbits_off"] = rec[i]["gset_off"] = PAG_DEBUG_NULL
        if D.get("gbits") is not None:
            words, off = D["dev_bits"]
            rec[i]["gbits_off"] = b_at + off
            bits.append(words)
            b_at += len(words)
            rec[i]["gset_off"], rec[i]["gmask"] = s_at, len(D["dev_set"]) - 1
            sets.append(D["dev_set"])
            s_at += len(D["dev_set"])
    nodes, bits, sets = (np.ascontiguousarray(np.concatenate(x), dtype=np.uint32) for x in (nodes, bits, sets))
    rq = np.array([(c, l, r, p) for c, l, r, p in reqs], dtype=np.uint64).reshape(-1)
    _ok(hip, hip.pag_debug_trav_seeds(C.byref(g), which, rec.ctypes.data, len(rec), _ptr(nodes), len(nodes), bits.ctypes.data, len(bits), sets.ctypes.data, len(sets),
                                      _ptr(rq), len(reqs), dev, out.ctypes.data, len(out), stride, 0))
    return out


def test_seed_first_equals_the_rule(hip):
    for name, G, Cc, dev, stride in R.seed_first_cases():
        half = dict(Cc, nodes=Cc["nodes"][:len(Cc["nodes"]) // 2])  # (a second contig in the launch: the same strand, its first half of k-mers)
        want = np.full(2 * stride + 3, SENT, dtype=np.uint32)
        for c, D in enumerate((Cc, half)):
            want[c * stride:(c + 1) * stride] = R.seed_first_words(R.seed_first(G, D, dev), stride, want[c * stride:(c + 1) * stride])
        out = _seeds(hip, G, 0, [Cc, half], [], dev, stride, np.full(2 * stride + 3, SENT, dtype=np.uint32))
        _first_diff(name, f"the words of two contigs (stride {stride}: count, (vertex, offset) pairs, then the caller's sentinels)", out, want,
                    lambda i: f"contig {i // stride}, word {i % stride}")


def _with_device_state(hip, G, D, below=0):
    """the rule's contig state D committed on the device; below = 32 / 64: the readers' g_lo that far under the commit's in_lo, the
    bitmap pointer moved with it (those ids read as not visited: zero words)"""
    if D.get("gbits") is None:
        return D
    front = below // 32
    bits, table = _commit(hip, D["committed"], D["g_lo"], D["g_hi"], front=front, label=f"commit into [{D['g_lo']}, {D['g_hi']})")
    E = dict(D, dev_bits=(bits, 0), dev_set=table, in_lo=D["g_lo"])
    if below:
        E["g_lo"] = D["g_lo"] - below
        E["gbits"] = np.concatenate([np.zeros(below, dtype=bool), D["gbits"]])
    return E


@pytest.mark.parametrize("state", [0, 1, 2])
def test_seed_window_equals_the_rule(hip, state):
    G, C0, dev, pos, _ = R.seed_window_case()
    label, D = R.window_states(G, C0, dev, pos)[state]
    D = _with_device_state(hip, G, D)
    reqs = [(0, left, right, pos) for (left, right), _ in R.WINDOW_REQUESTS]
    for stride in (64, 8):
        per = R.SEED_PARTS * stride
        want = np.full(len(reqs) * per + 5, SENT, dtype=np.uint32)
        lists = []
        for r, (_, left, right, _) in enumerate(reqs):
            lo, hi = R.window_bounds(D, left, right)
            parts = [R.seed_window_range(G, D, a, b, pos, dev) for a, b in R.window_split(lo, hi)]
            lists.append(R.seed_window_range(G, D, lo, hi, pos, dev))
            want[r * per:(r + 1) * per] = R.seed_window_words(parts, stride, want[r * per:(r + 1) * per])
        out = _seeds(hip, G, 1, [D], reqs, dev, stride, np.full(len(want), SENT, dtype=np.uint32))
        _first_diff(f"{label}, stride {stride}", "the words of the requests' parts (count, ids that fit, then the caller's sentinels)", out, want,
                    lambda i: f"request {R.WINDOW_REQUESTS[min(i // per, len(reqs) - 1)]}, part {i % per // stride}, word {i % stride}")
        if stride == 64:  # (nothing was clipped) the host's list of candidates is the rule's
            assert max(len(x) for x in lists) < stride
            for r in range(len(reqs)):
                assert R.window_candidates(out[r * per:(r + 1) * per], stride) == list(dict.fromkeys(lists[r])), R.WINDOW_REQUESTS[r]
        elif state == 0:  # (what the clipped run is there for: a count of 20, seven ids, the next part's words behind them)
            r = len(reqs) - 1
            assert want[r * per] == 20 and (want[r * per + 1:r * per + 8] != SENT).all() and want[r * per + 8] == 0


@pytest.mark.parametrize("below", [0, 32, 64])
def test_checkpoints_equal_the_rule(hip, below):
    G, D, dev, reqs = R.checkpoint_case()
    E = _with_device_state(hip, G, D, below)
    want = np.array([R.checkpoint(G, E, l, r, dev) for l, r, _, _ in reqs], dtype=np.uint32).reshape(-1)
    assert np.array_equal(want, np.array([R.checkpoint(G, D, l, r, dev) for l, r, _, _ in reqs], dtype=np.uint32).reshape(-1)), "the same state, read from a lower g_lo"
    out = _seeds(hip, G, 2, [E], [(0, l, r, 0) for l, r, _, _ in reqs], dev, 0, np.full(len(want) + 3, SENT, dtype=np.uint32))
    _first_diff(f"g_lo {below} below in_lo", "checkpoints (vertex, contig coordinate, abundance)", out, np.concatenate([want, [SENT] * 3]),
                lambda i: f"request {reqs[min(i // 3, len(reqs) - 1)][:3]}")


@pytest.mark.parametrize("below", [32, 64])
def test_seed_window_reads_a_commit_from_a_lower_g_lo(hip, below):
    G, D, dev, reqs = R.checkpoint_case()
    E = _with_device_state(hip, G, D, below)
    pos = 81
    rq = [(0, 0, 199, pos), (0, 60, 62, 61)]
    lists = [R.seed_window_range(G, E, *R.window_bounds(E, l, r), p, dev) for _, l, r, p in rq]
    assert lists == [R.seed_window_range(G, D, *R.window_bounds(D, l, r), p, dev) for _, l, r, p in rq]
    assert len(lists[0]) < len(R.seed_window_range(G, dict(D, gbits=None), 0, 200, pos, dev)), "the commit hides no candidate of the window"
    stride = 64
    out = _seeds(hip, G, 1, [E], rq, dev, stride, np.full(2 * R.SEED_PARTS * stride, SENT, dtype=np.uint32))
    for r in range(2):
        got = R.window_candidates(out[r * R.SEED_PARTS * stride:(r + 1) * R.SEED_PARTS * stride], stride)
        _first_diff(f"g_lo {below} below in_lo, request {rq[r]}", "the window's candidates", got, lists[r])


# =====================================================================================================================
# k_commit
# =====================================================================================================================
@pytest.mark.parametrize("in_lo,n_in", [(0, 45), (32, 1000), (37, 1001)])
def test_commit_equals_the_rule(hip, in_lo, n_in):
    rng = np.random.default_rng(in_lo)
    for length in (1, 255, 257, 70000):
        top = in_lo + n_in + 3000  # ids below (where in_lo > 0), inside and above the range, repeated
        seq = rng.integers(0, top, size=length).astype(np.uint32)
        if length > 1:
            seq[:6] = [in_lo, in_lo + n_in - 1, in_lo + n_in, max(in_lo, 1) - 1, top - 1, in_lo]
            assert len(np.unique(seq)) < length or length < 300
        _commit(hip, seq, in_lo, in_lo + n_in, label=f"{length} ids into [{in_lo}, {in_lo + n_in})")


# =====================================================================================================================
# k_pack_paths
# =====================================================================================================================
@pytest.mark.parametrize("which", [0, 1])
def test_pack_paths_equal_the_rule(hip, which):
    rng = np.random.default_rng(11)
    G = R.random_graph(rng, 900, [0] + list(range(1000, 1040)))
    _pack_and_compare(hip, G, R.pack_batches(rng, G)[which], f"batch {which}")


def test_pack_paths_across_2_31_and_a_log_at_its_clamp(hip):
    """Path coordinates on both sides of 2^31 in one block, blocks all below and all above it: the block tables' highest / lowest /
    lowest non-zero coordinate are unsigned maxima and minima.  And a leap job's log as walk_job writes it for such a path — the
    lowest contig-following coordinate clamped to 2^31 - 1, "none" recorded as the same value: blocks whose boundaries are all at
    the clamp, and blocks with one entry a little below it."""
    rng = np.random.default_rng(12)
    top = 1 << 31
    G = R.random_graph(rng, 900, [0] + list(range(top - 20, top + 20)))
    c_of = R.ctg_of(G["upos"])
    below, above, free = np.flatnonzero((c_of != 0) & (c_of < top)), np.flatnonzero(c_of >= top), np.flatnonzero(c_of == 0)
    assert min(len(below), len(above), len(free)) >= 64

    def job(length, leap):
        v = rng.integers(0, G["n_pos"], size=length).astype(np.uint32)
        if length >= 256:
            v[64:128], v[128:192] = rng.choice(below, size=64), rng.choice(above, size=64)
            v[192:256] = rng.choice(np.concatenate([above, free]), size=64)
        s = rng.integers(0, 1 << 24, size=length).astype(np.uint32)
        if not leap:
            return v, s, None
        c = c_of[v]
        # (the true value: none beside a coordinate-free vertex, a coordinate a little below the vertex's below 2^31, the vertex's own above)
        elow = np.where(c == 0, 0xFFFFFFFF, np.where(c < top, np.maximum(c, 8) - rng.integers(0, 8, size=length), c))
        x = (np.uint64(1) << np.uint64(63)) | (np.minimum(elow, 0x7FFFFFFF).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, size=length, dtype=np.uint64)
        x[rng.random(length) < 0.4] = 0  # (no boundary)
        return v, s, x

    batch = [job(63, True), job(300, False), job(300, True), job(65, True), job(1, True)]
    w = R.pack_job(G, *batch[2])
    agg, xagg = w[5 * 300:5 * 300 + 5 * 5].reshape(-1, 5).astype(np.int64), w[5 * 300 + 5 * 5:].reshape(-1, 2).astype(np.int64)
    assert agg[1, 0] < top <= agg[2, 3] and agg[3, 2] == 0 and agg[3, 3] >= top, "no block all below / all above 2^31 / above with coordinate-free vertices"
    assert ((agg[:, 0] >= top) & (agg[:, 3] < top)).any(), "no block whose coordinates lie on both sides of 2^31"
    assert xagg[2, 0] == xagg[3, 0] == 0x7FFFFFFF and 0x7FFFFF00 < xagg[1, 0] < 0x7FFFFFFF, f"no block with every boundary at the clamp / one below it: {xagg[:, 0]}"
    _pack_and_compare(hip, G, batch, "coordinates across 2^31")


def _pack_and_compare(hip, G, batch, label):
    offs, total = R.pack_layout(batch)
    want = np.full(total, SENT, dtype=np.uint32)
    seq_v, seq_s, seq_x, rows, at = [], [], [], [], 0
    for (v, s, x), off in zip(batch, offs):
        w = R.pack_job(G, v, s, x)
        want[off:off + len(w)] = w
        rows.append((at, len(v), off, int(x is not None)))
        seq_v.append(v)
        seq_s.append(s)
        seq_x.append(x if x is not None else np.zeros(len(v), dtype=np.uint64))
        at += len(v)
    seq_v, seq_s, seq_x = np.concatenate(seq_v), np.concatenate(seq_s), np.concatenate(seq_x)
    descs = np.array(rows, dtype=np.uint64).reshape(-1)
    g, keep = _cgraph(G)
    out = np.full(total, SENT, dtype=np.uint32)
    _ok(hip, hip.pag_debug_pack_paths(C.byref(g), seq_v.ctypes.data, seq_s.ctypes.data, seq_x.ctypes.data, len(seq_v), descs.ctypes.data, len(rows),
                                      max(r[1] for r in rows), out.ctypes.data, total, 0))

    def where(i):
        j = int(np.searchsorted(offs, i, side="right")) - 1
        n, leap = rows[j][1], rows[j][3]
        rel, arrays = i - offs[j], (5 if leap else 3)
        if rel < arrays * n:
            return f"job {j} ({n} entries{', leap' if leap else ''}): array {rel // n}, entry {rel % n}"
        rel -= arrays * n
        nb = -(-n // 64)
        if rel < 5 * nb:
            return f"job {j} ({n} entries{', leap' if leap else ''}): block table row {rel // 5}, word {rel % 5}"
        rel -= 5 * nb
        return f"job {j} ({n} entries): leap table row {rel // 2}, word {rel % 2}" if rel < 2 * nb and leap else f"the untouched word behind job {j}"

    _first_diff(label, "the packed words (arrays, block tables, and the untouched words between the jobs)", out, want, where)


# =====================================================================================================================
# k_clear_ranges
# =====================================================================================================================
def test_clear_ranges_equal_the_rule(hip):
    slot = 4352  # one range per slot of 17 lines of 256 bytes, sentinels on both sides
    ranges = [(16 + o, n, w) for n in (0, 1, 15, 16, 17, 4101) for o in range(16) for w in (0, 0xFFFFFFFF, 0x04030201)]
    ranges = [(i * slot + off, n, w) for i, (off, n, w) in enumerate(ranges)]
    assert all(off + n <= (i + 1) * slot - 16 for i, (off, n, _) in enumerate(ranges)) and {r[0] % 16 for r in ranges} == set(range(16))
    calls = [ranges[:1], ranges[1:4]] + [ranges[a:a + 40] for a in range(4, len(ranges), 40)]
    assert {len(c) for c in calls} >= {1, 3, 40}
    for call in calls:
        lo, hi = call[0][0] // slot * slot, (call[-1][0] // slot + 1) * slot
        rel = [(off - lo, n, w) for off, n, w in call]
        buf = np.full(hi - lo, 0xA5, dtype=np.uint8)
        want = R.clear_ranges(buf, rel)
        rows = np.array(rel, dtype=np.uint64).reshape(-1)
        _ok(hip, hip.pag_debug_clear_ranges(buf.ctypes.data, len(buf), rows.ctypes.data, len(rel), 0))
        _first_diff(f"{len(call)} ranges", "the cleared buffer", buf, want,
                    lambda i: "the slot of the range (start % 16, bytes, word) = " + str([(o % 16, n, hex(w)) for o, n, w in rel if o // slot == i // slot][0]) + f", byte {i % slot} of the slot")


# =====================================================================================================================
# k_concat_parts
# =====================================================================================================================
@pytest.mark.parametrize("sizes,first_at", [([9000], 0), ([0, 4097, 1], 0), ([1, 4096, 4095], 5),
                                            ([0, 1, 4095, 4096, 4097, 9000] * 16 + [3, 0, 70, 4096], 0)])
def test_concat_parts_equal_the_rule(hip, sizes, first_at):
    rng = np.random.default_rng(len(sizes))
    n_src = sum(sizes) + 100
    src_v, src_s = rng.integers(0, 1 << 32, size=n_src, dtype=np.uint64).astype(np.uint32), rng.integers(1, 1 << 24, size=n_src).astype(np.uint32)
    order = rng.permutation(len(sizes))  # (the parts lie in the jobs' buffers in another order than in the walk)
    frm = np.zeros(len(sizes), dtype=np.int64)
    at = 50
    for i in order:
        frm[i] = at
        at += sizes[i]
    starts = first_at + np.concatenate([[0], np.cumsum(sizes)[:-1]])
    parts = [(int(frm[i]), int(starts[i]), int(sizes[i])) for i in range(len(sizes))]
    n_out = first_at + sum(sizes) + 7
    out_v, out_s = np.full(n_out, SENT, dtype=np.uint32), np.full(n_out, SENT, dtype=np.uint32)
    want_v, want_s = R.concat_parts(src_v, src_s, parts, out_v, out_s, 0xF0005EED)
    assert (want_s == 0xF0005EED).sum() == (1 if first_at == 0 else 0) and (want_v[-7:] == SENT).all()
    rows = np.array(parts, dtype=np.uint64).reshape(-1)
    _ok(hip, hip.pag_debug_concat_parts(src_v.ctypes.data, src_s.ctypes.data, n_src, rows.ctypes.data, len(parts), out_v.ctypes.data, out_s.ctypes.data, n_out, 0xF0005EED, 0))
    label = f"{len(sizes)} parts, the first at {first_at}"
    part_of = lambda i: f"part {int(np.searchsorted(starts, i, side='right')) - 1}"
    _first_diff(label, "vertices", out_v, want_v, part_of)
    _first_diff(label, "steps (first_step at output index 0 only)", out_s, want_s, part_of)


# =====================================================================================================================
# the gathers
# =====================================================================================================================
@pytest.fixture(scope="module")
def gather_graph():
    return R.random_graph(np.random.default_rng(21), 1200, [0] + list(range(500, 530)))


@pytest.mark.parametrize("length", [1, 6143, 6145, 50000])
def test_gather_pc_and_path_equal_the_rule(hip, gather_graph, length):
    G = gather_graph
    rng = np.random.default_rng(length)
    g, keep = _cgraph(G)
    seq_v = rng.integers(0, G["n_pos"], size=length).astype(np.uint32)
    seq_s = rng.integers(0, 1 << 24, size=length).astype(np.uint32)
    seq_s[0] = 0
    out = np.full(length, SENT, dtype=np.uint32)
    _ok(hip, hip.pag_debug_gathers(C.byref(g), 0, seq_v.ctypes.data, None, length, 0, out.ctypes.data, 0))
    _first_diff(f"{length} entries", "k_gather_pc", out, R.ctg_of(G["upos"][seq_v]).astype(np.uint32), lambda i: f"new id {seq_v[i]}")
    want = R.gather_records(G, G["uold"][seq_v], seq_s, NODE)
    for max_blocks in (0, 24):  # (24 blocks: 6 144 entries a turn — 6 145 and 50 000 take the stride loop)
        rec = np.zeros(length, dtype=NODE)
        rec["reserved"] = 0x7777
        _ok(hip, hip.pag_debug_gathers(C.byref(g), 1, seq_v.ctypes.data, seq_s.ctypes.data, length, max_blocks, rec.ctypes.data, 0))
        for f in NODE.names:
            _first_diff(f"{length} entries, max_blocks {max_blocks}", f"k_gather_path .{f}", rec[f], want[f], lambda i: f"new id {seq_v[i]}")


@pytest.mark.parametrize("n", [1, 255, 257])
def test_gather_vertices_equal_the_rule(hip, gather_graph, n):
    G = gather_graph
    g, keep = _cgraph(G)
    vids = np.random.default_rng(n).integers(0, G["n_pos"], size=n).astype(np.uint32)
    rec = np.zeros(n, dtype=NODE)
    rec["reserved"], rec["step"] = 0x7777, 99
    _ok(hip, hip.pag_debug_gathers(C.byref(g), 2, vids.ctypes.data, None, n, 0, rec.ctypes.data, 0))
    want = R.gather_records(G, vids, np.zeros(n), NODE)
    for f in NODE.names:
        _first_diff(f"{n} vertices", f"k_gather_vertices .{f} (reserved and step are 0)", rec[f], want[f], lambda i: f"vertex {vids[i]}")
