"""The kernels around the walker waves, stated once more and independently of the device code (numpy only, no device).

k5_walk_aux.hip (and k_ctg_nodes of k5_view.hip) feed and empty the walker: strand k-mers to node ids, id ranges and bounds, the
first seeds (the reference's searchPANode with onlyFirst), the re-seed windows (searchPANode2 + filterPANodes), checkpoints, the
pack kernel with its block tables, the commit of a walk into the global visited structures, the batch clear, the concatenation
on the device, the gathers.  This module is their rules in plain words: written from the kernels' comments, DESIGN.md 3 and, for
the two seed searches, from what the reference does.  tests/test_gpu_walk_aux.py holds the kernels to them exactly;
tests/test_walk_aux_rule.py holds the vectorised rules to plain loops and the constructed cases to the shapes they are named for.

A graph is a dict of the arrays of a traversal graph (pag_travel.hpp TravGraph): ncode, npos_off, vpos, vcnt, vnode k-mer-major,
uold / newid / upos / ucnt in the coordinate order (view_rule.order).  A contig strand is a dict: nodes[n_kmers], ctg_left,
ctg_right, g_lo, g_hi, gbits (None or a bool array over [g_lo, g_hi)), gset (None or a Python set of new ids)."""
import numpy as np

import view_rule

PAG_NONE = 0xFFFFFFFF
SEED_PARTS = 16   # waves per re-seed window request (TRAV_SEED_PARTS)
BLOCK = 64        # entries per row of a block table
PACK_TURN = 64 * 256  # entries the pack kernel's grid takes per turn when it is at its largest (64 blocks of 256)
U32 = 0xFFFFFFFF


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def graph_from_lists(poslists, k=8, codes=None):
    """poslists[node] = [(ctg, ref, cnt), ...] (at least one each) -> the graph; inside a node ascending (ctg, ref)"""
    n_nodes = len(poslists)
    assert all(len(pl) for pl in poslists), "a node has at least one vertex"
    rows = [(n,) + tuple(t) for n, pl in enumerate(poslists) for t in sorted(pl)]
    a = np.array(rows, dtype=np.int64).reshape(-1, 4)
    vpos = (a[:, 1].astype(np.uint64) << np.uint64(32)) | a[:, 2].astype(np.uint64)
    npos_off = np.concatenate([[0], np.cumsum([len(pl) for pl in poslists])]).astype(np.uint32)
    uold, n_zero = view_rule.order(vpos)
    newid = np.empty(len(vpos), dtype=np.uint32)
    newid[uold] = np.arange(len(vpos), dtype=np.uint32)
    vcnt = a[:, 3].astype(np.uint16)
    G = {"k": k, "n_nodes": n_nodes, "n_pos": len(vpos), "n_zero": n_zero,
         "ncode": np.arange(n_nodes, dtype=np.uint32) if codes is None else np.asarray(codes, dtype=np.uint32), "npos_off": npos_off, "vpos": vpos,
         "vcnt": vcnt, "vnode": a[:, 0].astype(np.uint32), "uold": uold.astype(np.uint32), "newid": newid, "upos": vpos[uold],
         "ucnt": vcnt[uold].astype(np.uint32)}
    assert len(G["ncode"]) == n_nodes and (np.diff(G["ncode"].astype(np.int64)) > 0).all()
    return G


def random_graph(rng, n_nodes, coords, free=0.3, max_per_node=4):
    """a graph whose contig coordinates come from `coords` (few values: runs of vertices share one), a share `free` without one"""
    pl = []
    for _ in range(n_nodes):
        m = int(rng.integers(1, max_per_node + 1))
        pl.append([(0 if rng.random() < free or not len(coords) else int(rng.choice(coords)), int(rng.integers(1, 1 << 20)), int(rng.integers(0, 300)))
                   for _ in range(m)])
    return graph_from_lists(pl)


def ctg_of(pos):
    return (np.asarray(pos, dtype=np.uint64) >> np.uint64(32)).astype(np.int64)


# ---- k_id_bounds / k_ranges -------------------------------------------------------------------------------------------------
def id_bounds(G, coords):
    """first new id whose contig coordinate is >= x: the vertices without a coordinate stand first, the others ascending"""
    return np.searchsorted(ctg_of(G["upos"]), np.asarray(coords, dtype=np.int64), side="left").astype(np.uint32)


def id_bounds_loop(G, coords):
    c = ctg_of(G["upos"])
    return np.array([sum(1 for y in c if y < x) for x in coords], dtype=np.uint32)


# ---- k_ctg_nodes --------------------------------------------------------------------------------------------------------------
BASES = "ACGT"


def pack_bases(seq):
    """CompressedSeq: base i at bits 2 (i & 3) of byte i >> 2; padded to a 4-byte boundary"""
    out = np.zeros((len(seq) + 15) // 16 * 4, dtype=np.uint8)
    for i, ch in enumerate(seq):
        out[i >> 2] |= BASES.index(ch) << (2 * (i & 3))
    return out


def kmer_code(kmer):
    """the first base is the most significant pair of bits"""
    c = 0
    for ch in kmer:
        c = c * 4 + BASES.index(ch)
    return c


def revcomp(seq):
    return "".join(BASES[3 - BASES.index(ch)] for ch in reversed(seq))


def ctg_nodes(seq, forward, k, ncode):
    """node id (index into the ascending codes) of every k-mer of the strand: the contig as given, or its reverse complement"""
    s = seq if forward else revcomp(seq)
    index = {int(c): n for n, c in enumerate(ncode)}
    return np.array([index.get(kmer_code(s[i:i + k]), PAG_NONE) for i in range(max(len(s) - k + 1, 0))], dtype=np.uint32)


def code_bitmap(ncode, k):
    """bit per code that owns a node, and per 64-bit word the nodes before it"""
    n_words = ((1 << (2 * k)) + 63) // 64
    ncode = np.asarray(ncode, dtype=np.uint64)
    bitmap = np.zeros(n_words, dtype=np.uint64)
    np.bitwise_or.at(bitmap, (ncode >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ncode & np.uint64(63)))
    per = np.zeros(n_words + 1, dtype=np.uint32)
    np.add.at(per, (ncode >> np.uint64(6)).astype(np.int64) + 1, 1)
    return bitmap, np.cumsum(per[:-1], dtype=np.uint32)


# ---- visited ------------------------------------------------------------------------------------------------------------------
def visited(G, C, p):
    """filterPANodes on the device: vertex p is in the contig's global visited structures — its bit where its new id lies in
    [g_lo, g_hi), the hash set elsewhere; nothing is visited before the first commit (gbits None)"""
    if C.get("gbits") is None:
        return False
    u = int(G["newid"][p])
    if C["g_lo"] <= u < C["g_hi"]:
        return bool(C["gbits"][u - C["g_lo"]])
    return C.get("gset") is not None and u in C["gset"]


def on_strand_offset(G, C, p):
    """offset of vertex p on the strand, None when its contig coordinate is not in [ctg_left, ctg_right)"""
    pc = int(G["vpos"][p]) >> 32
    return pc - C["ctg_left"] if C["ctg_left"] <= pc < C["ctg_right"] else None


def positions(G, node):
    return range(int(G["npos_off"][node]), int(G["npos_off"][node + 1])) if node != PAG_NONE else range(0)


# ---- k_seed_first ---------------------------------------------------------------------------------------------------------------
def seed_first(G, C, dev):
    """searchPANode with onlyFirst: the k-mers of the strand in order; the first one that has a position on the strand within
    `dev` of the k-mer's own offset gives ALL its such positions, as (vertex, offset) pairs; later k-mers give nothing"""
    for i, node in enumerate(C["nodes"]):
        pairs = []
        for p in positions(G, int(node)):
            off = on_strand_offset(G, C, p)
            if off is not None and abs(off - i) <= dev:
                pairs.append((p, i))
        if pairs:
            return pairs
    return []


def seed_first_words(pairs, stride, before):
    """what the kernel leaves in the contig's `stride` words: the pairs that fit behind the count, the count of THOSE"""
    out = np.array(before, dtype=np.uint32)
    fit = pairs[:max((stride - 1) // 2, 0)]
    out[0] = len(fit)
    for n, (p, i) in enumerate(fit):
        out[1 + 2 * n], out[2 + 2 * n] = p, i
    return out


# ---- k_seed_window --------------------------------------------------------------------------------------------------------------
def window_bounds(C, left, right):
    """the offsets a request covers: [left, min(right, n_kmers - 1)], as a half-open pair (empty: left at or behind its end)"""
    end = min(right + 1, len(C["nodes"]))
    return left, max(end, left)


def seed_window_range(G, C, lo, hi, pos, dev):
    """searchPANode2 + filterPANodes over the offsets [lo, hi): every position on the strand within `dev` of `pos` (the ANCHOR,
    not the k-mer's own offset) that is not visited, by offset, then in position order"""
    out = []
    for i in range(lo, hi):
        for p in positions(G, int(C["nodes"][i])):
            off = on_strand_offset(G, C, p)
            if off is not None and abs(off - pos) <= dev and not visited(G, C, p):
                out.append(p)
    return out


def window_split(lo, hi):
    """the SEED_PARTS parts of [lo, hi): whole rows of 64 offsets each, the same number per part, the last ones cut at hi or empty"""
    span = hi - lo
    per = (-(-span // SEED_PARTS) + 63) // 64 * 64
    return [(min(lo + p * per, hi), min(lo + (p + 1) * per, hi)) for p in range(SEED_PARTS)]


def seed_window_words(parts, stride, before):
    """per part `stride` words: the UNCLIPPED count, then the ids that fit; nothing else is touched"""
    out = np.array(before, dtype=np.uint32)
    for p, ids in enumerate(parts):
        o = out[p * stride:(p + 1) * stride]
        o[0] = len(ids)
        fit = ids[:stride - 1]
        o[1:1 + len(fit)] = fit
    return out


def window_candidates(words, stride):
    """rounds::window_candidates in three lines: the parts' ids in order, every id once, where it first occurs"""
    ids = [int(x) for p in range(SEED_PARTS) for x in words[p * stride + 1:p * stride + 1 + int(words[p * stride])]]
    return list(dict.fromkeys(ids))


# ---- k_checkpoints --------------------------------------------------------------------------------------------------------------
def checkpoint(G, C, left, right, dev):
    """the most abundant vertex that lies ON the strand — at an offset i of the window, within `dev` of i — and whose bit in the
    visited bitmap is not set (the bitmap alone: a strand vertex has its id in [g_lo, g_hi)); ties: the lowest offset, then the
    first position.  (vertex, contig coordinate, abundance) or (PAG_NONE, 0, 0)"""
    lo, hi = window_bounds(C, left, right)
    best, best_key = (PAG_NONE, 0, 0), None
    for i in range(lo, hi):
        node = int(C["nodes"][i])
        for rank, p in enumerate(positions(G, node)):
            off = on_strand_offset(G, C, p)
            if off is None or abs(off - i) > dev:
                continue
            u = int(G["newid"][p])
            if C.get("gbits") is not None and C["g_lo"] <= u < C["g_hi"] and C["gbits"][u - C["g_lo"]]:
                continue
            key = (int(G["vcnt"][p]), -i, -rank)
            if best_key is None or key > best_key:
                best_key, best = key, (p, int(G["vpos"][p]) >> 32, int(G["vcnt"][p]))
    return best


# ---- k_pack_paths ---------------------------------------------------------------------------------------------------------------
def pack_words(length, leap):
    """words of one job: three arrays (five for a leap job), then five words (+ two) per block of 64 entries"""
    return (5 if leap else 3) * length + -(-length // BLOCK) * (7 if leap else 5)


def _blocks(a, fill):
    a = np.asarray(a, dtype=np.uint32)
    pad = -len(a) % BLOCK
    return np.concatenate([a, np.full(pad, fill, dtype=np.uint32)]).reshape(-1, BLOCK)


def pack_job(G, v, s, x=None):
    """the words of one job: its vertices (new ids), its steps, the contig coordinates of its vertices (+ the two halves of its
    iteration log), then per block of 64 entries: the highest coordinate; 1 + the highest id among the coordinate-free entries (0:
    none); the lowest coordinate; the lowest coordinate that is not 0 (all ones: none); the sum of the steps (mod 2^32) — and for a
    leap job per block, over the entries with the boundary bit (63) set: the lowest `elow` (bits 32..62), the lowest m0 (the low
    word); all ones where a block has no such entry"""
    v, s = np.asarray(v, dtype=np.uint32), np.asarray(s, dtype=np.uint32)
    c = ctg_of(G["upos"][v]).astype(np.uint32)
    free = c == 0
    agg = np.stack([_blocks(c, 0).max(axis=1), _blocks(np.where(free, v + np.uint32(1), 0), 0).max(axis=1), _blocks(c, U32).min(axis=1),
                    _blocks(np.where(free, U32, c), U32).min(axis=1), _blocks(s, 0).sum(axis=1, dtype=np.uint32)], axis=1).reshape(-1)
    if x is None:
        return np.concatenate([v, s, c, agg])
    x = np.asarray(x, dtype=np.uint64)
    xl, xh = (x & np.uint64(U32)).astype(np.uint32), (x >> np.uint64(32)).astype(np.uint32)
    bd = (xh >> np.uint32(31)) != 0
    xagg = np.stack([_blocks(np.where(bd, xh & np.uint32(0x7FFFFFFF), U32), U32).min(axis=1), _blocks(np.where(bd, xl, U32), U32).min(axis=1)], axis=1).reshape(-1)
    return np.concatenate([v, s, c, xl, xh, agg, xagg])


def pack_job_loop(G, v, s, x=None):
    c = [int(G["upos"][int(u)]) >> 32 for u in v]
    out = [int(u) for u in v] + [int(t) for t in s] + c
    if x is not None:
        out += [int(e) & U32 for e in x] + [int(e) >> 32 for e in x]
    xagg = []
    for b in range(0, len(v), BLOCK):
        e = range(b, min(b + BLOCK, len(v)))
        free = [int(v[i]) + 1 for i in e if c[i] == 0]
        nz = [c[i] for i in e if c[i] != 0]
        out += [max(c[i] for i in e), max(free) if free else 0, min(c[i] for i in e), min(nz) if nz else U32, sum(int(s[i]) for i in e) & U32]
        if x is not None:
            bd = [int(x[i]) for i in e if int(x[i]) >> 63]
            xagg += [min((y >> 32) & 0x7FFFFFFF for y in bd) if bd else U32, min(y & U32 for y in bd) if bd else U32]
    return np.array(out + xagg, dtype=np.uint32)


# ---- k_commit -----------------------------------------------------------------------------------------------------------------
def commit(seq_v, in_lo, in_hi, bits_before=None):
    """a finished walk recorded: a bit per id inside [in_lo, in_hi) (bit (u - in_lo) & 31 of word (u - in_lo) >> 5), the other
    ids, each once, in the set"""
    v = np.asarray(seq_v, dtype=np.int64)
    inside = (v >= in_lo) & (v < in_hi)
    words = np.zeros((in_hi - in_lo + 31) // 32, dtype=np.uint32) if bits_before is None else np.array(bits_before, dtype=np.uint32)
    d = v[inside] - in_lo
    np.bitwise_or.at(words, d >> 5, (np.uint32(1) << (d & 31).astype(np.uint32)))
    return words, np.unique(v[~inside]).astype(np.uint32)


def commit_loop(seq_v, in_lo, in_hi):
    words, outside = [0] * ((in_hi - in_lo + 31) // 32), set()
    for u in seq_v:
        u = int(u)
        if in_lo <= u < in_hi:
            words[(u - in_lo) // 32] |= 1 << ((u - in_lo) % 32)
        else:
            outside.add(u)
    return np.array(words, dtype=np.uint32), np.array(sorted(outside), dtype=np.uint32)


def bits_to_bool(words, n):
    return ((np.asarray(words, dtype=np.uint32)[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


# ---- k_clear_ranges -------------------------------------------------------------------------------------------------------------
def clear_ranges(buf, ranges):
    """every byte of a range becomes byte (address & 3) of the range's word — whole copies of the word from any 4-byte boundary;
    buf starts on such a boundary (the hook's device buffer starts on a 256-byte one), so the address is the offset here"""
    out = np.array(buf, dtype=np.uint8)
    for off, n, word in ranges:
        a = np.arange(off, off + n)
        out[off:off + n] = (int(word) >> (8 * (a & 3))) & 0xFF
    return out


# ---- k_concat_parts -------------------------------------------------------------------------------------------------------------
def concat_parts(src_v, src_s, parts, out_v, out_s, first_step):
    """the parts of a chosen walk one behind the other; the step of the very first vertex (output index 0) becomes first_step"""
    ov, os_ = np.array(out_v, dtype=np.uint32), np.array(out_s, dtype=np.uint32)
    for frm, start, n in parts:
        ov[start:start + n] = src_v[frm:frm + n]
        os_[start:start + n] = src_s[frm:frm + n]
        if start == 0 and n:
            os_[0] = first_step
    return ov, os_


# ---- gathers --------------------------------------------------------------------------------------------------------------------
def gather_records(G, vertices, steps, dtype):
    """pag_path_node of k-mer-major vertices: code of the node, the two coordinates, abundance, the given step"""
    v = np.asarray(vertices, dtype=np.int64)
    out = np.zeros(len(v), dtype=dtype)
    out["code"] = G["ncode"][G["vnode"][v]]
    out["ctg"] = ctg_of(G["vpos"][v])
    out["ref"] = (G["vpos"][v] & np.uint64(U32)).astype(np.uint32)
    out["cnt"] = G["vcnt"][v]
    out["step"] = np.asarray(steps, dtype=np.uint32).astype(np.int32)
    out["vid"] = v
    return out


# ---- constructed strands ------------------------------------------------------------------------------------------------------
STRAND_LEFT = 5000  # single-coordinate of the constructed strands' first base


def strand_case(n_kmers, dev, spec, none=(), share=(), tail=2, default=None):
    """A strand [STRAND_LEFT, STRAND_LEFT + n_kmers + tail) whose k-mer at offset i has a node of its own (node ids are handed out in
    offset order; offsets in `none` have no node, the offsets of a tuple in `share` one node together).  spec[i] lists the
    positions of the node of offset i:
      an int d        contig coordinate STRAND_LEFT + i + d (one that falls off the strand is kept: the ctg_left / ctg_right edge)
      ("at", off)     contig coordinate STRAND_LEFT + off
      "rev"           a coordinate on the opposite strand
      "free"          no contig coordinate
      ("cnt", x, c)   x as above with abundance c
    An offset without an entry gets `default` ([dev + 1]: one position, out by one).  -> (graph, contig)"""
    left, right = STRAND_LEFT, STRAND_LEFT + n_kmers + tail
    owner = {i: grp[0] for grp in share for i in grp}
    nodes = np.full(n_kmers, PAG_NONE, dtype=np.uint32)
    poslists, node_of = [], {}
    for i in range(n_kmers):
        if i in none:
            continue
        o = owner.get(i, i)
        if o not in node_of:
            node_of[o] = len(poslists)
            poslists.append([])
        nodes[i] = node_of[o]
        for n, item in enumerate(spec.get(i, [dev + 1] if default is None else default)):
            cnt = 1 + (7 * i + n) % 50
            if isinstance(item, tuple) and item[0] == "cnt":
                item, cnt = item[1], item[2]
            ctg = right + 10 + i if item == "rev" else 0 if item == "free" else left + item[1] if isinstance(item, tuple) else left + i + item
            assert ctg >= 0
            poslists[nodes[i]].append((ctg, 100 + 3 * i + n, cnt))
    G = graph_from_lists(poslists)
    C = {"nodes": nodes, "ctg_left": left, "ctg_right": right, "gbits": None, "gset": None}
    C["g_lo"], C["g_hi"] = (int(x) for x in id_bounds(G, [left, right]))
    return G, C


def with_visited(G, C, vertices, g_lo=None, g_hi=None):
    """the contig after a walk over `vertices` (k-mer-major ids) was committed into a bitmap over [g_lo, g_hi) (default: the strand's
    own range) and a set for the rest"""
    D = dict(C)
    D["g_lo"], D["g_hi"] = C["g_lo"] if g_lo is None else g_lo, C["g_hi"] if g_hi is None else g_hi
    words, outside = commit(G["newid"][np.asarray(vertices, dtype=np.int64)], D["g_lo"], D["g_hi"])
    D["gbits"], D["gset"] = bits_to_bool(words, D["g_hi"] - D["g_lo"]), set(int(u) for u in outside)
    D["committed"] = G["newid"][np.asarray(vertices, dtype=np.int64)]  # (the walk, as new ids: what a device commit is given)
    return D


def vertices_at(G, C, i):
    return list(positions(G, int(C["nodes"][i])))


def strand_vertices_at(G, C, i):
    """the vertices of the k-mer at offset i that lie on the strand, in position order"""
    return [p for p in vertices_at(G, C, i) if on_strand_offset(G, C, p) is not None]


# ---- the constructed cases: each asserts here, without a device, that it has the shape it is named for ----------------------------
SEED_DEV = 3


def seed_first_cases():
    """[(name, graph, contig, dev, stride)]"""
    dev, out = SEED_DEV, []

    def add(name, n_kmers, spec, stride=64, want=None, **kw):
        G, C = strand_case(n_kmers, dev, spec, **kw)
        pairs = seed_first(G, C, dev)
        if want is not None:
            assert [(int(G["vpos"][p] >> np.uint64(32)) - C["ctg_left"], i) for p, i in pairs] == want, (name, pairs)
        out.append((name, G, C, dev, stride))
        return G, C, pairs

    add("one k-mer, its position at ctg_left", 1, {0: [0]}, want=[(0, 0)])
    add("63 k-mers, the hit in the last lane of a partial row", 63, {62: [1]}, want=[(63, 62)])
    add("the first hit in lane 0", 64, {0: [2]}, want=[(2, 0)])
    add("the first hit in lane 63", 64, {63: [-1]}, want=[(62, 63)])
    add("the first hit in the second row", 65, {64: [0]}, want=[(64, 64)])
    add("no hit anywhere", 200, {}, want=[])
    add("two lanes of one row hit: the lower offset's matching positions, all of them, none of the other's", 200,
        {70: [2, -3, dev + 1, 0], 75: [0, 1]}, want=[(67, 70), (70, 70), (72, 70)])
    add("distance dev in, dev + 1 out, on both sides", 200, {130: [dev, dev + 1, -dev, -dev - 1]}, want=[(130 - dev, 130), (130 + dev, 130)])
    G, C, _ = add("a position at ctg_right is out", 63, {62: [3]}, want=[])
    assert int(G["vpos"][vertices_at(G, C, 62)[0]] >> np.uint64(32)) == C["ctg_right"]
    add("ctg_right - 1 is in, ctg_right out, ctg_left - 1 out", 63, {1: [-2], 62: [3, 2]}, want=[(64, 62)])
    add("the opposite strand and vertices without a contig coordinate do not count", 100, {10: ["rev", "free"], 20: ["free", 0, "rev"]}, want=[(20, 20)])
    add("k-mers without a node", 100, {40: [0]}, none=(0, 1, 2, 30, 39, 41), want=[(40, 40)])
    add("a k-mer that occurs twice hits at its second offset only, with the position near that one", 150, {10: [50], 100: [0]}, share=[(10, 100)], want=[(100, 100)])
    five = {3: [0, 1, -1, 2, -2]}
    for stride, fit in ((4, 1), (8, 3), (64, 5)):
        G, C, pairs = add(f"five matches against a stride of {stride}", 20, five, stride=stride)
        assert len(pairs) == 5 and seed_first_words(pairs, stride, np.full(stride, 7))[0] == fit
    return out


WIN_DEV, WIN_POS, WIN_KMERS = 5, 1500, 3100


def seed_window_case():
    """one strand of 3 100 k-mers whose anchor is offset 1 500: matches (positions within dev of the ANCHOR) at chosen k-mer offsets,
    nothing matching elsewhere.  -> (graph, contig, dev, pos, {k-mer offset: matches})"""
    at = lambda e: ("at", WIN_POS + e)
    spec = {0: [at(0)], 63: [at(-5)], 64: [at(5), at(6)], 700: [at(-5), "rev", at(0), at(5), at(-6), "free"], 1023: [at(1)], 1024: [at(-1)],
            2001: [at(2)], 3099: [at(-2), at(3)]}
    for i in range(1400, 1410):
        spec[i] = [at(i - 1405), at(1404 - i)]
    G, C = strand_case(WIN_KMERS, WIN_DEV, spec, none=(5, 699, 2500), share=[(700, 1800)], default=["rev", "free"])
    n_match = {i: len(seed_window_range(G, C, i, i + 1, WIN_POS, WIN_DEV)) for i in range(WIN_KMERS)}
    assert {i: n for i, n in n_match.items() if n} == {0: 1, 63: 1, 64: 1, 700: 3, 1023: 1, 1024: 1, 1800: 3, 2001: 1, 3099: 2, **{i: 2 for i in range(1400, 1410)}}
    assert n_match[699] == 0 == n_match[701], "the lane with several matches stands beside lanes with none"
    return G, C, WIN_DEV, WIN_POS, n_match


def window_states(G, C, dev, pos):
    """the visited states the window is searched under: none; a bitmap over the strand's ids with the first and the last id of
    the range and two of the three matches of offset 700 set; a bitmap over a range NARROWER than the strand, so that for the
    matches outside it the hash set answers — some of them in it, some not"""
    m = lambda i: seed_window_range(G, C, i, i + 1, pos, dev)
    first, last = int(G["uold"][C["g_lo"]]), int(G["uold"][C["g_hi"] - 1])
    A = with_visited(G, C, [first, last] + m(700)[:2])
    assert A["gbits"][0] and A["gbits"][-1] and len(seed_window_range(G, A, 700, 701, pos, dev)) == 1
    gone = m(1405) + m(64) + m(3099)[:1] + m(1400)
    B = with_visited(G, C, gone, C["g_lo"] + 8, C["g_lo"] + 24)
    u = G["newid"][np.asarray(gone)]
    inside = (u >= B["g_lo"]) & (u < B["g_hi"])
    assert inside.any() and (~inside).any() and B["gset"], "visited matches on both sides of the narrow range"
    every = seed_window_range(G, C, 0, len(C["nodes"]), pos, dev)
    assert any(not (B["g_lo"] <= G["newid"][p] < B["g_hi"]) and not visited(G, B, p) for p in every), "no unvisited match for the hash set to deny"
    return [("no visited state", C), ("bitmap over the strand", A), ("narrow bitmap and hash set", B)]


# (left, right) of the window requests, and what each is there for
WINDOW_REQUESTS = [
    ((700, 700), "span 1: the lane with several matches alone"),
    ((56, 71), "span 16: one part, matches in lanes 7 and 8 of its row"),
    ((1, 1023), "span 1 023: sixteen parts of 64, the last one cut by one"),
    ((0, 1023), "span 1 024, left = 0: sixteen full parts"),
    ((0, 1024), "span 1 025: parts of 128, the ninth holds one offset, seven start beyond the end"),
    ((100, 3099), "span 3 000: parts of 192, the last one of 120"),
    ((2000, 3099), "matches in the first and in the last used part, none in between"),
    ((3000, 10 ** 9), "right beyond n_kmers - 1"),
    ((3100, 5000), "left at the end: every part reports 0"),
    ((4000, 4000), "left beyond the end"),
    ((1400, 1409), "a part with 20 matches"),
]


def check_window_requests(G, C, dev, pos):
    """the split of every request has the shape its name says"""
    shapes = {}
    for (left, right), name in WINDOW_REQUESTS:
        lo, hi = window_bounds(C, left, right)
        parts = window_split(lo, hi)
        used = [b - a for a, b in parts if b > a]
        assert sum(used) == hi - lo and all(a <= b for a, b in parts)
        shapes[(left, right)] = (used, [len(seed_window_range(G, C, a, b, pos, dev)) for a, b in parts])
    assert shapes[(1, 1023)][0] == [64] * 15 + [63] and shapes[(0, 1023)][0] == [64] * 16
    assert shapes[(0, 1024)][0] == [128] * 8 + [1] and shapes[(0, 1024)][1][8] == 1
    assert shapes[(100, 3099)][0] == [192] * 15 + [120]
    used, cnt = shapes[(2000, 3099)]
    assert len(used) == 9 and cnt[0] > 0 and cnt[8] > 0 and not any(cnt[1:8])
    assert shapes[(3000, 10 ** 9)][0] == [64, 36] and shapes[(3100, 5000)][0] == [] == shapes[(4000, 4000)][0]
    assert shapes[(1400, 1409)][1][0] == 20 and shapes[(700, 700)][1][0] == 3
    return shapes


def checkpoint_case():
    """one strand of 200 k-mers, every offset with one candidate of low abundance and a vertex without a coordinate.
    -> (graph, contig with a visited state, dev, [(left, right, name, vertex the rule must pick or None)])"""
    dev = SEED_DEV
    c = lambda x, n: ("cnt", x, n)
    spec = {i: [c(0, 1 + i % 40), "free"] for i in range(200)}
    spec[137] = [c(1, 65535), "free"]
    spec[20], spec[30] = [c(0, 500)], [c(0, 500)]
    spec[50] = [c(-1, 700), c(1, 700), c(0, 600)]
    spec[60] = [c("rev", 9000), c(dev + 1, 9000), c(0, 45)]
    spec[61] = [c(0, 8000)]
    G, C0 = strand_case(200, dev, spec)
    gone = vertices_at(G, C0, 61) + [p for i in (80, 81, 82) for p in vertices_at(G, C0, i)]
    C = with_visited(G, C0, gone)
    assert C["g_lo"] >= 64, "room for a bitmap that starts 64 ids below the strand"
    on60 = [p for p in vertices_at(G, C, 60) if on_strand_offset(G, C, p) == 60][0]
    reqs = [(137, 137, "a window of one offset; abundance 65 535", strand_vertices_at(G, C, 137)[0]),
            (10, 73, "64 offsets", None), (10, 74, "65 offsets", None),
            (10, 139, "130 offsets, the winner in the last lane of the second row", strand_vertices_at(G, C, 137)[0]),
            (15, 35, "equal abundances at two offsets: the lower offset", strand_vertices_at(G, C, 20)[0]),
            (45, 55, "equal abundances within one k-mer: the first position", strand_vertices_at(G, C, 50)[0]),
            (59, 61, "off the strand, beyond dev and visited candidates of higher abundance lose", on60),
            (80, 82, "every candidate visited", PAG_NONE),
            (190, 10 ** 6, "right beyond the strand", None), (500, 600, "left beyond the strand", PAG_NONE)]
    for left, right, name, want in reqs:
        got = checkpoint(G, C, left, right, dev)
        assert want is None or got[0] == want, (name, got, want)
    assert G["vcnt"][strand_vertices_at(G, C, 137)[0]] == 65535 and (137 - 10) == 127
    return G, C, dev, reqs


def pack_batches(rng, G):
    """two batches of jobs [(v, s, x or None)]: the lengths the issue names (one turn of the grid's stride: 16 384 entries), a
    40 000-entry job beside a 1-entry job, leap jobs (x) and others mixed"""
    n_pos, n_zero = G["n_pos"], G["n_zero"]
    assert 64 <= n_zero <= n_pos - 64

    def job(length, leap):
        v = rng.integers(0, n_pos, size=length).astype(np.uint32)
        if length >= 192:
            v[64:128] = rng.integers(0, n_zero, size=64)        # a block whose vertices all lack a contig coordinate
            v[128:192] = rng.integers(n_zero, n_pos, size=64)   # a block with none that do
        s = rng.integers(0, 1 << 24, size=length).astype(np.uint32)
        x = None
        if leap:
            x = rng.integers(0, 1 << 63, size=length, dtype=np.uint64) | (rng.integers(0, 2, size=length).astype(np.uint64) << np.uint64(63))
            x[rng.random(length) < 0.5] = 0
            if length >= 128:
                x[64:128] &= np.uint64((1 << 63) - 1)  # a block without a boundary
        return v, s, x

    a = [job(n, leap) for n, leap in ((1, False), (63, True), (64, False), (65, True), (16384, True), (16385, False), (16385, True), (1, True))]
    b = [job(40000, True), job(1, False), job(40000, False)]
    for batch in (a, b):
        assert max(len(j[0]) for j in batch) > PACK_TURN and min(len(j[0]) for j in batch) == 1, "a job of several turns beside a short one"
    c = ctg_of(G["upos"][a[4][0]])
    assert (c[64:128] == 0).all() and (c[128:192] != 0).all() and len(a[5][0]) % BLOCK, "all-free block, none-free block, last partial block"
    assert (a[4][2] >> np.uint64(63)).any() and not (a[4][2][64:128] >> np.uint64(63)).any()
    return a, b


def pack_layout(batch):
    """word offsets of the jobs in the packed buffer, one untouched word between two jobs -> (offsets, total words)"""
    offs, at = [], 1
    for v, _, x in batch:
        offs.append(at)
        at += pack_words(len(v), x is not None) + 1
    return offs, at
