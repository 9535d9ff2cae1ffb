"""Probe (a script, not a test): what does a straight walk cost ON DEMAND?

Builds the bench workload (aligngraph2_amd/workload.py; the defaults are BASELINE configs[1]: 100k x 10 kb reads, 50 Mb reference,
k = 14), runs pag_travel (--blocks times over: the last run works from a settled pool) and takes the delivered paths.  The queries
are the straight pieces along them: a walk starts at the first vertex of every path and at every path vertex BEHIND A BRANCH — a
vertex whose predecessor's successor list (pag_successors_batch, one call, not measured) holds other than one record in its best
class (Amazing, else Excellent, else Good).  Every query walks under its contig strand's frame with empty tables (ctgRange and
the other strand from PositionMapper, splitSize = int(len * 0.9), splitMin = 1 - 0.9), dist = k, has_size = 0, limit 4 096.
pag_walk_straight_batch answers them all in one call, then the same queries in --calls calls.  One JSON line per measurement
to --out: ms_kernels (device time of the call's kernels: the walks are counted, scanned, filled), queries and path vertices
per second of that time, the device bytes the call is stated to allocate (pag_walk_straight_batch_bytes), the wall time of the
call with its copies; beside them pag_travel_stats.ms_compact and ms_walk of the same run: what the view with every list costs,
and what the walker takes to walk it.

    python tests/walk_straight_rate.py [--reads N --ref-len N] [--out profiles/walk_straight_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import aligngraph2_amd  # noqa: E402
from aligngraph2_amd import capi, workload  # noqa: E402
from bench import host_seqs  # noqa: E402

LIMIT = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-span", type=int, default=10_000)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=3, help="build + pag_travel runs before the queries; ms_compact and ms_walk of each are reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_straight_rate.json"))
    args = ap.parse_args()
    hip = aligngraph2_amd.load_hip()
    spec = workload.BigSpec(seed=2, ref_len=args.ref_len, n_reads=args.reads, read_span=args.read_span, k=args.k, eps=10, cov=2, threads=16)
    w = workload.BigWorkload(spec, device="cuda:0")
    torch.cuda.synchronize()
    name = "BASELINE configs[1]" if (args.reads, args.read_span, args.ref_len, args.k) == (100_000, 10_000, 50_000_000, 14) else \
        f"{args.reads} reads x {args.read_span}, reference {args.ref_len}, k {args.k} (not a BASELINE configuration)"
    raw = w.raw_input()
    inp = workload.PagBuildInput()
    err = C.c_int()
    g = C.c_void_p(hip.pag_create_from_bitmap(w.solid_bits.data_ptr(), w.n_solid, spec.k, 1, 0, C.byref(err)))
    if not g:
        raise SystemExit(f"pag_create_from_bitmap failed ({err.value}): {hip.pag_last_error().decode()}")
    ctg_seqs, keep = host_seqs(w.contig_codes())
    ctg_len = keep[2]
    orient = np.array([0 if r else 1 for _, _, r in w.ctgs], dtype=np.int32)
    ref_len = np.array([len(w.ref)], dtype=np.uint32)
    prm = capi.TravelParams(spec.threads, 0, 2 * spec.eps, 0.15, 0.90, 50)
    st, ts = capi.BuildStats(), capi.TravelStats()
    compact, walk = [], []
    for _ in range(args.blocks):  # (the same block again: the handle's pool settles in its third, bench.py --warmup)
        if hip.pag_prepare(g, C.byref(raw), C.byref(inp)) != 0 or hip.pag_process(g, C.byref(inp), C.byref(st)) != 0:
            raise SystemExit(f"build failed: {hip.pag_last_error().decode()}")
        if hip.pag_travel(g, C.byref(ctg_seqs), orient.ctypes.data, ref_len.ctypes.data, 1, C.byref(prm), C.byref(ts)) != 0:
            raise SystemExit(f"pag_travel failed: {hip.pag_last_error().decode()}")
        compact.append(ts.ms_compact)
        walk.append(ts.ms_walk)
    # PositionMapper over the contigs (position_mapper.hpp:18-25): strand c forward at [start, start + len), reverse 2 len further
    sizes = [int(x) for x in ctg_len]
    start = [sizes[0]]
    for i in range(1, len(sizes)):
        start.append(start[-1] + 3 * sizes[i - 1] + max(sizes[i - 1], sizes[i]))
    # the delivered paths, one frame per path
    node = capi.DTYPES["pag_path_node"]
    parts, frames, frame_of_part = [], [], []
    for c in range(len(w.ctgs)):
        n = C.c_uint64()
        p = hip.pag_travel_path_oriented(g, c, int(orient[c] != 0), C.byref(n))
        if not p or not n.value:
            continue
        path = np.frombuffer(C.string_at(p, n.value * node.itemsize), dtype=node)
        on_ctg = path["ctg"][path["ctg"] != 0]
        fwd, rev = start[c], start[c] + 2 * sizes[c]
        own, other = (fwd, rev) if len(on_ctg) == 0 or fwd <= int(on_ctg[0]) < fwd + sizes[c] else (rev, fwd)
        frame_of_part.append(len(frames))
        frames.append((own, own + sizes[c], other, other + sizes[c], int(sizes[c] * 0.9), 1 - 0.9, [0xFFFFFFFF, 0xFFFFFFFF], [0, 0], 0, 0))
        parts.append(path)
    frames = np.array(frames, dtype=capi.WALK_FRAME_DTYPE)
    path = np.concatenate(parts)
    first = np.cumsum([0] + [len(p) for p in parts[:-1]])
    pos = (path["ctg"].astype(np.uint64) << np.uint64(32)) | path["ref"].astype(np.uint64)
    # the branches: the best class of every path vertex's list (one pag_successors_batch call)
    off, status, rec = aligngraph2_amd.successors_batch(hip, g, path["code"], pos, prm.deviation, prm.error_rate)
    off = off.astype(np.int64)
    cls = np.array([9, 9, 2, 1, 0], dtype=np.int8)[rec["grade"]]  # (Skip is no class before leaping is allowed)
    owner = np.repeat(np.arange(len(path)), np.diff(off))
    best = np.minimum.reduceat(np.concatenate((cls, np.array([9], dtype=np.int8))), off[:-1])  # (the sentinel: lists at the end may be empty)
    best[np.diff(off) == 0] = 9
    in_best = np.bincount(owner[cls == best[owner]], minlength=len(path))
    in_best[best == 9] = 0
    is_start = np.zeros(len(path), dtype=bool)
    is_start[1:] = in_best[:-1] != 1
    is_start[first] = True
    at = np.flatnonzero(is_start)
    q = np.zeros(len(at), dtype=capi.WALK_QUERY_DTYPE)
    q["code"], q["pos"], q["dist"], q["limit"] = path["code"][at], pos[at], spec.k, LIMIT
    q["frame"] = np.repeat(np.array(frame_of_part), [len(p) for p in parts])[at]
    n_q = len(q)
    none = np.zeros(0, dtype=capi.SUCC_QUERY_DTYPE)
    node_off, alt_off = np.zeros(n_q + 1, dtype=np.uint64), np.zeros(n_q + 1, dtype=np.uint64)
    wstatus = np.zeros(n_q, dtype=np.int32)
    n_nodes, n_alts, ms = C.c_uint64(), C.c_uint64(), C.c_double()

    def call(lo, hi, nodes, alts):
        t0 = time.perf_counter()
        rc = hip.pag_walk_straight_batch(g, q[lo:hi].ctypes.data, hi - lo, frames.ctypes.data, len(frames), none.ctypes.data, 0, ctg_len.ctypes.data, len(ctg_len),
                                         prm.deviation, prm.error_rate, node_off[lo:].ctypes.data, None if nodes is None else nodes.ctypes.data,
                                         0 if nodes is None else len(nodes), alt_off[lo:].ctypes.data, None if alts is None or not len(alts) else alts.ctypes.data,
                                         0 if alts is None else len(alts), wstatus[lo:].ctypes.data, C.byref(n_nodes), C.byref(n_alts), C.byref(ms))
        return rc, time.perf_counter() - t0

    common = {"workload": name, "graph": {"tuples": int(st.n_tuples[0] + st.n_tuples[1]), "vertices": int(st.n_pos), "unique_edges": int(st.n_uniq_edges)},
              "pag_travel_of_the_same_run": {"ms_compact_per_block": compact, "ms_walk_per_block": walk, "ms_compact": compact[-1], "ms_walk": walk[-1],
                                             "path_vertices": int(len(path)), "paths": len(parts)},
              "deviation": int(prm.deviation), "error_rate": prm.error_rate, "limit": LIMIT}
    lines = []

    def line(what, n, vertices, ms_kernels, wall, device_bytes, **more):
        d = dict(common, measurement=what, queries=n, path_vertices_walked=vertices, ms_kernels=ms_kernels, queries_per_s=n / (ms_kernels * 1e-3),
                 vertices_per_s=vertices / (ms_kernels * 1e-3), ns_per_vertex=ms_kernels * 1e6 / max(vertices, 1), device_bytes=device_bytes,
                 wall_s_with_copies=wall, **more)
        lines.append(d)
        print(json.dumps(d), flush=True)

    # the sizing call: the walks are counted and scanned, nothing is filled
    rc, wall = call(0, n_q, None, None)
    if rc not in (capi.PAG_OK, capi.PAG_ERANGE):
        raise SystemExit(f"pag_walk_straight_batch failed ({rc}): {hip.pag_last_error().decode()}")
    nn, na = n_nodes.value, n_alts.value
    whole_n, whole_a = node_off.astype(np.int64), alt_off.astype(np.int64)
    lengths = np.diff(whole_n)
    line("one call, sizing only (count + scan)", n_q, nn, ms.value, wall, hip.pag_walk_straight_batch_bytes(n_q, len(frames), 0, 0, 0),
         statuses={str(s): int(c) for s, c in zip(*np.unique(wstatus, return_counts=True))}, alternatives=na,
         walk_length={"mean": float(lengths.mean()), "median": float(np.median(lengths)), "p99": float(np.percentile(lengths, 99)), "max": int(lengths.max())})
    nodes, alts = np.zeros(nn, dtype=capi.WALK_NODE_DTYPE), np.zeros(na, dtype=capi.SUCC_DTYPE)
    rc, wall = call(0, n_q, nodes, alts)
    if rc != capi.PAG_OK:
        raise SystemExit(f"pag_walk_straight_batch failed ({rc}): {hip.pag_last_error().decode()}")
    line("one call (count + scan + fill)", n_q, nn, ms.value, wall, hip.pag_walk_straight_batch_bytes(n_q, len(frames), 0, nn, na))
    # the same queries in --calls calls
    ms_sum = wall_sum = 0.0
    peak = calls = 0
    per = (n_q + args.calls - 1) // args.calls
    for lo in range(0, n_q, per):
        hi = min(n_q, lo + per)
        n_b, a_b = int(whole_n[hi] - whole_n[lo]), int(whole_a[hi] - whole_a[lo])
        rc, wall = call(lo, hi, nodes[:n_b], alts[:a_b])
        if rc != capi.PAG_OK or n_nodes.value != n_b or n_alts.value != a_b:
            raise SystemExit(f"pag_walk_straight_batch failed ({rc}) in the batch at {lo}: {hip.pag_last_error().decode()}")
        ms_sum += ms.value
        wall_sum += wall
        peak = max(peak, hip.pag_walk_straight_batch_bytes(hi - lo, len(frames), 0, n_b, a_b))
        calls += 1
    line(f"{calls} calls of {per} queries", n_q, nn, ms_sum, wall_sum, peak, calls=calls)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")
    hip.pag_destroy(g)


if __name__ == "__main__":
    main()
