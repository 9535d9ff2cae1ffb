"""Probe (a script, not a test): what does a successor list cost ON DEMAND?

Builds the bench workload (aligngraph2_amd/workload.py; the defaults are BASELINE configs[1]: 100k x 10 kb reads, 50 Mb reference,
k = 14), runs pag_travel once (--blocks times over: the last run's successor stage works from a settled pool), takes the vertices of the
delivered paths — the vertices a traversal actually stands on — and asks pag_successors_batch for their lists: all in one call,
then in calls of --batch vertices.  One JSON line per measurement to --out: ms_kernels (device time of the call's kernels: the
lists are counted, scanned, filled), queries and records per second of that time, the device bytes the call allocated
(pag_successors_batch_bytes), the wall time of the call with its copies; beside them pag_travel_stats.ms_compact of the same
run: what it costs to have EVERY list of the view ready before the first walk.

    python tests/succ_query_rate.py [--reads N --ref-len N] [--out profiles/succ_query_rate.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-span", type=int, default=10_000)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--blocks", type=int, default=5, help="build + pag_travel runs before the queries; ms_compact of each is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "succ_query_rate.json"))
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
    orient = np.array([0 if r else 1 for _, _, r in w.ctgs], dtype=np.int32)
    ref_len = np.array([len(w.ref)], dtype=np.uint32)
    prm = capi.TravelParams(spec.threads, 0, 2 * spec.eps, 0.15, 0.90, 50)
    st, ts = capi.BuildStats(), capi.TravelStats()
    compact = []
    for _ in range(args.blocks):  # (the same block again: the handle's pool settles in its third, bench.py --warmup)
        if hip.pag_prepare(g, C.byref(raw), C.byref(inp)) != 0 or hip.pag_process(g, C.byref(inp), C.byref(st)) != 0:
            raise SystemExit(f"build failed: {hip.pag_last_error().decode()}")
        if hip.pag_travel(g, C.byref(ctg_seqs), orient.ctypes.data, ref_len.ctypes.data, 1, C.byref(prm), C.byref(ts)) != 0:
            raise SystemExit(f"pag_travel failed: {hip.pag_last_error().decode()}")
        compact.append(ts.ms_compact)
    vn, vp, ve, vs, cut, fb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint64()
    hip.pag_travel_view_sizes(g, C.byref(vn), C.byref(vp), C.byref(ve), C.byref(vs), C.byref(cut), C.byref(fb))
    # the vertices of the delivered paths
    node = capi.DTYPES["pag_path_node"]
    parts = []
    for c in range(len(w.ctgs)):
        n = C.c_uint64()
        p = hip.pag_travel_path_oriented(g, c, int(orient[c] != 0), C.byref(n))
        if p and n.value:
            parts.append(np.frombuffer(C.string_at(p, n.value * node.itemsize), dtype=node))
    path = np.concatenate(parts)
    q = np.zeros(len(path), dtype=np.dtype(capi.PagSuccQuery))
    q["code"] = path["code"]
    q["pos"] = (path["ctg"].astype(np.uint64) << np.uint64(32)) | path["ref"].astype(np.uint64)
    n_q = len(q)
    off = np.zeros(n_q + 1, dtype=np.uint64)
    status = np.zeros(n_q, dtype=np.int32)
    total, ms = C.c_uint64(), C.c_double()

    def call(lo, hi, out, cap):
        t0 = time.perf_counter()
        rc = hip.pag_successors_batch(g, q[lo:hi].ctypes.data, hi - lo, prm.deviation, prm.error_rate, off[lo:].ctypes.data, status[lo:].ctypes.data,
                                      out.ctypes.data if cap else None, cap, C.byref(total), C.byref(ms))
        return rc, time.perf_counter() - t0

    common = {"workload": name, "graph": {"tuples": int(st.n_tuples[0] + st.n_tuples[1]), "vertices": int(st.n_pos), "unique_edges": int(st.n_uniq_edges)},
              "ms_compact_of_the_same_run": {"per_block": compact, "last": compact[-1], "view_vertices": vp.value, "view_records": vs.value, "view_cut": cut.value},
              "deviation": int(prm.deviation), "error_rate": prm.error_rate}
    lines = []

    def line(what, n, records, ms_kernels, wall, device_bytes, **more):
        d = dict(common, measurement=what, queries=n, records=records, ms_kernels=ms_kernels, queries_per_s=n / (ms_kernels * 1e-3),
                 records_per_s=records / (ms_kernels * 1e-3), device_bytes=device_bytes, wall_s_with_copies=wall, **more)
        lines.append(d)
        print(json.dumps(d), flush=True)

    # the sizing call: the lists are counted and scanned, nothing is filled
    rc, wall = call(0, n_q, None, 0)
    if rc not in (capi.PAG_OK, capi.PAG_ERANGE):
        raise SystemExit(f"pag_successors_batch failed ({rc}): {hip.pag_last_error().decode()}")
    n_rec = total.value
    missing = int(np.count_nonzero(status))
    whole_off = off.copy()
    line("one call, sizing only (count + scan)", n_q, n_rec, ms.value, wall, hip.pag_successors_batch_bytes(n_q, 0), vertices_not_in_the_graph=missing,
         distinct_queries=int(len(np.unique(q))))
    out = np.zeros(n_rec, dtype=np.dtype(capi.PagSucc))
    rc, wall = call(0, n_q, out, n_rec)
    if rc != capi.PAG_OK:
        raise SystemExit(f"pag_successors_batch failed ({rc}): {hip.pag_last_error().decode()}")
    line("one call (count + scan + fill)", n_q, n_rec, ms.value, wall, hip.pag_successors_batch_bytes(n_q, n_rec))
    grades = np.bincount(out["grade"], minlength=5).tolist()
    # in calls of --batch vertices
    ms_sum = wall_sum = 0.0
    peak = calls = 0
    for lo in range(0, n_q, args.batch):
        hi = min(n_q, lo + args.batch)
        n_b = int(whole_off[hi] - whole_off[lo])
        rc, wall = call(lo, hi, out, n_b)
        if rc != capi.PAG_OK or total.value != n_b:
            raise SystemExit(f"pag_successors_batch failed ({rc}) in the batch at {lo}: {hip.pag_last_error().decode()}")
        ms_sum += ms.value
        wall_sum += wall
        peak = max(peak, hip.pag_successors_batch_bytes(hi - lo, n_b))
        calls += 1
    line(f"calls of {args.batch} vertices", n_q, n_rec, ms_sum, wall_sum, peak, calls=calls, grades_of_the_one_call=grades)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")
    hip.pag_destroy(g)


if __name__ == "__main__":
    main()
