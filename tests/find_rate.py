"""Probe (a script, not a test): what does it cost to learn which vertices of the graph stand along the contigs?

Builds the bench workload (aligngraph2_amd/workload.py; the defaults are BASELINE configs[1]: 100k x 10 kb reads, 50 Mb reference,
k = 14), runs pag_prepare + pag_process, and asks pag_find_all_batch for every contig in both strands: in one call (sizing only,
then the full call), then in calls of one contig each.  One JSON line per measurement to --out: hits and vertices, ms_kernels (device
time of the call's kernels: the lists are counted, scanned, filled), the device bytes the call is stated to take
(pag_find_all_batch_bytes), the wall time of the call with its copies.  Beside them the only way the library offered before to learn
the same thing: pag_export_csr to the host, and a numpy.searchsorted of the contigs' k-mer codes over the exported node codes.

    python tests/find_rate.py [--reads N --ref-len N] [--out profiles/find_rate.json]
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


def strand_codes(bases, k, reverse):
    """the k-mer codes of a strand of 2-bit bases, first base most significant"""
    b = (3 - bases[::-1]) if reverse else bases
    n = len(b) - k + 1
    c = np.zeros(max(n, 0), dtype=np.uint32)
    for i in range(k):
        c = (c << np.uint32(2)) | b[i:i + n]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-span", type=int, default=10_000)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_rate.json"))
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
    st = capi.BuildStats()
    if hip.pag_prepare(g, C.byref(raw), C.byref(inp)) != 0 or hip.pag_process(g, C.byref(inp), C.byref(st)) != 0:
        raise SystemExit(f"build failed: {hip.pag_last_error().decode()}")
    ctg_codes = w.contig_codes()
    _, (packed, ctg_off, ctg_len) = host_seqs(ctg_codes)
    n_ctg = len(ctg_codes)
    packed_bytes = len(packed) - 64  # (host_seqs' padding)
    # every contig forward, then every contig reverse
    byte_off = np.concatenate((ctg_off, ctg_off))
    lengths = np.concatenate((ctg_len, ctg_len))
    reverse = np.concatenate((np.zeros(n_ctg, dtype=np.uint8), np.ones(n_ctg, dtype=np.uint8)))
    n_hits, n_vert, ms = C.c_uint64(), C.c_uint64(), C.c_double()

    def call(pick, hit_off, hits, vert):
        bo, ln, rv = np.ascontiguousarray(byte_off[pick]), np.ascontiguousarray(lengths[pick]), np.ascontiguousarray(reverse[pick])
        # (the packed bytes the picked sequences span, not the whole array: the call copies what it is given)
        base = int(bo.min())
        bo -= np.uint64(base)
        span = int((bo + (ln.astype(np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(4)).max())
        seqs = capi.PagSeqs(len(pick), bo.ctypes.data, ln.ctypes.data, packed.ctypes.data + base, span)
        t0 = time.perf_counter()
        rc = hip.pag_find_all_batch(g, C.byref(seqs), rv.ctypes.data, hit_off.ctypes.data, hits.ctypes.data if hits is not None else None,
                                    len(hits) if hits is not None else 0, vert.ctypes.data if vert is not None else None,
                                    len(vert) if vert is not None else 0, C.byref(n_hits), C.byref(n_vert), C.byref(ms))
        wall = time.perf_counter() - t0
        call.span = span
        return rc, wall

    common = {"workload": name, "k": spec.k, "graph": {"tuples": int(st.n_tuples[0] + st.n_tuples[1]), "nodes": int(st.n_nodes), "vertices": int(st.n_pos)},
              "contigs": n_ctg, "bases_searched": int(lengths.sum()), "solid_kmers": int(hip.pag_solid_count(g))}
    lines = []

    def line(what, **more):
        d = dict(common, measurement=what, **more)
        lines.append(d)
        print(json.dumps(d), flush=True)

    everything = np.arange(2 * n_ctg)
    hit_off = np.zeros(2 * n_ctg + 1, dtype=np.uint64)
    rc, wall = call(everything, hit_off, None, None)
    if rc not in (capi.PAG_OK, capi.PAG_ERANGE):
        raise SystemExit(f"pag_find_all_batch failed ({rc}): {hip.pag_last_error().decode()}")
    nh, nv = n_hits.value, n_vert.value
    line("one call, sizing only (count + scan)", sequences=2 * n_ctg, hits=nh, vertices=nv, ms_kernels=ms.value, wall_s_with_copies=wall,
         device_bytes=hip.pag_find_all_batch_bytes(2 * n_ctg, packed_bytes, 0, 0))
    hits = np.zeros(nh, dtype=capi.FIND_HIT_DTYPE)
    vert = np.zeros(nv, dtype=capi.FIND_VERTEX_DTYPE)
    rc, wall = call(everything, hit_off, hits, vert)
    if rc != capi.PAG_OK:
        raise SystemExit(f"pag_find_all_batch failed ({rc}): {hip.pag_last_error().decode()}")
    line("one call (count + scan + fill)", sequences=2 * n_ctg, hits=nh, vertices=nv, ms_kernels=ms.value, wall_s_with_copies=wall,
         device_bytes=hip.pag_find_all_batch_bytes(2 * n_ctg, packed_bytes, nh, nv), hits_per_s=nh / (ms.value * 1e-3),
         vertices_per_s=nv / (ms.value * 1e-3), hits_without_a_node=int((hits["n_pos"] == 0).sum()), most_positions_of_a_hit=int(hits["n_pos"].max()))
    rc, wall = call(everything, hit_off, hits, None)
    if rc != capi.PAG_OK:
        raise SystemExit(f"pag_find_all_batch failed ({rc}): {hip.pag_last_error().decode()}")
    line("one call, hits only (count + scan + fill without the vertex copy)", sequences=2 * n_ctg, hits=nh, vertices=nv, ms_kernels=ms.value,
         wall_s_with_copies=wall, device_bytes=hip.pag_find_all_batch_bytes(2 * n_ctg, packed_bytes, nh, 0))
    found_by_call = int((hits["n_pos"] != 0).sum())
    whole_off = hit_off.copy()
    # a contig per call, both strands
    ms_sum = wall_sum = 0.0
    peak = 0
    two = np.zeros(3, dtype=np.uint64)
    for c in range(n_ctg):
        rc, wall = call(np.array([c, n_ctg + c]), two, hits, vert)
        if rc != capi.PAG_OK or n_hits.value != int(whole_off[c + 1] - whole_off[c] + whole_off[n_ctg + c + 1] - whole_off[n_ctg + c]):
            raise SystemExit(f"pag_find_all_batch failed ({rc}) for contig {c}: {hip.pag_last_error().decode()}")
        ms_sum += ms.value
        wall_sum += wall
        peak = max(peak, hip.pag_find_all_batch_bytes(2, call.span, n_hits.value, n_vert.value))
    line("calls of one contig each (both strands)", calls=n_ctg, hits=nh, vertices=nv, ms_kernels=ms_sum, wall_s_with_copies=wall_sum, device_bytes=peak)
    del hits, vert
    # the way there was before: the whole graph to the host, the contigs' codes looked up in the exported node codes
    nn, npos, ne = C.c_uint64(), C.c_uint64(), C.c_uint64()
    t0 = time.perf_counter()
    hip.pag_csr_sizes(g, C.byref(nn), C.byref(npos), C.byref(ne))
    out = [np.empty(nn.value, np.uint32), np.empty(nn.value + 1, np.uint64), np.empty(npos.value, np.uint32), np.empty(npos.value, np.uint32),
           np.empty(npos.value, np.uint16), np.empty(nn.value + 1, np.uint64), np.empty(ne.value, np.uint32), np.empty(ne.value, np.int32)]
    csr = capi.Csr(nn.value, npos.value, ne.value, *[a.ctypes.data for a in out])
    if hip.pag_export_csr(g, C.byref(csr)) != 0:
        raise SystemExit(f"pag_export_csr failed: {hip.pag_last_error().decode()}")
    t_export = time.perf_counter() - t0
    t0 = time.perf_counter()
    codes = np.concatenate([strand_codes(b, spec.k, r) for r in (False, True) for b in ctg_codes])
    t_codes = time.perf_counter() - t0
    t0 = time.perf_counter()
    at = np.minimum(np.searchsorted(out[0], codes), len(out[0]) - 1)
    found = out[0][at] == codes
    n_found = int(found.sum())
    n_found_vert = int((out[1][at + 1] - out[1][at])[found].sum())
    t_search = time.perf_counter() - t0
    line("pag_export_csr to the host + numpy.searchsorted of the contigs' codes", exported_bytes=int(sum(a.nbytes for a in out)), wall_s_export=t_export,
         wall_s_codes_in_numpy=t_codes, wall_s_searchsorted=t_search, wall_s=t_export + t_codes + t_search, offsets=int(len(codes)), offsets_with_a_node=n_found,
         vertices=n_found_vert, agrees_with_the_call=bool(n_found == found_by_call and n_found_vert == nv))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")
    hip.pag_destroy(g)


if __name__ == "__main__":
    main()
