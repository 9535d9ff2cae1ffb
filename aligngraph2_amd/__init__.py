"""aligngraph2_amd — MI355X-native PAGraph hot path of AlignGraph2.

The product is native: `aligngraph2_amd/bin/pagraph` (host C++, drop-in for the reference's pagraph
command line) on top of `aligngraph2_amd/libpagraph_hip.so` (hand-written HIP kernels for gfx950 behind
the C ABI of include/pagraph_hip.h).  This Python package only locates / builds / launches them; capi.py is its one
restatement of that ABI for ctypes (load_hip() / load_host() bind it).
There is no CPU fallback: without the HIP library (or without a gfx950 device) everything raises.
"""
import ctypes as C
import os
import subprocess
import tempfile

from . import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(PKG, "libpagraph_hip.so")
HOST_LIB = os.path.join(PKG, "libpagraph_host.so")
PAGRAPH = os.path.join(PKG, "bin", "pagraph")
PA_CNS = os.path.join(PKG, "bin", "pa_cns")


def build(targets=("product",)):
    """Compile the HIP library (hipcc --offload-arch=gfx950) and the pagraph executable in-tree."""
    subprocess.run(["make", "-C", ROOT, *targets], check=True)


def require_built():
    for f in (LIB, PAGRAPH):
        if not os.path.exists(f):
            raise RuntimeError(f"{f} is missing — run aligngraph2_amd.build(); there is no CPU fallback")


def run_pagraph(argv, **kw):
    """Run the drop-in executable with the reference's argv (AlignGraph2.py:414-427) minus argv[0]."""
    require_built()
    return subprocess.run([PAGRAPH, *argv], **kw)


def run_pa_cns_batch(jobs, part_len=5000, top_k=3000, alpha=250, threads=16, **kw):
    """The consensus step for many contigs in one run (`pa_cns --batch`): jobs is a sequence of (backbone FASTA, 3-line ALN file,
    output FASTA), the parts of all of them go through the graph stage together.  Every output file and the three stdout lines per
    job, in the order of jobs, are what one `pa_cns -i -a -o` run per job writes (AlignGraph2.py:500-510).  **kw goes to
    subprocess.run; returns the CompletedProcess."""
    if not os.path.exists(PA_CNS):
        raise RuntimeError(f"{PA_CNS} is missing — run aligngraph2_amd.build()")
    jobs = [tuple(os.fspath(p) for p in job) for job in jobs]
    for job in jobs:
        if len(job) != 3 or any("\t" in p or "\n" in p or not p for p in job):
            raise ValueError(f"a job is (backbone, alignments, output), three paths without TAB or newline: {job!r}")
    with tempfile.NamedTemporaryFile("w", suffix=".pa_cns_batch.tsv") as manifest:
        manifest.write("".join("\t".join(job) + "\n" for job in jobs))
        manifest.flush()
        return subprocess.run([PA_CNS, "-t", str(threads), "-l", str(part_len), "-k", str(top_k), "--alpha", str(alpha), "--batch", manifest.name], **kw)


_hip = {}
_host = {}


def load_hip():
    """libpagraph_hip.so through ctypes (the C ABI of include/pagraph_hip.h, typed by capi.SIGNATURES).  Raises if it has not
    been built: there is no CPU fallback.  One HIP runtime per process: torch bundles its own libamdhip64 (same SONAME as /opt/rocm's); if our library
    were loaded first it would pull in the system runtime and a later `import torch` would mix it with torch's HSA ("no
    ROCm-capable device"), so torch is loaded first and both share torch's."""
    if "lib" not in _hip:
        if not os.path.exists(LIB):
            raise RuntimeError(f"{LIB} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        import torch
        torch.cuda.is_available()
        _hip["lib"] = capi.bind(C.CDLL(LIB))
    return _hip["lib"]


def load_host():
    """libpagraph_host.so through ctypes (include/pagraph_host.h, typed by capi.SIGNATURES).  It links libpagraph_hip.so, so
    that one is loaded first (load_hip: torch's HIP runtime before ours)."""
    if "lib" not in _host:
        load_hip()
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"{HOST_LIB} is missing: run __graft_entry__.build()")
        _host["lib"] = capi.bind(C.CDLL(HOST_LIB))
    return _host["lib"]


def _sized_then_filled(hip, name, call, totals, dtypes):
    """The two calls of a batch query `name` of the bound library `hip`: call(buf0, cap0, buf1, cap1, ...) with no room (the
    sizing call; it leaves the counts in `totals`, ctypes integers, the first one the count without which nothing is filled),
    then with numpy arrays of `dtypes` that hold them (an empty array goes as a null pointer).  Returns the arrays."""
    import numpy as np

    rc = call(*(None, 0) * len(totals))
    if rc not in (capi.PAG_OK, capi.PAG_ERANGE) or (rc == capi.PAG_ERANGE and totals[0].value == 0):
        raise RuntimeError(f"{name} failed ({rc}): {hip.pag_last_error().decode()}")
    bufs = [np.zeros(t.value, dtype=d) for t, d in zip(totals, dtypes)]
    if totals[0].value:
        rc = call(*(x for b in bufs for x in (b.ctypes.data if len(b) else None, len(b))))
        if rc != capi.PAG_OK:
            raise RuntimeError(f"{name} failed ({rc}): {hip.pag_last_error().decode()}")
    return bufs


def successors_batch(hip, g, codes, pos, deviation, error_rate):
    """pag_successors_batch (include/pagraph_hip.h) for the vertices (codes[i], pos[i]) of the finished graph in handle `g` of
    the bound library `hip`: a sizing call, then the real one.  Returns (off, status, records): off[n + 1] uint64, status[n]
    int32 (capi.PAG_OK, or capi.PAG_EINVAL where the graph holds no such vertex: an empty list), records off[-1] entries of
    capi.PagSucc as a numpy record array (code, step, pos, grade, ctg_similar), list i at records[off[i]:off[i + 1]]."""
    import numpy as np

    codes = np.asarray(codes)
    pos = np.asarray(pos)
    if codes.shape != pos.shape or codes.ndim != 1:
        raise ValueError("codes and pos are one-dimensional arrays of the same length")
    n = len(codes)
    q = np.zeros(n, dtype=np.dtype(capi.PagSuccQuery))
    q["code"], q["pos"] = codes, pos
    off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    total = C.c_uint64()
    handle = g if isinstance(g, C.c_void_p) else C.c_void_p(g)

    def call(out, cap):
        return hip.pag_successors_batch(handle, q.ctypes.data, n, int(deviation), float(error_rate), off.ctypes.data, status.ctypes.data,
                                        out, cap, C.byref(total), None)

    (records,) = _sized_then_filled(hip, "pag_successors_batch", call, (total,), (np.dtype(capi.PagSucc),))
    return off, status, records


def find_all_batch(hip, g, packed, byte_off, lengths, reverse=None):
    """pag_find_all_batch (include/pagraph_hip.h) for the sequences (byte_off[i], lengths[i]) of the 2-bit packed array `packed`
    (uint8, laid out as pag_seqs says; the 16 bytes of padding are added here) in the finished graph of handle `g` of the bound
    library `hip`; reverse[i] != 0 searches sequence i's reverse strand.  A sizing call, then the real one.  Returns
    (hit_off, hits, vertices): hit_off[n + 1] uint64, hits hit_off[-1] entries of capi.PagFindHit as a numpy record array (offset,
    code, first, n_pos), the hits of sequence i at hits[hit_off[i]:hit_off[i + 1]], vertices of capi.PagFindVertex (pos,
    abundance), those of hit h at vertices[h.first:h.first + h.n_pos]."""
    import numpy as np

    byte_off = np.ascontiguousarray(byte_off, dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    if byte_off.shape != lengths.shape or byte_off.ndim != 1:
        raise ValueError("byte_off and lengths are one-dimensional arrays of the same length")
    n = len(lengths)
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    padded = np.concatenate((packed, np.zeros(16, dtype=np.uint8)))
    rev = None
    if reverse is not None:
        rev = np.ascontiguousarray(np.asarray(reverse) != 0, dtype=np.uint8)
        if rev.shape != lengths.shape:
            raise ValueError("reverse has one entry per sequence")
    seqs = capi.PagSeqs(n, byte_off.ctypes.data, lengths.ctypes.data, padded.ctypes.data, len(packed))
    hit_off = np.zeros(n + 1, dtype=np.uint64)
    n_hits, n_vert = C.c_uint64(), C.c_uint64()
    handle = g if isinstance(g, C.c_void_p) else C.c_void_p(g)

    def call(hits, hit_cap, vert, vert_cap):
        return hip.pag_find_all_batch(handle, C.byref(seqs), None if rev is None else rev.ctypes.data, hit_off.ctypes.data, hits, hit_cap,
                                      vert, vert_cap, C.byref(n_hits), C.byref(n_vert), None)

    hits, vertices = _sized_then_filled(hip, "pag_find_all_batch", call, (n_hits, n_vert), (capi.FIND_HIT_DTYPE, capi.FIND_VERTEX_DTYPE))
    return hit_off, hits, vertices


def walk_straight_batch(hip, g, queries, frames, excl, ctg_len, deviation, error_rate):
    """pag_walk_straight_batch (include/pagraph_hip.h) in the finished graph of handle `g` of the bound library `hip`: queries,
    frames and excl are arrays of capi.WALK_QUERY_DTYPE, capi.WALK_FRAME_DTYPE and capi.SUCC_QUERY_DTYPE (or what numpy converts
    to them), ctg_len the contigs' lengths.  A sizing call, then the real one.  Returns (node_off, nodes, alt_off, alts, status):
    the path of query i at nodes[node_off[i]:node_off[i + 1]] (capi.WALK_NODE_DTYPE: code, step, pos, abundance), the chosen class
    of a walk that ended at a branch at alts[alt_off[i]:alt_off[i + 1]] (capi.SUCC_DTYPE), status[i] one of capi.PAG_WALK_END /
    BRANCH / LIMIT / LEAP, or capi.PAG_EINVAL where the graph holds no such vertex (an empty path)."""
    import numpy as np

    q = np.ascontiguousarray(queries, dtype=capi.WALK_QUERY_DTYPE)
    fr = np.ascontiguousarray(frames, dtype=capi.WALK_FRAME_DTYPE)
    ex = np.ascontiguousarray(excl, dtype=capi.SUCC_QUERY_DTYPE)
    lens = np.ascontiguousarray(ctg_len, dtype=np.uint32)
    if q.ndim != 1 or fr.ndim != 1 or ex.ndim != 1 or lens.ndim != 1:
        raise ValueError("queries, frames, excl and ctg_len are one-dimensional arrays")
    n = len(q)
    node_off, alt_off = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    n_nodes, n_alts = C.c_uint64(), C.c_uint64()
    handle = g if isinstance(g, C.c_void_p) else C.c_void_p(g)

    def call(nodes, node_cap, alts, alt_cap):
        return hip.pag_walk_straight_batch(handle, q.ctypes.data, n, fr.ctypes.data, len(fr), ex.ctypes.data, len(ex), lens.ctypes.data, len(lens),
                                           int(deviation), float(error_rate), node_off.ctypes.data, nodes, node_cap, alt_off.ctypes.data, alts, alt_cap,
                                           status.ctypes.data, C.byref(n_nodes), C.byref(n_alts), None)

    nodes, alts = _sized_then_filled(hip, "pag_walk_straight_batch", call, (n_nodes, n_alts), (capi.WALK_NODE_DTYPE, capi.SUCC_DTYPE))
    return node_off, nodes, alt_off, alts, status


def pagraph_argv(binary, in_dir, out_dir, threads=1, epsilon=10, cov=2, min_len=50):
    """The argv AlignGraph2.py uses for pagraph (reference AlignGraph2.py:414-427), incl. the doubled -r."""
    return [binary, "-t", str(threads), "-r", "dummy", "-k", os.path.join(in_dir, "kmer.bin"),
            "-c", os.path.join(in_dir, "ctg.fasta"), "-R", os.path.join(in_dir, "ref.fasta"),
            "-p", in_dir, "-a", os.path.join(in_dir, "aln"), "-o", out_dir, "-r", str(min_len),
            "--epsilon", str(epsilon), "-v", str(cov)]
