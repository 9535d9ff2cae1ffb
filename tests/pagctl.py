"""ctypes bindings used by the tests / bench / smoke: the HIP library (product), the C oracle (checker)
and the test-support loader that builds the flat pag_build_input from a pagraph input directory.

Nothing here is product code.  The oracle is only ever used as the checker.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_LIB = os.path.join(ROOT, "aligngraph2_amd", "libpagraph_hip.so")
ORACLE_LIB = os.path.join(ROOT, "oracle", "libpag_oracle.so")
TEST_LIB = os.path.join(ROOT, "tests", "harness", "bin", "libpagh_test.so")
WALK_TEST_LIB = os.path.join(ROOT, "tests", "harness", "bin", "libpagh_walk_test.so")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")


import sys  # noqa: E402

sys.path.insert(0, ROOT)
from aligngraph2_amd import capi  # noqa: E402  (importable without torch)
from aligngraph2_amd.capi import BuildStats, Csr  # noqa: E402,F401  (pag_build_stats, pag_csr: include/pagraph_hip.h)


def ensure_built(targets=("harness", "oracle")):
    """(Re)build test-side binaries if missing.  The product library is built by __graft_entry__.build()."""
    need = [t for t, f in (("harness", TEST_LIB), ("oracle", ORACLE_LIB)) if t in targets and not os.path.exists(f)]
    for t in need:
        subprocess.run(["make", "-C", ROOT, t], check=True, capture_output=True)


# the entry points the C oracle restates under its own prefix (oracle/pag_oracle.h): same parameters, same results
_ORACLE_TWINS = ("process", "csr_sizes", "export_csr", "debug_stream_sizes", "debug_streams", "reset", "destroy", "solid_count")


def _bind_twins(lib, prefix):
    """The prefix_* twins of `lib` get the types of their pag_* originals from capi.SIGNATURES, so the two cannot part."""
    twins = {"pag_" + t: prefix + "_" + t for t in _ORACLE_TWINS}
    return capi.bind(lib, rename=twins.get)


_libs = {}


def hip_lib():
    if "hip" not in _libs:
        import aligngraph2_amd
        _libs["hip"] = aligngraph2_amd.load_hip()  # (raises if the library is missing: no CPU fallback exists; typed by capi)
    return _libs["hip"]


def oracle_lib():
    if "oracle" not in _libs:
        ensure_built(("oracle",))
        lib = C.CDLL(ORACLE_LIB)
        _bind_twins(lib, "pago")
        lib.pago_create.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
        lib.pago_create.restype = C.c_void_p
        lib.pago_debug_enable.argtypes = [C.c_void_p, C.c_int]
        lib.pago_check_position.argtypes = [C.c_uint32] * 6 + [C.c_double]
        lib.pago_edge_similar.argtypes = [C.c_uint32] * 4 + [C.c_int, C.c_uint64, C.c_double]
        lib.pago_cluster_similar.argtypes = [C.c_uint32] * 4 + [C.c_uint64]
        lib.pago_kmer_codes.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p]
        lib.pago_kmer_codes.restype = C.c_uint64
        lib.pago_debug_max_tile_samples.argtypes = [C.c_void_p]
        lib.pago_debug_max_tile_samples.restype = C.c_uint64
        _libs["oracle"] = lib
    return _libs["oracle"]


def test_lib():
    if "test" not in _libs:
        ensure_built(("harness",))
        lib = C.CDLL(TEST_LIB)
        lib.pagh_load.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_uint64, C.c_uint64]
        lib.pagh_load.restype = C.c_void_p
        lib.pagh_view.argtypes = [C.c_void_p]
        lib.pagh_view.restype = C.c_void_p
        lib.pagh_raw_view.argtypes = [C.c_void_p]
        lib.pagh_raw_view.restype = C.c_void_p
        lib.pagh_kmer_words.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.pagh_kmer_words.restype = C.c_void_p
        lib.pagh_total_read_bases.argtypes = [C.c_void_p]
        lib.pagh_total_read_bases.restype = C.c_uint64
        lib.pagh_free.argtypes = [C.c_void_p]
        lib.pagh_free.restype = None
        _libs["test"] = lib
    return _libs["test"]


def walk_test_lib():
    """pagt_traverse_hostwalk: device graph exported, walk by the host restatement of the reference's PAlgorithm (test
    infrastructure, tests/harness/host_walk.cpp); same argument list as pagh_traverse."""
    if "walk" not in _libs:
        hip_lib()  # (the HIP runtime has to come from torch, see hip_lib)
        if not os.path.exists(WALK_TEST_LIB):
            subprocess.run(["make", "-C", ROOT, WALK_TEST_LIB[len(ROOT) + 1:]], check=True, capture_output=True)
        _libs["walk"] = C.CDLL(WALK_TEST_LIB)
    return _libs["walk"]


class LoadedInput:
    """A pagraph input directory parsed by the product's host pipeline into the flat C-ABI input."""

    def __init__(self, in_dir: str, threads: int = 1, eps: int = 10, cov: int = 2, block: int = 0, outer_sample=None):
        self.lib = test_lib()
        self.h = self.lib.pagh_load(in_dir.encode(), block, threads, eps, cov)
        if not self.h:
            raise RuntimeError(f"pagh_load failed for {in_dir}")
        self.view = self.lib.pagh_view(self.h)          # the HOST restatement of the preparation stage (checker)
        self.raw_view = self.lib.pagh_raw_view(self.h)  # what the product hands to pag_prepare
        n, k = C.c_uint64(), C.c_uint64()
        self.kmer_words = self.lib.pagh_kmer_words(self.h, C.byref(n), C.byref(k))
        self.n_kmer_words, self.k = n.value, k.value
        self.n_bases = self.lib.pagh_total_read_bases(self.h)
        if outer_sample is not None:
            self.set_outer_sample(outer_sample)

    def set_outer_sample(self, outer: int):
        """pagraph's outerSample (3, pagraph.cpp:113) replaced in both views: the host-prepared one (the oracle's, and
        run_hip(prepare=False)) and the raw one pag_prepare turns into the device-resident input."""
        from aligngraph2_amd.workload import PagBuildInput, PagRawInput
        C.cast(self.view, C.POINTER(PagBuildInput)).contents.outer_sample = outer
        C.cast(self.raw_view, C.POINTER(PagRawInput)).contents.outer_sample = outer

    def set_topk(self, topk_ctg: int, topk_ref: int):
        """pagraph's readToCtgTopK / readToRefTopK (-1 = all, pagraph.cpp:110-112) replaced in both views"""
        from aligngraph2_amd.workload import PagBuildInput, PagRawInput
        for view, typ in ((self.view, PagBuildInput), (self.raw_view, PagRawInput)):
            v = C.cast(view, C.POINTER(typ)).contents
            v.topk_ctg, v.topk_ref = topk_ctg, topk_ref

    def set_cov(self, cov: int):
        """the coverage filter (-v) replaced in both views; the prepared arrays do not depend on it"""
        from aligngraph2_amd.workload import PagBuildInput, PagRawInput
        C.cast(self.view, C.POINTER(PagBuildInput)).contents.cov_filter = cov
        C.cast(self.raw_view, C.POINTER(PagRawInput)).contents.cov_filter = cov

    def close(self):
        if self.h:
            self.lib.pagh_free(self.h)
            self.h = None


def _prepared_view(lib, g, inp: LoadedInput):
    """pag_prepare: the product's device-side preparation of the block -> a device-resident pag_build_input"""
    import biggen
    out = biggen.PagBuildInput()
    rc = lib.pag_prepare(g, inp.raw_view, C.byref(out))
    if rc != 0:
        raise RuntimeError(f"pag_prepare failed rc={rc} {lib.pag_last_error().decode()}")
    return out


def _hip_runtime():
    import torch
    return C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))


def free_device_bytes():
    """free device memory as hipMemGetInfo reports it (torch's HIP runtime; no torch allocation is made)"""
    rt = _hip_runtime()
    rt.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(), C.c_size_t()
    rc = rt.hipMemGetInfo(C.byref(free), C.byref(total))
    if rc != 0:
        raise RuntimeError(f"hipMemGetInfo failed ({rc})")
    return free.value


def device_bytes(ptr, n):
    """n bytes of device memory as a numpy array (through torch's HIP runtime)"""
    rt = _hip_runtime()
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    buf = np.empty(n, dtype=np.uint8)
    if n:
        rc = rt.hipMemcpy(buf.ctypes.data, ptr, n, 2)
        if rc != 0:
            raise RuntimeError(f"hipMemcpy failed ({rc})")
    return buf


def _run(lib, prefix, g, inp: LoadedInput, streams: bool, prepared=None):
    st = BuildStats()
    rc = getattr(lib, prefix + "_process")(g, C.byref(prepared) if prepared is not None else inp.view, C.byref(st))
    if rc != 0:
        msg = lib.pag_last_error().decode() if prefix == "pag" else ""
        raise RuntimeError(f"{prefix}_process failed rc={rc} {msg}")
    nn, np_, ne = C.c_uint64(), C.c_uint64(), C.c_uint64()
    getattr(lib, prefix + "_csr_sizes")(g, C.byref(nn), C.byref(np_), C.byref(ne))
    out = {
        "node_code": np.zeros(nn.value, np.uint32), "pos_off": np.zeros(nn.value + 1, np.uint64),
        "pos_ctg": np.zeros(np_.value, np.uint32), "pos_ref": np.zeros(np_.value, np.uint32),
        "pos_cnt": np.zeros(np_.value, np.uint16), "edge_off": np.zeros(nn.value + 1, np.uint64),
        "edge_to": np.zeros(ne.value, np.uint32), "edge_step": np.zeros(ne.value, np.int32),
    }
    csr = Csr(nn.value, np_.value, ne.value, *[out[k].ctypes.data for k in
                                                ("node_code", "pos_off", "pos_ctg", "pos_ref", "pos_cnt", "edge_off",
                                                 "edge_to", "edge_step")])
    rc = getattr(lib, prefix + "_export_csr")(g, C.byref(csr))
    if rc != 0:
        msg = lib.pag_last_error().decode() if prefix == "pag" else ""
        raise RuntimeError(f"{prefix}_export_csr failed rc={rc} {msg}")
    res = {"stats": st, "csr": out}
    if streams:
        nt, ne2 = C.c_uint64(), C.c_uint64()
        getattr(lib, prefix + "_debug_stream_sizes")(g, C.byref(nt), C.byref(ne2))
        s = {"tkey": np.zeros(nt.value, np.uint32), "tval": np.zeros(nt.value, np.uint64),
             "ekey": np.zeros(ne2.value, np.uint32), "eval": np.zeros(ne2.value, np.uint64)}
        getattr(lib, prefix + "_debug_streams")(g, *[s[k].ctypes.data for k in ("tkey", "tval", "ekey", "eval")])
        res["streams"] = s
    return res


def run_oracle(inp: LoadedInput, streams: bool = False, solid_codes=None):
    """solid_codes: a u64 array that replaces the input's solid-set file words (default: inp.kmer_words).  With streams,
    res["max_tile_samples"] = the most samples kept in one 1024-position tile of a read strand (K1's tile)."""
    lib = oracle_lib()
    if solid_codes is None:
        g = lib.pago_create(inp.kmer_words, inp.n_kmer_words, inp.k)
    else:
        solid_codes = np.ascontiguousarray(solid_codes, dtype=np.uint64)
        g = lib.pago_create(solid_codes.ctypes.data, len(solid_codes), inp.k)
    try:
        lib.pago_debug_enable(g, 1 if streams else 0)
        res = _run(lib, "pago", g, inp, streams)
        res["n_solid"] = lib.pago_solid_count(g)
        if streams:
            res["max_tile_samples"] = lib.pago_debug_max_tile_samples(g)
        return res
    finally:
        lib.pago_destroy(g)


def hip_create(inp: LoadedInput, device: int = 0, solid_codes=None, solid_bitmap=None):
    """pag_create from the input's solid-set file words, or from `solid_codes` (u64 array) instead, or
    pag_create_from_bitmap from `solid_bitmap` (u32 array, 4^k bits, host memory; its set bits are counted here)."""
    lib = hip_lib()
    err = C.c_int()
    if solid_bitmap is not None:
        bits = np.ascontiguousarray(solid_bitmap, dtype=np.uint32)
        n_solid = int(np.unpackbits(bits.view(np.uint8)).sum())
        g = lib.pag_create_from_bitmap(bits.ctypes.data, n_solid, inp.k, 0, device, C.byref(err))
    elif solid_codes is not None:
        codes = np.ascontiguousarray(solid_codes, dtype=np.uint64)
        g = lib.pag_create(codes.ctypes.data, len(codes), inp.k, device, C.byref(err))
    else:
        g = lib.pag_create(inp.kmer_words, inp.n_kmer_words, inp.k, device, C.byref(err))
    if not g:
        raise RuntimeError(f"pag_create failed rc={err.value}: {lib.pag_last_error().decode()}")
    return g


def keep_streams(on: bool):
    """PAG_DEBUG_KEEP_STREAMS: pag_process keeps copies of the emitted streams for pag_debug_streams"""
    if on:
        os.environ["PAG_DEBUG_KEEP_STREAMS"] = "1"
    else:
        os.environ.pop("PAG_DEBUG_KEEP_STREAMS", None)


def run_hip(inp: LoadedInput, streams: bool = False, device: int = 0, prepare: bool = True, solid_codes=None, solid_bitmap=None):
    """The product path: pag_prepare (device) -> pag_process.  prepare=False feeds pag_process the host restatement's
    arrays instead (the path the C ABI also accepts: host-resident pag_build_input).  solid_codes / solid_bitmap: see
    hip_create.  res["n_solid"] = pag_solid_count of the handle."""
    lib = hip_lib()
    keep_streams(streams)
    g = hip_create(inp, device, solid_codes, solid_bitmap)
    try:
        res = run_on(g, inp, streams, prepare)
        res["n_solid"] = lib.pag_solid_count(g)
        return res
    finally:
        lib.pag_destroy(g)


def run_on(g, inp: LoadedInput, streams: bool = False, prepare: bool = True):
    """run_hip's pag_prepare -> pag_process and export on a handle the caller made (hip_create) and keeps"""
    lib = hip_lib()
    keep_streams(streams)
    return _run(lib, "pag", g, inp, streams, _prepared_view(lib, g, inp) if prepare else None)


def first_diff(a: np.ndarray, b: np.ndarray):
    n = min(len(a), len(b))
    d = np.flatnonzero(a[:n] != b[:n])
    if len(d):
        return int(d[0])
    return None if len(a) == len(b) else n


def compare_results(hip, ora, label=""):
    """Raise AssertionError with a precise message at the first differing stage."""
    msgs = []
    if "streams" in hip and "streams" in ora:
        for k in ("tkey", "tval", "ekey", "eval"):
            a, b = hip["streams"][k], ora["streams"][k]
            i = first_diff(a, b)
            if i is not None:
                lo = max(0, i - 2)
                msgs.append(f"{label} stream {k}: len hip={len(a)} oracle={len(b)} first diff at {i}: "
                            f"hip={a[lo:i + 3].tolist()} oracle={b[lo:i + 3].tolist()}")
    hs, os_ = hip["stats"], ora["stats"]
    if hs.counts() != os_.counts():
        msgs.append(f"{label} count lines differ: hip={hs.counts()} oracle={os_.counts()}")
    for k in ("n_tuples", "n_edges"):
        if tuple(getattr(hs, k)) != tuple(getattr(os_, k)):
            msgs.append(f"{label} {k}: hip={tuple(getattr(hs, k))} oracle={tuple(getattr(os_, k))}")
    for k, a in hip["csr"].items():
        b = ora["csr"][k]
        i = first_diff(a, b)
        if i is not None:
            lo = max(0, i - 2)
            msgs.append(f"{label} csr {k}: len hip={len(a)} oracle={len(b)} first diff at {i}: "
                        f"hip={a[lo:i + 3].tolist()} oracle={b[lo:i + 3].tolist()}")
    if msgs:
        raise AssertionError("\n".join(msgs))


def run_reference(in_dir: str, out_dir: str, threads: int = 1, eps: int = 10, cov: int = 2, tool: str = "pagraph"):
    """Run the compiled reference (oracle/_ref) on an input directory; serialised threads for -t > 1."""
    import synth
    env = dict(os.environ)
    if threads > 1:
        env["LD_PRELOAD"] = os.path.join(REF_DIR, "libserial_threads.so")
    os.makedirs(out_dir, exist_ok=True)
    argv = synth.pagraph_argv(os.path.join(REF_DIR, tool), in_dir, out_dir, threads=threads, epsilon=eps, cov=cov)
    return subprocess.run(argv, env=env, capture_output=True, text=True)
