"""CPU: the line format of the per-contig path dumps and PositionMapper restated in Python (tests/dump_text.py) against every
body line of every golden dump, and the C ABI of the device renderer (pag_render_dump_lines, pag_travel_dump_text)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dump_text
import pagctl
from aligngraph2_amd import capi


def test_restatement_reproduces_every_line_of_every_golden_dump(workdir):
    """Every body line of every golden *.txt is parsed back into its record (k-mer -> code, the four numbers) and rendered
    again: the result must be the golden line.  That pins the restatement to the reference's outputs; the GPU tests then use it
    as the oracle for records no golden has (no golden has a step <= 0, a count above a few hundred, a coordinate of ten
    digits ...)."""
    cases = dump_text.dump_cases()
    assert len(cases) == 10
    n_lines = n_rev = n_noctg = longest = 0
    min_step = None
    for name in cases:
        ctg_len, ref_len = dump_text.case_lengths(name, workdir)
        cm, rm = dump_text.Mapper(ctg_len), dump_text.Mapper(ref_len)
        for f, (header, body) in dump_text.golden_dumps(name).items():
            assert header.count("\t") == 1
            for ln in body:
                k, rec = dump_text.parse_line(ln)
                assert dump_text.render_line(rec, k, cm, rm) == ln, f"{name}/{f}: {ln!r}"
                n_lines += 1
                ci, _ = cm.single_to_dual(rec[1])
                ri, _ = rm.single_to_dual(rec[2])
                n_rev += ci < 0 or ri < 0
                n_noctg += rec[1] == 0
                longest = max(longest, len(ln))
                min_step = rec[4] if min_step is None else min(min_step, rec[4])
    assert n_lines == 29473
    assert n_rev == 8162
    assert n_noctg == 1392
    assert longest == 46
    assert min_step > 0


def test_mapper_restatement_at_its_corners():
    m = dump_text.Mapper([100, 50])
    assert m.starts == [100, 100 + 300 + 100, 500 + 200]
    assert m.single_to_dual(0) == (0, 0)
    assert m.single_to_dual(100) == (1, 0) and m.single_to_dual(199) == (1, 99)
    assert m.single_to_dual(300) == (-1, 0) and m.single_to_dual(399) == (-1, 99)
    assert m.single_to_dual(500) == (2, 0) and m.single_to_dual(649) == (-2, 49)
    assert m.single_to_dual(5) == (-1, 5 - 100 - 200)  # before the first start: the unsigned difference wraps
    assert m.single_to_dual(700) == (-3, 0)            # at the end of the space


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pagctl.HIP_LIB):
        subprocess.run(["make", "-C", pagctl.ROOT, "product"], check=True, capture_output=True)
    return capi.bind(C.CDLL(pagctl.HIP_LIB))


def test_library_exports_the_renderer_and_load_hip_declares_it(lib):
    for f in ("pag_render_dump_lines", "pag_travel_dump_text"):
        assert hasattr(lib, f), f"libpagraph_hip.so does not export {f}"
    host = C.CDLL(os.path.join(pagctl.ROOT, "aligngraph2_amd", "libpagraph_host.so"))
    assert hasattr(host, "pagh_assemble_paths_text")
    import aligngraph2_amd
    hip = aligngraph2_amd.load_hip()
    assert hip.pag_render_dump_lines.argtypes is not None and len(hip.pag_render_dump_lines.argtypes) == 11
    assert hip.pag_render_dump_lines.restype is C.c_int
    assert hip.pag_travel_dump_text.argtypes is not None and len(hip.pag_travel_dump_text.argtypes) == 4
    assert hip.pag_travel_dump_text.restype is C.c_void_p


def test_renderer_has_no_cpu_fallback(lib):
    """Without a gfx950 device the call fails with PAG_ENODEV (bad arguments are refused before the device is looked for);
    with one it renders."""
    recs = dump_text.to_records([(0b0110, 101, 0, 7, 2)])
    ctg_len, ref_len = [100], [100]
    need = C.c_uint64(7)
    cl, rl = np.array(ctg_len, dtype=np.uint32), np.array(ref_len, dtype=np.uint32)
    assert lib.pag_render_dump_lines(recs.ctypes.data, 1, 17, cl.ctypes.data, 1, rl.ctypes.data, 1, None, 0, C.byref(need), 0) == dump_text.PAG_EINVAL
    assert need.value == 0
    assert lib.pag_render_dump_lines(recs.ctypes.data, 1, 2, cl.ctypes.data, 1, rl.ctypes.data, 1, None, 0, None, 0) == dump_text.PAG_EINVAL
    big = np.array([0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)  # a coordinate space beyond 32 bits
    assert lib.pag_render_dump_lines(recs.ctypes.data, 1, 2, big.ctypes.data, 2, rl.ctypes.data, 1, None, 0, C.byref(need), 0) == dump_text.PAG_EINVAL
    rc, n, text, guard_ok = dump_text.device_render(lib, recs, 2, ctg_len, ref_len, cap=64)
    if lib.pag_device_available():
        assert rc == dump_text.PAG_OK and guard_ok
        assert text[:n] == b"CG,101,0,7\t2\t1,1\t0,0\n"
    else:
        assert rc == dump_text.PAG_ENODEV and n == 0 and guard_ok
