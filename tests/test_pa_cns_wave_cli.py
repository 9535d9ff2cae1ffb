"""CPU: the lane-parallel device backend of bin/pa_cns (PA_CNS_BACKEND=wave, pag_cns_consensus_wave in csrc/hip/k_cns_wave.hip)
is part of the library's C ABI, and where no gfx950 device is present the executable accepts the backend name and fails with
the reason: there is no host fallback behind it.  The device runs it in tests/test_gpu_pa_cns_wave.py."""
import os
import subprocess

import pytest

import cns_cases
import pagctl

EXE = os.path.join(pagctl.ROOT, "aligngraph2_amd", "bin", "pa_cns")


def _lib():
    if not (os.path.exists(pagctl.HIP_LIB) and os.path.exists(EXE)):
        subprocess.run(["make", "-C", pagctl.ROOT, "product"], check=True, capture_output=True)
    import aligngraph2_amd
    return aligngraph2_amd.load_hip()


def test_library_exports_the_wave_entry_point():
    lib = _lib()
    assert hasattr(lib, "pag_cns_consensus_wave") and hasattr(lib, "pag_cns_consensus")


def test_wave_backend_without_a_device_exits_1_with_the_reason(tmp_path):
    lib = _lib()
    if lib.pag_device_available() != 0:
        pytest.skip("a gfx950 device is present: tests/test_gpu_pa_cns_wave.py runs the backend")
    case = cns_cases.CASES["one_part"]
    d = cns_cases.write_case(case, str(tmp_path / "in"))
    env = dict(os.environ, PA_CNS_BACKEND="wave")
    r = subprocess.run(cns_cases.argv(EXE, d, str(tmp_path / "o.fasta"), case), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 1, r.stderr[-500:]
    assert "pag_cns_consensus_wave" in r.stderr and "no gfx950 device" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(tmp_path / "o.fasta") or os.path.getsize(tmp_path / "o.fasta") == 0
