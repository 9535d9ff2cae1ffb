"""GPU: ONE handle reused across blocks of different sizes (small, large, small, then the small block again as a
host-resident input) builds what a fresh handle builds for each of them, bit-exact: count lines, every CSR array, the kept
streams (pagctl.compare_results) — and its device pool keeps the documented contract "reused and only ever grown": the
third block, no larger than what the pool already holds, allocates nothing (free device memory as hipMemGetInfo reports it
is the same after the third run as after the second).

The blocks are the two CASES of test_gpu_extract_params.py (same k): "dense" (40 reads) is the small one, "sparse" (160
reads) the large one.  The handle's solid set is complete, so that it serves both inputs.  The host-resident run goes
through the extraction's staging buffers, which the device-prepared runs before it leave idle.
"""
import numpy as np
import pytest

import pagctl
import synth
from test_gpu_extract_params import CASES, K


@pytest.mark.gpu
def test_one_handle_small_large_small_equals_fresh_handles(workdir):
    bits = np.full(4 ** K // 32, 0xFFFFFFFF, np.uint32)
    inputs = {}
    try:
        for name, (kw, threads) in CASES.items():
            d = str(workdir / ("handle_reuse_" + name))
            synth.generate(synth.Spec(**kw), d)
            inputs[name] = pagctl.LoadedInput(d, threads=threads)
        small = inputs["dense"]
        fresh = {name: pagctl.run_hip(inp, streams=True, solid_bitmap=bits) for name, inp in inputs.items()}
        fresh_host = pagctl.run_hip(small, streams=True, prepare=False, solid_bitmap=bits)
        assert fresh["dense"]["stats"].n_pos > 0 and fresh["sparse"]["stats"].n_pos > fresh["dense"]["stats"].n_pos

        g = pagctl.hip_create(small, solid_bitmap=bits)
        try:
            free = []
            for step, name in enumerate(("dense", "sparse", "dense")):
                res = pagctl.run_on(g, inputs[name], streams=True)
                free.append(pagctl.free_device_bytes())
                pagctl.compare_results(res, fresh[name], label=f"reused handle, run {step + 1} ({name})")
            res = pagctl.run_on(g, small, streams=True, prepare=False)
            free.append(pagctl.free_device_bytes())
            pagctl.compare_results(res, fresh_host, label="reused handle, run 4 (dense, host-resident input)")
            print("free device bytes after runs 1..4:", free)
            assert free[2] == free[1], free
        finally:
            pagctl.hip_lib().pag_destroy(g)
    finally:
        for inp in inputs.values():
            inp.close()
