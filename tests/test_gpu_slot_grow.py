"""GPU: the one grow rule of the handle's pool slots (slot_grow / slot_free / drain_deferred, csrc/hip/pag_graph_impl.hpp) through
its hook pag_debug_slot_grow, on a scratch slot of a scratch handle (pag_create, k = 4).  The small graphs of the suite seldom
make a slot grow with contents to keep (the send slots of shard_comm.hip, the regions of shard_serial.hip); here every branch of
the rule is taken once: from nothing, with kept bytes, no growth, keeping nothing, with the old array parked, and a refusal.

One hook call of ten steps, shared by the tests; a few allocations of at most 50 KB: milliseconds.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import pagctl

GROW, GROW_DEFERRED, DRAIN, FILL, FREE = range(5)
EINVAL = -22
STRIDE = 1024

# (need, want, keep, op)
STEPS = [
    (1000, 1256, 0, GROW),             # 0 (a) from nothing
    (3, 0, 0, FILL),                   # 1     ramp, seed 3
    (5000, 7756, 600, GROW),           # 2 (a) grown, 600 bytes kept
    (4000, 4256, 0, GROW),             # 3 (b) it holds that already
    (20000, 20256, 0, GROW),           # 4 (c) grown, nothing kept
    (11, 0, 0, FILL),                  # 5     ramp, seed 11
    (50000, 50256, 300, GROW_DEFERRED),  # 6 (d) grown while frees are deferred
    (0, 0, 0, DRAIN),                  # 7 (d) the parked array released
    (10 ** 6, 10 ** 6 + 256, 50257, GROW),  # 8 (e) more to keep than the slot holds
    (0, 0, 0, FREE),                   # 9
]


def ramp(n, seed):
    return ((np.arange(n, dtype=np.uint64) * 7 + seed) & 0xFF).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def run_steps():
    hip = pagctl.hip_lib()
    hook = hip.pag_debug_slot_grow  # (the first test fails here where the library has no such hook)
    codes = np.array([1, 2, 3], dtype=np.uint64)
    err = C.c_int()
    h = C.c_void_p(hip.pag_create(codes.ctypes.data, len(codes), 4, 0, C.byref(err)))
    assert h, hip.pag_last_error()
    try:
        steps = np.array(STEPS, dtype=np.uint64)
        out = np.zeros((len(STEPS), 5), dtype=np.uint64)
        kept = np.zeros((len(STEPS), STRIDE), dtype=np.uint8)
        rc = hook(h, steps.ctypes.data, len(STEPS), out.ctypes.data, kept.ctypes.data, STRIDE)
        assert rc == 0, hip.pag_last_error()
    finally:
        hip.pag_destroy(h)
    return {"rc": out[:, 0].astype(np.int64), "ptr": out[:, 1], "cap": out[:, 2], "parked": out[:, 3], "old_same": out[:, 4], "kept": kept}


@pytest.mark.gpu
def test_grows_from_nothing_and_keeps_the_first_bytes():
    rows = run_steps()
    assert rows["rc"][0] == 0 and rows["ptr"][0] != 0 and rows["cap"][0] == 1256
    assert rows["rc"][2] == 0 and rows["cap"][2] == 7756 and rows["cap"][2] >= 5000
    assert rows["ptr"][2] != rows["ptr"][0] and rows["ptr"][2] != 0
    assert np.array_equal(rows["kept"][2][:600], ramp(600, 3))
    assert rows["parked"][2] == 0  # (frees were not deferred: the old array is gone)


@pytest.mark.gpu
def test_a_slot_that_holds_the_bytes_is_left_alone():
    rows = run_steps()
    assert rows["rc"][3] == 0
    assert rows["ptr"][3] == rows["ptr"][2] and rows["cap"][3] == rows["cap"][2]


@pytest.mark.gpu
def test_grows_keeping_nothing():
    rows = run_steps()
    assert rows["rc"][4] == 0 and rows["cap"][4] == 20256 and rows["ptr"][4] != 0 and rows["parked"][4] == 0


@pytest.mark.gpu
def test_deferred_growth_parks_the_old_array_until_the_drain():
    rows = run_steps()
    assert rows["rc"][6] == 0 and rows["cap"][6] == 50256 and rows["ptr"][6] != rows["ptr"][4]
    assert rows["parked"][5] == 0 and rows["parked"][6] == 1
    assert np.array_equal(rows["kept"][6][:300], ramp(300, 11))
    assert rows["old_same"][6] == 1  # the parked array was read after the growth: the ramp is still there
    assert rows["rc"][7] == 0 and rows["parked"][7] == 0
    assert rows["ptr"][7] == rows["ptr"][6] and rows["cap"][7] == rows["cap"][6]


@pytest.mark.gpu
def test_keeping_more_than_the_slot_holds_is_refused():
    rows = run_steps()
    assert rows["rc"][8] == EINVAL
    assert rows["ptr"][8] == rows["ptr"][7] and rows["cap"][8] == rows["cap"][7] and rows["parked"][8] == 0
    assert rows["rc"][9] == 0 and rows["ptr"][9] == 0 and rows["cap"][9] == 0
