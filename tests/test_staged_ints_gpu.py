"""The int and byte arrays of a host caller come back to the element: altro_mpc_trigger, altro_lqr_gains, altro_mpc_ensemble and
altro_set_solve_mask called through ctypes with host arrays of ODD lengths (B = 5 ints, 5 bytes, B (steps + 1) = 15 ints), which a
staging block counted in doubles cannot hold without rounding (Staged, altro-cpp_amd/csrc/altro_devmem.hpp).  Every int and byte
output has guard elements behind it holding a sentinel: all of them must be intact, and what lies in front of them must equal, bit
for bit, what the _device entry point leaves in device memory on the same handle.

unicycle kTurn90, B = 5, N = 12, solved once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _trigger_common import AGE
from test_trigger_gpu import DeviceArray, _w_of  # device memory through the HIP runtime; the disturbance of its tracking step

pytestmark = pytest.mark.gpu

B, N, STEPS, SAMPLES, SEED, GUARD = 5, 12, 2, 64, 20240607, 8
LO, HI = np.array([-1.5, -1.5]), np.array([1.5, 1.5])  # problems.unicycle_turn90's control bound
SENTINEL = {np.dtype(np.int32): -1234567, np.dtype(np.uint8): 0xA5}


class Guarded:
    """`count` elements for the callee, GUARD more behind them; all hold the sentinel before the call"""

    def __init__(self, count, dtype):
        self.count, self.mark = count, SENTINEL[np.dtype(dtype)]
        self.all = np.full(count + GUARD, self.mark, dtype=dtype)

    def ptr(self, ctype):
        return self.all.ctypes.data_as(C.POINTER(ctype))

    @property
    def data(self):
        return self.all[:self.count]

    def intact(self):
        return bool((self.all[self.count:] == self.mark).all())


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _void(*arrays):
    return [C.c_void_p(d.ptr if d is not None else None) for d in arrays]


@pytest.fixture(scope="module")
def solved(A, P, hip_make):
    s = P.batch_turn90(hip_make, B, N=N)
    s.solve()
    yield s
    s.close()


@pytest.mark.parametrize("lookahead", [0, 2])
def test_trigger_ints_and_bytes(A, solved, lookahead):
    s = solved
    tracked = np.ascontiguousarray(s.mpc_track(STEPS, 1, w=_w_of(B, STEPS, s.n))["stats"][:, 0])
    assert tracked.shape == (B,) and tracked.dtype == A.TRACK_STATS_DTYPE
    age = np.arange(B, dtype=np.int32) % 3
    rule = A.TriggerRule(max_age=2, dx_tol=float(np.sort(tracked["max_dx"])[B // 2]), viol_tol=1e-4, on_unsolved=1, lookahead=lookahead,
                         ahead_tol=1e-6)
    mask, why = Guarded(B, np.uint8), Guarded(B, np.int32)
    s._call("mpc_trigger", C.byref(rule), tracked.ctypes.data_as(C.POINTER(A.TrackStats)), age.ctypes.data_as(C.POINTER(C.c_int)),
            LO.ctypes.data_as(C.POINTER(C.c_double)), HI.ctypes.data_as(C.POINTER(C.c_double)), mask.ptr(C.c_ubyte), why.ptr(C.c_int))
    assert mask.intact() and why.intact()
    dev = [DeviceArray(a) for a in (tracked, age, LO, HI, np.full(B, 7, dtype=np.uint8), np.full(B, -1, dtype=np.int32))]
    s._call("mpc_trigger_device", C.byref(rule), *_void(*dev))
    assert _bits(mask.data, dev[4].get()) and _bits(why.data, dev[5].get())
    assert set(np.unique(mask.data)) <= {0, 1} and (why.data[age >= 2] & AGE).all()
    for d in dev:
        d.free()


def test_lqr_fail_ints(solved):
    s = solved
    n, m = s.n, s.m
    Q, R = np.diag([10.0, 10.0, 1.0]), np.diag([0.1, 0.2])
    K, Pm, fail = np.zeros((B, N, n, m)), np.zeros((B, N + 1, n, n)), Guarded(B, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    s._call("lqr_gains", dp(Q), dp(R), None, C.c_int(0), dp(K), dp(Pm), fail.ptr(C.c_int))
    assert fail.intact()
    dev = [DeviceArray(a) for a in (Q, R, np.full_like(K, np.nan), np.full_like(Pm, np.nan), np.full(B, 77, dtype=np.int32))]
    s._call("lqr_gains_device", *_void(dev[0], dev[1], None), C.c_int(0), *_void(*dev[2:]))
    assert _bits(K, dev[2].get()) and _bits(Pm, dev[3].get()) and _bits(fail.data, dev[4].get())
    assert (fail.data == -1).all() and np.isfinite(K).all()
    for d in dev:
        d.free()


def test_ensemble_counts(A, solved):
    s = solved
    n, K1 = s.n, STEPS + 1
    Sigma0, W = 1e-4 * np.eye(n), 1e-6 * np.eye(n)
    alive, viol = Guarded(B * K1, np.int32), Guarded(B * K1, np.int32)
    summary = np.zeros(B, dtype=A.ENSEMBLE_STATS_DTYPE)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    head = (C.c_int(STEPS), C.c_int(SAMPLES), C.c_ulonglong(SEED), C.c_ulonglong(0))
    s._call("mpc_ensemble", *head, dp(Sigma0), C.c_int(0), dp(W), C.c_int(0), dp(LO), dp(HI), C.c_double(1e-4), None, None,
            alive.ptr(C.c_int), viol.ptr(C.c_int), summary.ctypes.data_as(C.POINTER(A.EnsembleStats)), None)
    assert alive.intact() and viol.intact()
    dev = [DeviceArray(a) for a in (Sigma0, W, LO, HI, np.full(B * K1, -3, dtype=np.int32), np.full(B * K1, -3, dtype=np.int32),
                                    np.zeros(B, dtype=A.ENSEMBLE_STATS_DTYPE))]
    s._call("mpc_ensemble_device", *head, *_void(dev[0]), C.c_int(0), *_void(dev[1]), C.c_int(0), *_void(dev[2], dev[3]), C.c_double(1e-4),
            *_void(None, None, dev[4], dev[5], dev[6], None))
    assert _bits(alive.data, dev[4].get()) and _bits(viol.data, dev[5].get()) and _bits(summary, dev[6].get())
    assert ((alive.data >= 0) & (alive.data <= SAMPLES)).all() and (viol.data <= alive.data).all() and (summary["samples"] == SAMPLES).all()
    for d in dev:
        d.free()


def test_solve_mask_bytes(solved):
    s = solved
    want = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    try:
        s._call("set_solve_mask", want.ctypes.data_as(C.c_void_p))
        got, count = Guarded(B, np.uint8), C.c_int(-1)
        s._call("get_solve_mask", got.ptr(C.c_ubyte), C.byref(count))
        assert got.intact() and _bits(got.data, want) and count.value == 3
        # the device entry point on the same handle leaves the same mask
        d = DeviceArray(want)
        s._call("set_solve_mask_device", C.c_void_p(d.ptr))
        again, count = Guarded(B, np.uint8), C.c_int(-1)
        s._call("get_solve_mask", again.ptr(C.c_ubyte), C.byref(count))
        assert again.intact() and _bits(again.data, got.data) and count.value == 3
        d.free()
    finally:
        s._call("set_solve_mask", C.c_void_p(None))
