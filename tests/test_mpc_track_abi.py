"""Closed-loop tracking (include/altro_mpc.h: altro_mpc_track, altro_mpc_track_device, altro_mpc_run_tracked), the parts that
need no GPU: the header and the exports, the ctypes mirror of altro_track_stats, and every refusal that is answered before
any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import _mpc_common as M  # noqa: F401  (the shared helpers; the GPU file uses them)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK_FUNCTIONS = ("altro_mpc_track", "altro_mpc_track_device", "altro_mpc_run_tracked")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def test_header_and_exports(A):
    """include/altro_mpc.h declares the three functions and the statistics record, the library exports them, and
    include/altro_hip.h declares none of them (every function of that header needs a twin in the oracle)."""
    mpc, hip = _declared("altro_mpc.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in TRACK_FUNCTIONS:
        assert f in mpc and f not in hip and hasattr(lib, f), f
    text = open(os.path.join(ROOT, "include", "altro_mpc.h")).read()
    assert "typedef struct altro_track_stats" in text and "ilqr.hpp:468-499" in text
    assert "altro_track_stats" not in open(os.path.join(ROOT, "include", "altro_hip.h")).read()
    for method in ("mpc_track", "mpc_track_device", "mpc_run_tracked"):
        assert callable(getattr(A.BatchSolver, method))


def test_stats_struct_is_40_bytes(A):
    assert ctypes.sizeof(A.TrackStats) == 40 == A.TRACK_STATS_DTYPE.itemsize
    assert [n for n, _ in A.TrackStats._fields_] == ["status", "steps_done", "cost", "violation", "max_dx", "max_du"]
    assert [getattr(A.TrackStats, n).offset for n, _ in A.TrackStats._fields_] == [0, 4, 8, 16, 24, 32]
    assert [A.TRACK_STATS_DTYPE.fields[n][1] for n, _ in A.TrackStats._fields_] == [0, 4, 8, 16, 24, 32]


def test_refusals_without_a_device(A, P):
    """steps / samples out of range and one-sided bounds are ALTRO_INVALID_ARG; a handle on which no backward pass has run is
    ALTRO_NOT_READY -- all of it before the device is touched, so it holds on a machine without one."""
    N = 20
    s = P.unicycle_turn90(_make(A), batch=2, N=N)
    lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
    for steps, samples in ((0, 1), (-3, 1), (N + 1, 1), (N + 40, 2), (1, 0), (N, -1)):
        for call in (lambda: s.mpc_track(steps, samples), lambda: s.mpc_track(steps, samples, log=False),
                     lambda: s.mpc_track_device(steps, samples)):
            with pytest.raises(A.AltroError) as e:
                call()
            assert f"({A.INVALID_ARG})" in str(e.value) and ("steps" in str(e.value) or "sample" in str(e.value))
    for kw in (dict(u_lo=lo), dict(u_hi=hi)):
        with pytest.raises(A.AltroError) as e:
            s.mpc_track(5, 1, **kw)
        assert f"({A.INVALID_ARG})" in str(e.value) and "u_lo" in str(e.value)
        with pytest.raises(A.AltroError) as e:
            s.mpc_run_tracked(2, 1, **kw)
        assert f"({A.INVALID_ARG})" in str(e.value) and "u_lo" in str(e.value)
    # in range, but no solve and no backward pass has left gains on this handle
    for call in (lambda: s.mpc_track(1), lambda: s.mpc_track(N, 7, u_lo=lo, u_hi=hi), lambda: s.mpc_track_device(N, 3)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value) and "gains" in str(e.value)
    # the loop: cycles and shift as altro_mpc_run checks them
    for cycles, shift in ((0, 1), (2, 0), (2, N), (2, -1)):
        with pytest.raises(A.AltroError) as e:
            s.mpc_run_tracked(cycles, shift)
        assert f"({A.INVALID_ARG})" in str(e.value)
    t = P.unicycle_turn90(_make(A), batch=2, N=N)
    t.set_steps(np.full(N, 0.1, dtype=np.float32))
    with pytest.raises(A.AltroError) as e:  # (the advance inside the loop does not move per-knot steps along the horizon)
        t.mpc_run_tracked(2, 1)
    assert f"({A.UNSUPPORTED})" in str(e.value)
    with pytest.raises(A.AltroError) as e:  # ... while tracking alone accepts them: its refusal is the missing gains
        t.mpc_track(3)
    assert f"({A.NOT_READY})" in str(e.value)
    lib = A.load_library()
    lib.altro_mpc_track.restype = lib.altro_mpc_track_device.restype = lib.altro_mpc_run_tracked.restype = int
    assert lib.altro_mpc_track(None, 1, 1, None, None, None, None, None, None, None) == A.INVALID_ARG
    assert lib.altro_mpc_track_device(None, 1, 1, None, None, None, None, None, None, None) == A.INVALID_ARG
    assert lib.altro_mpc_run_tracked(None, 1, 1, None, None, None, None, None, None, None, None) == A.INVALID_ARG
    # the binding checks shapes before it calls
    with pytest.raises(ValueError):
        s.mpc_track(5, 2, dx0=np.zeros((2, 3, 3)))
    with pytest.raises(ValueError):
        s.mpc_track(5, 2, w=np.zeros((2, 2, 4, 3)))
    with pytest.raises(ValueError):
        s.mpc_track(5, 2, u_lo=np.zeros(3), u_hi=np.zeros(3))
    with pytest.raises(ValueError):
        s.mpc_run_tracked(2, 5, w=np.zeros((2, 2, 3)))
