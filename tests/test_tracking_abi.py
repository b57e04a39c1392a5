"""Tracking a reference path (include/altro_tracking.h), the parts that need no GPU: the header and the exports, the binding's
methods, and every refusal that is answered before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("altro_set_lqr_tracking_cost", "altro_set_reference", "altro_set_reference_device", "altro_set_reference_offset",
             "altro_get_reference_offset", "altro_get_reference_terms")
METHODS = ("set_lqr_tracking_cost", "set_reference", "set_reference_device", "set_reference_offset", "get_reference_offset",
           "get_reference_terms")
N = 24


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def _refused(A, call, status, *words):
    with pytest.raises(A.AltroError) as e:
        call()
    assert f"({status})" in str(e.value), str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_header_and_exports(A):
    """include/altro_tracking.h declares the six functions, the library exports them, the binding has the methods; the
    header that the CPU oracle mirrors function by function declares none of them."""
    trk, hip = _declared("altro_tracking.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in FUNCTIONS:
        assert f in trk and f not in hip and hasattr(lib, f), f
    for method in METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    assert "altro_tracking.h" in open(os.path.join(ROOT, "include", "altro_hip.h")).read()
    assert "reference window" in open(os.path.join(ROOT, "include", "altro_mpc.h")).read()


def test_slalom_path_is_the_stated_one(P):
    """problems.slalom_path against the formulas of its docstring, written out once more as plain loops."""
    B, rows = 7, N + 1 + 12
    X, U, h = P.slalom_path(B, N, rows)
    assert h == np.float32(np.float32(3.0) / np.float32(N)) and X.shape == (B, rows, 3) and U.shape == (B, rows, 2)
    hd = float(h)
    for b in (0, 3, 6):
        a, v = 0.3 + 0.05 * (b % 5), 0.6 + 0.05 * (b % 5)
        x = y = 0.0
        for j in range(rows):
            th = a * np.sin(1.2 * j * hd)
            assert np.allclose(X[b, j], [x, y, th], rtol=0, atol=1e-13)
            assert np.allclose(U[b, j], [v, 1.2 * a * np.cos(1.2 * j * hd)], rtol=0, atol=1e-13)
            x += v * np.cos(th) * hd
            y += v * np.sin(th) * hd
    assert np.array_equal(X[5], X[0]) and np.array_equal(U[6], U[1])  # the parameter repeats with b mod 5


def test_refusals_without_a_device(A, P):
    """Bad knot ranges, a path without rows, a negative offset: ALTRO_INVALID_ARG.  A solve or a cost evaluation that meets a
    tracking knot with no reference path: ALTRO_NOT_READY.  All of it before the device is touched, so it holds on a machine
    without one."""
    s = A.BatchSolver(3, 2, N, 5)
    Q, R = np.eye(3), np.eye(2)
    for kb, ke in ((-1, 4), (0, N + 2), (5, 5), (7, 3)):
        _refused(A, lambda: s.set_lqr_tracking_cost(kb, ke, Q, R), A.INVALID_ARG, "knot range out of bounds")
    _refused(A, lambda: s.set_reference(np.zeros((0, 3))), A.INVALID_ARG, "at least one row")
    _refused(A, lambda: s.set_reference_device(0, 0, 5, 0), A.INVALID_ARG, "Xref")
    _refused(A, lambda: s.set_reference_device(4096, 0, 0, 0), A.INVALID_ARG, "at least one row")
    _refused(A, lambda: s.set_reference_offset(-1), A.INVALID_ARG, "negative")
    lib = A.load_library()
    for f in FUNCTIONS:
        getattr(lib, f).restype = int
    x = np.zeros((4, 3))
    xp = x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.altro_set_reference(s._h, xp, None, 0, 0) == A.INVALID_ARG
    assert lib.altro_set_reference(s._h, xp, None, -3, 1) == A.INVALID_ARG
    assert lib.altro_set_reference(s._h, None, None, 4, 0) == A.INVALID_ARG
    assert lib.altro_set_lqr_tracking_cost(s._h, 0, N, None, None) == A.INVALID_ARG
    assert lib.altro_get_reference_offset(s._h, None) == A.INVALID_ARG
    assert lib.altro_set_lqr_tracking_cost(None, 0, N, None, None) == A.INVALID_ARG
    assert lib.altro_set_reference(None, xp, None, 4, 0) == A.INVALID_ARG
    assert lib.altro_set_reference_device(None, None, None, 4, 0) == A.INVALID_ARG
    assert lib.altro_set_reference_offset(None, 0) == A.INVALID_ARG
    assert lib.altro_get_reference_offset(None, None) == A.INVALID_ARG
    # the binding checks shapes before it calls
    with pytest.raises(ValueError):
        s.set_reference(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        s.set_reference(np.zeros((3, 4, 3)))  # per instance, but not 5 instances
    with pytest.raises(ValueError):
        s.set_reference(np.zeros((4, 3)), np.zeros((5, 2)))

    # a tracking knot and no path: every call that evaluates costs refuses, and says which knot
    t = P.tracking_slalom(_make(A), batch=5, N=N)
    u = A.BatchSolver(3, 2, N, 5)
    u.set_model(A.MODEL_UNICYCLE)
    u.set_uniform_step(np.float32(0.125))
    xf = np.array([1.0, 1.0, 0.0])
    u.set_lqr_cost(0, N + 1, Q, R, xf, np.zeros(2))
    u.set_lqr_tracking_cost(N, N + 1, Q, R * 0)  # the last cost set on a knot wins: knot N tracks
    u.set_initial_state(np.zeros(3))
    for call in (u.solve, u.solve_ilqr, u.solve_async, u.al_init, u.cost, u.update_expansions, u.forward_pass,
                 lambda: u.mpc_run(2, 5), lambda: u.mpc_run_tracked(2, 5)):
        _refused(A, call, A.NOT_READY, f"knot {N} has a tracking cost", "altro_set_reference")
    # ... and an ordinary cost set over a tracking cost takes the knot back: nothing tracks, nothing is missing -- the
    # refusal that is left is the machine's (no device here), or none at all
    v = A.BatchSolver(3, 2, N, 5)
    v.set_lqr_tracking_cost(0, N + 1, Q, R)
    v.set_lqr_cost(0, N + 1, Q, R, xf, np.zeros(2))
    try:
        v.cost()
    except A.AltroError as e:
        assert "tracking" not in str(e)
    del t


def test_offset_before_the_device_state(A):
    """The window offset is recorded with the problem: set_reference puts it back to 0, and the getter answers before any
    device exists."""
    s = A.BatchSolver(3, 2, N, 2)
    assert s.get_reference_offset() == 0
    s.set_reference_offset(7)  # (an offset without a path is kept: the path may come later through the device)
    assert s.get_reference_offset() == 7
    s.set_reference(np.zeros((N + 13, 3)), np.zeros((N + 13, 2)))
    assert s.get_reference_offset() == 0
    s.set_reference_offset(12)
    assert s.get_reference_offset() == 12
    s.set_reference(np.zeros((2, N + 13, 3)))
    assert s.get_reference_offset() == 0


def test_ordinary_per_knot_costs_keep_their_limit(A, P):
    """The reference's idiom through altro_set_lqr_cost, one call per knot: recorded without complaint (the setters only
    record), and the limit and its text are the problem compiler's -- tests/test_tracking_layout.py."""
    s = P.tracking_slalom(_make(A), batch=5, N=N, per_knot=True)
    assert s.get_reference_offset() == 0
