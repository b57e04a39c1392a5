"""Knot constraints (include/altro_knot_params.h), the parts that need no GPU: the header and the exports, the binding's
methods, every refusal that is answered before any device work, the row map of an advance, and the two problems."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mpc_common as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("altro_add_knot_constraint", "altro_set_constraint_track", "altro_set_constraint_track_device", "altro_set_track_offset",
             "altro_get_track_offset", "altro_get_knot_params")
METHODS = ("add_knot_constraint", "set_constraint_track", "set_constraint_track_device", "set_track_offset", "get_track_offset",
           "get_knot_params", "add_knot_circle_constraint", "add_knot_control_bound")
N = 24
MOVING_CONS = [(1, N, 2, False), (0, N, 4, False)]  # problems.moving_obstacles: (k_begin, k_end, rows, equality)


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
    """include/altro_knot_params.h declares the six functions, the library exports them, the binding has the methods; the
    header that the CPU oracle mirrors function by function declares none of them; altro_mpc.h speaks of the track window."""
    knot, hip = _declared("altro_knot_params.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in FUNCTIONS:
        assert f in knot and f not in hip and hasattr(lib, f), f
    for method in METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    assert "track offset" in open(os.path.join(ROOT, "include", "altro_mpc.h")).read()


def test_tracks_are_the_stated_ones(P):
    """problems.moving_obstacle_tracks and ramped_bound_track against the formulas of the issue, written as plain loops."""
    B, rows = 7, N + 13
    Xref, _, _ = P.slalom_path(B, N, rows)
    circles, bounds = P.moving_obstacle_tracks(B, N, rows)
    assert circles.shape == (B, rows, 6) and bounds.shape == (B, rows, 4)
    for b in (0, 3, 6):
        p = b % 5
        for j in (0, 1, 10, rows - 1):
            want = [Xref[b, 10, 0] + 0.02 * p, Xref[b, 10, 1] + 0.45 - 0.045 * j, 0.10 + 0.01 * p,
                    Xref[b, j, 0] + 0.05, Xref[b, j, 1] - 0.30 + 0.004 * j, 0.15]
            assert np.allclose(circles[b, j], want, rtol=0, atol=1e-15)
            ub = 0.9 - 0.008 * j + 0.01 * p
            assert np.allclose(bounds[b, j], [-ub, -ub, ub, ub], rtol=0, atol=1e-15)
    t = P.ramped_bound_track(B, 16)
    assert t.shape == (B, 16, 4)
    for b in (0, 4, 6):
        for j in (0, 7, 15):
            ub = (0.5 + 0.05 * j + 0.02 * (b % 5)) * 256
            assert np.allclose(t[b, j], [-ub, -ub, ub, ub], rtol=0, atol=1e-12)


def test_refusals_without_a_device(A, P):
    """A bad range or index, rows < 1, a negative offset, an nparams that does not fit the kind, a bound's track with a
    non-finite entry, a track on an ordinary constraint: ALTRO_INVALID_ARG.  A solve, a cost evaluation or an MPC loop that
    meets a knot constraint with no track: ALTRO_NOT_READY.  All of it before the device is touched."""
    s = A.BatchSolver(3, 2, N, 5)
    for kb, ke in ((-1, 4), (0, N + 2), (5, 5), (7, 3)):
        _refused(A, lambda: s.add_knot_constraint(A.CON_CIRCLE, kb, ke, 3), A.INVALID_ARG, "knot range out of bounds")
    for kind, nparams in ((A.CON_GOAL, 2), (A.CON_GOAL, 4), (A.CON_CONTROL_BOUND, 2), (A.CON_CONTROL_BOUND, 5), (A.CON_CIRCLE, 0),
                          (A.CON_CIRCLE, 4), (A.CON_CIRCLE, -3), (A.CON_USER, 0)):
        _refused(A, lambda: s.add_knot_constraint(kind, 0, N, nparams), A.INVALID_ARG, "nparams does not fit the kind")
    _refused(A, lambda: s.add_knot_constraint(17, 0, N, 3), A.INVALID_ARG, "unknown constraint kind")
    _refused(A, lambda: s.add_knot_constraint(A.CON_USER, 0, N, 2, user_type=-1), A.INVALID_ARG, "nparams does not fit")
    s.add_control_bound(0, N, [-1.0, -1.0], [1.0, 1.0])  # registration 0: an ordinary constraint
    circle = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 6)
    bound = s.add_knot_control_bound(0, N)
    goal = s.add_knot_constraint(A.CON_GOAL, N, N + 1, 3)
    assert (circle, bound, goal) == (1, 2, 3)  # ONE constraint each, in registration order
    _refused(A, lambda: s.set_constraint_track(0, np.zeros((4, 4))), A.INVALID_ARG, "is not a knot constraint")
    lib = A.load_library()
    for f in FUNCTIONS:
        getattr(lib, f).restype = int
    x = np.zeros((4, 6))
    xp = x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for index in (-1, 4, 99):
        assert lib.altro_set_constraint_track(s._h, index, xp, 4, 0) == A.INVALID_ARG
        assert "is not a knot constraint" in s._errmsg(s._h)
        assert lib.altro_set_constraint_track_device(s._h, index, ctypes.c_void_p(4096), 4, 0) == A.INVALID_ARG
        assert lib.altro_get_knot_params(s._h, index, xp) == A.INVALID_ARG
    assert lib.altro_set_constraint_track(s._h, circle, xp, 0, 0) == A.INVALID_ARG and "at least one row" in s._errmsg(s._h)
    assert lib.altro_set_constraint_track(s._h, circle, xp, -2, 1) == A.INVALID_ARG
    assert lib.altro_set_constraint_track(s._h, circle, None, 4, 0) == A.INVALID_ARG
    assert lib.altro_set_constraint_track_device(s._h, circle, None, 4, 0) == A.INVALID_ARG
    assert lib.altro_set_constraint_track_device(s._h, circle, ctypes.c_void_p(4096), 0, 0) == A.INVALID_ARG
    _refused(A, lambda: s.set_track_offset(-1), A.INVALID_ARG, "negative")
    assert lib.altro_get_track_offset(s._h, None) == A.INVALID_ARG
    assert lib.altro_get_knot_params(s._h, circle, None) == A.INVALID_ARG
    for f, args in (("altro_add_knot_constraint", (A.CON_CIRCLE, 0, 0, N, 3, None)), ("altro_set_constraint_track", (0, xp, 4, 0)),
                    ("altro_set_constraint_track_device", (0, None, 4, 0)), ("altro_set_track_offset", (0,)),
                    ("altro_get_track_offset", (None,)), ("altro_get_knot_params", (0, xp))):
        assert getattr(lib, f)(None, *args) == A.INVALID_ARG, f
    # a bound's rows are chosen from its finite entries at problem definition: every entry of a knot bound's track is finite
    for bad in (np.inf, -np.inf, np.nan, np.finfo(np.float64).max):
        t = np.tile(np.array([-1.0, -1.0, 1.0, 1.0]), (5, 1))
        t[3, 2] = bad
        _refused(A, lambda: s.set_constraint_track(bound, t), A.INVALID_ARG, "must be finite")
    t = np.tile(np.array([-1.0, 0.5, 1.0, 0.25]), (5, 1))
    _refused(A, lambda: s.set_constraint_track(bound, t), A.INVALID_ARG, "Lower bound")
    # the binding checks shapes before it calls
    with pytest.raises(ValueError):
        s.set_constraint_track(circle, np.zeros((4, 5)))
    with pytest.raises(ValueError):
        s.set_constraint_track(circle, np.zeros((3, 4, 6)))  # per instance, but not 5 instances

    # a knot constraint and no track: every call that evaluates costs refuses, and says which constraint
    u = P.tracking_slalom(_make(A), batch=5, N=N, bounds=False)
    idx = u.add_knot_constraint(A.CON_CIRCLE, 1, N, 3)
    b2 = u.add_knot_control_bound(0, N, np.full((3, 2), -1.0), np.full((3, 2), 1.0))
    assert (idx, b2) == (0, 1)
    for call in (u.solve, u.solve_ilqr, u.solve_async, u.al_init, u.cost, u.update_expansions, u.forward_pass,
                 lambda: u.mpc_run(2, 5), lambda: u.mpc_run_tracked(2, 5)):
        _refused(A, call, A.NOT_READY, "constraint 0 is a knot constraint but has no parameter track", "altro_set_constraint_track")
    _refused(A, lambda: u.mpc_track(3, 1), A.NOT_READY)
    # ... with every track set nothing is missing: the refusal that is left is the machine's (no device here), or none
    u.set_constraint_track(idx, np.array([[5.0, 5.0, 0.1]]))
    try:
        u.cost()
    except A.AltroError as e:
        assert "track" not in str(e)


def test_offset_and_row_map_before_the_device_state(A, P):
    """The window offset is recorded with the problem and answers before any device exists; setting a track leaves it alone.
    altro_mpc_row_map of moving_obstacles: the knot constraints are ONE constraint each -- the circle's rows on [1, N), the
    bound's on [0, N) -- so the map is the per-constraint map of tests/_mpc_common.py."""
    s = P.moving_obstacles(_make(A), batch=5, N=N)
    assert (s.knot_circle, s.knot_bound) == (0, 1) and s.get_track_offset() == 0
    s.set_track_offset(7)
    circles, bounds = P.moving_obstacle_tracks(5, N, N + 13)
    s.set_constraint_track(s.knot_circle, circles[0])  # (shared this time)
    assert s.get_track_offset() == 7
    assert s.get_reference_offset() == 0  # the reference path's window is another one
    assert P.moving_obstacles(_make(A), batch=2, N=N, offset=12).get_track_offset() == 12
    assert len(s.mpc_row_map(1)) == 4 + 6 * (N - 1)
    for shift in (1, 5, N - 1):
        assert np.array_equal(s.mpc_row_map(shift), M.row_map(N, shift, MOVING_CONS)), shift
    r = P.ramped_bounds(_make(A), batch=5, N=10, offset=4)
    assert r.get_track_offset() == 4 and r.knot_bound == 1
    assert np.array_equal(r.mpc_row_map(3), M.row_map(10, 3, [(10, 11, 6, True), (0, 10, 4, False)]))


def test_compute_calls_without_a_device(A, P):
    """On a machine without a GPU the compute calls of a fully defined knot-constraint handle answer ALTRO_HIP_ERROR (or, on a
    machine with one, succeed); the offset getter needs no device either way."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    s = P.moving_obstacles(_make(A), batch=2, N=N, offset=3)
    if r.stdout.strip().endswith("True"):
        assert s.get_knot_params(s.knot_bound).shape == (2, N, 4)
    else:
        for call in (s.solve, s.cost, lambda: s.get_knot_params(s.knot_circle)):
            _refused(A, call, A.HIP_ERROR)
        for call in (lambda: s.set_constraint_track_device(s.knot_circle, 4096, 4, 0),):
            _refused(A, call, A.HIP_ERROR)
    assert s.get_track_offset() == 3


def test_ordinary_per_knot_constraints_are_recorded(A, P):
    """The reference's idiom through altro_add_constraint, one call per knot: recorded without complaint (the setters only
    record); the limit and its text are the problem compiler's -- tests/test_knot_params_layout.py."""
    s = P.moving_obstacles(_make(A), batch=5, N=N, per_knot=True)
    assert s.get_track_offset() == 0
    s = P.ramped_bounds(_make(A), batch=5, N=10, per_knot=True)
    assert s.get_track_offset() == 0
