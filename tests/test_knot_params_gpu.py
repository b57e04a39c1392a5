"""Knot constraints on the device (include/altro_knot_params.h): moving obstacles and ramped bounds against the CPU oracle
given one ordinary constraint per knot; a constant track against an ordinary constraint, bit for bit; host upload against
device upload; the window against a fresh handle; the window moving with the receding-horizon advance; the engine paths such
a handle takes; closed-loop tracking that sees the moving obstacle.
The problems are problems.moving_obstacles (N = 24, tracks of N + 13 = 37 rows) and problems.ramped_bounds (N = 10, 16 rows)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _ledger
import _mpc_common as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROWS = 24, 24 + 13
# the project's fp64 bars -- trajectories, expansions (tests/test_parity_gpu.py: step level), final cost
RTOL, ATOL = 1e-7, 1e-9
MOVING_CONS = [(1, N, 2, False), (0, N, 4, False)]  # problems.moving_obstacles: (k_begin, k_end, rows, equality)
MULTI = open(os.path.join(ROOT, "tests", "models", "cartpole_multi.hpp")).read()


def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceArray:
    """fp64 copy of a host array in device memory (hipMalloc / hipMemcpy through ctypes)."""

    def __init__(self, a):
        self.hip = _hip_runtime()
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(a.nbytes)) == 0
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), ctypes.c_int(1)) == 0  # host to device
        self.ptr = p.value

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def _state(s):
    """everything a solve leaves on the handle"""
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    return dict(stats=s.get_stats(), X=X, U=U, K=K, d=d, lam=s.get_duals(), rho=s.get_penalties(), x0=s.get_initial_state())


def _same(a, b, what, names=None):
    for name in names or a:
        assert a[name].tobytes() == b[name].tobytes(), (what, name)


def _window(track, offset, knots):
    """rows min(offset + k, rows - 1), k in knots, of a track [B][rows][np]"""
    return track[:, np.minimum(offset + np.asarray(knots), track.shape[1] - 1)]


def _compare_with_oracle(A, o, g, what, gains_bar=None):
    o.solve()
    g.solve()
    so, sg = o.get_stats(), g.get_stats()
    print(f"{what}: iterations {so['iterations_total'][:5]}, outer {so['iterations_outer'][:5]}, statuses {np.unique(so['status'])}")
    assert (so["status"] == A.SOLVED).all()
    for f in ("status", "iterations_total", "iterations_outer"):
        assert (so[f] == sg[f]).all(), (f, np.flatnonzero(so[f] != sg[f]))
    Xo, Uo = o.get_trajectory()
    Xg, Ug = g.get_trajectory()
    _ledger.close(Xg, Xo, RTOL, ATOL, "X")
    _ledger.close(Ug, Uo, RTOL, ATOL, "U")
    _ledger.close(sg["cost"], so["cost"], 1e-10, 0.0, "stat cost")
    _ledger.close(sg["violation"], so["violation"], 1e-7, 1e-12, "stat violation")
    if gains_bar is not None:
        Ko, do = o.get_gains()
        Kg, dg = g.get_gains()
        _ledger.close_normwise(Kg, Ko, gains_bar, "K normwise")
        # (the feedforward term d is the step of the LAST backward pass: at a converged solution it is zero up to rounding
        #  -- 1e-12 here against controls of 1e2 -- so its own norm is no scale; it is a control increment and is held to the
        #  same fraction of the controls' norm.  tests/test_parity_gpu.py's full-solve test compares K alone.)
        print(f"{what}: max |d| oracle {np.abs(do).max():.3g}, device {np.abs(dg).max():.3g}, max |U| {np.abs(Uo).max():.3g}")
        _ledger.close(dg, do, 0.0, gains_bar * np.abs(Uo).max(), "d against the controls' norm")
    return so


# ---- 1. against the oracle, which takes one ordinary constraint per knot -------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 12])
@pytest.mark.parametrize("batch", [5, 200])
def test_moving_obstacles_against_the_oracle(A, P, oracle_make, hip_make, batch, offset):
    """Status, total and outer iterations exact; X, U to 1e-7 relative + 1e-9 absolute; the final cost to 1e-10 relative, the
    violation to 1e-7 relative + 1e-12; every instance ends solved.  On the CPU oracle, offset 0: 20 / 20 / 21 / 22 / 20
    iterations, 5 outer, circle 0 active (clearance -2e-4 .. 0), the bound saturated on 2 to 14 knots; offset 12: 5 / 6 / 11 /
    15 / 14 iterations, 1 to 4 outer, the bound saturated on up to all 24 knots, the circles inactive."""
    o = P.moving_obstacles(oracle_make, batch=batch, N=N, rows=ROWS, offset=offset, per_knot=True)
    g = P.moving_obstacles(hip_make, batch=batch, N=N, rows=ROWS, offset=offset)
    so = _compare_with_oracle(A, o, g, f"moving_obstacles B {batch} offset {offset}")
    want = {0: ([20, 20, 21, 22, 20], [5, 5, 5, 5, 5]), 12: ([5, 6, 11, 15, 14], [1, 2, 3, 3, 4])}[offset]
    assert so["iterations_total"][:5].tolist() == want[0] and so["iterations_outer"][:5].tolist() == want[1]
    assert (so["iterations_total"].reshape(-1, 5) == np.array(want[0])).all()  # (the parameter repeats with b mod 5)
    o.close()
    g.close()


@pytest.mark.parametrize("offset", [0, 4])
def test_ramped_bounds_against_the_oracle(A, P, oracle_make, hip_make, offset):
    """problems.ramped_bounds (no tracking cost: the records hold constraint parameters only; n = 6, the MFMA recursion):
    the bars of the test above, and the gains to 1e-6 norm-wise.  On the CPU oracle: all solved, 17 to 20 iterations, 8 outer."""
    o = P.ramped_bounds(oracle_make, batch=5, N=10, offset=offset, per_knot=True)
    g = P.ramped_bounds(hip_make, batch=5, N=10, offset=offset)
    so = _compare_with_oracle(A, o, g, f"ramped_bounds offset {offset}", gains_bar=1e-6)
    assert so["iterations_total"].min() >= 17 and so["iterations_total"].max() <= 20 and (so["iterations_outer"] == 8).all()
    # the ramp binds at both ends of the horizon (window at row 0; from row 4 on the far end has widened past the controls)
    U = g.get_trajectory()[1]
    ub = _window(P.ramped_bound_track(5, 16), offset, np.arange(10))[:, :, 2]
    sat = np.abs(U).max(axis=2) >= ub - 1e-3
    print("saturated knots per instance:", [np.flatnonzero(r).tolist() for r in sat])
    assert sat[:, 0].all() and (offset != 0 or sat[:, -1].all())
    o.close()
    g.close()


@pytest.mark.parametrize("problem,offset", [("moving_obstacles", 0), ("moving_obstacles", 12), ("ramped_bounds", 4)])
def test_step_level_against_the_oracle(P, oracle_make, hip_make, problem, offset):
    """update_expansions, cost and one forward pass with the bars of tests/test_parity_gpu.py's step-level test."""
    n_knots = N if problem == "moving_obstacles" else 10
    o = getattr(P, problem)(oracle_make, batch=5, N=n_knots, offset=offset, per_knot=True)
    g = getattr(P, problem)(hip_make, batch=5, N=n_knots, offset=offset)
    for s in (o, g):
        s.rollout()
    _ledger.close(g.cost(), o.cost(), 1e-12, 0.0, "cost")
    for s in (o, g):
        s.update_expansions()
    for k in (0, 1, n_knots // 2, n_knots - 1, n_knots):
        eo, eg = o.get_expansion(k), g.get_expansion(k)
        for key in ("lxx", "lx") + (("A", "B", "lxu", "luu", "lu") if k < n_knots else ()):
            _ledger.close(eg[key], eo[key], 1e-10, 1e-12, "expansion " + key)
    _ledger.close(g.get_knot_costs(), o.get_knot_costs(), 1e-11, 1e-13, "knot costs")
    for s in (o, g):
        s.backward_pass()
        s.forward_pass()
    so, sg = o.get_stats(), g.get_stats()
    assert (so["alpha"] == sg["alpha"]).all()
    _ledger.close(sg["cost"], so["cost"], 1e-9, 0.0, "cost after the forward pass")
    Xo, Uo = o.get_trajectory()
    Xg, Ug = g.get_trajectory()
    _ledger.close(Xg, Xo, 1e-8, 1e-10, "X after the forward pass")
    _ledger.close(Ug, Uo, 1e-8, 1e-10, "U after the forward pass")
    o.close()
    g.close()


# ---- 2. a constant track is an ordinary constraint ------------------------------------------------------------------------------
def _turn90_with(A, P, make, batch, dtype, knot_kind, per_instance, rows):
    """kTurn90 (N = 24) with, in this order, two circles on [1, N), the control bound +-1.5 on [0, N) and the goal constraint on
    [N, N + 1).  knot_kind None: all three ordinary, and the handle forced onto the general kernels by uniform set_steps;
    else that one is a knot constraint whose track has `rows` equal rows (shared, or per instance)."""
    s = P.unicycle_turn90(make, batch=batch, N=N, dtype=dtype, constraints=False)
    xf = np.array([1.5, 1.5, np.pi / 2])
    circles = np.array([0.45, 0.2, 0.15, 1.15, 0.95, 0.2])
    bound = np.array([-1.5, -1.5, 1.5, 1.5])
    if per_instance:
        circles = circles + 0.01 * np.arange(batch)[:, None] * np.array([1.0, -1.0, 0.1, -1.0, 1.0, 0.1])
        xf = xf + 0.02 * np.arange(batch)[:, None] * np.array([1.0, -1.0, 0.5])
        bound = np.tile(bound, (batch, 1))  # (an ordinary bound is shared: the per-instance track repeats it)
    track = lambda p: np.repeat(p[..., None, :], rows, axis=-2)  # noqa: E731
    index = None
    for kind, kb, ke, par in ((A.CON_CIRCLE, 1, N, circles), (A.CON_CONTROL_BOUND, 0, N, bound), (A.CON_GOAL, N, N + 1, xf)):
        if kind == knot_kind:
            index = s.add_knot_constraint(kind, kb, ke, par.shape[-1])
            s.set_constraint_track(index, track(par))
        else:
            s.add_constraint(kind, kb, ke, par[0] if kind == A.CON_CONTROL_BOUND and par.ndim == 2 else par)
    if knot_kind is None:
        s.set_steps(np.full(N, np.float32(np.float32(3.0) / np.float32(N)), dtype=np.float32))
    return s, index, dict(zip((A.CON_CIRCLE, A.CON_CONTROL_BOUND, A.CON_GOAL), (circles, bound, xf)))


_ORDINARY = {}  # (dtype, per_instance) -> what the handle with ordinary constraints leaves: solved once, never changed


def _ordinary_turn90(A, P, make, batch, dtype_name, per_instance):
    key = (dtype_name, per_instance)
    if key not in _ORDINARY:
        u, _, _ = _turn90_with(A, P, make, batch, getattr(A, dtype_name), None, per_instance, 1)
        u.solve()
        _ORDINARY[key] = _state(u)
        u.close()
    return _ORDINARY[key]


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("rows", [1, 3], ids=["one_row", "equal_rows"])
@pytest.mark.parametrize("per_instance", [False, True], ids=["shared", "per_instance"])
@pytest.mark.parametrize("kind_name", ["CON_CIRCLE", "CON_CONTROL_BOUND", "CON_GOAL"])
def test_constant_track_equals_an_ordinary_constraint(A, P, hip_make, kind_name, per_instance, rows, dtype_name):
    """A track with one row, and one with three equal rows (the window inside the track, and clamped to its end), each shared
    and per instance, against altro_add_constraint on the general kernels: statistics, trajectory, duals, penalties and gains
    bit for bit, and get_knot_params returns the host rows."""
    B, kind, dtype = 5, getattr(A, kind_name), getattr(A, dtype_name)
    t, index, par = _turn90_with(A, P, hip_make, B, dtype, kind, per_instance, rows)
    got = t.get_knot_params(index)
    want = np.broadcast_to(par[kind][:, None, :] if per_instance else par[kind], got.shape)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    t.solve()
    a, b = _state(t), _ordinary_turn90(A, P, hip_make, B, dtype_name, per_instance)
    assert a["stats"]["iterations_total"].min() > 1
    if dtype == A.F64:
        assert (a["stats"]["status"] == A.SOLVED).all()
    _same(a, b, f"constant {kind_name}")
    t.close()


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("rows", [1, 2], ids=["one_row", "equal_rows"])
@pytest.mark.parametrize("per_instance", [False, True], ids=["shared", "per_instance"])
def test_constant_track_of_a_user_constraint(A, P, hip_make, per_instance, rows, dtype_name):
    """tests/models/cartpole_multi.hpp's sway limit (user constraint type 0, two parameters, two inequality rows) as a knot
    constraint with a constant track against altro_add_user_constraint_type, on problems.cartpole_multi's set-up."""
    kind = A.register_model_source("cartpole_multi", MULTI)
    B, Nc, dtype = 4, 60, getattr(A, dtype_name)
    goals = np.array([1.0, 0.8, 1.2, 0.9])
    sway = np.array([-0.05, 0.05]) + (0.004 * np.arange(B)[:, None] * np.array([-1.0, 1.0]) if per_instance else 0.0)
    pair = []
    for knot in (True, False):
        # problems.cartpole_multi, constraint by constraint (the sway limit is the second registration)
        s = hip_make(4, 1, Nc, B, dtype)
        h = np.float32(0.05)
        hd = float(h)
        stage = np.stack([goals, np.full(B, 1e-1 * hd), np.full(B, 2.0 * hd), np.full(B, 1e-1 * hd), np.full(B, 1e-1 * hd),
                          np.full(B, 1e-2 * hd)], axis=1)
        s.set_model(kind)
        s.set_uniform_step(h)
        s.set_user_cost(0, Nc, stage, type=0)
        s.set_user_cost(Nc, Nc + 1, np.stack([goals, np.full(B, 100.0), np.full(B, 100.0)], axis=1), type=1)
        s.add_control_bound(0, Nc, [-3.0], [3.0])
        if knot:
            index = s.add_knot_constraint(A.CON_USER, 1, Nc, 2, user_type=0)
            assert index == 1
            s.set_constraint_track(index, np.repeat(sway[..., None, :], rows, axis=-2))
        else:
            s.add_user_constraint(1, Nc, sway, type=0)
            s.set_steps(np.full(Nc, h, dtype=np.float32))
        s.add_user_constraint(1, Nc, np.array([0.6]), type=2)
        s.add_user_constraint(Nc, Nc + 1, goals[:, None].copy(), type=1)
        s.set_initial_state(np.zeros(4))
        s.set_trajectory(None, np.zeros((Nc, 1)))
        pair.append(s)
    t, u = pair
    t.solve()
    u.solve()
    a, b = _state(t), _state(u)
    assert a["stats"]["iterations_total"].min() > 1
    _same(a, b, "constant user constraint")
    t.close()
    u.close()


def test_knot_params_are_the_host_rows(A, P, hip_make):
    """70 instances (past one wavefront) with random rows of their own, two knot constraints of odd widths side by side (3 + 4
    parameters: a padded record), window at row 2 with the clamp inside it: get_knot_params returns the host rows bit for bit,
    before and after a new track and a new offset."""
    B, rows = 70, N - 3
    rng = np.random.RandomState(20261018)
    circ = rng.standard_normal((B, rows, 3))
    ub = 1.0 + rng.uniform(size=(B, rows, 2))
    bnd = np.concatenate([-ub, ub], axis=2)
    s = P.unicycle_turn90(hip_make, batch=B, N=N, constraints=False)
    ci = s.add_knot_constraint(A.CON_CIRCLE, 3, N - 2, 3)
    bi = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 4)
    s.set_constraint_track(ci, circ)
    s.set_constraint_track(bi, bnd)
    s.set_track_offset(2)
    assert s.get_knot_params(ci).tobytes() == np.ascontiguousarray(_window(circ, 2, np.arange(3, N - 2))).tobytes()
    assert s.get_knot_params(bi).tobytes() == np.ascontiguousarray(_window(bnd, 2, np.arange(N))).tobytes()
    assert (np.minimum(2 + np.arange(N), rows - 1) == rows - 1).sum() > 1
    s.set_constraint_track(ci, circ[7, :5])  # a shared, shorter track: the offset stays
    assert s.get_track_offset() == 2
    want = np.broadcast_to(circ[7, np.minimum(2 + np.arange(3, N - 2), 4)], (B, N - 5, 3))
    assert s.get_knot_params(ci).tobytes() == np.ascontiguousarray(want).tobytes()
    s.set_track_offset(0)
    assert s.get_knot_params(bi).tobytes() == np.ascontiguousarray(_window(bnd, 0, np.arange(N))).tobytes()
    s.close()


# ---- 3. host upload against device upload; shared against repeated ------------------------------------------------------------
def test_device_upload_and_shared_tracks(A, P, hip_make):
    B = 70
    circles, bounds = P.moving_obstacle_tracks(B, N, ROWS)
    host = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=5)
    dev = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=5)
    dc, db = DeviceArray(circles + 1.0), DeviceArray(bounds)
    dev.set_constraint_track_device(dev.knot_circle, dc.ptr, ROWS, True)  # (other circles first: the next call replaces them)
    dc2 = DeviceArray(circles)
    dev.set_constraint_track_device(dev.knot_circle, dc2.ptr, ROWS, True)
    dev.set_constraint_track_device(dev.knot_bound, db.ptr, ROWS, True)
    assert dev.get_track_offset() == 5  # a new track leaves the window alone
    for idx in (host.knot_circle, host.knot_bound):
        assert host.get_knot_params(idx).tobytes() == dev.get_knot_params(idx).tobytes()
    host.solve()
    dev.solve()
    _same(_state(host), _state(dev), "device upload")
    for d in (dc, dc2, db):
        d.free()
    # one shared track (instance 3's) against the same track repeated for every instance
    shared = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS)
    repeated = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS)
    for idx, track in ((shared.knot_circle, circles), (shared.knot_bound, bounds)):
        shared.set_constraint_track(idx, track[3])
        repeated.set_constraint_track(idx, np.repeat(track[3:4], B, axis=0))
        assert shared.get_knot_params(idx).tobytes() == repeated.get_knot_params(idx).tobytes()
    shared.solve()
    repeated.solve()
    _same(_state(shared), _state(repeated), "shared track")
    for s in (host, dev, shared, repeated):
        s.close()


# ---- 4. the window ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [5, 20])
def test_window_equals_a_fresh_handle(A, P, hip_make, offset):
    """Offset o on tracks of 37 rows against a fresh handle that is given rows o .. o + N - 1 on the host (o = 20: the window
    runs past the track, the last row is held)."""
    B = 5
    circles, bounds = P.moving_obstacle_tracks(B, N, ROWS)
    win = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    rows = np.minimum(offset + np.arange(N), ROWS - 1)
    if offset == 20:
        assert (rows == ROWS - 1).sum() > 1
    fresh = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    fresh.set_constraint_track(fresh.knot_circle, circles[:, rows])
    fresh.set_constraint_track(fresh.knot_bound, bounds[:, rows])
    fresh.set_track_offset(0)
    assert win.get_track_offset() == offset and fresh.get_track_offset() == 0
    for idx in (win.knot_circle, win.knot_bound):
        assert win.get_knot_params(idx).tobytes() == fresh.get_knot_params(idx).tobytes()
    win.solve()
    fresh.solve()
    _same(_state(win), _state(fresh), f"offset {offset}")
    win.close()
    fresh.close()


# ---- 5. the advance -----------------------------------------------------------------------------------------------------------------
def test_advance_moves_the_window(A, P, hip_make):
    B, shift = 5, 5
    s = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS)
    moved = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=shift)
    s.solve()
    before = _state(s)
    src = s.mpc_row_map(shift)
    assert np.array_equal(src, M.row_map(N, shift, MOVING_CONS))
    s.mpc_advance(shift)
    assert s.get_track_offset() == shift and s.get_reference_offset() == shift  # the tracking cost's window moves too
    for idx in (s.knot_circle, s.knot_bound):
        assert s.get_knot_params(idx).tobytes() == moved.get_knot_params(idx).tobytes()
    after = _state(s)
    Xn, Un, lam_n, rho_n = M.shifted(before["X"], before["U"], before["lam"], before["rho"], src, shift, M.reset_penalty(s))
    for name, want in (("X", Xn), ("U", Un), ("lam", lam_n), ("rho", rho_n), ("x0", before["X"][:, shift])):
        assert after[name].tobytes() == np.ascontiguousarray(want).tobytes(), name
    s.mpc_advance(shift, w=np.zeros((B, 3)))
    assert s.get_track_offset() == 2 * shift
    # no tracking cost: the track offset moves alone
    r = P.ramped_bounds(hip_make, batch=B, N=10)
    r.solve()
    r.mpc_advance(3)
    assert r.get_track_offset() == 3 and r.get_reference_offset() == 0
    want = _window(P.ramped_bound_track(B, 16), 3, np.arange(10))
    assert r.get_knot_params(r.knot_bound).tobytes() == np.ascontiguousarray(want).tobytes()
    r.set_track_offset(2**31 - 3)
    r.mpc_advance(5)
    assert r.get_track_offset() == 2**31 - 1  # saturates
    # a handle without a knot constraint keeps offset 0, and its results are those of a handle that never heard of tracks
    plain = P.unicycle_turn90(hip_make, batch=2, N=N)
    old = P.unicycle_turn90(hip_make, batch=2, N=N)
    plain.set_track_offset(0)
    for h in (plain, old):
        h.solve()
        h.mpc_advance(shift)
        h.solve()
    assert plain.get_track_offset() == 0
    _same(_state(plain), _state(old), "no knot constraint")
    for h in (s, moved, r, plain, old):
        h.close()


@pytest.mark.parametrize("B", [8, 1024])
def test_mpc_loops_equal_the_callers_loop(A, P, hip_make, B):
    """mpc_run and mpc_run_tracked (3 cycles, shift 5, the disturbance of _mpc_common.disturbance) against the caller's own
    loop of solve / mpc_track / mpc_advance: logs, statistics and what is left on the handle, bit for bit."""
    cycles, shift = 3, 5
    W = M.disturbance(cycles, B, 3)
    a = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS)
    b = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS)
    Xl, Ul, it, st = [], [], [], []
    for c in range(cycles):
        a.solve()
        X, U = a.get_trajectory()
        Xl.append(a.get_initial_state()[:, None])
        Xl.append(X[:, 1:shift])
        Ul.append(U[:, :shift])
        it.append(a.get_stats()["iterations_total"])
        st.append(a.get_stats()["status"])
        a.mpc_advance(shift, w=W[c])
    Xl.append(a.get_initial_state()[:, None])
    out = b.mpc_run(cycles, shift, W)
    assert out["X_cl"].tobytes() == np.ascontiguousarray(np.concatenate(Xl, axis=1)).tobytes()
    assert out["U_cl"].tobytes() == np.ascontiguousarray(np.concatenate(Ul, axis=1)).tobytes()
    assert np.array_equal(out["iterations"], np.stack(it, axis=1)) and np.array_equal(out["status"], np.stack(st, axis=1))
    assert a.get_track_offset() == b.get_track_offset() == cycles * shift
    _same(_state(a), _state(b), "mpc_run")
    assert a.get_knot_params(a.knot_circle).tobytes() == b.get_knot_params(b.knot_circle).tobytes()
    a.close()
    b.close()
    # tracked: w [cycles][B][shift][n] from the same closed formula, one row per tracked knot
    Wt = np.ascontiguousarray(M.disturbance(cycles * shift, B, 3).reshape(cycles, shift, B, 3).transpose(0, 2, 1, 3))
    lo, hi = np.array([-0.7, -0.7]), np.array([0.7, 0.7])
    a = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS)
    b = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS)
    Xl, Ul, track = [], [], []
    for c in range(cycles):
        a.solve()
        t = a.mpc_track(shift, 1, w=Wt[c][:, None], u_lo=lo, u_hi=hi)
        Xl.append(t["X_cl"][:, 0, :shift])
        Ul.append(t["U_cl"][:, 0])
        track.append(t["stats"][:, 0])
        a.mpc_advance(shift, x0=t["X_cl"][:, 0, shift])
    Xl.append(a.get_initial_state()[:, None])
    out = b.mpc_run_tracked(cycles, shift, Wt, u_lo=lo, u_hi=hi)
    assert out["X_cl"].tobytes() == np.ascontiguousarray(np.concatenate(Xl, axis=1)).tobytes()
    assert out["U_cl"].tobytes() == np.ascontiguousarray(np.concatenate(Ul, axis=1)).tobytes()
    assert out["track"].tobytes() == np.ascontiguousarray(np.stack(track, axis=1)).tobytes()
    assert a.get_track_offset() == b.get_track_offset() == cycles * shift
    _same(_state(a), _state(b), "mpc_run_tracked")
    a.close()
    b.close()


# ---- 6. the engine paths ------------------------------------------------------------------------------------------------------------
_SCRIPT = r'''
import importlib, sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
A = g.load_package()
P = importlib.import_module("altro_cpp_amd.problems")
make = lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)
out = {}
for B in (8, 1024, 4608):
    s = P.moving_obstacles(make, batch=B, N=24, rows=37, offset=5)
    s.solve()
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    t = s.get_timing()
    for name, v in (("stats", s.get_stats()), ("X", X), ("U", U), ("K", K), ("d", d), ("lam", s.get_duals()), ("rho", s.get_penalties()),
                    ("circle", s.get_knot_params(s.knot_circle)), ("bound", s.get_knot_params(s.knot_bound))):
        out["%%d_%%s" %% (B, name)] = v[:1024]
        if B == 4608:  # forty instances from each further quarter of the batch: one slice per chain
            for q in (1, 2, 3):
                out["%%d_%%s_q%%d" %% (B, name, q)] = v[q * 1152:q * 1152 + 40]
    out["%%d_timing" %% B] = np.array([t["fused_sweeps"], t["loop_workgroups"], t["segment_columns"], t["twin_workgroups"], t["sweeps"]])
    s.close()
np.savez(sys.argv[1], **out)
'''


def test_engine_paths(tmp_path):
    """Batches 8, 1024 and 4608 (one chain and the persistent kernel's domain; one chain of batched sweeps; four chains with
    shadow columns allocated): the three agree bit for bit on ALL their common instances (8, and 1024); forty instances from
    each further quarter of the 4608 -- one slice in every chain -- equal the instance of their parameter set (b mod 5: path,
    initial state and tracks repeat with it) in the batch of 8; no launch of the persistent or of the loop kernel, no twin, no
    segment column; and once more with LDS, candidates and shadow columns poisoned (ALTRO_HIP_DEBUG_POISON=1) in a fresh
    process, identical."""
    def run(tag, env_extra):
        out = str(tmp_path / f"{tag}.npz")
        subprocess.run([sys.executable, "-c", _SCRIPT % ROOT, out], check=True, env=dict(os.environ, **env_extra), timeout=600)
        return np.load(out)

    ref, poisoned = run("default", {}), run("poisoned", {"ALTRO_HIP_DEBUG_POISON": "1"})
    for B in (8, 1024, 4608):
        fused, loop_wg, seg_cols, twins, sweeps = ref[f"{B}_timing"]
        assert (fused, loop_wg, seg_cols, twins) == (0, 0, 0, 0) and sweeps > 1, (B, ref[f"{B}_timing"])
        for name in ("stats", "X", "U", "K", "d", "lam", "rho", "circle", "bound"):
            assert ref[f"{B}_{name}"][:8].tobytes() == ref[f"8_{name}"].tobytes(), (B, name)
            assert ref[f"{B}_{name}"].tobytes() == ref[f"1024_{name}"][:len(ref[f"{B}_{name}"])].tobytes(), (B, name)
    assert len(ref["4608_X"]) == len(ref["1024_X"]) == 1024
    for q in (1, 2, 3):
        same_set = (q * 1152 + np.arange(40)) % 5
        for name in ("stats", "X", "U", "K", "d", "lam", "rho", "circle", "bound"):
            assert ref[f"4608_{name}_q{q}"].tobytes() == np.ascontiguousarray(ref[f"8_{name}"][same_set]).tobytes(), (q, name)
    for k in ref.files:
        if not k.endswith("_timing"):
            assert ref[k].tobytes() == poisoned[k].tobytes(), ("poisoned", k)


# ---- 7. closed-loop tracking sees the moving obstacle --------------------------------------------------------------------------
def test_mpc_track_sees_the_moving_obstacle(A, P, hip_make):
    """mpc_track over the whole horizon on the solved handle: `violation` equals altro_max_violation of the tracked path on a
    second handle with the same tracks exactly, `cost` equals altro_cost to 1e-12 relative -- the bars of
    tests/test_mpc_track_gpu.py.  A disturbance that pushes ONE sample into circle 0 raises that sample's violation only."""
    B, S, offset = 5, 3, 0
    s = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    s.solve()
    b, j, i = np.meshgrid(np.arange(B), np.arange(S), np.arange(3), indexing="ij")
    dx0 = 1e-3 * np.sin(1.0 + 3.0 * j + 5.0 * b + 7.0 * i)
    out = s.mpc_track(N, S, dx0=dx0)
    st = out["stats"]
    assert (st["steps_done"] == N).all()
    for smp in range(S):  # (one handle per sample: the instance decides the tracks, so the batch cannot carry the samples)
        con = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
        con.set_trajectory(out["X_cl"][:, smp], out["U_cl"][:, smp])
        assert st["violation"][:, smp].tobytes() == con.max_violation().tobytes(), smp
        free = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=offset, bounds=False)
        free.set_trajectory(out["X_cl"][:, smp], out["U_cl"][:, smp])
        J = free.cost()
        print(f"sample {smp}: max relative cost difference {np.abs(st['cost'][:, smp] / J - 1).max():.3g}")
        _ledger.close(st["cost"][:, smp], J, 1e-12, 0.0, "mpc_track cost against altro_cost")
        con.close()
        free.close()
    # one sample of instance 2 is pushed at knot 9 towards the centre of circle 0 as it stands on knot 10
    circles, _ = P.moving_obstacle_tracks(B, N, ROWS)
    X = s.get_trajectory()[0]
    calm = s.mpc_track(N, S, w=np.zeros((B, S, N, 3)))
    w = np.zeros((B, S, N, 3))
    w[2, 1, 9, :2] = circles[2, 10, :2] - X[2, 10, :2]
    hit = s.mpc_track(N, S, w=w)
    dv = hit["stats"]["violation"] - calm["stats"]["violation"]
    print("violation with the push:", hit["stats"]["violation"][2], "without:", calm["stats"]["violation"][2])
    assert dv[2, 1] > 1e-3
    dv[2, 1] = 0.0
    assert not dv.any()
    s.close()


def test_solve_without_a_track_and_async(A, P, hip_make):
    """On a live device: a knot constraint whose track never came answers ALTRO_NOT_READY from the engine too (the device
    state exists); the new calls answer ALTRO_NOT_READY while a solve is in flight."""
    s = P.unicycle_turn90(hip_make, batch=2, N=N, constraints=False)
    ci = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 3)
    dz = DeviceArray(np.array([[0.5, 0.2, 0.1]]))
    got = s.get_initial_state()  # (creates the device state)
    assert got.shape == (2, 3) and not s.get_knot_params(ci).any()
    for call in (s.solve, s.cost, s.update_expansions):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value) and "track" in str(e.value)
    s.set_constraint_track_device(ci, dz.ptr, 1, False)
    s.solve()
    assert (s.get_stats()["status"] == A.SOLVED).all()
    with pytest.raises(A.AltroError) as e:
        s.add_knot_constraint(A.CON_CIRCLE, 1, N, 3)  # problem definition is over
    assert f"({A.NOT_READY})" in str(e.value)
    t = P.moving_obstacles(hip_make, batch=300, N=N, rows=ROWS)
    t.solve_async()
    for call in (lambda: t.set_constraint_track(t.knot_circle, np.zeros((4, 6))), lambda: t.set_track_offset(3), t.get_track_offset,
                 lambda: t.get_knot_params(t.knot_bound), lambda: t.set_constraint_track_device(t.knot_circle, 4096, 4, 0)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value) and "asynchronous" in str(e.value)
    t.wait()
    assert (t.get_stats()["status"] == A.SOLVED).all()
    dz.free()
    s.close()
    t.close()


# ---- 8. the facade ------------------------------------------------------------------------------------------------------------------
def test_facade_per_knot_constraint_loop(A, P, hip_make, tmp_path):
    """tests/cpp/knot_params_facade_driver.cpp: the reference's loops prob.SetConstraint(CircleConstraint, k) over knots
    1 .. 23 and prob.SetConstraint(ControlBound, k) over knots 0 .. 23, an object of its own on every knot (24 distinct knots,
    more than 8), beside the per-knot cost loop, solved through the facade; the C calls on the same rows give the same bits,
    and AdvanceHorizon(5) moves both windows.  (Before knot constraints existed the driver ended in "too many distinct
    knot-point classes".)"""
    B, offset, shift = 5, 5, 5
    exe = str(tmp_path / "knot_params_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "knot_params_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    Xref, Uref, h = P.slalom_path(B, N, ROWS)
    circles, bounds = P.moving_obstacle_tracks(B, N, ROWS)
    rows = np.minimum(offset + np.arange(N + 1), ROWS - 1)
    path = str(tmp_path / "rows.bin")
    np.ascontiguousarray(np.concatenate([Xref[:, rows], Uref[:, rows], circles[:, rows], bounds[:, rows]], axis=2)).tofile(path)
    r = subprocess.run([exe, path, str(B), str(N), repr(float(h))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = dict(X=np.full((B, N + 1, 3), np.nan), U=np.full((B, N, 2), np.nan))
    head = None
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) > 4 and f[0] == "first" and f[1] in ("x", "u"):
            got["X" if f[1] == "x" else "U"][int(f[2]), int(f[3])] = [float.fromhex(v) for v in f[4:]]
        elif len(f) == 9 and f[0] == "first" and f[1] == "iterations":
            head = (int(f[2]), int(f[4]), int(f[6]), int(f[8]))
    assert "advanced offset %d reference %d" % (shift, shift) in r.stdout.splitlines(), r.stdout[-300:]
    s = P.moving_obstacles(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    s.set_reference(Xref[:, rows], Uref[:, rows])  # the N + 1 rows the facade holds
    s.set_constraint_track(s.knot_circle, circles[:, rows])
    s.set_constraint_track(s.knot_bound, bounds[:, rows])
    s.set_track_offset(0)
    s.solve()
    st = s.get_stats()
    X, U = s.get_trajectory()
    assert head == (st["iterations_total"][0], st["iterations_outer"][0], st["status"][0], 0), head
    assert st["iterations_total"][0] > 1 and not np.isnan(got["X"]).any() and not np.isnan(got["U"]).any()
    assert got["X"].tobytes() == X.tobytes() and got["U"].tobytes() == U.tobytes()
    s.close()
