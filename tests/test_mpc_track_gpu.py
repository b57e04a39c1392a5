"""Closed-loop tracking on the device (include/altro_mpc.h: altro_mpc_track, altro_mpc_track_device, altro_mpc_run_tracked):
without a disturbance it is the rollout bit for bit; under disturbances it is the loop a caller composes on the host from
altro_get_gains and the dynamics; its statistics agree with altro_max_violation and altro_cost; lanes are independent; the
forward pass's limits stop a sample and nothing else; altro_mpc_run_tracked is the caller's own loop over the three entry
points; the facade's TrackClosedLoop gives the C call's bits.  N = 24 unless stated otherwise."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _mpc_common as M  # noqa: F401  (imported, never changed)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24
# the project's bar for trajectories
RTOL, ATOL = 1e-7, 1e-9


def _model_source(name):
    return open(os.path.join(ROOT, "tests", "models", name + ".hpp")).read()


def dx0_of(B, S, n, scale=1e-2):
    """dx0[b][s][i] = scale sin(1 + 3 s + 5 b + 7 i)  (the closed formula of _mpc_common.disturbance, with the sample in the
    place of the cycle)"""
    b, s, i = np.meshgrid(np.arange(B), np.arange(S), np.arange(n), indexing="ij")
    return scale * np.sin(1.0 + 3.0 * s + 5.0 * b + 7.0 * i)


def w_of(B, S, steps, n, scale=1e-2):
    """w[b][s][k][i] = scale sin(2 + 3 s + 5 b + 7 i + 11 k)"""
    b, s, k, i = np.meshgrid(np.arange(B), np.arange(S), np.arange(steps), np.arange(n), indexing="ij")
    return scale * np.sin(2.0 + 3.0 * s + 5.0 * b + 7.0 * i + 11.0 * k)


def _steps_of(N_):
    """non-uniform per-knot steps around 0.05"""
    return (0.05 * (1.0 + 0.4 * np.sin(1.0 + np.arange(N_)))).astype(np.float32)


def _build(A, P, make, case, batch=None, constraints=True):
    """-> (solver, solve)"""
    if case == "turn90_f64":
        s = P.unicycle_turn90(make, batch=batch or 5, N=N, constraints=constraints)
        return s, s.solve
    if case == "three_obstacles_f32":
        s = P.unicycle_three_obstacles(make, batch=batch or 3, N=N, dtype=A.F32, constraints=constraints)
        return s, s.solve
    if case == "triple_integrator":
        s = P.triple_integrator(make, batch=batch or 3, N=N)
        return s, s.solve_ilqr
    if case == "quadrotor12_f32":
        s = P.quadrotor12(make, batch=batch or 2, N=N, dtype=A.F32)
        return s, s.solve
    os.environ.setdefault("ALTRO_HIP_ARCH", "gfx950")
    if case == "cartpole_steps":  # a model per knot (RK4, Euler, the user's own map in turn) AND a step per knot
        kind = A.register_model_source("cartpole_steps", _model_source("cartpole_steps"))
        s = P.cartpole_steps(make, kind, np.arange(N, dtype=np.int32) % 3, batch=batch or 2, N=N, goal=np.linspace(0.5, 0.8, batch or 2))
        s.set_steps(_steps_of(N))
        return s, s.solve
    if case == "cartpole_multi":  # user costs and constraints of several classes, a step per knot
        kind = A.register_model_source("cartpole_multi", _model_source("cartpole_multi"))
        s = P.cartpole_multi(make, kind, batch=batch or 2, N=N, goal=np.linspace(0.5, 0.8, batch or 2))
        s.set_steps(_steps_of(N))
        return s, s.solve
    raise KeyError(case)


# ---- 1. zero disturbance is the rollout, bit for bit -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["turn90_f64", "triple_integrator", "quadrotor12_f32", "cartpole_steps", "cartpole_multi"])
def test_zero_disturbance_is_the_rollout(A, P, hip_make, case):
    """Solve, altro_rollout, track the whole horizon with three samples and neither dx0 nor w: every sample's log is the
    handle's X, U exactly and the deviations are zero.  The issue names cartpole_steps.hpp for the per-knot steps and
    cartpole_multi.hpp for the alternating knot models; the model list lives in cartpole_steps.hpp, so that case carries BOTH
    (models 0, 1, 2 in turn and non-uniform steps) and cartpole_multi.hpp runs with non-uniform steps."""
    s, solve = _build(A, P, hip_make, case)
    solve()
    s.rollout()
    X, U = s.get_trajectory()
    out = s.mpc_track(N, 3)
    st = out["stats"]
    assert out["X_cl"].shape == (s.batch, 3, N + 1, s.n) and out["U_cl"].shape == (s.batch, 3, N, s.m) and st.shape == (s.batch, 3)
    for j in range(3):
        assert np.array_equal(out["X_cl"][:, j], X), (case, j)
        assert np.array_equal(out["U_cl"][:, j], U), (case, j)
    assert (st["max_dx"] == 0).all() and (st["max_du"] == 0).all()
    assert (st["status"] == A.UNSOLVED).all() and (st["steps_done"] == N).all()
    assert np.isfinite(st["cost"]).all() and np.isfinite(st["violation"]).all()
    # a part of the horizon is the same rows
    part = s.mpc_track(7, 2)
    assert np.array_equal(part["X_cl"][:, 1], X[:, :8]) and np.array_equal(part["U_cl"][:, 0], U[:, :7])
    s.close()


# ---- 2. against the loop composed on the host --------------------------------------------------------------------------------
def _host_loop(s, helper, steps, dx0, w, lo=None, hi=None):
    """What a caller had to write: download X, U, K; per knot u = Ubar + K (x - Xbar) in numpy (np.clip where bounds are
    given); the step is the GPU's own altro_rollout on `helper`, a handle of B x S instances of the same problem, reading
    X[1].  -> X_cl, U_cl, U before the clip"""
    B, S, n, m = s.batch, dx0.shape[1], s.n, s.m
    Xbar, Ubar = s.get_trajectory()
    K, _ = s.get_gains()
    x = (s.get_initial_state()[:, None, :] + dx0).reshape(B * S, n)
    X_cl, U_cl, U_raw = [x.copy()], [], []
    Uh = np.zeros((B * S, s.N, m))
    for k in range(steps):
        dx = x.reshape(B, S, n) - Xbar[:, None, k]
        u = Ubar[:, None, k] + np.einsum("bil,bsl->bsi", K[:, k], dx)
        U_raw.append(u.copy())
        if lo is not None:
            u = np.clip(u, lo, hi)
        Uh[:, 0] = u.reshape(B * S, m)
        helper.set_initial_state(x)
        helper.set_trajectory(None, Uh)
        helper.rollout()
        x = helper.get_trajectory()[0][:, 1] + w[:, :, k].reshape(B * S, n)
        X_cl.append(x.copy())
        U_cl.append(u.reshape(B * S, m).copy())
    shape = lambda a, e: np.stack(a, axis=1).reshape(B, S, len(a), e)  # noqa: E731
    return shape(X_cl, n), shape(U_cl, m), shape([r.reshape(B * S, m) for r in U_raw], m)


HOST_CASES = [("turn90_f64", 3, 5, None), ("turn90_f64", 5, 40, None), ("three_obstacles_f32", 3, 5, None),
              ("three_obstacles_f32", 5, 40, None), ("turn90_f64", 3, 5, "saturate")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,B,S,mode", HOST_CASES)
def test_against_the_host_composed_loop(A, P, hip_make, case, B, S, mode):
    """B x S = 15 lanes and 200 lanes (not a multiple of 64, more than one wavefront).  States and controls to the project's
    trajectory bar (1e-9 absolute + 1e-7 relative), max_dx / max_du likewise.  The saturating case clips
    to the problem's own bounds under a disturbance fifty times larger, and first asserts on the numpy reference that a
    control does saturate."""
    s, solve = _build(A, P, hip_make, case, batch=B)
    helper, _ = _build(A, P, hip_make, case, batch=B * S)
    solve()
    scale = 0.5 if mode == "saturate" else 1e-2
    dx0, w = dx0_of(B, S, s.n, scale), w_of(B, S, N, s.n, scale)
    lo = hi = None
    if mode == "saturate":
        lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])  # problems.unicycle_turn90
    Xr, Ur, Uraw = _host_loop(s, helper, N, dx0, w, lo, hi)
    if mode == "saturate":
        assert (Uraw != Ur).any() and ((Ur == lo) | (Ur == hi)).any()
    out = s.mpc_track(N, S, dx0=dx0, w=w, u_lo=lo, u_hi=hi)
    Xbar, Ubar = s.get_trajectory()
    print(f"{case} {B} x {S} {mode}: max |X - X_host| {np.abs(out['X_cl'] - Xr).max():.3g}, max |U - U_host| {np.abs(out['U_cl'] - Ur).max():.3g}")
    assert np.allclose(out["X_cl"], Xr, rtol=RTOL, atol=ATOL)
    assert np.allclose(out["U_cl"], Ur, rtol=RTOL, atol=ATOL)
    st = out["stats"]
    assert (st["status"] == A.UNSOLVED).all() and (st["steps_done"] == N).all()
    assert np.allclose(st["max_dx"], np.abs(Xr - Xbar[:, None]).max(axis=(2, 3)), rtol=RTOL, atol=ATOL)
    assert np.allclose(st["max_du"], np.abs(Ur - Ubar[:, None]).max(axis=(2, 3)), rtol=RTOL, atol=ATOL)
    if mode == "saturate":
        assert (out["U_cl"] >= lo).all() and (out["U_cl"] <= hi).all()
    s.close()
    helper.close()


# ---- 3. statistics against entry points that already exist --------------------------------------------------------------------
def _handle_state(s):
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    return dict(X=X.copy(), U=U.copy(), K=K.copy(), d=d.copy(), lam=s.get_duals(), rho=s.get_penalties(), c=s.get_constraint_values(),
                x0=s.get_initial_state(), stats=s.get_stats().tobytes(), opts=bytes(s.get_options()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["turn90_f64", "three_obstacles_f32"])
def test_statistics_against_existing_entry_points(A, P, hip_make, case):
    """steps = N, B = 3, S = 5.  Violation: a second handle of B x S instances takes the tracked path through
    altro_set_trajectory and answers altro_max_violation -- a maximum has no summation order, so the two are equal exactly.
    Cost: the same problem without constraints answers altro_cost, equal to 1e-12 relative (about 25 ordered fp64 additions;
    contraction may differ between the kernels).  The call leaves the handle's constraint values, duals, penalties, trajectory,
    gains, initial state and statistics as they were, bit for bit."""
    B, S = 3, 5
    s, solve = _build(A, P, hip_make, case, batch=B)
    solve()
    before = _handle_state(s)
    out = s.mpc_track(N, S, dx0=dx0_of(B, S, s.n), w=w_of(B, S, N, s.n))
    stats_only = s.mpc_track(N, S, dx0=dx0_of(B, S, s.n), w=w_of(B, S, N, s.n), log=False)
    after = _handle_state(s)
    for name, v in before.items():
        assert np.array_equal(after[name], v) if isinstance(v, np.ndarray) else after[name] == v, name
    assert set(stats_only) == {"stats"} and stats_only["stats"].tobytes() == out["stats"].tobytes()
    Xl, Ul = out["X_cl"].reshape(B * S, N + 1, s.n), out["U_cl"].reshape(B * S, N, s.m)
    con, _ = _build(A, P, hip_make, case, batch=B * S)
    con.set_trajectory(Xl, Ul)
    viol = con.max_violation().reshape(B, S)
    assert (viol > 0).any()
    assert np.array_equal(out["stats"]["violation"], viol)
    free, _ = _build(A, P, hip_make, case, batch=B * S, constraints=False)
    free.set_trajectory(Xl, Ul)
    J = free.cost().reshape(B, S)
    print(f"{case}: max relative cost difference {np.abs(out['stats']['cost'] / J - 1).max():.3g}")
    assert np.allclose(out["stats"]["cost"], J, rtol=1e-12, atol=0.0)
    for h in (s, con, free):
        h.close()


# ---- 4. lanes are independent --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lanes_are_independent(A, P, hip_make):
    """Sample s of an S = 40 call equals an S = 1 call with that sample's inputs, bit for bit; a repeated call gives the same
    bytes."""
    B, S = 5, 40
    s, solve = _build(A, P, hip_make, "three_obstacles_f32", batch=B)
    solve()
    dx0, w = dx0_of(B, S, s.n), w_of(B, S, N, s.n)
    lo, hi = np.array([0.0, -3.0]), np.array([3.0, 3.0])
    big = s.mpc_track(N, S, dx0=dx0, w=w, u_lo=lo, u_hi=hi)
    again = s.mpc_track(N, S, dx0=dx0, w=w, u_lo=lo, u_hi=hi)
    for name in ("X_cl", "U_cl", "stats"):
        assert big[name].tobytes() == again[name].tobytes(), name
    for j in (0, 17, 39):
        one = s.mpc_track(N, 1, dx0=dx0[:, j:j + 1], w=w[:, j:j + 1], u_lo=lo, u_hi=hi)
        for name in ("X_cl", "U_cl", "stats"):
            assert np.ascontiguousarray(big[name][:, j:j + 1]).tobytes() == one[name].tobytes(), (name, j)
    s.close()


# ---- 5. limits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_limits_stop_one_sample_only(A, P, hip_make):
    """state_max = 3 and one sample 10 away on x[0]: that sample reports ALTRO_STATE_LIMIT with steps_done = 0 and quiet NaN
    from X_cl[1] (and U_cl[1]) on; every other sample is bit-identical to a run without that offset; with
    check_forwardpass_bounds = 0 the sample runs to the end.  A solver status, not a device fault."""
    B, S = 2, 6
    s, solve = _build(A, P, hip_make, "turn90_f64", batch=B)
    solve()
    s.set_options(state_max=3.0)
    dx0, w = dx0_of(B, S, s.n), w_of(B, S, N, s.n)
    ref = s.mpc_track(N, S, dx0=dx0, w=w)
    assert (ref["stats"]["status"] == A.UNSOLVED).all() and (ref["stats"]["steps_done"] == N).all()
    far = dx0.copy()
    far[1, 2, 0] = 10.0
    out = s.mpc_track(N, S, dx0=far, w=w)
    st = out["stats"]
    assert st["status"][1, 2] == A.STATE_LIMIT and st["steps_done"][1, 2] == 0
    assert np.array_equal(out["X_cl"][1, 2, 0], s.get_initial_state()[1] + far[1, 2]) and np.isfinite(out["U_cl"][1, 2, 0]).all()
    assert np.isnan(out["X_cl"][1, 2, 1:]).all() and np.isnan(out["U_cl"][1, 2, 1:]).all()
    assert np.isfinite(st["cost"][1, 2]) and st["max_dx"][1, 2] == 10.0
    others = np.ones((B, S), dtype=bool)
    others[1, 2] = False
    for name in ("X_cl", "U_cl", "stats"):
        assert out[name][others].tobytes() == ref[name][others].tobytes(), name
    s.set_options(check_forwardpass_bounds=0)
    free = s.mpc_track(N, S, dx0=far, w=w)
    assert free["stats"]["status"][1, 2] == A.UNSOLVED and free["stats"]["steps_done"][1, 2] == N
    assert np.isfinite(free["X_cl"][1, 2]).all() and np.isfinite(free["U_cl"][1, 2]).all()
    for name in ("X_cl", "U_cl", "stats"):
        assert free[name][others].tobytes() == ref[name][others].tobytes(), name
    # the control limit, checked behind the state limit (ilqr.hpp:484-495)
    u0 = np.linalg.norm(free["U_cl"][1, 2, 0])  # (the first control of the far sample, whatever the gains make of it)
    assert u0 > 0
    s.set_options(check_forwardpass_bounds=1, state_max=1e8, control_max=0.5 * u0)
    ctl = s.mpc_track(N, S, dx0=far, w=w)
    assert ctl["stats"]["status"][1, 2] == A.CONTROL_LIMIT and ctl["stats"]["steps_done"][1, 2] == 0
    assert np.array_equal(ctl["U_cl"][1, 2, 0], free["U_cl"][1, 2, 0]) and np.isnan(ctl["X_cl"][1, 2, 1:]).all()
    s.close()


# ---- 6. altro_mpc_run_tracked is the caller's own loop ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("batch", [8, 1024])
def test_run_tracked_is_the_callers_loop(A, P, hip_make, batch):
    """kTurn90 with N = 100, 4 cycles, shift 5, the warm-start options of tests/test_mpc_gpu.py: logs, iterations, statuses,
    tracking statistics and the handle's final trajectory, gains, duals, penalties and initial state are those of
    solve; mpc_track(5, 1, w[c]); mpc_advance(5, x0 = the tracked state) bit for bit."""
    cycles, shift = 4, 5
    lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
    W = np.stack([w_of(batch, 1, shift, 3)[:, 0] * np.cos(1.0 + c) for c in range(cycles)])  # [cycles][B][shift][n]
    a = P.batch_turn90(hip_make, batch)
    a.set_options(reset_duals=0, initial_penalty=0.0)
    rec = []
    for c in range(cycles):
        a.solve()
        st = a.get_stats()
        tr = a.mpc_track(shift, 1, w=W[c][:, None], u_lo=lo, u_hi=hi)
        rec.append(dict(iterations=st["iterations_total"].copy(), status=st["status"].copy(), X=tr["X_cl"][:, 0], U=tr["U_cl"][:, 0],
                        track=tr["stats"][:, 0]))
        a.mpc_advance(shift, x0=tr["X_cl"][:, 0, shift])
    b = P.batch_turn90(hip_make, batch)
    b.set_options(reset_duals=0, initial_penalty=0.0)
    out = b.mpc_run_tracked(cycles, shift, W, u_lo=lo, u_hi=hi)
    fa, fb = _handle_state(a), _handle_state(b)
    for name in ("X", "U", "K", "d", "lam", "rho", "x0", "stats"):
        assert np.array_equal(fa[name], fb[name]) if isinstance(fa[name], np.ndarray) else fa[name] == fb[name], name
    assert out["X_cl"].shape == (batch, cycles * shift + 1, 3) and out["U_cl"].shape == (batch, cycles * shift, 2)
    for c in range(cycles):
        rows = slice(c * shift, (c + 1) * shift)
        assert np.array_equal(out["iterations"][:, c], rec[c]["iterations"]) and np.array_equal(out["status"][:, c], rec[c]["status"]), c
        assert np.array_equal(out["X_cl"][:, c * shift:(c + 1) * shift + 1], rec[c]["X"]), c
        assert np.array_equal(out["U_cl"][:, rows], rec[c]["U"]), c
        assert np.ascontiguousarray(out["track"][:, c]).tobytes() == np.ascontiguousarray(rec[c]["track"]).tobytes(), c
    assert np.array_equal(out["X_cl"][:, -1], fa["x0"])
    assert (out["track"]["steps_done"] == shift).all() and (out["track"]["max_dx"] > 0).any()
    if batch == 8:  # without a disturbance and with outputs the caller does not want
        lib = A.load_library()
        lib.altro_mpc_run_tracked.restype = int
        assert lib.altro_mpc_run_tracked(b._h, 2, 1, None, None, None, None, None, None, None, None) == A.OK
    a.close()
    b.close()


# ---- 7. the facade ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_facade_track_closed_loop(A, P, hip_make):
    """perf/track_closed_loop: AugmentedLagrangianiLQR::TrackClosedLoop on the solved kTurn90 batch (N = 100) prints every state,
    control and statistic as a hexadecimal float; the C call on the same problem gives the same bits."""
    B, S, steps = 4, 3, 24
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "perf"), "track_closed_loop"])
    r = subprocess.run([os.path.join(ROOT, "perf", "track_closed_loop"), str(B), str(S), str(steps), "--dump"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^tracked 4 instances x 3 samples for 24 of 100 knots: stopped 0", r.stdout, re.M), r.stdout[:300]
    s = P.batch_turn90(hip_make, B)
    s.solve()
    out = s.mpc_track(steps, S, dx0=dx0_of(B, S, 3), w=w_of(B, S, steps, 3), u_lo=np.array([-1.5, -1.5]), u_hi=np.array([1.5, 1.5]))
    X, U = np.full_like(out["X_cl"], np.nan), np.full_like(out["U_cl"], np.nan)
    stats = np.zeros((B, S), dtype=A.TRACK_STATS_DTYPE)
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] in ("x", "u"):
            (X if f[0] == "x" else U)[int(f[1]), int(f[2]), int(f[3])] = [float.fromhex(v) for v in f[4:]]
        elif f and f[0] == "stats":
            stats[int(f[1]), int(f[2])] = (int(f[3]), int(f[4])) + tuple(float.fromhex(v) for v in f[5:])
    assert np.array_equal(X, out["X_cl"]) and np.array_equal(U, out["U_cl"])
    assert stats.tobytes() == out["stats"].tobytes()
    s.close()


# ---- the device-pointer variant and the asynchronous-solve guard ------------------------------------------------------------------
def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceBuffer:
    """`nbytes` of device memory (hipMalloc / hipMemcpy through ctypes), optionally filled from a host array."""

    def __init__(self, nbytes, fill=None):
        self.hip, self.nbytes = _hip_runtime(), nbytes
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        self.ptr = p.value
        if fill is not None:
            a = np.ascontiguousarray(fill)
            assert a.nbytes == nbytes
            assert self.hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(nbytes), ctypes.c_int(1)) == 0  # host to device

    def read(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(self.nbytes),
                                  ctypes.c_int(2)) == 0  # device to host
        return out

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


@pytest.mark.gpu
def test_device_pointers_and_the_asynchronous_guard(A, P, hip_make):
    """altro_mpc_track_device with every array in device memory gives the host variant's bytes; while an asynchronous solve
    owns the handle the tracking calls answer ALTRO_NOT_READY, and work again behind altro_wait."""
    B, S = 3, 5
    s, _ = _build(A, P, hip_make, "turn90_f64", batch=B)
    s.solve_async()
    for call in (lambda: s.mpc_track(N, S), lambda: s.mpc_track_device(N, S), lambda: s.mpc_run_tracked(2, 1)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value)
    s.wait()
    dx0, w = dx0_of(B, S, s.n), w_of(B, S, N, s.n)
    lo, hi = np.array([-1.5, -np.inf]), np.array([np.inf, 1.5])  # (+-inf allowed: no saturation on that side)
    host = s.mpc_track(N, S, dx0=dx0, w=w, u_lo=lo, u_hi=hi)
    bufs = dict(dx0=DeviceBuffer(dx0.nbytes, dx0), w=DeviceBuffer(w.nbytes, w), lo=DeviceBuffer(lo.nbytes, lo), hi=DeviceBuffer(hi.nbytes, hi),
                X=DeviceBuffer(host["X_cl"].nbytes), U=DeviceBuffer(host["U_cl"].nbytes), st=DeviceBuffer(host["stats"].nbytes))
    s.mpc_track_device(N, S, bufs["dx0"].ptr, bufs["w"].ptr, bufs["lo"].ptr, bufs["hi"].ptr, bufs["X"].ptr, bufs["U"].ptr, bufs["st"].ptr)
    assert bufs["X"].read(np.float64, host["X_cl"].shape).tobytes() == host["X_cl"].tobytes()
    assert bufs["U"].read(np.float64, host["U_cl"].shape).tobytes() == host["U_cl"].tobytes()
    assert bufs["st"].read(A.TRACK_STATS_DTYPE, (B, S)).tobytes() == host["stats"].tobytes()
    assert (host["U_cl"][..., 0] >= -1.5).all() and (host["U_cl"][..., 1] <= 1.5).all()
    for b in bufs.values():
        b.free()
    s.close()
