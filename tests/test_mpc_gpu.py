"""Receding-horizon advance on the device (include/altro_mpc.h): one advance against its numpy statement bit for bit, closed
loops against the host-composed advance (bit for bit) and against the CPU oracle, altro_mpc_run against the caller's own
loop, the asynchronous-solve guard, and the facade driver perf/benchmark_mpc."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _mpc_common as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARTPOLE = open(os.path.join(ROOT, "tests", "models", "cartpole.hpp")).read()
CYCLES, SHIFT = 6, 5


# ---- device memory without torch: the HIP runtime the solver library has already loaded into this process ---------------
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


# ---- 4. one advance against numpy, bit for bit ---------------------------------------------------------------------------
def _build(A, P, make, case):
    """-> (solver, solve, cons)"""
    if case == "turn90_f64_b1":
        s = P.batch_turn90(make, 1)
        return s, s.solve, M.TURN90_CONS(s.N)
    if case == "turn90_f64_b300":
        s = P.batch_turn90(make, 300)
        return s, s.solve, M.TURN90_CONS(s.N)
    if case == "three_obstacles_f32_b300":
        s = P.batch_three_obstacles(make, 300, dtype=A.F32)
        return s, s.solve, M.THREE_OBSTACLES_CONS(s.N)
    if case == "triple_integrator_b16":
        s = P.batch_triple_integrator(make, 16)
        return s, s.solve_ilqr, []
    if case == "quadrotor12_f32_b8":
        s = P.batch_quadrotor12(make, 8, dtype=A.F32)
        return s, s.solve, [(0, s.N, 8, False), (s.N, s.N + 1, 12, True)]
    if case == "cartpole_user_model_b5":
        os.environ.setdefault("ALTRO_HIP_ARCH", "gfx950")
        s = P.cartpole_move(make, A.register_model_source("cartpole", CARTPOLE), batch=5, goal=np.linspace(0.6, 1.2, 5))
        return s, s.solve, [(0, s.N, 2, False), (s.N, s.N + 1, 4, True)]
    raise KeyError(case)


def _snapshot(s):
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    return dict(X=X.copy(), U=U.copy(), K=K.copy(), d=d.copy(), lam=s.get_duals(), rho=s.get_penalties(), x0=s.get_initial_state(),
                stats=s.get_stats().copy(), opts=bytes(s.get_options()))


def _check_one_advance(s, cons, shift, w, before, after):
    N = s.N
    src = M.row_map(N, shift, cons) if cons else np.zeros(0, dtype=np.int32)
    assert len(src) == before["lam"].shape[1]
    Xn, Un, lam_n, rho_n = M.shifted(before["X"], before["U"], before["lam"], before["rho"], src, shift, M.reset_penalty(s))
    hold = np.minimum(np.arange(N) + shift, N - 1)
    for name, want in (("X", Xn), ("U", Un), ("K", before["K"][:, hold]), ("d", before["d"][:, hold]), ("lam", lam_n), ("rho", rho_n),
                       ("x0", before["X"][:, shift] + w)):
        assert np.array_equal(after[name], want), name
    assert after["stats"].tobytes() == before["stats"].tobytes() and after["opts"] == before["opts"]
    if cons:  # the terminal knot's rows stay
        p_term = s.num_constraints(N)
        assert p_term > 0 and np.array_equal(after["lam"][:, -p_term:], before["lam"][:, -p_term:])
        assert np.array_equal(after["rho"][:, -p_term:], before["rho"][:, -p_term:])


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 5, "N-1"])
@pytest.mark.parametrize("case", ["turn90_f64_b1", "turn90_f64_b300", "three_obstacles_f32_b300", "triple_integrator_b16",
                                  "quadrotor12_f32_b8", "cartpole_user_model_b5"])
def test_one_advance_is_the_numpy_statement(A, P, hip_make, case, shift):
    """Solve, snapshot X, U, K, d, lambda, rho, advance, read everything back: equal to the clamped-index statement; the new
    initial state is X_old[shift] + w; statistics, options and the terminal duals unchanged.  The host-array and the
    device-pointer variant give the same bits."""
    results = []
    for device in (False, True):
        s, solve, cons = _build(A, P, hip_make, case)
        sh = s.N - 1 if shift == "N-1" else shift
        solve()
        w = M.disturbance(1, s.batch, s.n)[0]
        before = _snapshot(s)
        if device:
            dw = DeviceArray(w)
            s.mpc_advance_device(sh, 0, dw.ptr)
            dw.free()
        else:
            s.mpc_advance(sh, w=w)
        after = _snapshot(s)
        _check_one_advance(s, cons, sh, w, before, after)
        with pytest.raises(A.AltroError) as e:  # the cost-to-go records belonged to the trajectory that has moved on
            s.get_ctg()
        assert f"({A.NOT_READY})" in str(e.value)
        results.append(after)
        s.close()
    for name in ("X", "U", "K", "d", "lam", "rho", "x0"):
        assert np.array_equal(results[0][name], results[1][name]), name


@pytest.mark.gpu
def test_given_initial_state_and_untouched_guess(A, P, hip_make):
    """x0 given ([n], [B][n], device pointer) replaces the plan's state; without w nothing is added; altro_reset_trajectory
    still restores the guess given through altro_set_trajectory."""
    s = P.batch_turn90(hip_make, 7)
    s.solve()
    X, _ = s.get_trajectory()
    s.mpc_advance(3)
    assert np.array_equal(s.get_initial_state(), X[:, 3])
    x1 = np.array([0.3, -0.2, 0.1])
    s.mpc_advance(1, x0=x1)
    assert np.array_equal(s.get_initial_state(), np.tile(x1, (7, 1)))
    xb, w = np.arange(21.0).reshape(7, 3) / 16, M.disturbance(1, 7, 3)[0]
    s.mpc_advance(2, x0=xb, w=w)
    assert np.array_equal(s.get_initial_state(), xb + w)
    dx, dw = DeviceArray(xb + 1.0), DeviceArray(w)
    s.mpc_advance_device(2, dx.ptr, dw.ptr)
    assert np.array_equal(s.get_initial_state(), xb + 1.0 + w)
    s.mpc_advance_device(2, dx.ptr, 0)
    assert np.array_equal(s.get_initial_state(), xb + 1.0)
    dx.free()
    dw.free()
    s.reset_trajectory()
    X0, U0 = s.get_trajectory()
    assert np.array_equal(U0, np.tile([0.1, 0.1], (7, s.N, 1))) and not X0.any()
    s.solve()  # ... and the handle solves on from the initial state the advance left
    assert np.array_equal(s.get_trajectory()[0][:, 0], xb + 1.0)


@pytest.mark.gpu
def test_mixed_problem_rows_start_afresh(A, P, hip_make):
    """The problem of tests/test_mpc_abi.py on the device: at shift 5 the circle's rows at knots 55 .. 59 start afresh --
    lambda = 0, rho = options.initial_penalty (or 1 when that is 0) -- and every other row moves."""
    s = M.mixed_problem(A, P, hip_make, batch=4)
    s.solve()
    assert s.num_constraints() == 552
    src = M.row_map(M.MIXED_N, 5, M.MIXED_CONS)
    fresh = np.nonzero(src < 0)[0]
    assert len(fresh) == 5
    for initial_penalty, want in ((3.0, 3.0), (0.0, 1.0)):
        s.set_options(initial_penalty=initial_penalty)
        before = _snapshot(s)
        assert (before["rho"][:, fresh] != want).all()  # (the solve raised them, and the last round's resets moved on)
        w = M.disturbance(1, 4, 3)[0]
        s.mpc_advance(5, w=w)
        after = _snapshot(s)
        _check_one_advance(s, M.MIXED_CONS, 5, w, before, after)
        assert (after["lam"][:, fresh] == 0).all() and (after["rho"][:, fresh] == want).all()
        s.update_penalties()  # (something other than the reset value in every row before the next round)
    assert np.isfinite(after["X"]).all() and np.isfinite(after["lam"]).all()


# ---- 5. closed loop: device advance against host-composed advance, bit for bit ----------------------------------------------
def _closed_loop(s, cons, W, device, set_penalties=True):
    """CYCLES x (solve; record; advance) -> per cycle (status, iterations_total, X, U, lambda, rho, x0 the cycle started from)"""
    src = M.row_map(s.N, SHIFT, cons)
    rec = []
    for c in range(CYCLES):
        x0 = s.get_initial_state() if device else None
        s.solve()
        st = s.get_stats()
        X, U = s.get_trajectory()
        rec.append(dict(status=st["status"].copy(), iterations=st["iterations_total"].copy(), X=X.copy(), U=U.copy(), lam=s.get_duals(),
                        rho=s.get_penalties(), x0=x0))
        if device:
            s.mpc_advance(SHIFT, w=W[c])
        else:
            M.host_advance(s, SHIFT, src, W[c], set_penalties=set_penalties)
    return rec


def _problem(A, P, make, problem, batch):
    if problem == "turn90":
        return P.batch_turn90(make, batch), M.TURN90_CONS(100)
    return P.batch_three_obstacles(make, batch, dtype=A.F32), M.THREE_OBSTACLES_CONS(100)


@pytest.mark.gpu
@pytest.mark.parametrize("initial_penalty", [0.0, 1.0])
@pytest.mark.parametrize("problem,batch", [("turn90", 8), ("turn90", 1024), ("turn90", 4608), ("three_obstacles", 512)])
def test_closed_loop_device_against_host_composed(A, P, hip_make, problem, batch, initial_penalty):
    """Two handles on the same problem, one after the other (equal engine paths): one advances on the device, the other through
    get_trajectory / get_duals / get_penalties -> numpy -> set_initial_state / set_trajectory / set_duals / set_penalties.
    The solver is deterministic across handles, so after every solve statuses, iteration counts, X, U, lambda and rho are equal
    bit for bit; a difference means the advance left device state behind that altro_set_trajectory resets."""
    W = M.disturbance(CYCLES, batch, 3)
    recs = []
    for device in (True, False):
        s, cons = _problem(A, P, hip_make, problem, batch)
        s.set_options(reset_duals=0, initial_penalty=initial_penalty)
        recs.append(_closed_loop(s, cons, W, device))
        s.close()
    for c, (dev, host) in enumerate(zip(*recs)):
        for name in ("status", "iterations", "X", "U", "lam", "rho"):
            assert np.array_equal(dev[name], host[name]), (c, name)
    warm = np.concatenate([r["iterations"][recs[0][0]["status"] == 0] for r in recs[0][1:]])
    print(f"{problem} x {batch}, initial_penalty {initial_penalty}: iterations of cycle 0 (max) {recs[0][0]['iterations'].max()}, "
          f"of the warm cycles (max over instances solved in cycle 0) {warm.max() if warm.size else '-'}")


# ---- 6. closed loop against the oracle ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_closed_loop_against_the_oracle(A, P, hip_make, oracle_make):
    """problems.batch_turn90, 16 instances, shift 5, six cycles, reset_duals = 0, initial_penalty = 1, the disturbance of
    _mpc_common.disturbance; the oracle's advance is composed on the host.  An instance is clean while it has ended kSolved in
    every cycle so far on the oracle; on clean instances status and iterations_total are exact and X, U agree to 1e-9 in every
    cycle, and at least 12 of the 16 are clean at the end (the oracle alone gives 15)."""
    B = 16
    W = M.disturbance(CYCLES, B, 3)
    g, cons = _problem(A, P, hip_make, "turn90", B)
    o, _ = _problem(A, P, oracle_make, "turn90", B)
    for s in (g, o):
        s.set_options(reset_duals=0, initial_penalty=1.0)
    rg = _closed_loop(g, cons, W, True)
    ro = _closed_loop(o, cons, W, False, set_penalties=False)  # (initial_penalty = 1: every solve sets the penalties itself)
    clean = np.ones(B, dtype=bool)
    for c in range(CYCLES):
        clean &= ro[c]["status"] == A.SOLVED
        print(f"cycle {c}: clean {int(clean.sum())}/{B}, oracle iterations max over clean {ro[c]['iterations'][clean].max()}, "
              f"max |X - X_oracle| {np.abs(rg[c]['X'][clean] - ro[c]['X'][clean]).max():.3g}, "
              f"max |U - U_oracle| {np.abs(rg[c]['U'][clean] - ro[c]['U'][clean]).max():.3g}")
        assert np.array_equal(rg[c]["status"][clean], ro[c]["status"][clean]), c
        assert np.array_equal(rg[c]["iterations"][clean], ro[c]["iterations"][clean]), c
        assert np.allclose(rg[c]["X"][clean], ro[c]["X"][clean], rtol=1e-9, atol=1e-9), c
        assert np.allclose(rg[c]["U"][clean], ro[c]["U"][clean], rtol=1e-9, atol=1e-9), c
    assert clean.sum() >= 12


# ---- 7. altro_mpc_run is the caller's own loop -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("problem,batch", [("turn90", 16), ("three_obstacles", 40)])
def test_mpc_run_is_the_python_loop(A, P, hip_make, problem, batch):
    W = M.disturbance(CYCLES, batch, 3)
    a, cons = _problem(A, P, hip_make, problem, batch)
    a.set_options(reset_duals=0, initial_penalty=0.0)
    rec = _closed_loop(a, cons, W, True)
    b, _ = _problem(A, P, hip_make, problem, batch)
    b.set_options(reset_duals=0, initial_penalty=0.0)
    out = b.mpc_run(CYCLES, SHIFT, W)
    fa, fb = _snapshot(a), _snapshot(b)
    for name in ("X", "U", "K", "d", "lam", "rho", "x0"):
        assert np.array_equal(fa[name], fb[name]), name
    assert fa["stats"].tobytes() == fb["stats"].tobytes()
    assert out["X_cl"].shape == (batch, CYCLES * SHIFT + 1, 3) and out["U_cl"].shape == (batch, CYCLES * SHIFT, 2)
    for c in range(CYCLES):
        assert np.array_equal(out["iterations"][:, c], rec[c]["iterations"]) and np.array_equal(out["status"][:, c], rec[c]["status"])
        rows = slice(c * SHIFT, (c + 1) * SHIFT)
        assert np.array_equal(out["X_cl"][:, rows], rec[c]["X"][:, :SHIFT]) and np.array_equal(out["U_cl"][:, rows], rec[c]["U"][:, :SHIFT])
        assert np.array_equal(out["X_cl"][:, c * SHIFT], rec[c]["x0"])  # the initial state cycle c was solved from
    assert np.array_equal(out["X_cl"][:, -1], fa["x0"])
    # without a disturbance, and with outputs the caller does not want
    lib = A.load_library()
    lib.altro_mpc_run.restype = int
    assert lib.altro_mpc_run(b._h, 2, 1, None, None, None, None, None) == A.OK
    a.close()
    b.close()


# ---- 8. an asynchronous solve owns the handle -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_advance_waits_for_the_asynchronous_solve(A, P, hip_make):
    ref = P.batch_turn90(hip_make, 64)
    ref.solve()
    s = P.batch_turn90(hip_make, 64)
    s.solve_async()
    for call in (lambda: s.mpc_advance(SHIFT), lambda: s.mpc_run(2, SHIFT), s.get_initial_state, lambda: s.mpc_row_map(1)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value)
    s.wait()
    assert s.get_stats().tobytes() == ref.get_stats().tobytes()
    for x, y in zip(s.get_trajectory(), ref.get_trajectory()):
        assert np.array_equal(x, y)
    s.mpc_advance(SHIFT)  # ... and is free again afterwards
    assert np.array_equal(s.get_initial_state(), ref.get_trajectory()[0][:, SHIFT])


# ---- 9. the facade ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_benchmark_mpc_driver(A, P, hip_make):
    """perf/benchmark_mpc: the kTurn90 loop through AugmentedLagrangianiLQR::AdvanceHorizon + Solve(); exits 0 (no warm cycle
    needs more iterations than the cold one) and, with --check, reports the iteration counts of the Python loop."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "perf"), "benchmark_mpc"])
    exe = os.path.join(ROOT, "perf", "benchmark_mpc")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(re.findall(r"^cycle \d+: solved \d+/16, iterations sum \d+ max \d+", r.stdout, re.M)) == 6
    B = 16
    r = subprocess.run([exe, str(CYCLES), str(B), str(SHIFT), "--check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {(int(c), int(b)): (int(it), int(st)) for c, b, it, st in re.findall(r"^iterations (\d+) (\d+) (\d+) (\d+)$", r.stdout, re.M)}
    assert len(got) == CYCLES * B
    s, cons = _problem(A, P, hip_make, "turn90", B)
    s.set_options(reset_duals=0)
    rec = _closed_loop(s, cons, M.disturbance(CYCLES, B, 3), True)
    for c in range(CYCLES):
        for b in range(B):
            assert got[(c, b)] == (rec[c]["iterations"][b], rec[c]["status"][b]), (c, b)
