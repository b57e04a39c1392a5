"""Multi-start on the device (include/altro_multistart.h): the selection on a real non-convex solve against the CPU oracle and
against the numpy statement of the rule, the spread / perturbation / best-start getters bit for bit against the getters of the
handle, altro_mpc_run_multistart against the caller's own loop, and the facade calls against the C calls.

Shapes: the 8 x 8 obstacle batch (N = 40) on which the oracle shows that the rule matters (problem 7: start 0 runs into the
inner-iteration limit, later starts solve; problem 3: the other way round); the triple integrator with P = 3, G = 5 (15
instances: no power of two, no multiple of the wavefront); kTurn90 with N = 24 at B = 1024 (G = 8) and B = 4608 (G = 9), handles
with shadow columns behind the batch that run every engine path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _mpc_common as M
import _multistart_common as MS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P8, G8, N8 = 8, 8, 40


# ---- device memory without torch: the HIP runtime the solver library has already loaded into this process ---------------
def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceBuffer:
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


# ---- the problems -------------------------------------------------------------------------------------------------------------
def _turn90(P, make, problems, starts, N=24, dtype=None):
    """kTurn90 with one goal per problem (the seeded goals of the config-2 batch); start g begins from the constant controls
    (0.1 + 0.05 g, 0.1 - 0.04 g)."""
    xf = np.repeat(P.batch_turn90_goals(problems), starts, axis=0)
    g = np.tile(np.arange(starts, dtype=np.float64), problems)
    u0 = np.stack([0.1 + 0.05 * g, 0.1 - 0.04 * g], axis=1)
    kw = {} if dtype is None else dict(dtype=dtype)
    return P.unicycle_turn90(make, batch=problems * starts, N=N, xf=xf, u0=u0, **kw)


def _triple(P, make, problems=3, starts=5, N=10):
    xf = np.repeat(P.batch_triple_integrator_goals(problems), starts, axis=0)
    s = P.triple_integrator(make, batch=problems * starts, N=N, constraints=True, xf=xf)
    g = np.tile(np.arange(starts, dtype=np.float64), problems)
    s.set_trajectory(None, np.repeat(np.stack([0.3 * g, -0.2 * g], axis=1)[:, None, :], N, axis=1))
    return s


def _build(A, P, make, case):
    """-> (solver, problems, starts)"""
    if case == "obstacles_f64":
        return MS.obstacle_batch(P, make, P8, G8, N8), P8, G8
    if case == "obstacles_f32":
        return MS.obstacle_batch(P, make, P8, G8, N8, dtype=A.F32), P8, G8
    if case == "triple_3x5":
        return _triple(P, make), 3, 5
    if case == "turn90_128x8":
        return _turn90(P, make, 128, 8), 128, 8
    if case == "turn90_512x9":
        return _turn90(P, make, 512, 9), 512, 9
    raise KeyError(case)


def _snapshot(s):
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    return dict(X=X.copy(), U=U.copy(), K=K.copy(), d=d.copy(), lam=s.get_duals(), rho=s.get_penalties(), cval=s.get_constraint_values(),
                costs=s.get_knot_costs(), x0=s.get_initial_state(), stats=s.get_stats().copy())


COLUMN = ("X", "U", "K", "d", "lam", "rho", "cval", "costs")  # what a spread copies


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _winner_columns(win, starts):
    """instance -> the column of its problem's winner"""
    return np.repeat(np.arange(len(win)) * starts + win, starts)


# ---- 1. the selection on a real solve --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_stats(P, oracle_make):
    o = MS.obstacle_batch(P, oracle_make, P8, G8, N8)
    o.solve()
    st = o.get_stats().copy()
    o.close()
    return st


def test_the_oracle_inputs_exercise_the_rule(oracle_stats):
    solved = (oracle_stats["status"] == MS.SOLVED).reshape(P8, G8)
    assert not solved[7, 0] and solved[7].any()  # problem 7: start 0 does not solve, a later start does
    assert solved[3, 0] and not solved[3].all()  # problem 3: start 0 solves, another start does not
    win = MS.rule_winners(oracle_stats, G8)
    assert win[7] != 0 and solved[np.arange(P8), win].all()


def test_selection_on_the_obstacle_batch_fp64(P, hip_make, oracle_stats):
    s = MS.obstacle_batch(P, hip_make, P8, G8, N8)
    s.solve()
    sg, so = s.get_stats(), oracle_stats
    # the project's fp64 bar: schedules are exact
    assert np.array_equal(sg["status"], so["status"]), (sg["status"].reshape(P8, G8), so["status"].reshape(P8, G8))
    assert np.array_equal(sg["iterations_total"], so["iterations_total"])
    before = _snapshot(s)
    win = s.multistart_select(G8)
    assert win.dtype == np.int32 and win.shape == (P8,)
    assert np.array_equal(win, MS.rule_winners(sg, G8)), (win, MS.rule_winners(sg, G8))  # index for index
    wo = MS.rule_winners(so, G8)
    cg, co = np.arange(P8) * G8 + win, np.arange(P8) * G8 + wo
    assert np.array_equal(sg["status"][cg], so["status"][co])
    # costs, not indices, against the oracle (several problems have starts that tie to rounding); the bar is the one
    # tests/test_parity_gpu.py applies to the cost of solved instances of this problem against the oracle
    print("winner cost, GPU against oracle: max rel", np.max(np.abs(sg["cost"][cg] - so["cost"][co]) / np.abs(so["cost"][co])))
    assert np.allclose(sg["cost"][cg], so["cost"][co], rtol=1e-10, atol=0.0)
    # select changes nothing on the handle
    after = _snapshot(s)
    for name in COLUMN + ("x0",):
        assert _same(before[name], after[name]), name
    assert before["stats"].tobytes() == after["stats"].tobytes()
    # the device form gives the same winners
    dw = DeviceBuffer(4 * P8)
    s.multistart_select_device(G8, dw.ptr)
    assert np.array_equal(dw.read(np.int32, (P8,)), win)
    dw.free()
    # starts = 1: every instance is its own problem; starts = B: one problem
    assert np.array_equal(s.multistart_select(1), np.zeros(P8 * G8, dtype=np.int32))
    assert s.multistart_select(P8 * G8)[0] == MS.rule_winner(sg["status"], sg["cost"], sg["violation"])
    s.close()


def test_selection_on_the_obstacle_batch_f32(A, P, hip_make):
    """ALTRO_F32 (fp32 records): no oracle twin of the schedule, the rule against the GPU's own statistics only."""
    s = MS.obstacle_batch(P, hip_make, P8, G8, N8, dtype=A.F32)
    s.solve()
    sg = s.get_stats()
    for G in (G8, 4, 16):
        assert np.array_equal(s.multistart_select(G), MS.rule_winners(sg, G)), G
    s.close()


# ---- 2. the spread -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["obstacles_f64", "obstacles_f32", "triple_3x5", "turn90_128x8", "turn90_512x9"])
def test_spread_copies_the_winner_column(A, P, hip_make, case):
    s, problems, starts = _build(A, P, hip_make, case)
    s.solve()
    before = _snapshot(s)
    want = MS.rule_winners(before["stats"], starts)
    win = s.multistart_spread(starts)
    assert np.array_equal(win, want)
    if case.startswith("obstacles"):
        assert len(set(win.tolist())) > 1  # (a spread that always copied start 0 would not pass)
    src = _winner_columns(win, starts)
    after = _snapshot(s)
    for name in COLUMN:
        assert _same(after[name], before[name][src]), name
    assert after["lam"].shape[1] > 0 and _same(after["x0"], before["x0"])
    assert after["stats"].tobytes() == before["stats"].tobytes()  # statistics stay per start
    with pytest.raises(A.AltroError) as e:  # as behind altro_set_trajectory: no cost-to-go replay
        s.get_ctg()
    assert f"({A.NOT_READY})" in str(e.value)
    # a second spread selects from the unchanged statistics and finds nothing to do; the device form, with and without winners
    dw = DeviceBuffer(4 * problems)
    s.multistart_spread_device(starts, dw.ptr)
    assert np.array_equal(dw.read(np.int32, (problems,)), win)
    dw.free()
    s.multistart_spread_device(starts)
    again = _snapshot(s)
    for name in COLUMN:
        assert _same(again[name], after[name]), name
    # the warm re-solve equals the one of a second handle that got the same state from the host
    t, _, _ = _build(A, P, hip_make, case)
    t.solve()
    t.set_trajectory(before["X"][src], before["U"][src])
    t.set_duals(before["lam"][src])
    t.set_penalties(before["rho"][src])
    for h in (s, t):
        h.set_options(reset_duals=0, initial_penalty=0.0)
        h.solve()
    ss, st = s.get_stats(), t.get_stats()
    assert np.array_equal(ss["status"], st["status"]) and np.array_equal(ss["iterations_total"], st["iterations_total"])
    for x, y in zip(s.get_trajectory(), t.get_trajectory()):
        assert _same(x, y)
    s.close()
    t.close()


def test_spread_with_one_start_is_a_no_op(A, P, hip_make):
    s, _, _ = _build(A, P, hip_make, "triple_3x5")
    s.solve()
    before = _snapshot(s)
    assert np.array_equal(s.multistart_spread(1), np.zeros(15, dtype=np.int32))
    after = _snapshot(s)
    for name in COLUMN + ("x0",):
        assert _same(before[name], after[name]), name
    s.close()


_POISON_SCRIPT = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import __graft_entry__ as graft
A = graft.load_package()
P = importlib.import_module("altro_cpp_amd.problems")
import test_multistart_gpu as T
s, problems, starts = T._build(A, P, P.make_hip, "turn90_128x8")
s.solve()
win = s.multistart_spread(starts)
s.set_options(reset_duals=0, initial_penalty=0.0)
s.solve()
X, U = s.get_trajectory()
np.savez(sys.argv[1], win=win, X=X, U=U, it=s.get_stats()["iterations_total"], lam=s.get_duals())
"""


def test_spread_needs_nothing_behind_the_batch(tmp_path):
    """Solve, spread, warm re-solve at B = 1024 (a handle with shadow columns) in two fresh processes, one of them with
    ALTRO_HIP_DEBUG_POISON: shadow columns filled with a pattern.  Identical: nothing beyond column B - 1 is needed."""
    def run(tag, env_extra):
        out = str(tmp_path / f"{tag}.npz")
        subprocess.run([sys.executable, "-c", _POISON_SCRIPT % (ROOT, os.path.join(ROOT, "tests")), out], check=True,
                       env=dict(os.environ, **env_extra), timeout=600)
        return np.load(out)

    ref, poisoned = run("default", {}), run("poisoned", {"ALTRO_HIP_DEBUG_POISON": "1"})
    for name in ("win", "X", "U", "it", "lam"):
        assert _same(ref[name], poisoned[name]), name


# ---- 3. the perturbation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["triple_3x5", "turn90_128x8"])
def test_perturb_is_a_plain_addition(A, P, hip_make, case):
    s, problems, starts = _build(A, P, hip_make, case)
    s.solve()
    rng = np.random.default_rng(7)
    B, N, m = s.batch, s.N, s.m
    before = _snapshot(s)
    U = before["U"]
    # one block per start, shared by all problems
    dU = rng.standard_normal((starts, N, m)) * 0.1
    s.multistart_perturb(starts, dU)
    U = U + np.tile(dU, (problems, 1, 1))
    assert _same(s.get_trajectory()[1], U)
    # per instance, host and device pointer
    dB = rng.standard_normal((B, N, m)) * 0.1
    s.multistart_perturb(starts, dB)
    U = U + dB
    assert _same(s.get_trajectory()[1], U)
    dd = DeviceBuffer(dB.nbytes, dB)
    s.multistart_perturb_device(starts, dd.ptr, True)
    U = U + dB
    assert _same(s.get_trajectory()[1], U)
    dd.free()
    dd = DeviceBuffer(dU.nbytes, dU)
    s.multistart_perturb_device(starts, dd.ptr, False)
    U = U + np.tile(dU, (problems, 1, 1))
    assert _same(s.get_trajectory()[1], U)
    dd.free()
    after = _snapshot(s)
    for name in ("X", "K", "d", "lam", "rho", "cval", "costs", "x0"):
        assert _same(before[name], after[name]), name
    assert before["stats"].tobytes() == after["stats"].tobytes()
    with pytest.raises(A.AltroError) as e:
        s.get_ctg()
    assert f"({A.NOT_READY})" in str(e.value)
    s.close()
    # it needs no finished solve
    t, _, _ = _build(A, P, hip_make, case)
    U0 = t.get_trajectory()[1]
    t.multistart_perturb(starts, dU)
    assert _same(t.get_trajectory()[1], U0 + np.tile(dU, (problems, 1, 1)))
    t.close()


# ---- 4. the best starts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["obstacles_f32", "triple_3x5", "turn90_128x8"])
def test_get_best_is_the_winner_rows(A, P, hip_make, case):
    s, problems, starts = _build(A, P, hip_make, case)
    s.solve()
    X, U = s.get_trajectory()
    stats = s.get_stats()
    win = MS.rule_winners(stats, starts)
    col = np.arange(problems) * starts + win
    best = s.multistart_get_best(starts)
    assert np.array_equal(best["winner"], win)
    assert _same(best["X"], X[col]) and _same(best["U"], U[col])
    assert best["stats"].tobytes() == stats[col].tobytes()
    bufs = dict(X=DeviceBuffer(best["X"].nbytes), U=DeviceBuffer(best["U"].nbytes), st=DeviceBuffer(best["stats"].nbytes),
                win=DeviceBuffer(best["winner"].nbytes))
    s.multistart_get_best_device(starts, bufs["X"].ptr, bufs["U"].ptr, bufs["st"].ptr, bufs["win"].ptr)
    assert bufs["X"].read(np.float64, best["X"].shape).tobytes() == best["X"].tobytes()
    assert bufs["U"].read(np.float64, best["U"].shape).tobytes() == best["U"].tobytes()
    assert bufs["st"].read(A.STATS_DTYPE, (problems,)).tobytes() == best["stats"].tobytes()
    assert np.array_equal(bufs["win"].read(np.int32, (problems,)), win)
    for b in bufs.values():
        b.free()
    # every pointer may be NULL, but not all of them
    lib = A.load_library()
    lib.altro_multistart_get_best.restype = ctypes.c_int
    only_u = np.zeros_like(best["U"])
    assert lib.altro_multistart_get_best(s._h, starts, None, only_u.ctypes.data_as(ctypes.c_void_p), None, None) == A.OK
    assert _same(only_u, best["U"])
    assert lib.altro_multistart_get_best(s._h, starts, None, None, None, None) == A.INVALID_ARG
    assert _same(s.get_trajectory()[0], X) and s.get_stats().tobytes() == stats.tobytes()
    s.close()


def test_an_asynchronous_solve_owns_the_handle(A, P, hip_make):
    s, _, starts = _build(A, P, hip_make, "triple_3x5")
    s.solve_async()
    for call in (lambda: s.multistart_select(starts), lambda: s.multistart_spread(starts), lambda: s.multistart_get_best(starts),
                 lambda: s.multistart_perturb(starts, np.zeros((starts, s.N, s.m))), lambda: s.mpc_run_multistart(starts, 2, 1)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value)
    s.wait()
    assert len(s.multistart_select(starts)) == 3  # (the solve behind altro_wait counts as finished)
    s.close()


# ---- 5. the loop ---------------------------------------------------------------------------------------------------------------
CYCLES, SHIFT = 4, 5


@pytest.mark.parametrize("case", ["obstacles_f32", "turn90_128x8"])
def test_mpc_run_multistart_is_the_callers_loop(A, P, hip_make, case):
    a, problems, starts = _build(A, P, hip_make, case)
    b, _, _ = _build(A, P, hip_make, case)
    B, N, n, m = a.batch, a.N, a.n, a.m
    W = np.repeat(M.disturbance(CYCLES, problems, n), starts, axis=1)  # one disturbance per problem, repeated per start
    g = np.arange(starts, dtype=np.float64)
    dU = np.broadcast_to(np.stack([0.02 * g, -0.03 * g], axis=1)[:, None, :], (starts, N, m)).copy()
    for h in (a, b):
        h.set_options(reset_duals=0, initial_penalty=0.0)
    rec = []
    for c in range(CYCLES):  # the caller's loop over the separate entry points
        a.solve()
        st = a.get_stats()
        win = a.multistart_spread(starts)
        X, U = a.get_trajectory()
        rec.append(dict(it=st["iterations_total"].copy(), status=st["status"].copy(), win=win, X=X.copy(), U=U.copy(),
                        x0=a.get_initial_state()))
        a.mpc_advance(SHIFT, w=W[c])
        a.multistart_perturb(starts, dU)
    out = b.mpc_run_multistart(starts, CYCLES, SHIFT, w=W, dU=dU)
    fa, fb = _snapshot(a), _snapshot(b)
    for name in ("X", "U", "K", "d", "lam", "rho", "x0"):
        assert _same(fa[name], fb[name]), name
    assert fa["stats"].tobytes() == fb["stats"].tobytes()
    assert out["winner"].shape == (problems, CYCLES) and out["X_cl"].shape == (B, CYCLES * SHIFT + 1, n)
    for c in range(CYCLES):
        assert np.array_equal(out["iterations"][:, c], rec[c]["it"]) and np.array_equal(out["status"][:, c], rec[c]["status"])
        assert np.array_equal(out["winner"][:, c], rec[c]["win"]), c
        rows = slice(c * SHIFT, (c + 1) * SHIFT)
        assert _same(out["X_cl"][:, rows], rec[c]["X"][:, :SHIFT]) and _same(out["U_cl"][:, rows], rec[c]["U"][:, :SHIFT])
        assert _same(out["X_cl"][:, c * SHIFT], rec[c]["x0"])
    assert _same(out["X_cl"][:, -1], fa["x0"])
    # after a spread the starts of a problem log identical rows: every G-th row is the problem's
    Xl = out["X_cl"].reshape(problems, starts, -1, n)
    assert (Xl == Xl[:, :1]).all()
    # per-instance perturbations, no disturbance, outputs the caller does not want
    lib = A.load_library()
    lib.altro_mpc_run_multistart.restype = ctypes.c_int
    dB = np.tile(dU, (problems, 1, 1))
    for h, per in ((a, 1), (b, 0)):
        d = dB if per else dU
        assert lib.altro_mpc_run_multistart(h._h, starts, 2, 1, None, d.ctypes.data_as(ctypes.c_void_p), per, None, None, None, None,
                                            None) == A.OK
    for x, y in zip(a.get_trajectory(), b.get_trajectory()):
        assert _same(x, y)
    a.close()
    b.close()


# ---- 6. the facade -------------------------------------------------------------------------------------------------------------
def test_facade_calls_give_the_c_calls_bits(A, P, hip_make, tmp_path):
    """tests/cpp/multistart_facade_driver.cpp: altro::problems::UnicycleProblem (kTurn90, N = 24) with 3 problems x 4 starts
    through the facade -- Solve, SelectStarts, GetBestStarts, PerturbControls, SpreadBestStart -- printing winners and every
    state and control as hexadecimal floats; the C calls on the same inputs give the same bits."""
    problems, starts, N = 3, 4, 24
    B = problems * starts
    exe = str(tmp_path / "multistart_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "multistart_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    xf = np.repeat(P.batch_turn90_goals(problems), starts, axis=0)
    g = np.tile(np.arange(starts, dtype=np.float64), problems)
    u0 = np.stack([0.1 + 0.05 * g, 0.1 - 0.04 * g], axis=1)
    dU = np.random.default_rng(3).standard_normal((starts, N, 2)) * 0.05
    path = str(tmp_path / "inputs.bin")
    np.concatenate([xf.ravel(), u0.ravel(), dU.ravel()]).tofile(path)
    r = subprocess.run([exe, path, str(problems), str(starts), str(N)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = {tag: dict(x=np.full((B if tag != "best" else problems, N + 1, 3), np.nan), u=np.full((B if tag != "best" else problems, N, 2), np.nan))
           for tag in ("best", "perturbed", "spread")}
    winners = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] in ("select", "bestwin", "spreadwin"):
            winners[f[0]] = [int(v) for v in f[1:]]
        elif f[0] in got:
            got[f[0]][f[1]][int(f[2]), int(f[3])] = [float.fromhex(v) for v in f[4:]]
    s = P.unicycle_turn90(hip_make, batch=B, N=N, xf=xf, u0=u0)
    s.solve()
    win = s.multistart_select(starts)
    assert winners["select"] == win.tolist() == winners["bestwin"] == winners["spreadwin"]
    best = s.multistart_get_best(starts)
    assert _same(got["best"]["x"], best["X"]) and _same(got["best"]["u"], best["U"])
    s.multistart_perturb(starts, dU)
    X, U = s.get_trajectory()
    assert _same(got["perturbed"]["x"], X) and _same(got["perturbed"]["u"], U)
    s.multistart_spread(starts)
    X, U = s.get_trajectory()
    assert _same(got["spread"]["x"], X) and _same(got["spread"]["u"], U)
    s.close()
