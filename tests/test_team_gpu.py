"""Teams on the device (include/altro_team.h): the fill against the numpy gather, bit for bit; the per-track base and the
window under the receding-horizon advance; a solve behind a device fill against a solve behind the same rows sent from the
host; every round against the CPU oracle given one ordinary circle per knot; the behaviour the exchange is for; the
clearance; the two loops against the caller's own; the facade.  The numpy statements are tests/_team_common.py's."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _ledger
import _mpc_common as M
import _team_common as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24
RTOL, ATOL = 1e-7, 1e-9  # tests/test_knot_params_gpu.py::_compare_with_oracle


def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceBuffer:
    """`count` doubles of device memory (hipMalloc / hipMemcpy through ctypes)."""

    def __init__(self, count):
        self.hip, self.count = _hip_runtime(), count
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(8 * count)) == 0
        self.ptr = p.value

    def get(self):
        out = np.empty(self.count)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(8 * self.count),
                                  ctypes.c_int(2)) == 0  # device to host
        return out

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


def _bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# (teams, agents, N, model, dtype, knots of the circle)
SHAPES = {
    "smallest_3x2": (3, 2, 12, "unicycle", "F64", None),
    "straddle_13x5": (13, 5, 24, "unicycle", "F64", None),
    "tripleint_2x3": (2, 3, 10, "tripleint", "F64", None),
    "chains_700x3_f32": (700, 3, 24, "unicycle", "F32", None),
    "terminal_row_2x4": (2, 4, 12, "unicycle", "F64", "all"),
}


def _shape_handle(A, P, make, name):
    """A handle of the shape with the team circle registered and a trajectory of random states on the device."""
    T, Ag, n_knots, model, dtype, knots = SHAPES[name]
    B, np_ = T * Ag, 3 * (Ag - 1)
    if model == "unicycle" and knots is None:
        s = P.team_ring(make, T, Ag, N=n_knots, dtype=getattr(A, dtype))
        idx, kb, ke = s.team_circle, 1, n_knots
    else:
        kb, ke = (0, n_knots + 1) if knots == "all" else (1, n_knots)
        s = (P.unicycle_turn90(make, batch=B, N=n_knots, constraints=False) if model == "unicycle"
             else P.triple_integrator(make, batch=B, N=n_knots, dtype=getattr(A, dtype)))
        idx = s.add_knot_constraint(A.CON_CIRCLE, kb, ke, np_)
        s.set_constraint_track(idx, np.zeros((1, np_)))
    rng = np.random.default_rng(11)
    X = rng.standard_normal((B, n_knots + 1, s.n))
    U = rng.standard_normal((B, n_knots, s.m)) * 0.1
    s.set_trajectory(X, U)
    return s, idx, kb, ke


# ---- 1. the fill, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_fill_is_the_numpy_gather(A, P, hip_make, name):
    s, idx, kb, ke = _shape_handle(A, P, hip_make, name)
    T, Ag = SHAPES[name][:2]
    B = T * Ag
    X, U = s.get_trajectory()
    before = dict(X=X, U=U, lam=s.get_duals(), rho=s.get_penalties(), stats=s.get_stats(), x0=s.get_initial_state())
    shared = 0.1 + 0.02 * np.arange(Ag)
    per = 0.05 + 0.001 * (np.arange(B) % 37)
    for mode in (A.TEAM_ALL, A.TEAM_PRIORITY):
        for rad in (shared, per):
            s.team_fill_tracks(Ag, idx, rad, mode)
            got = s.get_knot_params(idx)
            want = TC.fill_rows(X, Ag, rad, mode)[:, kb:ke]
            assert _bits(got, want), (name, mode, rad.shape, np.abs(got - want).max())
    X2, U2 = s.get_trajectory()
    after = dict(X=X2, U=U2, lam=s.get_duals(), rho=s.get_penalties(), stats=s.get_stats(), x0=s.get_initial_state())
    _same(before, after, "a fill changes nothing but the track")
    s.close()


# ---- 2. the base of a track and the window ----------------------------------------------------------------------------------------
def test_base_and_window(A, P, hip_make):
    T, Ag, B = 3, 2, 6
    rows_b = N + 13
    s = P.team_ring(hip_make, T, Ag, N=N)
    idx, rad = s.team_circle, s.team_radius
    bound_track = P.ramped_bound_track(B, rows_b)
    bound = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 4)
    s.set_constraint_track(bound, bound_track)
    s.set_track_offset(7)
    win = lambda off: bound_track[:, np.minimum(off + np.arange(N), rows_b - 1)]  # noqa: E731
    s.solve()
    bound_before = s.get_knot_params(bound)
    assert _bits(bound_before, win(7))
    X, _ = s.get_trajectory()
    s.team_fill_tracks(Ag, idx, rad)
    rows = TC.fill_rows(X, Ag, rad)
    assert _bits(s.get_knot_params(idx), rows[:, 1:N])
    assert _bits(s.get_knot_params(bound), bound_before) and s.get_track_offset() == 7
    # the advance: the team's window shows the former plans at min(k + 3, N), the bound's track has moved to offset 10
    s.mpc_advance(3, w=M.disturbance(1, B, 3)[0])
    assert s.get_track_offset() == 10
    assert _bits(s.get_knot_params(idx), TC.window(rows, 3)[:, 1:N])
    assert _bits(s.get_knot_params(bound), win(10))
    # a blended fill behind the advance and the next solve: the windowed old rows with the new plans
    s.solve()
    X2, _ = s.get_trajectory()
    new = TC.fill_rows(X2, Ag, rad)
    s.team_fill_tracks(Ag, idx, rad, A.TEAM_ALL, 0.5)
    mixed = TC.blend_rows(TC.window(rows, 3), new, 0.5)
    assert _bits(s.get_knot_params(idx), mixed[:, 1:N])
    assert not _bits(mixed, new)
    assert _bits(s.get_knot_params(bound), win(10)) and s.get_track_offset() == 10
    # its base is the offset of the fill: one more advance shows ITS rows one knot on
    s.mpc_advance(1)
    assert _bits(s.get_knot_params(idx), TC.window(mixed, 1)[:, 1:N]) and _bits(s.get_knot_params(bound), win(11))
    # blend = 1 is a bit copy again
    X3, _ = s.get_trajectory()
    s.team_fill_tracks(Ag, idx, rad, A.TEAM_PRIORITY, 1.0)
    assert _bits(s.get_knot_params(idx), TC.fill_rows(X3, Ag, rad, A.TEAM_PRIORITY)[:, 1:N])
    # altro_set_constraint_track as before: base 0 (offset 11 of a 5-row track: its last row), and no longer a team's track
    own = np.random.default_rng(5).standard_normal((B, 5, 3))
    s.set_constraint_track(idx, own)
    assert _bits(s.get_knot_params(idx), np.repeat(own[:, 4:5], N - 1, axis=1))
    s.team_fill_tracks(Ag, idx, rad, A.TEAM_ALL, 0.5)
    assert _bits(s.get_knot_params(idx), TC.fill_rows(X3, Ag, rad)[:, 1:N])
    s.close()


# ---- 3. a solve behind the device fill is a solve behind the same rows from the host -----------------------------------------------
def _fill_then_solve(A, P, make, T, Ag, on_device):
    s = P.team_ring(make, T, Ag, N=N)
    s.solve()
    if on_device:
        s.team_fill_tracks(Ag, s.team_circle, s.team_radius)
    else:
        s.set_constraint_track(s.team_circle, TC.fill_rows(s.get_trajectory()[0], Ag, s.team_radius))
    s.solve()
    out = _state(s)
    s.close()
    return out


_DEVICE_FILL = {}


@pytest.mark.parametrize("T,Ag", [(3, 2), (700, 3)])
def test_solve_equals_host_composition(A, P, hip_make, T, Ag):
    a = _fill_then_solve(A, P, hip_make, T, Ag, True)
    b = _fill_then_solve(A, P, hip_make, T, Ag, False)
    _DEVICE_FILL[(T, Ag)] = a
    print(f"B {T * Ag}: iterations {np.unique(a['stats']['iterations_total'])}, statuses {np.unique(a['stats']['status'])}")
    _same(a, b, f"device fill against host rows, B {T * Ag}")


_POISON_SCRIPT = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import __graft_entry__ as graft
A = graft.load_package()
P = importlib.import_module("altro_cpp_amd.problems")
import test_team_gpu as T
np.savez(sys.argv[1], **T._fill_then_solve(A, P, P.make_hip, 700, 3, True))
"""


def test_fill_needs_nothing_behind_the_batch(A, P, hip_make, tmp_path):
    """B = 2100 (shadow columns) in a fresh process with ALTRO_HIP_DEBUG_POISON: the same bits."""
    ref = _DEVICE_FILL.get((700, 3)) or _fill_then_solve(A, P, hip_make, 700, 3, True)
    out = str(tmp_path / "poisoned.npz")
    subprocess.run([sys.executable, "-c", _POISON_SCRIPT % (ROOT, os.path.join(ROOT, "tests")), out], check=True,
                   env=dict(os.environ, ALTRO_HIP_DEBUG_POISON="1"), timeout=600)
    got = np.load(out)
    _same(ref, got, "poisoned shadow columns")


# ---- 4. the oracle, round by round ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [TC.CASES[0], TC.CASES[5]], ids=TC.case_id)
def test_every_round_against_the_oracle(A, P, oracle_make, hip_make, case):
    """Each round the oracle gets the device's own parameters (get_knot_params) and pre-solve controls as one ordinary circle
    per knot, so errors cannot compound: statuses and iteration counts exact, X and U to 1e-7 relative + 1e-9."""
    T, Ag, mode, blend, rounds = case
    B = T * Ag
    g = P.team_ring(hip_make, T, Ag, N=N)
    idx, rad = g.team_circle, g.team_radius
    g.solve()
    for r in range(rounds):
        g.team_fill_tracks(Ag, idx, rad, mode, blend)
        rows = np.zeros((B, N + 1, 3 * (Ag - 1)))
        rows[:, 1:N] = g.get_knot_params(idx)
        o = P.team_ring(oracle_make, T, Ag, N=N, per_knot_track=rows, U=g.get_trajectory()[1])
        o.solve()
        g.solve()
        so, sg = o.get_stats(), g.get_stats()
        print(f"round {r}: iterations {so['iterations_total'].tolist()}, statuses {np.unique(so['status'])}")
        for f in ("status", "iterations_total", "iterations_outer"):
            assert (so[f] == sg[f]).all(), (r, f, so[f], sg[f])
        Xo, Uo = o.get_trajectory()
        Xg, Ug = g.get_trajectory()
        _ledger.close(Xg, Xo, RTOL, ATOL, "X")
        _ledger.close(Ug, Uo, RTOL, ATOL, "U")
        o.close()
    g.close()


# ---- 5. what the exchange is for -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_teams_stop_colliding(A, P, hip_make, case):
    """On the device's own plans the bars tests/test_team_oracle.py pins on the oracle: uncoupled <= -0.03, coupled >= -2e-3 in
    distance units, every instance solved."""
    T, Ag, mode, blend, rounds = case
    s = P.team_ring(hip_make, T, Ag, N=N)
    s.solve()
    unc = TC.distance_clearance(s.get_trajectory()[0], Ag, s.team_radius, 1, N)
    s.team_solve(Ag, s.team_circle, s.team_radius, mode, blend, rounds)
    cpl = TC.distance_clearance(s.get_trajectory()[0], Ag, s.team_radius, 1, N)
    st = s.get_stats()
    print(f"{TC.case_id(case)}: uncoupled {unc}, coupled {cpl}, statuses {np.unique(st['status'])}")
    assert (unc <= TC.UNCOUPLED_BAR).all(), unc
    assert (st["status"] == A.SOLVED).all(), st["status"]
    assert (cpl >= TC.COUPLED_BAR).all(), cpl
    # the device's own clearance says the same in squared units: negative exactly when the distance form is
    sq = s.team_clearance(Ag, s.team_circle, s.team_radius)
    assert ((sq < 0) == (cpl < 0)).all()
    s.close()


# ---- 6. the clearance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["straddle_13x5", "chains_700x3_f32"])
def test_clearance_is_the_numpy_minimum(A, P, hip_make, name):
    s, idx, kb, ke = _shape_handle(A, P, hip_make, name)
    T, Ag = SHAPES[name][:2]
    B = T * Ag
    X, U = s.get_trajectory()
    X[:, :, :2] *= 3.0  # (spread out: most teams clear ...)
    X[Ag + 1, 5, :2] = X[Ag, 5, :2] + 0.01  # (... and team 1 made to overlap)
    s.set_trajectory(X, U)
    shared = 0.1 + 0.02 * np.arange(Ag)
    per = 0.05 + 0.001 * (np.arange(B) % 37)
    s.team_fill_tracks(Ag, idx, shared, A.TEAM_PRIORITY)  # every pair counts whatever the mode of the last fill
    dev = DeviceBuffer(T)
    for rad in (shared, per):
        want = TC.clearance(X, Ag, rad, kb, ke)
        assert want[1] < 0 and (want > 0).any()
        assert _bits(s.team_clearance(Ag, idx, rad), want), rad.shape
        s.team_clearance_device(Ag, idx, rad, dev.ptr)
        assert _bits(dev.get(), want), rad.shape
    dev.free()
    X2, U2 = s.get_trajectory()
    assert _bits(X2, X) and _bits(U2, U)
    s.close()


# ---- 7. the loops ----------------------------------------------------------------------------------------------------------------
def test_team_solve_is_the_callers_loop(A, P, hip_make):
    T, Ag = 3, 2
    a, b = P.team_ring(hip_make, T, Ag, N=N), P.team_ring(hip_make, T, Ag, N=N)
    for s in (a, b):
        s.solve()
    TC.team_solve_loop(a, Ag, a.team_circle, a.team_radius, A.TEAM_ALL, 0.5, 3)
    b.team_solve(Ag, b.team_circle, b.team_radius, A.TEAM_ALL, 0.5, 3)
    _same(_state(a), _state(b), "altro_team_solve")
    assert _bits(a.get_knot_params(a.team_circle), b.get_knot_params(b.team_circle))
    a.close()
    b.close()


def test_mpc_run_team_is_the_callers_loop(A, P, hip_make):
    T, Ag, cycles, shift, rounds = 3, 2, 4, 3, 2
    B = T * Ag
    a, b = P.team_ring(hip_make, T, Ag, N=N), P.team_ring(hip_make, T, Ag, N=N)
    W = 0.1 * M.disturbance(cycles, B, 3)  # 1e-3
    for s in (a, b):
        s.set_options(reset_duals=0, initial_penalty=0.0)
        s.solve()
    want = TC.mpc_team_loop(a, Ag, a.team_circle, a.team_radius, A.TEAM_ALL, 0.5, rounds, cycles, shift, W)
    got = b.mpc_run_team(Ag, b.team_circle, b.team_radius, A.TEAM_ALL, 0.5, rounds, cycles, shift, w=W)
    print("clearance per team and cycle:\n", got["clear"], "\nstatuses", np.unique(got["status"]))
    assert got["clear"].shape == (T, cycles) and got["X_cl"].shape == (B, cycles * shift + 1, 3)
    for name in ("X_cl", "U_cl", "iterations", "status", "clear"):
        assert _bits(got[name], want[name]), name
    _same(_state(a), _state(b), "altro_mpc_run_team")
    assert _bits(a.get_knot_params(a.team_circle), b.get_knot_params(b.team_circle))
    assert a.get_track_offset() == b.get_track_offset() == cycles * shift
    a.close()
    b.close()


# ---- 8. the facade ---------------------------------------------------------------------------------------------------------------
def test_facade_gives_the_c_calls_bits(A, P, hip_make, tmp_path):
    """tests/cpp/team_facade_driver.cpp: Solve, TeamClearance, FillTeamTracks, SolveTeam on the ring with kTurn90's constraints,
    printing hexadecimal floats; the C calls on the same inputs give the same bits."""
    T, Ag, rounds = 2, 3, 3
    B = T * Ag
    exe = str(tmp_path / "team_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "team_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    x0, xf = P.team_ring_states(T, Ag)
    rad = np.full(Ag, P.TEAM_RING_RADIUS)
    path = str(tmp_path / "inputs.bin")
    np.concatenate([x0.ravel(), xf.ravel(), rad]).tofile(path)
    r = subprocess.run([exe, path, str(T), str(Ag), str(N), str(A.TEAM_ALL), "0.5", str(rounds)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    X, U, rows = np.full((B, N + 1, 3), np.nan), np.full((B, N, 2), np.nan), {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "team":
            (X if f[1] == "x" else U)[int(f[2]), int(f[3])] = [float.fromhex(v) for v in f[4:]]
        elif f[0] in ("uncoupled", "params", "coupled"):
            rows[f[0]] = np.array([float.fromhex(v) for v in f[1:]])
        elif f[0] in ("status", "index"):
            rows[f[0]] = int(f[1])
    s = P.unicycle_turn90(hip_make, batch=B, N=N, xf=xf, u0=np.array([0.1, 0.0]))
    s.set_initial_state(x0)
    idx = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 3 * (Ag - 1))
    assert idx == rows["index"]
    # the driver's per-knot loop of placeholder circles (1e-3 k, 0, radius 0), as the facade emits it: N + 1 rows, the rows
    # in front of and behind [1, N) repeat its ends
    seed = np.zeros((N + 1, Ag - 1, 3))
    seed[:, :, 0] = (1e-3 * np.clip(np.arange(N + 1), 1, N - 1))[:, None]
    s.set_constraint_track(idx, seed.reshape(N + 1, -1))
    s.solve()
    assert _bits(rows["uncoupled"], s.team_clearance(Ag, idx, rad)) and (rows["uncoupled"] < 0).all()
    s.team_fill_tracks(Ag, idx, rad)
    assert _bits(rows["params"], s.get_knot_params(idx))
    s.team_solve(Ag, idx, rad, A.TEAM_ALL, 0.5, rounds)
    Xs, Us = s.get_trajectory()
    assert _bits(X, Xs) and _bits(U, Us)
    assert _bits(rows["coupled"], s.team_clearance(Ag, idx, rad))
    assert rows["status"] == s.get_stats()["status"][0]
    s.close()
