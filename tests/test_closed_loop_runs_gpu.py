"""The four closed-loop runs of the C API (altro_mpc_run, altro_mpc_run_tracked, altro_mpc_run_multistart, altro_mpc_run_team)
share one driver and one run object on the engine (LoopBegin / LoopCycle / LoopEnd).  Each kind has its own "is the caller's
loop" test beside its feature; here is what only the shared run can get wrong:

* two runs back to back on ONE handle (2 cycles, then 3: the second Begin replaces the first run's blocks) are the caller's own
  loop of 5 cycles on a second handle, bit for bit, and a plain advance by the run's shift afterwards leaves both handles in
  the same state -- nothing of a finished run leaks into it;
* a run that is refused -- before its Begin, or in its first solve with the run's blocks already on the device -- leaves the
  handle usable: the next run equals the same run on a fresh handle.

kTurn90, batch 16, shift 2; four starts for the multi-start kind; the smallest team of tests/_team_common.py.
"""
import numpy as np
import pytest

import _mpc_common as M
import _team_common as TC
import test_mpc_gpu as TM            # _closed_loop, _problem
import test_mpc_track_gpu as TT      # w_of
import test_multistart_gpu as TMS    # _turn90

pytestmark = pytest.mark.gpu

B, SHIFT, FIRST, SECOND = 16, 2, 2, 3
CYCLES = FIRST + SECOND


def _state(s):
    """everything a solve and an advance leave on the handle"""
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    return dict(stats=s.get_stats(), X=X, U=U, K=K, d=d, lam=s.get_duals(), rho=s.get_penalties(), x0=s.get_initial_state())


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for name in a:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)


def _joined(first, second):
    """the logs of two runs back to back as the log of one: the second run starts from the state the first one ended in"""
    assert first["X_cl"][:, -1].tobytes() == second["X_cl"][:, 0].tobytes()
    out = {name: np.concatenate([first[name], second[name]], axis=1) for name in first if name != "X_cl"}
    out["X_cl"] = np.concatenate([first["X_cl"][:, :-1], second["X_cl"]], axis=1)
    return out


def _check(a, b, want, first, second, what):
    """a: the handle of the caller's loop; b: the handle of the two runs"""
    assert first["X_cl"].shape[1] == FIRST * SHIFT + 1 and second["X_cl"].shape[1] == SECOND * SHIFT + 1
    _same(want, _joined(first, second), what)
    _same(_state(a), _state(b), what)
    for s in (a, b):
        s.mpc_advance(SHIFT)
    _same(_state(a), _state(b), what + ", then a plain advance")
    assert a.get_track_offset() == b.get_track_offset() and a.get_reference_offset() == b.get_reference_offset()
    a.close()
    b.close()


def test_two_plain_runs_are_one_loop(A, P, hip_make, monkeypatch):
    monkeypatch.setattr(TM, "CYCLES", CYCLES)
    monkeypatch.setattr(TM, "SHIFT", SHIFT)
    W = M.disturbance(CYCLES, B, 3)
    a, cons = TM._problem(A, P, hip_make, "turn90", B)
    b, _ = TM._problem(A, P, hip_make, "turn90", B)
    for s in (a, b):
        s.set_options(reset_duals=0, initial_penalty=0.0)
    rec = TM._closed_loop(a, cons, W, True)
    want = dict(X_cl=np.concatenate([r["x0"][:, None] if k == 0 else r["X"][:, k:k + 1] for r in rec for k in range(SHIFT)] +
                                    [a.get_initial_state()[:, None]], axis=1),
                U_cl=np.concatenate([r["U"][:, :SHIFT] for r in rec], axis=1),
                iterations=np.stack([r["iterations"] for r in rec], axis=1), status=np.stack([r["status"] for r in rec], axis=1))
    first = b.mpc_run(FIRST, SHIFT, W[:FIRST])
    second = b.mpc_run(SECOND, SHIFT, W[FIRST:])
    _check(a, b, want, first, second, "mpc_run")


def test_two_tracked_runs_are_one_loop(A, P, hip_make):
    lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
    W = np.stack([TT.w_of(B, 1, SHIFT, 3)[:, 0] * np.cos(1.0 + c) for c in range(CYCLES)])  # [cycles][B][shift][n]
    a, b = P.batch_turn90(hip_make, B), P.batch_turn90(hip_make, B)
    for s in (a, b):
        s.set_options(reset_duals=0, initial_penalty=0.0)
    Xl, Ul, it, st, track = [], [], [], [], []
    for c in range(CYCLES):  # the caller's loop over the separate entry points
        a.solve()
        stats = a.get_stats()
        tr = a.mpc_track(SHIFT, 1, w=W[c][:, None], u_lo=lo, u_hi=hi)
        it.append(stats["iterations_total"].copy())
        st.append(stats["status"].copy())
        Xl.append(tr["X_cl"][:, 0, :SHIFT])
        Ul.append(tr["U_cl"][:, 0])
        track.append(tr["stats"][:, 0])
        a.mpc_advance(SHIFT, x0=tr["X_cl"][:, 0, SHIFT])
    want = dict(X_cl=np.concatenate(Xl + [a.get_initial_state()[:, None]], axis=1), U_cl=np.concatenate(Ul, axis=1),
                iterations=np.stack(it, axis=1), status=np.stack(st, axis=1), track=np.stack(track, axis=1))
    first = b.mpc_run_tracked(FIRST, SHIFT, W[:FIRST], u_lo=lo, u_hi=hi)
    second = b.mpc_run_tracked(SECOND, SHIFT, W[FIRST:], u_lo=lo, u_hi=hi)
    assert (want["track"]["steps_done"] == SHIFT).all()
    _check(a, b, want, first, second, "mpc_run_tracked")


def test_two_multistart_runs_are_one_loop(A, P, hip_make):
    starts = 4
    problems = B // starts
    a, b = TMS._turn90(P, hip_make, problems, starts), TMS._turn90(P, hip_make, problems, starts)
    W = np.repeat(M.disturbance(CYCLES, problems, a.n), starts, axis=1)  # one disturbance per problem, repeated per start
    g = np.arange(starts, dtype=np.float64)
    dU = np.broadcast_to(np.stack([0.02 * g, -0.03 * g], axis=1)[:, None, :], (starts, a.N, a.m)).copy()
    for s in (a, b):
        s.set_options(reset_duals=0, initial_penalty=0.0)
    Xl, Ul, it, st, win = [], [], [], [], []
    for c in range(CYCLES):  # the caller's loop over the separate entry points
        a.solve()
        stats = a.get_stats()
        it.append(stats["iterations_total"].copy())
        st.append(stats["status"].copy())
        win.append(a.multistart_spread(starts))
        X, U = a.get_trajectory()
        Xl += [a.get_initial_state()[:, None], X[:, 1:SHIFT]]
        Ul.append(U[:, :SHIFT])
        a.mpc_advance(SHIFT, w=W[c])
        a.multistart_perturb(starts, dU)
    want = dict(X_cl=np.concatenate(Xl + [a.get_initial_state()[:, None]], axis=1), U_cl=np.concatenate(Ul, axis=1),
                iterations=np.stack(it, axis=1), status=np.stack(st, axis=1), winner=np.stack(win, axis=1))
    first = b.mpc_run_multistart(starts, FIRST, SHIFT, w=W[:FIRST], dU=dU)
    second = b.mpc_run_multistart(starts, SECOND, SHIFT, w=W[FIRST:], dU=dU)
    assert first["winner"].shape == (problems, FIRST) and second["winner"].shape == (problems, SECOND)
    _check(a, b, want, first, second, "mpc_run_multistart")


def test_two_team_runs_are_one_loop(A, P, hip_make):
    T, Ag, mode, blend, _ = TC.CASES[0]  # the smallest team problem: three teams of two
    rounds = 2
    a, b = P.team_ring(hip_make, T, Ag), P.team_ring(hip_make, T, Ag)
    W = 0.1 * M.disturbance(CYCLES, T * Ag, 3)
    for s in (a, b):
        s.set_options(reset_duals=0, initial_penalty=0.0)
        s.solve()
    want = TC.mpc_team_loop(a, Ag, a.team_circle, a.team_radius, mode, blend, rounds, CYCLES, SHIFT, W)
    first = b.mpc_run_team(Ag, b.team_circle, b.team_radius, mode, blend, rounds, FIRST, SHIFT, w=W[:FIRST])
    second = b.mpc_run_team(Ag, b.team_circle, b.team_radius, mode, blend, rounds, SECOND, SHIFT, w=W[FIRST:])
    assert first["clear"].shape == (T, FIRST) and second["clear"].shape == (T, SECOND)
    assert a.get_knot_params(a.team_circle).tobytes() == b.get_knot_params(b.team_circle).tobytes()
    _check(a, b, want, first, second, "mpc_run_team")


def _slalom_without_reference(A, P, make):
    """problems.tracking_slalom with the reference held back -> (handle, Xref, Uref)"""
    N = 24
    s = make(3, 2, N, B, A.F64)
    Xref, Uref, h = P.slalom_path(B, N, N + 1 + 12)
    hd = float(h)
    s.set_model(A.MODEL_UNICYCLE)
    s.set_uniform_step(h)
    s.set_lqr_tracking_cost(0, N, np.diag([10.0, 10.0, 1.0]) * hd, np.eye(2) * (0.1 * hd))
    s.set_lqr_tracking_cost(N, N + 1, np.diag([10.0, 10.0, 1.0]), np.zeros((2, 2)))
    s.add_control_bound(0, N, [-0.7, -0.7], [0.7, 0.7])
    s.set_initial_state(Xref[:, 0] + np.array([0.0, 0.1, 0.0]))
    s.set_trajectory(None, np.tile(np.array([0.1, 0.1]), (N, 1)))
    return s, Xref, Uref


@pytest.mark.parametrize("uploaded", [False, True], ids=["before_the_upload", "on_the_device"])
def test_a_refused_run_leaves_the_handle_usable(A, P, hip_make, uploaded):
    """Without a reference path a tracking-cost handle answers ALTRO_NOT_READY: before the device state exists the driver says so
    ahead of Begin; on an uploaded handle the run's blocks are on the device when the first solve refuses, and End frees them."""
    W = M.disturbance(2, B, 3)
    s, Xref, Uref = _slalom_without_reference(A, P, hip_make)
    if uploaded:
        s.get_initial_state()
    with pytest.raises(A.AltroError) as e:
        s.mpc_run(2, SHIFT, W)
    assert f"({A.NOT_READY})" in str(e.value) and "no reference path is set" in str(e.value)
    s.set_reference(Xref, Uref)
    fresh, _, _ = _slalom_without_reference(A, P, hip_make)
    fresh.set_reference(Xref, Uref)
    _same(fresh.mpc_run(2, SHIFT, W), s.mpc_run(2, SHIFT, W), "the run after a refused one")
    _same(_state(fresh), _state(s), "the run after a refused one")
    assert fresh.get_reference_offset() == s.get_reference_offset() == 2 * SHIFT
    fresh.close()
    s.close()
