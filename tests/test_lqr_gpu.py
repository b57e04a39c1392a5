"""Time-varying LQR tracking gains on the device (include/altro_lqr.h) against their numpy statement (tests/_lqr_common.py).

The inputs of the statement are built as tests/test_cov_gpu.py builds them -- A_k, B_k from the CPU oracle, which is given the
GPU's trajectory (set_trajectory, update_expansions, get_expansion) -- with this file's own sizes: N = 24 and the batches the
lane groups of k_lqr_recur need (that file's `case` knows its own names only; its _x0s, _check, _inputs, _handle_state and
_same_state are used as they are).  The error of a matrix is max |gpu - numpy| / max |numpy| per (instance, knot); its bar is
the larger of
  * 8 x the same quantity between the float64 and the np.longdouble run of the statement on the same inputs, and
  * 4 N (n + m) 2^-52 max(1, kappa_S): the length of the accumulation times the conditioning of the one solve per knot.
Every parity handle and every reference is built once and shared; a test that installs gains builds its own handle."""
import os

import numpy as np
import pytest

import _cov_common as CC
import _lqr_common as LC
import _subset_common as SC
import _trigger_common as TG
from test_cov_gpu import _check as cov_check
from test_cov_gpu import _handle_state, _inputs, _same_state, _x0s
from test_mpc_track_gpu import DeviceBuffer
from test_user_model_gpu import CARTPOLE, cartpole_oracle  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

EPS = LC.EPS
N = 24


# ---- the cases: (GPU handle, oracle Jacobians) solved / linearised once ------------------------------------------------------------
def _build(A, P, make, name, kind=None):
    if name in ("turn90_5", "turn90_67", "turn90_f32", "turn90_steps"):
        B = 67 if name == "turn90_67" else 5
        s = P.unicycle_turn90(make, batch=B, N=N, dtype=A.F32 if name == "turn90_f32" else A.F64)
        if name == "turn90_steps":  # the general path: per-knot steps and times
            steps = (0.125 * (1.0 + 0.1 * np.sin(1.0 + np.arange(N)))).astype(np.float32)
            s.set_steps(steps)
            s.set_times(np.concatenate([[0.0], np.cumsum(steps)]).astype(np.float32))
        s.set_initial_state(_x0s(B, np.zeros(3)) if B == 5 else _x0s(B, np.zeros(3)) * 0.2)
        return s, "solve"
    if name == "tripleint_9":
        s = P.triple_integrator(make, batch=9, N=N, constraints=True)
        s.set_initial_state(_x0s(9, -np.array([1.0, 2.0, 0, 0, 0, 0])))
        return s, "solve"
    if name == "quad12_5":
        s = P.quadrotor12(make, batch=5, N=N, dtype=A.F64)
        s.set_initial_state(_x0s(5, np.zeros(12)))
        s.set_options(max_iterations_total=3, max_iterations_inner=3)
        return s, "solve_ilqr"
    assert name == "cartpole"
    s = P.cartpole_move(make, kind, batch=5, N=N, goal=np.linspace(0.6, 1.2, 5))
    s.set_initial_state(_x0s(5, np.zeros(4)))
    return s, "solve"


_CASES = {}


def case(A, P, hip_make, oracle_make, name, kind=None):
    """-> dict(g: the solved GPU handle, A, B: the oracle's Jacobians at the GPU's trajectory [B][N][n][.])"""
    if name not in _CASES:
        g, how = _build(A, P, hip_make, name, kind)
        getattr(g, how)()
        X, U = g.get_trajectory()
        o, _ = _build(A, P, oracle_make, "turn90_5" if name == "turn90_f32" else name, kind)  # (Jacobians in fp64 on both sides)
        o.set_trajectory(X, U)
        o.update_expansions()
        ex = [o.get_expansion(k) for k in range(g.N)]
        o.close()
        _CASES[name] = dict(g=g, A=np.stack([e["A"] for e in ex], axis=1), B=np.stack([e["B"] for e in ex], axis=1))
    return _CASES[name]


_REFS, _FRACTIONS = {}, {}


def _reference(name, c, Q, R, Qf):
    """the statement in float64 and longdouble on the case's Jacobians, once"""
    if name not in _REFS:
        _REFS[name] = LC.reference(c["A"], c["B"], Q, R, Qf)
    return _REFS[name]


def _parity(name, c, got, Q, R, Qf):
    """the bar of tests/_lqr_common.py: parity, which tests/test_recur_shapes_gpu.py and tests/test_recur_kernels_gpu.py share"""
    g = c["g"]
    LC.parity(name, _reference(name, c, Q, R, Qf), got, g.N, g.n, g.m, _FRACTIONS,
              os.environ.get("ALTRO_LQR_PARITY_OUT"))  # (how profiles/lqr_gains_parity.json is made)


# ---- 1. parity with the numpy statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["turn90_5", "turn90_67", "tripleint_9", "quad12_5", "turn90_steps", "turn90_f32"])
def test_parity(A, P, hip_make, oracle_make, name):
    """unicycle B = 5; B = 67 (16 instances per workgroup of k_lqr_recur, 64 per workgroup of the other two: wave and group
    boundaries); triple integrator (n = 6, G = 8) B = 9; 12-state B = 5 after solve_ilqr capped at 3 iterations; per-knot steps
    and times; an ALTRO_F32 handle (the Jacobians and the recursion are fp64 all the same)."""
    c = case(A, P, hip_make, oracle_make, name)
    g = c["g"]
    Q, R, Qf = LC.parity_weights(g.n, g.m)
    _parity(name, c, g.lqr_gains(Q, R, Qf), Q, R, Qf)


def test_parity_user_model(A, P, hip_make, cartpole_oracle):  # noqa: F811
    """the cart-pole user model (n = 4, m = 1), on the plug-in the suite's build leaves in the cache"""
    kind = A.register_model_source("cartpole", CARTPOLE)
    c = case(A, P, hip_make, cartpole_oracle, "cartpole", kind)
    g = c["g"]
    Q, R, Qf = LC.parity_weights(g.n, g.m)
    _parity("cartpole", c, g.lqr_gains(Q, R, Qf), Q, R, Qf)


# ---- 2. exact properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["turn90_67", "tripleint_9", "quad12_5"])
def test_exact_properties(A, P, hip_make, oracle_make, name):
    g = case(A, P, hip_make, oracle_make, name)["g"]
    B, n, m = g.batch, g.n, g.m
    Q, R, Qf = LC.parity_weights(n, m)
    before = _handle_state(g)
    got = g.lqr_gains(Q, R, Qf)
    _same_state(before, _handle_state(g), "lqr_gains without install")
    assert got["fail"].dtype == np.int32 and (got["fail"] == -1).all()
    assert (got["P"] == np.swapaxes(got["P"], 2, 3)).all() and np.isfinite(got["P"]).all() and np.isfinite(got["K"]).all()
    assert (got["P"][:, N] == CC.lower_sym(Qf)).all()
    assert (g.lqr_gains(Q, R)["P"][:, N] == CC.lower_sym(Q)).all()  # Qf NULL: Q
    again = g.lqr_gains(Q, R, Qf)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    # garbage above the diagonals is never read
    sym = g.lqr_gains(CC.lower_sym(Q), CC.lower_sym(R), CC.lower_sym(Qf))
    for k in got:
        assert got[k].tobytes() == sym[k].tobytes(), k
    # the device form, with canaries behind every output
    pad = 64
    Kc = np.ascontiguousarray(np.swapaxes(got["K"], 2, 3))  # [B][N][m n], column-major m x n
    dQ, dR, dQf = DeviceBuffer(Q.nbytes, Q), DeviceBuffer(R.nbytes, R), DeviceBuffer(Qf.nbytes, Qf)
    bufs = dict(K=DeviceBuffer(8 * (Kc.size + pad), np.full(Kc.size + pad, -77.0)),
                P=DeviceBuffer(8 * (got["P"].size + pad), np.full(got["P"].size + pad, -77.0)),
                fail=DeviceBuffer(4 * (B + pad), np.full(B + pad, -77, dtype=np.int32)))
    g.lqr_gains_device(dQ.ptr, dR.ptr, dQf.ptr, False, bufs["K"].ptr, bufs["P"].ptr, bufs["fail"].ptr)
    for key, want, dt in (("K", Kc, np.float64), ("P", got["P"], np.float64), ("fail", got["fail"], np.int32)):
        out = bufs[key].read(dt, (want.size + pad,))
        assert out[:want.size].tobytes() == want.tobytes(), key
        assert (out[want.size:] == -77).all(), key
    # outputs left NULL are not written, and the others do not depend on them
    for b in bufs.values():
        b.free()
    only = DeviceBuffer(8 * (Kc.size + pad), np.full(Kc.size + pad, -77.0))
    g.lqr_gains_device(dQ.ptr, dR.ptr, dQf.ptr, False, only.ptr, 0, 0)
    out = only.read(np.float64, (Kc.size + pad,))
    assert out[:Kc.size].tobytes() == Kc.tobytes() and (out[Kc.size:] == -77.0).all()
    alone = g.lqr_gains(Q, R, Qf, want=("P",))
    assert list(alone) == ["P"] and alone["P"].tobytes() == got["P"].tobytes()
    for b in (only, dQ, dR, dQf):
        b.free()


def test_independent_of_the_neighbours(A, P, hip_make, oracle_make):
    """the plan of instance 37 of the B = 67 case alone on a handle of batch 1: the same bits"""
    g = case(A, P, hip_make, oracle_make, "turn90_67")["g"]
    Q, R, Qf = LC.parity_weights(g.n, g.m)
    got = g.lqr_gains(Q, R, Qf)
    X, U = g.get_trajectory()
    for b in (0, 37, 66):
        one = P.unicycle_turn90(hip_make, batch=1, N=N)
        one.set_trajectory(X[b:b + 1], U[b:b + 1])
        alone = one.lqr_gains(Q, R, Qf)
        for k in ("K", "P", "fail"):
            assert alone[k][0].tobytes() == got[k][b].tobytes(), (b, k)
        one.close()


# ---- 3. install ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_install(A, P, hip_make, dtype_name):
    B = 5
    s = P.unicycle_turn90(hip_make, batch=B, N=N, dtype=getattr(A, dtype_name))
    s.set_initial_state(_x0s(B, np.zeros(3)))
    s.solve()
    Q, R, Qf = LC.parity_weights(s.n, s.m)
    before = _handle_state(s)
    got = s.lqr_gains(Q, R, Qf, install=False)
    _same_state(before, _handle_state(s), "install = 0")
    inst = s.lqr_gains(Q, R, Qf, install=True)
    for k in got:
        assert got[k].tobytes() == inst[k].tobytes(), k
    after = _handle_state(s)
    want = got["K"].astype(np.float32).astype(np.float64) if dtype_name == "F32" else got["K"]
    assert after["K"].tobytes() == np.ascontiguousarray(want).tobytes()
    assert (after["d"] == 0).all() and not np.signbit(after["d"]).any()
    assert before["K"].tobytes() != after["K"].tobytes()
    for k in before:
        if k not in ("K", "d"):
            assert before[k].tobytes() == after[k].tobytes(), k
    # the cost-to-go of the solver can no longer be replayed: its backward pass would write the solver's gains back
    with pytest.raises(A.AltroError) as e:
        s.get_ctg()
    assert f"({A.NOT_READY})" in str(e.value)
    assert _handle_state(s)["K"].tobytes() == after["K"].tobytes()
    s.close()


def test_install_on_a_handle_that_was_never_solved(A, P, hip_make, oracle_make):
    """a trajectory and a step, no solve: altro_mpc_track is refused before the call and accepted after it"""
    g = case(A, P, hip_make, oracle_make, "turn90_5")["g"]
    X, U = g.get_trajectory()
    s = P.unicycle_turn90(hip_make, batch=5, N=N)
    s.set_initial_state(X[:, 0])
    s.set_trajectory(X, U)
    with pytest.raises(A.AltroError) as e:
        s.mpc_track(N, 1)
    assert f"({A.NOT_READY})" in str(e.value)
    Q, R, Qf = LC.parity_weights(s.n, s.m)
    got = s.lqr_gains(Q, R, Qf, install=True)
    assert got["K"].tobytes() == g.lqr_gains(Q, R, Qf)["K"].tobytes()
    t = s.mpc_track(N, 1, dx0=np.full((5, 1, s.n), 1e-3))
    assert (t["stats"]["steps_done"] == N).all() and np.isfinite(t["X_cl"]).all()
    Kh, dh = s.get_gains()
    assert np.ascontiguousarray(Kh).tobytes() == got["K"].tobytes() and (dh == 0).all()
    s.close()


def test_no_step_is_refused(A, P, hip_make):
    s = hip_make(3, 2, N, 2, A.F64)
    s.set_model(A.MODEL_UNICYCLE)
    s.set_lqr_cost(0, N + 1, np.eye(3), np.eye(2), np.zeros(3), np.zeros(2))
    s.set_initial_state(np.zeros(3))
    with pytest.raises(A.AltroError) as e:
        s.lqr_gains(np.eye(3), np.eye(2))
    assert f"({A.NOT_READY})" in str(e.value) and "step" in str(e.value)
    s.close()


# ---- 4. the failure path ---------------------------------------------------------------------------------------------------------------
def _mixed_failure_qf(c, Q, R):
    """Qf = diag(-v, 50, 1) with v found by the statement (tests/_lqr_common.py: mixed_failure_qf)"""
    return LC.mixed_failure_qf(c["A"], c["B"], Q, R, lambda v: np.diag([-v, 50.0, 1.0]))[0]


def test_failure_path(A, P, hip_make, oracle_make):
    """An indefinite Qf, chosen with the statement so that some instances of the per-instance plans fail and others do not,
    and so that its neighbours in the search give the same answer (no pivot sits on the edge): fail equals the statement's,
    the NaN pattern matches, the instances that did not fail meet the parity bar's floor, and with install the failed
    instances keep their gain records bit for bit."""
    c = case(A, P, hip_make, oracle_make, "turn90_67")
    Q, R, _ = LC.parity_weights(3, 2)
    Qf = _mixed_failure_qf(c, Q, R)
    K, Pm, fail, _ = LC.gains(c["A"], c["B"], Q, R, Qf)
    assert (LC.gains(c["A"], c["B"], Q, R, Qf, dtype=np.longdouble)[2] == fail).all()
    print(f"Qf = diag({Qf[0, 0]:.5g}, 50, 1): {int((fail >= 0).sum())} of {len(fail)} instances fail, at knots {sorted(set(fail[fail >= 0].tolist()))}")
    s = P.unicycle_turn90(hip_make, batch=67, N=N)
    X, U = c["g"].get_trajectory()
    s.set_initial_state(X[:, 0])
    s.set_trajectory(X, U)
    s.solve()  # (gains to keep; the plan moves, so what is compared below is computed on the shared, untouched case)
    got = c["g"].lqr_gains(Q, R, Qf)
    assert (got["fail"] == fail).all()
    assert (np.isnan(got["K"]) == np.isnan(K)).all() and (np.isnan(got["P"]) == np.isnan(Pm)).all()
    for b in np.flatnonzero(fail >= 0):
        assert np.isnan(got["K"][b, :fail[b] + 1]).all() and np.isfinite(got["K"][b, fail[b] + 1:]).all()
        assert np.isnan(got["P"][b, :fail[b] + 1]).all() and np.isfinite(got["P"][b, fail[b] + 1:]).all()
    fine = ~np.isnan(Pm)
    scale = np.abs(Pm[fine]).max()
    assert np.abs(got["P"][fine] - Pm[fine]).max() <= 1e-9 * scale
    # install: the failed instances keep their records, the others get theirs
    before = SC.snapshot(s)
    inst = s.lqr_gains(Q, R, Qf, install=True)
    after = SC.snapshot(s)
    bad = inst["fail"] >= 0
    assert bad.any() and (~bad).any()
    assert not SC.differing(after, before, bad), SC.differing(after, before, bad)
    assert sorted(SC.differing(after, before, ~bad)) == ["K", "d"]
    assert np.ascontiguousarray(after["K"][~bad]).tobytes() == np.ascontiguousarray(inst["K"][~bad]).tobytes()
    s.close()


# ---- 5. the cost-to-go identity, end to end through the tracker ------------------------------------------------------------------------
def test_cost_to_go_identity(A, P, hip_make, oracle_make):
    """Triple integrator, B = 9, LQR gains installed; altro_mpc_track over the whole horizon, no clipping, no noise, one sample
    per instance with |dx0| = 1e-2 per state.  The deviation's dynamics are exactly linear, so
    sum_k (e_k^T Q e_k + du_k^T R du_k) + e_N^T Qf e_N = dx0^T P_0 dx0.  The bar of |sum - dx0^T P_0 dx0| / |dx0^T P_0 dx0| is
    the larger of 64 x what the statement's own rollout shows for the identity in float64 against longdouble and
    4 N (n + m) 2^-52 sum|terms| / |total|."""
    c = case(A, P, hip_make, oracle_make, "tripleint_9")
    B, n, m = 9, 6, 2
    Q, R, Qf = LC.parity_weights(n, m)
    s = P.triple_integrator(hip_make, batch=B, N=N, constraints=True)
    X, U = c["g"].get_trajectory()
    s.set_initial_state(X[:, 0])
    s.set_trajectory(X, U)
    got = s.lqr_gains(Q, R, Qf, install=True)
    dx0 = 1e-2 * np.where((np.arange(B)[:, None] + np.arange(n)[None, :]) % 3 == 0, -1.0, 1.0)
    t = s.mpc_track(N, 1, dx0=dx0[:, None, :])
    assert (t["stats"]["steps_done"] == N).all()
    E, dU = t["X_cl"][:, 0] - X, t["U_cl"][:, 0] - U
    ref = _reference("tripleint_9", c, Q, R, Qf)
    worst = 0.0
    for b in range(B):
        terms = LC.logged_cost(E[b], dU[b], Q, R, Qf, dtype=np.longdouble)
        total = np.longdouble(dx0[b]) @ got["P"][b, 0].astype(np.longdouble) @ np.longdouble(dx0[b])
        measured = float(abs(terms.sum() - total) / abs(total))
        t64 = LC.rollout_cost(c["A"][b], c["B"][b], ref["K"][b], Q, R, Qf, dx0[b])[0]
        tL = LC.rollout_cost(c["A"][b], c["B"][b], ref["KL"][b], Q, R, Qf, dx0[b], dtype=np.longdouble)[0]
        r64 = np.longdouble(t64.sum() - dx0[b] @ ref["P"][b, 0] @ dx0[b])
        rL = tL.sum() - np.longdouble(dx0[b]) @ ref["PL"][b, 0] @ np.longdouble(dx0[b])
        own = float(abs(r64 - rL) / abs(total))
        floor = 4 * N * (n + m) * EPS * float(np.abs(terms).sum() / abs(total))
        bar = max(64.0 * own, floor)
        worst = max(worst, measured / bar)
        print(f"instance {b}: identity residual {measured:.3e}, bar {bar:.3e} (64 x own {64 * own:.3e}, floor {floor:.3e})")
        assert measured <= bar, (b, measured, bar)
    print(f"cost-to-go identity: largest fraction of the bar {worst:.3f}")
    s.close()


# ---- 6. the consumers see the installed gains --------------------------------------------------------------------------------------------
def test_covariance_reads_the_installed_gains(A, P, hip_make, oracle_make):
    c = case(A, P, hip_make, oracle_make, "turn90_5")
    B, n = 5, 3
    X, U = c["g"].get_trajectory()
    s = P.unicycle_turn90(hip_make, batch=B, N=N)
    s.set_initial_state(X[:, 0])
    s.set_trajectory(X, U)
    s.solve()  # (the solver's gains; the plan it leaves is not the case's, so the Jacobians are taken again below)
    Sigma0, W = _inputs(B, n, N, 31)
    under_solver = s.cov_propagate(N, Sigma0, W, want=("Sigma", "su"))
    Q, R, Qf = LC.parity_weights(n, s.m)
    s.set_trajectory(X, U)  # the case's plan, whose Jacobians the case holds
    s.lqr_gains(Q, R, Qf, install=True)
    K = s.get_gains()[0].copy()
    got = s.cov_propagate(N, Sigma0, W, want=("Sigma", "su"))
    cov_check("installed LQR gains", got, dict(A=c["A"], B=c["B"], K=K), N, Sigma0, W, 3, N, n)
    assert CC.matrix_rel(got["Sigma"], under_solver["Sigma"])[:, 1:].max() > 1e-3
    assert np.abs(got["su"] - under_solver["su"]).max() > 0
    s.close()


# ---- 7. the policy -------------------------------------------------------------------------------------------------------------------------
def _all_rows(s):
    return np.ones(s.batch, bool)


def test_policy_solve_is_solve_then_install(A, P, hip_make):
    """altro_solve_al with the policy on leaves the bits of altro_solve_al followed by altro_lqr_gains(install = 1); with the
    policy cleared again a solve's bits are those of a handle that never had one."""
    B = 5
    Q, R, Qf = LC.parity_weights(3, 2)
    hs = []
    for _ in range(3):
        s = P.unicycle_turn90(hip_make, batch=B, N=N)
        s.set_initial_state(_x0s(B, np.zeros(3)))
        hs.append(s)
    pol, comp, plain = hs
    pol.set_lqr_policy(Q, R, Qf)  # (before the device state exists)
    assert pol.get_lqr_policy() is not None
    pol.solve()
    comp.solve()
    plain.solve()
    k_solver = SC.snapshot(comp)
    inst = comp.lqr_gains(Q, R, Qf, install=True)
    a, b = SC.snapshot(pol), SC.snapshot(comp)
    assert not SC.differing(a, b, _all_rows(pol)), SC.differing(a, b, _all_rows(pol))
    assert sorted(SC.differing(b, k_solver, _all_rows(pol))) == ["K", "d"]
    assert np.ascontiguousarray(a["K"]).tobytes() == inst["K"].tobytes()
    with pytest.raises(A.AltroError) as e:
        pol.get_ctg()
    assert f"({A.NOT_READY})" in str(e.value)
    # solve_ilqr ends with the pass too
    pol.solve_ilqr()
    comp.solve_ilqr()
    comp.lqr_gains(Q, R, Qf, install=True)
    a, b = SC.snapshot(pol), SC.snapshot(comp)
    assert not SC.differing(a, b, _all_rows(pol)), SC.differing(a, b, _all_rows(pol))
    # cleared: a fresh solve from the same start is the plain handle's
    pol.set_lqr_policy(None)
    assert pol.get_lqr_policy() is None
    for s in (pol, plain):
        s.set_initial_state(_x0s(B, np.zeros(3)))
        s.set_trajectory(None, np.tile([0.1, 0.1], (N, 1)))
        s.reset_stats()
        s.solve()
    a, b = SC.snapshot(pol), SC.snapshot(plain)
    assert not SC.differing(a, b, _all_rows(pol)), SC.differing(a, b, _all_rows(pol))
    for s in hs:
        s.close()


def test_policy_run_tracked_is_the_composed_loop(A, P, hip_make):
    """altro_mpc_run_tracked, B = 8, 3 cycles, shift 2, with the policy on, against the caller's loop with the policy off:
    solve, altro_lqr_gains(install), track, advance -- logs and final snapshot bit for bit."""
    B, cycles, shift = 8, 3, 2
    Q, R, Qf = LC.parity_weights(3, 2)
    run_h, ref_h = P.batch_turn90(hip_make, B, N=N), P.batch_turn90(hip_make, B, N=N)
    w = 1e-3 * np.sin(1.0 + np.arange(cycles * B * shift * 3)).reshape(cycles, B, shift, 3)
    lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
    run_h.set_lqr_policy(Q, R, Qf)
    got = run_h.mpc_run_tracked(cycles, shift, w=w, u_lo=lo, u_hi=hi)
    L = cycles * shift
    ref = dict(X_cl=np.zeros((B, L + 1, 3)), U_cl=np.zeros((B, L, 2)), iterations=np.zeros((B, cycles), dtype=np.int32),
               status=np.zeros((B, cycles), dtype=np.int32))
    track = []
    for c in range(cycles):
        ref_h.solve()
        assert (ref_h.lqr_gains(Q, R, Qf, install=True, want=("fail",))["fail"] == -1).all()
        st = ref_h.get_stats()
        ref["iterations"][:, c], ref["status"][:, c] = st["iterations_total"], st["status"]
        t = ref_h.mpc_track(shift, 1, w=w[c][:, None], u_lo=lo, u_hi=hi)
        track.append(t["stats"][:, 0])
        ref["X_cl"][:, c * shift:(c + 1) * shift + 1] = t["X_cl"][:, 0]
        ref["U_cl"][:, c * shift:(c + 1) * shift] = t["U_cl"][:, 0]
        ref_h.mpc_advance(shift, x0=t["X_cl"][:, 0, shift])
    ref["track"] = np.stack(track, axis=1)
    for key in ("X_cl", "U_cl", "iterations", "status"):
        assert TG.same_bits(got[key], ref[key]), key
    for field in ref["track"].dtype.names:
        assert TG.same_bits(np.ascontiguousarray(got["track"][field]), np.ascontiguousarray(ref["track"][field])), field
    a, b = SC.snapshot(run_h), SC.snapshot(ref_h)
    assert not SC.differing(a, b, np.ones(B, bool)), SC.differing(a, b, np.ones(B, bool))
    run_h.close()
    ref_h.close()


def test_policy_run_triggered_installs_under_the_mask(A, P, hip_make):
    """altro_mpc_run_triggered, B = 70, 3 cycles, shift 2, with the policy on, against the composed loop of
    tests/_trigger_common.py on a handle with the same policy (its solves run under the mask the rule left): logs and final
    snapshot bit for bit; around every solve of the loop an instance that was skipped keeps its whole snapshot, gain record
    included, and a solved one carries the LQR gains of its new plan."""
    B, cycles, shift = 70, 3, 2
    Q, R, Qf = LC.parity_weights(3, 2)
    rule = TG.rule_dict(max_age=3, dx_tol=1e-3)
    run_h, ref_h = P.batch_turn90(hip_make, B, N=N), P.batch_turn90(hip_make, B, N=N)
    w = TG.pulses(cycles, B, shift, 3, 1e-2)
    lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
    for s in (run_h, ref_h):
        s.set_lqr_policy(Q, R, Qf)
    ref = TG.composed_loop(ref_h, cycles, shift, rule, w, lo, hi, snapshot=SC.snapshot)
    counts = [int(mk.sum()) for mk in ref["masks"]]
    print(f"solved per cycle {counts}")
    assert counts[0] == B and any(0 < v < B for v in counts), counts
    skipped = 0
    for c, (before, after) in enumerate(ref["around"]):
        rows = ~ref["masks"][c]
        skipped += int(rows.sum())
        assert not SC.differing(after, before, rows), (c, SC.differing(after, before, rows))
        if (~rows).any():
            assert "K" in SC.differing(after, before, ~rows) and (after["d"][~rows] == 0).all()
    assert skipped > 0
    got = run_h.mpc_run_triggered(cycles, shift, rule, w=w, u_lo=lo, u_hi=hi)
    for key in ("X_cl", "U_cl", "iterations", "status", "reason"):
        assert TG.same_bits(got[key], ref[key]), key
    for field in ref["track"].dtype.names:
        assert TG.same_bits(np.ascontiguousarray(got["track"][field]), np.ascontiguousarray(ref["track"][field])), field
    a, b = SC.snapshot(run_h), SC.snapshot(ref_h)
    assert not SC.differing(a, b, np.ones(B, bool)), SC.differing(a, b, np.ones(B, bool))
    # a masked solve by hand: the masked-in instances carry the LQR gains of their plan, the others keep their records
    mask = np.arange(B) % 3 == 0
    before = SC.snapshot(ref_h)
    ref_h.set_solve_mask(mask)
    ref_h.solve()
    ref_h.set_solve_mask(None)
    after = SC.snapshot(ref_h)
    assert not SC.differing(after, before, ~mask)
    direct = ref_h.lqr_gains(Q, R, Qf)
    assert np.ascontiguousarray(after["K"][mask]).tobytes() == np.ascontiguousarray(direct["K"][mask]).tobytes()
    run_h.close()
    ref_h.close()


def test_asynchronous_solve(A, P, hip_make):
    """While an asynchronous solve owns the handle all four calls answer ALTRO_NOT_READY; the asynchronous solve itself ends
    with the policy's pass."""
    B = 5
    Q, R, Qf = LC.parity_weights(3, 2)
    s = P.unicycle_turn90(hip_make, batch=B, N=N)
    s.set_initial_state(_x0s(B, np.zeros(3)))
    s.set_lqr_policy(Q, R, Qf)
    s.solve_async()
    for call in (lambda: s.lqr_gains(Q, R, Qf), lambda: s.lqr_gains_device(8, 8, 0, True), lambda: s.set_lqr_policy(None),
                 lambda: s.get_lqr_policy()):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value)
    s.wait()
    assert s.get_lqr_policy() is not None
    K, d = s.get_gains()
    assert np.ascontiguousarray(K).tobytes() == s.lqr_gains(Q, R, Qf)["K"].tobytes() and (d == 0).all()
    s.close()
