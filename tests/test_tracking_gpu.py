"""Tracking a reference path on the device (include/altro_tracking.h): per-knot LQR tracking costs against the CPU oracle
given one ordinary cost per knot; a constant path against an ordinary cost group, bit for bit; host upload against device
upload; the window against a fresh handle; the window moving with the receding-horizon advance; the engine paths a tracking
handle takes; closed-loop tracking measured against the moving reference; the facade's per-knot SetCostFunction loop.
The problem is problems.tracking_slalom with N = 24 and a path of N + 1 + 12 = 37 rows unless stated otherwise."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _ledger
import _mpc_common as M  # noqa: F401  (imported, never changed)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ROWS = 24, 24 + 1 + 12
# the project's fp64 bars -- trajectories, expansions (tests/test_parity_gpu.py: step level), final cost
RTOL, ATOL = 1e-7, 1e-9
BOUND_CONS = [(0, N, 4, False)]  # problems.tracking_slalom(bounds=True): (k_begin, k_end, rows, equality)


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


def _same_terms(a, b, what):
    for name, x, y in zip("qrc", a, b):
        assert x.tobytes() == y.tobytes(), (what, name)


def _host_terms(Q, R, X, U):
    """q = -Q xref, r = -R uref, c = 0.5 xref'Q xref + 0.5 uref'R uref in the operation order of the problem compiler's
    linear_term (altro_problem.hpp): every sum from zero, left to right, no contraction -- plain Python floats."""
    def lin(W, ref):
        Wx = []
        for i in range(len(ref)):
            s = 0.0
            for j in range(len(ref)):
                s += float(W[i, j]) * float(ref[j])
            Wx.append(s)
        acc = 0.0
        for i in range(len(ref)):
            acc += float(ref[i]) * Wx[i]
        return [-v for v in Wx], acc
    q = np.zeros(X.shape)
    r = np.zeros(U.shape)
    c = np.zeros(X.shape[:-1])
    for idx in np.ndindex(*X.shape[:-1]):
        q[idx], xQx = lin(Q, X[idx])
        r[idx], uRu = lin(R, U[idx])
        c[idx] = 0.5 * xQx + 0.5 * uRu
    return q, r, c


# ---- 1. against the oracle, which takes one ordinary cost per knot -------------------------------------------------------------
@pytest.mark.parametrize("bounds", [True, False], ids=["bound", "free"])
@pytest.mark.parametrize("offset", [0, 12])
@pytest.mark.parametrize("batch", [5, 200])
def test_solve_against_the_oracle(A, P, oracle_make, hip_make, batch, offset, bounds):
    """Status, total and outer iterations exact; X, U to 1e-7 relative + 1e-9 absolute; the final cost to the bar of the
    full-solve comparisons (1e-10 relative), every measured figure in the ledger."""
    o = P.tracking_slalom(oracle_make, batch=batch, N=N, rows=ROWS, offset=offset, bounds=bounds, per_knot=True)
    g = P.tracking_slalom(hip_make, batch=batch, N=N, rows=ROWS, offset=offset, bounds=bounds)
    o.solve()
    g.solve()
    so, sg = o.get_stats(), g.get_stats()
    print(f"B {batch} offset {offset} bounds {bounds}: iterations {np.unique(so['iterations_total'])}, outer "
          f"{np.unique(so['iterations_outer'])}, statuses {np.unique(so['status'])}")
    if bounds:  # (checked on the CPU when the problem was chosen: with the bound every instance ends solved)
        assert (so["status"] == A.SOLVED).all()
    for f in ("status", "iterations_total", "iterations_outer"):
        assert (so[f] == sg[f]).all(), (f, np.flatnonzero(so[f] != sg[f]))
    Xo, Uo = o.get_trajectory()
    Xg, Ug = g.get_trajectory()
    _ledger.close(Xg, Xo, RTOL, ATOL, "X")
    _ledger.close(Ug, Uo, RTOL, ATOL, "U")
    _ledger.close(sg["cost"], so["cost"], 1e-10, 0.0, "stat cost")
    _ledger.close(sg["violation"], so["violation"], 1e-7, 1e-12, "stat violation")
    o.close()
    g.close()


@pytest.mark.parametrize("offset", [0, 12])
def test_step_level_against_the_oracle(P, oracle_make, hip_make, offset):
    """update_expansions, cost and one forward pass with the bars of tests/test_parity_gpu.py's step-level test."""
    o = P.tracking_slalom(oracle_make, batch=5, N=N, rows=ROWS, offset=offset, per_knot=True)
    g = P.tracking_slalom(hip_make, batch=5, N=N, rows=ROWS, offset=offset)
    for s in (o, g):
        s.rollout()
    _ledger.close(g.cost(), o.cost(), 1e-12, 0.0, "cost")
    for s in (o, g):
        s.update_expansions()
    for k in (0, 1, 11, N - 1, N):
        eo, eg = o.get_expansion(k), g.get_expansion(k)
        for key in ("lxx", "lx") + (("A", "B", "lxu", "luu", "lu") if k < N else ()):
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


# ---- 2. a constant path is an ordinary cost ---------------------------------------------------------------------------------
def _constant_pair(A, P, make, batch, per_instance):
    """-> (tracking handle whose every path row is xf, 0; set_lqr_cost handle on the general kernels through uniform
    set_steps; Q, R, Qf, xf)"""
    _, _, h = P.slalom_path(1, N, 1)
    hd = float(h)
    Q, R, Qf = np.diag([10.0, 10.0, 1.0]) * hd, np.eye(2) * (0.1 * hd), np.diag([10.0, 10.0, 1.0])
    xf = np.array([1.1, 0.45, 0.3]) + (0.07 * np.arange(batch)[:, None] * np.array([1.0, -1.0, 0.5]) if per_instance else 0.0)
    pair = []
    for tracking in (True, False):
        s = make(3, 2, N, batch, A.F64)
        s.set_model(A.MODEL_UNICYCLE)
        s.set_uniform_step(h)
        if tracking:
            s.set_lqr_tracking_cost(0, N, Q, R)
            s.set_lqr_tracking_cost(N, N + 1, Qf, R * 0)
            # one row (the window holds it on every knot) or, per instance, three equal rows
            s.set_reference(np.repeat(xf[:, None, :], 3, axis=1) if per_instance else xf[None, :])
        else:
            s.set_lqr_cost(0, N, Q, R, xf, np.zeros(2))
            s.set_lqr_cost(N, N + 1, Qf, R * 0, xf, np.zeros(2))
            s.set_steps(np.full(N, h, dtype=np.float32))
        s.add_control_bound(0, N, [-0.7, -0.7], [0.7, 0.7])
        s.set_initial_state(np.array([0.0, 0.1, 0.0]))
        s.set_trajectory(None, np.tile(np.array([0.1, 0.1]), (N, 1)))
        pair.append(s)
    return pair[0], pair[1], Q, R, Qf, xf


@pytest.mark.parametrize("per_instance", [False, True], ids=["shared", "per_instance"])
def test_constant_path_equals_an_ordinary_cost(A, P, hip_make, per_instance):
    B = 5
    t, u, Q, R, Qf, xf = _constant_pair(A, P, hip_make, B, per_instance)
    # the terms: what the problem compiler puts into the ordinary handle's parameter pool, to the bit
    X = np.broadcast_to(xf if per_instance else xf[None, :], (B, 3))
    q_s, r_s, c_s = _host_terms(Q, R, X, np.zeros((B, 2)))
    q_f, r_f, c_f = _host_terms(Qf, R * 0, X, np.zeros((B, 2)))
    q, r, c = t.get_reference_terms()
    for k in range(N + 1):
        want = (q_s, r_s, c_s) if k < N else (q_f, r_f, c_f)
        _same_terms((q[:, k], r[:, k], c[:, k]), want, f"knot {k}")
    t.solve()
    u.solve()
    a, b = _state(t), _state(u)
    assert (a["stats"]["status"] == A.SOLVED).all() and a["stats"]["iterations_total"].min() > 1
    _same(a, b, "constant path")
    t.close()
    u.close()


def test_terms_round_like_the_problem_compiler(A, hip_make):
    """Full (not diagonal) Q and R, a path of its own per instance, 70 instances (past one wavefront): every term equals
    the left-to-right sums of the problem compiler's linear_term bit for bit -- no contraction in k_ref_terms."""
    B, rows = 70, N + 5
    rng = np.random.RandomState(20261018)
    Lq, Lr = rng.standard_normal((3, 3)), rng.standard_normal((2, 2))
    Q, R = Lq @ Lq.T + np.eye(3), Lr @ Lr.T + np.eye(2)
    Q, R = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
    Xref, Uref = rng.standard_normal((B, rows, 3)), rng.standard_normal((B, rows, 2))
    s = hip_make(3, 2, N, B, A.F64)
    s.set_model(A.MODEL_UNICYCLE)
    s.set_uniform_step(np.float32(0.1))
    s.set_lqr_cost(0, N + 1, np.eye(3), np.eye(2), np.zeros(3), np.zeros(2))
    s.set_lqr_tracking_cost(3, N + 1, Q, R)  # knots 0 .. 2 keep the ordinary cost: their records read zero
    s.set_reference(Xref, Uref)
    s.set_reference_offset(2)
    s.set_initial_state(np.zeros(3))
    q, r, c = s.get_reference_terms()
    assert not q[:, :3].any() and not r[:, :3].any() and not c[:, :3].any()
    row = np.minimum(2 + np.arange(N + 1), rows - 1)
    _same_terms((q[:, 3:], r[:, 3:], c[:, 3:]), _host_terms(Q, R, Xref[:, row[3:]], Uref[:, row[3:]]), "full Q, R")
    s.close()


# ---- 3. host upload against device upload; shared against repeated ------------------------------------------------------------
def test_device_upload_and_shared_path(A, P, hip_make):
    B = 70
    Xref, Uref, _ = P.slalom_path(B, N, ROWS)
    host = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=5)
    dev = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=5)
    dx, du = DeviceArray(Xref), DeviceArray(Uref)
    dev.set_reference_device(dx.ptr, du.ptr, ROWS, True)
    assert dev.get_reference_offset() == 0  # a new path starts at its first row
    dev.set_reference_offset(5)
    _same_terms(host.get_reference_terms(), dev.get_reference_terms(), "device upload")
    host.solve()
    dev.solve()
    _same(_state(host), _state(dev), "device upload")
    dx.free()
    du.free()
    # one shared path (instance 3's) against the same path repeated for every instance; Uref left out = zeros
    shared = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
    repeated = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
    shared.set_reference(Xref[3])
    repeated.set_reference(np.repeat(Xref[3:4], B, axis=0), np.zeros((B, ROWS, 2)))
    for s in (shared, repeated):
        s.set_initial_state(Xref[3, 0] + np.array([0.0, 0.1, 0.0]))
    _same_terms(shared.get_reference_terms(), repeated.get_reference_terms(), "shared path")
    shared.solve()
    repeated.solve()
    _same(_state(shared), _state(repeated), "shared path")
    for s in (host, dev, shared, repeated):
        s.close()


# ---- 4. the window ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [5, 20])
def test_window_equals_a_fresh_handle(A, P, hip_make, offset):
    """Offset o on the path of 37 rows against a fresh handle that is given rows o .. o + N on the host (o = 20: the window
    runs past the path, the last row is held)."""
    B = 5
    Xref, Uref, _ = P.slalom_path(B, N, ROWS)
    win = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    rows = np.minimum(offset + np.arange(N + 1), ROWS - 1)
    if offset == 20:
        assert (rows == ROWS - 1).sum() > 1
    fresh = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    fresh.set_reference(Xref[:, rows], Uref[:, rows])
    assert win.get_reference_offset() == offset and fresh.get_reference_offset() == 0
    _same_terms(win.get_reference_terms(), fresh.get_reference_terms(), f"offset {offset}")
    win.solve()
    fresh.solve()
    _same(_state(win), _state(fresh), f"offset {offset}")
    win.close()
    fresh.close()


# ---- 5. the advance -----------------------------------------------------------------------------------------------------------------
def test_advance_moves_the_window(A, P, hip_make):
    B, shift = 5, 5
    s = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
    moved = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
    moved.set_reference_offset(shift)
    s.solve()
    before = _state(s)
    src = s.mpc_row_map(shift)
    assert np.array_equal(src, M.row_map(N, shift, BOUND_CONS))
    s.mpc_advance(shift)
    assert s.get_reference_offset() == shift
    _same_terms(s.get_reference_terms(), moved.get_reference_terms(), "advance")
    after = _state(s)
    Xn, Un, lam_n, rho_n = M.shifted(before["X"], before["U"], before["lam"], before["rho"], src, shift, M.reset_penalty(s))
    for name, want in (("X", Xn), ("U", Un), ("lam", lam_n), ("rho", rho_n), ("x0", before["X"][:, shift])):
        assert after[name].tobytes() == np.ascontiguousarray(want).tobytes(), name
    s.mpc_advance(shift, w=np.zeros((B, 3)))
    assert s.get_reference_offset() == 2 * shift
    # a handle without a tracking cost: the advance leaves the offset alone
    plain = P.unicycle_turn90(hip_make, batch=2, N=N)
    assert plain.get_reference_offset() == 0
    plain.solve()
    plain.mpc_advance(shift)
    assert plain.get_reference_offset() == 0
    q, r, c = plain.get_reference_terms()
    assert not q.any() and not r.any() and not c.any()
    for h in (s, moved, plain):
        h.close()


def test_mpc_loops_equal_the_callers_loop(A, P, hip_make):
    """mpc_run and mpc_run_tracked (3 cycles, shift 5, the disturbance of _mpc_common.disturbance) against the caller's own
    loop of solve / mpc_track / mpc_advance: logs, statistics and what is left on the handle, bit for bit."""
    B, cycles, shift = 5, 3, 5
    W = M.disturbance(cycles, B, 3)
    a = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
    b = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
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
    assert a.get_reference_offset() == b.get_reference_offset() == cycles * shift
    _same(_state(a), _state(b), "mpc_run")
    _same_terms(a.get_reference_terms(), b.get_reference_terms(), "mpc_run")
    a.close()
    b.close()
    # tracked: w [cycles][B][shift][n] from the same closed formula, one row per tracked knot
    Wt = np.ascontiguousarray(M.disturbance(cycles * shift, B, 3).reshape(cycles, shift, B, 3).transpose(0, 2, 1, 3))
    lo, hi = np.array([-0.7, -0.7]), np.array([0.7, 0.7])
    a = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
    b = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS)
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
    assert a.get_reference_offset() == b.get_reference_offset() == cycles * shift
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
    s = P.tracking_slalom(make, batch=B, N=24, rows=37, offset=5)
    s.solve()
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    t = s.get_timing()
    q, r, c = s.get_reference_terms()
    for name, v in (("stats", s.get_stats()), ("X", X), ("U", U), ("K", K), ("d", d), ("lam", s.get_duals()), ("rho", s.get_penalties()),
                    ("q", q), ("r", r), ("c", c)):
        out["%%d_%%s" %% (B, name)] = v[:40]
    out["%%d_timing" %% B] = np.array([t["fused_sweeps"], t["loop_workgroups"], t["segment_columns"], t["twin_workgroups"], t["sweeps"]])
    s.close()
np.savez(sys.argv[1], **out)
'''


def test_engine_paths(tmp_path):
    """Batches 8, 1024 and 4608 (one chain and the persistent kernel's domain; one chain of batched sweeps; four chains with
    shadow columns allocated): the first 40 instances -- eight parameter sets, b mod 5 -- agree bit for bit across the three,
    no launch of the persistent or of the loop kernel, no segment column; and once more with LDS, candidates and shadow
    columns poisoned (ALTRO_HIP_DEBUG_POISON=1) in a fresh process, identical."""
    def run(tag, env_extra):
        out = str(tmp_path / f"{tag}.npz")
        subprocess.run([sys.executable, "-c", _SCRIPT % ROOT, out], check=True, env=dict(os.environ, **env_extra), timeout=600)
        return np.load(out)

    ref, poisoned = run("default", {}), run("poisoned", {"ALTRO_HIP_DEBUG_POISON": "1"})
    for B in (8, 1024, 4608):
        fused, loop_wg, seg_cols, twins, sweeps = ref[f"{B}_timing"]
        assert (fused, loop_wg, seg_cols, twins) == (0, 0, 0, 0) and sweeps > 1, (B, ref[f"{B}_timing"])
        for name in ("stats", "X", "U", "K", "d", "lam", "rho", "q", "r", "c"):
            assert ref[f"{B}_{name}"][:8].tobytes() == ref[f"8_{name}"].tobytes(), (B, name)
            assert ref[f"{B}_{name}"].tobytes() == ref[f"1024_{name}"][:len(ref[f"{B}_{name}"])].tobytes(), (B, name)
    for k in ref.files:
        if not k.endswith("_timing"):
            assert ref[k].tobytes() == poisoned[k].tobytes(), ("poisoned", k)


# ---- 7. closed-loop tracking measures the moving reference -----------------------------------------------------------------------
def test_mpc_track_cost_is_the_tracking_cost(A, P, hip_make):
    """mpc_track over the whole horizon on the solved tracking handle: `cost` equals altro_cost of the tracked path on a
    second handle (same window) to 1e-12 relative, `violation` equals altro_max_violation exactly -- the bars of
    tests/test_mpc_track_gpu.py."""
    B, S, offset = 5, 3, 5
    s = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    s.solve()
    b, j, i = np.meshgrid(np.arange(B), np.arange(S), np.arange(3), indexing="ij")
    dx0 = 1e-2 * np.sin(1.0 + 3.0 * j + 5.0 * b + 7.0 * i)
    out = s.mpc_track(N, S, dx0=dx0)
    st = out["stats"]
    assert (st["steps_done"] == N).all()
    for smp in range(S):  # (one handle per sample: the instance decides the path, so the batch cannot carry the samples)
        con = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
        con.set_trajectory(out["X_cl"][:, smp], out["U_cl"][:, smp])
        assert st["violation"][:, smp].tobytes() == con.max_violation().tobytes(), smp
        free = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=offset, bounds=False)
        free.set_trajectory(out["X_cl"][:, smp], out["U_cl"][:, smp])
        J = free.cost()
        print(f"sample {smp}: max relative cost difference {np.abs(st['cost'][:, smp] / J - 1).max():.3g}")
        assert np.allclose(st["cost"][:, smp], J, rtol=1e-12, atol=0.0)
        con.close()
        free.close()
    s.close()


def test_solve_without_a_path_and_async(A, P, hip_make):
    """On a live device: a tracking handle whose path never came answers ALTRO_NOT_READY from the engine too (the device state
    exists: set_reference_device was refused nothing); and the new calls answer ALTRO_NOT_READY while a solve is in flight."""
    s = hip_make(3, 2, N, 2, A.F64)
    s.set_model(A.MODEL_UNICYCLE)
    s.set_uniform_step(np.float32(0.125))
    s.set_lqr_tracking_cost(0, N + 1, np.eye(3), np.eye(2))
    s.set_initial_state(np.zeros(3))
    q, r, c = s.get_reference_terms()  # (creates the device state; no path: the records are zero)
    assert not q.any() and not c.any()
    for call in (s.solve, s.cost, s.update_expansions):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value) and "reference" in str(e.value)
    s.set_reference(np.zeros((1, 3)))
    s.solve()
    t = P.tracking_slalom(hip_make, batch=300, N=N, rows=ROWS)
    t.solve_async()
    for call in (lambda: t.set_reference(np.zeros((4, 3))), lambda: t.set_reference_offset(3), t.get_reference_offset,
                 t.get_reference_terms, lambda: t.set_reference_device(4096, 0, 4, 0)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value) and "asynchronous" in str(e.value)
    t.wait()
    assert (t.get_stats()["status"] == A.SOLVED).all()
    s.close()
    t.close()


# ---- 8. the facade ------------------------------------------------------------------------------------------------------------------
def test_facade_per_knot_cost_loop(A, P, hip_make, tmp_path):
    """tests/cpp/tracking_facade_driver.cpp: the reference's loop prob.SetCostFunction(LQRCost(Q, R, xref_k, uref_k), k) over
    the 25 knots (window at row 5 of the slalom path) solved through the facade; the C calls on the same rows give the same
    bits, and AdvanceHorizon(5) moves the window.  (Before tracking costs existed the driver ended in "too many distinct cost
    functions".)"""
    B, offset, shift = 5, 5, 5
    exe = str(tmp_path / "tracking_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "tracking_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    Xref, Uref, h = P.slalom_path(B, N, ROWS)
    rows = np.minimum(offset + np.arange(N + 1), ROWS - 1)
    path = str(tmp_path / "path.bin")
    np.ascontiguousarray(np.concatenate([Xref[:, rows], Uref[:, rows]], axis=2)).tofile(path)
    r = subprocess.run([exe, path, str(B), str(N), str(offset), repr(float(h))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = dict(X=np.full((B, N + 1, 3), np.nan), U=np.full((B, N, 2), np.nan))
    head = None
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) > 4 and f[0] == "first" and f[1] in ("x", "u"):
            got["X" if f[1] == "x" else "U"][int(f[2]), int(f[3])] = [float.fromhex(v) for v in f[4:]]
        elif len(f) == 9 and f[0] == "first" and f[1] == "iterations":
            head = (int(f[2]), int(f[4]), int(f[6]), int(f[8]))
    assert "advanced offset %d" % shift in r.stdout.splitlines(), r.stdout[-300:]
    s = P.tracking_slalom(hip_make, batch=B, N=N, rows=ROWS, offset=offset)
    s.set_reference(Xref[:, rows], Uref[:, rows])  # the N + 1 rows the facade holds
    s.solve()
    st = s.get_stats()
    X, U = s.get_trajectory()
    assert head == (st["iterations_total"][0], st["iterations_outer"][0], st["status"][0], 0), head
    assert st["iterations_total"][0] > 1 and not np.isnan(got["X"]).any() and not np.isnan(got["U"]).any()
    assert got["X"].tobytes() == X.tobytes() and got["U"].tobytes() == U.tobytes()
    s.close()
