"""Shared by tests/test_knot_termination_gpu.py: the two problems that take a knot-routed handle (Engine::KnotRouted: a
tracking cost and knot constraints, the *_trk kernels) to the exits of the iLQR and AL loops, each stated twice -- for the
device with the tracking cost, the reference path, the knot constraints and a window offset, and for the CPU oracle with one
ordinary set_lqr_cost / add_constraint per knot from the same rows.

MO is problems.moving_obstacles(N = 24, rows = 37, offset = 5): five parameter sets, b mod 5.
GU is the give-up problem of tests/test_termination_gpu.py stated per knot: the indefinite R on knots [0, ks) only, following a
path that moves towards the goal under a control bound that widens along the horizon.  Everything is closed-form arithmetic
(no RNG); path and track differ from row to row and from instance to instance."""
import numpy as np

N_MO, ROWS_MO, OFFSET_MO = 24, 37, 5
GU_OFFSET = 3
GIVEUP_OPTS = dict(bp_reg_max=1e-3, bp_reg_fail_threshold=3)


def alternating(N, a, b):
    """Per-knot steps of two alternating values (tests/test_termination_gpu.py::alternating)."""
    return np.where(np.arange(N) % 2 == 0, np.float32(a), np.float32(b)).astype(np.float32)


def mo(P, make, batch, per_knot, steps=False, dtype=0, offset=OFFSET_MO, **opts):
    """problems.moving_obstacles at the window offset; ``steps``: alternating per-knot steps 0.05 / 0.04"""
    s = P.moving_obstacles(make, batch=batch, N=N_MO, rows=ROWS_MO, offset=offset, per_knot=per_knot, dtype=dtype)
    if steps:
        s.set_steps(alternating(N_MO, 0.05, 0.04))
    if opts:
        s.set_options(**opts)
    return s


def gu_rows(n, m, N, batch, xf):
    """(Xref [B][rows][n], Uref [B][rows][m], track [B][rows][2 m]) of GU, rows = N + 1 + GU_OFFSET; row r belongs to knot
    k = r - GU_OFFSET of the window the tests use: xref = xf (0.5 + 0.5 k / N), uref = (0.01 sin 0.3 k, 0, ...), the bound
    +-(0.1 + 0.001 k + 0.0002 (b mod 5)).  (The rows in front of the window continue the formulas to k < 0: a kernel that reads
    them reads other numbers.)"""
    rows = N + 1 + GU_OFFSET
    k = np.arange(rows, dtype=np.float64) - GU_OFFSET
    Xref = xf[:, None, :] * (0.5 + 0.5 * k / N)[None, :, None]
    Uref = np.zeros((batch, rows, m))
    Uref[:, :, 0] = 0.01 * np.sin(0.3 * k)[None, :]
    ub = (0.1 + 0.001 * k)[None, :] + 0.0002 * (np.arange(batch) % 5)[:, None]
    track = np.concatenate([np.repeat(-ub[:, :, None], m, axis=2), np.repeat(ub[:, :, None], m, axis=2)], axis=2)
    return Xref, Uref, track


def gu(A, make, kind, n, m, N, ks, batch, per_knot, dtype=0, steps=False, **opts):
    """The give-up problem per knot.  Unicycle (kind A.MODEL_UNICYCLE / the oracle's built-in): the costs and goals of
    test_model_shapes_gpu.unicycle_restart_mix; else tests/models/shape_chain.hpp with those of chain_restart(mix=True).  R is
    indefinite (-2e-3 on every other control) on knots [0, ks) and 1e-3 I on [ks, N); Q = 1e-3 I; x0 = 0; the initial controls
    are 0.05 / 0.5 / 0.08 by b mod 3 -- the middle third starts outside the bound, whose penalty makes Quu definite."""
    unicycle = kind == A.MODEL_UNICYCLE
    if unicycle:
        xf = np.tile(np.array([1.0, 0.5, 0.3]), (batch, 1)) + np.linspace(0, 0.3, batch)[:, None]
        Qf = np.eye(n) * 10.0
    else:
        xf = np.tile(0.3 + 0.1 * np.arange(n), (batch, 1)) + np.linspace(0, 0.3, batch)[:, None]
        Qf = np.eye(n) * 0.05
    Q = np.eye(n) * 1e-3
    Rneg = np.diag([-2e-3 if j % 2 == 0 else 1e-3 for j in range(m)])
    Rpos = np.eye(m) * 1e-3
    Xref, Uref, track = gu_rows(n, m, N, batch, xf)
    s = make(n, m, N, batch, dtype)
    s.set_model(kind)
    s.set_uniform_step(np.float32(0.05))
    if per_knot:
        for k in range(N + 1):
            r = GU_OFFSET + k
            s.set_lqr_cost(k, k + 1, Q if k < N else Qf, (Rneg if k < ks else Rpos) if k < N else Rpos * 0, Xref[:, r], Uref[:, r])
        for k in range(N):
            s.add_constraint(A.CON_CONTROL_BOUND, k, k + 1, track[:, GU_OFFSET + k])
    else:
        s.set_lqr_tracking_cost(0, ks, Q, Rneg)
        s.set_lqr_tracking_cost(ks, N, Q, Rpos)
        s.set_lqr_tracking_cost(N, N + 1, Qf, Rpos * 0)
        s.set_reference(Xref, Uref)
        s.knot_bound = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 2 * m)
        s.set_constraint_track(s.knot_bound, track)
        s.set_reference_offset(GU_OFFSET)
        s.set_track_offset(GU_OFFSET)
    s.set_initial_state(np.zeros(n))
    U = np.zeros((batch, N, m))
    U[0::3] = 0.05
    U[1::3] = 0.5
    U[2::3] = 0.08
    s.set_trajectory(None, U)
    if steps:
        s.set_steps(alternating(N, 0.05, 0.04))
    s.set_options(**dict(GIVEUP_OPTS, **opts))
    return s
