"""Shared by tests/test_knot_shapes_gpu.py: the problems that put a knot-routed handle (a tracking cost and knot constraints,
Engine::KnotRouted) on every shape of the model matrix, and the host statements they are compared with.

chain_tracking is tests/models/shape_chain.hpp following a path it can follow -- its own RK4 rollout under a seeded control
signal -- under a control bound that tightens along the track.  Costs are symmetric and NOT diagonal.  Everything is seeded by
arithmetic (no RNG).  moving_obstacles_starts is problems.moving_obstacles laid out as problems x adjacent starts."""
import numpy as np

from test_model_shapes_gpu import chain_rk4

H = np.float32(0.05)


def sym(k, d, o):
    """k x k: d on the diagonal, o on the first off-diagonals"""
    return d * np.eye(k) + o * (np.eye(k, k=1) + np.eye(k, k=-1))


def chain_costs(n, m, hd=None):
    """-> Q, R on [0, N); Qf on knot N (R = 0 there).  hd: the step the host scales with (default: float(H))"""
    hd = float(H) if hd is None else hd
    return sym(n, 2.0, 0.5) * hd, sym(m, 0.1, 0.02) * hd, sym(n, 5.0, 1.0)


def chain_path(n, m, batch, rows, hd=None):
    """(Xref [B][rows][n], Uref [B][rows][m]): Uref[b, r, j] = (0.3 + 0.02 (b mod 5)) sin(2 t + 0.7 j) + 0.1 cos(0.9 t (1 + j)),
    t = r h; Xref[b, 0] = 0 and Xref[b, r + 1] the chain's RK4 step from Xref[b, r] under Uref[b, r].  hd: the step the host
    builds the path with (default: float(H), what the library integrates with)."""
    hd = float(H) if hd is None else hd
    t = (np.arange(rows) * hd)[None, :, None]
    j = np.arange(m, dtype=np.float64)[None, None, :]
    amp = (0.3 + 0.02 * (np.arange(batch) % 5))[:, None, None]
    Uref = amp * np.sin(2.0 * t + 0.7 * j) + 0.1 * np.cos(0.9 * t * (1.0 + j))
    Xref = np.zeros((batch, rows, n))
    for r in range(rows - 1):
        Xref[:, r + 1] = chain_rk4(Xref[:, r], Uref[:, r:r + 1], hd, n, m)
    return Xref, Uref


def chain_bound(m, batch, rows):
    """ub [B][rows] = 0.3 (1 - 0.01 r) + 0.01 (b mod 5), and the track [B][rows][2 m] = (-ub ... | +ub ...)"""
    ub = 0.3 * (1.0 - 0.01 * np.arange(rows))[None, :] + 0.01 * (np.arange(batch) % 5)[:, None]
    return ub, np.concatenate([np.repeat(-ub[:, :, None], m, axis=2), np.repeat(ub[:, :, None], m, axis=2)], axis=2)


BOUND_ROWS = 100  # the ramp 0.3 (1 - 0.01 r) closes at row 100 (the library refuses lb >= ub): a longer track ends at row 99, which is held


def window(a, offset, knots):
    """rows min(offset + k, rows - 1), k in knots, of a path or track [B][rows][.]"""
    return a[:, np.minimum(offset + np.asarray(knots), a.shape[1] - 1)]


ULPS = ("x0+", "x0-", "Q+", "Q-", "R+", "xref+", "uref+", "bound+")


def chain_tracking(A, make, kind, n, m, batch=12, N=20, rows=None, offset=0, dtype=0, per_knot=False, ulp=None, host_step=None):
    """The chain following chain_path under chain_bound, the windows of both at row ``offset``; x0 = Xref[offset] with 0.1 added
    to state 0, U = 0.  ``per_knot``: one set_lqr_cost and one ordinary control bound per knot from the same rows (what the
    CPU oracle takes), as problems.moving_obstacles does.
    ``ulp``: one of ULPS -- that input moved by one unit in the last place, every element, before it is sent (how far the
    REFERENCE's answer moves under the smallest change of its inputs).
    ``host_step``: the step the host builds costs and path with, where not the fp32-rounded float(H); the library is given
    H either way (its steps are 32-bit floats)."""
    rows = N + 1 + 8 if rows is None else rows
    Q, R, Qf = chain_costs(n, m, host_step)
    Xref, Uref = chain_path(n, m, batch, rows, host_step)
    _, track = chain_bound(m, batch, min(rows, BOUND_ROWS))
    x0 = Xref[:, min(offset, rows - 1)].copy()
    x0[:, 0] += 0.1
    if ulp is not None:
        moved = dict(Q=Q, R=R, xref=Xref, uref=Uref, bound=track, x0=x0)
        moved[ulp[:-1]] = np.nextafter(moved[ulp[:-1]], np.inf if ulp[-1] == "+" else -np.inf)
        Q, R, Xref, Uref, track, x0 = (moved[k] for k in ("Q", "R", "xref", "uref", "bound", "x0"))
    s = make(n, m, N, batch, dtype)
    s.set_model(kind)
    s.set_uniform_step(H)
    if per_knot:
        for k in range(N + 1):
            row = min(offset + k, rows - 1)
            s.set_lqr_cost(k, k + 1, Q if k < N else Qf, R if k < N else R * 0, Xref[:, row], Uref[:, row])
        for k in range(N):
            s.add_constraint(A.CON_CONTROL_BOUND, k, k + 1, track[:, min(offset + k, track.shape[1] - 1)])
    else:
        s.set_lqr_tracking_cost(0, N, Q, R)
        s.set_lqr_tracking_cost(N, N + 1, Qf, R * 0)
        s.set_reference(Xref, Uref)
        s.knot_bound = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 2 * m)
        s.set_constraint_track(s.knot_bound, track)
        if offset:
            s.set_reference_offset(offset)
            s.set_track_offset(offset)
    s.set_initial_state(x0)
    s.set_trajectory(None, np.zeros((N, m)))
    return s


def tracking_cost(Q, R, Qf, Xw, Uw, X, U):
    """The tracking cost of one instance over the window's rows Xw [N+1][n], Uw [N+1][m] in np.longdouble:
    sum_k 0.5 (x_k - xref_k)'Q(x_k - xref_k) + 0.5 (u_k - uref_k)'R(u_k - uref_k), Qf and no control term on knot N."""
    L = np.longdouble
    Q, R, Qf = Q.astype(L), R.astype(L), Qf.astype(L)
    J = L(0)
    N = U.shape[0]
    for k in range(N + 1):
        dx = X[k].astype(L) - Xw[k].astype(L)
        J += L(0.5) * dx @ ((Q if k < N else Qf) @ dx)
        if k < N:
            du = U[k].astype(L) - Uw[k].astype(L)
            J += L(0.5) * du @ (R @ du)
    return J


# ---- problems.moving_obstacles as problems x adjacent starts ---------------------------------------------------------------------
# The ladder of constant initial controls, start g: (v, omega) = LADDER[g].  The tracking cost pulls every start of a problem
# into the same minimum, so the starts differ by the rounding of their iterations alone.  Chosen on the CPU oracle (N = 24,
# offset 0, six problems) among the 4-subsets of v in {-0.5, 0, 0.1, 0.3, 0.6, 0.9} x omega in {-1, -0.5, 0, 0.1, 0.5, 1}
# for the widest margin between winner and runner-up: 4.1e-10 relative at the narrowest problem (the cost bar is 1e-10),
# winners 1, 3, 2, 0, 3, 1 -- every start wins somewhere.
LADDER = np.array([[0.0, 0.5], [0.0, 1.0], [0.1, -1.0], [0.9, -1.0]])


def moving_obstacles_starts(A, P, make, problems=6, starts=4, N=24, rows=None, offset=0, per_knot=False, dtype=0, ladder=LADDER):
    """problems.moving_obstacles for ``problems`` parameter sets, each repeated for ``starts`` adjacent instances (path and
    tracks identical within a problem: built for P and np.repeat-ed); start g begins from the constant controls ladder[g].
    problems.moving_obstacles itself gives every instance its own parameter set, so its calls are stated again here;
    tests/test_knot_shapes_gpu.py::test_multistart_problem_is_moving_obstacles holds the two together."""
    rows = N + 13 if rows is None else rows
    rep = lambda a: np.repeat(a, starts, axis=0)  # noqa: E731
    Xref, Uref, h = P.slalom_path(problems, N, rows)
    circles, bounds = P.moving_obstacle_tracks(problems, N, rows)
    Xref, Uref, circles, bounds = rep(Xref), rep(Uref), rep(circles), rep(bounds)
    hd = float(h)
    Q, R, Qf = np.diag([10.0, 10.0, 1.0]) * hd, np.eye(2) * (0.1 * hd), np.diag([10.0, 10.0, 1.0])
    s = make(3, 2, N, problems * starts, dtype)
    s.set_model(A.MODEL_UNICYCLE)
    s.set_uniform_step(h)
    if per_knot:
        for k in range(N + 1):
            row = min(offset + k, rows - 1)
            s.set_lqr_cost(k, k + 1, Q if k < N else Qf, R if k < N else R * 0, Xref[:, row], Uref[:, row])
        for k in range(N):
            row = min(offset + k, rows - 1)
            if k >= 1:
                s.add_constraint(A.CON_CIRCLE, k, k + 1, circles[:, row])
            s.add_constraint(A.CON_CONTROL_BOUND, k, k + 1, bounds[:, row])
    else:
        s.set_lqr_tracking_cost(0, N, Q, R)
        s.set_lqr_tracking_cost(N, N + 1, Qf, R * 0)
        s.set_reference(Xref, Uref)
        s.knot_circle = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 6)
        s.knot_bound = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 4)
        s.set_constraint_track(s.knot_circle, circles)
        s.set_constraint_track(s.knot_bound, bounds)
        if offset:
            s.set_reference_offset(offset)
            s.set_track_offset(offset)
    s.set_initial_state(Xref[:, min(offset, rows - 1)] + np.array([0.0, 0.1, 0.0]))
    u0 = np.tile(np.asarray(ladder, dtype=np.float64)[:starts], (problems, 1))
    s.set_trajectory(None, np.repeat(u0[:, None, :], N, axis=1))
    return s
