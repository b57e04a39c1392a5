"""Shared by the team tests (include/altro_team.h): the fill, the blend, the window and the clearance stated in numpy -- every
operation rounded on its own, as the kernels do it -- and the caller's loops over the separate entry points."""
import numpy as np

ALL, PRIORITY = 0, 1
# the bars tests/test_team_oracle.py pins on the CPU oracle and tests/test_team_gpu.py asserts on the device's own plans
UNCOUPLED_BAR, COUPLED_BAR = -0.03, -2e-3
# (teams, agents, mode, blend, rounds) of the behaviour cases
CASES = [(3, 2, ALL, 0.5, 8), (2, 3, ALL, 0.5, 8), (2, 5, ALL, 0.5, 10), (3, 2, PRIORITY, 1.0, 2), (2, 3, PRIORITY, 1.0, 3),
         (2, 5, PRIORITY, 1.0, 5)]


def case_id(case):
    T, A, mode, blend, rounds = case
    return f"T{T}_A{A}_{'priority' if mode == PRIORITY else 'damped'}_{rounds}rounds"


def peer_of(A):
    """[A][A - 1]: circle slot i of agent a is peer i if i < a else i + 1"""
    a, i = np.meshgrid(np.arange(A), np.arange(A - 1), indexing="ij")
    return np.where(i < a, i, i + 1)


def per_instance(radius, B, A):
    radius = np.asarray(radius, dtype=np.float64)
    return radius.copy() if radius.shape == (B,) and A != B else np.tile(radius, B // A)


def fill_rows(X, A, radius, mode=ALL):
    """The track a fill with blend = 1 writes, [B][N + 1][3 (A - 1)], from X [B][N + 1][n]."""
    B, K, _ = X.shape
    T = B // A
    rad = per_instance(radius, B, A).reshape(T, A)
    Xt = X.reshape(T, A, K, -1)
    peer = peer_of(A)
    out = np.zeros((T, A, K, A - 1, 3))
    for a in range(A):
        for i in range(A - 1):
            j = peer[a, i]
            out[:, a, :, i, 0] = Xt[:, j, :, 0]
            out[:, a, :, i, 1] = Xt[:, j, :, 1]
            out[:, a, :, i, 2] = 0.0 if mode == PRIORITY and j > a else (rad[:, a] + rad[:, j])[:, None]
    return out.reshape(B, K, 3 * (A - 1))


def window(track, ahead):
    """What the window shows of a track [B][rows][np] written `ahead` knots ago: rows min(ahead + r, rows - 1)."""
    rows = track.shape[1]
    return track[:, np.minimum(ahead + np.arange(rows), rows - 1)]


def blend_rows(old, new, blend):
    """centre = old + blend * (new - old), three roundings; the radii of `new`."""
    out = new.copy()
    o, w = old.reshape(old.shape[:2] + (-1, 3)), out.reshape(out.shape[:2] + (-1, 3))
    d = w[..., :2] - o[..., :2]
    p = blend * d
    w[..., :2] = o[..., :2] + p
    return out


def clearance(X, A, radius, k_begin, k_end):
    """[T]: min over knots [k_begin, k_end) and pairs a < j of (dx dx + dy dy) - R R, R = radius[a] + radius[j]"""
    B = X.shape[0]
    T = B // A
    rad = per_instance(radius, B, A).reshape(T, A)
    Xt = X.reshape(T, A, X.shape[1], -1)[:, :, k_begin:k_end]
    best = np.full(T, np.inf)
    for a in range(A):
        for j in range(a + 1, A):
            dx = Xt[:, a, :, 0] - Xt[:, j, :, 0]
            dy = Xt[:, a, :, 1] - Xt[:, j, :, 1]
            R = (rad[:, a] + rad[:, j])[:, None]
            xx, yy, RR = dx * dx, dy * dy, R * R
            best = np.minimum(best, ((xx + yy) - RR).min(axis=1))
    return best


def distance_clearance(X, A, radius, k_begin, k_end):
    """[T]: min(|p_a - p_j| - R) in distance units, what the behaviour bars are stated in"""
    B = X.shape[0]
    T = B // A
    rad = per_instance(radius, B, A).reshape(T, A)
    Xt = X.reshape(T, A, X.shape[1], -1)[:, :, k_begin:k_end]
    best = np.full(T, np.inf)
    for a in range(A):
        for j in range(a + 1, A):
            d = np.hypot(Xt[:, a, :, 0] - Xt[:, j, :, 0], Xt[:, a, :, 1] - Xt[:, j, :, 1])
            best = np.minimum(best, (d - (rad[:, a] + rad[:, j])[:, None]).min(axis=1))
    return best


def host_exchange(P, make, teams, agents, mode, blend, rounds, N=24, log=None):
    """The caller's loop on a library without knot constraints (the CPU oracle): an uncoupled solve, then per round a FRESH
    handle from problems.team_ring(per_knot_track = the rows the previous plans give, blended with the previous rows) with
    the previous round's U as the guess.  Returns (X, U, stats) of the last round and, through `log`, the distance clearance
    of every round (entry 0: uncoupled)."""
    s = P.team_ring(make, teams, agents, N=N, per_knot_track=np.zeros((teams * agents, N + 1, 3 * (agents - 1))))
    s.solve()
    X, U = s.get_trajectory()
    stats = s.get_stats()
    rad = s.team_radius
    s.close()
    if log is not None:
        log.append(distance_clearance(X, agents, rad, 1, N))
    track = None
    for _ in range(rounds):
        new = fill_rows(X, agents, rad, mode)
        track = new if track is None or blend == 1.0 else blend_rows(track, new, blend)
        s = P.team_ring(make, teams, agents, N=N, per_knot_track=track, U=U)
        s.solve()
        X, U = s.get_trajectory()
        stats = s.get_stats()
        s.close()
        if log is not None:
            log.append(distance_clearance(X, agents, rad, 1, N))
    return X, U, stats


def team_solve_loop(s, agents, index, radius, mode, blend, rounds):
    """altro_team_solve as the caller writes it"""
    for _ in range(rounds):
        s.team_fill_tracks(agents, index, radius, mode, blend)
        s.solve()


def mpc_team_loop(s, agents, index, radius, mode, blend, rounds, cycles, shift, w):
    """altro_mpc_run_team as the caller writes it; the logs in the shapes the library gives them"""
    B, n, m, T = s.batch, s.n, s.m, s.batch // agents
    L = cycles * shift
    out = dict(X_cl=np.zeros((B, L + 1, n)), U_cl=np.zeros((B, L, m)), iterations=np.zeros((B, cycles), dtype=np.int32),
               status=np.zeros((B, cycles), dtype=np.int32), clear=np.zeros((T, cycles)))
    for c in range(cycles):
        team_solve_loop(s, agents, index, radius, mode, blend, rounds)
        st = s.get_stats()
        out["iterations"][:, c], out["status"][:, c] = st["iterations_total"], st["status"]
        out["clear"][:, c] = s.team_clearance(agents, index, radius)
        X, U = s.get_trajectory()
        out["X_cl"][:, c * shift:(c + 1) * shift] = X[:, :shift]
        out["U_cl"][:, c * shift:(c + 1) * shift] = U[:, :shift]
        s.mpc_advance(shift, w=None if w is None else w[c])
    out["X_cl"][:, L] = s.get_initial_state()
    return out
