"""Shared by tests/test_mpc_abi.py and tests/test_mpc_gpu.py: the receding-horizon advance of include/altro_mpc.h stated in
numpy, the host-composed advance (getters -> numpy -> setters, what a caller had to write before the device-side
advance existed), and the problem built to exercise the per-constraint row map."""
import numpy as np

# (k_begin, k_end, rows, equality) of every constraint, in registration order
TURN90_CONS = lambda N: [(0, N, 4, False), (N, N + 1, 3, True)]                            # noqa: E731  problems.unicycle_turn90
THREE_OBSTACLES_CONS = lambda N: [(1, N, 3, False), (0, N, 4, False), (N, N + 1, 3, True)]  # noqa: E731  problems.unicycle_three_obstacles
MIXED_N = 100
MIXED_CONS = [(0, MIXED_N, 4, False), (1, 60, 1, False), (70, MIXED_N + 1, 3, True)]


def mixed_problem(A, P, make, batch=1, dtype=None):
    """The kTurn90 set-up with N = 100 and, in this order: the control bound +-1.5 on [0, N), ONE circle (0.6, 0.2, 0.15) on
    [1, 60), the goal constraint on [70, N] -- an equality, so it sits in front of the inequalities on those knots although
    it was added last."""
    N = MIXED_N
    s = P.unicycle_turn90(make, batch=batch, N=N, dtype=A.F64 if dtype is None else dtype, constraints=False)
    s.add_control_bound(0, N, [-1.5, -1.5], [1.5, 1.5])
    s.add_circle_constraint(1, 60, np.array([[0.6, 0.2, 0.15]]))
    s.add_constraint(A.CON_GOAL, 70, N + 1, np.array([1.5, 1.5, np.pi / 2]))
    return s


def row_labels(N, cons):
    """(knot, constraint, row of the constraint) of every dual / penalty row: by knot, equalities first, then inequalities,
    each in registration order."""
    labels = []
    for k in range(N + 1):
        here = [j for j, (kb, ke, _, _) in enumerate(cons) if kb <= k < ke]
        for j in [j for j in here if cons[j][3]] + [j for j in here if not cons[j][3]]:
            labels += [(k, j, i) for i in range(cons[j][2])]
    return labels


def row_map(N, shift, cons):
    """Section 1 of the contract: a row of constraint j at stage knot k comes from the same row of j at min(k + shift, N - 1)
    if j is attached there, else it starts afresh (-1); the terminal knot's rows stay."""
    labels = row_labels(N, cons)
    index = {lab: r for r, lab in enumerate(labels)}
    return np.array([index[(k, j, i)] if k == N else index.get((min(k + shift, N - 1), j, i), -1) for k, j, i in labels],
                    dtype=np.int32)


def shifted(X, U, lam, rho, src, shift, reset_rho):
    """X, U [B][knots][.], lam, rho [B][rows] after an advance by `shift` (clamped index; rows by the map `src`)."""
    N = U.shape[1]
    Xn = X[:, np.minimum(np.arange(N + 1) + shift, N)]
    Un = U[:, np.minimum(np.arange(N) + shift, N - 1)]
    if lam.shape[1]:
        take = np.maximum(src, 0)
        lam_n = np.where(src >= 0, lam[:, take], 0.0)
        rho_n = np.where(src >= 0, rho[:, take], reset_rho)
    else:
        lam_n, rho_n = lam.copy(), rho.copy()
    return np.ascontiguousarray(Xn), np.ascontiguousarray(Un), lam_n, rho_n


def reset_penalty(solver):
    p = solver.get_options().initial_penalty
    return p if p > 0 else 1.0


def host_advance(solver, shift, src, w=None, set_penalties=True):
    """The advance composed on the host from the getters and setters: five synchronising round trips per cycle."""
    X, U = solver.get_trajectory()
    lam, rho = solver.get_duals(), solver.get_penalties()
    Xn, Un, lam_n, rho_n = shifted(X, U, lam, rho, src, shift, reset_penalty(solver))
    solver.set_initial_state(X[:, shift] + w if w is not None else X[:, shift].copy())
    solver.set_trajectory(Xn, Un)
    if lam.shape[1]:
        solver.set_duals(lam_n)
        if set_penalties:
            solver.set_penalties(rho_n)


def disturbance(cycles, batch, n):
    """w[c][b][i] = 1e-2 sin(1 + 3c + 5b + 7i)"""
    c, b, i = np.meshgrid(np.arange(cycles), np.arange(batch), np.arange(n), indexing="ij")
    return 1e-2 * np.sin(1.0 + 3.0 * c + 5.0 * b + 7.0 * i)
