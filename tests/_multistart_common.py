"""Shared by the multi-start tests (include/altro_multistart.h): the numpy statement of the selection rule and the start
family of the obstacle batch."""
import numpy as np

SOLVED = 0


def rule_class(status, cost, violation):
    """Class of every start: 0 solved with finite numbers, 1 any other status with finite numbers, 2 a NaN or an infinity."""
    status, cost, violation = np.asarray(status), np.asarray(cost, dtype=np.float64), np.asarray(violation, dtype=np.float64)
    finite = np.isfinite(cost) & np.isfinite(violation)
    return np.where(~finite, 2, np.where(status == SOLVED, 0, 1))


def rule_winner(status, cost, violation):
    """The winner among the starts of ONE problem: the lowest class; inside class 0 the lowest cost, inside class 1 the lowest
    violation, then the lowest cost; every tie to the lowest index (comparisons are fp64 `<`: -0.0 and 0.0 tie)."""
    cost, violation = np.asarray(cost, dtype=np.float64), np.asarray(violation, dtype=np.float64)
    cls = rule_class(status, cost, violation)
    idx = np.nonzero(cls == cls.min())[0]
    if cls.min() == 2:
        return int(idx[0])
    if cls.min() == 1:
        idx = idx[violation[idx] == violation[idx].min()]
    idx = idx[cost[idx] == cost[idx].min()]
    return int(idx[0])


def rule_winners(stats, starts):
    """Winners [P] of a handle's get_stats() (or any record array with status, cost, violation)."""
    P = len(stats) // starts
    return np.array([rule_winner(stats["status"][p * starts:(p + 1) * starts], stats["cost"][p * starts:(p + 1) * starts],
                                 stats["violation"][p * starts:(p + 1) * starts]) for p in range(P)], dtype=np.int32)


def start_guesses(starts, N):
    """The start family: start 0 keeps the factory guess U = 0.01; start g = 1 .. uses the constant guess
    U[:, 0] = 0.6 + 0.1 g, U[:, 1] = (-1)^g * 0.25 * ceil(g / 2).  [starts][N][2]."""
    U = np.full((starts, N, 2), 0.01)
    for g in range(1, starts):
        U[g, :, 0] = 0.6 + 0.1 * g
        U[g, :, 1] = (-1.0) ** g * 0.25 * np.ceil(g / 2.0)
    return U


def obstacle_batch(P_mod, make, problems=8, starts=8, N=40, dtype=None):
    """unicycle_three_obstacles with the circles of the first `problems` rows of batch_obstacle_circles(64), each repeated
    for `starts` starts; start g of problem p is instance p * starts + g."""
    circles = np.repeat(P_mod.batch_obstacle_circles(64)[:problems], starts, axis=0)
    kw = {} if dtype is None else dict(dtype=dtype)
    s = P_mod.unicycle_three_obstacles(make, batch=problems * starts, N=N, circles=circles, **kw)
    s.set_trajectory(None, np.tile(start_guesses(starts, N), (problems, 1, 1)))
    return s
