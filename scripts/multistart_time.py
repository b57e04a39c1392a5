#!/usr/bin/env python3
"""Multi-start (include/altro_multistart.h): what the tail of a cycle costs on the device, and what the starts buy.

(a) Cycle tail, a time.  kTurn90 fp64, N = 100, P = 512 problems x G = 8 starts (one goal per problem, start g from the
    constant controls (0.1 + 0.05 g, 0.1 - 0.04 g)).  Alternating in one process after a warm-up, host clock around calls that
    end in a device synchronise:
      device_tail   BatchSolver.multistart_spread + multistart_perturb: three kernel launches, the winners (2 KB) come back
                    and the perturbation ([G][N][m]) goes over;
      host_tail     the same effect composed from the getters and setters that existed before: get_stats, the rule in numpy,
                    get_trajectory + get_duals + get_penalties, the winners' rows expanded in numpy, U + dU, set_trajectory +
                    set_duals + set_penalties.  GAINS CANNOT BE SET from the host (there is no setter), so this path leaves
                    every start with its own gains, and the stored constraint values and knot costs stay too: it does less.
    A solve runs between the tails (untimed) so that every tail meets fresh, distinct columns.
(b) Solved fraction, not a time.  The config-3 obstacle batch (problems.batch_obstacle_circles) at N = 100, P = 512 problems,
    G = 8 starts of the family of tests/_multistart_common.py: the fraction of problems whose start 0 is ALTRO_SOLVED against
    the fraction whose WINNER is, from the GPU and from the CPU oracle (schedules are exact, so the two must agree).

Prints one JSON line and writes it to --out.

    python scripts/multistart_time.py [--reps 20] [--out profiles/multistart_time.json] [--skip-oracle]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import _multistart_common as MS  # noqa: E402  (the numpy statement of the rule and the start family)

PROBLEMS, STARTS, N = 512, 8, 100


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def cycle_tail(A, P, reps):
    B = PROBLEMS * STARTS
    xf = np.repeat(P.batch_turn90_goals(PROBLEMS), STARTS, axis=0)
    g = np.tile(np.arange(STARTS, dtype=np.float64), PROBLEMS)
    u0 = np.stack([0.1 + 0.05 * g, 0.1 - 0.04 * g], axis=1)
    s = P.unicycle_turn90(P.make_hip, batch=B, N=N, xf=xf, u0=u0)
    gs = np.arange(STARTS, dtype=np.float64)
    dU = np.broadcast_to(np.stack([0.02 * gs, -0.03 * gs], axis=1)[:, None, :], (STARTS, N, s.m)).copy()
    dB = np.tile(dU, (PROBLEMS, 1, 1))
    X, U = np.empty((B, N + 1, s.n)), np.empty((B, N, s.m))

    def device_tail():
        s.multistart_spread(STARTS)
        s.multistart_perturb(STARTS, dU)

    def host_tail():
        win = MS.rule_winners(s.get_stats(), STARTS)
        src = np.repeat(np.arange(PROBLEMS) * STARTS + win, STARTS)
        s.get_trajectory(X, U)
        lam, rho = s.get_duals(), s.get_penalties()
        s.set_trajectory(np.ascontiguousarray(X[src]), U[src] + dB)
        s.set_duals(np.ascontiguousarray(lam[src]))
        s.set_penalties(np.ascontiguousarray(rho[src]))

    def timed(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):  # warm-up: code objects, staging buffers of both paths
        for tail in (device_tail, host_tail):
            s.solve()
            tail()
    t_dev, t_host, t_solve = [], [], []
    for _ in range(reps):
        for tail, acc in ((device_tail, t_dev), (host_tail, t_host)):
            t_solve.append(timed(s.solve))
            acc.append(timed(tail))
    rows = s.num_constraints()
    s.close()
    # what can be counted from the code, per cycle tail
    counted = dict(
        device=dict(kernel_launches=3, host_to_device_bytes=int(dU.nbytes), device_to_host_bytes=4 * PROBLEMS),
        host=dict(kernel_launches_at_least=4, note="the layout kernels of get_trajectory and set_trajectory (X and U each way); duals "
                  "and penalties are transposed on the host", host_to_device_bytes=int(8 * B * ((N + 1) * s.n + N * s.m + 2 * rows)),
                  device_to_host_bytes=int(8 * B * ((N + 1) * s.n + N * s.m) + 2 * 8 * rows * B + 22 * 8 * B)))
    return dict(problem="kTurn90 fp64", N=N, problems=PROBLEMS, starts=STARTS, reps=reps, device_tail_ms=summary(t_dev),
                host_tail_ms=summary(t_host), solve_between_ms=summary(t_solve),
                host_tail_note="the host path cannot set gains, stored constraint values or knot costs: it does less than the spread",
                device_below_host=bool(np.median(t_dev) < np.median(t_host)), counted=counted)


def solved_fraction(A, P, make, label):
    circles = np.repeat(P.batch_obstacle_circles(PROBLEMS), STARTS, axis=0)
    s = P.unicycle_three_obstacles(make, batch=PROBLEMS * STARTS, N=N, circles=circles)
    s.set_trajectory(None, np.tile(MS.start_guesses(STARTS, N), (PROBLEMS, 1, 1)))
    t0 = time.perf_counter()
    s.solve()
    secs = time.perf_counter() - t0
    st = s.get_stats().copy()
    win = s.multistart_select(STARTS) if label == "gpu" else MS.rule_winners(st, STARTS)
    s.close()
    assert np.array_equal(win, MS.rule_winners(st, STARTS))
    solved = (st["status"] == MS.SOLVED).reshape(PROBLEMS, STARTS)
    return dict(source=label, start0_solved=float(solved[:, 0].mean()), winner_solved=float(solved[np.arange(PROBLEMS), win].mean()),
                any_start_solved=float(solved.any(axis=1).mean()), per_start_solved=[float(v) for v in solved.mean(axis=0)],
                winner_histogram=[int(v) for v in np.bincount(win, minlength=STARTS)], solve_seconds=secs), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistart_time.json"))
    ap.add_argument("--skip-oracle", action="store_true")
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    probe = P.batch_turn90(P.make_hip, 1)
    probe.rollout()  # (fails here, loudly, without a device: nothing below falls back)
    name, cus = probe.device_info()
    probe.close()
    tail = cycle_tail(A, P, max(args.reps, 10))
    frac = [solved_fraction(A, P, P.make_hip, "gpu")]
    if not args.skip_oracle:
        olib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "liboracle.so"))
        frac.append(solved_fraction(A, P, lambda n, m, N_, b, d: A.BatchSolver(n, m, N_, b, d, _lib=olib, _prefix="oracle_"), "oracle"))
    out = dict(metric="multistart_time", device=name, cycle_tail=tail,
               solved_fraction=dict(problem="unicycle_three_obstacles fp64, batch_obstacle_circles", N=N, problems=PROBLEMS, starts=STARTS,
                                    rows=[f for f, _ in frac]))
    if len(frac) == 2:
        out["solved_fraction"]["statuses_agree"] = bool(np.array_equal(frac[0][1]["status"], frac[1][1]["status"]))
        out["solved_fraction"]["iterations_agree"] = bool(np.array_equal(frac[0][1]["iterations_total"], frac[1][1]["iterations_total"]))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
