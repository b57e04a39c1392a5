#!/usr/bin/env python3
"""Wall time of one receding-horizon advance, on the device against composed on the host (include/altro_mpc.h).

kTurn90 fp64 (problems.batch_turn90) in a warm loop -- reset_duals = 0, initial_penalty = 1, shift 5, a disturbance of size
1e-2 on the new initial state -- at batch 1, 64 and 4096.  Per batch size, host clock around work that ends in a device
synchronise:
  (a) device_advance   BatchSolver.mpc_advance: one kernel launch, only the disturbance crosses to the device;
  (b) host_advance     the same advance written with the entry points that existed before it: get_trajectory + get_duals,
                       a numpy shift, set_initial_state + set_trajectory + set_duals (with initial_penalty = 1 every solve
                       sets the penalties itself, so none has to be carried) -- the baseline;
  (c) warm_solve       the solve between two advances.
(a) and (b) alternate in one process after a warm-up; medians with min / max.  Prints one JSON line and writes it to --out.

    python scripts/mpc_cycle_time.py [--batches 1,64,4096] [--reps 20] [--out profiles/mpc_cycle_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SHIFT = 5


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def measure(A, P, batch, reps):
    s = P.batch_turn90(P.make_hip, batch)
    s.set_options(reset_duals=0, initial_penalty=1.0)
    N, n = s.N, s.n
    src = s.mpc_row_map(SHIFT)  # (built once, outside the timed sections)
    take = np.maximum(src, 0)
    kx, ku = np.minimum(np.arange(N + 1) + SHIFT, N), np.minimum(np.arange(N) + SHIFT, N - 1)
    X, U = np.empty((batch, N + 1, n)), np.empty((batch, N, s.m))
    b, i = np.meshgrid(np.arange(batch), np.arange(n), indexing="ij")

    def w(c):
        return 1e-2 * np.sin(1.0 + 3.0 * c + 5.0 * b + 7.0 * i)

    def device_advance(c):
        s.mpc_advance(SHIFT, w=w(c))

    def host_advance(c):
        s.get_trajectory(X, U)
        lam = s.get_duals()
        s.set_initial_state(X[:, SHIFT] + w(c))
        s.set_trajectory(np.ascontiguousarray(X[:, kx]), np.ascontiguousarray(U[:, ku]))
        s.set_duals(np.where(src >= 0, lam[:, take], 0.0))

    def timed(f, *a):
        t0 = time.perf_counter()
        f(*a)
        return (time.perf_counter() - t0) * 1e3

    c = 0
    for _ in range(3):  # warm-up: code objects, the row map on the device, the staging buffers of both paths
        for adv in (device_advance, host_advance):
            s.solve()
            adv(c)
            c += 1
    t_dev, t_host, t_solve, iters = [], [], [], []
    for _ in range(reps):
        for adv, acc in ((device_advance, t_dev), (host_advance, t_host)):
            t_solve.append(timed(s.solve))
            iters.append(int(s.get_stats()["iterations_total"].max()))
            acc.append(timed(adv, c))
            c += 1
    s.close()
    return dict(batch=batch, reps=reps, device_advance_ms=summary(t_dev), host_advance_ms=summary(t_host), warm_solve_ms=summary(t_solve),
                warm_solve_iterations_max=max(iters), device_below_host=bool(np.median(t_dev) < np.median(t_host)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_cycle_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    import importlib
    P = importlib.import_module("altro_cpp_amd.problems")
    rows = [measure(A, P, int(b), max(args.reps, 20)) for b in args.batches.split(",")]
    probe = P.batch_turn90(P.make_hip, 1)
    probe.rollout()
    name, cus = probe.device_info()
    line = json.dumps(dict(metric="mpc_cycle_time", problem="kTurn90 fp64, N = 100", shift=SHIFT, device=name, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
