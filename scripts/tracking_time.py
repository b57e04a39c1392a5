#!/usr/bin/env python3
"""What following a reference path costs (include/altro_tracking.h).

kTurn90-sized problems (problems.unicycle_turn90: unicycle, N = 100, control bound and goal constraint, fp64) at batch 8, 1024
and 4096, host clock around work that ends in a device synchronise, medians of runs that alternate in one process:
  (a) tracking   the problem with its stage and terminal costs as TRACKING costs over a constant path (every row the goal):
                 the general kernels' twins, the terms read per knot from the reference-term records;
      general    the same problem with the ordinary costs, put on the general kernels by uniform per-knot steps
                 (set_steps): the same kernels without the records.  (a) - general = the price of the per-knot record;
  (b) fast       the ordinary problem on the default path (staged forward pass, persistent tail kernel).  (a) - fast = what
                 a tracking caller pays for the routing: the figure the LDS-staged follow-up is judged by;
  (c) advance    one mpc_advance(5) on the tracking handle (the window moves on the device, k_ref_terms recomputes the terms)
      reupload   the same window sent again from the host through set_reference.
All three solves compute the same iterations (a constant path gives an ordinary cost group's bits); the script checks that.
Prints one JSON line and writes it to --out.

    python scripts/tracking_time.py [--batches 8,1024,4096] [--reps 10] [--out profiles/tracking_time.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

N, SHIFT = 100, 5


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def timed(f, *a):
    t0 = time.perf_counter()
    f(*a)
    return (time.perf_counter() - t0) * 1e3


def tracking_turn90(A, P, batch, rows):
    """problems.unicycle_turn90 with tracking costs over a constant path of `rows` rows"""
    s = P.make_hip(3, 2, N, batch, A.F64)
    h = np.float32(np.float32(3.0) / np.float32(N))
    hd = float(h)
    xf = np.array([1.5, 1.5, np.pi / 2])
    s.set_model(A.MODEL_UNICYCLE)
    s.set_uniform_step(h)
    s.set_lqr_tracking_cost(0, N, np.eye(3) * (1e-2 * hd), np.eye(2) * (1e-2 * hd))
    s.set_lqr_tracking_cost(N, N + 1, np.eye(3) * 100.0, np.zeros((2, 2)))
    s.set_reference(np.tile(xf, (rows, 1)))
    s.add_control_bound(0, N, [-1.5, -1.5], [1.5, 1.5])
    s.add_constraint(A.CON_GOAL, N, N + 1, xf)
    s.set_initial_state(np.zeros(3))
    s.set_trajectory(None, np.tile(np.array([0.1, 0.1]), (N, 1)))
    return s, h


def measure(A, P, batch, reps):
    rows = N + 1 + SHIFT
    trk, h = tracking_turn90(A, P, batch, rows)
    gen = P.unicycle_turn90(P.make_hip, batch=batch, N=N)
    gen.set_steps(np.full(N, h, dtype=np.float32))
    fast = P.unicycle_turn90(P.make_hip, batch=batch, N=N)
    handles = (("tracking", trk), ("general", gen), ("fast", fast))
    for _ in range(2):  # warm-up: code objects, staging buffers
        for _, s in handles:
            s.reset_trajectory()
            s.solve()
    it = {name: s.get_stats()["iterations_total"].copy() for name, s in handles}
    assert (it["tracking"] == it["general"]).all() and (it["tracking"] == it["fast"]).all()
    t = {name: [] for name, _ in handles}
    for _ in range(reps):
        for name, s in handles:
            s.reset_trajectory()
            t[name].append(timed(s.solve))
    # (c) the window: moved on the device against sent again from the host
    path = np.tile(np.array([1.5, 1.5, np.pi / 2]), (rows, 1))
    window = np.ascontiguousarray(path[SHIFT:SHIFT + N + 1])
    t_adv, t_up = [], []
    for _ in range(2 + reps):
        trk.set_reference(path)  # (offset back to 0, outside the timed sections)
        t_adv.append(timed(trk.mpc_advance, SHIFT))
        t_up.append(timed(trk.set_reference, window))
    out = dict(batch=batch, reps=reps, iterations_max=int(it["tracking"].max()), tracking_solve_ms=summary(t["tracking"]),
               general_solve_ms=summary(t["general"]), fast_solve_ms=summary(t["fast"]),
               record_price_ms=float(np.median(t["tracking"]) - np.median(t["general"])),
               routing_price_ms=float(np.median(t["tracking"]) - np.median(t["fast"])),
               advance_ms=summary(t_adv[2:]), reupload_ms=summary(t_up[2:]))
    for _, s in handles:
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,1024,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    rows = [measure(A, P, int(b), args.reps) for b in args.batches.split(",")]
    probe = P.unicycle_turn90(P.make_hip, batch=1, N=N)
    probe.rollout()
    name, _ = probe.device_info()
    line = json.dumps(dict(metric="tracking_time", problem="kTurn90 fp64, N = 100, constant path", shift=SHIFT, device=name, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
