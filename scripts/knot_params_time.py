#!/usr/bin/env python3
"""What per-knot constraint parameters cost (include/altro_knot_params.h).

A problems.moving_obstacles-sized problem (unicycle following the slalom path, N = 100, two circles on [1, N), a control bound
on [0, N), fp64) at batch 8, 1024 and 4096, host clock around work that ends in a device synchronise, medians of runs that
alternate in one process:
  (a) knot       the circles and the bound as KNOT constraints over constant tracks (every row the same): the parameters
                 are read per knot from the knot-parameter records;
      ordinary   the same problem with altro_add_constraint, on the same general kernels (uniform set_steps; the tracking
                 cost routes both handles alike).  (a) - ordinary = the price of the per-knot read;
  (b) advance    one mpc_advance(5) on the knot handle (both windows move on the device; k_knot_params copies the records)
      reupload   the same window of both tracks sent again from the host through set_constraint_track.
Both solves compute the same iterations (a constant track gives an ordinary constraint's bits); the script checks that.
Prints one JSON line and writes it to --out.

    python scripts/knot_params_time.py [--batches 8,1024,4096] [--reps 10] [--out profiles/knot_params_time.json]
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


def constant_parameters(P, batch, rows):
    """circles [B][6] near the path (circle 0 above knot 40, circle 1 beside knot 70) and the shared bound +-0.9"""
    Xref, _, _ = P.slalom_path(batch, N, rows)
    p = (np.arange(batch) % 5).astype(np.float64)
    circles = np.stack([Xref[:, 40, 0] + 0.02 * p, Xref[:, 40, 1] + 0.16, 0.10 + 0.01 * p,
                        Xref[:, 70, 0] + 0.05, Xref[:, 70, 1] - 0.30, np.full(batch, 0.15)], axis=1)
    return circles, np.array([-0.9, -0.9, 0.9, 0.9])


def build(A, P, batch, rows, knot):
    s = P.tracking_slalom(P.make_hip, batch=batch, N=N, rows=rows, bounds=False)
    circles, bound = constant_parameters(P, batch, rows)
    if knot:
        s.knot_circle = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 6)
        s.knot_bound = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 4)
        s.set_constraint_track(s.knot_circle, np.repeat(circles[:, None, :], rows, axis=1))
        s.set_constraint_track(s.knot_bound, np.tile(bound, (batch, rows, 1)))
    else:
        s.add_constraint(A.CON_CIRCLE, 1, N, circles)
        s.add_constraint(A.CON_CONTROL_BOUND, 0, N, bound)
        s.set_steps(np.full(N, np.float32(np.float32(3.0) / np.float32(N)), dtype=np.float32))
    return s


def measure(A, P, batch, reps):
    rows = N + 1 + SHIFT
    knot, ordinary = build(A, P, batch, rows, True), build(A, P, batch, rows, False)
    handles = (("knot", knot), ("ordinary", ordinary))
    for _ in range(2):  # warm-up: code objects, staging buffers
        for _, s in handles:
            s.reset_trajectory()
            s.solve()
    it = {name: s.get_stats()["iterations_total"].copy() for name, s in handles}
    assert (it["knot"] == it["ordinary"]).all()
    t = {name: [] for name, _ in handles}
    for _ in range(reps):
        for name, s in handles:
            s.reset_trajectory()
            t[name].append(timed(s.solve))
    # (b) the window: moved on the device against sent again from the host
    circles, bound = constant_parameters(P, batch, rows)
    ctrack = np.repeat(circles[:, None, :], rows, axis=1)
    btrack = np.tile(bound, (batch, rows, 1))
    cwin, bwin = np.ascontiguousarray(ctrack[:, SHIFT:SHIFT + N]), np.ascontiguousarray(btrack[:, SHIFT:SHIFT + N])

    def reupload():
        knot.set_constraint_track(knot.knot_circle, cwin)
        knot.set_constraint_track(knot.knot_bound, bwin)

    t_adv, t_up = [], []
    for _ in range(2 + reps):
        knot.set_constraint_track(knot.knot_circle, ctrack)  # (the whole tracks and offset 0, outside the timed sections)
        knot.set_constraint_track(knot.knot_bound, btrack)
        knot.set_track_offset(0)
        t_adv.append(timed(knot.mpc_advance, SHIFT))
        knot.set_track_offset(0)
        t_up.append(timed(reupload))
    out = dict(batch=batch, reps=reps, iterations_max=int(it["knot"].max()), knot_solve_ms=summary(t["knot"]),
               ordinary_solve_ms=summary(t["ordinary"]), per_knot_read_price_ms=float(np.median(t["knot"]) - np.median(t["ordinary"])),
               advance_ms=summary(t_adv[2:]), reupload_ms=summary(t_up[2:]))
    for _, s in handles:
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,1024,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knot_params_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    rows = [measure(A, P, int(b), args.reps) for b in args.batches.split(",")]
    probe = P.unicycle_turn90(P.make_hip, batch=1, N=N)
    probe.rollout()
    name, _ = probe.device_info()
    line = json.dumps(dict(metric="knot_params_time", problem="slalom tracking fp64, N = 100, two circles + control bound, constant tracks",
                           shift=SHIFT, device=name, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
