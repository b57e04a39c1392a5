#!/usr/bin/env python3
"""The solve mask (include/altro_subset.h): what a masked solve and a sequential team round cost, against the PARENT's
unmasked solve where a parent build is given (--parent-lib: a libaltro_hip.so built from the commit before the mask).

Alternating legs in one process after a warm-up, host clock around calls that end in a device synchronise; results are checked
to agree before anything is timed.

  teams    problems.team_ring fp64, N = 100, 512 teams x 8 agents (B = 4096).  Every leg starts from the uncoupled plans
           (re-solved, untimed): one sequential sweep (8 masked solves of 512), one damped round (1 solve of 4096), the damped
           exchange's 8 rounds -- each with the clearance it reaches (distance units, worst team and share of teams at or
           above the bar of -2e-3).  With --parent-lib the damped legs also run on the parent build.
  config2  bench.py's config 2 (unicycle kTurn90, N = 100, fp64), B = 4096: reset_trajectory, then a solve under a mask of
           1/8, 1/2 and all instances (every 8th, every other, all ones) and without a mask; with --parent-lib the unmasked
           solve of the parent build beside them.  Shows what k_mask_compact and the lost device-side loop cost.

Prints one JSON line and writes it to --out.

    python scripts/subset_time.py [--reps 10] [--parent-lib PATH] [--out profiles/subset_time.json]
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
import _team_common as TC  # noqa: E402

TEAMS, AGENTS, N, B2 = 512, 8, 100, 4096


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)), reps=len(ms))


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def team_legs(A, P, make, reps, sequential):
    """name -> (times, clearance record) of the team legs on a handle made by `make`"""
    s = P.team_ring(make, TEAMS, AGENTS, N=N)
    idx, rad = s.team_circle, s.team_radius
    U0 = np.tile(np.array([0.1, 0.0]), (N, 1))
    seed = np.zeros((1, 3 * (AGENTS - 1)))

    def uncoupled():
        s.set_constraint_track(idx, seed)
        s.set_trajectory(None, U0)
        s.solve()

    legs = dict(damped_1_round=lambda: s.team_solve(AGENTS, idx, rad, A.TEAM_ALL, 0.5, 1),
                damped_8_rounds=lambda: s.team_solve(AGENTS, idx, rad, A.TEAM_ALL, 0.5, 8))
    if sequential:
        legs["sequential_1_sweep"] = lambda: s.team_solve_sequential(AGENTS, idx, rad, 1)
    times, clear, plans = {k: [] for k in legs}, {}, {}
    for rep in range(reps + 1):  # (rep 0: warm-up of every leg's code objects and buffers)
        for name, leg in legs.items():
            uncoupled()
            t = timed(leg)
            if rep:
                times[name].append(t)
                continue
            X = s.get_trajectory()[0]
            d = TC.distance_clearance(X, AGENTS, rad, 1, N)
            st = s.get_stats()
            clear[name] = dict(worst_team=float(d.min()), teams_at_or_above_bar=float((d >= TC.COUPLED_BAR).mean()),
                               solved_fraction=float((st["status"] == 0).mean()))
            plans[name] = X
    uncoupled()
    d = TC.distance_clearance(s.get_trajectory()[0], AGENTS, rad, 1, N)
    clear["uncoupled"] = dict(worst_team=float(d.min()), teams_at_or_above_bar=float((d >= TC.COUPLED_BAR).mean()))
    name = s.device_info()[0]
    s.close()
    return name, {k: summary(v) for k, v in times.items()}, clear, plans


def config2_legs(P, make, reps, masks):
    """name -> times of reset_trajectory + solve under each mask (None: no mask); the results of the masked-in instances"""
    s = P.batch_turn90(make, B2, N=N)
    times, results = {k: [] for k in masks}, {}
    for rep in range(reps + 1):
        for name, mask in masks.items():
            if name != "parent_unmasked":
                s.set_solve_mask(mask)
            s.reset_trajectory()
            s.get_stats()  # (the copies of the reset are done)
            t = timed(s.solve)
            if rep:
                times[name].append(t)
            else:
                results[name] = (s.get_trajectory(), s.get_stats())
    s.close()
    return {k: summary(v) for k, v in times.items()}, results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="libaltro_hip.so of the parent commit: its unmasked solves beside the new ones")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    reps = max(args.reps, 5)
    parent_make = None
    if args.parent_lib:
        plib = ctypes.CDLL(os.path.abspath(args.parent_lib))
        assert not hasattr(plib, "altro_set_solve_mask"), "--parent-lib must be a build without the solve mask"
        parent_make = lambda n, m, N_, b, d: A.BatchSolver(n, m, N_, b, d, _lib=plib)  # noqa: E731

    device, team, clear, plans = team_legs(A, P, P.make_hip, reps, True)
    out = dict(metric="subset_time", device=device, reps=reps,
               teams=dict(problem="team_ring fp64", N=N, teams=TEAMS, agents=AGENTS, batch=TEAMS * AGENTS, ms=team, clearance=clear))
    if parent_make:
        _, pteam, pclear, pplans = team_legs(A, P, parent_make, reps, False)
        out["teams"]["parent_ms"] = pteam
        out["teams"]["parent_agrees_bit_for_bit"] = {k: bool(plans[k].tobytes() == pplans[k].tobytes()) for k in pplans}
    else:
        out["teams"]["parent_ms"] = "not measured (no --parent-lib)"

    idx = np.arange(B2)
    masks = dict(unmasked=None, masked_all=np.ones(B2, bool), masked_half=idx % 2 == 0, masked_eighth=idx % 8 == 0)
    c2, res = config2_legs(P, P.make_hip, reps, masks)
    (X0, U0), st0 = res["unmasked"]
    agree = {}
    for name, mask in masks.items():
        if mask is None:
            continue
        (X, U), st = res[name]
        agree[name] = bool(X[mask].tobytes() == X0[mask].tobytes() and U[mask].tobytes() == U0[mask].tobytes()
                           and (st["iterations_total"][mask] == st0["iterations_total"][mask]).all())
    out["config2"] = dict(problem="unicycle kTurn90 fp64 (bench.py config 2)", N=N, batch=B2, ms=c2,
                          masked_in_instances_agree_with_unmasked_bit_for_bit=agree)
    if parent_make:
        pc2, pres = config2_legs(P, parent_make, reps, dict(parent_unmasked=None))
        out["config2"]["parent_ms"] = pc2["parent_unmasked"]
        (Xp, Up), _ = pres["parent_unmasked"]
        out["config2"]["parent_agrees_bit_for_bit"] = bool(Xp.tobytes() == X0.tobytes() and Up.tobytes() == U0.tobytes())
    else:
        out["config2"]["parent_ms"] = "not measured (no --parent-lib)"
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
