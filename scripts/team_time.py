#!/usr/bin/env python3
"""Teams (include/altro_team.h): what one exchange of plans costs on the device against the same rows composed on the host.

kTurn90-like ring scenario (problems.team_ring) fp64, N = 100, T = 512 teams x A = 8 agents: B = 4096, and a track of
B (N + 1) 3 (A - 1) doubles = 87 MB.  Alternating in one process after a warm-up, host clock around calls that end in a device
synchronise:
  device_fill   BatchSolver.team_fill_tracks: the radii (32 KB) go over, k_team_tracks and k_knot_params run;
  host_fill     the same rows composed from what existed before: get_trajectory (the whole batch down), the gather in numpy
                (tests/_team_common.fill_rows), set_constraint_track (the 87 MB up, then k_knot_params);
  solve         the AL solve between them (both fills leave the same track, so the solves are the same work).
The two fills are checked to leave the same parameters, bit for bit, before anything is timed.

Prints one JSON line and writes it to --out.

    python scripts/team_time.py [--reps 10] [--out profiles/team_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import _team_common as TC  # noqa: E402  (the numpy statement of the fill)

TEAMS, AGENTS, N = 512, 8, 100


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "team_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    B = TEAMS * AGENTS
    s = P.team_ring(P.make_hip, TEAMS, AGENTS, N=N)
    idx, rad = s.team_circle, s.team_radius
    s.solve()  # the uncoupled plans (fails here, loudly, without a device: nothing below falls back)
    name, _ = s.device_info()
    X, U = np.empty((B, N + 1, s.n)), np.empty((B, N, s.m))

    def device_fill():
        s.team_fill_tracks(AGENTS, idx, rad)

    def host_fill():
        s.get_trajectory(X, U)
        s.set_constraint_track(idx, TC.fill_rows(X, AGENTS, rad))

    device_fill()
    a = s.get_knot_params(idx)
    host_fill()
    same = a.tobytes() == s.get_knot_params(idx).tobytes()
    for _ in range(2):  # warm-up: code objects, staging buffers and pages of both paths
        for fill in (device_fill, host_fill):
            fill()
            s.solve()
    t_dev, t_host, t_solve = [], [], []
    for _ in range(max(args.reps, 5)):
        for fill, acc in ((device_fill, t_dev), (host_fill, t_host)):
            acc.append(timed(fill))
            t_solve.append(timed(s.solve))
    st = s.get_stats()
    s.close()
    track_bytes = 8 * B * (N + 1) * 3 * (AGENTS - 1)
    counted = dict(device=dict(kernel_launches=2, host_to_device_bytes=8 * B, device_to_host_bytes=0),
                   host=dict(kernel_launches=3, note="the layout kernels of get_trajectory (X and U), then k_knot_params",
                             host_to_device_bytes=track_bytes, device_to_host_bytes=8 * B * ((N + 1) * s.n + N * s.m)))
    out = dict(metric="team_time", device=name, problem="team_ring fp64", N=N, teams=TEAMS, agents=AGENTS, batch=B,
               track_bytes=track_bytes, reps=len(t_dev), fills_agree_bit_for_bit=bool(same), device_fill_ms=summary(t_dev),
               host_fill_ms=summary(t_host), solve_between_ms=summary(t_solve),
               host_over_device=float(np.median(t_host) / np.median(t_dev)),
               solved_fraction_last_solve=float((st["status"] == 0).mean()), counted=counted)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
