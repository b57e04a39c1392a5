#!/usr/bin/env python3
"""Median wall time (ms) of eight C calls that stage host arrays -- altro_mpc_track, altro_cov_propagate,
altro_multistart_get_best, altro_mpc_advance, and four that stage ints and bytes: altro_mpc_trigger (lookahead 2),
altro_mpc_ensemble (2 steps, 64 samples), altro_lqr_gains (K, P, fail) and altro_set_solve_mask (set from host bytes, then
cleared) -- on the checkout given by --root (default: this one), so that two builds can be timed in alternating processes.  kTurn90 fp64, batch 64, N = 100, solved once; --reps runs of each call, interleaved, after 20
warm runs; one line "HOSTCALLS {json}".  --once --only CALL makes that one call once (for a kernel / memory-copy trace).

    python scripts/host_staging_time.py [--root ../other-checkout] [--reps 300]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--once", action="store_true", help="one run of each call (for a trace)")
ap.add_argument("--only", default="")
a = ap.parse_args()
root = os.path.abspath(a.root)
sys.path.insert(0, root)
import __graft_entry__ as graft
assert os.path.dirname(os.path.abspath(graft.__file__)) == root
A = graft.load_package()
P = importlib.import_module("altro_cpp_amd.problems")
B, G, STEPS, SHIFT = 64, 4, 5, 2
s = P.batch_turn90(lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d, device_id=0), batch=B)
s.solve()
n, m, N = s.n, s.m, s.N
b, j, k, i = np.meshgrid(np.arange(B), np.arange(1), np.arange(STEPS), np.arange(n), indexing="ij")
w = 1e-2 * np.sin(2.0 + 5.0 * b + 7.0 * i + 11.0 * k)
lo, hi = np.array([-1.5, -1.5]), np.array([1.5, 1.5])
Sigma0 = np.tile(1e-4 * np.eye(n), (B, 1, 1))
Wn = np.tile(1e-6 * np.eye(n), (B, 1, 1))
x0 = s.get_trajectory()[0][:, SHIFT].copy()
wa = 1e-3 * np.sin(np.arange(B * n)).reshape(B, n)
tracked = s.mpc_track(2, 1, w=w[:, :, :2], u_lo=lo, u_hi=hi)["stats"][:, 0].copy()
age = (np.arange(B) % 3).astype(np.int32)
rule = dict(max_age=2, dx_tol=float(np.median(tracked["max_dx"])), viol_tol=1e-4, on_unsolved=1, lookahead=2, ahead_tol=1e-6)
Q, Rw = np.diag([10.0, 10.0, 1.0]), np.diag([0.1, 0.2])
some = (np.arange(B) % 3 != 1).astype(np.uint8)


def mask_on_and_off():
    s.set_solve_mask(some)
    s.set_solve_mask(None)


calls = dict(mpc_track=lambda: s.mpc_track(STEPS, 1, w=w, u_lo=lo, u_hi=hi),
             cov_propagate=lambda: s.cov_propagate(N, Sigma0, Wn),
             multistart_get_best=lambda: s.multistart_get_best(G),
             mpc_advance=lambda: s.mpc_advance(SHIFT, x0=x0, w=wa),
             mpc_trigger=lambda: s.mpc_trigger(rule, tracked=tracked, age=age, u_lo=lo, u_hi=hi),
             mpc_ensemble=lambda: s.mpc_ensemble(2, 64, seed=7, Sigma0=Sigma0[0], W=Wn[0], u_lo=lo, u_hi=hi, viol_tol=1e-4),
             lqr_gains=lambda: s.lqr_gains(Q, Rw),
             set_solve_mask=mask_on_and_off)
if a.only:
    calls = {a.only: calls[a.only]}
out = {}
if a.once:
    for f in calls.values():
        f()
else:
    for _ in range(20):
        for f in calls.values():
            f()
    t = {key: [] for key in calls}
    for _ in range(a.reps):
        for key, f in calls.items():
            t0 = time.perf_counter()
            f()
            t[key].append((time.perf_counter() - t0) * 1e3)
    out = {key: float(np.median(v)) for key, v in t.items()}
s.close()
print("HOSTCALLS " + json.dumps(dict(root=os.path.basename(root) or "new", ms=out)))
