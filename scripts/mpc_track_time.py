#!/usr/bin/env python3
"""Wall time of closed-loop tracking on the device (include/altro_mpc.h: altro_mpc_track_device) against the open-loop rollout.

kTurn90 fp64 with N = 100 (problems.batch_turn90), solved once.  Two shapes:
  hop       B = 4096, S = 1,    steps = 5     what one cycle of an MPC loop tracks (with logs, as altro_mpc_run_tracked)
  ensemble  B = 64,   S = 1024, steps = 100   a disturbance ensemble over the whole horizon, statistics only and with logs
Every array of the tracking call lives in device memory (allocated through the HIP runtime the solver library has loaded), so
the time is the launch and the kernel, not the copies.  Yardstick, in the same process: altro_rollout on a handle of B x S
instances of the same problem -- k_rollout runs the same chain of discrete steps, one lane per instance, without feedback,
cost, violation or logging, over its whole horizon of 100 knots; both are therefore also given per knot.  Host clock around
calls that end in a device synchronise; the tracking call and the rollout alternate after a warm-up; medians with min / max.
Prints one JSON line and writes it to --out.

    python scripts/mpc_track_time.py [--reps 30] [--out profiles/mpc_track_time.json]
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
import __graft_entry__ as graft  # noqa: E402

SHAPES = (("hop", 4096, 1, 5), ("ensemble", 64, 1024, 100))


def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceBuffer:
    def __init__(self, hip, nbytes, fill=None):
        self.hip = hip
        p = ctypes.c_void_p()
        if hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) != 0:
            raise RuntimeError(f"hipMalloc of {nbytes} bytes failed")
        self.ptr = p.value
        if fill is not None:
            a = np.ascontiguousarray(fill, dtype=np.float64)
            assert a.nbytes == nbytes
            if hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(nbytes), ctypes.c_int(1)) != 0:
                raise RuntimeError("hipMemcpy to the device failed")

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def measure(A, P, name, B, S, steps, reps):
    s = P.batch_turn90(P.make_hip, B)
    s.solve()
    N, n, m, L = s.N, s.n, s.m, B * S
    hip = hip_runtime()
    b, j, k, i = np.meshgrid(np.arange(B), np.arange(S), np.arange(steps), np.arange(n), indexing="ij")
    w = DeviceBuffer(hip, L * steps * n * 8, 1e-2 * np.sin(2.0 + 3.0 * j + 5.0 * b + 7.0 * i + 11.0 * k))
    dx0 = DeviceBuffer(hip, L * n * 8, 1e-2 * np.sin(1.0 + 3.0 * j[:, :, 0] + 5.0 * b[:, :, 0] + 7.0 * i[:, :, 0]))
    X, U = DeviceBuffer(hip, L * (steps + 1) * n * 8), DeviceBuffer(hip, L * steps * m * 8)
    st = DeviceBuffer(hip, L * ctypes.sizeof(A.TrackStats))
    # the yardstick: B x S instances of the same problem (the goals of the first B repeat), open-loop rollout of N knots
    goals = np.repeat(P.batch_turn90_goals(B), S, axis=0)
    y = P.unicycle_turn90(P.make_hip, batch=L, N=N, xf=goals)
    calls = dict(stats_only=lambda: s.mpc_track_device(steps, S, dx0.ptr, w.ptr, 0, 0, 0, 0, st.ptr),
                 with_logs=lambda: s.mpc_track_device(steps, S, dx0.ptr, w.ptr, 0, 0, X.ptr, U.ptr, st.ptr),
                 rollout=y.rollout)
    for _ in range(3):
        for f in calls.values():
            f()
    t = {key: [] for key in calls}
    for _ in range(reps):
        for key, f in calls.items():
            t[key].append(timed(f))
    for buf in (w, dx0, X, U, st):
        buf.free()
    s.close()
    y.close()
    row = dict(shape=name, batch=B, samples=S, steps=steps, lanes=L, reps=reps, rollout_knots=N)
    for key, ms in t.items():
        row[key + "_ms"] = summary(ms)
    per_knot = {key: float(np.median(ms)) / (N if key == "rollout" else steps) * 1e3 for key, ms in t.items()}
    row["us_per_knot"] = per_knot
    row["ratio_per_knot_stats_only_to_rollout"] = per_knot["stats_only"] / per_knot["rollout"]
    row["ratio_per_knot_with_logs_to_rollout"] = per_knot["with_logs"] / per_knot["rollout"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_track_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    rows = [measure(A, P, name, B, S, steps, max(args.reps, 10)) for name, B, S, steps in SHAPES]
    probe = P.batch_turn90(P.make_hip, 1)
    probe.rollout()
    dev, cus = probe.device_info()
    line = json.dumps(dict(metric="mpc_track_time", problem="kTurn90 fp64, N = 100", device=dev, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
